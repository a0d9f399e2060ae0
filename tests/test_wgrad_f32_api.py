"""CPU-side contract of the exact fp32 weight gradient: hgnn_wgrad_f32's symbols and signatures, its workspace query
against the restated shape function, every refusal (decided before any HIP call, so visible without a device), the
``fused.set_wgrad_f32`` switch and the library branch of ``fused._atb`` that it leaves alone.

The entries are additions: the header keeps HGNN_ABI_VERSION where it is (additions only, as for every entry added
since), and header, binding and library agree on it."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import conftest
import wgrad_f32_ref as F
from hierarchicalgnn_amd import _lib, fused

HEADER = os.path.join(conftest.ROOT, "include", "hgnn_hip.h")
SYMBOLS = ("hgnn_wgrad_f32_workspace_bytes", "hgnn_wgrad_f32")
P = 0x10000          # a 16-byte aligned address that must never be touched


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_symbols_are_declared_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    code = _code()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.declared_symbols(), f"{name} is not bound"
        assert re.search(r"\bint %s\s*\(" % name, code), f"{name} is not declared in include/hgnn_hip.h"
    v = int(re.search(r"#define\s+HGNN_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert v == _lib.ABI_VERSION == _lib.load().hgnn_abi_version()


def test_declared_signatures():
    code = re.sub(r"\s+", " ", _code())
    assert "int hgnn_wgrad_f32_workspace_bytes(int64_t M, int32_t Ho, int32_t Hi, size_t* bytes);" in code
    assert ("int hgnn_wgrad_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t M, int32_t Ho, "
            "int32_t Hi, float* out, int64_t ldo, void* workspace, size_t workspace_bytes, hgnn_stream_t stream);") in code
    c = ctypes
    _lib.load()
    res, args = _lib._SIGNATURES["hgnn_wgrad_f32_workspace_bytes"]
    assert res is c.c_int and args == [c.c_int64, c.c_int32, c.c_int32, c.POINTER(c.c_size_t)]
    res, args = _lib._SIGNATURES["hgnn_wgrad_f32"]
    assert res is c.c_int and args == [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int64, c.c_int32, c.c_int32,
                                       c.c_void_p, c.c_int64, c.c_void_p, c.c_size_t, c.c_void_p]


def _ws(M, Ho, Hi):
    n = ctypes.c_size_t(0)
    rc = _lib.load().hgnn_wgrad_f32_workspace_bytes(M, Ho, Hi, ctypes.byref(n))
    return rc, n.value


def test_workspace_query_is_the_restated_shape_function():
    widths = (8, 24, 128, 136, 256, 264, 512, 520, 1024)
    ms = (0, 1, 15, 16, 17, 127, 128, 129, 130, 255, 256, 257, 1000, 4096, 5000, 65537, 70001, 120_000, 2_000_000,
          (1 << 31) + 5)
    for Ho in widths:
        for Hi in widths:
            for M in ms:
                rc, n = _ws(M, Ho, Hi)
                assert rc == 0 and n == F.workspace_bytes(M, Ho, Hi), (M, Ho, Hi, n, F.shape_for(M, Ho, Hi))
    for Ho, Hi in F.SHAPES:
        for M in F.m_edges(Ho, Hi):
            assert _ws(M, Ho, Hi) == (0, F.workspace_bytes(M, Ho, Hi))


def _refused(what, *args):
    lib = _lib.load()
    rc = lib.hgnn_wgrad_f32(*args)
    msg = lib.hgnn_last_error().decode()
    assert rc == 1, (what, rc)                               # HGNN_ERR_INVALID_ARG
    assert msg.startswith("hgnn_wgrad_f32: "), (what, msg)
    return msg


def test_every_refusal_gives_its_status_and_message_and_touches_no_pointer():
    """the operand / out / workspace addresses are unmapped: a refusal that read or wrote one would fault"""
    big = 1 << 40
    ok = dict(A=P, lda=128, B=P, ldb=64, M=1000, Ho=128, Hi=64, out=P, ldo=64, ws=P, nbytes=big)

    def call(what, **kw):
        a = dict(ok, **kw)
        return _refused(what, a["A"], a["lda"], a["B"], a["ldb"], a["M"], a["Ho"], a["Hi"], a["out"], a["ldo"], a["ws"],
                        a["nbytes"], None)

    for Ho, Hi in ((12, 64), (128, 20), (0, 64), (128, -8)):
        assert "multiples of 8" in call("width", Ho=Ho, Hi=Hi, lda=1040, ldb=1040, ldo=1040)
    for Ho, Hi in ((1032, 64), (128, 1032), (2048, 2048)):
        assert "at most 1024" in call("wide", Ho=Ho, Hi=Hi, lda=2048, ldb=2048, ldo=2048)
    assert "got 1032, 64" in call("wide", Ho=1032, lda=2048)
    assert "ldo < Hi" in call("ldo", ldo=56)
    assert "ldo < Hi" in call("out", out=None)
    for kw in (dict(lda=130), dict(ldb=66), dict(lda=120), dict(ldb=60)):
        assert "multiples of 4 floats and cover the columns" in call("stride", **kw)
    for kw in (dict(A=P + 4), dict(B=P + 8), dict(A=None), dict(B=None)):
        assert "not 16-byte aligned" in call("operand", **kw)
    need = F.workspace_bytes(1000, 128, 64)
    assert "workspace too small" in call("no workspace", ws=None)
    assert f"({need - 1} < {need})" in call("small workspace", nbytes=need - 1)
    assert "unaligned" in call("unaligned workspace", ws=P + 4)
    assert "workspace too small" in call("M = 0 still wants its workspace", M=0, ws=None)
    assert _ws(10, 12, 64)[0] == 1 and _ws(10, 64, 1032)[0] == 1 and _ws(-1, 64, 64)[0] == 1
    assert _lib.load().hgnn_wgrad_f32_workspace_bytes(10, 64, 64, None) == 1


def test_operator_refuses_cpu_tensors_loudly():
    from hierarchicalgnn_amd.ops import wgrad_f32
    with pytest.raises(RuntimeError, match="HIP device"):
        wgrad_f32(torch.zeros(4, 8), torch.zeros(4, 8))


def test_switch_defaults_to_off_and_sets():
    assert "HGNN_WGRAD_F32" in os.environ or fused._wgrad_f32_on is False
    old = fused._wgrad_f32_on
    try:
        fused.set_wgrad_f32(True)
        assert fused._wgrad_f32_on is True
        fused.set_wgrad_f32(0)
        assert fused._wgrad_f32_on is False
    finally:
        fused.set_wgrad_f32(old)
    # the initial contents of ``stats`` stay as they are: both counters are created on first use
    assert "bwd_layer_f32_calls" in fused.stats


@pytest.mark.parametrize("value,expect", [(None, False), ("1", True), ("0", False)])
def test_switch_follows_the_environment_in_a_fresh_process(value, expect):
    env = {k: v for k, v in os.environ.items() if k != "HGNN_WGRAD_F32"}
    if value is not None:
        env["HGNN_WGRAD_F32"] = value
    env["PYTHONPATH"] = conftest.ROOT + os.pathsep + env.get("PYTHONPATH", "")
    code = ("from hierarchicalgnn_amd import fused; "
            "print(fused._wgrad_f32_on, 'wgrad_f32_calls' in fused.stats, 'library_wgrad_calls' in fused.stats)")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(expect), "False", "False"]


@pytest.mark.parametrize("n", [1, 300, 5000])
def test_atb_on_cpu_tensors_is_the_library_bit_for_bit(n):
    """switch off: ``_atb`` is today's code (A^T B; the row-block form from 4096 rows on) and counts nothing for the
    new kernel; switch on: CPU tensors still take the library"""
    g = torch.Generator().manual_seed(n)
    A, B = torch.randn(n, 24, generator=g), torch.randn(n, 40, generator=g)
    chunks = max(16, min(256, n // 8192))
    c = n // chunks
    if c < 256:
        want = A.t() @ B
    else:
        want = torch.bmm(A[:c * chunks].reshape(chunks, c, 24).transpose(1, 2),
                         B[:c * chunks].reshape(chunks, c, 40)).sum(dim=0)
        if c * chunks < n:
            want += A[c * chunks:].t() @ B[c * chunks:]
    old = fused._wgrad_f32_on
    try:
        for flag in (False, True):
            fused.set_wgrad_f32(flag)
            n0, l0 = fused.stats.get("wgrad_f32_calls", 0), fused.stats.get("library_wgrad_calls", 0)
            got = fused._atb(A, B)
            assert torch.equal(got, want)
            assert fused.stats.get("wgrad_f32_calls", 0) == n0 == fused.stats.get("wgrad_f32_calls", n0)
            assert fused.stats["library_wgrad_calls"] == l0 + 1
    finally:
        fused.set_wgrad_f32(old)
