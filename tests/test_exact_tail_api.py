"""CPU-side contract of the exact route's last kernels: the symbols and signatures of hgnn_project_f32 and the narrow
products, the narrow weight gradient's workspace query against the restated shape function, every refusal (decided
before any HIP call, so visible without a device), the ``fused.set_project_f32`` / ``fused.set_narrow_f32`` switches and
the library branches they leave alone.

The entries are additions: the header keeps HGNN_ABI_VERSION where it is."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import conftest
import exact_tail_ref as T
from hierarchicalgnn_amd import _lib, fused

HEADER = os.path.join(conftest.ROOT, "include", "hgnn_hip.h")
SYMBOLS = ("hgnn_project_f32", "hgnn_linear_narrow_f32", "hgnn_outer_narrow_f32", "hgnn_wgrad_narrow_f32_workspace_bytes",
           "hgnn_wgrad_narrow_f32")
COUNTERS = ("project_f32_calls", "narrow_linear_calls", "narrow_outer_calls", "narrow_wgrad_calls",
            "library_project_calls", "library_head_calls")
P = 0x10000          # a 16-byte aligned address that must never be touched
INVALID, UNSUPPORTED = 1, 4


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
    assert v == 26 == _lib.ABI_VERSION == _lib.load().hgnn_abi_version()


def test_declared_signatures():
    code = re.sub(r"\s+", " ", _code())
    assert ("int hgnn_project_f32(const float* x, int64_t ldx, int64_t M, int32_t K, const float* w0, const float* w1, "
            "int64_t ldw, int32_t N, float* out0, float* out1, int64_t ldo, hgnn_stream_t stream);") in code
    assert ("int hgnn_linear_narrow_f32(const float* x, int64_t ldx, int64_t M, int32_t K, const float* W, int64_t ldw, "
            "const float* bias, int32_t n, float* out, int64_t ldo, hgnn_stream_t stream);") in code
    assert ("int hgnn_outer_narrow_f32(const float* y, int64_t ldy, int64_t M, int32_t n, const float* W, int64_t ldw, "
            "int32_t K, const float* add, float* out, int64_t ldo, hgnn_stream_t stream);") in code
    assert "int hgnn_wgrad_narrow_f32_workspace_bytes(int64_t M, int32_t n, int32_t K, size_t* bytes);" in code
    assert ("int hgnn_wgrad_narrow_f32(const float* y, int64_t ldy, int32_t n, const float* x, int64_t ldx, int32_t K, "
            "int64_t M, float* out, int64_t ldo, float* colsum, void* workspace, size_t workspace_bytes, "
            "hgnn_stream_t stream);") in code
    c = ctypes
    v, i64, i32 = c.c_void_p, c.c_int64, c.c_int32
    _lib.load()
    want = {"hgnn_project_f32": [v, i64, i64, i32, v, v, i64, i32, v, v, i64, v],
            "hgnn_linear_narrow_f32": [v, i64, i64, i32, v, i64, v, i32, v, i64, v],
            "hgnn_outer_narrow_f32": [v, i64, i64, i32, v, i64, i32, v, v, i64, v],
            "hgnn_wgrad_narrow_f32_workspace_bytes": [i64, i32, i32, c.POINTER(c.c_size_t)],
            "hgnn_wgrad_narrow_f32": [v, i64, i32, v, i64, i32, i64, v, i64, v, v, c.c_size_t, v]}
    for name, args in want.items():
        res, got = _lib._SIGNATURES[name]
        assert res is c.c_int and got == args, name


def _ws(M, n, K):
    b = ctypes.c_size_t(0)
    rc = _lib.load().hgnn_wgrad_narrow_f32_workspace_bytes(M, n, K, ctypes.byref(b))
    return rc, b.value


def test_workspace_query_is_the_restated_shape_function():
    ms = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1000, 4096, 5000, 65537, 70001, 120_000, 2_000_000, (1 << 31) - 1)
    for n in (1, 2, 3, 6, 8, 9, 16, 17, 31, 32):
        for K in (4, 8, 16, 60, 64, 128, 256, 260, 512, 1024):
            for M in ms:
                assert _ws(M, n, K) == (0, T.wgrad_workspace_bytes(M, n, K)), (M, n, K, T.wgrad_shape(M, n, K))
    for n in T.NARROW_N:
        for K in T.NARROW_K:
            for M in T.narrow_m(n, K):
                assert _ws(M, n, K) == (0, T.wgrad_workspace_bytes(M, n, K))


def _refused(name, status, what, *args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = lib.hgnn_last_error().decode()
    assert rc == status, (name, what, rc, msg)
    assert msg.startswith(name + ": "), (what, msg)
    return msg


def test_projection_refusals_touch_no_pointer():
    """the operand and output addresses are unmapped: a refusal that read or wrote one would fault"""
    ok = dict(x=P, ldx=128, M=1000, K=128, w0=P, w1=P, ldw=384, N=256, out0=P, out1=P, ldo=256)

    def call(status, what, **kw):
        a = dict(ok, **kw)
        return _refused("hgnn_project_f32", status, what, a["x"], a["ldx"], a["M"], a["K"], a["w0"], a["w1"], a["ldw"],
                        a["N"], a["out0"], a["out1"], a["ldo"], None)

    for K, N in ((0, 256), (8, 256), (24, 256), (528, 256), (-16, 256), (128, 0), (128, 8), (128, 40), (128, 1040)):
        assert f"unsupported shape K={K} N={N}" in call(UNSUPPORTED, "shape", K=K, N=N, ldx=2048, ldw=2048, ldo=2048)
    assert "bad M" in call(INVALID, "M", M=-1) and "bad M" in call(INVALID, "M", M=1 << 31)
    for kw in (dict(w1=None), dict(out1=None)):
        assert "together or not at all" in call(INVALID, "blocks", **kw)
    for kw in (dict(ldx=120), dict(ldx=130), dict(ldw=124), dict(ldw=386), dict(ldo=248), dict(ldo=258)):
        assert "multiples of 4 floats and cover the columns" in call(INVALID, "stride", **kw)
    for kw in (dict(x=None), dict(w0=None), dict(out0=None)):
        assert "NULL pointer" in call(INVALID, "null", **kw)
    for kw in (dict(x=P + 4), dict(w0=P + 8), dict(w1=P + 4), dict(out0=P + 12), dict(out1=P + 4)):
        assert "16-byte aligned" in call(INVALID, "alignment", **kw)


def test_narrow_refusals_touch_no_pointer():
    lin = dict(x=P, ldx=256, M=1000, K=256, W=P + 4, ldw=256, bias=P + 4, n=3, out=P + 4, ldo=3)
    out = dict(y=P + 4, ldy=3, M=1000, n=3, W=P + 4, ldw=256, K=256, add=P, out=P, ldo=256)
    wg = dict(y=P + 4, ldy=3, n=3, x=P, ldx=256, K=256, M=1000, out=P + 4, ldo=256, colsum=P + 4, ws=P + 4, nbytes=1 << 40)

    def linear(status, what, **kw):
        a = dict(lin, **kw)
        return _refused("hgnn_linear_narrow_f32", status, what, a["x"], a["ldx"], a["M"], a["K"], a["W"], a["ldw"],
                        a["bias"], a["n"], a["out"], a["ldo"], None)

    def outer(status, what, **kw):
        a = dict(out, **kw)
        return _refused("hgnn_outer_narrow_f32", status, what, a["y"], a["ldy"], a["M"], a["n"], a["W"], a["ldw"],
                        a["K"], a["add"], a["out"], a["ldo"], None)

    def wgrad(status, what, **kw):
        a = dict(wg, **kw)
        return _refused("hgnn_wgrad_narrow_f32", status, what, a["y"], a["ldy"], a["n"], a["x"], a["ldx"], a["K"],
                        a["M"], a["out"], a["ldo"], a["colsum"], a["ws"], a["nbytes"], None)

    for call in (linear, outer, wgrad):
        for n, K in ((0, 256), (33, 256), (-1, 256), (3, 0), (3, 2), (3, 6), (3, 1028), (3, -4)):
            big = dict(ldx=2048, ldw=2048) if call is linear else dict(ldo=2048, ldw=2048) if call is outer \
                else dict(ldx=2048, ldo=2048)
            assert f"unsupported widths n={n} K={K}" in call(UNSUPPORTED, "widths", n=n, K=K, **big)
        assert "bad M" in call(INVALID, "M", M=-1)
    for kw in (dict(ldx=252), dict(ldx=258)):
        assert "ldx must be a multiple of 4 floats that covers K" in linear(INVALID, "ldx", **kw)
        assert "ldx must be a multiple of 4 floats that covers K" in wgrad(INVALID, "ldx", **kw)
    for kw in (dict(ldo=252), dict(ldo=258)):
        assert "ldo must be a multiple of 4 floats that covers K" in outer(INVALID, "ldo", **kw)
    for kw in (dict(ldw=255), dict(ldo=2)):
        assert "do not cover the columns" in linear(INVALID, "narrow stride", **kw)
    for kw in (dict(ldy=2), dict(ldw=255)):
        assert "do not cover the columns" in outer(INVALID, "narrow stride", **kw)
    for kw in (dict(ldy=2), dict(ldo=255)):
        assert "do not cover the columns" in wgrad(INVALID, "narrow stride", **kw)
    for kw in (dict(x=None), dict(W=None), dict(out=None)):
        assert "NULL pointer" in linear(INVALID, "null", **kw)
    for kw in (dict(y=None), dict(W=None), dict(out=None)):
        assert "NULL pointer" in outer(INVALID, "null", **kw)
    for kw in (dict(y=None), dict(x=None), dict(out=None)):
        assert "NULL pointer" in wgrad(INVALID, "null", **kw)
    assert "x must be 16-byte aligned" in linear(INVALID, "x", x=P + 4)
    assert "x must be 16-byte aligned" in wgrad(INVALID, "x", x=P + 8)
    for kw in (dict(out=P + 4), dict(add=P + 8)):
        assert "out and add must be 16-byte aligned" in outer(INVALID, "wide", **kw)
    for kw in (dict(W=P + 2), dict(bias=P + 1), dict(out=P + 3)):
        assert "4-byte aligned" in linear(INVALID, "narrow", **kw)
    for kw in (dict(y=P + 2), dict(W=P + 1)):
        assert "4-byte aligned" in outer(INVALID, "narrow", **kw)
    for kw in (dict(y=P + 2), dict(out=P + 1), dict(colsum=P + 3)):
        assert "4-byte aligned" in wgrad(INVALID, "narrow", **kw)
    need = T.wgrad_workspace_bytes(1000, 3, 256)
    assert "workspace too small" in wgrad(INVALID, "no workspace", ws=None)
    assert f"({need - 1} < {need})" in wgrad(INVALID, "small workspace", nbytes=need - 1)
    assert "unaligned" in wgrad(INVALID, "unaligned workspace", ws=P + 2)
    assert "workspace too small" in wgrad(INVALID, "M = 0 still wants its workspace", M=0, ws=None)
    assert _ws(10, 0, 64)[0] == UNSUPPORTED and _ws(10, 3, 6)[0] == UNSUPPORTED and _ws(-1, 3, 64)[0] == INVALID
    assert _lib.load().hgnn_wgrad_narrow_f32_workspace_bytes(10, 3, 64, None) == INVALID
    assert _lib.load().hgnn_last_error().decode().startswith("hgnn_wgrad_narrow_f32_workspace_bytes: ")


def test_operators_refuse_cpu_tensors_loudly():
    from hierarchicalgnn_amd import ops
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.project_f32(torch.zeros(4, 16), torch.zeros(16, 16))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.linear_narrow_f32(torch.zeros(4, 16), torch.zeros(3, 16))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.outer_narrow_f32(torch.zeros(4, 3), torch.zeros(3, 16))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.wgrad_narrow_f32(torch.zeros(4, 3), torch.zeros(4, 16))


@pytest.mark.parametrize("name", ["project_f32", "narrow_f32"])
def test_switch_defaults_to_off_and_sets(name):
    var, setter = f"_{name}_on", getattr(fused, "set_" + name)
    assert "HGNN_" + name.upper() in os.environ or getattr(fused, var) is False
    old = getattr(fused, var)
    try:
        setter(True)
        assert getattr(fused, var) is True
        setter(0)
        assert getattr(fused, var) is False
    finally:
        setter(old)


@pytest.mark.parametrize("value,expect", [(None, False), ("1", True), ("0", False)])
def test_switches_follow_the_environment_in_a_fresh_process(value, expect):
    """each switch follows its own variable alone; the new counters are absent from a fresh ``stats``"""
    for mine, other in (("HGNN_PROJECT_F32", "HGNN_NARROW_F32"), ("HGNN_NARROW_F32", "HGNN_PROJECT_F32")):
        env = {k: v for k, v in os.environ.items() if k not in (mine, other)}
        if value is not None:
            env[mine] = value
        env["PYTHONPATH"] = conftest.ROOT + os.pathsep + env.get("PYTHONPATH", "")
        code = ("from hierarchicalgnn_amd import fused; "
                f"print(fused._{mine[5:].lower()}_on, fused._{other[5:].lower()}_on, "
                f"any(k in fused.stats for k in {COUNTERS!r}), fused._wgrad_f32_on, fused._bwd_layer_f32_on)")
        env.pop("HGNN_WGRAD_F32", None), env.pop("HGNN_BWD_LAYER_F32", None)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert out.stdout.split() == [str(expect), "False", "False", "False", "False"]


@pytest.mark.parametrize("n", [1, 300, 5000])
def test_cpu_tensors_still_take_the_library_bit_for_bit(n):
    """switches on: ``_atb`` with a 3-wide operand, the head's last Linear and the first layer's input gradient keep
    their library expressions on CPU tensors, and no native counter moves"""
    g = torch.Generator().manual_seed(n)
    A, B = torch.randn(n, 3, generator=g), torch.randn(n, 40, generator=g)
    chunks = max(16, min(256, n // 8192))
    c = n // chunks
    if c < 256:
        want = A.t() @ B
    else:
        want = torch.bmm(A[:c * chunks].reshape(chunks, c, 3).transpose(1, 2),
                         B[:c * chunks].reshape(chunks, c, 40)).sum(dim=0)
        if c * chunks < n:
            want += A[c * chunks:].t() @ B[c * chunks:]
    lin = torch.nn.Linear(40, 1)
    old = fused._narrow_f32_on, fused._project_f32_on
    try:
        for flag in (False, True):
            fused.set_narrow_f32(flag)
            fused.set_project_f32(flag)
            before = {k: fused.stats.get(k, 0) for k in COUNTERS + ("library_wgrad_calls", "library_dgrad_calls")}
            assert torch.equal(fused._atb(A, B), want)
            assert fused._head_linear(B, lin, False) is None and fused._head_linear(B, lin, True) is None
            assert fused._narrow_dgrad(B, lin.weight.detach().t()[:, :1], None, None) is None
            after = {k: fused.stats.get(k, 0) for k in before}
            moved = {k: after[k] - before[k] for k in before if after[k] != before[k]}
            assert moved == dict(library_wgrad_calls=1, library_head_calls=2, **({"library_dgrad_calls": 1} if flag else {}))
    finally:
        fused.set_narrow_f32(old[0])
        fused.set_project_f32(old[1])
