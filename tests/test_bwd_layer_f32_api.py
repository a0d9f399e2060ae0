"""CPU-side contract of the exact-fp32 fused backward layer: hgnn_mlp_backward_layer_f32's symbols, its host-side
support matrix, the binding's constants, the ``fused.set_bwd_layer_f32`` switch, and the proof that the exact cases of
tests/test_gpu_bwd_layer_f32.py tell a subtly wrong kernel from a right one."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import bwd_layer_f32_ref as B
import conftest
from hierarchicalgnn_amd import _lib, fused

HEADER = os.path.join(conftest.ROOT, "include", "hgnn_hip.h")
SYMBOLS = ("hgnn_mlp_backward_layer_supported_f32", "hgnn_mlp_backward_layer_f32")


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    txt = open(HEADER).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.declared_symbols(), f"{name} is not bound"
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/hgnn_hip.h"
    assert "HGNN_MLP_BWD_F32_BLOCKS" in txt


def test_blocks_constant_matches_the_header():
    m = re.search(r"#define\s+HGNN_MLP_BWD_F32_BLOCKS\s+(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == _lib.MLP_BWD_F32_BLOCKS == B.BLOCKS


def test_support_matrix_through_the_c_abi():
    ok = _lib.load().hgnn_mlp_backward_layer_supported_f32
    for K, N in B.CELL_LN + B.CELL_INPUT:
        assert ok(K, N) == 1, (K, N)
    for K, N in ((512, 1024), (256, 96), (72, 128)):
        assert ok(K, N) == 0, (K, N)
    for K in (64, 1024):
        for N in B.EXACT_N:
            assert ok(K, N) == 1, (K, N)
    for K, N in ((48, 128), (1040, 128), (0, 128), (-64, 128), (256, 0), (256, 32)):
        assert ok(K, N) == 0, (K, N)


def test_switch_defaults_to_off_and_gates_the_support_check():
    assert "HGNN_BWD_LAYER_F32" in os.environ or fused._bwd_layer_f32_on is False
    old = fused._bwd_layer_f32_on
    try:
        fused.set_bwd_layer_f32(False)
        assert not any(fused._bwd_layer_f32_supported(K, N) for K, N in B.CELL_LN + B.CELL_INPUT)
        fused.set_bwd_layer_f32(True)
        assert all(fused._bwd_layer_f32_supported(K, N) for K, N in B.CELL_LN + B.CELL_INPUT)
        assert not fused._bwd_layer_f32_supported(512, 1024)
    finally:
        fused.set_bwd_layer_f32(old)
    assert "bwd_layer_f32_calls" in fused.stats


@pytest.mark.parametrize("value,expect", [(None, False), ("1", True), ("0", False)])
def test_switch_follows_the_environment_in_a_fresh_process(value, expect):
    env = {k: v for k, v in os.environ.items() if k != "HGNN_BWD_LAYER_F32"}
    if value is not None:
        env["HGNN_BWD_LAYER_F32"] = value
    env["PYTHONPATH"] = conftest.ROOT + os.pathsep + env.get("PYTHONPATH", "")
    code = "from hierarchicalgnn_amd import fused; print(fused._bwd_layer_f32_on, fused._bwd_layer_f32_supported(256, 512))"
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(expect), str(expect)]


def test_cpu_tensors_are_refused_loudly():
    dz, W = torch.zeros(4, 64), torch.zeros(64, 64)
    n0 = fused.stats["bwd_layer_f32_calls"]
    with pytest.raises(RuntimeError, match="HIP device"):
        fused._bwd_layer_f32(dz, W, None, None, None, 0, 1e-5)
    with pytest.raises(RuntimeError, match="HIP device"):
        fused._bwd_layer_f32(dz, W, torch.zeros(4, 64), torch.ones(64), torch.zeros(64), 1, 1e-5, want_a=True)
    assert fused.stats["bwd_layer_f32_calls"] == n0


@pytest.mark.parametrize("N", B.EXACT_N)
@pytest.mark.parametrize("K", B.EXACT_K)
def test_every_mutant_is_told_apart_in_fp32(K, N):
    """at every (M, K, N, form) of the GPU file's exact cases: the float64 product is exact in fp32, and each mutant of
    it differs from it in at least one fp32 element -- no bf16 rounding hides a one-unit error"""
    for M in B.EXACT_M:
        for form in B.FORMS:
            dz, W, skip = B.exact_case(M, K, N, form)
            ref = B.dgrad_ref_f32(dz, W, skip)
            assert float(ref.abs().max()) < B.G.EXACT_LIMIT
            for name, wrong in B.dgrad_mutants_f32(dz, W, skip).items():
                assert not torch.equal(wrong, ref), f"M={M} K={K} N={N} {form}: mutant {name} equals the reference"
