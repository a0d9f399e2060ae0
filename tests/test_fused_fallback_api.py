"""The library path of ``mlp.concat_mlp`` is visible (``fused.stats["library_calls"]``) and can be refused
(``strict``); the process-level switches round-trip; the constants of the N = 1024 backward layer agree between the
header and the binding.  No GPU needed."""
import os
import re

import pytest
import torch

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hgnn_hip.h")


def test_options_accepts_strict_and_refuses_unknown_names():
    from hierarchicalgnn_amd import fused
    assert "strict" in fused._OPTION_NAMES and fused._opt("strict") is False
    with fused.options(strict=True):
        assert fused._opt("strict") is True
        with fused.options(strict=False):
            assert fused._opt("strict") is False
        assert fused._opt("strict") is True
    assert fused._opt("strict") is False
    with pytest.raises(TypeError):
        with fused.options(stricter=True):
            pass


def _net_and_rows():
    from hierarchicalgnn_amd import make_mlp
    torch.manual_seed(3)
    net = make_mlp(24, 40, 8, 2, layer_norm=True, output_activation="Tanh", hidden_activation="GELU")
    return net, torch.randn(11, 24)


def test_concat_mlp_on_cpu_rows_counts_one_library_call():
    from hierarchicalgnn_amd import fused, mlp
    net, x = _net_and_rows()
    n0 = fused.stats["library_calls"]
    out = mlp.concat_mlp(net, [(x, None)])
    assert fused.stats["library_calls"] == n0 + 1
    assert torch.equal(out, net(x))
    with torch.no_grad():
        out = mlp.concat_mlp(net, [(x, None)])
    assert fused.stats["library_calls"] == n0 + 2 and torch.equal(out, net(x))


def test_strict_raises_instead_of_falling_back():
    from hierarchicalgnn_amd import fused, mlp
    net, x = _net_and_rows()
    n0 = fused.stats["library_calls"]
    with fused.options(strict=True):
        with pytest.raises(RuntimeError) as e:
            mlp.concat_mlp(net, [(x, None)])
    assert "24 -> 40 -> 8" in str(e.value) and "float32" in str(e.value)
    assert fused.stats["library_calls"] == n0
    fused.set_strict(True)
    try:
        with pytest.raises(RuntimeError):
            mlp.concat_mlp(net, [(x, None)])
        with fused.options(strict=False):                      # the context overrides the process default
            assert torch.equal(mlp.concat_mlp(net, [(x, None)]), net(x))
    finally:
        fused.set_strict(False)
    assert torch.equal(mlp.concat_mlp(net, [(x, None)]), net(x))


def test_process_switches_round_trip():
    from hierarchicalgnn_amd import fused
    old = fused._bwd_layer_wide
    try:
        fused.set_bwd_layer_wide(True)
        assert fused._bwd_layer_wide is True
        fused.set_bwd_layer_wide(False)
        assert fused._bwd_layer_wide is False and not fused._bwd_layer_supported(512, 1024)
    finally:
        fused.set_bwd_layer_wide(old)
    assert fused._strict is False
    fused.set_strict(1)
    assert fused._strict is True and fused._opt("strict") is True
    fused.set_strict(False)
    assert fused._strict is False


def test_new_counters_exist():
    from hierarchicalgnn_amd import fused
    for k in ("library_calls", "library_dgrad_calls", "bwd_layer_calls", "hybrid_train_calls"):
        assert fused.stats[k] >= 0


def test_tile_rows_constant_matches_the_header_and_the_abi_is_26():
    from hierarchicalgnn_amd import _lib
    txt = open(HEADER).read()
    assert int(re.search(r"#define\s+HGNN_MLP_BWD_TILE_ROWS_N1024\s+(\d+)", txt).group(1)) == _lib.MLP_BWD_TILE_ROWS_N1024
    assert int(re.search(r"#define\s+HGNN_MLP_BWD_BLOCKS\s+(\d+)", txt).group(1)) == _lib.MLP_BWD_BLOCKS
    assert int(re.search(r"#define\s+HGNN_ABI_VERSION\s+(\d+)", txt).group(1)) == 26 == _lib.ABI_VERSION
    assert _lib.load().hgnn_abi_version() == 26
    assert _lib.load().hgnn_mlp_backward_layer_supported_bf16(512, 1024) == 1
