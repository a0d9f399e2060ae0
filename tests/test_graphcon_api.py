"""CPU: the boundary of the device-side graph construction (csrc/graphcon.hip): header, binding and exports agree, the
workspace sizes are computed on the host (that of hgnn_knn_edges needs the HIP runtime for rocprim's share, so only its
refusals are checked here), the defaults of the module are unchanged, and the Python entry points validate
their inputs before they touch a device."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import conftest
from hierarchicalgnn_amd import _lib

HEADER = os.path.join(conftest.ROOT, "include", "hgnn_hip.h")
ENTRY_POINTS = ("hgnn_knn_edges_workspace_bytes", "hgnn_knn_edges", "hgnn_graph_attention_workspace_bytes",
                "hgnn_graph_attention_forward", "hgnn_graph_attention_backward")


def test_entry_points_are_declared_exported_and_bound_under_abi_26():
    txt = open(HEADER).read()
    assert int(re.search(r"#define\s+HGNN_ABI_VERSION\s+(\d+)", txt).group(1)) == 26 == _lib.ABI_VERSION
    lib = _lib.load()
    assert lib.hgnn_abi_version() == 26
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\(", txt) and name in _lib.declared_symbols() and hasattr(lib, name)
    assert int(re.search(r"#define\s+HGNN_GC_ST_BAD_ID\s+(\d+)", txt).group(1)) == _lib.GC_ST_BAD_ID
    for name in ("MAX_DIM", "FN_SIGMOID", "FN_EXP", "TRAINING", "NORM", "MEAN", "VAR", "RSTD", "SUMF", "E", "DBETA",
                 "DGAMMA", "SGF", "STATE"):
        assert int(re.search(rf"#define\s+HGNN_GA_{name}\s+(\d+)", txt).group(1)) == getattr(_lib, "GA_" + name)


def test_workspace_sizes_are_host_side_functions():
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    # the sizes of hgnn_knn_edges hold rocprim's own scratch, which rocprim sizes per device: their values are
    # checked where a device exists (tests/test_gpu_graphcon.py); the refusals below come before that
    assert lib.hgnn_knn_edges_workspace_bytes(-1, 5, 10, 0, ctypes.byref(nb)) != 0
    assert lib.hgnn_knn_edges_workspace_bytes(10, 0, 10, 0, ctypes.byref(nb)) != 0
    assert lib.hgnn_knn_edges_workspace_bytes(10, 5, 2 ** 31 + 1, 1, ctypes.byref(nb)) != 0    # n > 2^31
    assert lib.hgnn_knn_edges_workspace_bytes(2 ** 29, 2, 10, 0, ctypes.byref(nb)) != 0        # nq K >= 2^30
    got = []
    for e in (0, 2, 4_000_000):
        for backward in (0, 1):
            assert lib.hgnn_graph_attention_workspace_bytes(e, backward, ctypes.byref(nb)) == 0
            got.append(nb.value)
    assert len(set(got)) == 1 and got[0] > 0                           # one partial per workgroup: no [E] scratch
    assert lib.hgnn_graph_attention_workspace_bytes(-1, 0, ctypes.byref(nb)) != 0


def test_python_surface_is_exported_and_defaults_are_unchanged():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import graph_construction as G, ops
    assert H.knn_edges is ops.knn_edges and H.attention_weights is G.attention_weights
    assert G.stats is ops.gc_stats and G.stats["host_reads"] >= 0
    M = G.DynamicGraphConstruction
    assert inspect.signature(M.build_graph).parameters["fused"].default is None
    assert inspect.signature(M.edge_weights).parameters["fused"].default is None
    assert inspect.signature(ops.knn_edges).parameters["sym"].default is False
    p = inspect.signature(G.attention_weights).parameters
    assert p["norm"].default is False and p["logits"].default is False
    assert list(inspect.signature(M.build_graph).parameters)[:5] == ["self", "src_embeddings", "dst_embeddings", "sym",
                                                                     "k"]
    assert list(inspect.signature(M.edge_weights).parameters)[:7] == ["self", "src_embeddings", "dst_embeddings",
                                                                      "graph", "norm", "logits", "stat_reduce"]
    for hp in (None, {}, {"knn_method": "sorted"}, {"graph_construction": "torch"}):
        assert M("sigmoid", hp).fused is False
    assert M("exp", {"graph_construction": "fused"}).fused is True
    with pytest.raises(ValueError, match="graph_construction"):
        M("exp", {"graph_construction": "triton"})
    m = M("sigmoid", {"graph_construction": "fused"})
    assert sorted(m.state_dict()) == sorted(M("sigmoid", {}).state_dict())      # same checkpoint keys


def _inputs(e=6, n=4, d=8):
    return torch.randn(n, d), torch.randn(n, d), torch.zeros(2, e, dtype=torch.long), torch.nn.BatchNorm1d(1)


def test_cpu_tensors_are_refused_loudly():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd.graph_construction import DynamicGraphConstruction
    a, b, g, bn = _inputs()
    with pytest.raises(RuntimeError, match="HIP device"):
        H.attention_weights(a, b, g, bn, "sigmoid")
    with pytest.raises(RuntimeError, match="HIP device"):
        H.knn_edges(torch.zeros(3, 2, dtype=torch.long), 4)
    m = DynamicGraphConstruction("exp", {"graph_construction": "fused"})
    with pytest.raises(RuntimeError, match="HIP device"):
        m.edge_weights(a, b, g)
    with pytest.raises(RuntimeError, match="HIP device"):
        DynamicGraphConstruction("exp", {}).edge_weights(a, b, g, fused=True)


def test_bad_arguments_raise_value_error_before_a_device_is_touched():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd.graph_construction import DynamicGraphConstruction
    a, b, g, bn = _inputs()
    idx = torch.zeros(3, 2, dtype=torch.long)
    bad_calls = [
        lambda: H.attention_weights(a.double(), b.double(), g, bn, "sigmoid"),     # embedding dtype
        lambda: H.attention_weights(a, b[:, :4], g, bn, "sigmoid"),                # D mismatch
        lambda: H.attention_weights(torch.randn(4, 17), torch.randn(4, 17), g, bn, "sigmoid"),   # D > 16
        lambda: H.attention_weights(a.reshape(-1), b, g, bn, "sigmoid"),           # shape
        lambda: H.attention_weights(a, b, g.float(), bn, "sigmoid"),               # graph dtype
        lambda: H.attention_weights(a, b, g.reshape(-1), bn, "sigmoid"),           # graph shape
        lambda: H.attention_weights(a, b, g[:1], bn, "sigmoid"),
        lambda: H.attention_weights(a, b, g, torch.nn.BatchNorm1d(2), "sigmoid"),  # not BatchNorm1d(1)
        lambda: H.attention_weights(a, b, g, torch.nn.BatchNorm1d(1, affine=False), "sigmoid"),
        lambda: H.attention_weights(a, b, g, bn, "tanh"),                          # unknown function
        lambda: H.attention_weights(a, b, g, bn, torch.tanh),
        lambda: H.attention_weights(a, b, g[:, :1], bn, "exp"),                    # training mode, E = 1
        lambda: H.attention_weights(a, b, g[:, :0], bn, "exp"),                    # training mode, E = 0
        lambda: H.knn_edges(idx.int(), 4),                                         # idx dtype
        lambda: H.knn_edges(idx.reshape(-1), 4),                                   # idx shape
        lambda: H.knn_edges(idx, -1),
        lambda: H.knn_edges(idx, 2 ** 31 + 1),                                     # n > 2^31
        lambda: H.knn_edges(idx, 2 ** 31 + 1, sym=True),
        lambda: DynamicGraphConstruction("exp", {"graph_construction": "fused"}).edge_weights(
            a, b, g, stat_reduce=lambda t: t),                                     # fused + synchronised BatchNorm
        lambda: DynamicGraphConstruction("exp", {}).edge_weights(a, b, g, stat_reduce=lambda t: t, fused=True),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="sigmoid.*exp"):
        H.attention_weights(a, b, g, bn, "tanh")
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        H.attention_weights(a, b, g[:, :1], bn, "exp")


def test_c_entry_points_refuse_bad_arguments_on_the_host():
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)                                   # never dereferenced: the checks come first
    # training mode with one edge, D out of range, an unknown function, unknown flag bits
    for e, d, flags, fn in ((1, 8, _lib.GA_TRAINING, 0), (4, 0, 0, 0), (4, 17, 0, 0), (4, 8, 0, 2), (4, 8, 4, 0)):
        rc = lib.hgnn_graph_attention_forward(one, 4, one, 4, d, one, _lib.DT_I64, e, one, one, one, one, one, 1e-5,
                                              0.1, flags, fn, one, one, one, one, one, 1 << 20, null)
        assert rc != 0, (e, d, flags, fn)
    rc = lib.hgnn_knn_edges(one, 4, 2, 2 ** 31 + 1, 1, one, 16, one, one, 1 << 20, null)
    assert rc != 0
    rc = lib.hgnn_knn_edges(one, 4, 2, 8, 1, one, 8, one, one, 1 << 20, null)      # cap < 2 nq K with sym
    assert rc != 0
