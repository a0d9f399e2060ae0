"""CPU: the boundary of the weighted BCE operator and the edge classifier's step: header, binding and exports agree,
and the Python entry points validate their inputs before they touch a device."""
import ctypes
import os
import re

import pytest
import torch

import conftest
from hierarchicalgnn_amd import _lib

HEADER = os.path.join(conftest.ROOT, "include", "hgnn_hip.h")
ENTRY_POINTS = ("hgnn_weighted_bce_workspace_bytes", "hgnn_weighted_bce_forward", "hgnn_weighted_bce_backward")
HP = dict(weight_leak=0.1, ptcut=1.0, pt_interval=0.5, weight_min=0.1, log_weight_ratio=0.0,
          true_edges="pid_true_edges")


def test_entry_points_are_declared_exported_and_bound_under_abi_26():
    txt = open(HEADER).read()
    assert int(re.search(r"#define\s+HGNN_ABI_VERSION\s+(\d+)", txt).group(1)) == 26 == _lib.ABI_VERSION
    lib = _lib.load()
    assert lib.hgnn_abi_version() == 26
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\(", txt) and name in _lib.declared_symbols() and hasattr(lib, name)
    for name in ("COMBINE_SUM", "COMBINE_MAX", "ST_BAD_ID", "ST_BAD_SCORE", "KT", "KF", "ST", "SF", "LOSS", "STATE"):
        assert int(re.search(rf"#define\s+HGNN_WB_{name}\s+(\d+)", txt).group(1)) == getattr(_lib, "WB_" + name)


def test_workspace_size_is_a_host_side_function_of_nothing_but_the_direction():
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    sizes = []
    for p in (0, 1, 2_000_000):
        assert lib.hgnn_weighted_bce_workspace_bytes(p, 0, ctypes.byref(nb)) == 0
        sizes.append(nb.value)
    assert sizes[0] == sizes[1] == sizes[2] > 0          # one partial per workgroup of the largest grid: no [P] scratch
    assert lib.hgnn_weighted_bce_workspace_bytes(2_000_000, 1, ctypes.byref(nb)) == 0 and nb.value == 0
    assert lib.hgnn_weighted_bce_workspace_bytes(-1, 0, ctypes.byref(nb)) != 0


def test_python_surface_is_exported():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import edge_classifier
    for name in ("weighted_bce_loss", "weighted_bce_check", "ec_training_loss", "ec_shared_evaluation"):
        assert getattr(H, name) is getattr(edge_classifier, name)
    import inspect
    assert inspect.signature(H.bipartite_loss).parameters["fused"].default is False
    assert inspect.signature(H.bc_training_loss).parameters["fused"].default is False


def _inputs(p=6, n=4):
    return (torch.full((p,), 0.5), torch.zeros(2, p, dtype=torch.long), torch.zeros(p, dtype=torch.bool),
            torch.ones(n))


def test_cpu_tensors_are_refused_loudly():
    import hierarchicalgnn_amd as H
    s, g, y, pt = _inputs()
    with pytest.raises(RuntimeError, match="HIP device"):
        H.weighted_bce_loss(s, g, y, pt, HP)
    batch = {"edge_index": g, "y": y, "y_pid": y, "pt": pt}
    for mode in ("pid_true_edges", "modulewise_true_edges"):
        with pytest.raises(RuntimeError, match="HIP device"):
            H.ec_training_loss(s, batch, dict(HP, true_edges=mode))


def test_bad_dtypes_shapes_and_modes_raise_value_error():
    import hierarchicalgnn_amd as H
    s, g, y, pt = _inputs()
    bad_calls = [
        lambda: H.weighted_bce_loss(s.double(), g, y, pt, HP),                    # scores dtype
        lambda: H.weighted_bce_loss(s.reshape(2, 3), g, y, pt, HP),               # scores shape
        lambda: H.weighted_bce_loss(s, g.float(), y, pt, HP),                     # graph dtype
        lambda: H.weighted_bce_loss(s, g[:, :5], y, pt, HP),                      # graph shape
        lambda: H.weighted_bce_loss(s, g.reshape(-1), y, pt, HP),
        lambda: H.weighted_bce_loss(s, g, y.float(), pt, HP),                     # y dtype
        lambda: H.weighted_bce_loss(s, g, y[:5], pt, HP),                         # y shape
        lambda: H.weighted_bce_loss(s, g, y, pt.double(), HP),                    # pt dtype
        lambda: H.weighted_bce_loss(s, g, y, pt, HP, pt_b=pt.reshape(2, 2)),      # pt_b shape
        lambda: H.weighted_bce_loss(s, g, y, pt, HP, keep=y.long()),              # keep dtype
        lambda: H.weighted_bce_loss(s, g, y, pt, HP, keep=y[:5]),                 # keep shape
        lambda: H.weighted_bce_loss(s, g, y, pt, HP, combine="mean"),             # unknown combine
        lambda: H.ec_training_loss(s, {"edge_index": g, "y": y, "y_pid": y, "pt": pt},
                                   dict(HP, true_edges="sequential_true_edges")),  # unknown mode
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
