"""Surface of the assignment loss: exports, C symbols, ABI number, error behaviour without a GPU."""
import ctypes
import os
import re

import pytest
import torch

import hierarchicalgnn_amd as H
from hierarchicalgnn_amd import _lib, assignment, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports():
    for name in ("max_weight_matching", "bipartite_loss", "bc_embedding_loss", "bc_training_loss", "gap_bound"):
        assert callable(getattr(H, name)) and getattr(H, name) is getattr(assignment, name)
    assert "host_reads" in assignment.stats
    assert callable(synth.assignment_event)


def test_c_symbols_resolve_and_abi_stays_26():
    lib = _lib.load()
    for name in ("hgnn_assign_match", "hgnn_assign_match_workspace_bytes"):
        assert name in _lib.declared_symbols() and getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "hgnn_hip.h")).read()
    assert re.search(r"#define HGNN_ABI_VERSION 26\b", header)
    assert lib.hgnn_abi_version() == 26 == _lib.ABI_VERSION
    for name in ("hgnn_assign_match", "hgnn_assign_match_workspace_bytes"):
        assert re.search(r"\bint %s\(" % name, header)
    for name, value in (("HGNN_AM_SCALE_BITS", _lib.AM_SCALE_BITS), ("HGNN_AM_INFO", _lib.AM_INFO),
                        ("HGNN_AM_ST_BAD_ID", _lib.AM_ST_BAD_ID), ("HGNN_AM_ST_BAD_WEIGHT", _lib.AM_ST_BAD_WEIGHT),
                        ("HGNN_AM_ST_OVERFLOW", _lib.AM_ST_OVERFLOW), ("HGNN_AM_ST_BUDGET", _lib.AM_ST_BUDGET),
                        ("HGNN_AM_HOST_READS", _lib.AM_HOST_READS), ("HGNN_AM_TAIL_ROUNDS", _lib.AM_TAIL_ROUNDS)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name


def test_workspace_bytes_rejects_empty_and_oversized_problems():
    # argument checks come before anything that needs a device
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    assert lib.hgnn_assign_match_workspace_bytes(0, 5, 5, ctypes.byref(nb)) != 0
    assert b"positive" in lib.hgnn_last_error()
    assert lib.hgnn_assign_match_workspace_bytes(10, 1 << 29, 1 << 29, ctypes.byref(nb)) != 0
    assert b"2^30" in lib.hgnn_last_error()


def test_gap_bound_conditions():
    # the two conditions of the design: 1e-4 at config-3 size, and 0 on the 2^-12 grid
    assert 0 < H.gap_bound(12_000, 10_000, 2.0 ** 10) <= 1e-4
    assert H.gap_bound(12_000, 10_000, 2.0 ** 10) == 22_000 * 2.0 ** -30
    assert H.gap_bound(12_000, 10_000, 2.0 ** 10, grid_bits=12) == 0.0
    with pytest.raises(ValueError):
        H.gap_bound(1 << 20, 1 << 20, 2.0 ** 20)


def test_cpu_tensors_raise():
    ev = synth.assignment_event(400, 30, 3, seed=1)
    g = ev["bipartite_graph"]
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.max_weight_matching(g[0], g[1], ev["scores"], 400, 30)
    hp = {"weight_leak": 0.1, "ptcut": 1.0, "pt_interval": 0.5, "weight_min": 0.1, "log_weight_ratio": 0.0,
          "train_r": 1.0}
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.bipartite_loss(ev["scores"], g, ev, hp)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.bc_embedding_loss(torch.zeros(400, 4), torch.zeros(2, 5, dtype=torch.long), ev, hp)


def test_assignment_event_shape_and_dyadic_grid():
    ev = synth.assignment_event(2000, 100, 5, seed=3, dyadic=True)
    assert ev["bipartite_graph"].shape == (2, 10_000) and ev["scores"].shape == (10_000,)
    s = ev["scores"].double() * 4096
    assert torch.equal(s, s.round()) and s.min() >= 1 and s.max() <= 4096
    assert int(ev["bipartite_graph"][1].max()) < 100
    again = synth.assignment_event(2000, 100, 5, seed=3, dyadic=True)
    assert all(torch.equal(ev[k], again[k]) for k in ev)
    ev = synth.assignment_event(2000, 100, 5, seed=3)
    assert 0 < float(ev["scores"].min()) and float(ev["scores"].max()) < 1
