"""Surface of the GPU HDBSCAN: exports, C symbols, ABI number, the cuml shim, error behaviour without a GPU."""
import ctypes
import importlib
import os
import re
import sys

import pytest
import torch

import hierarchicalgnn_amd as H
from hierarchicalgnn_amd import _lib, tracking

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hgnn_hdbscan_workspace_bytes", "hgnn_hdbscan_f32", "hgnn_hdbscan_tree_host")


def test_exports():
    mod = importlib.import_module("hierarchicalgnn_amd.hdbscan")
    assert H.hdbscan is mod.hdbscan and H.hdbscan_tree is mod.hdbscan_tree
    assert H.embedding_track_candidates is tracking.embedding_track_candidates
    assert "host_reads" in mod.stats


def test_c_symbols_resolve_and_abi_stays_26():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "hgnn_hip.h")).read()
    for name in NAMES:
        assert name in _lib.declared_symbols() and getattr(lib, name) is not None
        assert re.search(r"\bint %s\(" % name, header)
    assert re.search(r"#define HGNN_ABI_VERSION 26\b", header)
    assert lib.hgnn_abi_version() == 26 == _lib.ABI_VERSION
    for name, value in (("HGNN_HDB_ROUNDS", _lib.HDB_ROUNDS), ("HGNN_HDB_HOST_READS", _lib.HDB_HOST_READS),
                        ("HGNN_HDB_N_CLUSTERS", _lib.HDB_N_CLUSTERS), ("HGNN_HDB_STAGE_SYNC", _lib.HDB_STAGE_SYNC),
                        ("HGNN_HDB_T_CORE_NS", _lib.HDB_T_CORE_NS), ("HGNN_HDB_T_SORT_NS", _lib.HDB_T_SORT_NS),
                        ("HGNN_HDB_T_TREE_NS", _lib.HDB_T_TREE_NS), ("HGNN_HDB_T_ROUND0_NS", _lib.HDB_T_ROUND0_NS),
                        ("HGNN_HDB_INFO", _lib.HDB_INFO)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert re.search(r"#define HGNN_HDBSCAN_LAMBDA_DUP 0x1p100\b", header) and _lib.HDBSCAN_LAMBDA_DUP == 2.0 ** 100


def test_argument_errors_come_with_a_message():
    # argument checks come before anything that needs a device
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    assert lib.hgnn_hdbscan_workspace_bytes(100, 17, 5, 5, ctypes.byref(nb)) != 0
    assert b"D must be in [1, 16]" in lib.hgnn_last_error()
    assert lib.hgnn_hdbscan_workspace_bytes(4, 8, 5, 5, ctypes.byref(nb)) != 0
    assert b"below min_cluster_size" in lib.hgnn_last_error()
    assert lib.hgnn_hdbscan_workspace_bytes(1000, 8, 5, 129, ctypes.byref(nb)) != 0
    assert b"min_samples must be in [1, 128]" in lib.hgnn_last_error()
    assert lib.hgnn_hdbscan_workspace_bytes((1 << 21) + 1, 8, 5, 5, ctypes.byref(nb)) != 0
    assert b"2^21" in lib.hgnn_last_error()
    info = (ctypes.c_int64 * _lib.HDB_INFO)()
    assert lib.hgnn_hdbscan_f32(None, 100, 8, 5, 5, None, None, None, None, info, None, 0, None) != 0
    assert b"NULL points" in lib.hgnn_last_error()
    assert lib.hgnn_hdbscan_f32(ctypes.c_void_p(256), 100, 17, 5, 5, None, None, None, None, info, None, 0, None) != 0
    assert b"D must be in [1, 16]" in lib.hgnn_last_error()
    assert lib.hgnn_hdbscan_f32(ctypes.c_void_p(256), 100, 8, 5, 5, None, None, None, None, info, None, 0, None) != 0
    assert b"NULL output" in lib.hgnn_last_error()


def test_cpu_tensors_raise():
    x = torch.zeros(100, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.hdbscan(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.hdbscan_tree(x, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.embedding_track_candidates(x)


def test_cuml_shim_surface():
    sys.path.insert(0, os.path.join(ROOT, "cuml_shim"))
    try:
        from cuml.cluster import HDBSCAN
    finally:
        sys.path.pop(0)
    m = HDBSCAN(min_cluster_size=7, metric="euclidean", cluster_selection_method="eom", verbose=0)
    assert m.min_cluster_size == 7 and callable(m.fit_predict)
    with pytest.raises(NotImplementedError, match="metric"):
        HDBSCAN(min_cluster_size=5, metric="manhattan")
    with pytest.raises(NotImplementedError, match="cluster_selection_method"):
        HDBSCAN(min_cluster_size=5, cluster_selection_method="leaf")
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.fit_predict(torch.zeros(50, 8))
    with pytest.raises(TypeError, match="DLPack"):
        m.fit_predict([[0.0, 1.0]])
