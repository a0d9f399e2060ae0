"""CPU-only checks of the sorted kNN's public surface: argument errors that need no device, and the header."""
import inspect
import os
import re

import pytest
import torch

import conftest

HEADER = os.path.join(conftest.ROOT, "include", "hgnn_hip.h")


def test_bad_method_is_a_value_error():
    from hierarchicalgnn_amd.ops import knn_radius
    x = torch.zeros(4, 3)
    for bad in ("grid", "", "Sorted", None):
        with pytest.raises(ValueError, match="method"):
            knn_radius(x, x, 3, 1.0, method=bad)


def test_cpu_tensors_are_refused_by_both_methods():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd.graph_construction import find_neighbors
    from hierarchicalgnn_amd.ops import knn_radius
    x = torch.zeros(4, 3)
    for method in ("brute", "sorted"):
        with pytest.raises(RuntimeError, match="HIP device"):
            knn_radius(x, x, 3, 1.0, method=method)
    with pytest.raises(RuntimeError, match="HIP device"):
        find_neighbors(x, x, 1.0, 7, method="sorted")
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.frnn_graph(x, 1.0, 7, method="sorted")


def test_stats_need_a_sorted_call_first():
    from hierarchicalgnn_amd import ops
    if ops._knn_sorted_stats is None:
        with pytest.raises(RuntimeError, match="sorted"):
            ops.knn_radius_stats()


def test_method_is_an_optional_last_argument():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd.graph_construction import DynamicGraphConstruction, find_neighbors
    from hierarchicalgnn_amd.ops import knn_radius
    assert inspect.signature(knn_radius).parameters["method"].default == "brute"
    assert list(inspect.signature(knn_radius).parameters)[:5] == ["query", "points", "k", "radius", "return_dist2"]
    assert inspect.signature(H.frnn_graph).parameters["method"].default is None
    assert inspect.signature(find_neighbors).parameters["method"].default is None
    assert DynamicGraphConstruction("exp", {}).knn_method is None
    assert DynamicGraphConstruction("exp", {"knn_method": "sorted"}).knn_method == "sorted"


def test_header_declares_both_functions():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    ws = re.search(r"int\s+hgnn_knn_sorted_workspace_bytes\s*\(([^)]*)\)\s*;", txt)
    run = re.search(r"int\s+hgnn_knn_radius_sorted_f32\s*\(([^)]*)\)\s*;", txt)
    assert ws and run
    assert [a.split()[0] for a in ws.group(1).split(",")] == ["int64_t", "int64_t", "int32_t", "int32_t", "size_t*"]
    assert "stats_out" in run.group(1) and "radius_dev" in run.group(1) and "workspace_bytes" in run.group(1)
    from hierarchicalgnn_amd import _lib
    assert {"hgnn_knn_sorted_workspace_bytes", "hgnn_knn_radius_sorted_f32"} <= set(_lib.declared_symbols())
    assert len(_lib._SIGNATURES["hgnn_knn_radius_sorted_f32"][1]) == len(run.group(1).split(","))
