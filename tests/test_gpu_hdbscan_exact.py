"""GPU: exact conformance of hgnn_hdbscan_f32 (csrc/hdbscan.hip) at its dispatch edges, against the numpy restatement
(tests/hdbscan_ref.py) evaluated on the cases of tests/hdbscan_exact_cases.py (proved by
tests/test_hdbscan_exact_ref.py).  Every comparison is equality of bits or of integers.

  * per case: core2 on bits, the MST edges element for element in the library's (w2, min, max) order, w2 on bits,
    the labels element for element, and rounds <= ceil(log2 N).  The cases run all 15 k_hdb_core<KP, DP>
    instantiations with min_samples on both sides of every KP edge, D on both sides of every DP edge, N on the tile
    and slice edges (255 .. 513, 4096, 4097), duplicated points (zero-weight multi-way levels built from device
    output) and lattice patches whose levels join up to 272 points.
  * buffers: one case per DP through ctypes with a workspace of exactly the reported size between guard zones,
    filled with 0xFF twice and with 0x00 twice: the same bits four times, the reference's.
  * a side stream, a non-contiguous view of the points.
  * one NaN and one +inf coordinate among 300 finite points: the "joined nothing" error, and the reference result
    on the next call.

Measured wall time on an MI355X: 2.5 s for the file (88 tests); the slowest tests take 0.31 s (N = 4096 and 4097, the
restatement included).

Wrong kernels run once on an MI355X against this file (library variants built outside the tree): the rank pick
``s == k`` for ``s == k - 1`` in k_hdb_core failed 87 of the 88 tests (all but the table check); k_hdb_nearest never
scanning the last candidate slice failed 17, among them edge_n511, edge_n512, edge_n513, edge_n4096, both track-like
duplicate cases, seven of the N = 257 grid cases, patch_17x16_ms1 and the side-stream test."""
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch

import hdbscan_exact_cases as X
from test_gpu_scalar_ops_exact import Workspace, assert_bits, on_side_stream

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _H():
    import hierarchicalgnn_amd
    return hierarchicalgnn_amd


def _stats():
    return importlib.import_module("hierarchicalgnn_amd.hdbscan").stats     # the package's `hdbscan` is the function


def _x(name):
    return torch.from_numpy(X.points(X.CASES[name])).to(DEV)


def _check(name, got, what=""):
    """got: (labels, edges, w2, core2) as numpy arrays"""
    labels, edges, w2, core2 = got
    rl, re, rw, rc, _ = X.reference(name)
    what = f"{name}{what} {X.TABLE[name]}"
    assert_bits(core2, rc, f"{what}: core2")
    assert edges.dtype == np.int64 and edges.shape == re.shape, what
    if not np.array_equal(edges, re):
        i = int(np.flatnonzero((edges != re).any(1))[0])
        raise AssertionError(f"{what}: MST edge {i} is {edges[i].tolist()} (w2 {w2[i]!r}), want {re[i].tolist()} "
                             f"(w2 {rw[i]!r}); {int((edges != re).any(1).sum())} of {len(re)} edges differ")
    assert_bits(w2, rw, f"{what}: w2")
    assert labels.dtype == np.int64
    assert np.array_equal(labels, rl), (f"{what}: {int((labels != rl).sum())} of {len(rl)} labels differ, the first at "
                                        f"{int(np.flatnonzero(labels != rl)[0])}")


def _run(name, x=None):
    c = X.CASES[name]
    out = _H().hdbscan_tree(_x(name) if x is None else x, c["mcs"], c["ms"])
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("name", X.NAMES)
def test_case_matches_the_restatement(name):
    got = _run(name)
    last = _stats()["last"]
    n = len(X.CASES[name]["q"])
    assert last["n"] == n and 1 <= last["rounds"] <= math.ceil(math.log2(n)), last
    _check(name, got)


def test_every_instantiation_is_among_the_cases():
    assert {v[:2] for v in X.TABLE.values()} >= {(kp, dp) for kp in (8, 16, 32, 64, 128) for dp in (4, 8, 16)}


def _ctypes_call(name, fill, stream=None):
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    c = X.CASES[name]
    n, d = c["q"].shape
    nb = ctypes.c_size_t(0)
    _lib.check(lib.hgnn_hdbscan_workspace_bytes(n, d, c["mcs"], c["ms"], ctypes.byref(nb)), "workspace_bytes")
    ws = Workspace(nb.value, fill)
    x = _x(name)
    labels = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    edges = torch.full((n - 1, 2), -7, dtype=torch.int64, device=DEV)
    w2 = torch.full((n - 1,), -7.0, dtype=torch.float32, device=DEV)
    core2 = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    info = (ctypes.c_int64 * _lib.HDB_INFO)()
    _lib.check(lib.hgnn_hdbscan_f32(_lib.ptr(x), n, d, c["mcs"], c["ms"], _lib.ptr(labels), _lib.ptr(edges),
                                    _lib.ptr(w2), _lib.ptr(core2), info, ws.ptr(), nb.value,
                                    _lib.current_stream(x.device)), "hgnn_hdbscan_f32")
    torch.cuda.synchronize()
    ws.done(f"{name} fill {fill:#x}")
    return tuple(t.cpu().numpy() for t in (labels, edges, w2, core2))


@pytest.mark.parametrize("name", ["grid_d4_ms33", "dup_mcs5_ms5", "grid_d9_ms17"])
def test_poisoned_exact_size_workspace(name):
    """DP = 4, 8 and 16; nothing may be read from the workspace before it is written"""
    assert [X.TABLE[n][1] for n in ("grid_d4_ms33", "dup_mcs5_ms5", "grid_d9_ms17")] == [4, 8, 16]
    for fill in (0xFF, 0xFF, 0x00, 0x00):
        _check(name, _ctypes_call(name, fill), f" (workspace filled with {fill:#x})")


def test_side_stream():
    name = "edge_n513"
    _check(name, on_side_stream(lambda: _run(name)), " (side stream)")


def test_non_contiguous_points():
    name = "grid_d5_ms9"
    x = _x(name)
    wide = torch.full((x.shape[0] + 1, 2 * x.shape[1] + 1), float("nan"), device=DEV)
    wide[1:, 1::2] = x
    view = wide[1:, 1::2]
    assert not view.is_contiguous() and torch.equal(view, x)
    _check(name, _run(name, view), " (strided view)")


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_one_non_finite_coordinate_is_an_error_and_the_next_call_is_clean(bad):
    name = "edge_n257"
    x = _x(name)
    dirty = torch.cat([x, x[:43] + 0.25])
    assert dirty.shape[0] == 300 and bool(torch.isfinite(dirty).all())
    dirty = torch.cat([dirty[:150], torch.tensor([[0.0, 0.0, bad, 0.0, 0.0, 0.0, 0.0, 0.0]], device=DEV), dirty[150:]])
    with pytest.raises(RuntimeError, match="joined nothing"):
        _H().hdbscan_tree(dirty, 5, 5)
    _check(name, _run(name), " (after the error)")
