"""CPU tests of the HDBSCAN contract: the numpy restatement (tests/hdbscan_ref.py) against scipy / sklearn, the
fixtures of tests/golden/hdbscan_cases.npz against the restatement, and the library's host tree stage
(hgnn_hdbscan_tree_host, csrc/hdbscan.hip) against the restatement's labels.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdbscan_ref as R  # noqa: E402
from golden import make_hdbscan_golden as G  # noqa: E402

from conftest import load_golden  # noqa: E402

SMALL = [n for n in G.EXACT if n != "tracks2000"]


@pytest.fixture(scope="module")
def cases():
    return load_golden("hdbscan_cases.npz")


def _x(cases, name):
    return cases[name + "/q"].astype(np.float32) / np.float32(128.0)


def test_fixture_inputs_are_on_the_grid_and_distinct(cases):
    for name in G.EXACT:
        q = cases[name + "/q"]
        assert q.dtype == np.int16 and np.abs(q).max() <= 128
        assert len(np.unique(q, axis=0)) == len(q), name
        assert tuple(cases[name + "/params"]) == G.EXACT[name]
    assert {cases[n + "/q"].shape[1] for n in G.EXACT} >= {3, 8, 16}
    # the many-way case: 36 points, at most 3 distinct merge weights
    assert len(np.unique(cases["lattice_manyway/w2"])) <= 3
    assert (cases["chain_all_noise/labels"] < 0).all() and (cases["n_eq_mcs/labels"] < 0).all()
    assert cases["two_blobs/labels"].max() == 1


@pytest.mark.parametrize("name", list(G.EXACT))
def test_fixtures_are_the_restatement(cases, name):
    """the stored expectations are what the restatement computes, and every EOM decision has a float64 margin
    above 1e-9 relative (so no summation order can flip one)"""
    mcs, ms = G.EXACT[name]
    labels, edges, w2, c2, info = R.hdbscan(_x(cases, name), mcs, ms, return_all=True)
    assert info["eom_margin"] > 1e-9
    assert np.array_equal(labels, cases[name + "/labels"])
    assert np.array_equal(edges, cases[name + "/edges"])
    assert np.array_equal(w2, cases[name + "/w2"]) and np.array_equal(c2, cases[name + "/core2"])
    kept = labels[labels >= 0]
    assert kept.size == 0 or np.bincount(kept).min() >= mcs
    # canonical numbering: first appearances ascend
    first = [int(np.flatnonzero(labels == c)[0]) for c in range(labels.max() + 1)]
    assert first == sorted(first)


@pytest.mark.parametrize("name", SMALL)
def test_mst_weights_match_scipy_on_sklearn_core_distances(cases, name):
    """sqrt of the sorted MST weight multiset == sorted weights of scipy's minimum_spanning_tree on the dense
    mutual-reachability matrix from sklearn's core distances; exact on the grid (the multiset is the same for any
    MST, so ties do not matter)"""
    from scipy.sparse.csgraph import minimum_spanning_tree
    from sklearn.neighbors import NearestNeighbors
    mcs, ms = G.EXACT[name]
    x = _x(cases, name).astype(np.float64)
    core = NearestNeighbors(n_neighbors=ms, algorithm="brute").fit(x).kneighbors(x)[0][:, -1]
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    mr = np.maximum(np.maximum(d, core[:, None]), core[None, :])
    np.fill_diagonal(mr, 0.0)
    ref = np.sort(minimum_spanning_tree(mr).data)
    got = np.sqrt(np.sort(cases[name + "/w2"]).astype(np.float64))
    assert ref.shape == got.shape
    assert np.array_equal(core, np.sqrt(cases[name + "/core2"].astype(np.float64)))
    assert np.array_equal(ref, got)


def _components(n, a, b):
    parent = np.arange(n)

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for u, v in zip(a.tolist(), b.tolist()):
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(v) for v in range(n)])


@pytest.mark.parametrize("name", ["tracks300", "uniform", "lattice_manyway", "d3", "ms10"])
def test_cuts_of_the_mst_are_the_components_of_the_thresholded_graph(cases, name):
    x = _x(cases, name)
    n = len(x)
    c2, w2, edges = cases[name + "/core2"], cases[name + "/w2"], cases[name + "/edges"]
    full = np.maximum(np.maximum(R.d2_rows(x, 0, n), c2[:, None]), c2[None, :])
    for qt in (0.1, 0.3, 0.5, 0.8, 0.95):
        t = np.quantile(w2, qt)
        keep = w2 <= t
        mine = _components(n, edges[keep, 0], edges[keep, 1])
        i, j = np.nonzero(np.triu(full <= t, 1))
        assert np.array_equal(mine, _components(n, i, j)), (name, qt)


def test_against_sklearn_within_twice_its_own_tie_noise(cases):
    """1 - B <= 2 (1 - A): two tie orders of sklearn differ from each other on tied points; the tie-free rule can
    differ from either only on those same points"""
    from sklearn.metrics import adjusted_rand_score
    x = cases["continuous/x"]
    sk, a = G.sklearn_self_ari(x)
    labels, edges, w2, c2, info = R.hdbscan(x, 5, 5, return_all=True)
    b = adjusted_rand_score(sk, labels)
    print(f"A = {a:.6f}, B = {b:.6f}; stored {cases['continuous/AB']}")
    assert a < 1.0, "vacuous bound: sklearn agrees with itself on this fixture"
    assert 1 - b <= 2 * (1 - a)
    assert np.array_equal(labels, cases["continuous/labels"]) and np.array_equal(w2, cases["continuous/w2"])
    assert np.array_equal(sk, cases["continuous/sklearn_labels"])
    assert np.allclose(cases["continuous/AB"], [a, b], rtol=0, atol=1e-12)


def test_restatement_is_permutation_invariant(cases):
    x = _x(cases, "d3")
    base = R.hdbscan(x, 5)
    p = np.random.default_rng(5).permutation(len(x))
    lp = R.hdbscan(x[p], 5)
    back = np.empty_like(lp)
    back[p] = lp
    assert np.array_equal(R.canonical(back), base)


@pytest.mark.parametrize("name", list(G.EXACT) + ["continuous"])
def test_host_tree_stage_gives_the_restatement_labels(cases, name):
    """hgnn_hdbscan_tree_host (the tree stage hgnn_hdbscan_f32 runs on the host) on the restatement's MST"""
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    if name == "continuous":
        x, mcs = cases["continuous/x"], 5
        _, edges, w2, _, _ = R.hdbscan(x, 5, 5, return_all=True)
    else:
        mcs = G.EXACT[name][0]
        edges, w2 = cases[name + "/edges"], cases[name + "/w2"]
    n = len(w2) + 1
    e = np.ascontiguousarray(edges, np.int64)
    w = np.ascontiguousarray(w2, np.float32)
    out = np.empty(n, np.int64)
    nc = ctypes.c_int64(-1)
    _lib.check(lib.hgnn_hdbscan_tree_host(e.ctypes.data, w.ctypes.data, n, mcs, out.ctypes.data, ctypes.byref(nc)),
               "hgnn_hdbscan_tree_host")
    assert np.array_equal(out, cases[name + "/labels"])
    assert nc.value == out.max() + 1
    # the order of equal-weight edges must not matter: reverse every run of equal w2
    order = np.lexsort((-np.arange(n - 1), w))
    e2, w2r = np.ascontiguousarray(e[order]), np.ascontiguousarray(w[order])
    _lib.check(lib.hgnn_hdbscan_tree_host(e2.ctypes.data, w2r.ctypes.data, n, mcs, out.ctypes.data, None),
               "hgnn_hdbscan_tree_host")
    assert np.array_equal(out, cases[name + "/labels"])


def test_host_tree_stage_rejects_a_cycle():
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    e = np.array([[0, 1], [0, 1], [2, 3]], np.int64)
    w = np.array([1, 2, 3], np.float32)
    out = np.empty(4, np.int64)
    assert lib.hgnn_hdbscan_tree_host(e.ctypes.data, w.ctypes.data, 4, 2, out.ctypes.data, None) != 0
    assert b"spanning tree" in lib.hgnn_last_error()
