"""CPU: the cases of tests/hdbscan_exact_cases.py are proved here, and shown not to be vacuous.  No GPU.

1. Conditions on the inputs (not tolerances: when one fails the input changes, not the condition): every coordinate
   on the grid, every EOM decision of the restatement with a float64 margin above 1e-9 relative (or no decision at
   all), labels that are not all noise for at least one case of every KP, zero-weight edges in the duplicate cases,
   every (KP, DP) instantiation and the slice layouts at N = 4096 and 4097 reached by ``TABLE``.
2. The library's host tree stage (hgnn_hdbscan_tree_host) returns the restatement's labels on the restatement's MST
   for every case, the duplicate ones (lambda = HGNN_HDBSCAN_LAMBDA_DUP, zero-weight multi-way levels) included.
3. Mutants of the restatement (hdbscan_ref.MUTANTS).  ``MUST_MOVE`` names, per mutant, the cases whose core2, MST
   or labels it has to change; a mutant that leaves one of them alone fails.

     rank_lo       rank k-2: every case with min_samples >= 2 but dup_two_locations (both locations hold at least
                   min_samples points, so ranks k-2 and k-1 are both the distance 0)
     rank_hi       rank k: every case with min_samples < N
     last_point    the point N-1 never a candidate: every case (the D = 1 lattice ends with an end point and
                   dup_two_locations with a point of the 5-point location for this)
     last_slice    the last candidate slice never offered, restated as the MST of the graph without the edges whose
                   two ends both lie in that slice (an edge is offered from either end): the cases whose last slice
                   holds both ends of an MST edge: N = 511, 512, 4096 and the two track-like duplicate cases.  With
                   a one-point last slice (257, 513, 4097) this graph loses no edge.  A Boruvka kernel that skips
                   the slice loses more than this restatement (an edge seen only from its far end serves the far
                   component, not the near one): run on the GPU, such a kernel also failed edge_n513 and seven of
                   the N = 257 grid cases (tests/test_gpu_hdbscan_exact.py)
     tie_maxmin    ties ordered by (max, min): the four lattice patches and the two track-like duplicate cases
     binary        every edge its own level: the four lattice patches (a level there joins up to 272 points)
     lambda_denorm lambda(w2 = 0) = 1 / sqrt(2^-149): NO case.  A cluster collects a lambda(0) term only from
                   points that leave it at a zero-weight level, and below such a level there is no further split, so
                   the cluster is a leaf of the condensed tree.  EOM compares the stability of clusters that HAVE
                   children, which therefore never holds such a term, with sums below them: either value of
                   lambda(0) is far above every finite lambda on the grid (at most 128), so no decision and no
                   label can differ.  test_lambda_of_duplicates_cannot_show_in_labels pins this; what the duplicate
                   cases do check is item 2 above."""
import ctypes

import numpy as np
import pytest

import hdbscan_exact_cases as X
import hdbscan_ref as R

PATCHES = tuple(n for n in X.NAMES if X.CASES[n]["family"] == "patch")
DUP_TRACKS = ("dup_mcs5_ms5", "dup_mcs4_ms3")
SMALL = tuple(n for n in X.NAMES if len(X.CASES[n]["q"]) <= 1000)
MUST_MOVE = {
    "rank_lo": tuple(n for n in SMALL if X.CASES[n]["ms"] >= 2 and n != "dup_two_locations"),
    "rank_hi": tuple(n for n in SMALL if X.CASES[n]["ms"] < len(X.CASES[n]["q"])),
    "last_point": SMALL,
    "last_slice": ("edge_n511", "edge_n512", "edge_n4096") + DUP_TRACKS,
    "tie_maxmin": PATCHES + DUP_TRACKS,
    "binary": PATCHES,
    "lambda_denorm": (),
}


def test_inputs_are_on_the_grid():
    for name, c in X.CASES.items():
        q = c["q"]
        assert q.dtype == np.int16 and q.ndim == 2 and np.abs(q).max() <= 128, name
        assert 1 <= q.shape[1] <= 16 and 2 <= c["mcs"] <= len(q) and 1 <= c["ms"] <= len(q), name
        x = X.points(c)
        assert x.dtype == np.float32 and np.array_equal(x.astype(np.float64) * 128, q), name
        if c["family"] != "dup":
            assert len(np.unique(q, axis=0)) == len(q), name


def test_the_cases_are_the_ones_the_launch_geometry_asks_for():
    t = X.TABLE
    assert {v[:2] for v in t.values()} >= {(kp, dp) for kp in (8, 16, 32, 64, 128) for dp in (4, 8, 16)}
    for d in X.DIMS:
        for ms in X.MIN_SAMPLES:
            c = X.CASES[f"grid_d{d}_ms{ms}"]
            assert c["q"].shape == (X.N_GRID, d) and c["ms"] == ms
    assert np.array_equal(np.sort(X.CASES["grid_d1_ms8"]["q"][:, 0]), np.arange(-128, 129))
    for ms in (8, 9, 128):
        assert len(X.CASES[f"n_eq_ms{ms}"]["q"]) == ms == X.CASES[f"n_eq_ms{ms}"]["ms"]
    for ms in (1, 2):
        c = X.CASES[f"n2_ms{ms}"]
        assert len(c["q"]) == 2 and c["mcs"] == 2 and c["ms"] == ms
    for n in X.EDGE_N:
        c = X.CASES[f"edge_n{n}"]
        assert c["q"].shape == (n, 8) and (c["mcs"], c["ms"]) == (5, 5)
    # hdb_layout: 16 full slices of 256 at 4096; 9 slices of 512 with a one-point last slice at 4097
    assert t["edge_n4096"][2:] == (16, 256) and t["edge_n4097"][2:] == (9, 512) and 4097 - 8 * 512 == 1
    assert t["edge_n255"][2:] == t["edge_n256"][2:] == (1, 256) and t["edge_n257"][2:] == (2, 256)
    assert t["edge_n512"][2:] == (2, 256) and t["edge_n513"][2:] == (3, 256)
    assert (X.CASES["dup_mcs5_ms5"]["mcs"], X.CASES["dup_mcs5_ms5"]["ms"]) == (5, 5)
    assert (X.CASES["dup_mcs4_ms3"]["mcs"], X.CASES["dup_mcs4_ms3"]["ms"]) == (4, 3)
    assert len(np.unique(X.CASES["dup_two_locations"]["q"], axis=0)) == 2
    for name in DUP_TRACKS:
        c = X.CASES[name]
        _, cnt = np.unique(c["q"], axis=0, return_counts=True)
        assert (cnt == 7).sum() >= 6 and (cnt == 2).sum() >= 10 and c["ms"] in cnt
    assert len(X.CASES["patch_16x16_ms1"]["q"]) == 256 and len(X.CASES["patch_17x16_ms5"]["q"]) == 272
    for name in PATCHES:
        q = X.CASES[name]["q"]
        assert q.shape[1] == 4 and not q[:, 2:].any() and (np.diff(np.unique(q[:, 0])) == 2).all()


def test_every_eom_decision_has_a_margin_and_every_kp_a_cluster():
    has_cluster = set()
    for name in X.NAMES:
        labels, edges, w2, c2, info = X.reference(name)
        m = info["eom_margin"]
        assert m > 1e-9 or np.isinf(m), (name, m)
        assert np.isfinite(w2).all() and np.isfinite(c2).all() and (w2[1:] >= w2[:-1]).all()
        if labels.max() >= 0:
            has_cluster.add(X.TABLE[name][0])
            assert np.bincount(labels[labels >= 0]).min() >= X.CASES[name]["mcs"]
    assert has_cluster == {8, 16, 32, 64, 128}


def test_duplicate_cases_have_zero_weight_edges():
    for name in DUP_TRACKS:
        w2 = X.reference(name)[2]
        assert 30 <= (w2 == 0).sum() < len(w2) // 2, name          # 6 groups of 7 and one of min_samples
    labels, _, w2, c2, _ = X.reference("dup_two_locations")
    assert (w2 == 0).sum() == len(w2) - 1 and w2[-1] > 0 and not c2.any()
    assert labels.min() == 0 and labels.max() == 1
    for name in PATCHES:                                            # at most a handful of distinct levels
        assert len(np.unique(X.reference(name)[2])) <= 4, name


@pytest.mark.parametrize("name", X.NAMES)
def test_host_tree_stage_gives_the_restatement_labels(name):
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    labels, edges, w2, _, _ = X.reference(name)
    n = len(labels)
    e, w = np.ascontiguousarray(edges, np.int64), np.ascontiguousarray(w2, np.float32)
    out = np.full(n, -7, np.int64)
    nc = ctypes.c_int64(-1)
    _lib.check(lib.hgnn_hdbscan_tree_host(e.ctypes.data, w.ctypes.data, n, X.CASES[name]["mcs"], out.ctypes.data,
                                          ctypes.byref(nc)), "hgnn_hdbscan_tree_host")
    assert np.array_equal(out, labels) and nc.value == labels.max() + 1


def _moved(name, mutant):
    c = X.CASES[name]
    want = X.reference(name)
    got = R.hdbscan(X.points(c), c["mcs"], c["ms"], return_all=True, mutant=mutant)
    return [k for k, a, b in zip(("labels", "edges", "w2", "core2"), got, want) if not np.array_equal(a, b)]


@pytest.mark.parametrize("mutant", [m for m in R.MUTANTS if MUST_MOVE[m]])
def test_mutant_moves_every_case_it_is_listed_for(mutant):
    assert set(MUST_MOVE) == set(R.MUTANTS)
    still = [name for name in MUST_MOVE[mutant] if not _moved(name, mutant)]
    assert not still, f"{mutant} changes nothing of {still}"


def test_lambda_of_duplicates_cannot_show_in_labels():
    for name in DUP_TRACKS + ("dup_two_locations",):
        assert _moved(name, "lambda_denorm") == []
