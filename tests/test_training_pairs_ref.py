"""CPU: the row-by-row restatement of the pair construction (tests/training_pairs_ref.py) against the reference's own
outputs in tests/golden/embedding_samples.npz and against the restatement of the existing composition
(tests/embedding_ref.py: graph_intersection on the expanded prediction graph)."""
import numpy as np
import pytest

import embedding_ref as R
import training_pairs_ref as TP
from test_embedding_golden import Z


def _fixture_idx(scatter):
    pred = Z["ev/pred"]
    n = Z["ev/pid"].shape[0]
    return TP.idx_from_pairs(pred, n, scatter=np.random.default_rng(3) if scatter else None)


def test_fixture_prediction_graph_is_row_sorted_with_duplicates():
    pred = Z["ev/pred"]
    assert (np.diff(pred[0]) >= 0).all()
    assert np.unique(R._keys(pred)).size < pred.shape[1]                       # duplicate pairs
    idx = _fixture_idx(False)
    assert 1 <= idx.shape[1] <= 128 and np.array_equal(TP.pairs_from_idx(idx), pred)
    sc = _fixture_idx(True)
    assert np.array_equal(TP.pairs_from_idx(sc), pred)
    assert (sc[:, :-1] == -1).any() and not np.array_equal(sc, idx)           # padding inside the rows


@pytest.mark.parametrize("scatter", [False, True], ids=["tail", "scattered"])
@pytest.mark.parametrize("mode", TP.MODES)
def test_restatement_matches_reference_fixture(mode, scatter):
    g, y = TP.training_pairs(_fixture_idx(scatter), Z["ev/modulewise_true_edges"], Z["ev/signal_mask"], Z["ev/pid"],
                             mode)
    assert g.dtype == np.int64 and y.dtype == bool
    assert np.array_equal(g, Z[f"ts/{mode}/graph"]) and np.array_equal(y, Z[f"ts/{mode}/y"])


CASES = [(300, 16, 200, "mixed", "mixed"), (257, 7, 64, "mixed", "mixed"), (100, 1, 40, "mixed", "mixed"),
         (120, 16, 80, "none", "mixed"), (120, 16, 80, "all", "mixed"), (90, 5, 60, "mixed", "one"),
         (90, 5, 60, "mixed", "zero"), (50, 3, 0, "mixed", "mixed"), (1, 4, 8, "all", "zero")]


@pytest.mark.parametrize("mode", TP.MODES)
@pytest.mark.parametrize("n,k,t,signal,pid_kind", CASES)
def test_restatement_equals_the_composition_on_random_cases(n, k, t, signal, pid_kind, mode):
    rng = np.random.default_rng(1000 * n + 10 * k + t)
    idx, mte, sm, pid = TP.random_case(rng, n, k, t, signal, pid_kind)
    g, y = TP.training_pairs(idx, mte, sm, pid, mode)
    rg, ry = R.training_samples(TP.pairs_from_idx(idx), mte, sm, pid, mode)
    assert np.array_equal(g, rg) and np.array_equal(y, ry)
    if mode == "pid_true_edges":
        assert not y.any()
    if n >= 90 and signal != "none" and t > 0:
        eb = TP.e_bidir(mte, sm)
        assert eb.shape[1] > 0 and (mode == "pid_true_edges" or y.sum() == eb.shape[1])


def test_random_cases_cover_the_contract():
    rng = np.random.default_rng(11)
    idx, mte, sm, pid = TP.random_case(rng, 300, 16, 200)
    rows = np.arange(300)[:, None]
    assert ((idx == rows).sum(1) > 0).any()                                    # self pairs
    assert any(np.unique(r[r >= 0]).size < (r >= 0).sum() for r in idx)        # in-row duplicates
    assert (idx[1] == -1).all() and (idx[:, 0] == -1).any() and (idx[:, -1] >= 0).any()
    assert (pid == 0).any() and (mte[0] == mte[1]).any()
    assert np.unique(R._keys(mte)).size < mte.shape[1]                         # duplicate truth columns
    assert np.isin(R._keys(mte[::-1]), R._keys(mte)).any()                     # a pair in both directions
    # truth pairs that rows hold: the modulewise membership test has work to do
    assert np.isin(R._keys(TP.pairs_from_idx(idx)), R._keys(TP.e_bidir(mte, sm))).any()


def test_skip_bad_treats_bad_ids_as_empty():
    rng = np.random.default_rng(5)
    idx, mte, sm, pid = TP.random_case(rng, 40, 6, 20)
    bad_idx, bad_mte = idx.copy(), mte.copy()
    idx[3, 2], bad_idx[3, 2] = -1, 40
    idx[5, 0], bad_idx[5, 0] = -1, -2
    bad_mte = np.concatenate([mte[:, :4], [[40], [1]], mte[:, 4:]], 1)
    for mode in TP.MODES:
        a = TP.training_pairs(bad_idx, bad_mte, sm, pid, mode, skip_bad=True)
        b = TP.training_pairs(idx, mte, sm, pid, mode)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
