"""CPU: the restatement of hgnn_track_records (tests/tracking_records_ref.py) agrees with the scalar restatement
(tests/tracking_ref.py) on every exact case, conserves its counts, and the cases can see what the GPU test
(tests/test_gpu_tracking_records.py) relies on them to see: a particle that keeps two matches through a hash
collision, a candidate held by two particles, the slot rule and the NaN-propagating reduction of the variables."""
import numpy as np
import pytest

import tracking_exact_cases as X
import tracking_records_ref as R
import tracking_ref as T

MODES = (False, True)


def _same_scalars(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert type(a[k]) is type(b[k]) and T.same(a[k], b[k]), (k, a[k], b[k])


@pytest.mark.parametrize("name", X.NAMES)
def test_scalars_equal_the_scalar_restatement(name):
    c = X.CASES[name]
    for use_primary in MODES:
        _same_scalars(R.restate(c, use_primary)["scalars"], X.restate(c, use_primary))


@pytest.mark.parametrize("name", R.NAMES)
def test_conservation_sums(name):
    c = R.CASES[name]
    for use_primary in MODES:
        r = R.restate(c, use_primary)
        t, p, k = r["totals"], r["particles"], r["candidates"]
        want = [t["n_part"], t["n_truth"], t["n_kept"], t["n_mask"]]
        assert [p["pid"].size, int(p["reconstructable"].sum()), int(p["n_kept"].sum()), int(p["n_mask"].sum())] == want
        assert int(p["n_match"].sum()) == t["n_match"] and k["label"].size == t["n_cand"]
        assert int(k["n_kept"].sum()) == t["n_kept"] and int(k["n_mask"].sum()) == t["n_mask"]
        for v in range(r["hist"].shape[0]):
            assert r["hist"][v].sum(0)[:4].tolist() == want, (name, v)
        # the scalars' counts are the tables' sums wherever the scalar restatement defines them
        s = r["scalars"]
        assert (s["n_part"], s["n_cand"], s["n_kept"]) == (t["n_part"], t["n_cand"], t["n_kept"] * (not s["no_match"]))
        if not s["no_match"]:
            assert (s["n_mask"], s["n_truth"], s["n_match"]) == (t["n_mask"], t["n_truth"], t["n_match"])
        # a particle's pointer names a candidate that counts it, and the other way round
        has = p["cand_index"] >= 0
        assert np.array_equal(has, p["n_kept"] > 0) and np.all(k["n_kept"][p["cand_index"][has]] > 0)
        assert np.all(p["shared"][has] <= k["size"][p["cand_index"][has]]) and np.all(p["shared"][has] > 0)
        assert np.all(p["shared"][~has] == 0)
        held = k["particle"] >= 0
        assert np.array_equal(held, k["n_kept"] > 0) and np.all(p["n_kept"][k["particle"][held]] > 0)
        assert np.all(k["shared"][~held] == 0)


def test_hash_collision_keeps_two_matches_of_one_particle():
    c = R.EXTRA["records_hash_collision"]
    h = T.cluster_hash(8193)
    assert h[c["c0"]] == h[c["c0"] + 1] and c["c0"] + 1 < 8192
    for use_primary in MODES:
        r = R.restate(c, use_primary)
        assert r["totals"]["n_cand"] == 8193 and np.all(r["candidates"]["n_kept"] == 1)    # every candidate kept
        p = r["particles"]
        row = int(np.flatnonzero(p["pid"] == c["split_pid"])[0])
        assert p["nhits"][row] == 4 and p["n_match"][row] == 2 and p["n_kept"][row] == 2
        assert p["cand_index"][row] == c["c0"] and p["shared"][row] == 2
        assert np.all(np.delete(p["n_kept"], row) == 1)
        assert r["totals"]["n_kept"] == p["pid"].size + 1
        assert [int(r["candidates"]["particle"][c["c0"] + j]) for j in (0, 1)] == [row, row]
        # the scalar restatement counts both too: the records only say where
        _same_scalars(r["scalars"], X.restate(c, use_primary))


def test_two_particles_share_one_candidate():
    c = R.EXTRA["records_shared_candidate"]
    for use_primary in MODES:
        r = R.restate(c, use_primary)
        k, p = r["candidates"], r["particles"]
        col = int(np.flatnonzero(k["label"] == c["label"])[0])
        rows = sorted(int(np.flatnonzero(p["pid"] == q)[0]) for q in c["pids"])
        assert k["size"][col] == 4 and k["n_kept"][col] == 2 and k["particle"][col] == rows[0]
        assert k["shared"][col] == 2
        assert [int(p["cand_index"][q]) for q in rows] == [col, col]
        _same_scalars(r["scalars"], X.restate(c, use_primary))


def _differs(a, b):
    if not np.array_equal(a["hist"], b["hist"]):
        return True
    x, y = a["particles"]["values"], b["particles"]["values"]
    return not np.array_equal(x.view(np.uint32) * ~np.isnan(x), y.view(np.uint32) * ~np.isnan(y)) or \
        not np.array_equal(np.isnan(x), np.isnan(y))


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_cases_see_the_mutants(mutant):
    seen = [n for n in R.NAMES if _differs(R.restate(R.CASES[n], False), R.restate(R.CASES[n], False, mutant=mutant))]
    assert seen, f"no case tells {mutant} from the contract"
    # and the unmutated parts stay what they were
    n = seen[0]
    a, b = R.restate(R.CASES[n], False), R.restate(R.CASES[n], False, mutant=mutant)
    assert a["totals"] == b["totals"] and all(np.array_equal(a["candidates"][k], b["candidates"][k])
                                              for k in a["candidates"])


def test_slot_rule_on_values():
    """the slot rule, spelled out: on an edge goes up, -0.0 equals a 0.0 edge, a NaN and +inf overflow"""
    e = np.float32([0.0, 1.0, 2.0])
    x = np.float32([-1.0, -0.0, 0.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 1.0, 2.0, np.inf, -np.inf,
                    np.nan, 1e-45])
    assert np.searchsorted(e, x, "right").tolist() == [0, 1, 1, 1, 2, 3, 3, 0, 3, 1]
