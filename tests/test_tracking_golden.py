"""CPU: the restatement of the reference's eval_metrics (tests/tracking_ref.py) against the reference's own outputs
pinned in tests/golden/tracking_eval.npz (tests/golden/make_tracking_golden.py)."""
import os

import numpy as np
import pytest

import tracking_ref as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracking_eval.npz")


def load_cases():
    z = np.load(GOLDEN, allow_pickle=False)
    out = []
    for name in z["cases"]:
        d = {k: z[f"{name}/{k}"] for k in ("hit", "cand", "pid", "pt", "primary", "params", "expected", "status")}
        d["name"] = str(name)
        out.append(d)
    return out


CASES = load_cases()


def restate(cs):
    pt_cut, nhits_cut, majority_cut, use_primary = cs["params"]
    return T.track_eval(cs["hit"], cs["cand"], cs["pid"], cs["pt"], cs["primary"] if use_primary else None,
                        float(pt_cut), int(nhits_cut), float(majority_cut))


def check_against_reference(r, cs, rel_means=1e-12):
    status = int(cs["status"])
    if status != 0:           # default_response (1), or the reference raised on an empty / fully filtered B (2)
        assert r["no_match"], cs["name"]
        assert all(r[k] == 0 and type(r[k]) is int for k in T.KEYS)
        return
    assert not r["no_match"], cs["name"]
    e = cs["expected"]
    assert T.same(r["track_eff"], e[0]), (cs["name"], r, e)
    assert T.same(r["track_pur"], e[1]), (cs["name"], r, e)
    assert T.same(r["hit_eff"], e[2], rel_means), (cs["name"], r, e)
    assert T.same(r["hit_pur"], e[3], rel_means), (cs["name"], r, e)


@pytest.mark.parametrize("cs", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_reference(cs):
    check_against_reference(restate(cs), cs)


def test_fixture_covers_the_contract():
    names = {c["name"] for c in CASES}
    for must in ("hash_tie_C6000", "size_filter_fp32_boundary", "pt_cut_fp32_boundary", "duplicates",
                 "pids_40bit_signed", "no_match_mixed", "no_match_after_filter", "zero_truth_nan", "all_filtered",
                 "pt_nan_noise", "pt_nan_mixed"):
        assert must in names
    # NaN pt propagates into ptmin: not reconstructable, neither in the mask nor in n_truth
    noise = next(c for c in CASES if c["name"] == "pt_nan_noise")
    sel = noise["pid"] == 0
    assert sel.sum() >= noise["params"][1] and np.isnan(noise["pt"][sel]).all()
    assert not np.isnan(noise["pt"][~sel]).any()
    finite = dict(noise, pt=np.where(sel, np.float32(5.0), noise["pt"]))
    assert restate(finite)["n_truth"] == restate(noise)["n_truth"] + 1
    assert restate(finite)["track_eff"] != restate(noise)["track_eff"] == noise["expected"][0]
    mixed = next(c for c in CASES if c["name"] == "pt_nan_mixed")
    assert np.isnan(mixed["pt"]).sum() == 1 and int(mixed["status"]) == 0
    r = restate(mixed)
    assert (r["n_kept"], r["n_mask"], r["n_truth"], r["hit_eff"]) == (3, 1, 1, 1.0)
    assert restate(dict(mixed, pt=np.nan_to_num(mixed["pt"], nan=2.0)))["hit_eff"] == (6 / 8 + 1) / 2
    tie = restate(next(c for c in CASES if c["name"] == "hash_tie_C6000"))
    assert tie["track_eff"] == 2.0 and tie["n_kept"] == 2
    assert np.isnan(restate(next(c for c in CASES if c["name"] == "zero_truth_nan"))["track_eff"])
    assert any(c["params"][3] == 1 for c in CASES) and any(c["params"][2] == 0.75 for c in CASES)
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("C", [1, 2, 3, 7, 100, 4505, 4506, 6000, 10_000, 123_457])
def test_cluster_hash_is_numpy_linspace(C):
    assert np.array_equal(T.cluster_hash(C), np.linspace(1, 1 + 1e-12, C))


def test_hash_has_4505_distinct_values():
    assert np.unique(T.cluster_hash(20_000)).size == 4505
    assert (1 + 1e-12) - 1.0 == 1.000088900582341e-12
