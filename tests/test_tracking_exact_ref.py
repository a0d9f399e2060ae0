"""CPU: the cases of tests/tracking_exact_cases.py are proved here, and shown not to be vacuous.  No GPU.

1. Exactness.  Every term n / col and n / nhits that enters one of the two means is dyadic with a denominator of at
   most 2^9 and there are fewer than 2^20 of them, so each sum is exact in float64 in any order; the restatement's
   means are the one correctly rounded quotient of that exact sum and the count.
2. Shuffling the pairs and renumbering the hits leaves every entry of the restatement's result unchanged, bit for
   bit: the expectation does not depend on an order the kernel is free to choose.
3. The sizes on the launch edges are present.
4. Mutants of the restatement (tracking_ref.MUTANTS): each must change the result of every case built for it
   (``MUST_MOVE``).  tie_low is listed for edge_split_even only: in the ``spread_*_ties`` cases the lower label
   would give the same counts and the same term n / col = 1, what those cases pin is that exactly ONE of up to 129
   tied candidates matches."""
from fractions import Fraction

import numpy as np
import pytest

import tracking_exact_cases as X
import tracking_ref as T

MUST_MOVE = {
    "size_gt": ("edge_size_eq",), "col_gt": ("edge_col_eq",), "row_gt": ("edge_row_eq",),
    "kept_ge": ("edge_kept_eq", "edge_size_eq"), "pt_ge": ("edge_pt_eq",), "nhits_gt": ("edge_nhits_eq",),
    "tie_low": ("edge_split_even",), "dup_once": ("edge_duplicates",), "size_f64": ("edge_size_f32",),
}
MODES = (False, True)


def _bits(r):
    return {k: np.float64(v).view(np.uint64) if not isinstance(v, bool) else v for k, v in r.items()}


def _exact_sum(t):
    return sum((Fraction(int(n), int(d)) for n, d in t), Fraction(0))


@pytest.mark.parametrize("name", X.NAMES)
def test_terms_are_dyadic_and_the_means_exact(name):
    c = X.CASES[name]
    for use_primary in MODES:
        pur, eff = X.terms(c, use_primary)
        r = X.restate(c, use_primary)
        for t in (pur, eff):
            assert len(t) < 2 ** 20
            for n, d in t:
                den = Fraction(int(n), int(d)).denominator
                assert den & (den - 1) == 0 and den <= 2 ** 9, (name, n, d)
        if r["no_match"]:
            assert len(pur) == 0 or r["n_kept"] == 0
            continue
        assert r["n_kept"] == len(pur) and r["n_mask"] == len(eff)
        s_pur, s_eff = _exact_sum(pur), _exact_sum(eff)
        assert Fraction(float(s_pur)) == s_pur and Fraction(float(s_eff)) == s_eff
        with np.errstate(all="ignore"):
            assert T.same(r["hit_pur"], np.float64(float(s_pur)) / np.float64(len(pur)))
            assert T.same(r["hit_eff"], np.float64(float(s_eff)) / np.float64(len(eff)))


@pytest.mark.parametrize("name", X.NAMES)
def test_restatement_does_not_depend_on_pair_or_hit_order(name):
    c = X.CASES[name]
    rng = np.random.default_rng(len(name))
    for use_primary in MODES:
        want = _bits(X.restate(c, use_primary))
        order = rng.permutation(c["hit"].size)
        assert _bits(X.restate(c, use_primary, hit=c["hit"][order], cand=c["cand"][order])) == want
        new = rng.permutation(c["pid"].size)
        moved = {k: np.empty_like(c[k]) for k in ("pid", "pt", "primary")}
        for k in moved:
            moved[k][new] = c[k]
        hit = new[c["hit"]] if c["hit"].size else c["hit"]
        assert _bits(X.restate(c, use_primary, hit=hit, **moved)) == want


def test_the_sizes_are_the_ones_the_launch_geometry_asks_for():
    for b in X.B_SIZES:
        for n in X.N_SIZES:
            c = X.CASES[f"fill_b{b}_n{n}"]
            assert c["hit"].size == b and c["pid"].size == n
    fills = [c for c in X.CASES.values() if c["family"] == "fill"]
    assert any((c["pid"] == 0).any() for c in fills) and any(not (c["pid"] == 0).any() for c in fills)
    assert any(c["pid"].min() < 0 and c["pid"].max() > 1 << 40 for c in fills)
    assert any(c["cand"].min() < 0 and c["cand"].max() > 1 << 40 for c in fills)
    for n in X.WAVE_SIZES:
        for w in ("lowpt", "prim"):
            c = X.CASES[f"hits_{n}_{w}"]
            assert (c["pid"] == -77).sum() == n
            last = np.flatnonzero(c["pid"] == -77)[-1]
            if w == "lowpt":          # reconstructable but for its last hit: moves n_truth
                assert c["pt"][last] < c["pt_cut"] and (c["pt"][c["pid"] == -77][:-1] > c["pt_cut"]).all()
            else:
                assert c["primary"][last] == 1 and c["primary"][c["pid"] == -77].sum() == 1
        c = X.CASES[f"spread_{n}_big"]
        assert len(np.unique(c["cand"][np.isin(c["hit"], np.flatnonzero(c["pid"] == 31))])) == n
        r = X.restate(X.CASES[f"spread_{n}_ties"], False)
        assert r["n_cand"] == n + 3 and r["n_match"] == 1 + 3
    for p in X.P_SIZES:
        c = X.CASES[f"parts_{p}"]
        assert len(np.unique(c["pid"])) == p and np.bincount(np.unique(c["pid"], return_inverse=True)[1]).max() == 2
    assert X.restate(X.CASES["edge_c_eq_1"], False)["n_cand"] == 1
    r = X.restate(X.CASES["edge_all_filtered"], False)
    assert r["no_match"] and r["n_cand"] == 0 and X.CASES["edge_all_filtered"]["hit"].size == 8
    assert X.CASES["edge_no_pairs"]["hit"].size == 0 and X.CASES["edge_no_pairs"]["pid"].size > 0
    assert X.CASES["edge_no_pairs_no_hits"]["pid"].size == 0
    c = X.CASES["edge_size_f32"]
    thr = c["nhits_cut"] * c["majority_cut"]
    assert thr > 16 and np.float32(thr) == 16
    dup = X.CASES["edge_duplicates"]
    assert len(np.unique(np.stack([dup["hit"], dup["cand"]], 1), axis=0)) < dup["hit"].size
    # most cases give metrics, some the default response, with and without primary
    for use_primary in MODES:
        nm = [X.restate(c, use_primary)["no_match"] for c in X.CASES.values()]
        assert 10 <= sum(nm) <= len(nm) // 2


def test_boundary_cases_sit_on_their_comparison():
    def r(name, **kw):
        return X.restate(X.CASES[name], False, **kw)
    base = r("edge_nhits_eq")
    assert base["n_truth"] == 4 and base["n_mask"] == 4                 # three background particles and the fourth
    assert r("edge_pt_eq")["n_truth"] == 3 and r("edge_pt_eq")["n_kept"] == 4
    assert r("edge_size_eq")["n_cand"] == 4 and r("edge_size_eq")["n_match"] == 4 and r("edge_size_eq")["n_kept"] == 3
    assert r("edge_col_eq")["n_kept"] == 4 and r("edge_row_eq")["n_kept"] == 4
    assert r("edge_kept_eq")["n_match"] == 4 and r("edge_kept_eq")["n_kept"] == 3
    s = r("edge_split_even")
    assert s["n_cand"] == 5 and s["n_match"] == 4 and s["hit_pur"] == (3 + 0.5) / 4
    d = r("edge_duplicates")
    assert d["n_cand"] == 5 and d["n_kept"] == 4 and d["hit_eff"] == (3 + 1.5) / 4
    for name in ("edge_nan_lane_loop", "edge_nan_wave_merge", "edge_nan_first", "edge_nan_all"):
        x = r(name)
        assert x["n_kept"] == 4 and x["n_mask"] == 3 and x["n_truth"] == 3 + (63 if "all" not in name else 0), name


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_mutant_moves_every_case_built_for_it(mutant):
    assert set(MUST_MOVE) == set(T.MUTANTS)
    for name in MUST_MOVE[mutant]:
        c = X.CASES[name]
        assert _bits(X.restate(c, False, mutant=mutant)) != _bits(X.restate(c, False)), (mutant, name)
