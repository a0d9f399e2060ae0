"""CPU: the restatement of the score-cut scan (tests/trackscan_ref.py) on the cases of tests/trackscan_cases.py.

  * at every cut it equals ``tracking_ref.track_eval`` of the graph filtered INDEPENDENTLY at that cut (components by
    label propagation from scratch, no state carried between cuts), and the integer edge counts counted directly;
  * at most a third of all (case, cut) rows are no_match, so a pass of the GPU test cannot rest on NaN rows;
  * every term n / col and n / nhits that enters one of the two means, at every cut of every case, is dyadic with a
    denominator of at most 2^9 (``tracking_exact_cases.terms``), so the sums are exact in float64 in any order and the
    restatement need not restate the device's reduction tree: rows are compared on bits;
  * every wrong kernel listed in trackscan_ref.MUTANTS fails at least one case.
"""
from fractions import Fraction

import numpy as np
import pytest

import tracking_exact_cases as E
import tracking_ref as T
import trackscan_cases as X
import trackscan_ref as R

MODES = (False, True)


def _components(src, dst, n):
    """(label = smallest vertex id of the component, present) by label propagation until nothing changes"""
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    src, dst = src[ok], dst[ok]
    label = np.arange(n)
    present = np.zeros(n, bool)
    present[src] = present[dst] = True
    while True:
        low = np.minimum(label[src], label[dst])
        new = label.copy()
        np.minimum.at(new, src, low)
        np.minimum.at(new, dst, low)
        if np.array_equal(new, label):
            return label, present
        label = new


def _independent(c, cut, use_primary):
    """what the single-cut functions compute at ``cut``: the pairs and the evaluation"""
    cut = np.float32(cut)
    with np.errstate(invalid="ignore"):
        ok = c["score"] >= cut
    if c["mode"] == "edge":
        if not ok.any():
            ok = ~np.isnan(c["score"])               # score >= -inf
        label, present = _components(c["a"][ok], c["b"][ok], c["inverse_mask"].size)
        v = np.flatnonzero(present)
        hit, cand = c["inverse_mask"][v], label[v]
    else:
        hit, cand = c["a"][ok], c["b"][ok]
        if c["inverse_mask"] is not None:
            hit = c["inverse_mask"][hit]
    with np.errstate(all="ignore"):
        r = T.track_eval(hit, cand, c["pid"], c["pt"], c["primary"] if use_primary else None, c["pt_cut"],
                         c["nhits_cut"], c["majority_cut"])
    return hit, cand, r


@pytest.mark.parametrize("name", X.NAMES)
def test_every_cut_equals_the_independently_filtered_graph(name):
    c = X.CASES[name]
    for use_primary in MODES:
        rows = X.expected(name, use_primary)
        assert len(rows) == len(c["cuts"])
        for t, cut in enumerate(c["cuts"]):
            hit, cand, want = _independent(c, cut, use_primary)
            got = rows[t]
            what = f"{name} primary={use_primary} cut {t} = {cut}"
            assert sorted(zip(got["hit"].tolist(), got["cand"].tolist())) == sorted(zip(hit.tolist(), cand.tolist())), what
            assert got["empty"] == (hit.size == 0), what
            for k in ("no_match", "n_kept", "n_mask", "n_truth", "n_cand", "n_part", "n_match"):
                assert got[k] == want[k], (what, k)
            if not got["empty"]:
                for k in T.KEYS:
                    assert T.same(got[k], want[k]), (what, k)
            with np.errstate(invalid="ignore"):
                ok = c["score"] >= np.float32(cut)
            kept, y = c["keep"] != 0, c["truth"] != 0
            assert (got["n_pass"], got["n_true_pass"], got["n_true"]) == \
                (int((kept & ok).sum()), int((kept & ok & y).sum()), int((kept & y).sum())), what


@pytest.mark.parametrize("name", X.NAMES)
def test_terms_are_dyadic_at_every_cut(name):
    c = X.CASES[name]
    for use_primary in MODES:
        summed = 0
        for r in X.expected(name, use_primary):
            pur, eff = E.terms(dict(c, hit=r["hit"], cand=r["cand"]), use_primary)
            assert r["no_match"] or (r["n_kept"], r["n_mask"]) == (len(pur), len(eff))
            for n, d in list(pur) + list(eff):
                den = Fraction(int(n), int(d)).denominator
                assert den & (den - 1) == 0 and den <= 2 ** 9, (name, n, d)
            summed += len(pur) + len(eff)
        assert summed > 0 or name in ("e_v1_m1_t1", "e_v300_m0_t3", "e_v64_all_nan", "p_b0_t1", "p_b1_t2"), name


def test_matching_happens_in_two_thirds_of_the_rows():
    rows = [r for name in X.NAMES for p in MODES for r in X.expected(name, p)]
    no_match = sum(bool(r["no_match"]) for r in rows)
    assert 3 * no_match <= len(rows), f"{no_match} of {len(rows)} rows are no_match"
    assert any(r["empty"] for r in rows) and any(not r["no_match"] for r in rows)


def _differs(a, b):
    va, ia = R.row_vector(a)
    vb, ib = R.row_vector(b)
    idx = sorted(set(ia) & set(ib))
    return ia != ib or any(not T.same(va[i], vb[i]) for i in idx)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_wrong_kernel_fails_a_case(mutant):
    caught = []
    for name in X.NAMES:
        want = X.expected(name, True)
        got = X.restate(X.CASES[name], True, mutant=mutant)
        if any(_differs(g, w) for g, w in zip(got, want)):
            caught.append(name)
    assert caught, f"mutant {mutant} passes every case"
