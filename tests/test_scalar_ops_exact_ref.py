"""CPU: the references of tests/scalar_ops_exact_ref.py are proved here, and the cases shown not to be vacuous.

1. Representability.  Every named intermediate of the three operators (raw, d, l, x, the coefficients: float32; the
   sums, the mean and the variance: float64) converts to the kernel's type without rounding on the generated cases.
   This is what lets the GPU file compare bits instead of holding a bar.
2. The integer references agree with the float64 restatements the suite already has (pairloss_ref.py, wbce_ref.py,
   graphcon_ref.py) on the same cases.
3. The backward cases of the pair hinge carry the degree census (0, 1, 15, 16, 17, 32, 33 entries and a hub), class
   sums that are powers of two, and terms whose float32 sums are exact in any order.
4. Reference mutants: each one changes at least one asserted quantity on every case it applies to, and applies to at
   least one case of every size family it can apply to.  ``cap_branch_flipped`` applies to none: pt_weighting is
   continuous at the cap (the flipped heaviside multiplies pt - cap = 0), which test_ptw_is_exact_on_the_grid shows;
   ``leak_from_cut`` is the neighbouring mistake that does show."""
from fractions import Fraction

import numpy as np
import pytest

import graphcon_ref as GR
import pairloss_ref as PR
import scalar_ops_exact_ref as X
import wbce_ref as WR

IDS = {np.int32: "i32", np.int64: "i64"}
SMALL = X.FAMILIES[:3]
APPLICABLE = {
    "wbce": {"last_dropped", "group_dropped", "counted_twice", "row_b_early", "keep_ignored", "true_as_false",
             "pt_a_both", "leak_from_cut"},
    "hinge": {"last_dropped", "group_dropped", "counted_twice", "row_b_early", "true_as_false", "leak_from_cut"},
    "attn": {"last_dropped", "counted_twice", "row_b_early"},
}


def _f32_exact(v):
    v = np.asarray(v, np.float64)
    return bool(np.array_equal(v.astype(np.float32).astype(np.float64), v))


@pytest.mark.parametrize("leak", X.LEAKS)
def test_ptw_is_exact_on_the_grid(leak):
    grid = np.concatenate([np.arange(25) / 8.0, [np.nan]]).astype(np.float32)
    got, parts = X.ptw_f32(grid, leak)
    want = X.ptw32(grid, leak)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64) * 32, want)
    for p, w, inter in zip(grid, want, zip(*parts)):              # every intermediate against exact rationals
        q = Fraction(0) if np.isnan(p) else Fraction(float(p))
        x, z = q - Fraction(1, 2), q - 1
        r = min((x if x > 0 else 0) / Fraction(1, 2), 1)
        t1, t2 = Fraction(1, 2) * r, Fraction(leak) * (z if z > 0 else 0)
        assert [Fraction(float(v)) for v in inter] == [x, z, r, t1, t2]
        assert Fraction(1, 2) + t1 + t2 == Fraction(int(w), 32)
    hp = X.hp(leak)
    assert np.array_equal(PR.pt_weighting(grid, hp) * 32, want)  # the float64 restatement, exactly
    # the three branches and both corners are on the grid and in every table
    table = X.pt_table(X.N_NODES, np.random.default_rng(0))
    assert table[2] == 0.5 and table[3] == 1.0 and np.isnan(table).any()
    assert (table < 0.5).any() and ((table > 0.5) & (table < 1.0)).any() and (table > 1.0).any()
    # continuity at the cap: the flipped branch is the same function, so no case can tell them apart
    assert np.array_equal(X.ptw32(grid, leak, "cap_branch_flipped"), want)
    if leak:
        assert not np.array_equal(X.ptw32(grid, leak, "leak_from_cut"), want)


def _families(op, families=X.FAMILIES):
    return [pytest.param(idt, fam, id=f"{IDS[idt]}-{fam}") for idt in X.IDTS for fam in families]


@pytest.mark.parametrize("idt,family", _families("wbce"))
def test_wbce_intermediates_are_exact(idt, family):
    f = np.float32
    for c in X.cases("wbce", idt, family):
        r = X.wbce_exact(c)
        t = X.wbce_terms(c, c["scores"])
        assert t["raw32"].max(initial=0) < 2 ** 24 and _f32_exact(t["raw32"] / 32.0), X.name(c)
        s = c["scores"][r["live"]]
        assert np.isin(s, (0.0, 1.0)).all()
        with np.errstate(divide="ignore"):
            for v in (s, f(1) - s):                                   # l = -max(log(v), -100) in float32: 0 or 100
                ell = -np.maximum(np.log(v.astype(f)), f(-100))
                assert np.isin(ell, (0.0, 100.0)).all()
        for k in ("ST32", "SF32", "LT", "LF"):                         # float64 holds every partial sum
            assert r[k] < 2 ** 53
        assert r["ST"] * 32 == r["ST32"] and r["LTf"] * 32 == r["LT"] and r["LFf"] * 32 == r["LF"]
        if c["P"] >= 64:
            want = X.ST_BAD_ID | X.ST_BAD_SCORE
            assert r["status"] == want, X.name(c)
        sq = c["scores_q"][X.wbce_terms(c, c["scores_q"])["live"]]
        assert np.isin(sq, (0, 0.25, 0.5, 0.75, 1)).all() and _f32_exact([c["grad_out"]])
        assert np.log2(c["grad_out"]) % 1 == 0


@pytest.mark.parametrize("idt,family", _families("wbce", SMALL))
def test_wbce_reference_agrees_with_the_float64_restatement(idt, family):
    for c in X.cases("wbce", idt, family):
        if c["P"] == 0:
            continue
        r = X.wbce_exact(c)
        live = r["live"]
        g = np.asarray(c["graph"]).astype(np.int64)[:, live]
        for scores, exact in ((c["scores"], True), (c["scores_q"], False)):
            live_q = X.wbce_terms(c, scores)["live"]
            assert np.array_equal(live_q, live)                        # both score arrays plant the same pairs
            loss, grad, _, (st, sf) = WR.weighted_bce(scores[live], g, c["y"][live], c["pt_a"], c["hp"],
                                                      pt_b=c["pt_b"], combine=c["combine"])
            assert (st, sf) == (r["ST"], r["SF"]), X.name(c)
            if exact:
                assert abs(loss - r["LOSS"]) <= 1e-12 * abs(r["LOSS"]), X.name(c)
            else:
                mine = X.wbce_grad_f32(c, r["KT"], r["KF"])
                assert not mine[~live].any()
                ref = grad * c["grad_out"]
                assert np.abs(mine[live] - ref).max(initial=0) <= 1e-6 * np.abs(ref).max(initial=1e-30), X.name(c)


@pytest.mark.parametrize("idt,family", _families("hinge"))
def test_hinge_intermediates_are_exact(idt, family):
    f = np.float32
    for c in X.cases("hinge", idt, family):
        assert np.abs(c["pts"]).max() <= 3 and np.array_equal(c["E"], c["pts"])
        t = X.hinge_terms(c)
        r = X.hinge_exact(c)
        assert r["on_grid"], X.name(c)
        live = t["live"]
        d2, d = t["d2"][live], t["d"][live]
        assert (d2 >= 1).all() and (d2 <= 36 * c["D"]).all() and (d * d == d2).all()
        s = d2.astype(f)                                               # the float32 sum of squares: small integers
        assert np.array_equal(s + f(1e-12), s) and np.array_equal(np.sqrt(s + f(1e-12)), d.astype(f))
        assert _f32_exact(t["raw32"] / 32.0) and _f32_exact(c["scale"] * d) and _f32_exact([c["margin"]])
        assert float(c["margin"]).is_integer() and c["scale"] in (0.5, 1.0, 2.0)
        for k in ("ST32", "SF32", "LT", "LF"):
            assert r[k] < 2 ** 53
        if c["P"] >= 1000:                                             # beyond, inside and exactly on the margin
            gap = (2 * c["margin"] - 2 * c["scale"] * d)[~t["y"][live]]
            assert (gap < 0).any() and (gap > 0).any() and (gap == 0).any(), X.name(c)
            assert r["status"] == 1


@pytest.mark.parametrize("idt,family", _families("hinge", SMALL))
def test_hinge_reference_agrees_with_the_float64_restatement(idt, family):
    for c in X.cases("hinge", idt, family):
        if c["P"] == 0:
            continue
        r = X.hinge_exact(c)
        live = r["live"]
        g = np.asarray(c["graph"]).astype(np.int64)[:, live]
        loss, _, _, _ = PR.pair_hinge(c["E"], g, c["y"][live], c["pt"], c["hp"], margin=c["margin"], scale=c["scale"])
        assert abs(loss - r["LOSS"]) <= 1e-9 * max(abs(r["LOSS"]), 1e-300), (X.name(c), loss, r["LOSS"])
        # off the power-of-two grid the GPU test holds grad_E to the 1e-4 bar against hinge_grad_exact: it is the
        # float64 restatement's gradient
        _, ref, _, _ = PR.pair_hinge(c["E"], g, c["y"][live], c["pt"], c["hp"], margin=c["margin"], scale=c["scale"])
        grad = X.hinge_grad_exact(c, r["KT"], r["KF"])[0]
        assert np.abs(grad - ref * c["grad_out"]).max() <= 1e-9 * max(np.abs(ref).max(), 1e-300), X.name(c)


@pytest.mark.parametrize("idt", X.IDTS, ids=IDS.values())
def test_hinge_backward_cases_census_sums_and_exact_gradient(idt):
    for c in X.backward_cases(idt):
        what = X.name(c)
        r = X.hinge_exact(c)
        t = X.hinge_terms(c)
        assert r["on_grid"] and r["status"] == 0
        for s32 in (r["ST32"], r["SF32"]):                             # each class's raw sum: a power of two
            assert s32 > 0 and s32 & (s32 - 1) == 0, what
        assert np.log2(c["grad_out"]) % 1 == 0
        inside = ~t["y"] & (c["margin"] - c["scale"] * t["d"] > 0)
        assert inside.any() and np.isin(t["d"][inside], (1, 2, 4)).all(), what
        v, _, _ = X.hinge_lists(c)
        deg = np.bincount(v, minlength=c["N"])
        assert sorted(deg[list(c["census"])]) == [1, 15, 16, 17, 32, 33] and deg[c["empty"]] == 0, what
        for node, n in c["census"].items():
            assert deg[node] == n
        assert deg[c["hub"]] == deg.max() > 128, what                  # above both plan chunks of the GPU test
        cf, _ = X.hinge_coef(c, r["KT"], r["KF"])
        assert _f32_exact(cf) and (cf != 0).any()
        assert X.hinge_grad_is_exact(c, r["KT"], r["KF"]), what
        grad, term, _ = X.hinge_grad_exact(c, r["KT"], r["KF"])
        assert _f32_exact(term) and _f32_exact(grad) and not grad[c["empty"]].any()
        _, ref, _, _ = PR.pair_hinge(c["E"], np.asarray(c["graph"]).astype(np.int64), c["y"], c["pt"], c["hp"],
                                     margin=c["margin"], scale=c["scale"])
        ref = ref * c["grad_out"]
        assert np.abs(grad - ref).max() <= 1e-9 * np.abs(ref).max(), what


@pytest.mark.parametrize("idt,family", _families("attn"))
def test_attention_statistics_are_exact(idt, family):
    trained = 0
    for c in X.cases("attn", idt, family):
        r = X.attn_exact(c)
        E = c["P"]
        assert np.abs(r["x"]).max(initial=0) <= 9 * c["D"] and _f32_exact(r["x"])
        a, b = np.asarray(c["graph"]).astype(np.int64)
        live = (a >= 0) & (a < c["Na"]) & (b >= 0) & (b < c["Nb"])
        if E and E <= 4096:                                            # the float32 tree of hgnn_edge_dot_f32
            x32 = GR.dot_f32(c["A"].astype(np.float32), c["B"].astype(np.float32), a[live], b[live])
            assert np.array_equal(x32, r["x"][live].astype(np.float32))
        if not c["training"]:
            continue
        trained += 1
        assert E >= 2 and E & (E - 1) == 0
        mu, m2 = Fraction(r["sx"], E), Fraction(r["sxx"], E)
        var = m2 - mu * mu
        for exact, got in ((mu, r["MEAN"]), (mu * mu, r["MEAN"] * r["MEAN"]), (m2, r["sxx"] / E), (var, r["VAR"])):
            assert Fraction(got) == exact, X.name(c)                   # float64 holds each of them without rounding
        m = Fraction(1, 4)
        assert Fraction(c["momentum"] if c["momentum"] is not None else 1 / (c["nbt"] + 1)) == m
        rm = (1 - m) * Fraction(c["running_mean"]) + m * mu
        assert Fraction(float(rm)) == rm and np.float32(float(rm)) == r["running_mean"]
        unbiased = Fraction(float(var) * E / (E - 1.0))                # ONE float64 division, as the kernel's
        rv = (1 - m) * Fraction(c["running_var"]) + m * unbiased
        assert np.float32(float(rv)) == r["running_var"] and r["nbt"] == c["nbt"] + 1
        if E <= 4096:
            ref = GR.attention_ref(c["A"], c["B"], np.where(live, np.stack([a, b]), 0), c["gamma"], c["beta"],
                                   c["running_mean"], c["running_var"], c["nbt"], c["fn"], c["norm"], True,
                                   momentum=c["momentum"])
            if live.all():
                assert (ref["running_mean"], ref["running_var"], ref["nbt"]) == \
                    (float(r["running_mean"]), float(r["running_var"]), r["nbt"]), X.name(c)
    assert trained, (family, "no training-mode case")


def _moved(c):
    """{mutant: whether it changes an asserted quantity}; the forward's quantities are tried first"""
    fwd, both = X.asserted(c, backward=False), None
    out = {}
    for m in X.MUTANTS:
        if X.applies(m, c):
            out[m] = X.asserted(c, m, backward=False) != fwd
            if not out[m]:
                both = X.asserted(c) if both is None else both
                out[m] = X.asserted(c, m) != both
    return out


@pytest.mark.parametrize("op", X.OPS)
@pytest.mark.parametrize("idt,family", _families(None))
def test_every_mutant_moves_every_case_it_applies_to(op, idt, family):
    seen = set()
    for c in X.cases(op, idt, family):
        moved = _moved(c)
        seen |= set(moved)
        assert all(moved.values()), (X.name(c), [m for m, v in moved.items() if not v])
    want = set(APPLICABLE[op])
    if family == "tiny":
        want.discard("leak_from_cut")                                  # needs a pair with pt between cut and cap
    assert seen == want, (op, family, sorted(want - seen), sorted(seen - want))


@pytest.mark.parametrize("idt", X.IDTS, ids=IDS.values())
def test_every_mutant_moves_the_backward_cases(idt):
    for c in X.backward_cases(idt):
        moved = _moved(c)
        assert {"list_truncated_16", "empty_node_unwritten", "last_dropped", "counted_twice"} <= set(moved)
        assert all(moved.values()), (X.name(c), [m for m, v in moved.items() if not v])


def test_sizes_sit_on_the_launch_edges():
    for idt, vec in X.VEC.items():
        wg = 256 * vec
        assert X.sizes(idt, "workgroup") == (wg - 1, wg, wg + 1)
        assert X.sizes(idt, "two_workgroups") == (2 * wg - 1, 2 * wg + 1)
        assert X.sizes(idt, "trip") == (2048 * wg - 1, 2048 * wg, 2048 * wg + 5)
        assert set(X.sizes(idt, "workgroup", 1)) <= set(X.attention_sizes(idt, "workgroup"))
    assert X.sizes(np.int32, "workgroup") == (1023, 1024, 1025) and X.sizes(np.int64, "workgroup") == (511, 512, 513)
    dims = {c["D"] for idt in X.IDTS for fam in X.FAMILIES for c in X.cases("hinge", idt, fam)}
    assert dims == set(X.DIMS) == {c["D"] for c in X.backward_cases(np.int64)}
