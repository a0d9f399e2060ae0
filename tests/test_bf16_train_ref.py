"""CPU proof of tests/bf16_train_ref.py, the mirror tests/test_gpu_bf16_train_mirror.py holds the bf16 training route to.
Here the dumps z_l come from the float64 forward, rounded to bf16.

  1  the mirror WITHOUT roundings equals float64 torch autograd through torch.nn modules to 1e-12, on every case: it is
     the right derivative;
  2  the bars: the float32 emulation (both summation orders) stays within HALF of each of the three class bars on every
     case, forward and backward; the normwise parameter bar is within the cap BF16_GRAD / 10; dgamma, dbeta and dbias
     of the last layer stay within half of ln_ref.F32_BAR.  The worst figure per class and the case that set it are printed;
     each bar is held to its figure from both sides (worst <= bar / 2 <= 1.05 worst); dgamma / dbeta of every layer and
     the last dbias are held to ln_ref.F32_BAR per (case, quantity) wherever both emulation orders stay within half of it,
     and the table of those that do not (bf16_train_ref.CLASS_BAR_QUANTS) is asserted;
  3  every mutant of the mirror exceeds a bar by a factor of at least 2 on every case where its branch is live, and
     every mutant is live somewhere; "bias from the rounded against the unrounded rows" is nowhere twice a bar, hence no mutant;
  4  the case table reaches every branch of fused._FusedMLPTrainBf16._backward (from widths and switches alone).
"""
import functools

import pytest
import torch

import bf16_train_ref as T
import ln_ref as R


@functools.lru_cache(maxsize=None)
def _rounded(name):
    """(case, flags, forward mirror out, dumps, upstream gradient, mirror params, mirror rows) with every rounding on"""
    case = T.build(name)
    flags = T.fused_flags(case)
    out, zs, _ = T.forward_mirror(case)
    g = T.grad_out(case, zs)
    P, rows = T.mirror(case, zs, g, flags)
    return case, flags, out, zs, g, P, rows


# -------------------------------------------------------------------------------------------------- 1. the derivative
@pytest.mark.parametrize("name", T.CASES)
def test_mirror_without_roundings_is_float64_autograd(name):
    case = T.build(name)
    _, _, zhat = T.forward_mirror(case, rounding=False, kernel_gelu=False)
    g = T.grad_out(case, zhat)
    P, rows, zs = T.autograd64(case, g)
    for a, b in zip(zs, zhat):
        assert R.rel_err(a.numpy(), b.numpy()) <= 1e-12
    mP, mrows = T.mirror(case, zs, g, T.fused_flags(case), rounding=False)
    assert set(mP) == set(P) and set(mrows) == set(rows), (sorted(mrows), sorted(rows))
    for k in P:
        assert R.rel_err(mP[k].numpy(), P[k].numpy()) <= 1e-12, k
    for k in rows:
        assert R.rel_err(mrows[k][0].numpy(), rows[k].numpy()) <= 1e-12, k
        assert bool((mrows[k][1] >= mrows[k][0].abs() * (1 - 1e-12)).all()), f"{k}: scale below |ref|"
    for k in ("T", "U", "D", "S"):              # a tensor that takes no part or needs no gradient has none
        used = any(k == kk for kk, _ in case["segs"]) or case["skip"] == k
        assert (f"d{k}" in mrows) == (used and T.needs_grad(case, k)), k


# ---------------------------------------------------------------------------------------------------------- 2. the bars
def test_bars_and_cap():
    assert T.P_NORM_BAR <= T.P_NORM_CAP == pytest.approx(3e-3)
    from test_gpu_bf16_train import BF16_GRAD
    assert T.P_NORM_CAP == pytest.approx(BF16_GRAD / 10)
    assert T.F32_BAR == 1e-4


_worst = {}


@functools.lru_cache(maxsize=None)
def _emulated(name):
    """[(order, quantity, measure, value, bar)] of the emulation against the mirror, forward and backward"""
    case, flags, out, zs, g, P, rows = _rounded(name)
    res = []
    for order in ("fwd", "rev"):
        eP, erows = T.emulate(case, zs, g, flags, order)
        eo, ezs = T.emulate_forward(case, order)
        res += [(order,) + t for t in T.compare(case, eP, erows, P, rows) + T.compare_forward(eo, ezs, out, zs)]
    return res


def test_bars_are_twice_the_emulations_worst():
    """worst <= bar / 2 <= 1.05 worst for each class bar: not looser than the figure behind it either"""
    worst = {"rel": 0.0, "elem": 0.0, "excess": 0.0}
    for name in T.CASES:
        for order, q, m, v, bar in _emulated(name):
            if bar != T.F32_BAR:
                worst[m] = max(worst[m], v)
    print("\nWORST " + " ".join(f"{k} {v:.4e}" for k, v in worst.items()))
    for m, bar in (("rel", T.P_NORM_BAR), ("elem", T.P_ELEM_BAR), ("excess", T.D_ROW_BAR)):
        assert worst[m] <= bar / 2 <= 1.05 * worst[m], (m, worst[m], bar)


def test_f32_held_split():
    """per (case, quantity): dgamma / dbeta of every layer and the last dbias are held to F32_BAR exactly where both
    emulation orders stay within half of it; the others are the table CLASS_BAR_QUANTS"""
    fell = {}
    for name in T.CASES:
        case = T.build(name)
        worst = {}
        for order, q, m, v, bar in _emulated(name):
            if m == "rel" and T.f32_candidate(case, q):
                worst[q] = max(worst.get(q, 0.0), v)
        assert set(worst) == {f"L{l}.{k}" for l in range(case["n"]) for k in ("dgamma", "dbeta")} | {f"L{case['n'] - 1}.db"}
        out = tuple(sorted(q for q, v in worst.items() if not v <= T.F32_BAR / 2))
        if out:
            fell[name] = out
    assert fell == {k: tuple(sorted(v)) for k, v in T.CLASS_BAR_QUANTS.items()}, fell


@pytest.mark.parametrize("name", T.CASES)
def test_emulation_within_half_of_every_bar(name):
    lines, bad = [], []
    for order, q, m, v, bar in _emulated(name):
        cls = "f32" if bar == T.F32_BAR else m
        lines.append(f"EMUL {name} {order} {q}.{m} {v:.3g} / {bar:.3g} = {v / bar:.3f}")
        if not v <= bar / 2:
            bad.append(lines[-1])
        if v > _worst.get(cls, (-1.0,))[0]:
            _worst[cls] = (v, name, q, order)
    print("\n" + "\n".join(lines))
    print("WORST SO FAR " + "; ".join(f"{k}: {v[0]:.3e} ({v[1]}, {v[2]}, {v[3]})" for k, v in sorted(_worst.items())))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------- 3. mutants
def _exceeds(case, mP, mrows, P, rows):
    """worst value / bar of a mutant's quantities against the mirror (a quantity the mutant does not even produce counts
    as infinitely wrong)"""
    if set(mP) != set(P) or set(mrows) != set(rows):
        return float("inf"), "missing"
    got_rows = {k: v[0].numpy() for k, v in mrows.items()}
    got_P = {k: v.numpy() for k, v in mP.items()}
    return max((v / bar, f"{q}.{m}") for q, m, v, bar in T.compare(case, got_P, got_rows, P, rows))


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_mutants_exceed_a_bar_twofold_wherever_live(mutant):
    live = [n for n in T.CASES if T.mutant_live(T.build(n), mutant, _rounded(n)[4])]
    assert live, f"{mutant}: no case takes its branch"
    lines, bad = [], []
    for name in live:
        case, flags, out, zs, g, P, rows = _rounded(name)
        ratio, where = _exceeds(case, *T.mirror(case, zs, g, flags, mutant=mutant), P, rows)
        lines.append(f"MUTANT {mutant} {name}: {ratio:.3g} x bar at {where}")
        if mutant == "bias_sum_last_row_missing":      # on a bias that wgrad_bf16's colsum or the fallback sum delivers
            q = where.rsplit(".", 1)[0]
            assert q.endswith(".db") and not T.f32_held(case, q), lines[-1]
        if not ratio >= 2.0:
            bad.append(lines[-1])
    print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


def test_mutants_change_nothing_where_not_live():
    for mutant in T.MUTANTS:
        for name in T.CASES:
            case, flags, out, zs, g, P, rows = _rounded(name)
            if T.mutant_live(case, mutant, g):
                continue
            ratio, where = _exceeds(case, *T.mirror(case, zs, g, flags, mutant=mutant), P, rows)
            assert ratio <= 0.0, (mutant, name, where)


def test_bias_from_unrounded_rows_is_no_mutant():
    """the colsum bias gradients sum the ROUNDED rows, the row kernel's the unrounded ones; the two differ by 0.6e-3 ..
    2.6e-3 normwise: nowhere twice a parameter bar, so the difference cannot be rejected and is not a mutant"""
    for name in T.CASES:
        case, flags, out, zs, g, P, rows = _rounded(name)
        for k, v in T.bias_from_unrounded_rows(case, zs, g, flags).items():
            if T.f32_held(case, k):
                continue
            assert R.rel_err(v.numpy(), P[k].numpy()) < 2 * T.P_NORM_BAR, (name, k)
            assert R.elem_err(v.numpy(), P[k].numpy()) <= T.P_ELEM_BAR, (name, k)


# ------------------------------------------------------------------------------------------------------ 4. non-vacuity
REACHED_BY = {
    "fused_boundary": {"cell2", "cell3", "L256", "L512_wide"},
    "unfused_boundary": {"L512_unfused"},
    "bwd_N256": {"cell2", "cell3"},
    "bwd_N512": {"L256"},
    "bwd_N1024": {"L512_wide"},
    "colsum_bias0": {"cell2", "direct_first"},
    "fallback_bias": {"all_gathered"},
    "column_blocks": {"L512_unfused", "L512_wide"},
    "folded_skip": {"cell2", "direct_first", "single256"},
    "no_skip": {"no_skip", "all_gathered"},
    "foreign_skip": {"foreign_skip"},
    "n1": {"single256"},
    "direct_not_last": {"direct_first"},
    "two_tables": {"all_gathered"},
    "two_gathers_one_table": {"cell2"},
    "no_grad": {"no_grad_inputs"},
    "stride0_grad": {"ones_grad"},
    "autocast": {"autocast"},
    "eps": {"eps1e-3"},
}


def test_case_table_reaches_every_branch():
    got = {n: T.branches(T.build(n)) for n in T.CASES}
    for tag, cases in REACHED_BY.items():
        for n in cases:
            assert tag in got[n], (tag, n, sorted(got[n]))
    assert set().union(*got.values()) == set(REACHED_BY), set().union(*got.values()) ^ set(REACHED_BY)
    # the unfused route delivers every bias from the row kernel; n == 1 has no boundary at all
    assert got["L512_unfused"].isdisjoint({"fused_boundary", "colsum_bias0", "fallback_bias"})
    assert got["single256"].isdisjoint({"fused_boundary", "unfused_boundary"})
    assert T.routing(T.build("L512_unfused")) == dict(fused_train_calls=1, bwd_layer_calls=1, library_dgrad_calls=2)
    assert T.routing(T.build("L512_wide")) == dict(fused_train_calls=1, bwd_layer_calls=3, library_dgrad_calls=0)
    assert T.routing(T.build("cell3")) == dict(fused_train_calls=1, bwd_layer_calls=3, library_dgrad_calls=0)
    assert T.routing(T.build("all_gathered")) == dict(fused_train_calls=1, bwd_layer_calls=1, library_dgrad_calls=0)
    assert T.routing(T.build("no_grad_inputs")) == dict(fused_train_calls=1, bwd_layer_calls=1, library_dgrad_calls=0)
    for n in T.CASES:                      # no table small enough for the forward's pre-projection (4 rows <= M)
        assert 4 * T.N_TAB > T.build(n)["M"]
    for a, b in T.SAME_BITS_AS.items():    # the bit equalities compare like with like
        ca, cb = T.build(a), T.build(b)
        assert all(torch.equal(x, y) for la, lb in zip(ca["layers"], cb["layers"]) for x, y in zip(la[:4], lb[:4]))
        assert all(torch.equal(ca["tables"][k], cb["tables"][k]) for k in ca["tables"]) and torch.equal(ca["r"], cb["r"])


def test_relu_case_keeps_rows_and_guards_the_jump():
    case, flags, out, zs, g, P, rows = _rounded("relu")
    live = int((g.abs().sum(dim=1) > 0).sum())
    assert 64 < live < case["M"], live
    for l in range(case["n"] - 1):
        W, b, gm, bt, act = case["layers"][l]
        y = T.ln_act_forward64(zs[l], gm.double(), bt.double(), R.ACT_NONE, case["eps"])
        assert float(y[g.abs().sum(dim=1) > 0].abs().min()) >= T.RELU_GUARD
