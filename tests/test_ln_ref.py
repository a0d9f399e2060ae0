"""tests/ln_ref.py proves itself, and proves that tests/test_gpu_mlp_layernorm.py is both passable and meaningful:

  * the float64 definition equals torch's float64 layer_norm + activation and float64 autograd to 1e-12;
  * every offset case achieves its r (median |row mean| / row std of every layer's z within [0.7, 1.4] x r), the
    const rows have std exactly 0;
  * A CORRECT KERNEL CAN PASS: the `centred` float32 emulation, whose GEMM accumulates from the bias like the kernels
    do, stays at or below HALF of every fp32 bar of the GPU file for every (case, launch shape) it uses, in both
    summation orders, and shows zero violations of the bf16 single-layer bound after one bf16 rounding;
  * the same for the `pooled` form of the feature-split kernels, and for the backward's dz rows and column sums;
  * A SUBTLY WRONG KERNEL CANNOT: `onepass_shift` exceeds the fp32 bar on r64 (at the shapes that keep r = 64), r256
    and const_c256 and violates the bf16 bound at r256; a kernel without eps, or with the default eps where the module
    says 1e-3, exceeds the bars on the s-8 / eps1e-3 cases.

Where r is lowered (ln_ref.r_eff: the accumulation error of an offset row grows with r sqrt(K / GROUP) in ANY fp32
kernel whose accumulator starts at the bias): on the exact fp32 kernel r64 runs at 16 for K <= 256 and at 8 for K = 384 /
768, r256 at 64 (K <= 128) or 32; on the split-bf16 kernel r64 runs at 32 (K = 256, 384) or 16 (K = 768), r256 at 128 or
64; const_c256 follows r256; bf16 launches keep r up to 256 for K <= 512 and run at 128 above.  The row kernels and the
backward layer take z directly and keep every nominal r.  The printed tables (pytest -s) carry the r of every line and
mark the (case, shape) pairs at which the lowered r no longer tells one-pass + shift from centred (NOT DISCRIMINATING);
every launch shape keeps at least its r256 case discriminating on the split-bf16 kernels.
"""
import numpy as np
import pytest
import torch

import ln_ref as R

EMUL_ROWS = [0, R.M_ROWS // 2, R.M_ROWS - 1] + list(range(1, 22))     # the const rows + 21 more (rows are independent)
ORDERS = ("fwd", "rev")
_TORCH_ACT = {R.ACT_NONE: lambda t: t, R.ACT_GELU: torch.nn.functional.gelu, R.ACT_TANH: torch.tanh, R.ACT_RELU: torch.relu}


def _carries_elem_bar(case):
    """the GPU file's rule: element-wise bar for nominal r <= 64 (const_cC counts as r = C)"""
    nominal = case["nominal_r"] if case["const"] is None else float(case["name"][len("const_c"):])
    return nominal <= 64


@pytest.mark.parametrize("name", R.CASES)
def test_definition_equals_torch_float64(name):
    case = R.make_case(name, [96, 64, 64, 32], M=67, seed=3)
    x = case["x"].double()
    h = x
    for W, b, gm, bt, act in case["layers"]:
        z = torch.nn.functional.linear(h, W.double(), b.double())
        h = _TORCH_ACT[act](torch.nn.functional.layer_norm(z, [z.shape[1]], gm.double(), bt.double(), case["eps"]))
    ref = h + case["skip"].double()
    assert float((case["ref"] - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # backward of the last layer against float64 autograd
    W, b, gm, bt, act = case["layers"][-1]
    z = case["zs"][-1].clone().requires_grad_(True)
    g_, b_ = gm.double().requires_grad_(True), bt.double().requires_grad_(True)
    go = torch.randn(z.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    _TORCH_ACT[act](torch.nn.functional.layer_norm(z, [z.shape[1]], g_, b_, case["eps"])).backward(go)
    dz, dg, db, dbias = R.ln_act_backward(z.detach(), go, gm, bt, act, case["eps"])
    for got, want in ((dz, z.grad), (dg, g_.grad), (db, b_.grad), (dbias, z.grad.sum(0))):
        assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), float(z.grad.abs().max()))


@pytest.mark.parametrize("cfg", sorted(R.F32_CONFIGS))
def test_cases_achieve_their_offset(cfg):
    for name in R.CASES:
        case = R.case_for(R.F32_CONFIGS[cfg], name)
        rows = [i for i in range(R.M_ROWS) if i not in case["const_rows"]]
        for l, z in enumerate(case["zs"]):
            if case["layers"][l][2] is None:
                continue
            want = case["r"] if case["const"] is None else (case["const"] / float(z[rows].std(dim=1).mean()) if l == 0 else 0.0)
            got = float((z[rows].mean(dim=1).abs() / z[rows].std(dim=1, unbiased=False)).median())
            if want >= 8:
                assert 0.7 * want <= got <= 1.4 * want, (cfg, name, l, got, want)
        if case["const_rows"]:
            assert float(case["zs"][0][case["const_rows"]].std(dim=1, unbiased=False).abs().max()) == 0.0
            assert float((case["zs"][0][case["const_rows"]] - case["const"]).abs().max()) == 0.0
    for W in (64, 256, 1024):
        for name in ("r16", "r64", "r256"):
            rc = R.make_rows_case(name, W)
            got = float((rc["z"].double().mean(1).abs() / rc["z"].double().std(1, unbiased=False)).median())
            assert 0.7 * rc["r"] <= got <= 1.4 * rc["r"]
        rc = R.make_rows_case("const_c256", W)
        assert float(rc["z"][rc["const_rows"]].double().std(1, unbiased=False).max()) == 0.0


def _figures(case, out):
    ref = case["ref"][EMUL_ROWS].numpy()
    f = dict(rel=R.rel_err(out, ref), elem=R.elem_err(out, ref))
    if case["const_rows"]:
        f["const"] = R.rows_err(out, ref, [0, 1, 2])          # EMUL_ROWS starts with the three const rows
    return f


def _exceeds_f32_bars(case, f):
    return f["rel"] > R.F32_BAR or (_carries_elem_bar(case) and f["elem"] > R.F32_BAR) or f.get("const", 0.0) > R.F32_BAR


F32_LAUNCHES = [(c, False) for c in sorted(R.F32_CONFIGS)] + [(c, True) for c in sorted(R.F32_CONFIGS) if R.F32_CONFIGS[c]["split"]]


@pytest.mark.parametrize("cfg,matrix", F32_LAUNCHES)
def test_fp32_bars_admit_centred_and_reject_the_wrong_kernels(cfg, matrix):
    lines = []
    for name in R.CASES:
        case = R.case_for(R.F32_CONFIGS[cfg], name, matrix=matrix)
        for order in ORDERS:
            f = _figures(case, R.emul_net(case, "centred", order, EMUL_ROWS))
            lines.append(f"{cfg:10s} {'split' if matrix else 'exact'} {name:11s} r={case['r']:<5g} centred/{order}: " + " ".join(f"{k} {v:.1e}" for k, v in f.items()))
            assert f["rel"] <= 0.5 * R.F32_BAR, lines[-1]
            assert not _carries_elem_bar(case) or f["elem"] <= 0.5 * R.F32_BAR, lines[-1]
            assert f.get("const", 0.0) <= 0.5 * R.F32_BAR, lines[-1]
        if matrix and case["zs"][0].shape[1] % 128 == 0:     # the statistics as the feature-split kernels pool them
            for order in ORDERS:
                f = _figures(case, R.emul_net(case, "pooled", order, EMUL_ROWS))
                lines.append(f"{cfg:10s} split {name:11s} r={case['r']:<5g} pooled/{order}: " + " ".join(f"{k} {v:.1e}" for k, v in f.items()))
                assert f["rel"] <= 0.5 * R.F32_BAR and f.get("const", 0.0) <= 0.5 * R.F32_BAR, lines[-1]
                assert not _carries_elem_bar(case) or f["elem"] <= 0.5 * R.F32_BAR, lines[-1]
        wrong = []
        if name in ("r16", "r64", "r256", "const_c256"):
            if max(case["r"], case["const"] or 0) >= (128 if case["const"] else 64):
                wrong.append(("onepass_shift", "inside"))
            else:   # r lowered below where one-pass + shift leaves the bars: this (case, shape) guards nothing by itself
                f = _figures(case, R.emul_net(case, "onepass_shift", "fwd", EMUL_ROWS))
                lines.append(f"{cfg:10s} {'split' if matrix else 'exact'} {name:11s} r={case['r']:<5g} onepass_shift/fwd: "
                             + " ".join(f"{k} {v:.1e}" for k, v in f.items())
                             + ("   (fails)" if _exceeds_f32_bars(case, f) else "   NOT DISCRIMINATING at this r"))
        if name.startswith("s-8") or name == "eps1e-3":
            wrong.append(("centred", "omit"))
        if name == "eps1e-3":
            wrong.append(("centred", "default"))
        for mode, eps_mode in wrong:
            for order in ORDERS:
                f = _figures(case, R.emul_net(case, mode, order, EMUL_ROWS, eps_mode))
                lines.append(f"{cfg:10s} {'split' if matrix else 'exact'} {name:11s} r={case['r']:<5g} {mode}/eps {eps_mode}/{order}: "
                             + " ".join(f"{k} {v:.1e}" for k, v in f.items()) + "   (must fail)")
                assert _exceeds_f32_bars(case, f), lines[-1]
    print("\n" + "\n".join(lines))


@pytest.mark.parametrize("cfg", sorted(R.BF16_SINGLE))
def test_bf16_single_layer_bound_admits_centred_and_rejects_onepass(cfg):
    lines = []
    for name in R.CASES:
        case = R.case_for(R.BF16_SINGLE[cfg], name, bf16=True)
        ref = case["ref"][EMUL_ROWS].numpy()
        for mode in ("centred",) + (("onepass_shift",) if name == "r256" and case["r"] >= 128 else ()):
            for order in ORDERS:
                out = torch.from_numpy(R.emul_net(case, mode, order, EMUL_ROWS)).bfloat16().float().numpy()
                ratio = R.bf16_ratio(out, ref)
                lines.append(f"{cfg:10s} {name:11s} r={case['r']:<5g} {mode}/{order}: worst error / bound {ratio:.2f}")
                assert (ratio <= 1.0) == (mode == "centred"), lines[-1]
    print("\n" + "\n".join(lines))


@pytest.mark.parametrize("W", [64, 256, 1024])
def test_row_cases_keep_the_nominal_offset_and_reject_onepass(W):
    """z handed over directly (row kernels, backward layer): no GEMM, nominal r; centred within half the bars,
    one-pass + shift outside them at r64 / r256 (fp32) and at r256 after one bf16 rounding"""
    lines = []
    for name in R.CASES:
        rc = R.make_rows_case(name, W)
        z, gm, bt = rc["z"].numpy(), rc["gamma"].numpy(), rc["beta"].numpy()
        ref = R.ln_act_forward(rc["z"], rc["gamma"], rc["beta"], R.ACT_GELU, rc["eps"]).numpy()
        for order in ORDERS:
            out = R.emul_ln_act(z, gm, bt, R.ACT_GELU, rc["eps"], "centred", order)
            rel, elem = R.rel_err(out, ref), R.elem_err(out, ref)
            lines.append(f"W={W:<5d} {name:11s} centred/{order}: rel {rel:.1e} elem {elem:.1e}")
            assert rel <= 0.5 * R.F32_BAR and (rc["r"] > 64 or elem <= 0.5 * R.F32_BAR), lines[-1]
            assert R.bf16_ratio(torch.from_numpy(out).bfloat16().float().numpy(), ref) <= 1.0
            if name in ("r64", "r256"):
                bad = R.emul_ln_act(z, gm, bt, R.ACT_GELU, rc["eps"], "onepass_shift", order)
                rel, elem = R.rel_err(bad, ref), R.elem_err(bad, ref)
                lines.append(f"W={W:<5d} {name:11s} onepass_shift/{order}: rel {rel:.1e} elem {elem:.1e}   (must fail)")
                assert rel > R.F32_BAR or (rc["r"] <= 64 and elem > R.F32_BAR), lines[-1]
                if name == "r256":
                    assert R.bf16_ratio(torch.from_numpy(bad).bfloat16().float().numpy(), ref) > 1.0
        # the backward: dz rows (normwise, element-wise for r <= 64) and the fp32 column sums, fp32 and bf16-exact inputs
        for bf16 in (False, True):
            rb = R.make_rows_case(name, W, bf16=bf16)
            refs = [t.numpy() for t in R.ln_act_backward(rb["z"], rb["g"], rb["gamma"], rb["beta"], R.ACT_GELU, rb["eps"])]
            for order in ORDERS:
                got = R.emul_ln_act_backward(rb["z"].numpy(), rb["g"].numpy(), gm, bt, R.ACT_GELU, rb["eps"], order)
                errs = [R.rel_err(a, b) for a, b in zip(got, refs)]
                elem = R.elem_err(got[0], refs[0])
                lines.append(f"W={W:<5d} {name:11s} backward {'bf16' if bf16 else 'f32 '}/{order}: dz rel {errs[0]:.1e} elem {elem:.1e} "
                             f"dgamma {errs[1]:.1e} dbeta {errs[2]:.1e} dbias {errs[3]:.1e}")
                assert max(errs) <= 0.5 * R.F32_BAR and (rb["r"] > 64 or elem <= 0.5 * R.F32_BAR), lines[-1]
    print("\n" + "\n".join(lines))
