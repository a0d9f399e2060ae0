"""Conformance of every LayerNorm-bearing MLP entry under row offset, scale and eps (tests/ln_ref.py: the float64
definition, the cases, and -- tests/test_ln_ref.py -- the proof that a centred kernel passes these bars with 2x
headroom while a one-pass + shift kernel, a kernel without eps and a kernel with the wrong eps do not).

Bars (none tuned on a device result):
  fp32 rows        conftest.rel_err <= 1e-4 in every case; conftest.elem_err <= 1e-4 on forward rows for nominal
                   r <= 64 (outputs and the dz rows of _ln_act_backward); the const rows on their own:
                   |out - ref| <= 1e-4 max|ref|.  (Parameter and table gradients of the training round trips are sums
                   over rows: normwise bar.)
  bf16 rows of a single-layer entry (single-layer launches, _ln_act_*, _bwd_layer)
                   EVERY element: |out - ref| <= 2^-8 |ref| + 1e-4 max|ref|.
  bf16 multi-layer launches / training round trip
                   4 * BF16_TOL (test_gpu_bf16.py), BF16_OUT / BF16_GRAD (test_gpu_bf16_train.py), unchanged at every case.
  fp32 column sums (dgamma, dbeta, dbias)   rel_err <= 1e-4, for fp32 and bf16 rows alike (accumulated in fp32 before any rounding).
  every entry is called twice per case: torch.equal.

Offsets: a case's nominal r is lowered per launch shape by ln_ref.r_eff (a correct kernel's accumulator starts at the
bias and rounds at r sigma on every step); entries that take z directly keep the nominal r.

Every test loops over the cases, prints one line per (entry, case) -- worst error / bar -- and fails at the end with
the list of the cases outside a bar.

Worst measured error / bar per entry on an MI355X (the case and quantity that set it), with the pooled centred statistics;
in brackets the same figure with the one-pass + shift statistics these kernels had before:
  exact fp32 kernel      latent 32 0.26, 128 0.26, 256 0.33, head 0.29, narrow encoder 0.38, single 512 0.28 (r256, normwise)
  split-bf16 fp32        latent 128 x2 0.52 [6.9], x3 0.70 [13.1]; latent 256 x2 0.47 [1.8], x3 0.44 [4.2]; head 0.68 [17.6];
                         M = 65,617: 128-row / 64-row 0.49 [0.87: r64 runs at 16 there]
  bf16 single layers     0.94 - 0.97 [5.4 - 38 at r256]     (2^-9 |ref| of the 2^-8 |ref| bound is the rounding itself)
  bf16 multi-layer       feature-split 0.10 - 0.13 [0.11 - 0.18], whole-wave (one-pass, unchanged) 0.10 - 0.13
  _ln_act_* (unchanged)  fp32 0.38, bf16 0.96
  _bwd_layer             (256,128) 0.94, (512,256) 0.95, (1024,512) 0.94 [13.8: dgamma at r256]
  training round trip    fp32 exact 0.19, split-bf16 0.45 [1.35]; bf16 at r = 64 is 1.9 - 6.3 x BF16_GRAD on every gradient
                         with either statistics (z is dumped in bf16): it runs at ln_ref.R_BF16_TRAIN
"""
import numpy as np
import pytest
import torch

import ln_ref as R
from conftest import elem_err, rel_err
from test_gpu_bf16 import BF16_TOL
from test_gpu_bf16_train import BF16_GRAD, BF16_OUT

pytestmark = pytest.mark.gpu
BAR = R.F32_BAR
_ACT_MOD = {R.ACT_GELU: torch.nn.GELU, R.ACT_TANH: torch.nn.Tanh, R.ACT_RELU: torch.nn.ReLU}


def _net(case):
    mods = []
    for W, b, gm, bt, act in case["layers"]:
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        lin.weight.data.copy_(W)
        lin.bias.data.copy_(b)
        mods.append(lin)
        if gm is not None:
            ln = torch.nn.LayerNorm(W.shape[0], eps=case["eps"])
            ln.weight.data.copy_(gm)
            ln.bias.data.copy_(bt)
            mods += [ln, _ACT_MOD[act]()]
    return torch.nn.Sequential(*mods).cuda()


def _segments(case):
    dt = torch.bfloat16 if case["bf16"] else torch.float32
    segs = [(t.cuda().to(dt), None if i is None else i.cuda()) for t, i in case["segments"]]
    return segs, (segs[-1][0] if case["skip"] is not None else None)


def _nominal(case):
    return case["nominal_r"] if case["const"] is None else float(case["name"][len("const_c"):])


class _Report:
    """one line per (entry, case): worst error / bar; the failures are raised together at the end"""

    def __init__(self, entry):
        self.entry, self.lines, self.bad = entry, [], []

    def add(self, case_name, what, value, bar):
        ratio = value / bar
        self.lines.append(f"RATIO {self.entry} {case_name} {what} {value:.3g} / {bar:.3g} = {ratio:.3f}")
        if not ratio <= 1.0:
            self.bad.append(self.lines[-1])

    def f32_rows(self, case_name, what, out, ref, nominal, const_rows=(), elem=True):
        out, ref = out.detach().double().cpu().numpy(), np.asarray(ref, np.float64)
        assert out.shape == ref.shape, (what, out.shape, ref.shape)
        self.add(case_name, what + ".rel", rel_err(out, ref), BAR)
        if elem and nominal <= 64:
            self.add(case_name, what + ".elem", elem_err(out, ref), BAR)
        if len(const_rows):
            self.add(case_name, what + ".const", R.rows_err(out, ref, list(const_rows)), BAR)

    def bf16_elems(self, case_name, what, out, ref):
        assert out.dtype == torch.bfloat16
        self.add(case_name, what + ".bf16", R.bf16_ratio(out.float().cpu().numpy(), np.asarray(ref, np.float64)), 1.0)

    def norm(self, case_name, what, out, ref, bar):
        self.add(case_name, what, rel_err(out.detach().double().cpu().numpy(), np.asarray(ref, np.float64)), bar)

    def same(self, case_name, a, b):
        if not torch.equal(a, b):
            self.bad.append(f"{self.entry} {case_name}: two calls differ")

    def done(self):
        print("\n" + "\n".join(self.lines))
        assert not self.bad, "\n".join(self.bad)


def _forward(case):
    from hierarchicalgnn_amd import fused
    net = _net(case)
    segs, skip = _segments(case)
    with torch.no_grad():
        assert fused.supported(net, segs, skip)
        n0 = fused.stats["fused_calls"]
        out = fused.fused_concat_mlp(net, segs, skip)
        assert fused.stats["fused_calls"] > n0
        again = fused.fused_concat_mlp(net, segs, skip)
    return out, again


# ------------------------------------------------------------------------------------------------- fp32 forward entries
@pytest.mark.both_fp32_gemms
@pytest.mark.parametrize("cfg", [c for c in sorted(R.F32_CONFIGS) if R.F32_CONFIGS[c]["split"]])
def test_fp32_mlp_on_both_gemm_kernels(cfg, request):
    """fused_concat_mlp at latent 128 / 256, 2 and 3 layers, 3 segments (two gathered, one direct = skip), and the score
    head K -> 256 -> 256 -> 1: the exact fp32 kernel and the split-bf16 kernel (the marker asserts that it ran)"""
    fp32_gemm = request.node.callspec.params["fp32_gemm"]
    rep = _Report(f"{cfg}/{fp32_gemm}")
    for name in R.CASES:
        case = R.case_for(R.F32_CONFIGS[cfg], name, matrix=fp32_gemm == "split_bf16")
        out, again = _forward(case)
        rep.f32_rows(name, "out", out, case["ref"].numpy(), _nominal(case), case["const_rows"])
        rep.same(name, out, again)
    rep.done()


@pytest.mark.parametrize("cfg", [c for c in sorted(R.F32_CONFIGS) if not R.F32_CONFIGS[c]["split"]])
def test_fp32_mlp_exact_kernel_only(cfg):
    """latent 32, the narrow encoder (LayerNorm over 56 of 64 padded features) and one single-layer launch, o = 512"""
    rep = _Report(f"{cfg}/exact")
    for name in R.CASES:
        case = R.case_for(R.F32_CONFIGS[cfg], name)
        out, again = _forward(case)
        rep.f32_rows(name, "out", out, case["ref"].numpy(), _nominal(case), case["const_rows"])
        rep.same(name, out, again)
    rep.done()


def test_fp32_split3_rows128_and_rows64_at_65617_rows():
    """K -> 512 -> 256 at M = 65,617 = 65,536 + 81: the 128-row-tile kernel (option mlp_split3_rows128 = 1) and the
    64-row kernel (0), both held to the bar.  r64 is what the issue asks for here; it runs at r = 16 at this shape, where
    one-pass + shift statistics still pass, so r256 (r = 64 at K = 768: tests/test_ln_ref.py shows one-pass + shift
    outside the bar at this shape) runs too -- it is the case that guards the 128-row kernel's pooled statistics."""
    from hierarchicalgnn_amd import _lib, fused
    M = 65536 + 81
    lib = _lib.load()
    rep = _Report("L256x2/split_bf16/M65617")
    try:
        for name in ("r64", "r256"):
            case = R.case_for(R.F32_CONFIGS["L256x2"], name, matrix=True, M=M, ref_device="cuda")
            net = _net(case)
            segs, skip = _segments(case)
            for rows128 in (1, 0):
                _lib.check(lib.hgnn_set_option(b"mlp_split3_rows128", rows128))
                with torch.no_grad(), fused.options(fp32_split3=True):
                    n0 = fused.stats.get("split3_calls", 0)
                    out = fused.fused_concat_mlp(net, segs, skip)
                    again = fused.fused_concat_mlp(net, segs, skip)
                    assert fused.stats.get("split3_calls", 0) == n0 + 2
                rep.f32_rows(name, f"rows128={rows128}.out", out, case["ref"].numpy(), _nominal(case))
                rep.same(name, out, again)
    finally:
        _lib.check(lib.hgnn_set_option(b"mlp_split3_rows128", 1))
    rep.done()


# ------------------------------------------------------------------------------------------------- bf16 forward entries
@pytest.mark.parametrize("cfg", sorted(R.BF16_CONFIGS))
def test_bf16_multi_layer_launches(cfg):
    """whole-wave kernel (set_bf16_split(False)) at latent 32 / 128, feature-split kernel at latent 128 / 256 / 512, 2 and
    3 layers: the suite's own bar for them, unchanged at every case (hidden rows are post-LayerNorm)"""
    from hierarchicalgnn_amd import fused
    rep = _Report(cfg)
    old = fused._bf16_split
    fused.set_bf16_split(R.BF16_CONFIGS[cfg]["split"])
    try:
        for name in R.CASES:
            case = R.case_for(R.BF16_CONFIGS[cfg], name, bf16=True)
            net = _net(case)
            segs, skip = _segments(case)
            assert fused._wants_split(net, segs) == R.BF16_CONFIGS[cfg]["split"]
            out, again = _forward(case)
            assert out.dtype == torch.bfloat16
            rep.norm(name, "out", out.float(), case["ref"].numpy(), 4 * BF16_TOL)
            rep.same(name, out, again)
    finally:
        fused.set_bf16_split(old)
    rep.done()


@pytest.mark.parametrize("cfg", sorted(R.BF16_SINGLE))
def test_bf16_single_layer_launches(cfg):
    """feature-split single-layer launches, o in {256, 512, 1024}, with and without skip: the element-wise bf16 bound"""
    rep = _Report("single_" + cfg)
    for name in R.CASES:
        case = R.case_for(R.BF16_SINGLE[cfg], name, bf16=True)
        out, again = _forward(case)
        rep.bf16_elems(name, "out", out, case["ref"].numpy())
        rep.same(name, out, again)
    rep.done()


# --------------------------------------------------------------------------------------------------- the row kernels
@pytest.mark.parametrize("act", [R.ACT_GELU, R.ACT_TANH, R.ACT_RELU])
@pytest.mark.parametrize("W", [64, 256, 1024])
@pytest.mark.parametrize("bf16", [False, True])
def test_ln_act_row_kernels(bf16, W, act):
    """fused._ln_act_forward / _ln_act_backward on z = sigma (randn + r) given directly (nominal r, const rows literal)"""
    from hierarchicalgnn_amd import fused
    rep = _Report(f"ln_act_{'bf16' if bf16 else 'f32'}_W{W}_act{act}")
    for name in R.CASES:
        rc = R.make_rows_case(name, W, seed=act, bf16=bf16)
        dt = torch.bfloat16 if bf16 else torch.float32
        z, g = rc["z"].cuda().to(dt), rc["g"].cuda().to(dt)
        gm, bt = rc["gamma"].cuda(), rc["beta"].cuda()
        a_ref = R.ln_act_forward(rc["z"], rc["gamma"], rc["beta"], act, rc["eps"]).numpy()
        if act == R.ACT_RELU:
            # ReLU' jumps at 0: an element whose pre-activation is within rounding of 0 may legitimately land on either
            # side.  The pre-activations are O(1); no upstream gradient reaches the elements within 1e-3 of 0.
            y_ref = R.ln_act_forward(rc["z"], rc["gamma"], rc["beta"], R.ACT_NONE, rc["eps"])
            rc["g"] = torch.where(y_ref.abs() < 1e-3, torch.zeros_like(rc["g"]), rc["g"])
            g = rc["g"].cuda().to(dt)
        dz_ref, dg_ref, db_ref, dbias_ref = [t.numpy() for t in
                                             R.ln_act_backward(rc["z"], rc["g"], rc["gamma"], rc["beta"], act, rc["eps"])]
        out = fused._ln_act_forward(z, gm, bt, act, rc["eps"])
        dz, dg, db, dbias = fused._ln_act_backward(z, g, gm, bt, act, rc["eps"])
        if bf16:
            rep.bf16_elems(name, "out", out, a_ref)
            rep.bf16_elems(name, "dz", dz, dz_ref)
        else:
            rep.f32_rows(name, "out", out, a_ref, rc["r"], rc["const_rows"])
            rep.f32_rows(name, "dz", dz, dz_ref, rc["r"], rc["const_rows"])
        rep.norm(name, "dbias", dbias, dbias_ref, BAR)            # (summed in fp32 from the unrounded rows, bf16 too)
        rep.norm(name, "dgamma", dg, dg_ref, BAR)
        rep.norm(name, "dbeta", db, db_ref, BAR)
        rep.same(name, out, fused._ln_act_forward(z, gm, bt, act, rc["eps"]))
        again = fused._ln_act_backward(z, g, gm, bt, act, rc["eps"])
        for a, b in zip((dz, dg, db, dbias), again):
            rep.same(name, a, b)
    rep.done()


@pytest.mark.parametrize("K,N", [(256, 128), (512, 256), (1024, 512)])
def test_bf16_backward_layer_ln_form(K, N):
    """fused._bwd_layer, LayerNorm form: dz' = dLN(act'(LN(z')) (dz W)), a' = act(LN(z')), dgamma, dbeta; z' as above"""
    from hierarchicalgnn_amd import fused
    assert fused._bwd_layer_supported(K, N)
    rep = _Report(f"bwd_layer_K{K}_N{N}")
    gen = torch.Generator().manual_seed(K + N)
    dz = torch.randn(R.M_ROWS, K, generator=gen).bfloat16().float()
    Wt = (torch.randn(K, N, generator=gen) / K ** 0.5)
    da_ref = dz.double() @ Wt.bfloat16().double()
    for name in R.CASES:
        rc = R.make_rows_case(name, N, seed=K, bf16=True)
        a_ref = R.ln_act_forward(rc["z"], rc["gamma"], rc["beta"], R.ACT_GELU, rc["eps"]).numpy()
        dzp_ref, dg_ref, db_ref, _ = [t.numpy() for t in
                                      R.ln_act_backward(rc["z"], da_ref, rc["gamma"], rc["beta"], R.ACT_GELU, rc["eps"])]
        args = (dz.cuda().bfloat16(), Wt.cuda(), rc["z"].cuda().bfloat16(), rc["gamma"].cuda(), rc["beta"].cuda(),
                R.ACT_GELU, rc["eps"])
        dzp, a_prev, dg, db = fused._bwd_layer(*args, want_a=True)
        rep.bf16_elems(name, "a_prev", a_prev, a_ref)
        rep.bf16_elems(name, "dz_prev", dzp, dzp_ref)
        rep.norm(name, "dgamma", dg, dg_ref, BAR)
        rep.norm(name, "dbeta", db, db_ref, BAR)
        for a, b in zip((dzp, a_prev, dg, db), fused._bwd_layer(*args, want_a=True)):
            rep.same(name, a, b)
    rep.done()


# ------------------------------------------------------------------------------------------------ training round trips
def _autograd64(case, r_out):
    """float64 autograd through the definition's modules: out and the gradients of the table, the direct rows and
    every parameter"""
    net = _net(case).cpu().double()
    table = case["segments"][0][0].double().requires_grad_(True)
    direct = case["segments"][-1][0].double().requires_grad_(True)
    x = torch.cat([table[i] for _, i in case["segments"][:-1]] + [direct], dim=1)
    out = net(x) + direct
    (out * r_out.double()).sum().backward()
    return out.detach(), table.grad, direct.grad, [p.grad for p in net.parameters()]


def _train_once(case, net, r_out, bf16):
    from hierarchicalgnn_amd import fused, mlp
    dt = torch.bfloat16 if bf16 else torch.float32
    net.zero_grad(set_to_none=True)
    table = case["segments"][0][0].cuda().to(dt).requires_grad_(True)
    direct = case["segments"][-1][0].cuda().to(dt).requires_grad_(True)
    segs = [(table, i.cuda()) for _, i in case["segments"][:-1]] + [(direct, None)]
    n0 = fused.stats["fused_train_calls"]
    out = mlp.concat_mlp(net, segs, skip=direct)
    assert fused.stats["fused_train_calls"] == n0 + 1
    (out.float() * r_out.cuda()).sum().backward()
    return [out.detach(), table.grad, direct.grad] + [p.grad.clone() for p in net.parameters()]


@pytest.mark.parametrize("mode", ["bf16", "f32_exact", "f32_split3"])
def test_training_round_trip_latent128(mode):
    """forward with dumps, backward, all gradients, at latent 128, 2 layers: bf16 through mlp.concat_mlp with grad; fp32
    on the exact kernels and with set_fp32_split3_training(True).  The fp32 round trips run case r64 (at r_eff); the
    bf16 one runs at r = ln_ref.R_BF16_TRAIN = 2 -- z is dumped in bf16 -- and PRINTS, without asserting, what r = 64 and
    r = 256 give (DESIGN.md records them)."""
    from hierarchicalgnn_amd import fused
    bf16 = mode == "bf16"
    case = R.case_for(R.F32_CONFIGS["L128x2"], "r64", bf16=bf16, matrix=mode != "f32_exact",
                      r=R.R_BF16_TRAIN if bf16 else None)   # (the bf16 dumps of z cap the offset: ln_ref.R_BF16_TRAIN)
    r_out = torch.randn(R.M_ROWS, 128, generator=torch.Generator().manual_seed(5))
    ref = _autograd64(case, r_out)
    ref = [ref[0], ref[1], ref[2]] + ref[3]
    net = _net(case)
    names = ["out", "d_table", "d_direct"] + ["d_" + n for n, _ in net.named_parameters()]
    old, old_t = fused._fp32_split3, fused._fp32_split3_train
    rep = _Report("train_" + mode)
    try:
        fused.set_fp32_split3(mode == "f32_split3")
        fused.set_fp32_split3_training(mode == "f32_split3")
        n_s3 = fused.stats.get("split3_calls", 0)
        got = _train_once(case, net, r_out, bf16)
        again = _train_once(case, net, r_out, bf16)
        assert (fused.stats.get("split3_calls", 0) > n_s3) == (mode == "f32_split3")
    finally:
        fused.set_fp32_split3(old)
        fused.set_fp32_split3_training(old_t)
    label = f"r{case['r']:g}"
    if bf16:   # figures only: the offsets the bf16 dump format cannot carry
        for r_big in (64.0, 256.0):
            big = R.case_for(R.F32_CONFIGS["L128x2"], "r64", bf16=True, matrix=True, r=r_big)
            ref_big = _autograd64(big, r_out)
            got_big = _train_once(big, _net(big), r_out, True)
            worst = max(rel_err(a.float().cpu().numpy(), b.numpy()) for a, b in zip(got_big[1:], [ref_big[1], ref_big[2]] + ref_big[3]))
            print(f"FIGURE train_bf16 r{r_big:g}: out {rel_err(got_big[0].float().cpu().numpy(), ref_big[0].numpy()) / BF16_OUT:.2f} x BF16_OUT, "
                  f"worst gradient {worst / BF16_GRAD:.2f} x BF16_GRAD")
    for nm, a, b, c in zip(names, got, ref, again):
        if bf16:
            rep.norm(label, nm, a.float(), b.numpy(), BF16_OUT if nm == "out" else BF16_GRAD)
        elif nm == "out":
            rep.f32_rows(label, nm, a, b.numpy(), _nominal(case))
        else:
            rep.norm(label, nm, a, b.numpy(), BAR)
        rep.same(label, a, c)
    rep.done()
