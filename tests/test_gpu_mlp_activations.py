"""SiLU, LeakyReLU, ELU and Sigmoid (HGNN_ACT_* 4..7) through every kernel that takes an activation code, against the
float64 definitions of tests/act_ref.py (= torch.nn at its defaults) at the bars the tests of the same kernels use for
GELU / Tanh: fp32 rows 1e-4 normwise and element-wise (tests/test_gpu_mlp_layernorm.py, exact and split-bf16 alike),
bf16 multi-layer launches 4 * BF16_TOL, bf16 single-layer entries (row kernels, backward layer) ln_ref.bf16_ratio <= 1
on every element, their fp32 column sums 1e-4 normwise.
tests/test_act_ref.py proves the fp32 cases at half the bar in a float32 emulation; no bar comes from a device result.

Shapes: each kernel at its narrowest width, M in {1, 64, 193}, 97-row tables gathered by index.  Every entry is called
twice: the same bits."""
import numpy as np
import pytest
import torch

import act_ref as A
import ln_ref as R
from conftest import elem_err, rel_err
from test_gpu_bf16 import BF16_TOL

pytestmark = pytest.mark.gpu
BAR = R.F32_BAR
ACT_MOD = {R.ACT_GELU: torch.nn.GELU, R.ACT_TANH: torch.nn.Tanh, R.ACT_RELU: torch.nn.ReLU, A.ACT_SILU: torch.nn.SiLU,
           A.ACT_LEAKY_RELU: torch.nn.LeakyReLU, A.ACT_ELU: torch.nn.ELU, A.ACT_SIGMOID: torch.nn.Sigmoid}
MS = (1, 64, R.M_ROWS)


def net_of(case):
    """the Sequential of a case, as make_mlp lays it out (with or without LayerNorm)"""
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
            mods.append(ln)
        if act:
            mods.append(ACT_MOD[act]())
    return torch.nn.Sequential(*mods).cuda()


def segments_of(case):
    dt = torch.bfloat16 if case["bf16"] else torch.float32
    segs = [(t.cuda().to(dt), None if i is None else i.cuda()) for t, i in case["segments"]]
    return segs, (segs[-1][0] if case["skip"] is not None else None)


def check_f32(tag, out, ref):
    out, ref = out.detach().double().cpu().numpy(), np.asarray(ref, np.float64)
    assert out.shape == ref.shape and np.isfinite(out).all(), tag
    r, e = rel_err(out, ref), elem_err(out, ref)
    print(f"RATIO {tag} rel {r:.3g} elem {e:.3g} / {BAR:.3g}")
    assert r <= BAR and e <= BAR, (tag, r, e)


def _twice(net, segs, skip):
    from hierarchicalgnn_amd import fused
    with torch.no_grad():
        assert fused.supported(net, segs, skip)
        lib0, n0 = fused.stats["library_calls"], fused.stats["fused_calls"]
        out = fused.fused_concat_mlp(net, segs, skip)
        again = fused.fused_concat_mlp(net, segs, skip)
        assert fused.stats["fused_calls"] >= n0 + 2 and fused.stats["library_calls"] == lib0
    assert torch.equal(out, again)
    return out


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("cfg", sorted(A.F32_ACT_CONFIGS))
def test_exact_fp32_kernel(cfg, M):
    """latent 32 with two and three layers, the H = 64 head and the small-K encoders: the compile-time SiLU
    instantiations (SiLU + Tanh / SiLU output) and the runtime switch (any other combination)"""
    from hierarchicalgnn_amd import fused
    case = A.case_for(A.F32_ACT_CONFIGS[cfg], M=M)
    with fused.options(fp32_split3=False):
        out = _twice(net_of(case), *segments_of(case))
    check_f32(f"exact/{cfg}/M{M}", out, case["ref"].numpy())


def _dumps(case, split3=False):
    """the pre-LayerNorm rows the differentiable forward dumps (exact fp32 route)"""
    from hierarchicalgnn_amd import fused
    net = net_of(case)
    segs, skip = segments_of(case)
    assert fused.supported_train(net, segs, skip)
    out = fused.fused_concat_mlp_train(net, segs, skip)
    n = len(case["layers"])
    return out, list(out.grad_fn.saved_tensors)[-n:]


def test_silu_layers_compile_time_and_runtime_switch_same_bits():
    """hidden SiLU + SiLU output runs the compile-time instantiation, hidden SiLU + ELU output the runtime switch of the
    same kernel; both call act_apply: the last layer's pre-LayerNorm rows, which depend on the two SiLU layers only, are
    the same bits (the cases share widths, hence weights and inputs)"""
    a = A.case_for(A.F32_ACT_CONFIGS["L32x3_silu_silu"])
    b = A.case_for(A.F32_ACT_CONFIGS["L32x3_silu_elu"])
    assert all(torch.equal(x[0], y[0]) for x, y in zip(a["layers"], b["layers"]))
    _, za = _dumps(a)
    _, zb = _dumps(b)
    assert za[2].shape == (R.M_ROWS, 32) and torch.equal(za[2], zb[2]) and torch.equal(za[1], zb[1])
    check_f32("exact/dump z2", za[2], a["zs"][2].numpy())


@pytest.mark.parametrize("split3", [False, True], ids=["exact", "split_bf16"])
def test_forced_runtime_switch_against_the_compile_time_instantiation(split3):
    """hgnn_set_option("mlp_act_switch", 1) (what tools/bench_mlp_activations.py times the switch with) sends a
    combination that has an instantiation through ACT = -1 of the same kernel.  Exact fp32 kernel: the same bits.
    Split-bf16 kernel: the same source arithmetic, but the compiler may contract an inlined activation's last product
    into the hi / mid split of the hidden rows, so both are held to the kernel's bar against float64 instead"""
    from hierarchicalgnn_amd import _lib, fused
    lib = _lib.load()
    for cfg in ("L128x2_silu_tanh", "L128x3_silu_silu"):
        case = A.case_for(A.SPLIT3_ACT_CONFIGS[cfg], matrix=split3)
        net = net_of(case)
        segs, skip = segments_of(case)
        with fused.options(fp32_split3=split3):
            own = _twice(net, segs, skip)
            _lib.check(lib.hgnn_set_option(b"mlp_act_switch", 1))
            try:
                forced = _twice(net, segs, skip)
            finally:
                _lib.check(lib.hgnn_set_option(b"mlp_act_switch", 0))
        if split3:
            check_f32(f"split3 forced switch/{cfg}", forced, case["ref"].numpy())
            check_f32(f"split3 compile-time/{cfg}", own, case["ref"].numpy())
        else:
            assert torch.equal(own, forced), cfg


@pytest.mark.parametrize("M", MS[1:])
@pytest.mark.parametrize("cfg", sorted(A.SPLIT3_ACT_CONFIGS))
def test_split_bf16_fp32_kernel(cfg, M):
    """latent 128, the split-bf16 kernel's narrowest: compile-time SiLU and the runtime switch"""
    from hierarchicalgnn_amd import fused
    case = A.case_for(A.SPLIT3_ACT_CONFIGS[cfg], matrix=True, M=M)
    with fused.options(fp32_split3=True):
        n0 = fused.stats.get("split3_calls", 0)
        out = _twice(net_of(case), *segments_of(case))
        assert fused.stats.get("split3_calls", 0) == n0 + 2
    check_f32(f"split3/{cfg}/M{M}", out, case["ref"].numpy())


def test_split_bf16_128_row_tile_at_its_smallest_m():
    """K -> 512 -> 256 at M = 65,536 + 81, the smallest row count region that takes the 128-row K-half tile; rows
    gathered from 97-row tables.  SiLU + Tanh (compile-time) and SiLU + ELU (switch)"""
    from hierarchicalgnn_amd import fused
    for acts in ([A.ACT_SILU, R.ACT_TANH], [A.ACT_SILU, A.ACT_ELU]):
        case = A.make_case("r0", [768, 512, 256], acts, M=65536 + 81, group=R.GROUP_MATRIX, ref_device="cuda")
        with fused.options(fp32_split3=True):
            out = _twice(net_of(case), *segments_of(case))
        check_f32(f"split3/rows128/{acts}", out, case["ref"].numpy())


@pytest.mark.parametrize("cfg", sorted(A.BF16_ACT_CONFIGS))
def test_bf16_kernels(cfg):
    """whole-wave bf16 kernel at latent 32, feature-split kernel at latent 128"""
    from hierarchicalgnn_amd import fused
    split = A.BF16_ACT_CONFIGS[cfg]["split"]
    old = fused._bf16_split
    fused.set_bf16_split(split)
    try:
        for M in MS:
            case = A.case_for(A.BF16_ACT_CONFIGS[cfg], bf16=True, M=M)
            net = net_of(case)
            segs, skip = segments_of(case)
            assert fused._wants_split(net, segs) == split
            out = _twice(net, segs, skip)
            assert out.dtype == torch.bfloat16
            r = rel_err(out.float().cpu().numpy(), case["ref"].numpy())
            print(f"RATIO bf16/{cfg}/M{M} {r:.3g} / {4 * BF16_TOL:.3g}")
            assert r <= 4 * BF16_TOL
    finally:
        fused.set_bf16_split(old)


# ------------------------------------------------------------------------------------------------------- row kernels
def _rows_ref(z, g, gm, bt, act, eps):
    z, g, gm, bt = z.double(), g.double(), gm.double(), bt.double()
    mean, rstd = R.ln_stats64(z, eps)
    xh = (z - mean) * rstd
    y = xh * gm + bt
    dy = g * A.act_grad64(y, act)
    gg = dy * gm
    dz = rstd * (gg - gg.mean(dim=1, keepdim=True) - xh * (gg * xh).mean(dim=1, keepdim=True))
    return A.act64(y, act), dz, (dy * xh).sum(0), dy.sum(0), dz.sum(0)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("W", [64, 1024])
@pytest.mark.parametrize("act", A.NEW_CODES)
def test_ln_act_row_kernels(act, W, bf16):
    """hgnn_ln_act_forward / backward at their narrowest and widest width, rows that carry ELU's tiny-|x| range through
    a unit LayerNorm scale (gamma = rstd^-1 would need the statistics: the tiny values enter through beta instead)"""
    from hierarchicalgnn_amd import fused
    z, g = A.tiny_rows(W)
    gen = torch.Generator().manual_seed(W + act)
    gm = 1 + 0.2 * torch.randn(W, generator=gen)
    bt = 0.2 * torch.randn(W, generator=gen)
    # some columns: gamma = 0 and beta in the cancelling range, so y = beta exactly there
    tiny = torch.tensor([s * 2.0 ** e for e in range(-20, -5) for s in (1.0, -1.0)])
    gm[:tiny.numel()] = 0.0
    bt[:tiny.numel()] = tiny
    dt = torch.bfloat16 if bf16 else torch.float32
    zc, gc = z.to(dt), g.to(dt)
    a_ref, dz_ref, dgm, dbt, dbias = _rows_ref(zc.float(), gc.float(), gm, bt, act, 1e-5)
    zd, gd, gmd, btd = zc.cuda(), gc.cuda(), gm.cuda(), bt.cuda()
    out = fused._ln_act_forward(zd, gmd, btd, act, 1e-5)
    assert torch.equal(out, fused._ln_act_forward(zd, gmd, btd, act, 1e-5))
    res = fused._ln_act_backward(zd, gd, gmd, btd, act, 1e-5)
    res2 = fused._ln_act_backward(zd, gd, gmd, btd, act, 1e-5)
    assert all(torch.equal(x, y) for x, y in zip(res, res2))
    tag = f"ln_act/{A.ACT_NAME[act]}/W{W}/{'bf16' if bf16 else 'f32'}"
    if bf16:
        for what, got, ref in (("out", out, a_ref), ("dz", res[0], dz_ref)):
            ratio = R.bf16_ratio(got.float().cpu().numpy(), ref.numpy())
            print(f"RATIO {tag} {what} bf16 {ratio:.3f}")
            assert ratio <= 1.0, (tag, what, ratio)
    else:
        check_f32(tag + " out", out, a_ref.numpy())
        check_f32(tag + " dz", res[0], dz_ref.numpy())
        # ELU in the cancelling range, held RELATIVELY: exp(x) - 1 in float32 would be off by 2^-24 / |x|
        if act == A.ACT_ELU:
            cols = slice(0, tiny.numel())
            got, ref = out[:, cols].double().cpu().numpy(), a_ref[:, cols].numpy()
            assert float((np.abs(got - ref) / np.abs(ref)).max()) <= 16 * A.U
    for what, got, ref in (("dgamma", res[1], dgm), ("dbeta", res[2], dbt), ("dbias", res[3], dbias)):
        r = rel_err(got.double().cpu().numpy(), ref.numpy())
        print(f"RATIO {tag} {what} {r:.3g}")
        assert r <= BAR, (tag, what, r)


# ---------------------------------------------------------------------------------------------------- backward layers
@pytest.mark.parametrize("act", [A.ACT_SILU, A.ACT_ELU], ids=["silu_compile_time", "elu_switch"])
def test_backward_layer_f32(act):
    """hgnn_mlp_backward_layer_f32 at its smallest (K, N) = (64, 64): dz W fused with the LayerNorm / activation backward
    of the layer below and its recomputed activations"""
    from hierarchicalgnn_amd import fused
    K = N = 64
    gen = torch.Generator().manual_seed(5 + act)
    dz = torch.randn(R.M_ROWS, K, generator=gen)
    Wm = torch.randn(K, N, generator=gen) / K ** 0.5
    c = R.make_rows_case("r0", N)
    da = dz.double() @ Wm.double()
    a_ref, dzp_ref, dgm, dbt, dbias = _rows_ref(c["z"], da, c["gamma"], c["beta"], act, c["eps"])
    old = fused._bwd_layer_f32_on
    fused.set_bwd_layer_f32(True)
    try:
        args = (dz.cuda(), Wm.cuda(), c["z"].cuda(), c["gamma"].cuda(), c["beta"].cuda(), act, c["eps"])
        res = fused._bwd_layer_f32(*args, want_a=True)
        res2 = fused._bwd_layer_f32(*args, want_a=True)
    finally:
        fused.set_bwd_layer_f32(old)
    assert all(torch.equal(x, y) for x, y in zip(res, res2))
    tag = f"bwd_layer_f32/{A.ACT_NAME[act]}"
    check_f32(tag + " dz_prev", res[0], dzp_ref.numpy())
    check_f32(tag + " a_prev", res[1], a_ref.numpy())
    for what, got, ref in (("dgamma", res[2], dgm), ("dbeta", res[3], dbt), ("dbias", res[4], dbias)):
        assert rel_err(got.double().cpu().numpy(), ref.numpy()) <= BAR, (tag, what)


@pytest.mark.parametrize("act", [A.ACT_SILU, A.ACT_ELU], ids=["silu", "elu"])
def test_backward_layer_bf16(act):
    """hgnn_mlp_backward_layer_bf16 at its smallest (K, N), held as tests/test_gpu_mlp_layernorm.py holds it for GELU
    (test_bf16_backward_layer_ln_form, the reference built the same way): every element of a_prev and dz_prev within
    2^-8 |ref| + 1e-4 max|ref| (ln_ref.bf16_ratio), dgamma / dbeta -- summed in fp32 -- within 1e-4 normwise"""
    from hierarchicalgnn_amd import _lib, fused
    lib = _lib.load()
    K, N = next((k, n) for n in (64, 128, 256) for k in (64, 128, 256)
                if lib.hgnn_mlp_backward_layer_supported_bf16(k, n))
    gen = torch.Generator().manual_seed(K + N + act)
    dz = torch.randn(R.M_ROWS, K, generator=gen).bfloat16().float()
    Wt = torch.randn(K, N, generator=gen) / K ** 0.5
    da_ref = dz.double() @ Wt.bfloat16().double()
    for name in ("r0", "r16"):
        rc = R.make_rows_case(name, N, seed=K, bf16=True)
        a_ref, dzp_ref, dgm, dbt, _ = _rows_ref(rc["z"], da_ref, rc["gamma"], rc["beta"], act, rc["eps"])
        args = (dz.cuda().bfloat16(), Wt.cuda(), rc["z"].cuda().bfloat16(), rc["gamma"].cuda(), rc["beta"].cuda(), act,
                rc["eps"])
        res = fused._bwd_layer(*args, want_a=True)
        assert all(torch.equal(x, y) for x, y in zip(res, fused._bwd_layer(*args, want_a=True)))
        tag = f"bwd_layer_bf16/{A.ACT_NAME[act]} (K={K}, N={N}) {name}"
        for what, got, ref in (("dz_prev", res[0], dzp_ref), ("a_prev", res[1], a_ref)):
            assert got.dtype == torch.bfloat16
            ratio = R.bf16_ratio(got.float().cpu().numpy(), ref.numpy())
            print(f"RATIO {tag} {what} bf16 {ratio:.3f}")
            assert ratio <= 1.0, (tag, what, ratio)
        for what, got, ref in (("dgamma", res[2], dgm), ("dbeta", res[3], dbt)):
            r = rel_err(got.double().cpu().numpy(), ref.numpy())
            print(f"RATIO {tag} {what} {r:.3g} / {BAR:.3g}")
            assert r <= BAR, (tag, what, r)


@pytest.mark.parametrize("cfg", ["L32x2_silu_elu", "L32x3_elu_leaky", "head64_silu"])
def test_training_round_trip_exact_fp32(cfg):
    """the differentiable fused MLP with the new codes: gradients of inputs, weights and biases against float64
    autograd (latent 32: ATen rows for the 32-wide layer, HIP row kernels for the 64-wide ones)"""
    from hierarchicalgnn_amd import fused
    case = A.case_for(A.F32_ACT_CONFIGS[cfg])
    net = net_of(case)
    segs, skip = segments_of(case)
    tabs = []
    for t, _ in segs:
        if not any(t is u for u in tabs):
            t.requires_grad_(True)
            tabs.append(t)
    assert fused.supported_train(net, segs, skip)
    lib0 = fused.stats["library_calls"]
    out = fused.fused_concat_mlp_train(net, segs, skip)
    wts = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).cuda()
    (out * wts).sum().backward()
    assert fused.stats["library_calls"] == lib0
    # float64 autograd on the CPU
    net64 = net_of(case).cpu().double()
    net64.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    t64 = [t.detach().cpu().double().requires_grad_(True) for t in tabs]
    lookup = {id(t): u for t, u in zip(tabs, t64)}
    x64 = torch.cat([lookup[id(t)] if i is None else lookup[id(t)][i.cpu()] for t, i in segs], dim=1)
    o64 = net64(x64)
    if skip is not None:
        o64 = o64 + lookup[id(skip)]
    (o64 * wts.cpu().double()).sum().backward()
    check_f32(f"train/{cfg} out", out, o64.detach().numpy())
    for t, u in zip(tabs, t64):
        assert rel_err(t.grad.double().cpu().numpy(), u.grad.numpy()) <= BAR
    for (name, p), q in zip(net.named_parameters(), net64.parameters()):
        r = rel_err(p.grad.double().cpu().numpy(), q.grad.numpy())
        print(f"RATIO train/{cfg} {name} {r:.3g}")
        assert r <= BAR, (cfg, name, r)
