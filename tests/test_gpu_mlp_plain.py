"""The LayerNorm-less route (``fused.set_plain_layers`` -> hgnn_mlp_forward_f32_plain, hgnn_act_rows_*) against the
float64 definition (tests/act_ref.py).  Without a LayerNorm nothing renormalises the rows, so the bar is normwise
against max|ref| plus ln_ref's element-wise form, at ``act_ref.PLAIN_BAR`` = 1e-4: sized from the k-ascending
fma-chain model in act_ref.py, proved at half of it by tests/test_act_ref.py.  Column sums and parameter gradients
(sums over rows): normwise."""
import numpy as np
import pytest
import torch

import act_ref as A
import ln_ref as R
from conftest import rel_err
from test_gpu_mlp_activations import check_f32, net_of, segments_of

pytestmark = pytest.mark.gpu
BAR = A.PLAIN_BAR
MS = (1, 64, R.M_ROWS)


@pytest.fixture
def plain():
    from hierarchicalgnn_amd import fused
    old = fused._plain_layers
    fused.set_plain_layers(True)
    yield fused
    fused.set_plain_layers(old)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("cfg", sorted(A.PLAIN_CONFIGS))
def test_plain_forward(cfg, M, plain):
    """every accepted family at its narrowest width: cells with two and three layers, heads (w = 1 and 8), small-K
    encoders, the narrow encoder (56 of 64 stored rows); SiLU, LeakyReLU, ELU, Sigmoid, GELU and Tanh"""
    fused = plain
    case = A.case_for(A.PLAIN_CONFIGS[cfg], plain=True, M=M)
    net = net_of(case)
    segs, skip = segments_of(case)
    assert fused._is_plain(fused._parse(net))
    with torch.no_grad():
        assert fused.supported(net, segs, skip)
        c0 = (fused.stats["plain_calls"], fused.stats["library_calls"])
        out = fused.fused_concat_mlp(net, segs, skip)
        again = fused.fused_concat_mlp(net, segs, skip)
        assert (fused.stats["plain_calls"], fused.stats["library_calls"]) == (c0[0] + 2, c0[1])
    assert torch.equal(out, again)
    check_f32(f"plain/{cfg}/M{M}", out, case["ref"].numpy())


def test_option_off_keeps_the_library_path():
    from hierarchicalgnn_amd import fused
    from hierarchicalgnn_amd.mlp import concat_mlp
    assert not fused._plain_layers_on()
    case = A.case_for(A.PLAIN_CONFIGS["L32x2_silu_tanh"], plain=True)
    net = net_of(case)
    segs, skip = segments_of(case)
    with torch.no_grad():
        assert not fused.supported(net, segs, skip) and not fused.supported_train(net, segs, skip)
        c0 = (fused.stats["plain_calls"], fused.stats["library_calls"])
        lib = concat_mlp(net, segs, skip)
        assert (fused.stats["plain_calls"], fused.stats["library_calls"]) == (c0[0], c0[1] + 1)
        with pytest.raises(RuntimeError, match="strict"), fused.options(strict=True):
            concat_mlp(net, segs, skip)
        with fused.options(plain_layers=True, strict=True):
            on = concat_mlp(net, segs, skip)
        assert (fused.stats["plain_calls"], fused.stats["library_calls"]) == (c0[0] + 1, c0[1] + 1)
        # bf16 rows without LayerNorm stay on the library path, counted there
        seg16 = [(t.bfloat16(), i) for t, i in segs]
        with fused.options(plain_layers=True):
            assert not fused.supported(net, seg16, seg16[-1][0])
            concat_mlp(net, seg16, seg16[-1][0])
        assert (fused.stats["plain_calls"], fused.stats["library_calls"]) == (c0[0] + 1, c0[1] + 2)
    check_f32("plain vs library", on, lib.double().cpu().numpy())


def test_narrow_encoder_trains_on_the_library_path(plain):
    """a last layer narrower than its storage that is no head has no dumps: no-grad it runs on the plain kernel, under
    autograd it is refused by the route and counted in library_calls"""
    from hierarchicalgnn_amd.mlp import concat_mlp
    fused = plain
    case = A.case_for(A.PLAIN_CONFIGS["narrow64_silu"], plain=True)
    net = net_of(case)
    segs, skip = segments_of(case)
    with torch.no_grad():
        assert fused.supported(net, segs, skip)
    assert not fused.supported_train(net, segs, skip)
    c0 = (fused.stats["plain_calls"], fused.stats["library_calls"])
    out = concat_mlp(net, segs, skip)
    assert out.requires_grad
    assert (fused.stats["plain_calls"], fused.stats["library_calls"]) == (c0[0], c0[1] + 1)
    check_f32("plain/narrow64 library training forward", out, case["ref"].numpy())
    # the same shape with a plain last Linear wider than a head's: refused in training as well, not raised at the launch
    lin = torch.nn.Linear(128, 56).cuda()
    net2 = torch.nn.Sequential(*list(net)[:4], lin)
    assert fused._is_plain(fused._parse(net2)) and not fused.supported_train(net2, segs, None)
    assert concat_mlp(net2, segs, None).shape == (R.M_ROWS, 56)


def test_save_pre_dumps_are_the_pre_activation_rows(plain):
    fused = plain
    for cfg in ("L32x3_elu_leaky", "L64x2_leaky_silu", "head64_silu"):
        case = A.case_for(A.PLAIN_CONFIGS[cfg], plain=True)
        net = net_of(case)
        segs, skip = segments_of(case)
        assert fused.supported_train(net, segs, skip)
        out = fused.fused_concat_mlp_train(net, segs, skip)
        check_f32(f"plain/{cfg} train out", out, case["ref"].numpy())
        n_dump = sum(1 for l, lay in enumerate(case["layers"]) if lay[4] != 0 or l < len(case["layers"]) - 1)
        zs = list(out.grad_fn.saved_tensors)[-n_dump:]
        for l, z in enumerate(zs):
            check_f32(f"plain/{cfg} z{l}", z, case["zs"][l].numpy())


@pytest.mark.parametrize("W", [64, 1024])
@pytest.mark.parametrize("act", (R.ACT_GELU, R.ACT_TANH) + A.NEW_CODES)
def test_act_rows_entries(act, W, plain):
    fused = plain
    z, g = A.tiny_rows(W)
    a_ref = A.act64(z, act)
    dz_ref = g.double() * A.act_grad64(z, act)
    zd, gd = z.cuda(), g.cuda()
    out = fused._act_rows_forward(zd, act)
    dz, dbias = fused._act_rows_backward(zd, gd, act)
    dz2, dbias2 = fused._act_rows_backward(zd, gd, act)
    assert torch.equal(out, fused._act_rows_forward(zd, act)) and torch.equal(dz, dz2) and torch.equal(dbias, dbias2)
    tag = f"act_rows/{A.ACT_NAME[act]}/W{W}"
    check_f32(tag + " out", out, a_ref.numpy())
    check_f32(tag + " dz", dz, dz_ref.numpy())
    r = rel_err(dbias.double().cpu().numpy(), dz_ref.sum(0).numpy())
    print(f"RATIO {tag} dbias {r:.3g}")
    assert r <= BAR
    if act == A.ACT_ELU:      # the cancelling range, relatively
        n = 30
        got, ref = out[0, :n].double().cpu().numpy(), a_ref[0, :n].numpy()
        assert float((np.abs(got - ref) / np.abs(ref)).max()) <= 16 * A.U
    # M = 0: nothing launched forward, zero column sums backward
    e = torch.empty((0, W), device="cuda")
    assert fused._act_rows_forward(e, act).shape == (0, W)
    assert float(fused._act_rows_backward(e, e, act)[1].abs().max()) == 0.0


@pytest.mark.parametrize("cfg", ["L32x3_elu_leaky", "L64x2_leaky_silu", "head64_tanh_w8", "enc6_elu"])
def test_training_round_trip(cfg, plain):
    """loss = sum(out * fixed weights): gradients of inputs, weights and biases against float64 autograd"""
    fused = plain
    case = A.case_for(A.PLAIN_CONFIGS[cfg], plain=True)
    net = net_of(case)
    segs, skip = segments_of(case)
    tabs = [t.requires_grad_(True) for t, _ in segs]
    assert fused.supported_train(net, segs, skip)
    c0 = (fused.stats["plain_calls"], fused.stats["library_calls"])
    out = fused.fused_concat_mlp_train(net, segs, skip)
    wts = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).cuda()
    (out * wts).sum().backward()
    assert (fused.stats["plain_calls"], fused.stats["library_calls"]) == (c0[0] + 1, c0[1])
    net64 = net_of(case).cpu().double()
    t64 = [t.detach().cpu().double().requires_grad_(True) for t in tabs]
    x64 = torch.cat([u if i is None else u[i.cpu()] for u, (_, i) in zip(t64, segs)], dim=1)
    o64 = net64(x64)
    if skip is not None:
        o64 = o64 + t64[-1]
    (o64 * wts.cpu().double()).sum().backward()
    check_f32(f"plain train/{cfg} out", out, o64.detach().numpy())
    for s, (t, u) in enumerate(zip(tabs, t64)):
        r = rel_err(t.grad.double().cpu().numpy(), u.grad.numpy())
        print(f"RATIO plain train/{cfg} table{s} {r:.3g}")
        assert r <= BAR
    for (name, p), q in zip(net.named_parameters(), net64.parameters()):
        r = rel_err(p.grad.double().cpu().numpy(), q.grad.numpy())
        print(f"RATIO plain train/{cfg} {name} {r:.3g}")
        assert r <= BAR, (cfg, name, r)
