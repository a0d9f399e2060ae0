"""GPU parity of the fused fp32 MLP at hidden = output (``hgnn_mlp_forward_f32_square``: the exact kernel's square
instantiations, zero-padded parameters between the grid widths) and at 1 and 4 to 8 layers (groups of at most three
layers): forward against the CPU oracle, small-K encoders and the narrow last layer, LayerNorm conformance under row
offset / scale / eps (tests/ln_ref.py, the bars and the report of tests/test_gpu_mlp_layernorm.py), the training round
trip against autograd through the library path, depth, checkpointed cells, whole models under ``strict``, and the
routes that must not change.

Every test asserts that the square route is what ran (``fused._route(...).entry`` and the ``square_calls`` /
``fused_calls`` / ``fused_train_calls`` counters).  The bar is the project's fp32 bar, 1e-4, everywhere.

Worst measured error / bar of the conformance entries on an MI355X (the case and quantity that set it): h = 128 x 3
layers (grid) 0.22 (r256, normwise), h = 96 x 2 layers (padded to 128) 0.32 (r16 and r64, element-wise)."""
import json
import os

import pytest
import torch

import conftest
import ln_ref as R
from conftest import rel_err
from test_gpu_mlp_layernorm import _nominal, _net, _Report, _segments

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _mk(in_w, hidden, out, layers, out_act, seed, hidden_act="GELU"):
    from hierarchicalgnn_amd import make_mlp
    torch.manual_seed(seed)
    net = make_mlp(in_w, hidden, out, layers, layer_norm=True, output_activation=out_act, hidden_activation=hidden_act)
    for p in net.parameters():  # non-trivial LayerNorm affine / biases
        if p.dim() == 1:
            p.data.add_(0.2 * torch.randn_like(p))
    return net


def _counts():
    from hierarchicalgnn_amd import fused
    return fused.stats["fused_calls"], fused.stats["square_calls"], fused.stats["fused_train_calls"], \
        fused.stats["library_calls"]


def _square_forward(net, segs, skip, launches=1, square=None):
    """two no-grad calls on the square route (asserted): (out, again).  ``launches``: groups of a deep network, of
    which ``square`` (default: all) are launches of the square entry"""
    from hierarchicalgnn_amd import fused
    with torch.no_grad():
        assert fused.supported(net, segs, skip)
        r = fused._route(net, segs, skip, train=False)
        assert r.entry == "f32_square" and not r.chain and len(r.groups) == (launches if launches > 1 else 0)
        c0 = _counts()
        out = fused.fused_concat_mlp(net, segs, skip)
        c1 = _counts()
        assert (c1[0] - c0[0], c1[1] - c0[1], c1[3] - c0[3]) == (launches, launches if square is None else square, 0)
        again = fused.fused_concat_mlp(net, segs, skip)
    return out, again


def _cpu_segments(L, nseg, M, g, gather=True, n_tab=97):
    table = torch.randn(n_tab, L, generator=g)
    idx0 = torch.randint(0, n_tab, (M,), generator=g)
    idx1 = torch.randint(0, n_tab, (M,), generator=g)
    direct = torch.randn(M, L, generator=g)
    if gather:
        segs = [(table, idx0), (table, idx1), (direct, None)][3 - nseg:]
    else:
        segs = [(torch.randn(M, L, generator=g), None) for _ in range(nseg - 1)] + [(direct, None)]
    return segs, direct


def _cat(segs_cpu):
    return torch.cat([t if i is None else t[i] for t, i in segs_cpu], dim=1)


def _cuda(segs_cpu):
    return [(t.cuda(), None if i is None else i.cuda()) for t, i in segs_cpu]


# h on the grid {32, 64, 128, 256} and padded {48, 96, 192}, each in 2 and 3 layers; M in {1, 63, 65, 193}; 1, 2 and 3
# segments with and without gather; with and without skip; Tanh and GELU outputs; one SiLU-hidden case (compile-time
# codes) and one ReLU-hidden case (the runtime switch)
FORWARD = [
    # h, layers, nseg, gather, M, out_act, skip, hidden_act
    (32, 2, 3, True, 193, "Tanh", True, "GELU"), (32, 3, 1, False, 1, "GELU", False, "GELU"),
    (64, 2, 3, True, 65, "Tanh", True, "GELU"), (64, 3, 2, True, 63, "GELU", True, "GELU"),
    (128, 2, 2, False, 63, "GELU", False, "GELU"), (128, 3, 3, True, 193, "Tanh", True, "GELU"),
    (256, 2, 3, True, 65, "Tanh", True, "GELU"), (256, 3, 2, True, 193, "GELU", True, "GELU"),
    (48, 2, 3, True, 193, "Tanh", True, "GELU"), (48, 3, 1, False, 63, "GELU", True, "GELU"),
    (96, 2, 3, False, 65, "GELU", False, "GELU"), (96, 3, 3, True, 1, "Tanh", True, "GELU"),
    (192, 2, 2, True, 63, "Tanh", True, "GELU"), (192, 3, 3, True, 65, "GELU", True, "GELU"),
    (64, 2, 3, True, 193, "Tanh", True, "SiLU"), (128, 3, 3, True, 65, "SiLU", True, "SiLU"),
    (64, 3, 3, True, 193, "Tanh", True, "ReLU"), (96, 2, 3, True, 193, "Tanh", True, "ReLU"),
]


@pytest.mark.parametrize("h,layers,nseg,gather,M,out_act,skip,hid_act", FORWARD)
def test_square_mlp_vs_oracle(h, layers, nseg, gather, M, out_act, skip, hid_act):
    from oracle import hgnn_oracle as O
    g = torch.Generator().manual_seed(h * 10 + layers + nseg)
    net = _mk(nseg * h, h, h, layers, out_act, seed=h + layers, hidden_act=hid_act)
    segs_cpu, direct = _cpu_segments(h, nseg, M, g, gather)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    ref = O.mlp_apply(sd, "", _cat(segs_cpu), layers, hid_act, out_act, True) + (direct if skip else 0)
    net = net.cuda()
    segs = _cuda(segs_cpu)
    out, again = _square_forward(net, segs, segs[-1][0] if skip else None)
    assert out.shape == ref.shape
    assert rel_err(out.cpu().numpy(), ref.numpy()) <= TOL
    assert torch.equal(out, again)


@pytest.mark.parametrize("h,layers", [(64, 2), (96, 3), (128, 3), (192, 2)])
def test_square_preprojected_segments_equal_the_full_k_kernel(h, layers):
    """hgnn_mlp_desc.n_pre on the square route: between the grid widths the projections are [rows, P] with zero padded
    columns; both forms against the oracle"""
    from hierarchicalgnn_amd import fused
    from oracle import hgnn_oracle as O
    g = torch.Generator().manual_seed(7 * h + layers)
    out_act = "Tanh" if layers == 2 else "GELU"
    net = _mk(3 * h, h, h, layers, out_act, seed=h + 1)
    segs_cpu, direct = _cpu_segments(h, 3, 1777, g, n_tab=101)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    ref = O.mlp_apply(sd, "", _cat(segs_cpu), layers, "GELU", out_act, True) + direct
    net, segs = net.cuda(), _cuda(segs_cpu)
    skip = segs[-1][0]
    try:
        for on in (True, False):
            fused.set_preproject(on)
            with torch.no_grad():
                d = fused._descriptor(net, segs, skip, "f32_square")[0]
            assert int(d.n_pre) == (2 if on else 0) and int(d.n_seg) == (1 if on else 3)
            out = _square_forward(net, segs, skip)[0]
            assert rel_err(out.cpu().numpy(), ref.numpy()) <= TOL
    finally:
        fused.set_preproject(True)


@pytest.mark.parametrize("kind", ["node_enc", "edge_enc", "narrow"])
@pytest.mark.parametrize("h", [64, 96])
def test_square_encoders_and_the_narrow_last_layer(kind, h):
    """small-K encoders 3 -> h -> h -> h and 6 -> h -> h (gathered 12-byte rows) and the supernode encoder
    h -> h -> h -> h - 8 (64 -> 56, 96 -> 88)"""
    from hierarchicalgnn_amd import make_mlp
    from oracle import hgnn_oracle as O
    g = torch.Generator().manual_seed(len(kind) + h)
    N, M = 300, 333
    torch.manual_seed(7 + h)
    x3 = torch.rand(N, 3, generator=g) * 2 - 1
    i0 = torch.randint(0, N, (M,), generator=g)
    i1 = torch.randint(0, N, (M,), generator=g)
    rows = torch.randn(M, h, generator=g)
    if kind == "node_enc":
        net, segs_cpu, layers = make_mlp(3, h, h, 3, layer_norm=True, output_activation="GELU"), [(x3, None)], 3
    elif kind == "edge_enc":
        net, segs_cpu, layers = make_mlp(6, h, h, 2, layer_norm=True, output_activation="GELU"), [(x3, i0), (x3, i1)], 2
    else:
        net, segs_cpu, layers = make_mlp(h, h, h - 8, 3, layer_norm=True, output_activation="GELU"), [(rows, None)], 3
    for p in net.parameters():
        if p.dim() == 1:
            p.data.add_(0.2 * torch.randn_like(p))
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    ref = O.mlp_apply(sd, "", _cat(segs_cpu), layers, "GELU", "GELU", True)
    out, again = _square_forward(net.cuda(), _cuda(segs_cpu), None)
    assert out.shape == ref.shape
    assert rel_err(out.cpu().numpy(), ref.numpy()) <= TOL
    assert torch.equal(out, again)


def test_narrow_square_encoder_trains_on_the_library_path():
    from hierarchicalgnn_amd import fused, make_mlp, mlp
    net = make_mlp(64, 64, 56, 3, layer_norm=True, output_activation="GELU").cuda()
    x = torch.randn(40, 64, device="cuda").requires_grad_(True)
    assert not fused.supported_train(net, [(x, None)], None)
    c0 = _counts()
    mlp.concat_mlp(net, [(x, None)]).sum().backward()
    c1 = _counts()
    assert (c1[2] - c0[2], c1[3] - c0[3]) == (0, 1)
    with torch.no_grad():
        assert fused.supported(net, [(x.detach(), None)], None)


def test_bf16_rows_stay_on_the_library_path():
    from hierarchicalgnn_amd import fused, mlp
    net = _mk(64, 64, 64, 2, "GELU", seed=1).cuda()
    x = torch.randn(70, 64, device="cuda").bfloat16()
    c0 = _counts()
    with torch.no_grad():
        assert not fused.supported(net, [(x, None)], None)
        y = mlp.concat_mlp(net, [(x, None)])
    c1 = _counts()
    assert y.dtype == torch.bfloat16 and (c1[1] - c0[1], c1[3] - c0[3]) == (0, 1)


def test_square_option_switches_the_route_off():
    from hierarchicalgnn_amd import fused
    net = _mk(64, 64, 64, 2, "GELU", seed=1).cuda()
    x = torch.randn(70, 64, device="cuda")
    with torch.no_grad():
        assert fused.supported(net, [(x, None)], None)
        with fused.options(square=False):
            assert not fused.supported(net, [(x, None)], None)


def test_split3_marked_module_runs_the_exact_kernel():
    """a module marked for split-bf16 GEMMs (``fp32_gemm: split_bf16``) at hidden = latent = 256, 128-aligned segments"""
    from hierarchicalgnn_amd import fused
    from oracle import hgnn_oracle as O
    g = torch.Generator().manual_seed(5)
    net = _mk(768, 256, 256, 3, "GELU", seed=2)
    segs_cpu, direct = _cpu_segments(256, 3, 130, g)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    ref = O.mlp_apply(sd, "", _cat(segs_cpu), 3, "GELU", "GELU", True) + direct
    net = net.cuda()
    net._hgnn_split3 = True
    segs = _cuda(segs_cpu)
    n0 = fused.stats.get("split3_calls", 0)
    out, again = _square_forward(net, segs, segs[-1][0])
    assert fused.stats.get("split3_calls", 0) == n0
    assert rel_err(out.cpu().numpy(), ref.numpy()) <= TOL and torch.equal(out, again)


CONFORMANCE = {
    "h128x3": dict(widths=[384, 128, 128, 128]),
    "h96x2": dict(widths=[288, 96, 96]),
}


@pytest.mark.parametrize("cfg", sorted(CONFORMANCE))
def test_square_layernorm_conformance(cfg):
    """row offset, scale, eps and constant rows (ln_ref.CASES): one grid configuration (no padded feature) and one padded
    one (32 masked features in every layer).

    Worst measured error / bar on an MI355X (the case and quantity that set it): h128x3 0.22 (r256, normwise), h96x2
    0.32 (r16 / r64, element-wise); the report this test prints (``RATIO`` lines) has every case."""
    rep = _Report(f"{cfg}/square")
    for name in R.CASES:
        case = R.case_for(CONFORMANCE[cfg], name)
        segs, skip = _segments(case)
        out, again = _square_forward(_net(case), segs, skip)
        rep.f32_rows(name, "out", out, case["ref"].numpy(), _nominal(case), case["const_rows"])
        rep.same(name, out, again)
    rep.done()


@pytest.mark.parametrize("h,layers", [(64, 2), (96, 3), (128, 3)])
def test_square_train_backward_matches_autograd(h, layers):
    """the differentiable variant on the square route (dumps at the real widths + the hand-written backward on the
    unpadded parameters) against autograd through the library path: outputs and every gradient"""
    from hierarchicalgnn_amd import fused, mlp
    g = torch.Generator().manual_seed(h + layers)
    out_act = "Tanh" if layers == 2 else "GELU"
    net = _mk(3 * h, h, h, layers, out_act, seed=h).cuda()
    n_tab, M = 83, 500
    table0 = torch.randn(n_tab, h, generator=g).cuda()
    direct0 = torch.randn(M, h, generator=g).cuda()
    i0 = torch.randint(0, n_tab, (M,), generator=g).cuda()
    i1 = torch.randint(0, n_tab, (M,), generator=g).cuda()
    r = torch.randn(M, h, generator=g).cuda()
    results = {}
    try:
        for name, on in (("fused", True), ("library", False)):
            fused.set_enabled(True, train=on)
            net.zero_grad(set_to_none=True)
            table = table0.clone().requires_grad_(True)
            direct = direct0.clone().requires_grad_(True)
            segs = [(table, i0), (table, i1), (direct, None)]
            assert fused.supported_train(net, segs, direct) == on
            if on:
                assert fused._route(net, segs, direct, train=True).entry == "f32_square"
            c0 = _counts()
            out = mlp.concat_mlp(net, segs, skip=direct)
            c1 = _counts()
            assert (c1[2] - c0[2], c1[1] - c0[1], c1[3] - c0[3]) == ((1, 1, 0) if on else (0, 0, 1))
            (out * r).sum().backward()
            results[name] = [out.detach(), table.grad, direct.grad] + [p.grad.clone() for p in net.parameters()]
    finally:
        fused.set_enabled(True)
    for a, b in zip(results["fused"], results["library"]):
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) <= TOL


def _groups(n):
    return 1 if n <= 3 else (n - 1) // 3 + 1


@pytest.mark.parametrize("n", [1, 4, 5, 7])
@pytest.mark.parametrize("ratio", [1, 2])
def test_depth_vs_oracle(n, ratio):
    """make_mlp(3L, h, L, n) at L = 64 with h = L and h = 2L: one launch per group of at most three layers"""
    from oracle import hgnn_oracle as O
    L = 64
    h = ratio * L
    g = torch.Generator().manual_seed(n * 3 + ratio)
    net = _mk(3 * L, h, L, n, "Tanh", seed=n + ratio)
    segs_cpu, direct = _cpu_segments(L, 3, 193, g)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    ref = O.mlp_apply(sd, "", _cat(segs_cpu), n, "GELU", "Tanh", True) + direct
    net, segs = net.cuda(), _cuda(segs_cpu)
    # the last group of h = 2L: one layer 128 -> 64 (square entry), two or three layers 128 -> (128 ->) 128 -> 64 (grid)
    n_last = n - 3 * (_groups(n) - 1)
    square = _groups(n) if (ratio == 1 or n_last == 1) else _groups(n) - 1
    out, again = _square_forward(net, segs, segs[-1][0], launches=_groups(n), square=square)
    assert out.shape == ref.shape
    assert rel_err(out.cpu().numpy(), ref.numpy()) <= TOL
    assert torch.equal(out, again)


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("ratio", [1, 2])
def test_depth_train_backward_matches_autograd(n, ratio):
    """each group its own differentiable call: ``fused_train_calls`` grows by the number of groups"""
    from hierarchicalgnn_amd import fused, mlp
    L = 64
    h = ratio * L
    g = torch.Generator().manual_seed(n + ratio)
    net = _mk(3 * L, h, L, n, "Tanh", seed=n).cuda()
    n_tab, M = 83, 500
    table0 = torch.randn(n_tab, L, generator=g).cuda()
    direct0 = torch.randn(M, L, generator=g).cuda()
    i0 = torch.randint(0, n_tab, (M,), generator=g).cuda()
    i1 = torch.randint(0, n_tab, (M,), generator=g).cuda()
    r = torch.randn(M, L, generator=g).cuda()
    results = {}
    try:
        for name, on in (("fused", True), ("library", False)):
            fused.set_enabled(True, train=on)
            net.zero_grad(set_to_none=True)
            table = table0.clone().requires_grad_(True)
            direct = direct0.clone().requires_grad_(True)
            segs = [(table, i0), (table, i1), (direct, None)]
            assert fused.supported_train(net, segs, direct) == on
            c0 = _counts()
            out = mlp.concat_mlp(net, segs, skip=direct)
            c1 = _counts()
            assert (c1[2] - c0[2], c1[3] - c0[3]) == ((_groups(n), 0) if on else (0, 1))
            (out * r).sum().backward()
            results[name] = [out.detach(), table.grad, direct.grad] + [p.grad.clone() for p in net.parameters()]
    finally:
        fused.set_enabled(True)
    for a, b in zip(results["fused"], results["library"]):
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) <= TOL


def test_deep_head_and_what_stays_on_the_library_path():
    """five LayerNorm'ed layers ending in a plain 1-wide Linear run as groups + a product over the hidden rows; a hidden
    width that changes along the network, nine layers and a width above 256 stay on the library path"""
    from hierarchicalgnn_amd import fused, make_mlp
    from oracle import hgnn_oracle as O
    g = torch.Generator().manual_seed(11)
    net = make_mlp(128, 64, 1, 6, layer_norm=True, output_activation=None, hidden_activation="GELU")
    x = torch.randn(130, 128, generator=g)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    ref = O.mlp_apply(sd, "", x, 6, "GELU", None, True)
    net, xc = net.cuda(), x.cuda()
    with torch.no_grad():
        r = fused._route(net, [(xc, None)], None, train=False)
        assert r is not None and r.head and len(r.groups) == 2
        c0 = _counts()
        out = fused.fused_concat_mlp(net, [(xc, None)], None)
        c1 = _counts()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 2)
    assert rel_err(out.cpu().numpy(), ref.numpy()) <= TOL
    mods = list(_mk(64, 64, 64, 2, "GELU", seed=1)) + list(_mk(64, 128, 64, 3, "GELU", seed=2))
    mixed = torch.nn.Sequential(*mods).cuda()
    x64 = torch.randn(10, 64, device="cuda")
    with torch.no_grad():
        assert not fused.supported(mixed, [(x64, None)], None)
        assert not fused.supported(_mk(64, 64, 64, 9, "GELU", seed=3).cuda(), [(x64, None)], None)
        assert not fused.supported(_mk(64, 272, 272, 4, "GELU", seed=3).cuda(), [(x64, None)], None)


@pytest.mark.parametrize("kind", ["ignn", "hgnn"])
def test_checkpointed_cells_at_hidden_equal_latent(kind):
    """an InteractionGNNCell and a HierarchicalGNNCell at latent = hidden = 64 through torch.utils.checkpoint: the
    no-grad first pass and the recompute under autograd both run the square kernel; outputs and gradients against the
    library path"""
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import fused, synth
    torch.manual_seed(3)
    L = 64
    hp = dict(latent=L, hidden=L, nb_edge_layer=2, nb_node_layer=3, layernorm=True, hidden_activation="GELU",
              checkpointing=True)
    _, ei = synth.trackml_event(600, 3000, seed=4)
    graph = synth.directed(ei).cuda()
    nodes0 = torch.randn(600, L, device="cuda")
    edges0 = torch.randn(graph.shape[1], L, device="cuda")
    if kind == "ignn":
        cell = H.InteractionGNNCell(hp).cuda()
        inputs0 = [nodes0, edges0]
        extra = (graph,)
    else:
        cell = H.HierarchicalGNNCell(hp).cuda()
        S = 40
        bg, bw = synth.bipartite_assignment(600, S, 5, seed=2)
        sg, sw = synth.super_graph(S, 10, seed=2)
        inputs0 = [nodes0, edges0, torch.randn(S, L, device="cuda"), torch.randn(sg.shape[1], L, device="cuda")]
        extra = (graph, bg.cuda(), bw.cuda(), sg.cuda(), sw.cuda())
    rs = [torch.randn_like(t) for t in inputs0]
    results = {}
    try:
        for name, on in (("fused", True), ("library", False)):
            fused.set_enabled(on)
            cell.zero_grad(set_to_none=True)
            inputs = [t.clone().requires_grad_(True) for t in inputs0]
            c0 = _counts()
            outs = cell(*inputs, *extra)
            c1 = _counts()
            sum((o * r).sum() for o, r in zip(outs, rs)).backward()
            c2 = _counts()
            if on:
                n_mlp = c1[0] - c0[0]
                assert n_mlp >= 2 and c1[1] - c0[1] == n_mlp             # no-grad first pass: every network, square
                assert (c2[2] - c1[2], c2[1] - c1[1]) == (n_mlp, n_mlp)   # recompute under autograd
                assert c2[3] == c0[3]
            else:
                assert c2[:3] == c0[:3]
            results[name] = [o.detach() for o in outs] + [t.grad for t in inputs] + \
                [p.grad.clone() for p in cell.parameters()]
    finally:
        fused.set_enabled(True)
    for a, b in zip(results["fused"], results["library"]):
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) <= TOL


def _raw(name, **over):
    with open(os.path.join(conftest.GOLDEN, "ref_configs.json")) as f:
        return dict(json.load(f)[name]["raw"], **over)


def _event():
    from hierarchicalgnn_amd import synth
    x, ei = synth.trackml_event(600, 3000, seed=5)
    return x.cuda(), ei.cuda()


def _strict_vs_disabled(forward):
    """``forward()`` under strict (no library call, nothing raised) against the same model with the fused kernels off"""
    from hierarchicalgnn_amd import fused
    c0 = _counts()
    with fused.options(strict=True), torch.no_grad():
        s = forward()
    c1 = _counts()
    assert c1[3] == c0[3] and c1[1] > c0[1] and c1[0] > c0[0]
    fused.set_enabled(False)
    try:
        with torch.no_grad():
            ref = forward()
    finally:
        fused.set_enabled(True)
    assert bool(torch.isfinite(s).all())
    assert rel_err(s.cpu().numpy(), ref.cpu().numpy()) <= TOL


def test_ec_in_at_hidden_ratio_1_and_four_node_layers_has_no_library_mlp():
    from hierarchicalgnn_amd.models import EC_InteractionGNN
    torch.manual_seed(0)
    hp = _raw("EC-IN", hidden="ratio", hidden_ratio=1, latent=32, nb_node_layer=4, n_interaction_graph_iters=2)
    model = EC_InteractionGNN(hp).cuda().eval()
    x, ei = _event()
    _strict_vs_disabled(lambda: model(x, ei))


def test_bc_hgnn_gmm_at_hidden_ratio_1_has_no_library_mlp():
    from hierarchicalgnn_amd import synth
    from hierarchicalgnn_amd.models import BC_MessagePassing
    torch.manual_seed(0)
    hp = _raw("BC-HGNN-GMM", hidden="ratio", hidden_ratio=1, latent=64, emb_dim=8, n_interaction_graph_iters=1,
              n_hierarchical_graph_iters=1)
    model = BC_MessagePassing(hp).cuda().eval()
    x, ei = _event()
    bg, bw = synth.bipartite_assignment(600, 40, 5, seed=2)
    sg, sw = synth.super_graph(40, 10, seed=2)
    means = torch.nn.functional.normalize(torch.randn(40, 8)).cuda()

    def forward():
        directed, emb, nodes, edges, _ = model.embed(x, ei)
        n_out, sn_out, _, _ = model.hgnn_block(nodes, edges, directed, means, bg.cuda(), bw.cuda(), sg.cuda(), sw.cuda())
        return model.score(n_out, sn_out, bg.cuda())

    _strict_vs_disabled(forward)


def test_existing_routes_are_unchanged():
    """one shape each of the grid entry, the padded entry and the latent-512 chain keeps entry and ``chain`` flag"""
    from hierarchicalgnn_amd import fused
    x = lambda w: [(torch.randn(10, w, device="cuda"), None)]   # noqa: E731
    with torch.no_grad():
        r = fused._route(_mk(192, 128, 64, 3, "GELU", seed=1).cuda(), x(192), None, train=False)
        assert (r.entry, r.chain, r.groups) == ("f32", False, ())
        r = fused._route(_mk(288, 192, 96, 2, "GELU", seed=1).cuda(), x(288), None, train=False)
        assert (r.entry, r.chain, r.groups) == ("f32_padded", False, ())
        r = fused._route(_mk(512, 1024, 512, 3, "GELU", seed=1).cuda(), x(512), None, train=False)
        assert (r.entry, r.chain, r.groups) == ("f32", True, ())
        assert fused._route(_mk(192, 64, 40, 2, "GELU", seed=1).cuda(), x(192), None, train=False) is None
    xg = [(torch.randn(10, 192, device="cuda").requires_grad_(True), None)]
    r = fused._route(_mk(192, 128, 64, 3, "GELU", seed=1).cuda(), xg, None, train=True)
    assert (r.entry, r.train) == ("f32", True)
    xg = [(torch.randn(10, 288, device="cuda").requires_grad_(True), None)]
    r = fused._route(_mk(288, 192, 96, 2, "GELU", seed=1).cuda(), xg, None, train=True)
    assert (r.entry, r.train) == ("f32_padded", True)
