"""GPU parity of the fused fp32 MLP at the widths BETWEEN the template grid's (``hgnn_mlp_forward_f32_padded``: zero-padded
parameters on the next grid instantiation, LayerNorm statistics masked to the real features, rows in HBM at their real
widths): forward against the CPU oracle, LayerNorm conformance under row offset / scale / eps (tests/ln_ref.py, the bars
and the report of tests/test_gpu_mlp_layernorm.py), encoders and heads, pre-projection on / off, the training round trip
against autograd through the library path, and whole models at latent 96.

Every test asserts that the padded route is what ran (``fused.supported`` and the ``padded_calls`` / ``fused_calls`` /
``fused_train_calls`` counters).  The bar is the project's fp32 bar, 1e-4, everywhere (tests/test_mlp_padded_ref.py
proves that masked statistics on padded parameters stay within half of it on every conformance case).

Worst measured error / bar of the conformance entries on an MI355X (the case and quantity that set it): latent 96 x 2
layers 0.28 (s+8_r64, element-wise), latent 144 x 3 layers 0.28 (r16, element-wise), head H = 192 0.29 (r256, normwise),
narrow encoder 96 -> 192 -> 192 -> 88 0.38 (r256, normwise).  With mean = sum * (1 / n) instead of sum / n the
const_c256 case of latent 144 x 3 was at 1.29: 1 / 288 is rounded, the mean of an exactly constant row is then off by
an ulp."""
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
    return fused.stats["fused_calls"], fused.stats["padded_calls"], fused.stats["fused_train_calls"]


def _padded_forward(net, segs, skip):
    """two no-grad calls on the padded route (asserted): (out, again)"""
    from hierarchicalgnn_amd import fused
    with torch.no_grad():
        assert fused.supported(net, segs, skip)
        assert fused._route(net, segs, skip, train=False).entry == "f32_padded"
        c0 = _counts()
        out = fused.fused_concat_mlp(net, segs, skip)
        c1 = _counts()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 1)
        again = fused.fused_concat_mlp(net, segs, skip)
    return out, again


# (L, h): every pair of the list in 2 and 3 layers; 1, 2 and 3 segments, M in {1, 63, 65, 193}, Tanh / GELU outputs, with
# and without skip spread over them; one ReLU-hidden case (activations read from the descriptor at run time)
FORWARD = [
    (16, 32, 2, 3, 193, "Tanh", True, "GELU"), (16, 32, 3, 1, 1, "GELU", False, "GELU"),
    (48, 96, 2, 3, 65, "Tanh", True, "GELU"), (48, 96, 3, 2, 63, "GELU", True, "GELU"),
    (96, 192, 2, 3, 193, "Tanh", True, "GELU"), (96, 192, 3, 3, 65, "GELU", False, "GELU"),
    (96, 192, 2, 3, 193, "Tanh", True, "ReLU"), (96, 192, 2, 1, 63, "GELU", True, "GELU"),
    (144, 288, 2, 3, 63, "Tanh", True, "GELU"), (144, 288, 3, 2, 193, "GELU", True, "GELU"),
    (240, 480, 2, 3, 65, "Tanh", False, "GELU"), (240, 480, 3, 3, 63, "GELU", True, "GELU"),
    (64, 192, 2, 3, 193, "Tanh", True, "GELU"), (64, 192, 3, 1, 65, "GELU", True, "GELU"),
    (128, 512, 2, 2, 63, "GELU", False, "GELU"), (128, 512, 3, 3, 1, "Tanh", True, "GELU"),
]


@pytest.mark.parametrize("L,h,layers,nseg,M,out_act,skip,hid_act", FORWARD)
def test_padded_mlp_vs_oracle(L, h, layers, nseg, M, out_act, skip, hid_act):
    from oracle import hgnn_oracle as O
    g = torch.Generator().manual_seed(L * 10 + layers + h)
    net = _mk(nseg * L, h, L, layers, out_act, seed=L + layers, hidden_act=hid_act)
    n_tab = 97
    table = torch.randn(n_tab, L, generator=g)
    idx0 = torch.randint(0, n_tab, (M,), generator=g)
    idx1 = torch.randint(0, n_tab, (M,), generator=g)
    direct = torch.randn(M, L, generator=g)
    segs_cpu = [(table, idx0), (table, idx1), (direct, None)][3 - nseg:]
    x = torch.cat([t if i is None else t[i] for t, i in segs_cpu], dim=1)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    ref = O.mlp_apply(sd, "", x, layers, hid_act, out_act, True) + (direct if skip else 0)
    net = net.cuda()
    segs = [(t.cuda(), None if i is None else i.cuda()) for t, i in segs_cpu]
    out, again = _padded_forward(net, segs, segs[-1][0] if skip else None)
    assert out.shape == ref.shape
    assert rel_err(out.cpu().numpy(), ref.numpy()) <= TOL
    assert torch.equal(out, again)


CONFORMANCE = {
    "L96x2": dict(widths=[288, 192, 96]),
    "L144x3": dict(widths=[432, 288, 288, 144]),
    "head192": dict(widths=[192, 192, 192], nseg=2, skip=False, acts=[R.ACT_GELU, R.ACT_GELU], head=1),
    "narrow88": dict(widths=[96, 192, 192, 88], nseg=1, skip=False),
}


@pytest.mark.parametrize("cfg", sorted(CONFORMANCE))
def test_padded_layernorm_conformance(cfg):
    """row offset, scale, eps and constant rows (ln_ref.CASES) on the masked statistics: 64 (L96), 224 (L144) padded
    features in the hidden layers, 32 / 112 / 40 in the last"""
    rep = _Report(f"{cfg}/padded")
    for name in R.CASES:
        case = R.case_for(CONFORMANCE[cfg], name)
        segs, skip = _segments(case)
        out, again = _padded_forward(_net(case), segs, skip)
        rep.f32_rows(name, "out", out, case["ref"].numpy(), _nominal(case), case["const_rows"])
        rep.same(name, out, again)
    rep.done()


@pytest.mark.parametrize("kind", ["node_enc", "edge_enc", "supernode_enc", "emb_head", "score_head"])
def test_padded_encoders_and_heads(kind):
    """small-K encoders 3 -> 192 -> 192 -> 96 and 6 -> 192 -> 96 (gathered 12-byte rows), the supernode encoder
    96 -> 192 -> 192 -> 88, the embedding head 96 -> 192 -> 192 -> 8 and the width-1 head 192 -> 192 -> 192 -> 1"""
    from hierarchicalgnn_amd import make_mlp
    from oracle import hgnn_oracle as O
    g = torch.Generator().manual_seed(len(kind))
    N, M, L = 300, 333, 96
    torch.manual_seed(7)
    x3 = torch.rand(N, 3, generator=g) * 2 - 1
    i0 = torch.randint(0, N, (M,), generator=g)
    i1 = torch.randint(0, N, (M,), generator=g)
    rows = torch.randn(M, L, generator=g)
    tab = torch.randn(50, L, generator=g)
    it = torch.randint(0, 50, (M,), generator=g)
    if kind == "node_enc":
        net, segs_cpu, layers, acts = make_mlp(3, 2 * L, L, 3, layer_norm=True, output_activation="GELU"), [(x3, None)], 3, ("GELU", "GELU")
    elif kind == "edge_enc":
        net, segs_cpu, layers, acts = make_mlp(6, 2 * L, L, 2, layer_norm=True, output_activation="GELU"), [(x3, i0), (x3, i1)], 2, ("GELU", "GELU")
    elif kind == "supernode_enc":
        net, segs_cpu, layers, acts = make_mlp(L, 2 * L, L - 8, 3, layer_norm=True, output_activation="GELU"), [(rows, None)], 3, ("GELU", "GELU")
    elif kind == "emb_head":
        net = make_mlp(L, 2 * L, 8, 3, layer_norm=True, output_activation=None, hidden_activation="Tanh")
        segs_cpu, layers, acts = [(rows, None)], 3, ("Tanh", None)
    else:
        net = make_mlp(2 * L, 2 * L, 1, 3, layer_norm=True, output_activation=None, hidden_activation="GELU")
        segs_cpu, layers, acts = [(rows, None), (tab, it)], 3, ("GELU", None)
    for p in net.parameters():
        if p.dim() == 1:
            p.data.add_(0.2 * torch.randn_like(p))
    xin = torch.cat([t if i is None else t[i] for t, i in segs_cpu], dim=1)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    ref = O.mlp_apply(sd, "", xin, layers, acts[0], acts[1], True)
    segs = [(t.cuda(), None if i is None else i.cuda()) for t, i in segs_cpu]
    out, again = _padded_forward(net.cuda(), segs, None)
    assert out.shape == ref.shape
    assert rel_err(out.cpu().numpy(), ref.numpy()) <= TOL
    assert torch.equal(out, again)


@pytest.mark.parametrize("L,h,layers", [(96, 192, 2), (144, 288, 3), (64, 192, 2)])
def test_padded_preprojected_segments_equal_the_full_k_kernel(L, h, layers):
    """hgnn_mlp_desc.n_pre on the padded route: the projections are [rows, 2P] with zero padded columns"""
    from hierarchicalgnn_amd import fused
    g = torch.Generator().manual_seed(7 * L + layers)
    net = _mk(3 * L, h, L, layers, "Tanh" if layers == 2 else "GELU", seed=L + 1).cuda()
    n_tab, M = 101, 1777
    table = torch.randn(n_tab, L, generator=g).cuda()
    direct = torch.randn(M, L, generator=g).cuda()
    i0 = torch.randint(0, n_tab, (M,), generator=g).cuda()
    i1 = torch.randint(0, n_tab, (M,), generator=g).cuda()
    segs = [(table, i0), (table, i1), (direct, None)]
    outs = {}
    try:
        for on in (True, False):
            fused.set_preproject(on)
            with torch.no_grad():
                d = fused._descriptor(net, segs, direct, "f32_padded")[0]
            assert int(d.n_pre) == (2 if on else 0) and int(d.n_seg) == (1 if on else 3)
            outs[on] = _padded_forward(net, segs, direct)[0]
    finally:
        fused.set_preproject(True)
    assert rel_err(outs[True].cpu().numpy(), outs[False].cpu().numpy()) <= TOL


@pytest.mark.parametrize("L,h,layers", [(96, 192, 2), (144, 288, 3), (64, 192, 3)])
def test_padded_train_backward_matches_autograd(L, h, layers):
    """the differentiable variant on the padded route (dumps at the real widths + the hand-written backward on the
    unpadded parameters) against autograd through the library path: outputs and every gradient"""
    from hierarchicalgnn_amd import fused, mlp
    g = torch.Generator().manual_seed(L + layers)
    out_act = "Tanh" if layers == 2 else "GELU"
    net = _mk(3 * L, h, L, layers, out_act, seed=L).cuda()
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
            assert (c1[2] - c0[2], c1[1] - c0[1]) == ((1, 1) if on else (0, 0))
            (out * r).sum().backward()
            results[name] = [out.detach(), table.grad, direct.grad] + [p.grad.clone() for p in net.parameters()]
    finally:
        fused.set_enabled(True)
    for a, b in zip(results["fused"], results["library"]):
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) <= TOL


def test_padded_heads_train_on_the_library_path():
    from hierarchicalgnn_amd import fused, make_mlp
    net = make_mlp(192, 192, 1, 3, layer_norm=True, output_activation=None, hidden_activation="GELU").cuda()
    x = torch.randn(40, 192, device="cuda").requires_grad_(True)
    assert not fused.supported_train(net, [(x, None)], None)
    with torch.no_grad():
        assert fused.supported(net, [(x, None)], None)


def test_checkpointed_cell_at_latent_96():
    """one InteractionGNNCell at latent 96 through torch.utils.checkpoint: the no-grad first pass and the recompute
    under autograd both run the padded kernel; outputs and gradients against the library path"""
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import fused, synth
    torch.manual_seed(3)
    L = 96
    hp = dict(latent=L, hidden=2 * L, nb_edge_layer=2, nb_node_layer=3, layernorm=True, hidden_activation="GELU",
              checkpointing=True)
    cell = H.InteractionGNNCell(hp).cuda()
    _, ei = synth.trackml_event(600, 3000, seed=4)
    graph = synth.directed(ei).cuda()
    nodes0 = torch.randn(600, L, device="cuda")
    edges0 = torch.randn(graph.shape[1], L, device="cuda")
    rn, re_ = torch.randn_like(nodes0), torch.randn_like(edges0)
    results = {}
    try:
        for name, on in (("fused", True), ("library", False)):
            fused.set_enabled(on)
            cell.zero_grad(set_to_none=True)
            nodes, edges = nodes0.clone().requires_grad_(True), edges0.clone().requires_grad_(True)
            c0 = _counts()
            out_n, out_e = cell(nodes, edges, graph)
            c1 = _counts()
            ((out_n * rn).sum() + (out_e * re_).sum()).backward()
            c2 = _counts()
            if on:
                assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 2)            # no-grad first pass: node + edge network
                assert (c2[2] - c1[2], c2[1] - c1[1]) == (2, 2)            # recompute under autograd
            else:
                assert c2 == c0
            results[name] = [out_n.detach(), out_e.detach(), nodes.grad, edges.grad] + [p.grad.clone() for p in cell.parameters()]
    finally:
        fused.set_enabled(True)
    for a, b in zip(results["fused"], results["library"]):
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) <= TOL


def _counting():
    """(calls, restore): count every mlp.concat_mlp call of the model mirrors (test_bc_forward_latent256_has_no_library_mlp)"""
    import hierarchicalgnn_amd.gnn_utils as gu
    import hierarchicalgnn_amd.models as mo
    from hierarchicalgnn_amd import mlp
    calls = {"n": 0}
    real = mlp.concat_mlp

    def counting(net, segments, skip=None, bf16_tail=False, out=None):
        calls["n"] += 1
        return real(net, segments, skip, bf16_tail, out)

    gu.concat_mlp = mo.concat_mlp = counting

    def restore():
        gu.concat_mlp = mo.concat_mlp = real
    return calls, restore


def _raw(name, **over):
    with open(os.path.join(conftest.GOLDEN, "ref_configs.json")) as f:
        return dict(json.load(f)[name]["raw"], **over)


def test_ec_in_at_latent_96_has_no_library_mlp():
    from hierarchicalgnn_amd import fused, synth
    from hierarchicalgnn_amd.models import EC_InteractionGNN
    torch.manual_seed(0)
    model = EC_InteractionGNN(_raw("EC-IN", latent=96)).cuda().eval()
    x, ei = synth.trackml_event(3000, 18000, seed=5)
    x, ei = x.cuda(), ei.cuda()
    calls, restore = _counting()
    try:
        c0 = _counts()
        with torch.no_grad():
            s = model(x, ei)
        c1 = _counts()
    finally:
        restore()
    expected = 2 + 2 * 14 + 1                        # encoders, 14 cells, edge classifier
    assert calls["n"] == expected
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (expected, expected)
    fused.set_enabled(False)
    try:
        with torch.no_grad():
            ref = model(x, ei)
    finally:
        fused.set_enabled(True)
    assert _counts() == c1
    assert rel_err(s.cpu().numpy(), ref.cpu().numpy()) <= TOL


def test_bc_hgnn_gmm_at_latent_96_has_no_library_mlp():
    from hierarchicalgnn_amd import fused, synth
    from hierarchicalgnn_amd.models import BC_MessagePassing
    torch.manual_seed(0)
    model = BC_MessagePassing(_raw("BC-HGNN-GMM", latent=96, emb_dim=8)).cuda().eval()
    x, ei = synth.trackml_event(3000, 18000, seed=5)
    x, ei = x.cuda(), ei.cuda()
    bg, bw = synth.bipartite_assignment(3000, 40, 5, seed=2)
    sg, sw = synth.super_graph(40, 10, seed=2)
    means = torch.nn.functional.normalize(torch.randn(40, 8)).cuda()

    def forward():
        with torch.no_grad():
            directed, emb, nodes, edges, _ = model.embed(x, ei)
            n_out, sn_out, _, _ = model.hgnn_block(nodes, edges, directed, means, bg.cuda(), bw.cuda(), sg.cuda(), sw.cuda())
            return model.score(n_out, sn_out, bg.cuda())

    calls, restore = _counting()
    try:
        c0 = _counts()
        s = forward()
        c1 = _counts()
    finally:
        restore()
    expected = 2 + 2 * 6 + 1 + 2 + 4 * 6 + 1        # encoders, IGNN cells, emb head, super encoders, HGNN cells, head
    assert calls["n"] == expected
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (expected, expected)
    fused.set_enabled(False)
    try:
        ref = forward()
    finally:
        fused.set_enabled(True)
    assert bool(torch.isfinite(s).all())
    assert rel_err(s.cpu().numpy(), ref.cpu().numpy()) <= TOL
