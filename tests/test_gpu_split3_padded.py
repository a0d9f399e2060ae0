"""GPU checks of the split-bf16 fp32 MLP at the widths BETWEEN its two (``hgnn_mlp_forward_f32_split3_padded``: the
64-row split-bf16 kernel on zero-padded, split parameters; ``fused.set_split3_padded``, off by default): forward against
an fp64 evaluation at the split-bf16 kernel's own bar (2e-5), LayerNorm conformance under row offset / scale / eps
(tests/ln_ref.py with the matrix-pipe grouping, the fp32 bar 1e-4), bit equality with the native kernel on the grid
shapes, dispatch, whole models at latent 96 against the exact padded route, and graph capture.

Every forward test asserts the route (``fused._route(...).entry``) and the counters: ``split3_padded_calls`` + 1,
``padded_calls`` and ``split3_calls`` unchanged.  The option is switched on by a fixture that restores it.

Worst error / bar of the conformance entries on an MI355X: L96x2 0.56, L144x3 0.77, L192x2 0.63, L64h192 0.42 (details in
``test_split3_padded_layernorm_conformance``'s docstring).
"""
import copy
import ctypes
import json
import os
import threading

import pytest
import torch

import conftest
import ln_ref as R
from test_gpu_mlp_layernorm import _nominal, _net, _Report, _segments
from test_gpu_split3 import AB_BOUND

pytestmark = pytest.mark.gpu
ENTRY = "f32_split3_padded"


@pytest.fixture()
def padded():
    """the opt-in route on (and the split-bf16 inference default it depends on), restored afterwards"""
    from hierarchicalgnn_amd import fused
    old = fused._split3_padded, fused._fp32_split3
    fused.set_split3_padded(True)
    fused.set_fp32_split3(True)
    yield fused
    fused.set_split3_padded(old[0])
    fused.set_fp32_split3(old[1])


def _mk(in_w, hidden, out, layers, out_act, seed, hidden_act="GELU"):
    from hierarchicalgnn_amd import make_mlp
    torch.manual_seed(seed)
    net = make_mlp(in_w, hidden, out, layers, layer_norm=True, output_activation=out_act, hidden_activation=hidden_act)
    for p in net.parameters():  # non-trivial LayerNorm affine / biases
        if p.dim() == 1:
            p.data.add_(0.2 * torch.randn_like(p))
    return net.cuda()


def _counts(fused):
    s = fused.stats
    return s.get("split3_padded_calls", 0), s["padded_calls"], s.get("split3_calls", 0), s["fused_calls"]


def _forward(fused, net, segs, skip):
    """two no-grad calls on the new route (asserted with its counters): (out, again)"""
    with torch.no_grad():
        assert fused._route(net, segs, skip, train=False).entry == ENTRY
        c0 = _counts(fused)
        out = fused.fused_concat_mlp(net, segs, skip)
        c1 = _counts(fused)
        assert tuple(b - a for a, b in zip(c0, c1)) == (1, 0, 0, 1)
        again = fused.fused_concat_mlp(net, segs, skip)
    return out, again


def _segs(L, nseg, M, n_tab, seed):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(n_tab, L, generator=g).cuda()
    i0 = torch.randint(0, n_tab, (M,), generator=g).cuda()
    i1 = torch.randint(0, n_tab, (M,), generator=g).cuda()
    direct = torch.randn(M, L, generator=g).cuda()
    return [(table, i0), (table, i1), (direct, None)][3 - nseg:], direct


def _fp64(net, segs, skip):
    with torch.no_grad():
        x = torch.cat([t.double() if i is None else t.double()[i] for t, i in segs], dim=1)
        ref = copy.deepcopy(net).double()(x)
        return ref if skip is None else ref + skip.double()


# (in segment width L, hidden h, layers, segments, M, skip, gathered table rows, pre-projection, hidden act, out width)
# table rows <= M / 4: the two gathered segments are pre-projected (n_pre = 2) unless switched off.  Between them: a wave
# with no real feature (h = 192, 144, 288, 384), partly real slices (16 of 64 at h = 144, 32 of 64 at h = 288 / 480, 8 of
# 32 at o = 72, 24 of 32 at o = 88), one- and two-panel partial segments (96, 80, 64 / 144, 192, 240), 1, 2 and 3 segments,
# partial last tiles (M = 1, 63, 65, 193).
# The latent-72 case (h = 144, o = 72: 16 of 64 and 8 of 32 real features in a wave) cannot have 72-wide segments: every
# fused fp32 kernel, the exact padded one included, takes segments that are multiples of 16 wide, and the new route is
# only reached where the exact padded check accepts.  It runs 3 x 80 -> 144 -> 72 with skip rows of their own.
# The network without skip, 288 -> 192 -> 88, has the shape and the GELU output of the networks that run without skip in
# the models (the encoders; 88 = latent - emb_dim outputs as the supernode encoder's).  With a Tanh output and no skip
# rows max |ref| is 1 and the relative measure becomes an absolute one, which the split-bf16 ARITHMETIC does not meet at
# 2e-5 at any width: measured on an MI355X 2.3e-5 - 2.9e-5 on this route (o = 64, 88, 96) and 2.3e-5 - 2.7e-5 on the native
# kernel at latent 128 / 256, evenly over the columns (the exact kernels: 1.5e-6 - 2.9e-6).  That case is held to the
# project's split-against-exact bound instead (test_split3_padded_tanh_output_without_skip).
FORWARD = [
    (96, 192, 2, 3, 193, True, 40, True, "GELU", None, None),
    (96, 192, 3, 2, 65, False, 97, True, "GELU", None, None),
    (80, 144, 2, 3, 63, True, 97, True, "GELU", 72, None),            # latent 72: see the note above
    (144, 288, 3, 3, 193, True, 40, True, "GELU", None, None),
    (192, 384, 2, 3, 65, True, 97, True, "GELU", None, None),
    (240, 480, 2, 1, 1, True, 97, True, "GELU", None, None),
    (64, 192, 2, 3, 193, True, 40, False, "GELU", None, None),
    (128, 512, 3, 2, 63, False, 97, True, "GELU", None, None),
    (96, 192, 2, 3, 193, False, 97, True, "GELU", 88, "GELU"),  # 288 -> 192 -> 88, no skip: see the note above
    (96, 192, 2, 3, 193, True, 97, True, "ReLU", None, None),         # activations read from the descriptor at run time
]


@pytest.mark.parametrize("L,h,layers,nseg,M,skip,n_tab,pre,hid_act,o,out_act", FORWARD)
def test_split3_padded_mlp_vs_fp64(padded, L, h, layers, nseg, M, skip, n_tab, pre, hid_act, o, out_act):
    """max |out - ref| / max |ref| <= 2e-5: test_split3_mlp_vs_fp64's expression and bar for the same arithmetic"""
    fused = padded
    o = L if o is None else o
    out_act = ("Tanh" if layers == 2 else "GELU") if out_act is None else out_act
    net = _mk(nseg * L, h, o, layers, out_act, seed=L + 7 * layers + nseg, hidden_act=hid_act)
    segs, direct = _segs(L, nseg, M, n_tab, seed=L * 10 + layers + h)
    sk = None if not skip else (direct if o == L else torch.randn(M, o, device="cuda"))
    with fused.options(preproject=pre):
        with torch.no_grad():
            d = fused._descriptor(net, segs, sk, ENTRY, dry=True)[0]
        projected = pre and nseg == 3 and 4 * n_tab <= M
        assert int(d.n_pre) == (2 if projected else 0) and int(d.n_seg) == (1 if projected else nseg)
        out, again = _forward(fused, net, segs, sk)
    ref = _fp64(net, segs, sk)
    assert out.dtype == torch.float32 and out.shape == ref.shape == (M, o)
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    print(f"\nsplit3_padded L={L} h={h} layers={layers} nseg={nseg} M={M}: {err:.3g} / 2e-5")
    assert err <= 2e-5
    assert torch.equal(out, again)


def test_split3_padded_tanh_output_without_skip(padded):
    """288 -> 192 -> 88 with a Tanh output and no skip rows: |ref| <= 1, so this is the ABSOLUTE error of the split-bf16
    arithmetic.  The NATIVE kernel runs the same kind of network beside it (384 -> 256 -> 128, Tanh, no skip, same rows and
    seeds): measured 2.3e-5 on this route and 2.3e-5 - 2.7e-5 on the native kernel, i.e. the native kernel does not meet
    2e-5 on this kind of network either (FORWARD's note).  Bounds: both within the project's stated split-against-exact
    bound, test_gpu_split3.AB_BOUND = 5e-5 (fp64 stands in for the exact kernel, which is within 3e-6 of it), and this
    route within twice the native kernel's own error (the same arithmetic; the factor covers the scatter of a maximum
    over 193 x 88 against 193 x 128 elements of two different networks)"""
    fused, M = padded, 193
    errs = {}
    for L, o in ((96, 88), (128, 128)):
        net = _mk(3 * L, 2 * L, o, 2, "Tanh", seed=L + 7 * 2 + 3)
        segs, _ = _segs(L, 3, M, 97, seed=L * 10 + 2 + 2 * L)
        if L == 96:
            out, again = _forward(fused, net, segs, None)
        else:
            with torch.no_grad():
                assert fused._route(net, segs, None, train=False).entry == "f32_split3"
                out = fused.fused_concat_mlp(net, segs, None)
                again = fused.fused_concat_mlp(net, segs, None)
        errs[L] = float((out.double() - _fp64(net, segs, None)).abs().max())
        assert torch.equal(out, again)
    print(f"\nTanh, no skip: max |out - ref| = {errs[96]:.3g} (288 -> 192 -> 88, this route), {errs[128]:.3g} "
          f"(384 -> 256 -> 128, native kernel); bound {AB_BOUND:g}")
    assert errs[128] <= AB_BOUND and errs[96] <= AB_BOUND
    assert errs[96] <= 2 * errs[128]


def test_forward_cases_use_the_preprojected_path_with_and_without_it():
    assert sum(1 for c in FORWARD if c[3] == 3 and 4 * c[6] <= c[4] and c[7]) >= 2
    assert sum(1 for c in FORWARD if c[3] == 3 and 4 * c[6] <= c[4] and not c[7]) >= 1


CONFORMANCE = {
    "L96x2": dict(widths=[288, 192, 96]),
    "L144x3": dict(widths=[432, 288, 288, 144]),
    "L192x2": dict(widths=[576, 384, 192]),
    "L64h192": dict(widths=[192, 192, 64]),
}


@pytest.mark.parametrize("cfg", sorted(CONFORMANCE))
def test_split3_padded_layernorm_conformance(padded, cfg):
    """row offset, scale, eps and constant rows (ln_ref.CASES, matrix-pipe grouping) on the count-weighted pooled
    statistics; the bar is ln_ref.F32_BAR = 1e-4 (rel, elem for nominal r <= 64, const rows).

    Worst measured error / bar per configuration on an MI355X (the case and quantity that set it): L96x2 0.56 (r256,
    normwise), L144x3 0.77 (r64, element-wise), L192x2 0.63 (r64, element-wise), L64h192 0.42 (r256, normwise); the native
    split-bf16 kernels sit at 0.44 - 0.70 of the same bar (tests/test_gpu_mlp_layernorm.py), the float32 emulation of the
    pooling alone (tests/test_split3_padded_ref.py, no split truncation) at 0.23 - 0.40."""
    rep = _Report(f"{cfg}/split3_padded")
    for name in R.CASES:
        case = R.case_for(CONFORMANCE[cfg], name, matrix=True)
        segs, skip = _segments(case)
        out, again = _forward(padded, _net(case), segs, skip)
        rep.f32_rows(name, "out", out, case["ref"].numpy(), _nominal(case), case["const_rows"])
        rep.same(name, out, again)
    rep.done()


def _call(lib, name, d, M, n_out):
    from hierarchicalgnn_amd import _lib
    out = torch.empty((M, n_out), dtype=torch.float32, device="cuda")
    _lib.check(getattr(lib, name)(ctypes.byref(d), _lib.ptr(out), _lib.current_stream(out.device)), name)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("M,n_tab", [(193, 97), (40000, 2000)])
@pytest.mark.parametrize("layers", [2, 3])
@pytest.mark.parametrize("L", [128, 256])
def test_grid_shapes_return_the_native_kernels_bits(padded, L, layers, M, n_tab):
    """latent 128 / 256 (nothing padded): the new entry on the native weight stream and on descriptors as
    fused._descriptor builds them -- for either entry -- equals hgnn_mlp_forward_f32_split3 bit for bit (M < 65,536: both
    run the 64-row kernel).  M = 40000 pre-projects the two gathered segments."""
    from hierarchicalgnn_amd import _lib
    fused, lib = padded, _lib.load()
    net = _mk(3 * L, 2 * L, L, layers, "Tanh" if layers == 2 else "GELU", seed=L + layers)
    segs, direct = _segs(L, 3, M, n_tab, seed=L + M)
    with torch.no_grad():
        for entry, split_proj in (("f32_split3", True), (ENTRY, False)):
            d, keep, m, n_out = fused._descriptor(net, segs, direct, entry, split_proj)
            assert (m, n_out) == (M, L) and int(d.n_pre) == (2 if M == 40000 else 0)
            d.w_last_rows = 0
            assert lib.hgnn_mlp_supported_f32_split3(ctypes.byref(d)) == 1
            native = _call(lib, "hgnn_mlp_forward_f32_split3", d, M, L)
            d.w_last_rows = L
            assert lib.hgnn_mlp_supported_f32_split3_padded(ctypes.byref(d)) == 1
            new = _call(lib, "hgnn_mlp_forward_f32_split3_padded", d, M, L)
            assert torch.equal(new, native), (entry, float((new - native).abs().max()))
            del keep
    ref = _fp64(net, segs, direct)
    assert float((new.double() - ref).abs().max() / ref.abs().max()) <= 2e-5


def test_dispatch_keeps_todays_routes_unless_everything_asks_for_the_new_one():
    from hierarchicalgnn_amd import fused
    L = 96
    net = _mk(3 * L, 2 * L, L, 2, "Tanh", seed=4)
    segs, direct = _segs(L, 3, 193, 97, seed=11)
    old = fused._split3_padded, fused._fp32_split3
    fused.set_fp32_split3(True)
    fused.set_split3_padded(False)
    try:
        route = lambda **kw: fused._route(net, segs, direct, train=kw.get("train", False)).entry   # noqa: E731
        with torch.no_grad():
            assert route() == "f32_padded"                                   # option off: today's route
            n0 = fused.stats.get("split3_padded_calls", 0)
            p0 = fused.stats["padded_calls"]
            exact = fused.fused_concat_mlp(net, segs, direct)
            assert fused.stats.get("split3_padded_calls", 0) == n0 and fused.stats["padded_calls"] == p0 + 1
            seen = []
            with fused.options(split3_padded=True):
                assert route() == ENTRY
                def other():                                                 # (grad mode is per thread too)
                    with torch.no_grad():
                        seen.append((fused._opt("split3_padded"), route()))
                t = threading.Thread(target=other)
                t.start()
                t.join()
                with fused.options(fp32_split3=False):                       # the exact arithmetic asked for
                    assert route() == "f32_padded"
                with fused.training_forward():                               # the no-grad pass of a training step
                    assert route() == "f32_padded"
                    fused.fused_concat_mlp(net, segs, direct)
                    assert fused.stats.get("split3_padded_calls", 0) == n0
                net._hgnn_split3 = False                                     # hparams["fp32_gemm"] = "exact"
                assert route() == "f32_padded"
                net._hgnn_split3 = None
                new = fused.fused_concat_mlp(net, segs, direct)
                assert fused.stats.get("split3_padded_calls", 0) == n0 + 1
            assert seen == [(False, "f32_padded")]                           # another thread keeps the default
            assert route() == "f32_padded"
            assert not torch.equal(new, exact) and float((new - exact).abs().max()) < 1e-4
        # under autograd: the differentiable padded route of today, never the new one
        fused.set_split3_padded(True)
        n0 = fused.stats.get("split3_padded_calls", 0)
        x = direct.clone().requires_grad_(True)
        tsegs = segs[:2] + [(x, None)]
        assert fused._route(net, tsegs, x, train=False) is None
        assert fused._route(net, tsegs, x, train=True).entry == "f32_padded"
        from hierarchicalgnn_amd import mlp
        t0 = fused.stats["fused_train_calls"]
        mlp.concat_mlp(net, tsegs, skip=x).sum().backward()
        assert fused.stats["fused_train_calls"] == t0 + 1 and fused.stats.get("split3_padded_calls", 0) == n0
        assert x.grad is not None
    finally:
        fused.set_split3_padded(old[0])
        fused.set_fp32_split3(old[1])


def test_model_pinned_to_exact_keeps_the_exact_padded_route(padded):
    """hparams["fp32_gemm"] = "exact" with the option on: every MLP of the model stays on f32_padded"""
    from hierarchicalgnn_amd import synth
    from hierarchicalgnn_amd.models import EC_InteractionGNN
    torch.manual_seed(0)
    model = EC_InteractionGNN(_raw("EC-IN", latent=96, n_interaction_graph_iters=2, fp32_gemm="exact")).cuda().eval()
    x, ei = synth.trackml_event(600, 3000, seed=5)
    c0 = _counts(padded)
    with torch.no_grad():
        model(x.cuda(), ei.cuda())
    c1 = _counts(padded)
    assert c1[0] == c0[0] and c1[1] - c0[1] == 2 + 2 * 2 + 1 == c1[3] - c0[3]


def _raw(name, **over):
    with open(os.path.join(conftest.GOLDEN, "ref_configs.json")) as f:
        return dict(json.load(f)[name]["raw"], **over)


def _counting(fused):
    """(kinds, restore): every mlp.concat_mlp call of the model mirrors, classified by what the dispatch rule says about
    its network: 'cell' (LayerNorm on every layer, 16-multiple segments, hidden width above 128, not the narrow
    three-layer encoder) or 'other' (small-K encoders, heads, the narrow supernode encoder)"""
    import hierarchicalgnn_amd.gnn_utils as gu
    import hierarchicalgnn_amd.models as mo
    from hierarchicalgnn_amd import mlp
    kinds = []
    real = mlp.concat_mlp

    def counting(net, segments, skip=None, bf16_tail=False, out=None):
        layers = fused._parse(net)
        h, o = layers[0][0].out_features, layers[-1][0].out_features
        cell = all(ln is not None for _, ln, _ in layers) and all(int(t.shape[1]) % 16 == 0 for t, _ in segments) \
            and h > 128 and not fused._narrow_encoder(layers)
        kinds.append("cell" if cell else "other")
        return real(net, segments, skip, bf16_tail, out)

    gu.concat_mlp = mo.concat_mlp = counting

    def restore():
        gu.concat_mlp = mo.concat_mlp = real
    return kinds, restore


def _on_and_off(fused, forward, n_cell, n_other):
    """``forward()`` with the option on (counters asserted) and off; max |scores_on - scores_off|"""
    kinds, restore = _counting(fused)
    lib0 = fused.stats["library_calls"]
    try:
        c0 = _counts(fused)
        on = forward()
        c1 = _counts(fused)
    finally:
        restore()
    assert (kinds.count("cell"), kinds.count("other")) == (n_cell, n_other)
    assert fused.stats["library_calls"] == lib0
    assert tuple(b - a for a, b in zip(c0, c1)) == (n_cell, n_other, 0, n_cell + n_other)
    with fused.options(split3_padded=False):
        off = forward()
    c2 = _counts(fused)
    assert tuple(b - a for a, b in zip(c1, c2)) == (0, n_cell + n_other, 0, n_cell + n_other)
    assert bool(torch.isfinite(on).all())
    d = float((on - off).abs().max())
    print(f"\nmax |scores_on - scores_off| = {d:.3g} (bound {AB_BOUND:g})")
    return d


def test_ec_in_at_latent_96_runs_its_cells_on_the_new_route(padded):
    """the 28 cell networks on hgnn_mlp_forward_f32_split3_padded, the 2 small-K encoders and the head on the exact
    padded kernel, no library MLP; scores within the project's split-against-exact bound of the exact padded route"""
    from hierarchicalgnn_amd import synth
    from hierarchicalgnn_amd.models import EC_InteractionGNN
    torch.manual_seed(0)
    model = EC_InteractionGNN(_raw("EC-IN", latent=96)).cuda().eval()
    x, ei = synth.trackml_event(3000, 18000, seed=5)
    x, ei = x.cuda(), ei.cuda()

    def forward():
        with torch.no_grad():
            return model(x, ei)

    assert _on_and_off(padded, forward, 28, 3) <= AB_BOUND


def test_bc_hgnn_gmm_at_latent_96_runs_its_cells_on_the_new_route(padded):
    from hierarchicalgnn_amd import synth
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

    # IGNN cells 2 x 6, HGNN cells 4 x 6, the superedge encoder | node / edge encoders (3- and 6-wide inputs), embedding
    # head, the narrow supernode encoder (96 -> 192 -> 192 -> 88), score head
    assert _on_and_off(padded, forward, 2 * 6 + 4 * 6 + 1, 2 + 1 + 1 + 1) <= AB_BOUND


def test_split3_padded_forward_is_graph_capturable(padded):
    """one padded forward (weight streams, padded vectors and int32 indices cached by the warm-up call) captured on a single stream:
    the replay equals the eager result, also after the inputs changed in place"""
    fused = padded
    L, M = 96, 193
    net = _mk(3 * L, 2 * L, L, 2, "Tanh", seed=2)
    segs, direct = _segs(L, 3, M, 97, seed=3)
    with torch.no_grad():
        assert fused._route(net, segs, direct, train=False).entry == ENTRY
        eager = fused.fused_concat_mlp(net, segs, direct)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fused.fused_concat_mlp(net, segs, direct)                        # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        n0 = fused.stats.get("split3_padded_calls", 0)
        with torch.cuda.graph(g, stream=s):
            out = fused.fused_concat_mlp(net, segs, direct)
        assert fused.stats.get("split3_padded_calls", 0) == n0 + 1
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        direct.mul_(0.5)
        eager2 = fused.fused_concat_mlp(net, segs, direct)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager2) and not torch.equal(eager2, eager)
