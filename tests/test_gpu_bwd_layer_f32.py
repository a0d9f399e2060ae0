"""hgnn_mlp_backward_layer_f32 (csrc/mlp_bwd_f32.hip) and its route through fused._FusedMLPTrain.

  * input form, exact: integer grids (tests/gemm_ref.py), the fp32 result must equal the float64 product bit for bit;
    guarded output buffers, every call twice;
  * LayerNorm form on an exact GEMM half: the same grids for dz and W, so da is exact and only the epilogue can err;
  * LayerNorm form, bars: the four cell shapes + (1024, 128), ln_ref.CASES, GELU / Tanh / ReLU, against the float64
    definition on the project's fp32 bars (tests/test_bwd_layer_f32_ref.py proves on the CPU that a float32 emulation of
    this arithmetic stays within half of each);
  * rows do not depend on the trip of the persistent tile loop that computes them;
  * routing: with fused.set_bwd_layer_f32(True) the exact training backward makes the expected launches and agrees with
    the library route and with the switch off, in the edge-update shape (skip = the last segment), the node-update
    shape (skip = the first of two or three direct segments) and an InteractionGNNCell step; the skip gradient is
    returned once;
  * refused calls write nothing.

Wall time of this file alone on an MI355X: 98 tests in about 5 s (the slowest, the InteractionGNNCell step, 1.6 s).  Worst measured ratios to the
1e-4 bar: 0.47 on a' (r256, Tanh, N = 128), 0.26 on dz', 0.19 on the column sums, 0.014 on const rows.
"""
import ctypes

import pytest
import torch

import bwd_layer_f32_ref as B
import ln_ref as R
from conftest import rel_err
from test_gpu_fused import TOL, _mk
from test_gpu_gemm_exact import assert_bits
from test_gpu_mlp_layernorm import BAR, _Report
from test_gpu_rows_exact import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _L():
    from hierarchicalgnn_amd import _lib
    return _lib


@pytest.fixture()
def on():
    from hierarchicalgnn_amd import fused
    old = fused._bwd_layer_f32_on
    fused.set_bwd_layer_f32(True)
    yield fused
    fused.set_bwd_layer_f32(old)


def _call(dz, wt, M, K, N, out_ptr, z=None, gm=None, bt=None, act=0, eps=1e-5, skip=None, a_prev=None, partials=None):
    """the C entry itself -> status"""
    L = _L()
    return L.load().hgnn_mlp_backward_layer_f32(L.ptr(dz), M, K, N, L.ptr(wt), L.ptr(z), L.ptr(gm), L.ptr(bt), act, eps,
                                                L.ptr(skip), out_ptr, L.ptr(a_prev), L.ptr(partials),
                                                L.current_stream(torch.device(DEV)))


def _where(row, col):
    tile = row // 64
    return (f"tile {tile} (trip {tile // B.BLOCKS + 1} of workgroup {tile % B.BLOCKS}), wave {row % 64 // 16}, "
            f"row lane {row % 16}, feature tile {col // 16}, lane group {col % 16 // 4}, register {col % 4}")


# --------------------------------------------------------------------------------------------------- input form, exact
@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("K", B.EXACT_K)
@pytest.mark.parametrize("N", B.EXACT_N)
def test_input_form_exact(on, N, K, form):
    L = _L()
    for M in B.EXACT_M:
        dz, W, skip = B.exact_case(M, K, N, form)
        dz, W = dz.to(DEV), W.to(DEV)
        skip = skip.to(DEV) if skip is not None else None
        what = f"input form M={M} K={K} N={N} {form}"
        s = dz.double() @ W.double()
        ref = (s if skip is None else s + skip.double()).float()
        g = Guarded(M, N, torch.float32)
        L.check(_call(dz, W.t().contiguous(), M, K, N, g.ptr(), skip=skip), "hgnn_mlp_backward_layer_f32")
        g.all_written(what)
        assert_bits(g.check(what), ref, what, _where)
        again = on._bwd_layer_f32(dz, W, None, None, None, 0, 1e-5, skip=skip)[0]
        assert_bits(again, ref, what + " (second call, through fused._bwd_layer_f32)", _where)


# ------------------------------------------------------------------------------------- LayerNorm form, exact GEMM half
@pytest.mark.parametrize("K", B.EXACT_K)
@pytest.mark.parametrize("N", B.EXACT_N)
def test_ln_form_on_an_exact_gemm_half(on, N, K):
    """dz and W from the integer grids: da = dz W is exact in fp32, so every error here is the epilogue's.  The bars are
    the fp32 ones; the column sums of the three cases are checked normwise"""
    M = R.M_ROWS
    dz, W, _ = B.exact_case(M, K, N, "plain")
    da = dz.double() @ W.double()
    rep = _Report(f"bwd_layer_f32_exact_gemm_K{K}_N{N}")
    for name in ("r0", "r64", "const_c0.5"):
        rc = R.make_rows_case(name, N, seed=K)
        a_ref = R.ln_act_forward(rc["z"], rc["gamma"], rc["beta"], R.ACT_GELU, rc["eps"]).numpy()
        dz_ref, dg_ref, db_ref, dbias_ref = [t.numpy() for t in R.ln_act_backward(
            rc["z"], da, rc["gamma"], rc["beta"], R.ACT_GELU, rc["eps"])]
        args = (dz.to(DEV), W.to(DEV), rc["z"].to(DEV), rc["gamma"].to(DEV), rc["beta"].to(DEV), R.ACT_GELU, rc["eps"])
        dzp, a_prev, dg, db, dbias = on._bwd_layer_f32(*args, want_a=True)
        rep.f32_rows(name, "a_prev", a_prev, a_ref, rc["r"], rc["const_rows"])
        rep.f32_rows(name, "dz_prev", dzp, dz_ref, rc["r"], rc["const_rows"])
        rep.norm(name, "dgamma", dg, dg_ref, BAR)
        rep.norm(name, "dbeta", db, db_ref, BAR)
        rep.norm(name, "dbias", dbias, dbias_ref, BAR)
        for a, b in zip((dzp, a_prev, dg, db, dbias), on._bwd_layer_f32(*args, want_a=True)):
            rep.same(name, a, b)
    rep.done()


# ------------------------------------------------------------------------------------------------ LayerNorm form, bars
@pytest.mark.parametrize("act", B.BAR_ACTS, ids=["GELU", "Tanh", "ReLU"])
@pytest.mark.parametrize("K,N", B.BAR_SHAPES)
def test_ln_form_bars(on, K, N, act):
    assert on._bwd_layer_f32_supported(K, N)
    rep = _Report(f"bwd_layer_f32_K{K}_N{N}_act{act}")
    for name in R.CASES:
        rc, dz, W, ref = B.bar_case(K, N, name, act)
        args = (dz.to(DEV), W.to(DEV), rc["z"].to(DEV), rc["gamma"].to(DEV), rc["beta"].to(DEV), act, rc["eps"])
        n0 = on.stats["bwd_layer_f32_calls"]
        dzp, a_prev, dg, db, dbias = on._bwd_layer_f32(*args, want_a=True)
        assert on.stats["bwd_layer_f32_calls"] == n0 + 1
        rep.f32_rows(name, "a_prev", a_prev, ref["a"], rc["r"], rc["const_rows"])
        rep.f32_rows(name, "dz_prev", dzp, ref["dz"], rc["r"], rc["const_rows"])
        rep.norm(name, "dgamma", dg, ref["dgamma"], BAR)
        rep.norm(name, "dbeta", db, ref["dbeta"], BAR)
        rep.norm(name, "dbias", dbias, ref["dbias"], BAR)
        for a, b in zip((dzp, a_prev, dg, db, dbias), on._bwd_layer_f32(*args, want_a=True)):
            rep.same(name, a, b)
        no_a = on._bwd_layer_f32(*args, want_a=False)
        assert no_a[1] is None
        rep.same(name, no_a[0], dzp)
    rep.done()


@pytest.mark.parametrize("K,N", [(256, 512), (128, 64)])
def test_ln_form_one_row_idle_workgroups_write_zeros(on, K, N):
    """M = 1: one workgroup has a tile (one valid row of 64), the other 511 write zero partial rows"""
    L = _L()
    gen = torch.Generator().manual_seed(K + N)
    dz = torch.randn(1, K, generator=gen)
    W = torch.randn(K, N, generator=gen) / K ** 0.5
    rc = R.make_rows_case("r16", N, M=1, seed=K)
    ref = R.ln_act_backward(rc["z"], dz.double() @ W.double(), rc["gamma"], rc["beta"], R.ACT_GELU, rc["eps"])
    partials = torch.full((B.BLOCKS, 3, N), float("nan"), device=DEV)
    g, ga = Guarded(1, N, torch.float32), Guarded(1, N, torch.float32)
    L.check(_call(dz.to(DEV), W.t().contiguous().to(DEV), 1, K, N, g.ptr(), z=rc["z"].to(DEV), gm=rc["gamma"].to(DEV),
                  bt=rc["beta"].to(DEV), act=R.ACT_GELU, eps=rc["eps"], a_prev=ga.out, partials=partials),
            "hgnn_mlp_backward_layer_f32")
    g.all_written("dz'")
    ga.all_written("a'")
    g.check("dz'")
    ga.check("a'")
    assert bool((partials[1:] == 0).all()), "an idle workgroup wrote a non-zero partial"
    assert rel_err(g.out.cpu().numpy(), ref[0].numpy()) <= BAR
    for i, name in enumerate(("dgamma", "dbeta", "dbias")):
        assert rel_err(partials[0, i].cpu().numpy(), ref[1 + i].numpy()) <= BAR, name
        assert rel_err(partials.sum(0)[i].cpu().numpy(), ref[1 + i].numpy()) <= BAR, name


def test_no_rows(on):
    """M = 0: the input form returns at once; the LayerNorm form still runs and every workgroup writes zero partials;
    the wrapper launches nothing"""
    L = _L()
    N, K = 128, 256
    dz = torch.empty(0, K, device=DEV)
    wt = torch.ones(N, K, device=DEV)
    assert _call(dz, wt, 0, K, N, ctypes.c_void_p(0)) == L.HGNN_OK
    z = torch.ones(1, N, device=DEV)                      # a non-NULL address selects the LayerNorm form
    partials = torch.full((B.BLOCKS, 3, N), float("nan"), device=DEV)
    L.check(_call(dz, wt, 0, K, N, ctypes.c_void_p(0), z=z, gm=z[0], bt=z[0], act=1, partials=partials),
            "hgnn_mlp_backward_layer_f32")
    assert bool((partials == 0).all())
    n0 = on.stats["bwd_layer_f32_calls"]
    out = on._bwd_layer_f32(dz, wt.t(), torch.empty(0, N, device=DEV), torch.ones(N, device=DEV),
                            torch.zeros(N, device=DEV), 1, 1e-5, want_a=True)
    assert out[0].shape == (0, N) and out[1].shape == (0, N)
    assert all(bool((t == 0).all()) and t.shape == (N,) for t in out[2:])
    assert on._bwd_layer_f32(dz, wt.t(), None, None, None, 0, 1e-5)[0].shape == (0, N)
    assert on.stats["bwd_layer_f32_calls"] == n0


# ---------------------------------------------------------------------------------------------------- trip invariance
def _trips():
    trip = B.trip_rows()
    return 2 * trip + 65, [(trip, 2 * trip), (2 * trip, 2 * trip + 65)]


def test_ln_form_rows_do_not_depend_on_the_trip(on):
    M, ranges = _trips()
    K, N, act = 256, 512, R.ACT_GELU
    g = torch.Generator(device=DEV).manual_seed(5)
    dz = torch.randn(M, K, device=DEV, generator=g)
    W = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
    z = 1.5 * torch.randn(M, N, device=DEV, generator=g) + 0.2
    gamma = 1 + 0.2 * torch.randn(N, device=DEV, generator=g)
    beta = 0.2 * torch.randn(N, device=DEV, generator=g)
    dzp, a_prev = on._bwd_layer_f32(dz, W, z, gamma, beta, act, 1e-5, want_a=True)[:2]
    for s, e in ranges:
        sub = on._bwd_layer_f32(dz[s:e], W, z[s:e], gamma, beta, act, 1e-5, want_a=True)
        what = f"LN form K={K} N={N} GELU, rows {s}..{e} alone"
        assert_bits(dzp[s:e], sub[0], what + ": dz'", lambda r, c, s=s: _where(s + r, c))
        assert_bits(a_prev[s:e], sub[1], what + ": a'", lambda r, c, s=s: _where(s + r, c))


def test_input_form_rows_do_not_depend_on_the_trip(on):
    M, ranges = _trips()
    K, N = 512, 256
    g = torch.Generator(device=DEV).manual_seed(3)
    dz = torch.randn(M, K, device=DEV, generator=g)
    W = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
    skip = torch.randn(M, N, device=DEV, generator=g)
    full = on._bwd_layer_f32(dz, W, None, None, None, 0, 1e-5, skip=skip)[0]
    for s, e in ranges:
        sub = on._bwd_layer_f32(dz[s:e], W, None, None, None, 0, 1e-5, skip=skip[s:e])[0]
        assert_bits(full[s:e], sub, f"input form K={K} N={N} with skip, rows {s}..{e} alone",
                    lambda r, c, s=s: _where(s + r, c))


# ------------------------------------------------------------------------------------------------------------ routing
def _train(net, table0, direct0, i0, i1, r):
    from hierarchicalgnn_amd import mlp
    net.zero_grad(set_to_none=True)
    table = table0.clone().requires_grad_(True)
    direct = direct0.clone().requires_grad_(True)
    out = mlp.concat_mlp(net, [(table, i0), (table, i1), (direct, None)], skip=direct)
    (out * r).sum().backward()
    return [out.detach(), table.grad, direct.grad] + [p.grad.clone() for p in net.parameters()]


@pytest.mark.parametrize("L,layers", [(128, 2), (256, 2), (256, 3)])
def test_training_backward_routes_through_the_fused_layer(L, layers):
    """concat_mlp under autograd, two gathered segments + one direct segment that is also the skip (the shape of
    test_gpu_fused.test_fused_train_backward_matches_autograd): layers - 1 LayerNorm-form launches, one input-form
    launch per gathered segment (S W_s) and one for the direct segment with the skip gradient folded in"""
    from hierarchicalgnn_amd import fused
    g = torch.Generator().manual_seed(L + layers)
    net = _mk(3 * L, L, layers, "Tanh" if layers == 2 else "GELU", seed=L).cuda()
    n_tab, M = 83, 500
    table0 = torch.randn(n_tab, L, generator=g).cuda()
    direct0 = torch.randn(M, L, generator=g).cuda()
    i0 = torch.randint(0, n_tab, (M,), generator=g).cuda()
    i1 = torch.randint(0, n_tab, (M,), generator=g).cuda()
    r = torch.randn(M, L, generator=g).cuda()
    old = fused._bwd_layer_f32_on
    results = {}
    try:
        for name, switch, train in (("off", False, True), ("on", True, True), ("library", False, False)):
            fused.set_bwd_layer_f32(switch)
            fused.set_enabled(True, train=train)
            n0, t0 = fused.stats["bwd_layer_f32_calls"], fused.stats["fused_train_calls"]
            results[name] = _train(net, table0, direct0, i0, i1, r)
            assert (fused.stats["fused_train_calls"] == t0 + 1) == train
            assert fused.stats["bwd_layer_f32_calls"] - n0 == ((layers - 1) + 3 if switch else 0), name
    finally:
        fused.set_enabled(True)
        fused.set_bwd_layer_f32(old)
    for other in ("library", "off"):
        for i, (a, b) in enumerate(zip(results["on"], results[other])):
            assert rel_err(a.cpu().numpy(), b.cpu().numpy()) <= TOL, (other, i)
    # direct.grad = dz W_s + the skip gradient r, once: twice would be off by |r| ~ 1, far outside TOL
    skip_once = results["on"][2] - results["library"][2]
    assert float(skip_once.abs().max()) <= TOL * float(results["library"][2].abs().max())
    assert torch.equal(results["on"][0], results["off"][0])


@pytest.mark.parametrize("L,n_direct", [(128, 2), (128, 3), (256, 2)])
def test_node_update_shape_skip_is_the_first_of_several_direct_segments(L, n_direct):
    """the node update of both cells: every segment direct, the FIRST one also the skip rows
    (InteractionGNNCell: [nodes, edge messages], HierarchicalGNNCell: + supernode messages; three layers, GELU).  One
    input-form launch per direct segment, the skip gradient folded into the first one and returned once whatever
    follows it"""
    from hierarchicalgnn_amd import fused, mlp
    layers = 3
    g = torch.Generator().manual_seed(7 * L + n_direct)
    net = _mk(n_direct * L, L, layers, "GELU", seed=L + n_direct).cuda()
    M = 333
    rows0 = [torch.randn(M, L, generator=g).cuda() for _ in range(n_direct)]
    r = torch.randn(M, L, generator=g).cuda()

    def run():
        net.zero_grad(set_to_none=True)
        rows = [t.clone().requires_grad_(True) for t in rows0]
        out = mlp.concat_mlp(net, [(t, None) for t in rows], skip=rows[0])
        (out * r).sum().backward()
        return [out.detach()] + [t.grad for t in rows] + [p.grad.clone() for p in net.parameters()]

    old = fused._bwd_layer_f32_on
    results = {}
    try:
        for name, switch, train in (("off", False, True), ("on", True, True), ("library", False, False)):
            fused.set_bwd_layer_f32(switch)
            fused.set_enabled(True, train=train)
            n0, t0 = fused.stats["bwd_layer_f32_calls"], fused.stats["fused_train_calls"]
            results[name] = run()
            assert (fused.stats["fused_train_calls"] == t0 + 1) == train
            assert fused.stats["bwd_layer_f32_calls"] - n0 == ((layers - 1) + n_direct if switch else 0), name
    finally:
        fused.set_enabled(True)
        fused.set_bwd_layer_f32(old)
    for other in ("library", "off"):
        for i, (a, b) in enumerate(zip(results["on"], results[other])):
            assert rel_err(a.cpu().numpy(), b.cpu().numpy()) <= TOL, (other, i)


def test_interaction_cell_training_step_switch_on_against_off():
    """a real model step through the route: InteractionGNNCell forward + backward (node update: the skip is the first of
    two direct segments; edge update: two gathered segments and the skip last), every gradient with the switch on
    against off"""
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import fused, synth
    torch.manual_seed(3)
    L = 128
    hp = dict(latent=L, hidden=2 * L, nb_edge_layer=2, nb_node_layer=3, layernorm=True, hidden_activation="GELU")
    _, ei = synth.trackml_event(2000, 12000, seed=2)
    graph = synth.directed(ei).cuda()
    cell = H.InteractionGNNCell(hp).cuda()
    nodes0 = torch.randn(2000, L).cuda()
    edges0 = torch.randn(graph.shape[1], L).cuda()
    rn, re_ = torch.randn_like(nodes0), torch.randn_like(edges0)

    def step():
        cell.zero_grad(set_to_none=True)
        n, e = nodes0.clone().requires_grad_(True), edges0.clone().requires_grad_(True)
        on_, oe = cell(n, e, graph)
        ((on_ * rn).sum() + (oe * re_).sum()).backward()
        return [on_.detach(), oe.detach(), n.grad, e.grad] + [p.grad.clone() for p in cell.parameters()]

    old = fused._bwd_layer_f32_on
    try:
        fused.set_bwd_layer_f32(False)
        off = step()
        fused.set_bwd_layer_f32(True)
        n0 = fused.stats["bwd_layer_f32_calls"]
        on_res = step()
        assert fused.stats["bwd_layer_f32_calls"] - n0 == (2 + 2) + (1 + 3)      # node update, edge update
    finally:
        fused.set_bwd_layer_f32(old)
    names = ["nodes", "edges", "nodes.grad", "edges.grad"] + [n for n, _ in cell.named_parameters()]
    for name, a, b in zip(names, on_res, off):
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) <= TOL, name


def test_misaligned_parameter_views_are_copied_not_refused(on):
    """gamma / beta as slices of a flattened parameter buffer that start off the 16-byte grid"""
    K, N, M = 128, 128, 70
    g = torch.Generator(device=DEV).manual_seed(11)
    dz = torch.randn(M, K, device=DEV, generator=g)
    W = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
    z = torch.randn(M, N, device=DEV, generator=g)
    flat = torch.randn(2 * N + 2, device=DEV, generator=g)
    gamma, beta = flat[1:N + 1], flat[N + 1:2 * N + 1]
    assert gamma.data_ptr() % 16 and beta.data_ptr() % 16
    a = on._bwd_layer_f32(dz, W, z, gamma, beta, 1, 1e-5, want_a=True)
    b = on._bwd_layer_f32(dz, W, z, gamma.clone(), beta.clone(), 1, 1e-5, want_a=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("what", ["K72", "N96", "N1024", "null_out", "ln_without_partials", "ln_with_skip"])
def test_bad_arguments_are_refused_and_nothing_is_written(what):
    L = _L()
    M, K, N = 40, 128, 128
    k, n = {"K72": (72, N), "N96": (K, 96), "N1024": (K, 1024)}.get(what, (K, N))
    dz = torch.ones(M, 1024, device=DEV)
    wt = torch.ones(1024, 1024, device=DEV)
    z = torch.ones(M, 1024, device=DEV)
    gm = torch.ones(1024, device=DEV)
    g = Guarded(M, 1024, torch.float32)
    out_ptr = ctypes.c_void_p(0) if what == "null_out" else g.ptr()
    if what == "ln_without_partials":
        status = _call(dz, wt, M, k, n, out_ptr, z=z, gm=gm, bt=gm, act=1)
    elif what == "ln_with_skip":
        partials = torch.zeros(B.BLOCKS, 3, N, device=DEV)
        status = _call(dz, wt, M, k, n, out_ptr, z=z, gm=gm, bt=gm, act=1, skip=z, partials=partials)
    else:
        status = _call(dz, wt, M, k, n, out_ptr)
    torch.cuda.synchronize()
    assert status != L.HGNN_OK
    assert bool((g.bits == g.poison).all()), "a refused call wrote output rows"
    if what in ("K72", "N96", "N1024"):
        assert status == 4                                   # HGNN_ERR_UNSUPPORTED
