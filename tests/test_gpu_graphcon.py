"""GPU: the device-side graph construction (csrc/graphcon.hip) against its proven references (tests/graphcon_ref.py).

``knn_edges`` must equal ``hierarchy_ref.edges_from_knn`` exactly.  Launch constants behind the large case: the k_gc
kernels run one thread per slot in workgroups of 256, the grid is ceil(slots / 256) and is never capped (nq K < 2^30
keeps it below 2^22 workgroups), so no size is a second trip of one grid; what does change with the size is rocprim's
path -- a single-workgroup scan and sort below a few thousand items, the multi-workgroup look-back scan and the
multi-pass radix sort above.  nq = 120000, K = 5 (600000 slots, 1200000 keys with sym: the bipartite shape of the
shipped configuration) is far into the latter and is the large case.

The attention operator runs ``graphcon_ref.cases()``; one workgroup trip covers 2048 x 256 = 524288 edges, the case
"big" has 525000.  Its figures against the float64 oracle are held to the 1e-4 bar of ``conftest.assert_parity``;
tests/test_graphcon_ref.py shows that the float32 emulation of the same arithmetic keeps half of it.
Running statistics are compared with what ``nn.BatchNorm1d`` leaves on the same x: ATen's are the float32 results of a
float32 pass (relative error about log2(E) 2^-24 ~ 1e-6 in the mean; the variance loses another (mean^2 + var) / var,
at most ~ 30 for these inputs), ours are float64 sums rounded once, so the bounds are 1e-5 for the mean and 1e-4 for
the variance; ``num_batches_tracked`` must be equal."""
import ctypes

import numpy as np
import pytest
import torch

import conftest
import graphcon_ref as R
import hierarchy_ref as HR
from conftest import assert_parity, load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
POISON = 0x5A5A5A5A5A5A5A5A
GUARD = 64


# ------------------------------------------------------------------ knn_edges
def _raw_knn_edges(idx, n_pts, sym):
    """``hgnn_knn_edges`` into poisoned buffers with guard zones on both sides; returns the graph after checking that
    nothing but the first B entries of the two rows (and the two info words) was written"""
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    nq, K = idx.shape
    cap = (2 if sym else 1) * nq * K
    nb = ctypes.c_size_t(0)
    _lib.check(lib.hgnn_knn_edges_workspace_bytes(nq, K, n_pts, int(sym), ctypes.byref(nb)), "workspace")
    ws = torch.full((nb.value + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    buf = torch.full((GUARD + 2 * cap + GUARD,), POISON, dtype=torch.int64, device=DEV)
    info = torch.full((GUARD + 2 + GUARD,), POISON, dtype=torch.int64, device=DEV)
    edges = buf[GUARD:GUARD + 2 * cap]
    _lib.check(lib.hgnn_knn_edges(_lib.ptr(idx), nq, K, n_pts, int(sym), ctypes.c_void_p(edges.data_ptr()), cap,
                                  ctypes.c_void_p(info[GUARD:].data_ptr()), _lib.ptr(ws), nb.value,
                                  _lib.current_stream(idx.device)), "hgnn_knn_edges")
    torch.cuda.synchronize()
    count, status = info[GUARD:GUARD + 2].tolist()
    assert bool((info[:GUARD] == POISON).all()) and bool((info[GUARD + 2:] == POISON).all())
    assert bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + 2 * cap:] == POISON).all())
    assert bool((ws[nb.value:] == 0x5A).all())
    rows = edges.view(2, cap)
    assert bool((rows[:, count:] == POISON).all())                 # nothing past the count in either row
    return rows[:, :count].clone(), status


SHAPES = [(nq, K) for nq in (1, 63, 64, 65, 257, 4097) for K in (1, 5, 10, 32)]


def _n_pts(nq, K, i):
    """nq != n_pts both ways, and n_pts >= K so that a row can hold K distinct ids"""
    return max(K, nq + 3 if i % 2 else nq // 2 + 1)


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("fill", ["empty", "full", "prefix", "holes"])
def test_knn_edges_equals_the_torch_formulation(fill, sym):
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import graph_construction as G
    for i, (nq, K) in enumerate(SHAPES):
        n_pts = _n_pts(nq, K, i)
        idx = R.knn_pattern(nq, K, n_pts, fill, 1000 * i + K)
        want = HR.edges_from_knn(idx, sym, max(nq, n_pts))
        reads = G.stats["host_reads"]
        got = H.knn_edges(idx.to(DEV), n_pts, sym=sym)
        assert G.stats["host_reads"] == reads + 1, (nq, K)
        assert got.dtype == torch.int64 and got.is_contiguous() and got.shape == want.shape, (nq, K, got.shape)
        assert torch.equal(got.cpu(), want), (nq, K, n_pts)
        if fill == "empty":
            assert got.shape == (2, 0)
        if i % 5 == 0:                      # the C entry point into poisoned buffers: K = 1, 5, 10, 32, 1 in turn
            raw, status = _raw_knn_edges(idx.to(DEV), n_pts, sym)
            assert status == 0 and torch.equal(raw.cpu(), want), (nq, K)


def test_knn_edges_reference_cases():
    import hierarchicalgnn_amd as H
    for name, idx, n_pts in R.edge_cases():
        for sym in (False, True):
            want = HR.edges_from_knn(idx, sym, max(idx.shape[0], n_pts))
            assert torch.equal(H.knn_edges(idx.to(DEV), n_pts, sym=sym).cpu(), want), (name, sym)
            raw, status = _raw_knn_edges(idx.to(DEV), n_pts, sym)
            assert status == 0 and torch.equal(raw.cpu(), want), (name, sym)


@pytest.mark.parametrize("sym", [False, True])
def test_knn_edges_large_case(sym):
    import hierarchicalgnn_amd as H
    nq, K, n_pts = 120_000, 5, 10_000
    idx = R.knn_pattern(nq, K, n_pts, "holes", 77)
    if sym:
        idx = idx[:10_000].contiguous()                            # the super graph: 10k x 10k
        idx[:, 0] = torch.arange(10_000)                           # every row a self-pair, as a kNN of a set in itself
        nq = 10_000
    want = HR.edges_from_knn(idx, sym, max(nq, n_pts))
    got = H.knn_edges(idx.to(DEV), n_pts, sym=sym)
    assert torch.equal(got.cpu(), want)


def test_knn_edges_workspace_grows_with_the_slots():
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    sizes = {}
    for sym in (0, 1):
        for nq in (0, 1, 1000, 120_000):
            assert lib.hgnn_knn_edges_workspace_bytes(nq, 5, 10_000, sym, ctypes.byref(nb)) == 0
            sizes[sym, nq] = nb.value
        assert sizes[sym, 1000] < sizes[sym, 120_000]
    assert sizes[0, 120_000] >= 4 * 120_000 * 5                   # the int32 positions of the slots
    assert sizes[1, 120_000] >= 3 * 8 * 2 * 120_000 * 5           # keys, sorted keys, distinct keys


@pytest.mark.parametrize("bad", [-2, 40, 1 << 40])
@pytest.mark.parametrize("sym", [False, True])
def test_knn_edges_bad_id_is_reported_and_the_next_call_is_clean(bad, sym):
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import graph_construction as G
    idx = R.knn_pattern(65, 5, 40, "holes", 3)
    good = idx.clone()
    idx[17, 2] = bad
    reads = G.stats["host_reads"]
    with pytest.raises(ValueError, match="knn_edges"):
        H.knn_edges(idx.to(DEV), 40, sym=sym)
    assert G.stats["host_reads"] == reads + 1                      # the error comes from the same single read
    raw, status = _raw_knn_edges(idx.to(DEV), 40, sym)             # the slot is skipped, the rest is the graph
    skipped = idx.clone()
    skipped[17, 2] = -1
    assert status == 1 and torch.equal(raw.cpu(), HR.edges_from_knn(skipped, sym, 65))
    assert torch.equal(H.knn_edges(good.to(DEV), 40, sym=sym).cpu(), HR.edges_from_knn(good, sym, 65))


# ------------------------------------------------------------------ the attention operator
def _bn(inp, momentum):
    bn = torch.nn.BatchNorm1d(1, momentum=momentum).to(DEV)
    with torch.no_grad():
        bn.weight.fill_(inp["gamma"])
        bn.bias.fill_(inp["beta"])
        bn.running_mean.fill_(inp["running_mean"])
        bn.running_var.fill_(inp["running_var"])
        bn.num_batches_tracked.fill_(inp["nbt"])
    return bn


_GPU_CASES = {}


def _gpu_case(c):
    """device inputs, the kNN graph and the float64 oracle of one case: computed once, never modified"""
    from hierarchicalgnn_amd.ops import knn_radius
    name, D, E, seed, training, fn, norm, gl, same, bw = c
    if name not in _GPU_CASES:
        inp = R.case_inputs(D, E, seed, same)
        A = inp["A"].to(DEV)
        B = A if same else inp["B"].to(DEV)
        idx = knn_radius(A, B, R.K_CASE, 2.1)                      # unit vectors: every point is within 2.1
        assert bool((idx >= 0).all())
        graph = R.case_graph(idx, E)
        g_w = inp["g_w"].to(DEV) if bw else None
        g_l = inp["g_logits"].to(DEV) if gl and bw else None
        o = R.oracle64(A, B, graph, inp["gamma"], inp["beta"], inp["running_mean"], inp["running_var"], fn, norm,
                       training, g_w=g_w, g_logits=g_l, same=same)
        _GPU_CASES[name] = (inp, A, B, graph, g_w, g_l, o)
    return _GPU_CASES[name]


def _run(c, A, B, graph, inp, g_w, g_l, momentum):
    """one forward (+ backward) of the operator on fresh leaves and a fresh BatchNorm"""
    from hierarchicalgnn_amd import graph_construction as G
    name, D, E, seed, training, fn, norm, gl, same, bw = c
    bn = _bn(inp, momentum).train(training)
    a = A.clone().requires_grad_(True)
    b = a if same else B.clone().requires_grad_(True)
    flags = (G._lib.GA_TRAINING if training else 0) | (G._lib.GA_NORM if norm else 0)
    w, z, x, state = G._GraphAttention.apply(a, b, bn.weight, bn.bias, graph, bn, G._GA_FN[fn], flags)
    out = dict(weights=w.detach(), logits=z.detach(), x=x, bn=bn)
    if bw:
        loss = (w * g_w).sum()
        if g_l is not None:
            loss = loss + (z * g_l).sum()
        loss.backward()
        out.update(dA=a.grad, dB=None if same else b.grad, dbn=torch.cat([bn.weight.grad, bn.bias.grad]))
    return out


@pytest.mark.parametrize("c", R.cases(), ids=[c[0] for c in R.cases()])
def test_attention_operator_against_the_float64_oracle(c):
    from hierarchicalgnn_amd.ops import edge_dot
    name, D, E, seed, training, fn, norm, gl, same, bw = c
    inp, A, B, graph, g_w, g_l, o = _gpu_case(c)
    momentum = None if seed % 2 else 0.1
    r = _run(c, A, B, graph, inp, g_w, g_l, momentum)
    assert graph.shape == (2, E)
    with torch.no_grad():
        x_ref = edge_dot(A, graph[0], B, graph[1])
    assert torch.equal(r["x"], x_ref), name                        # the bits of hgnn_edge_dot_f32
    got = dict(r)
    if bw:
        got.update(dgamma=r["dbn"][0], dbeta=r["dbn"][1])
    # graphcon_ref.errors: every quantity on its own (dgamma and dbeta too), each scaled so that its bar reads 1e-4:
    # dA / dB at gx_bar (1e-4 but for E = 2 in training mode), a vanishing dbeta as |dbeta| / S at 1e-6
    errs = R.errors(got, o, c, x_ref, g_w)
    print(f"{name}: normwise/element-wise " + ", ".join(f"{q} {a:.3g}/{b:.3g}" for q, (a, b) in errs.items()))
    assert set(errs) == {"weights", "logits"} | ({"dA", "dgamma", "dbeta"} | (set() if same else {"dB"}) if bw else set())
    for what, ref_key, tol in (("weights", "weights", TOL), ("logits", "logits", TOL)) + \
            ((("dA", "dA", R.gx_bar(training, E, x_ref.cpu())),) if bw else ()) + \
            ((("dB", "dB", R.gx_bar(training, E, x_ref.cpu())),) if bw and not same else ()) + \
            ((("dgamma", "dgamma", TOL),) if bw else ()) + \
            ((("dbeta", "dbeta", TOL),) if bw and not R.dbeta_is_zero(fn, norm, gl) else ()):
        assert_parity(got[what].reshape(o[ref_key].shape), o[ref_key], tol, f"{name} {what}")
    if bw and R.dbeta_is_zero(fn, norm, gl):
        scale = R.dbeta_scale(g_w.cpu().numpy(), o["weights"].cpu().numpy())
        assert abs(float(got["dbeta"])) <= R.DBETA_ZERO_BOUND * scale, (name, float(got["dbeta"]), scale)
    for q, (a, b) in errs.items():
        assert a <= TOL and b <= TOL, (name, q, a, b)
    # running statistics: nn.BatchNorm1d on the same x, from the same state
    bn_ref = _bn(inp, momentum).train(training)
    with torch.no_grad():
        bn_ref(x_ref.unsqueeze(1))
    bn = r["bn"]
    assert int(bn.num_batches_tracked) == int(bn_ref.num_batches_tracked) == inp["nbt"] + int(training)
    rm, rm_ref = float(bn.running_mean), float(bn_ref.running_mean)
    rv, rv_ref = float(bn.running_var), float(bn_ref.running_var)
    print(f"{name}: running mean {rm!r} vs {rm_ref!r}, running var {rv!r} vs {rv_ref!r}")
    if training:
        assert abs(rm - rm_ref) <= 1e-5 * abs(rm_ref) and abs(rv - rv_ref) <= 1e-4 * abs(rv_ref), name
        assert rm != float(np.float32(inp["running_mean"]))
    else:
        assert rm == rm_ref == float(np.float32(inp["running_mean"])) and rv == rv_ref      # eval: nothing is written
    # a second call on the same input: the same bits
    r2 = _run(c, A, B, graph, inp, g_w, g_l, momentum)
    for k in ("weights", "logits", "x") + (("dA", "dbn") if bw else ()) + (("dB",) if bw and not same else ()):
        assert torch.equal(r[k], r2[k]), (name, k)
    assert float(r2["bn"].running_var) == rv and float(r2["bn"].running_mean) == rm


def test_attention_index_types_bf16_and_out_of_range_ids():
    import hierarchicalgnn_amd as H
    c = [c for c in R.cases() if c[0] == "mode3"][0]
    inp, A, B, graph, g_w, g_l, o = _gpu_case(c)
    bn = _bn(inp, 0.1).eval()
    with torch.no_grad():
        w64, z64 = H.attention_weights(A, B, graph, bn, "sigmoid", norm=True, logits=True)
        w32, z32 = H.attention_weights(A, B, graph.int(), bn, torch.sigmoid, norm=True, logits=True)
        assert w64.shape == (graph.shape[1], 1) and torch.equal(w64, w32) and torch.equal(z64, z32)
        wb = H.attention_weights(A.bfloat16(), B.bfloat16(), graph, bn, "sigmoid", norm=True)
        assert torch.equal(wb, H.attention_weights(A.bfloat16().float(), B.bfloat16().float(), graph, bn, "sigmoid",
                                                   norm=True))
        bad = graph.clone()
        bad[0, 5], bad[1, 9] = A.shape[0], -1                      # never used as an address: x = 0 there
        _, zb = H.attention_weights(A, B, bad, bn, "sigmoid", logits=True)
        z0 = float(bn.weight) * (0.0 - float(bn.running_mean)) / (float(bn.running_var) + bn.eps) ** 0.5 + float(bn.bias)
        assert abs(float(zb[5]) - z0) <= 1e-5 * abs(z0) and float(zb[5]) == float(zb[9])
        keep = torch.ones(graph.shape[1], dtype=torch.bool, device=DEV)
        keep[5] = keep[9] = False
        _, zg = H.attention_weights(A, B, graph, bn, "sigmoid", logits=True)
        assert torch.equal(zb[keep], zg[keep])


def test_attention_backward_with_int32_graph_equals_int64():
    import hierarchicalgnn_amd as H
    for cname, same in (("mode3", False), ("same_train", True)):
        c = [c for c in R.cases() if c[0] == cname][0]
        inp, A, B, graph, g_w, g_l, o = _gpu_case(c)
        res = {}
        for dt in (torch.int64, torch.int32):
            bn = _bn(inp, 0.1).train()
            a = A.clone().requires_grad_(True)
            b = a if same else B.clone().requires_grad_(True)
            w, z = H.attention_weights(a, b, graph.to(dt), bn, "sigmoid", norm=True, logits=True)
            ((w.squeeze(1) * g_w).sum() + (z * g_l).sum()).backward()
            res[dt] = (w.detach(), z.detach(), a.grad, b.grad, bn.weight.grad, bn.bias.grad, bn.running_var.clone())
        for t64, t32 in zip(res[torch.int64], res[torch.int32]):
            assert torch.equal(t64, t32), cname
        assert float(res[torch.int32][2].abs().sum()) > 0 and float(res[torch.int32][4].abs()) > 0


def test_attention_host_side_rules_on_device_tensors():
    import hierarchicalgnn_amd as H
    c = [c for c in R.cases() if c[0] == "mode0"][0]
    inp, A, B, graph, g_w, g_l, o = _gpu_case(c)
    bn = _bn(inp, 0.1).train()
    for e in (0, 1):
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            H.attention_weights(A, B, graph[:, :e], bn, "exp")
    assert int(bn.num_batches_tracked) == inp["nbt"]
    bn.eval()
    w, z = H.attention_weights(A, B, graph[:, :0], bn, "exp", norm=True, logits=True)
    assert w.shape == (0, 1) and z.shape == (0,) and w.dtype == torch.float32 and w.is_cuda
    w1 = H.attention_weights(A, B, graph[:, :1], bn, "exp", norm=True)
    assert w1.shape == (1, 1) and abs(float(w1.detach()) - 1.0) <= 1e-6    # one edge, divided by its own mean
    with pytest.raises(ValueError, match="sigmoid.*exp"):
        H.attention_weights(A, B, graph, bn, "tanh")


def test_attention_no_host_read_under_sync_debug_mode():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import graph_construction as G
    c = [c for c in R.cases() if c[0] == "D8_E4097"][0]
    inp, A, B, graph, g_w, g_l, o = _gpu_case(c)
    bn = _bn(inp, None).train()
    a, b = A.clone().requires_grad_(True), B.clone().requires_grad_(True)

    def step():
        w, z = H.attention_weights(a, b, graph, bn, "exp", norm=True, logits=True)
        ((w.squeeze(1) * inp_gw).sum() + (z * inp_gl).sum()).backward()
        return w

    inp_gw, inp_gl = inp["g_w"].to(DEV), inp["g_logits"].to(DEV)
    step()                                                         # warm-up: code objects, allocator, the two plans
    torch.cuda.synchronize()
    reads = G.stats["host_reads"]
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        w = step()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert G.stats["host_reads"] == reads
    assert bool(torch.isfinite(w).all()) and int(bn.num_batches_tracked) == inp["nbt"] + 2


# ------------------------------------------------------------------ the module
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("sym,fn", [(False, "exp"), (True, "sigmoid")])
def test_module_fused_route_equals_the_default_route(sym, fn, training):
    from hierarchicalgnn_amd.graph_construction import DynamicGraphConstruction
    g = torch.Generator().manual_seed(11)
    n, s, k = 400, 40, 5
    src = torch.nn.functional.normalize(torch.randn(n, 8, generator=g)).to(DEV)
    dst = src if sym else torch.nn.functional.normalize(torch.randn(s, 8, generator=g)).to(DEV)
    out = {}
    for route in ("torch", "fused"):
        m = DynamicGraphConstruction(fn, {"graph_construction": route}).to(DEV).train(training)
        m.knn_radius.fill_(0.9)
        a = src.clone().requires_grad_(True)
        b = a if sym else dst.clone().requires_grad_(True)
        graph, w, z = m(a, b, sym=sym, norm=True, k=k, logits=True)
        # fixed upstream gradients: w.sum() and z.sum() are constants under the normalisations
        up = torch.randn(2, graph.shape[1], generator=torch.Generator().manual_seed(5)).to(DEV)
        ((w.squeeze(1) * up[0]).sum() + (z * up[1]).sum()).backward()
        out[route] = (graph, w.detach(), z.detach(), m.knn_radius.clone(), a.grad, m.weight_normalization)
    t, f = out["torch"], out["fused"]
    assert 0 < t[0].shape[1] < (2 if sym else 1) * n * k           # the radius cuts: rows with empty slots
    assert f[0].dtype == torch.int64 and f[0].is_contiguous() and torch.equal(t[0], f[0])
    assert f[1].shape == t[1].shape == (t[0].shape[1], 1)
    assert_parity(f[1], t[1], TOL, "weights")
    assert_parity(f[2], t[2], TOL, "logits")
    assert_parity(f[3], t[3], TOL, "knn_radius")
    assert_parity(f[4], t[4], TOL, "d/d embeddings")
    assert (float(t[3]) != float(np.float32(0.9))) == training
    assert int(f[5].num_batches_tracked) == int(t[5].num_batches_tracked) == int(training)
    assert_parity(f[5].running_var, t[5].running_var, TOL, "running_var")
    assert_parity(f[5].running_mean, t[5].running_mean, TOL, "running_mean")
    # the per-call override selects the same routes
    m = DynamicGraphConstruction(fn, {}).to(DEV).eval()
    m.knn_radius.fill_(0.9)
    with torch.no_grad():
        assert torch.equal(m.build_graph(src, dst, sym=sym, k=k, fused=True), m.build_graph(src, dst, sym=sym, k=k))
        assert_parity(m.edge_weights(src, dst, t[0], norm=True, fused=True), m.edge_weights(src, dst, t[0], norm=True),
                      TOL, "override")


def test_fused_edge_weights_against_reference_capture():
    """the bar of test_gpu_graph_construction.test_edge_weights_against_reference_capture, on the fused route"""
    from hierarchicalgnn_amd.graph_construction import DynamicGraphConstruction
    z = load_golden("bc_hgnn_L32.npz")
    hp = {k[3:]: z[k].item() for k in z.files if k.startswith("hp.")}
    hp["graph_construction"] = "fused"
    emb = torch.from_numpy(z["embeddings"]).to(DEV)
    means = torch.from_numpy(z["cell0.in.supernodes"])[:, :hp["emb_dim"]].contiguous().to(DEV)
    for name, fn, src, dst, gkey, wkey in (
            ("bipartite_graph_construction", "exp", emb, means, "cell0.in.bipartite_graph",
             "cell0.in.bipartite_edge_weights"),
            ("super_graph_construction", "sigmoid", means, means, "cell0.in.super_graph",
             "cell0.in.super_edge_weights")):
        m = DynamicGraphConstruction(fn, hp)
        pre = f"sd.hgnn_block.{name}."
        m.load_state_dict({k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}, strict=True)
        m = m.to(DEV).eval()
        assert m.fused
        graph = torch.from_numpy(z[gkey]).to(DEV)
        with torch.no_grad():
            w = m.edge_weights(src, dst, graph, norm=True)
        assert w.shape == z[wkey].shape
        assert rel_err(w.cpu().numpy(), z[wkey]) <= TOL, name


# ------------------------------------------------------------------ one model
def test_bc_message_passing_fused_route_equals_the_default_route():
    from hierarchicalgnn_amd.models import BC_MessagePassing
    z = load_golden("bc_hgnn_L32.npz")
    hp = {k[3:]: z[k].item() for k in z.files if k.startswith("hp.")}
    assert hp["latent"] == 32
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    x = torch.from_numpy(z["x"]).to(DEV)
    graph = torch.from_numpy(z["edge_index"]).to(DEV)
    assert 100 <= x.shape[0] <= 2000
    out = {}
    for route in ("torch", "fused"):
        model = BC_MessagePassing(dict(hp, graph_construction=route))
        model.load_state_dict(sd, strict=True)
        model = model.to(DEV).train()
        torch.manual_seed(0)
        bg, scores, _ = model(x, graph)
        scores.sum().backward()
        params = [p for p in model.parameters() if p.grad is not None]
        out[route] = (bg, scores.detach(), params[0].grad, params[-1].grad)
    t, f = out["torch"], out["fused"]
    assert torch.equal(t[0], f[0])
    assert_parity(f[1], t[1], TOL, "scores")
    assert_parity(f[2], t[2], TOL, "first weight's gradient")
    assert_parity(f[3], t[3], TOL, "last weight's gradient")
