"""hgnn_project_f32 (csrc/project_f32.hip), the narrow products (csrc/narrow_f32.hip), their operators and their routes
through ``fused`` (``set_project_f32`` / ``set_narrow_f32``).

  * bit-exact: the integer grids of tests/exact_tail_ref.py (every product and partial sum an integer below 2^22) at
    every shape and every M edge of the restated shape functions; the wide_a / wide_b grids are the ones no split-bf16
    kernel can pass.  tests/test_exact_tail_ref.py proves on the CPU that an emulation of each order contract passes
    every case and that every mutant fails every case it applies to;
  * views: weight blocks as column blocks of one [N, 3K] matrix, x as a column slice at a 16-byte offset, the output
    as a column slice inside a poisoned buffer, tab[N, 3] with 12-byte rows: all in place;
  * random data against the a-priori bars; two calls and a call on a second stream give the same bits;
  * routes: with a switch on each listed site is one native call and its library counter does not move; off, every
    output and gradient has the bits of the parent's expression; on against off only what the switch touches moves, and
    it stays inside the bar around a float64 evaluation; the checkpointed two-pass forward stays bitwise deterministic;
  * an InteractionGNNCell training step and the EC-IN latent-128 forward + training step against the reference's
    fixtures with all four switches on;
  * no library GEMM: a profiler over that EC-IN step sees no aten matrix product with all four switches on, and does
    see ``aten::mm`` with them off.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import exact_tail_ref as T
from conftest import assert_parity, load_golden, rel_err
from test_gpu_cells import TOL as CELL_TOL, _hp, _load
from test_gpu_configs import TOL as CONFIG_TOL, _cfg, _seeded, _sketch_close
from test_gpu_fused import _mk
from test_gpu_gemm_exact import assert_bits, f32_of, filler
from test_gpu_rows_exact import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
COUNTERS = ("project_f32_calls", "narrow_linear_calls", "narrow_outer_calls", "narrow_wgrad_calls",
            "library_project_calls", "library_head_calls", "library_dgrad_calls", "library_wgrad_calls",
            "wgrad_f32_calls", "bwd_layer_f32_calls")


def _L():
    from hierarchicalgnn_amd import _lib
    return _lib


def _ops():
    from hierarchicalgnn_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def lib():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _L().load()


@contextlib.contextmanager
def switches(project=False, narrow=False, wgrad=False, bwd_layer=False):
    from hierarchicalgnn_amd import fused
    old = fused._project_f32_on, fused._narrow_f32_on, fused._wgrad_f32_on, fused._bwd_layer_f32_on
    try:
        fused.set_project_f32(project)
        fused.set_narrow_f32(narrow)
        fused.set_wgrad_f32(wgrad)
        fused.set_bwd_layer_f32(bwd_layer)
        yield fused
    finally:
        fused.set_project_f32(old[0])
        fused.set_narrow_f32(old[1])
        fused.set_wgrad_f32(old[2])
        fused.set_bwd_layer_f32(old[3])


def _counts():
    from hierarchicalgnn_amd import fused
    return {k: fused.stats.get(k, 0) for k in COUNTERS}


def _moved(before):
    after = _counts()
    return {k: after[k] - before[k] for k in COUNTERS if after[k] != before[k]}


# ------------------------------------------------------------------ projection, bit-exact
def _project_raw(x, w0, w1, out0, out1):
    """the C entry on tensors as they are (views included)"""
    L = _L()
    M, K, N = x.shape[0], x.shape[1], w0.shape[0]
    ld = lambda t, w: int(t.stride(0)) if t.shape[0] > 1 else w
    L.check(L.load().hgnn_project_f32(L.ptr(x), ld(x, K), M, K, L.ptr(w0), L.ptr(w1), ld(w0, K), N,
                                      ctypes.c_void_p(out0.data_ptr()),
                                      ctypes.c_void_p(out1.data_ptr()) if out1 is not None else None,
                                      ld(out0, N) if M > 1 else max(N, int(out0.stride(0))),
                                      L.current_stream(x.device)), "hgnn_project_f32")


@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("grid", T.GRIDS)
@pytest.mark.parametrize("shape", T.PROJECT_SHAPES, ids=lambda s: f"K{s[0]}_N{s[1]}")
def test_projection_exact(shape, grid, blocks):
    """plain operands through the operator; then the weight blocks as column blocks of one [N, 3K] matrix, x as a
    column slice at a 16-byte offset and the outputs as column slices inside guarded buffers, all in place"""
    K, N = shape
    for M in T.project_m(N):
        x, w0, w1 = T.project_operands(grid, M, K, N, T.seed_of("project", grid, M, K, N))
        refs = [f32_of(T.project_ref(x, w)).to(DEV) for w in (w0, w1)][:blocks]
        x, w0, w1 = x.to(DEV), w0.to(DEV), w1.to(DEV)
        what = f"project_f32 {grid} M={M} K={K} N={N} blocks={blocks}"
        t = T.project_tiles(M, N, blocks)
        where = lambda r, h: f"row tile {r // 64} of {t['row_tiles']}, pass {h // t['pass_width']} of {t['passes']}"
        outs = _ops().project_f32(x, w0, w1 if blocks == 2 else None)
        assert len(outs) == blocks
        for b in range(blocks):
            assert_bits(outs[b], refs[b], f"{what} block {b}", where)
        if M == 0:
            continue
        # views
        wide = filler(N, 3 * K, 21, torch.float32)
        wide[:, :K], wide[:, 2 * K:] = w0, w1
        px = filler(M, K + 12, 22, torch.float32)
        px[:, 4:4 + K] = x
        xv, v0, v1 = px[:, 4:4 + K], wide[:, :K], wide[:, 2 * K:]
        assert xv.data_ptr() % 16 == 0 and v1.data_ptr() % 16 == 0
        guards = [Guarded(M, N + 8, torch.float32) for _ in range(blocks)]
        views = [g.out[:, 4:4 + N] for g in guards]
        _project_raw(xv, v0, v1 if blocks == 2 else None, views[0], views[1] if blocks == 2 else None)
        for b, g in enumerate(guards):
            g.check(f"{what} block {b} (views)")
            inner = g.bits[g.pad:g.bits.numel() - g.pad].view(M, -1)
            beside = torch.cat([inner[:, :4], inner[:, 4 + N:]], dim=1)
            assert bool((beside == g.poison).all()), f"{what}: wrote beside the column slice of out{b}"
            assert_bits(views[b].contiguous(), refs[b], f"{what} block {b} (views)", where)


def test_projection_operator_reads_column_blocks_in_place_and_pads(monkeypatch):
    lib = _L().load()
    real = lib.hgnn_project_f32
    seen = []

    def spy(x, ldx, M, K, w0, w1, ldw, *rest):
        seen.append((x.value, ldx, w0.value, w1.value, ldw))
        return real(x, ldx, M, K, w0, w1, ldw, *rest)

    monkeypatch.setattr(lib, "hgnn_project_f32", spy)
    K, N, M = 32, 64, 100
    x, w0, w1 = T.project_operands("wide_b", M, K, N, 5)
    W = filler(N, 3 * K, 3, torch.float32)
    W[:, :K], W[:, K:2 * K] = w0.to(DEV), w1.to(DEV)
    x = x.to(DEV)
    outs = _ops().project_f32(x, W[:, :K], W[:, K:2 * K], width=80)
    assert seen == [(x.data_ptr(), K, W.data_ptr(), W.data_ptr() + 4 * K, 3 * K)], "a readable column block was copied"
    for o, w in zip(outs, (w0, w1)):
        assert o.shape == (M, 80) and not bool(o[:, N:].any())
        assert_bits(o[:, :N].contiguous(), f32_of(T.project_ref(x.cpu(), w)).to(DEV), "padded projection")


# ------------------------------------------------------------------ narrow products, bit-exact
_dev_cache = {}


def _dev(t):
    """device copy; the 70,001-row wide-side array is uploaded once per K"""
    if t.shape[0] != T.BIG_M or t.shape[1] < 4 or t.numel() < T.BIG_M * 4:
        return t.to(DEV)
    key = (t.data_ptr(), tuple(t.shape))
    if key not in _dev_cache:
        _dev_cache.clear()
        _dev_cache[key] = t.to(DEV)
    return _dev_cache[key]


def _ws_bytes(M, n, K):
    b = ctypes.c_size_t(0)
    _L().check(_L().load().hgnn_wgrad_narrow_f32_workspace_bytes(M, n, K, ctypes.byref(b)), "workspace query")
    return b.value


@pytest.mark.parametrize("n", T.NARROW_N)
@pytest.mark.parametrize("K", T.NARROW_K)
def test_narrow_products_exact(K, n):
    ops = _ops()
    for M in T.narrow_m(n, K):
        for grid in T.grids_at(M):
            what = f"{grid} M={M} n={n} K={K}"
            x, W, bias = T.linear_operands(grid, M, K, n, T.seed_of("linear", grid, M, n, K))
            xd, Wd, bd = _dev(x), W.to(DEV), bias.to(DEV)
            assert_bits(ops.linear_narrow_f32(xd, Wd, bd), f32_of(T.linear_ref(x, W, bias)).to(DEV), "linear " + what)
            assert_bits(ops.linear_narrow_f32(xd, Wd), f32_of(T.linear_ref(x, W)).to(DEV), "linear, no bias, " + what)
            del xd
            y, W, add = T.outer_operands(grid, M, n, K, T.seed_of("outer", grid, M, n, K))
            yd, Wd, ad = y.to(DEV), W.to(DEV), _dev(add)
            assert_bits(ops.outer_narrow_f32(yd, Wd, ad), f32_of(T.outer_ref(y, W, add)).to(DEV), "outer " + what)
            assert_bits(ops.outer_narrow_f32(yd, Wd), f32_of(T.outer_ref(y, W)).to(DEV), "outer, no add, " + what)
            del ad
            y, x = T.wgrad_operands(grid, M, n, K, T.seed_of("wgrad", grid, M, n, K))
            r, cs = T.wgrad_ref(y, x)
            yd, xd = y.to(DEV), _dev(x)
            sh = T.wgrad_shape(M, n, K)
            where = lambda j, k: f"{sh['slices']} slices of {sh['rows_per_slice']} rows"
            colsum = torch.full((n,), float("nan"), device=DEV)
            assert_bits(ops.wgrad_narrow_f32(yd, xd, colsum=colsum), f32_of(r).to(DEV), "wgrad " + what, where)
            assert_bits(colsum, f32_of(cs).to(DEV), "wgrad colsum " + what)
            assert_bits(ops.wgrad_narrow_f32(yd, xd), f32_of(r).to(DEV), "wgrad, no colsum, " + what, where)
            assert _ws_bytes(M, n, K) == T.wgrad_workspace_bytes(M, n, K), what
            del xd


def test_table_with_12_byte_rows_is_read_in_place(monkeypatch):
    """y = tab[N, 3] (the encoders' table): the narrow side needs no 16-byte rows"""
    lib = _L().load()
    real = lib.hgnn_wgrad_narrow_f32
    seen = []

    def spy(y, ldy, n, x, ldx, *rest):
        seen.append((y.value, ldy, x.value, ldx))
        return real(y, ldy, n, x, ldx, *rest)

    monkeypatch.setattr(lib, "hgnn_wgrad_narrow_f32", spy)
    M, K = 1000, 128
    y, x = T.wgrad_operands("wide_b", M, 3, K, 77)
    parent = filler(M + 1, 3, 5, torch.float32)
    parent[1:] = y.to(DEV)
    tab = parent[1:]                                        # starts 12 bytes into the allocation
    px = filler(M, K + 8, 6, torch.float32)
    px[:, 4:4 + K] = x.to(DEV)
    xv = px[:, 4:4 + K]
    assert tab.data_ptr() % 16 == 12 and tab.stride(0) == 3
    out = _ops().wgrad_narrow_f32(tab, xv)
    assert seen == [(tab.data_ptr(), 3, xv.data_ptr(), K + 8)], "a readable operand was copied"
    assert_bits(out, f32_of(T.wgrad_ref(y, x)[0]).to(DEV), "wgrad of tab[N, 3]")


# ------------------------------------------------------------------ random data
_random = {}


def random_case():
    if not _random:
        g = torch.Generator().manual_seed(2024)
        rn = lambda *s: torch.randn(*s, generator=g).to(DEV)
        _random.update(x=rn(5000, 256), w0=rn(512, 256), w1=rn(512, 256), W=rn(6, 256), b=rn(6), y=rn(5000, 6),
                       add=rn(5000, 256))
    return _random


def _ratio(got, ref, bar):
    return float(((got.double().cpu() - ref).abs() / bar).max())


def test_random_data_inside_the_a_priori_bars():
    d = {k: v.cpu() for k, v in random_case().items()}
    c = random_case()
    ops = _ops()
    o0, o1 = ops.project_f32(c["x"], c["w0"], c["w1"])
    ratios = {"project0": _ratio(o0, T.project_ref(d["x"], d["w0"]), T.bar_project(d["x"], d["w0"])),
              "project1": _ratio(o1, T.project_ref(d["x"], d["w1"]), T.bar_project(d["x"], d["w1"])),
              "linear": _ratio(ops.linear_narrow_f32(c["x"], c["W"], c["b"]), T.linear_ref(d["x"], d["W"], d["b"]),
                               T.bar_linear(d["x"], d["W"], d["b"])),
              "outer": _ratio(ops.outer_narrow_f32(c["y"], c["W"], c["add"]), T.outer_ref(d["y"], d["W"], d["add"]),
                              T.bar_outer(d["y"], d["W"], d["add"]))}
    cs = torch.empty(6, device=DEV)
    out = ops.wgrad_narrow_f32(c["y"], c["x"], colsum=cs)
    (r, rcs), (bar, bar_cs) = T.wgrad_ref(d["y"], d["x"]), T.bar_wgrad(d["y"], d["x"])
    ratios["wgrad"], ratios["colsum"] = _ratio(out, r, bar), _ratio(cs, rcs, bar_cs)
    print("worst |err| / bar:", {k: round(v, 4) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0


def test_same_bits_in_every_call_and_on_a_second_stream():
    c = random_case()
    ops = _ops()

    def run():
        cs = torch.empty(6, device=DEV)
        return (*ops.project_f32(c["x"], c["w0"], c["w1"]), ops.linear_narrow_f32(c["x"], c["W"], c["b"]),
                ops.outer_narrow_f32(c["y"], c["W"], c["add"]), ops.wgrad_narrow_f32(c["y"], c["x"], colsum=cs), cs)

    first = run()
    for a, b in zip(run(), first):
        assert_bits(a, b, "second call")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = run()
    side.synchronize()
    for a, b in zip(other, first):
        assert_bits(a, b, "second stream")


# ------------------------------------------------------------------ routes
def _edge_update(L):
    """two gathered segments of one table + a direct segment that is also the skip (the edge network's shape)"""
    from hierarchicalgnn_amd import mlp
    g = torch.Generator().manual_seed(L)
    net = _mk(3 * L, L, 2, "Tanh", seed=L).cuda()
    n_tab, M = 300, 6000
    table0 = torch.randn(n_tab, L, generator=g).cuda()
    direct0 = torch.randn(M, L, generator=g).cuda()
    i0 = torch.randint(0, n_tab, (M,), generator=g).cuda()
    i1 = torch.randint(0, n_tab, (M,), generator=g).cuda()
    r = torch.randn(M, L, generator=g).cuda()

    def run(train=True):
        if not train:
            with torch.no_grad():
                return [("out", mlp.concat_mlp(net, [(table0, i0), (table0, i1), (direct0, None)], skip=direct0))]
        net.zero_grad(set_to_none=True)
        table = table0.clone().requires_grad_(True)
        direct = direct0.clone().requires_grad_(True)
        out = mlp.concat_mlp(net, [(table, i0), (table, i1), (direct, None)], skip=direct)
        (out * r).sum().backward()
        return [("out", out.detach()), ("table.grad", table.grad), ("direct.grad", direct.grad)] + \
               [(k, p.grad.clone()) for k, p in net.named_parameters()]

    return net, run, table0


def _node_update(L):
    """every segment direct, the first one also the skip; three layers (the node network's shape)"""
    from hierarchicalgnn_amd import mlp
    g = torch.Generator().manual_seed(7 * L)
    net = _mk(2 * L, L, 3, "GELU", seed=L + 2).cuda()
    M = 300
    rows0 = [torch.randn(M, L, generator=g).cuda() for _ in range(2)]
    r = torch.randn(M, L, generator=g).cuda()

    def run(train=True):
        if not train:
            with torch.no_grad():
                return [("out", mlp.concat_mlp(net, [(t, None) for t in rows0], skip=rows0[0]))]
        net.zero_grad(set_to_none=True)
        rows = [t.clone().requires_grad_(True) for t in rows0]
        out = mlp.concat_mlp(net, [(t, None) for t in rows], skip=rows[0])
        (out * r).sum().backward()
        return [("out", out.detach())] + [(f"rows{i}.grad", t.grad) for i, t in enumerate(rows)] + \
               [(k, p.grad.clone()) for k, p in net.named_parameters()]

    return net, run, None


@pytest.mark.parametrize("train", [False, True], ids=["no_grad", "train"])
@pytest.mark.parametrize("L", [32, 128])
@pytest.mark.parametrize("shape", ["edge_update", "node_update"])
def test_projection_route(shape, L, train):
    """the edge update's two gathered segments of one table are ONE hgnn_project_f32 launch per forward and no library
    projection is left; the node update (direct segments only) has no projection and does not move at all.  Off: the
    bits of the parent's ``torch.matmul``.  On against off: the projection is inside its bar around float64"""
    net, run, table = (_edge_update if shape == "edge_update" else _node_update)(L)
    n_proj = 1 if shape == "edge_update" else 0
    from hierarchicalgnn_amd import fused
    real = fused._preprojections
    seen = []

    def recording(tables, cols, proj, lin0, *rest):
        P = real(tables, cols, proj, lin0, *rest)
        seen.append((proj, cols, {i: p.detach() for i, p in P.items()}))
        return P

    def parent(tables, cols, proj, lin0, bf16, split_proj, width):
        """the parent's expression, restated"""
        assert not bf16 and not split_proj and not width
        return {i: torch.matmul(tables[i].detach(), lin0.weight.detach()[:, cols[i][0]:cols[i][1]].t()) for i in proj}

    with switches() as fused:
        fused._preprojections = parent
        try:
            want = run(train)
        finally:
            fused._preprojections = real
        c0 = _counts()
        off = run(train)
        assert _moved(c0).get("library_project_calls", 0) == 2 * n_proj and "project_f32_calls" not in _moved(c0)
        for (name, a), (_, b) in zip(off, want):
            assert_bits(a, b, f"switch off, {name}: not the bits of the parent's expression")
    with switches(project=True) as fused:
        fused._preprojections = recording
        try:
            c0 = _counts()
            on = run(train)
            moved = _moved(c0)
        finally:
            fused._preprojections = real
        assert moved.get("project_f32_calls", 0) == n_proj and "library_project_calls" not in moved, moved
        assert_bits(run(train)[0][1], on[0][1], "two runs with the switch on")
    if n_proj == 0:
        for (name, a), (_, b) in zip(on, off):
            assert_bits(a, b, f"no projection in this shape, {name}")
        return
    assert len(seen) == 1 and len(seen[0][2]) == 2
    proj, cols, P = seen[0]
    W = net[0].weight.detach().double().cpu()
    worst = 0.0
    for i in proj:
        w = W[:, cols[i][0]:cols[i][1]].float()
        ratio = _ratio(P[i], T.project_ref(table.cpu(), w), T.bar_project(table.cpu(), w))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (i, ratio)
    print(f"{shape} L={L} train={train}: worst |P - ref64| / bar = {worst:.4f}")


def _head(L, w):
    """a score head K -> H -> H -> w on direct rows (IN.py:107-115)"""
    from hierarchicalgnn_amd import mlp
    from hierarchicalgnn_amd import make_mlp
    g = torch.Generator().manual_seed(31 * L + w)
    torch.manual_seed(L + w)
    net = make_mlp(2 * L, 2 * L, w, 3, layer_norm=True, output_activation=None, hidden_activation="GELU").cuda()
    M = 3000
    rows0 = torch.randn(M, 2 * L, generator=g).cuda()
    r = torch.randn(M, w, generator=g).cuda()

    def run(train=True):
        if not train:
            with torch.no_grad():
                return [("out", mlp.concat_mlp(net, [(rows0, None)], skip=None))]
        net.zero_grad(set_to_none=True)
        rows = rows0.clone().requires_grad_(True)
        out = mlp.concat_mlp(net, [(rows, None)], skip=None)
        (out * r).sum().backward()
        return [("out", out.detach()), ("rows.grad", rows.grad)] + [(k, p.grad.clone()) for k, p in net.named_parameters()]

    return net, run


@pytest.mark.parametrize("w", [1, 8])
@pytest.mark.parametrize("L,train", [(32, True), (128, True), (512, False)], ids=["L32_train", "L128_train", "L512_chain"])
def test_head_route(L, w, train):
    """the plain last Linear of a head: one linear call per forward (+ one outer and one wgrad call in the backward),
    no library head call; off, the bits of the parent's ``F.linear`` on the hidden rows (and of autograd through it);
    on, each of the three products is inside its a-priori bar around a float64 evaluation of the same operands.  The
    no-grad branch is reached through the fp32 chain of latent 512 (hidden 1024): an exact no-grad head at latent <= 256
    runs its last Linear inside the fused kernel"""
    from hierarchicalgnn_amd import fused
    net, run = _head(L, w)
    real_head = fused._head_linear
    with switches():
        fused._head_linear = lambda hidden, lin, differentiable: None      # the parent: the library expression alone
        try:
            want = run(train)
        finally:
            fused._head_linear = real_head
        c0 = _counts()
        off = run(train)
        assert _moved(c0).get("library_head_calls", 0) == 1
        assert not any(k.startswith("narrow_") for k in _moved(c0))
        for (name, a), (_, b) in zip(off, want):
            assert_bits(a, b, f"switch off, {name}: not the bits of the parent's expression")
    ops = _ops()
    real = ops.linear_narrow_f32, ops.outer_narrow_f32, ops.wgrad_narrow_f32
    calls = []

    def recorder(kind, fn):
        def f(*a, **kw):
            out = fn(*a, **kw)
            if not done:
                calls.append((kind, [t.detach().cpu() for t in a[:2]], out.detach().clone()))
            return out
        return f

    done = []
    with switches(narrow=True):
        ops.linear_narrow_f32, ops.outer_narrow_f32, ops.wgrad_narrow_f32 = \
            [recorder(k, f) for k, f in zip(("linear", "outer", "wgrad"), real)]
        try:
            c0 = _counts()
            on = run(train)
            moved = _moved(c0)
            done.append(True)
            again = run(train)
        finally:
            ops.linear_narrow_f32, ops.outer_narrow_f32, ops.wgrad_narrow_f32 = real
    assert "library_head_calls" not in moved, moved
    assert moved.get("narrow_linear_calls", 0) == 1, moved
    assert moved.get("narrow_outer_calls", 0) == (1 if train else 0), moved
    assert moved.get("narrow_wgrad_calls", 0) == (1 if train else 0), moved
    for (name, a), (_, b) in zip(again, on):
        assert_bits(a, b, f"two runs with the switch on, {name}")
    # what the head's hidden layers compute does not depend on the switch: the hidden rows handed to the narrow Linear
    # are the ones the library saw
    kinds = [c[0] for c in calls]
    assert kinds == (["linear", "outer", "wgrad"] if train else ["linear"]), kinds
    Wc, bc = net[-1].weight.detach().cpu(), net[-1].bias.detach().cpu()
    for kind, args, out in calls:
        if kind == "linear":
            ratio = _ratio(out, T.linear_ref(args[0], Wc, bc), T.bar_linear(args[0], Wc, bc))
            assert_bits(out, on[0][1], "the head's output is the narrow Linear's")
        elif kind == "outer":
            ratio = _ratio(out, T.outer_ref(args[0], Wc), T.bar_outer(args[0], Wc))
        else:
            (r, rcs), (bar, bar_cs) = T.wgrad_ref(args[0], args[1]), T.bar_wgrad(args[0], args[1])
            ratio = max(_ratio(out, r, bar), _ratio(dict(on)[f"{len(net) - 1}.bias"], rcs, bar_cs))
            assert_bits(out, dict(on)[f"{len(net) - 1}.weight"], "the last Linear's weight gradient is the narrow wgrad's")
        print(f"head L={L} w={w} {kind}: worst |err| / bar = {ratio:.4f}")
        assert ratio <= 1.0, (kind, ratio)


def _encoder(L):
    """an encoder on a 3-wide table (the hits' coordinates): the first layer's weight gradient is tab^T dz with a
    3-wide side, its input gradient dz . W with w_s = 3"""
    from hierarchicalgnn_amd import mlp
    g = torch.Generator().manual_seed(5 * L)
    net = _mk(3, L, 2, "GELU", seed=L + 9).cuda()
    M = 5000
    tab0 = torch.randn(M, 3, generator=g).cuda()
    r = torch.randn(M, L, generator=g).cuda()

    def run():
        net.zero_grad(set_to_none=True)
        tab = tab0.clone().requires_grad_(True)
        out = mlp.concat_mlp(net, [(tab, None)], skip=None)
        (out * r).sum().backward()
        return [("out", out.detach()), ("tab.grad", tab.grad)] + [(k, p.grad.clone()) for k, p in net.named_parameters()]

    return net, run


@pytest.mark.parametrize("L", [64, 128])
def test_encoder_route(L):
    """the 3-wide first layer: ``_atb(dz, tab[N, 3])`` is one narrow wgrad call and ``dz @ W_s`` one narrow linear call,
    the library counters do not move; off, nothing is counted for the narrow kernels; on against off only
    ``0.weight.grad`` and ``tab.grad`` move, inside the a-priori bars around float64 (checked on the recorded operands)"""
    from hierarchicalgnn_amd import fused
    net, run = _encoder(L)
    real_atb, real_dgrad = fused._atb, fused._narrow_dgrad
    calls = []

    def recording_atb(A, B, net=None):
        out = real_atb(A, B, net)
        calls.append(("atb", A.detach(), B.detach(), out.detach()))
        return out

    def recording_dgrad(x, W_s, weight, cols):
        out = real_dgrad(x, W_s, weight, cols)
        if out is not None:
            calls.append(("dgrad", x.detach(), W_s.detach(), out.detach()))
        return out

    with switches() as fused:
        t0 = fused.stats["fused_train_calls"]
        c0 = _counts()
        off = run()
        assert fused.stats["fused_train_calls"] == t0 + 1, "the fused training route did not run"
        assert not any(k.startswith("narrow_") for k in _moved(c0)), _moved(c0)
    with switches(narrow=True) as fused:
        fused._atb, fused._narrow_dgrad = recording_atb, recording_dgrad
        try:
            c0 = _counts()
            on = run()
            moved = _moved(c0)
        finally:
            fused._atb, fused._narrow_dgrad = real_atb, real_dgrad
    assert moved.get("narrow_wgrad_calls", 0) == 1 and moved.get("narrow_linear_calls", 0) == 1, moved
    assert "library_dgrad_calls" not in moved and moved.get("library_wgrad_calls", 0) == 1, moved   # the L x L layer
    touched = {"0.weight", "tab.grad"}
    for (name, a), (_, b) in zip(on, off):
        if name not in touched:
            assert_bits(a, b, f"switch on against off, {name}")
    for kind, A, B, out in calls:
        A, B = A.cpu(), B.cpu()
        if kind == "dgrad":                       # x [M, H] . W_s [H, 3]
            ratio = _ratio(out, T.linear_ref(A, B.t()), T.bar_linear(A, B.t()))
        elif min(A.shape[1], B.shape[1]) <= 32:   # dz^T tab, the narrow side second: the transposed narrow product
            ratio = _ratio(out.t(), T.wgrad_ref(B, A)[0], T.bar_wgrad(B, A)[0])
        else:
            continue
        assert ratio <= 1.0, (kind, tuple(A.shape), tuple(B.shape), ratio)


def test_checkpointed_two_pass_forward_is_bitwise_deterministic():
    """an InteractionGNNCell training step twice with all four switches on: the recompute of the checkpoint segment and
    the first pass use the same kernels, so outputs and gradients repeat bit for bit"""
    import hierarchicalgnn_amd as H
    z = load_golden("ignn_cell_L32.npz")
    cell = _load(H.InteractionGNNCell(_hp(32)), z)

    def step():
        cell.zero_grad(set_to_none=True)
        nodes = torch.from_numpy(z["nodes"]).cuda().requires_grad_(True)
        edges = torch.from_numpy(z["edges"]).cuda().requires_grad_(True)
        on, oe = torch.utils.checkpoint.checkpoint(cell, nodes, edges, torch.from_numpy(z["graph"]).cuda(),
                                                   use_reentrant=True)
        ((on * torch.from_numpy(z["r_nodes"]).cuda()).sum() + (oe * torch.from_numpy(z["r_edges"]).cuda()).sum()).backward()
        return [on.detach(), oe.detach(), nodes.grad, edges.grad] + [p.grad.clone() for p in cell.parameters()]

    with switches(project=True, narrow=True, wgrad=True, bwd_layer=True):
        c0 = _counts()
        first = step()
        assert _moved(c0).get("project_f32_calls", 0) >= 2, _moved(c0)      # both passes
        second = step()
    for i, (a, b) in enumerate(zip(first, second)):
        assert_bits(a, b, f"tensor {i} of the second step")


# ------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("latent", [32, 128])
def test_interaction_cell_training_step_against_the_reference(latent):
    import hierarchicalgnn_amd as H
    z = load_golden(f"ignn_cell_L{latent}.npz")
    cell = _load(H.InteractionGNNCell(_hp(latent)), z)
    nodes = torch.from_numpy(z["nodes"]).cuda().requires_grad_(True)
    edges = torch.from_numpy(z["edges"]).cuda().requires_grad_(True)
    graph = torch.from_numpy(z["graph"]).cuda()
    with switches(project=True, narrow=True, wgrad=True, bwd_layer=True):
        c0 = _counts()
        on, oe = cell(nodes, edges, graph)
        ((on * torch.from_numpy(z["r_nodes"]).cuda()).sum() + (oe * torch.from_numpy(z["r_edges"]).cuda()).sum()).backward()
        moved = _moved(c0)
    assert moved.get("project_f32_calls", 0) >= 1 and "library_project_calls" not in moved, moved
    for k, p in cell.named_parameters():
        got, want = p.grad.cpu().numpy().astype(np.float64), z["grad." + k].astype(np.float64)
        assert rel_err(got, want) <= CELL_TOL, k
        assert np.linalg.norm(got - want) <= CELL_TOL * np.linalg.norm(want), k


def _ec_in():
    from hierarchicalgnn_amd.models import EC_InteractionGNN
    z = load_golden("ec_in_L128.npz")
    model = _seeded(EC_InteractionGNN, _cfg("EC-IN"), z)
    return model, z, torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["edge_index"]).cuda()


def test_ec_in_latent128_against_the_reference_with_all_switches_on():
    model, z, x, graph = _ec_in()
    with switches(project=True, narrow=True, wgrad=True, bwd_layer=True):
        c0 = _counts()
        with torch.inference_mode():
            scores = model(x, graph)
        assert np.abs(scores.cpu().numpy() - z["scores"]).max() <= CONFIG_TOL
        assert_parity(scores, z["scores"], CONFIG_TOL, "scores")
        x = x.clone()
        scores = model(x, graph)
        (scores * torch.from_numpy(z["r_scores"]).cuda()).sum().backward()
        moved = _moved(c0)
    print("EC-IN L128, all switches on:", moved)
    assert moved.get("project_f32_calls", 0) > 0 and moved.get("narrow_linear_calls", 0) > 0
    assert moved.get("narrow_wgrad_calls", 0) > 0
    assert_parity(x.grad, z["grad_x"], CONFIG_TOL, "d loss / d x")
    _sketch_close(model, z)


# ------------------------------------------------------------------ no library GEMM
GEMM_OPS = ("aten::mm", "aten::addmm", "aten::bmm", "aten::baddbmm", "aten::mv", "aten::addmv", "aten::_scaled_mm")


def _profiled_step(model, z, x, graph):
    from torch.profiler import ProfilerActivity, profile
    model.zero_grad(set_to_none=True)
    x = x.clone()
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        scores = model(x, graph)
        loss = (scores * torch.from_numpy(z["r_scores"]).cuda()).sum()
        loss.backward()
        torch.cuda.synchronize()
    names = {}
    for e in prof.events():
        if e.name in GEMM_OPS:
            names[e.name] = names.get(e.name, 0) + 1
    return names


def test_exact_training_step_issues_no_library_gemm():
    """EC-IN latent 128, forward + loss + backward under the CPU profiler (it records autograd's thread too: with the
    switches off the same detector sees ``aten::mm``).  All four switches on: no aten matrix product at all, and no
    ``library_*`` counter moves"""
    model, z, x, graph = _ec_in()
    with switches():
        off = _profiled_step(model, z, x, graph)
    print("switches off:", off)
    assert off.get("aten::mm", 0) > 0, "the detector does not see the library GEMMs of the default route"
    with switches(project=True, narrow=True, wgrad=True, bwd_layer=True):
        c0 = _counts()
        on = _profiled_step(model, z, x, graph)
        moved = _moved(c0)
    print("all four switches on:", on, moved)
    assert on == {}, f"library GEMMs left in the exact step: {on}"
    assert not any(k.startswith("library_") for k in moved), moved
