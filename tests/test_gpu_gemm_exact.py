"""Exact conformance of the matrix kernels of the training path and of the persistent tile loops.

Inputs come from the integer grids of tests/gemm_ref.py (every product and partial sum an integer below 2^22 -- two
bits under fp32's exact range, because the term alignment inside the bf16 matrix instruction is not measured), so
every comparison is ``torch.equal`` on the bits against a float64 product of the same tensors on the device; bf16
outputs are that sum rounded once to nearest even.  tests/test_gemm_ref.py proves the references and proves, with
mutants, that no case here is vacuous.  Outputs of the C ABI calls live in poisoned buffers (>= 64 guard elements on
either side, and the columns beside a column slice); every entry is called twice and must return the same bits.

  a  hgnn_wgrad_bf16             128x128 / 256x128 / 256x256 tiles, partial tiles, every M edge of wg::shape_for (a
                                 last slice of 1 / 32 / all rows, >= 5 slices), colsum, lda > Ho and ldb > Hi with
                                 ldo > Hi, the slice count behind hgnn_wgrad_workspace_bytes
  b  hgnn_wgrad_f32_split3       one partial and one full shape per tile; small / mid_a / mid_b / mid_both (all four
                                 products), colsum of a mid operand
  c  hgnn_mlp_backward_layer_bf16, input form: N x K x the 64-row tile edges, skip rows, W a column slice; two full
                                 trips of the 512-workgroup tile loop + 65 rows
  d  hgnn_linear_f32_split3 (four products) and hgnn_project_f32_split3 (three; one and two weight streams)
  e  trip invariance: the rows of trips 2 and 3 of every persistent tile loop, recomputed by a call of their own, have
     the same bits (LayerNorm and input form of the backward layer; the split-bf16 fp32 forward at latent 128 with
     two / three layers and latent 256 on 64- and 128-row tiles, inference and training forward with its dumps)
  f  misaligned operand views of the two weight-gradient wrappers are copied, not refused

A trip covers ``gemm_ref.trip_rows`` rows: 512 x 64 for the backward layer; CUs x residency x tile rows for the
forward (the CU count is read from the device; on the 256 CUs of an MI355X: 32,768 / 32,768 / 16,384 / 32,768 rows
for latent 128 x2, x3, latent 256 on 64- and on 128-row tiles).

Wall time of this file on an MI355X: 9.3 s for the 199 tests; the slowest case 1.0 s (the first LayerNorm-form trip
test, which also pays the float64 autograd reference), the three-trip backward-layer cases 0.3-0.6 s.
"""
import ctypes

import pytest
import torch

import gemm_ref as G
import ln_ref
import rows_ref as R
from test_gpu_rows_exact import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def lib():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from hierarchicalgnn_amd import _lib
    return _lib.load()


@pytest.fixture()
def split3():
    """the split-bf16 kernels for no-grad forwards AND under autograd (as tests/test_gpu_split3.py)"""
    from hierarchicalgnn_amd import fused
    old, old_b = fused._fp32_split3, fused._fp32_split3_train
    fused.set_fp32_split3(True)
    fused.set_fp32_split3_training(True)
    yield fused
    fused.set_fp32_split3(old)
    fused.set_fp32_split3_training(old_b)


def _L():
    from hierarchicalgnn_amd import _lib
    return _lib


def cus() -> int:
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()]) if t.is_floating_point() else t


def assert_bits(out, ref, what, where=None):
    """equal bits at every element; on failure name the first wrong element and (``where(row, col)``) its coordinates"""
    assert out.shape == ref.shape, (what, tuple(out.shape), tuple(ref.shape))
    ob, rb = _bits(out), _bits(ref)
    assert ob.dtype == rb.dtype, (what, out.dtype, ref.dtype)
    if torch.equal(ob, rb):
        return
    bad = torch.nonzero(ob != rb)
    idx = tuple(int(i) for i in bad[0])
    show = lambda t: float(G.bits_to_float(t[idx].cpu()) if t.dtype == torch.int16 else t[idx])
    at = f" ({where(*idx)})" if where is not None else ""
    raise AssertionError(f"{what}: {bad.shape[0]} of {ob.numel()} elements differ; first at {list(idx)}{at}: "
                         f"got {show(out)}, want {show(ref)}")


def f32_of(s):
    """the float64 integers ``s`` as fp32 (exact below 2^24)"""
    f = s.float()
    assert torch.equal(f.double(), s)
    return f


def filler(rows, cols, seed, dtype):
    """non-zero grid values for the columns beside a column slice: a read of the wrong column changes the result"""
    return G.small(rows, cols, seed).to(DEV).to(dtype)


# ------------------------------------------------------------------ a, b: the split-K weight gradients
WGRAD_FORMS = ("plain", "with_colsum", "slices")


def run_wgrad(fn, dz, rows, form):
    """``fn`` = ops.wgrad_bf16 / ops.wgrad_f32_split3 on device operands of its dtype, in one of three forms: plain;
    with colsum; operands AND out as column slices of wider parents (lda > Ho, ldb > Hi, ldo > Hi at an odd column
    offset) with colsum.  Returns (out, colsum or None) after the guard checks."""
    M, Ho, Hi = dz.shape[0], dz.shape[1], rows.shape[1]
    what = f"{fn.__name__} M={M} Ho={Ho} Hi={Hi} {form}"
    if form == "slices":
        per16 = 16 // dz.element_size()
        pa = filler(M, Ho + 3 * per16, 11, dz.dtype)
        pb = filler(M, Hi + 5 * per16, 12, dz.dtype)
        pa[:, per16:per16 + Ho] = dz
        pb[:, 2 * per16:2 * per16 + Hi] = rows
        dz, rows = pa[:, per16:per16 + Ho], pb[:, 2 * per16:2 * per16 + Hi]
        assert M < 2 or (dz.stride(0) > Ho and rows.stride(0) > Hi)
        g = Guarded(Ho, Hi + 5, torch.float32)
        out = g.out[:, 3:3 + Hi]
    else:
        g = Guarded(Ho, Hi, torch.float32)
        out = g.out
    cs = Guarded(1, Ho, torch.float32) if form != "plain" else None
    got = fn(dz, rows, out=out, colsum=cs.out.view(-1) if cs is not None else None)
    assert got.data_ptr() == out.data_ptr()
    g.check(what)
    inner = g.bits[g.pad:g.bits.numel() - g.pad].view(Ho, -1)
    if form == "slices":
        beside = torch.cat([inner[:, :3], inner[:, 3 + Hi:]], dim=1)
        assert bool((beside == g.poison).all()), f"{what}: wrote beside the column slice of out"
        inner = inner[:, 3:3 + Hi]
    assert not bool((inner == g.poison).any()), f"{what}: output elements never written"
    if cs is not None:
        cs.check(what + " colsum")
        cs.all_written(what + " colsum")
    return out, (cs.out.view(-1) if cs is not None else None)


def check_wgrad(fn, dz, rows, form):
    M, Ho, Hi = dz.shape[0], dz.shape[1], rows.shape[1]
    sh = G.shape_for(M, Ho, Hi)
    out, cs = run_wgrad(fn, dz, rows, form)
    ref, ref_cs = G.wgrad_ref(dz, rows)
    where = lambda ho, hi: (f"ho tile {ho // sh['to']}, hi tile {hi // sh['ti']} of {sh['to']}x{sh['ti']}; "
                            f"{sh['slices']} slices of {sh['rows_per_slice']} rows")
    what = f"{fn.__name__} M={M} Ho={Ho} Hi={Hi} {form}"
    assert_bits(out, f32_of(ref), what, where)
    if cs is not None:
        assert_bits(cs, f32_of(ref_cs), what + " colsum",
                    lambda ho: f"ho tile {ho // sh['to']}; {sh['slices']} slices")
    again = fn(dz, rows)                                   # second call, fresh output: the same bits
    assert_bits(again, out.contiguous(), what + " (second call)", where)
    # the slice count behind the workspace size is the restatement's
    n = ctypes.c_size_t(0)
    _L().check(_L().load().hgnn_wgrad_workspace_bytes(M, Ho, Hi, ctypes.byref(n)), "hgnn_wgrad_workspace_bytes")
    assert n.value % ((Ho * Hi + Ho) * 4) == 0 and n.value // ((Ho * Hi + Ho) * 4) == sh["slices"], (what, n.value, sh)


@pytest.mark.parametrize("form", WGRAD_FORMS)
@pytest.mark.parametrize("shape", [s for s, _ in G.WGRAD_SHAPES], ids=lambda s: f"{s[0]}x{s[1]}")
def test_wgrad_bf16_exact(shape, form):
    from hierarchicalgnn_amd.ops import wgrad_bf16
    Ho, Hi = shape
    for M in G.m_edges(Ho, Hi):
        dz, rows = G.wgrad_operands("small", M, Ho, Hi, G.wgrad_seed("small", M, Ho, Hi))
        check_wgrad(wgrad_bf16, dz.to(DEV).bfloat16(), rows.to(DEV).bfloat16(), form)


@pytest.mark.parametrize("grid", G.GRIDS)
@pytest.mark.parametrize("shape", G.WGRAD_S3_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_wgrad_f32_split3_exact(shape, grid):
    """all four products: the result is the float64 product on every grid, mid_both included; colsum of a mid operand
    (mid_a, mid_both); the column-slice form on the small grid"""
    from hierarchicalgnn_amd.ops import wgrad_f32_split3
    Ho, Hi = shape
    for M in G.m_edges(Ho, Hi):
        dz, rows = G.wgrad_operands(grid, M, Ho, Hi, G.wgrad_seed(grid, M, Ho, Hi))
        check_wgrad(wgrad_f32_split3, dz.to(DEV), rows.to(DEV), "slices" if grid == "small" else "with_colsum")


# ------------------------------------------------------------------ f: misaligned operand views
@pytest.mark.parametrize("which", ["column_offset", "row_stride"])
def test_wgrad_bf16_copies_a_view_the_kernel_cannot_read(which):
    """``wide[:, 4:132]`` starts 8 bytes off a 16-byte boundary; a 388-column parent has a row stride that is no
    multiple of 8 elements: the wrapper copies such an operand (as wgrad_f32_split3 does) instead of refusing it"""
    from hierarchicalgnn_amd.ops import wgrad_bf16
    M, Ho, Hi = 257, 64, 128
    dz, rows = G.wgrad_operands("small", M, Ho, Hi, 5)
    dz = dz.to(DEV).bfloat16()
    wide = filler(M, 388 if which == "row_stride" else 392, 6, torch.bfloat16)
    c0 = 8 if which == "row_stride" else 4
    wide[:, c0:c0 + Hi] = rows.to(DEV).bfloat16()
    view = wide[:, c0:c0 + Hi]
    assert view.data_ptr() % 16 != 0 if which == "column_offset" else view.stride(0) % 8 != 0
    ref, ref_cs = G.wgrad_ref(dz, view)
    assert_bits(wgrad_bf16(dz, view), f32_of(ref), f"wgrad_bf16 rows view ({which})")
    cs = torch.empty(Hi, device=DEV)
    ref_t, ref_cs = G.wgrad_ref(view, dz)
    assert_bits(wgrad_bf16(view, dz, colsum=cs), f32_of(ref_t), f"wgrad_bf16 dz view ({which})")
    assert_bits(cs, f32_of(ref_cs), f"wgrad_bf16 dz view ({which}) colsum")


@pytest.mark.parametrize("which", ["column_offset", "row_stride"])
def test_wgrad_f32_split3_copies_a_view_the_kernel_cannot_read(which):
    """column offset 1 (4 bytes off) and a 387-column parent (row stride no multiple of 4 floats)"""
    from hierarchicalgnn_amd.ops import wgrad_f32_split3
    M, Ho, Hi = 257, 64, 128
    dz, rows = G.wgrad_operands("mid_b", M, Ho, Hi, 7)
    dz = dz.to(DEV)
    wide = filler(M, 387 if which == "row_stride" else 388, 8, torch.float32)
    c0 = 4 if which == "row_stride" else 1
    wide[:, c0:c0 + Hi] = rows.to(DEV)
    view = wide[:, c0:c0 + Hi]
    assert view.data_ptr() % 16 != 0 if which == "column_offset" else view.stride(0) % 4 != 0
    ref, _ = G.wgrad_ref(dz, view)
    assert_bits(wgrad_f32_split3(dz, view), f32_of(ref), f"wgrad_f32_split3 rows view ({which})")
    cs = torch.empty(Hi, device=DEV)
    ref_t, ref_cs = G.wgrad_ref(view, dz)
    assert_bits(wgrad_f32_split3(view, dz, colsum=cs), f32_of(ref_t), f"wgrad_f32_split3 dz view ({which})")
    assert_bits(cs, f32_of(ref_cs), f"wgrad_f32_split3 dz view ({which}) colsum")


# ------------------------------------------------------------------ c: the input form of the bf16 backward layer
def bwd_layer_guarded(dz, W, skip):
    """hgnn_mlp_backward_layer_bf16, input form, into a guarded buffer (what fused._bwd_layer does, with our ``out``)"""
    from hierarchicalgnn_amd import fused
    L = _L()
    M, K, N = int(dz.shape[0]), int(dz.shape[1]), int(W.shape[1])
    wt = fused._fragment_order(W.detach().t().to(torch.bfloat16).contiguous())
    g = Guarded(M, N, torch.bfloat16)
    L.check(L.load().hgnn_mlp_backward_layer_bf16(L.ptr(dz), M, K, N, L.ptr(wt), None, None, None, 0, 1e-5,
                                                   L.ptr(skip), g.ptr(), None, None, L.current_stream(dz.device)),
            "hgnn_mlp_backward_layer_bf16")
    g.all_written("backward layer")
    return g.check("backward layer")


def where_bwd(row, col):
    trip, wg, tile = G.trip_of_row("bwd_layer", row, 0)
    return f"tile {tile} = trip {trip + 1} of workgroup {wg}, row {row % 64} of the tile"


def check_dgrad(dz, W, skip, what):
    from hierarchicalgnn_amd import fused
    s = dz.double() @ W.bfloat16().double()
    if skip is not None:
        s = s + skip.double()
    ref = R.bf16_bits_rne(f32_of(s))
    out = bwd_layer_guarded(dz, W, skip)
    assert_bits(out.view(torch.int16), ref, what, where_bwd)
    again = fused._bwd_layer(dz, W, None, None, None, 0, 1e-5, skip=skip)[0]
    assert again.dtype == torch.bfloat16
    assert_bits(again.view(torch.int16), ref, what + " (through fused._bwd_layer)", where_bwd)


DGRAD_FORMS = ("plain", "skip", "skip_wslice")


def _dgrad_case(M, K, N, form):
    dz, W, skip = G.dgrad_operands(M, K, N, G.dgrad_seed(M, K, N), form != "plain")
    dz, W = dz.to(DEV).bfloat16(), W.to(DEV)
    skip = skip.to(DEV).bfloat16() if skip is not None else None
    if form == "skip_wslice":                              # W: a column slice of a wider weight, as for a segment
        full = filler(K, 3 * N, 21, torch.float32)
        full[:, N:2 * N] = W
        W = full[:, N:2 * N]
    return dz, W, skip


@pytest.mark.parametrize("form", DGRAD_FORMS)
@pytest.mark.parametrize("K", G.DGRAD_K)
@pytest.mark.parametrize("N", G.DGRAD_N)
def test_backward_layer_input_form_exact(N, K, form):
    for M in G.TILE_M:
        check_dgrad(*_dgrad_case(M, K, N, form), f"backward layer input form M={M} K={K} N={N} {form}")


@pytest.mark.parametrize("N", G.DGRAD_N)
def test_backward_layer_input_form_exact_over_three_trips(N):
    """M = two full trips of the 512 x 64-row tile loop + 65 rows (a full tile and a one-row tile in trip 3)"""
    from hierarchicalgnn_amd import _lib
    assert _lib.MLP_BWD_BLOCKS == G.BWD_LAYER_BLOCKS
    M = 2 * G.trip_rows("bwd_layer", cus()) + 65
    check_dgrad(*_dgrad_case(M, 128, N, "skip"), f"backward layer input form M={M} K=128 N={N}")


# ------------------------------------------------------------------ d: the split-bf16 fp32 GEMMs
def where_rows64(row, col):
    return f"row tile {row // 64}, row {row % 64} of the tile, 16-column tile {col // 16}"


def _weight_with_block(b_t, seed):
    """an fp32 Linear weight [rows of b_t, 3 x its columns] whose middle column block is ``b_t``; the blocks beside it
    hold other non-zero values"""
    n = b_t.shape[1]
    W = filler(b_t.shape[0], 3 * n, seed, torch.float32)
    W[:, n:2 * n] = b_t
    return torch.nn.Parameter(W), (n, 2 * n)


@pytest.mark.parametrize("cols", [False, True], ids=["whole", "block"])
@pytest.mark.parametrize("grid", G.GRIDS)
@pytest.mark.parametrize("K", G.LINEAR_K)
@pytest.mark.parametrize("N", G.LINEAR_N)
def test_linear_f32_split3_exact(split3, N, K, grid, cols):
    """x . W[:, cols] through fused._split3_linear.  The kernel forms all FOUR products (k_linear_f32_split3<.., FOUR =
    true>, the data gradient of the fp32 training backward), so on every grid -- mid_both included -- the result is the
    float64 product, and on mid_both it must differ from the three-product sum."""
    L = _L()
    for M in G.TILE_M:
        a, b = G.operands(grid, M, K, N, G.linear_seed(grid, M, K, N))
        x, b = a.to(DEV), b.to(DEV)
        if cols:
            weight, c = _weight_with_block(b, 31)              # Linear weight [K out, 3N in]
        else:
            weight, c = torch.nn.Parameter(b.clone()), None
        what = f"linear_f32_split3 M={M} K={K} N={N} {grid} cols={c}"
        ref = f32_of(G.split3_ref(x, b, four=True))
        assert torch.equal(ref.double(), x.double() @ b.double())
        if grid == "mid_both":
            assert not torch.equal(G.split3_ref(x, b, four=False), ref.double())
        n0 = split3.stats.get("split3_linear_calls", 0)
        out = split3._split3_linear(x, weight, c, torch.nn.Sequential())
        assert out is not None and split3.stats.get("split3_linear_calls", 0) == n0 + 1
        assert_bits(out, ref, what, where_rows64)
        Wv = split3._split3_weight(weight, None if c is None else (tuple(c),), False, transpose=True)
        g = Guarded(M, N, torch.float32)
        L.check(L.load().hgnn_linear_f32_split3(L.ptr(x), M, K, L.ptr(Wv), N, None, g.ptr(),
                                                L.current_stream(x.device)), "hgnn_linear_f32_split3")
        g.all_written(what)
        assert_bits(g.check(what), ref, what + " (guarded, second call)", where_rows64)


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("grid", G.GRIDS)
@pytest.mark.parametrize("K", G.LINEAR_K)
@pytest.mark.parametrize("N", G.LINEAR_N)
def test_project_f32_split3_exact(split3, N, K, grid, streams):
    """table . W[:, cols]^T through fused._split3_project, one and two weight streams over the same table.  THREE
    products: bitwise the float64 product on small / mid_a / mid_b, and split3_ref(four=False) on mid_both."""
    L = _L()
    for M in G.TILE_M:
        a, b = G.operands(grid, M, K, N, G.linear_seed(grid, M, K, N))
        _, b2 = G.operands(grid, M, K, N, G.linear_seed(grid, M, K, N) + 50)
        table, b, b2 = a.to(DEV), b.to(DEV), b2.to(DEV)
        W = filler(N, 3 * K, 41, torch.float32)                      # Linear weight [N out, 3K in]
        W[:, K:2 * K] = b.t()
        W[:, 2 * K:] = b2.t()
        weight = torch.nn.Parameter(W)
        cols = [(K, 2 * K), (2 * K, 3 * K)][:streams]
        refs = [f32_of(G.split3_ref(table, bb, four=False)) for bb in (b, b2)[:streams]]
        if grid == "mid_both":
            assert not torch.equal(refs[0].double(), table.double() @ b.double())
        else:
            assert torch.equal(refs[0].double(), table.double() @ b.double())
        what = f"project_f32_split3 M={M} K={K} N={N} {grid} streams={streams}"
        outs = split3._split3_project(table, weight, cols)
        assert outs is not None and len(outs) == streams
        for i, (o, r) in enumerate(zip(outs, refs)):
            assert_bits(o, r, f"{what} out{i}", where_rows64)
        Wv = [split3._split3_weight(weight, (tuple(c),), False) for c in cols]
        gs = [Guarded(M, N, torch.float32) for _ in cols]
        L.check(L.load().hgnn_project_f32_split3(L.ptr(table), M, K, L.ptr(Wv[0]), L.ptr(Wv[1]) if streams > 1 else None,
                                                 N, gs[0].ptr(), gs[1].ptr() if streams > 1 else None,
                                                 L.current_stream(table.device)), "hgnn_project_f32_split3")
        for i, (g, r) in enumerate(zip(gs, refs)):
            g.all_written(what)
            assert_bits(g.check(what), r, f"{what} out{i} (guarded, second call)", where_rows64)


# ------------------------------------------------------------------ e: trip invariance of the persistent tile loops
def trips_2_and_3(kernel):
    """(M, [(begin, end) of trip 2, of trip 3]) for M = two full trips + 193 rows"""
    T = G.trip_rows(kernel, cus())
    return 2 * T + 193, [(T, 2 * T), (2 * T, 2 * T + 193)]


def where_trip(kernel, first_row):
    def where(row, col):
        trip, wg, tile = G.trip_of_row(kernel, first_row + row, cus())
        return f"row {first_row + row}: tile {tile} = trip {trip + 1} of workgroup {wg}"
    return where


@pytest.mark.parametrize("act", [1, 2], ids=["GELU", "Tanh"])
@pytest.mark.parametrize("K,N", [(256, 128), (256, 256), (256, 512)])
def test_backward_layer_ln_form_rows_do_not_depend_on_the_trip(K, N, act):
    from hierarchicalgnn_amd import fused
    M, ranges = trips_2_and_3("bwd_layer")
    g = torch.Generator(device=DEV).manual_seed(K + N + act)
    dz = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    W = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
    z = (1.5 * torch.randn(M, N, device=DEV, generator=g) + 0.2).bfloat16()
    gamma = 1 + 0.2 * torch.randn(N, device=DEV, generator=g)
    beta = 0.2 * torch.randn(N, device=DEV, generator=g)
    dzp, a_prev, dg, db = fused._bwd_layer(dz, W, z, gamma, beta, act, 1e-5, want_a=True)
    for t, (s, e) in enumerate(ranges):
        sub = fused._bwd_layer(dz[s:e], W, z[s:e], gamma, beta, act, 1e-5, want_a=True)
        what = f"backward layer LN form K={K} N={N} act={act}, trip {t + 2} alone"
        assert_bits(dzp[s:e], sub[0], what + ": dz'", where_trip("bwd_layer", s))
        assert_bits(a_prev[s:e], sub[1], what + ": a'", where_trip("bwd_layer", s))
    # dgamma / dbeta: their summation order changes with the workgroup count -> against float64 at the fp32 bar
    acts = {1: torch.nn.functional.gelu, 2: torch.tanh}
    zf = z.double().requires_grad_(True)
    gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    acts[act](torch.nn.functional.layer_norm(zf, [N], gm, bt, 1e-5)).backward(dz.double() @ W.bfloat16().double())
    for got, want, name in ((dg, gm.grad, "dgamma"), (db, bt.grad, "dbeta")):
        err = float((got.double() - want).abs().max() / want.abs().max())
        assert err <= ln_ref.F32_BAR, (name, err)


def test_backward_layer_input_form_rows_do_not_depend_on_the_trip():
    from hierarchicalgnn_amd import fused
    M, ranges = trips_2_and_3("bwd_layer")
    K, N = 128, 256
    g = torch.Generator(device=DEV).manual_seed(3)
    dz = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    W = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
    skip = torch.randn(M, N, device=DEV, generator=g).bfloat16()
    full = fused._bwd_layer(dz, W, None, None, None, 0, 1e-5, skip=skip)[0]
    for t, (s, e) in enumerate(ranges):
        sub = fused._bwd_layer(dz[s:e], W, None, None, None, 0, 1e-5, skip=skip[s:e])[0]
        assert_bits(full[s:e], sub, f"backward layer input form with skip, trip {t + 2} alone", where_trip("bwd_layer", s))


FORWARD_KERNELS = [("split3_l128", 128, 2, None), ("split3_l128", 128, 3, None),
                   ("split3_l256_rows64", 256, 2, 0), ("split3_l256_rows128", 256, 2, 1)]


@pytest.mark.parametrize("mode", ["inference", "training_forward"])
@pytest.mark.parametrize("kernel,L,layers,rows128", FORWARD_KERNELS,
                         ids=["latent128x2", "latent128x3", "latent256_rows64", "latent256_rows128"])
def test_split3_forward_rows_do_not_depend_on_the_trip(split3, kernel, L, layers, rows128, mode):
    """three segments (a small gathered table: pre-projected in every call; a large one: gathered inside the kernel; direct
    rows) + skip rows.  The 128-row kernel only runs from 65,536 rows on: its separate calls are filled up to that
    many with rows of trip 1 BEHIND the rows under test, so those are computed in trip 1 (and 2) of the same kernel."""
    from hierarchicalgnn_amd import make_mlp
    L_ = _L()
    M, ranges = trips_2_and_3(kernel)
    min_rows = 65536 if rows128 == 1 else 0
    assert M >= min_rows
    torch.manual_seed(L + layers)
    out_act = "Tanh" if layers == 2 else "GELU"
    net = make_mlp(3 * L, 2 * L, L, layers, layer_norm=True, output_activation=out_act, hidden_activation="GELU").to(DEV)
    for p in net.parameters():
        if p.dim() == 1:
            p.data.add_(0.2 * torch.randn_like(p))
    n_small, n_big = 40, M // 4 + 1          # 4 * 40 <= 193: projected in every call; 4 * n_big > M: never
    small_t, big_t = torch.randn(n_small, L, device=DEV), torch.randn(n_big, L, device=DEV)
    i0 = torch.randint(0, n_small, (M,), device=DEV)
    i1 = torch.randint(0, n_big, (M,), device=DEV)
    direct = torch.randn(M, L, device=DEV)

    def run(rows):
        """(out, dumps) on the given rows (None: all)"""
        a, b, d = (i0, i1, direct) if rows is None else (i0[rows], i1[rows], direct[rows])
        segs = [(small_t, a), (big_t, b), (d, None)]
        n0 = split3.stats.get("split3_calls", 0)
        if mode == "inference":
            with torch.no_grad():
                assert split3.supported(net, segs, d)
                out, dumps = split3.fused_concat_mlp(net, segs, d), []
        else:
            assert split3.supported_train(net, segs, d)
            out = split3.fused_concat_mlp_train(net, segs, d)
            dumps = list(out.grad_fn.saved_tensors[-layers:])                # the pre-LayerNorm rows of every layer
            assert all(tuple(z.shape) == (d.shape[0], w) for z, w in zip(dumps, [2 * L] * (layers - 1) + [L]))
            out = out.detach()
        assert split3.stats.get("split3_calls", 0) == n0 + 1                 # the split-bf16 kernel ran
        return out, dumps

    try:
        if rows128 is not None:
            L_.check(L_.load().hgnn_set_option(b"mlp_split3_rows128", rows128), "hgnn_set_option")
        full, full_dumps = run(None)
        for t, (s, e) in enumerate(ranges):
            rows = torch.arange(s, e, device=DEV)
            if e - s < min_rows:
                rows = torch.cat([rows, torch.arange(0, min_rows - (e - s), device=DEV)])
            sub, sub_dumps = run(rows)
            what = f"{kernel} x{layers} {mode}, trip {t + 2} in a call of its own"
            assert_bits(full[s:e], sub[:e - s], what + ": out", where_trip(kernel, s))
            for l, (zf, zs) in enumerate(zip(full_dumps, sub_dumps)):
                assert_bits(zf[s:e], zs[:e - s], what + f": dump of layer {l}", where_trip(kernel, s))
    finally:
        if rows128 is not None:
            L_.check(L_.load().hgnn_set_option(b"mlp_split3_rows128", 1), "hgnn_set_option")
    assert bool(torch.isfinite(full).all())
