"""Exact-arithmetic conformance of the HBM-bound row kernels (K1..K6, fp32 and bf16 rows).

Inputs come from the dyadic grids of tests/rows_ref.py, so every product and every partial sum is exact in fp32 in
any order: each comparison below is ``torch.equal`` against an int64 CPU reference (bf16: the exact sum rounded
once, round-to-nearest-even), at every element.  The exactness bound (list length x 512 units < 2^24, i.e. lists
shorter than 32768 rows) is asserted by the reference on every case.  tests/test_rows_ref.py proves the reference.

Outputs of the C ABI calls live inside a poisoned buffer (NaN-pattern guard rows before and after); the guards
must be intact after each call, which is how a too-wide 16-byte store at a column tail shows up without a fault.
The entry points take contiguous rows only (no row stride), so there is no column-slice form to guard beside.
The fp32 partial buffer is filled with NaN before each reduce: a partial row that is read but was never written
poisons the result.

List lengths: ``rows_ref.standard_lengths`` (0..193 at every loop edge, c-1 .. 3c+1 and 64c+1 for the plan's
chunk c, runs of empty destinations; first and last destination empty / one row / split).

Pruning rule of the fp32 reduce cross product (20 widths x 5 variants x 5 chunks x 2 nt_loads x 3 end placements):
  A  every width x every variant at the default chunk, nt_loads=1
  B  every width x every explicit chunk (1, 5, 64, 100), nt_loads=1, variant rotating with (width + chunk)
  C  every width x every variant at chunk 5, nt_loads=0
the end placement rotates with (width + variant + chunk).  bf16: every width x every variant at the default chunk
and x every explicit chunk with rotating variant.

Kernel instantiation -> test id that reaches it (widths F; fp32 nvec = F/4, bf16 ncol = F/8):

  dispatch_seg (segreduce.hip), main pass; W = weight, RS = row_scale; TAG 2 = sorted index; NT = nt_loads
    k_seg_reduce_scalar<W,RS>          F%4 or F>1024   test_f32_reduce_exact[F{1,3,6,1028,1100}-*]
    k_seg_reduce<4,1,4,..>             nvec<=4         test_f32_reduce_exact[F{4,16}-*]
    k_seg_reduce<8,1,4,..>             nvec<=8         test_f32_reduce_exact[F{20,32}-*]
    k_seg_reduce<16,1,4,..>            nvec<=16        test_f32_reduce_exact[F{36,64}-*]
    k_seg_reduce<32,1,4,..>            nvec<=32        test_f32_reduce_exact[F{68,128}-*]
    k_seg_reduce<64,1,16,0,0,..,16>    nvec<=64 plain  test_f32_reduce_exact[F{132,252,256}-{plain,sorted}-*],
                                       (headline)      test_headline_all_rows[*]
    k_seg_reduce<64,1,8,W,RS,..>       nvec<=64 W      test_f32_reduce_exact[F{132,252,256}-{weight,gss,sorted_weight}-*]
    k_seg_reduce<64,2,4,..>            nvec<=128       test_f32_reduce_exact[F{260,512}-*]
    k_seg_reduce<64,4,2,..>            nvec<=256       test_f32_reduce_exact[F{516,1024}-*]
      <..,W=0,RS=0,TAG 0>  *-plain-*      <..,W=1,RS=0,TAG 0>  *-weight-*, *-sorted_weight-*
      <..,W=1,RS=1,TAG 0>  *-gss-*        <..,W=0,RS=0,TAG 2>  *-sorted-*
      <..,NT=true>  *-nt1                 <..,NT=false>  *-nt0
    combine pass <..,W=0,RS=0,TAG 1> of the same width: every case (all have split lists, one with > 64 partials)
    row_scale without weight: refused           test_unsupported_forms_raise
  launch_seg_bf16 (segreduce_bf16.hip), main pass <RL,U,W,RS,false,WPB> + combine <RL,4,0,0,true,4>
    <4,4,..,4>  ncol<=4   test_bf16_reduce_exact[F{8,32}-*]       <8,4,..,4>   ncol<=8   ..[F{40,64}-*]
    <16,4,..,4> ncol<=16  ..[F{72,128}-*]                         <32,4,..,8>  ncol<=32  ..[F{136,256}-*]
    <64,16,..,16> ncol<=64 ..[F{264,504,512}-*], test_headline_bf16_all_rows
    F % 8 != 0 or F > 512: refused              test_unsupported_forms_raise
  dispatch_spread<W> / k_spread_rows<RL,VPL,W,WPB>, k_spread_rows_scalar<W>: same width classes
                                                test_f32_spread_exact[F*] (plain and weighted, chunks default/1/100),
                                                test_f32_backward_exact[F*] (through autograd)
    hgnn_spread_rows_bf16 k_spread_rows_bf16<RL,W,8>   test_bf16_spread_gather_exact[F*]
  dispatch_gather<W,RS> / k_gather_rows<RL,VPL,U,W,RS>, k_gather_rows_scalar<W,RS>
                                                test_f32_gather_exact[F*] (all four W/RS forms, padding indices)
    hgnn_gather_rows_bf16 k_gather_rows_bf16<RL,W>     test_bf16_spread_gather_exact[F*]
  hgnn_edge_dot_f32 / k_edge_dot<RL,VPL>, k_edge_dot_scalar
                                                test_f32_edge_dot_exact[F*] (gathered / identity operands),
                                                test_f32_backward_exact[F*] (d/dweight)
  grid-stride second trip of the streaming kernels   test_streaming_kernels_second_grid_trip
"""
import contextlib
import ctypes

import pytest
import torch

import rows_ref as R

pytestmark = pytest.mark.gpu

F32_VECTOR = (4, 16, 20, 32, 36, 64, 68, 128, 132, 256, 252, 260, 512, 516, 1024)
F32_SCALAR = (1, 3, 6, 1028, 1100)
F32_WIDTHS = F32_VECTOR + F32_SCALAR
BF16_WIDTHS = (8, 32, 40, 64, 72, 128, 136, 256, 264, 504, 512)
VARIANTS = ("plain", "weight", "gss", "sorted", "sorted_weight")
BF16_VARIANTS = ("plain", "weight", "gss")
CHUNKS = (1, 5, 64, 100)             # explicit GraphPlan(chunk=); 0 = the default (32 at these sizes)
STREAM_M = (0, 1, 63, 64, 65, 1024)  # rows of the streaming kernels: tile edges and a multiple of the 256-row block
POISON32 = 0x7FC0BEEF                # a quiet-NaN pattern
POISON16 = 0x7FC1


def _f32_cases():
    cases = []
    for wi, F in enumerate(F32_WIDTHS):
        for vi, v in enumerate(VARIANTS):                                   # A
            cases.append((F, v, 0, R.ENDS[(wi + vi) % 3], 1))
        for ci, c in enumerate(CHUNKS):                                     # B
            cases.append((F, VARIANTS[(wi + ci) % 5], c, R.ENDS[(wi + ci + 1) % 3], 1))
        for vi, v in enumerate(VARIANTS):                                   # C
            cases.append((F, v, 5, R.ENDS[(wi + vi + 2) % 3], 0))
    return cases


def _bf16_cases():
    cases = []
    for wi, F in enumerate(BF16_WIDTHS):
        for vi, v in enumerate(BF16_VARIANTS):
            cases.append((F, v, 0, R.ENDS[(wi + vi) % 3], 1))
        for ci, c in enumerate(CHUNKS):
            cases.append((F, BF16_VARIANTS[(wi + ci) % 3], c, R.ENDS[(wi + ci + 1) % 3], 1))
    return cases


def _case_id(c):
    F, v, chunk, ends, nt = c
    return f"F{F}-{v}-c{chunk or 'default'}-{ends}-nt{nt}"


# ------------------------------------------------------------------ library access
@pytest.fixture(scope="module", autouse=True)
def lib():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from hierarchicalgnn_amd import _lib
    import hierarchicalgnn_amd as H
    yield _lib.load()
    _GRAPHS.clear()
    _PLANS.clear()
    H.clear_plan_cache()


def _L():
    from hierarchicalgnn_amd import _lib
    return _lib


@contextlib.contextmanager
def nt_loads(value):
    L = _L()
    try:
        L.check(L.load().hgnn_set_option(b"nt_loads", int(value)), "hgnn_set_option")
        yield
    finally:
        L.check(L.load().hgnn_set_option(b"nt_loads", 1), "hgnn_set_option")


class Guarded:
    """``rows`` x ``F`` output rows inside a poisoned buffer with at least 64 guard elements on either side"""

    def __init__(self, rows, F, dtype):
        self.pad = F * -(-64 // F)
        n = rows * F
        self.buf = torch.empty(2 * self.pad + n, dtype=dtype, device="cuda")
        self.bits = self.buf.view(torch.int32 if dtype == torch.float32 else torch.int16)
        self.poison = POISON32 if dtype == torch.float32 else POISON16
        self.bits.fill_(self.poison)
        self.out = self.buf[self.pad:self.pad + n].view(rows, F)
        assert dtype == torch.float32 and F % 4 or self.out.data_ptr() % 16 == 0

    def ptr(self):
        return ctypes.c_void_p(self.out.data_ptr())

    def check(self, what):
        lo, hi = self.bits[:self.pad], self.bits[self.bits.numel() - self.pad:]
        assert bool((lo == self.poison).all()), f"{what}: wrote BEFORE the first output row"
        assert bool((hi == self.poison).all()), f"{what}: wrote PAST the last output row"
        return self.out

    def all_written(self, what):
        n = int((self.bits[self.pad:self.bits.numel() - self.pad] == self.poison).sum())
        assert n == 0, f"{what}: {n} output elements never written"


def seg_reduce(plan, src, weight=None, row_scale=None):
    """hgnn_segment_reduce_{f32,bf16} into a guarded buffer, with a NaN-filled partial buffer"""
    L = _L()
    F = int(src.shape[1])
    bf16 = src.dtype == torch.bfloat16
    g = Guarded(plan.N, F, src.dtype)
    partial = plan.partial(F)
    partial.fill_(float("nan"))
    fn = L.load().hgnn_segment_reduce_bf16 if bf16 else L.load().hgnn_segment_reduce_f32
    L.check(fn(ctypes.byref(plan.c), L.ptr(src), F, L.ptr(weight), L.ptr(row_scale), g.ptr(), L.ptr(partial),
               L.current_stream(src.device)), "hgnn_segment_reduce")
    g.all_written("segment_reduce")
    return g.check("segment_reduce")


def spread_rows(plan, table, weight=None):
    L = _L()
    F = int(table.shape[1])
    g = Guarded(plan.M, F, table.dtype)
    fn = L.load().hgnn_spread_rows_bf16 if table.dtype == torch.bfloat16 else L.load().hgnn_spread_rows_f32
    L.check(fn(ctypes.byref(plan.c), L.ptr(table), F, L.ptr(weight), g.ptr(), L.current_stream(table.device)),
            "hgnn_spread_rows")
    g.all_written("spread_rows")
    return g.check("spread_rows")


def gather_rows(table, idx32, weight=None, row_scale=None):
    L = _L()
    F, M = int(table.shape[1]), int(idx32.numel())
    g = Guarded(M, F, table.dtype)
    if table.dtype == torch.bfloat16:
        assert row_scale is None
        rc = L.load().hgnn_gather_rows_bf16(L.ptr(table), int(table.shape[0]), F, L.ptr(idx32), M, L.ptr(weight),
                                            g.ptr(), L.current_stream(table.device))
    else:
        rc = L.load().hgnn_gather_rows_f32(L.ptr(table), int(table.shape[0]), F, L.ptr(idx32), M, L.ptr(weight),
                                           L.ptr(row_scale), g.ptr(), L.current_stream(table.device))
    L.check(rc, "hgnn_gather_rows")
    g.all_written("gather_rows")
    return g.check("gather_rows")


def edge_dot(A, ai32, B, bi32, M):
    L = _L()
    g = Guarded(M, 1, torch.float32)
    L.check(L.load().hgnn_edge_dot_f32(L.ptr(A), L.ptr(ai32), int(A.shape[0]), L.ptr(B), L.ptr(bi32),
                                       int(B.shape[0]), int(A.shape[1]), M, g.ptr(), L.current_stream(A.device)),
            "hgnn_edge_dot_f32")
    g.all_written("edge_dot")
    return g.check("edge_dot").view(-1)


def assert_same(out, ref, what, lengths=None):
    """bitwise equality at every element; on failure name the first wrong element (and its list length)"""
    out = out.detach().cpu()
    assert out.shape == ref.shape and out.dtype == ref.dtype, (what, out.shape, ref.shape, out.dtype, ref.dtype)
    if torch.equal(out, ref):
        return
    bad = torch.nonzero(out != ref)
    r = int(bad[0][0])
    c = int(bad[0][1]) if out.dim() > 1 else None
    got, want = (out[r, c], ref[r, c]) if c is not None else (out[r], ref[r])
    ln = f", list of {lengths[r]} rows" if lengths is not None else ""
    raise AssertionError(f"{what}: {bad.shape[0]} of {out.numel()} elements differ; first at row {r}{ln}, "
                         f"column {c}: got {float(got)}, want {float(want)}")


# ------------------------------------------------------------------ graphs and plans, shared across widths
_GRAPHS = {}
_PLANS = {}


class Graph:
    def __init__(self, ends, chunk):
        c = chunk or 32
        self.lengths = R.standard_lengths(c, ends, seed=17 * c + R.ENDS.index(ends))
        self.shuf, self.srt = R.index_with_lengths(self.lengths, seed=c + 5)
        self.M, self.N = int(self.shuf.numel()), len(self.lengths)
        assert chunk or R.default_chunk(self.M) == 32
        self.n_src = 301
        self.gather = torch.randint(0, self.n_src, (self.M,), generator=torch.Generator().manual_seed(c + 9))
        self.dev = {k: getattr(self, k).cuda() for k in ("shuf", "srt", "gather")}


def graph(ends, chunk):
    key = (ends, chunk)
    if key not in _GRAPHS:
        _GRAPHS[key] = Graph(ends, chunk)
    return _GRAPHS[key]


def plan_for(ends, chunk, kind):
    """kind: 'shuf' (scatter on the shuffled index), 'srt' (sorted index), 'gss' (shuffled destination + gather)"""
    import hierarchicalgnn_amd as H
    key = (ends, chunk, kind)
    if key not in _PLANS:
        g = graph(ends, chunk)
        if kind == "gss":
            p = H.GraphPlan(g.dev["shuf"], g.N, g.dev["gather"], g.n_src, chunk=chunk)
        else:
            p = H.GraphPlan(g.dev[kind], g.N, chunk=chunk)
        assert p.chunk == (chunk or 32)
        assert p.sorted == (kind == "srt"), "a destination-sorted index must be reported as plan.sorted (TAG 2 path)"
        _PLANS[key] = p
    return _PLANS[key]


def run_reduce_case(dtype, F, variant, chunk, ends, nt):
    g = graph(ends, chunk)
    seed = 1000 * F + 10 * chunk + VARIANTS.index(variant)
    w = rs = gat = None
    kind = "srt" if variant.startswith("sorted") else ("gss" if variant == "gss" else "shuf")
    index = g.srt if kind == "srt" else g.shuf
    if variant in ("weight", "sorted_weight", "gss"):
        w = R.weights(g.M, seed + 1)
    if variant == "gss":
        src, rs, gat = R.features(g.n_src, F, seed, dtype), R.row_scales(g.n_src, seed + 2), g.gather
    else:
        src = R.features(g.M, F, seed, dtype)
    ref = R.scatter_ref(src, index, g.N, weight=w, gather=gat, row_scale=rs)
    plan = plan_for(ends, chunk, kind)
    dev = [None if t is None else t.cuda() for t in (src, w, rs)]
    with nt_loads(nt):
        out = seg_reduce(plan, *dev)
    assert_same(out, ref, _case_id((F, variant, chunk, ends, nt)), g.lengths)


# ------------------------------------------------------------------ the plan on the standard indices
@pytest.mark.parametrize("chunk", (0,) + CHUNKS)
@pytest.mark.parametrize("ends", R.ENDS)
@pytest.mark.parametrize("kind", ("shuf", "srt"))
def test_plan_on_standard_lengths(ends, chunk, kind):
    g = graph(ends, chunk)
    plan = plan_for(ends, chunk, kind)
    want = R.plan_reference(g.lengths, plan.chunk)
    c = plan.counts_host()
    assert (c["work"], c["split"], c["partial"], c["valid"], c["err"]) == \
        (want["work"], want["split"], want["partial"], g.M, 0)
    assert c["work"] <= plan.c.max_work and c["split"] <= plan.c.max_split and c["partial"] <= plan.c.max_partial
    index = g.srt if kind == "srt" else g.shuf
    assert torch.equal(plan.perm[:g.M].cpu().long(), torch.sort(index, stable=True).indices)
    assert plan.rowptr[:g.N + 1].cpu().tolist() == want["rowptr"]
    for name in ("wi_begin", "wi_end", "wi_dst", "wi_target"):
        assert getattr(plan, name)[:c["work"]].cpu().tolist() == want[name], name
    assert plan.split_dst[:c["split"]].cpu().tolist() == want["split_dst"]
    assert plan.split_pbegin[:c["split"] + 1].cpu().tolist() == want["split_pbegin"]
    n_part = torch.tensor(want["split_pbegin"]).diff()
    assert int(n_part.max()) > 64, "no destination with more than 64 partial rows"


# ------------------------------------------------------------------ fp32 segmented reduce, every instantiation
@pytest.mark.parametrize("case", _f32_cases(), ids=_case_id)
def test_f32_reduce_exact(case):
    run_reduce_case(torch.float32, *case)


@pytest.mark.parametrize("case", _bf16_cases(), ids=_case_id)
def test_bf16_reduce_exact(case):
    """fp32 accumulation, fp32 partials, ONE rounding (to nearest even) in the main or the combine pass: 100 % of
    the elements equal the rounded exact sum"""
    run_reduce_case(torch.bfloat16, *case)


def test_every_branch_meets_every_variant_and_chunk():
    """the pruning rule keeps every (width x variant) and every (width x chunk) pair, and both nt_loads settings"""
    for cases, widths, variants in ((_f32_cases(), F32_WIDTHS, VARIANTS), (_bf16_cases(), BF16_WIDTHS, BF16_VARIANTS)):
        have_v = {(F, v) for F, v, *_ in cases}
        have_c = {(F, c) for F, _, c, *_ in cases}
        assert have_v == {(F, v) for F in widths for v in variants}
        assert have_c == {(F, c) for F in widths for c in (0,) + CHUNKS}
    assert {(F, v) for F, v, _, _, nt in _f32_cases() if nt == 0} == {(F, v) for F in F32_WIDTHS for v in VARIANTS}


# ------------------------------------------------------------------ spread / gather / edge dot through the C ABI
@pytest.mark.parametrize("F", F32_WIDTHS)
def test_f32_spread_exact(F):
    for i, chunk in enumerate((0, 1, 100)):
        ends = R.ENDS[(F + i) % 3]
        g, plan = graph(ends, chunk), plan_for(ends, chunk, "shuf")
        table, w = R.features(g.N, F, F + i), R.weights(g.M, F + i + 1)
        assert_same(spread_rows(plan, table.cuda()), R.spread_ref(table, g.shuf), f"spread F{F} c{chunk}")
        assert_same(spread_rows(plan, table.cuda(), w.cuda()), R.spread_ref(table, g.shuf, w),
                    f"spread weighted F{F} c{chunk}")


def _padded_index(M, rows, seed):
    idx = torch.randint(0, rows, (M,), generator=torch.Generator().manual_seed(seed))
    idx[::5] = -1                                            # padding entries: zero rows
    if M:
        idx[M - 1] = rows - 1
    return idx


@pytest.mark.parametrize("F", F32_WIDTHS)
def test_f32_gather_exact(F):
    rows = 97
    table, rs = R.features(rows, F, F), R.row_scales(rows, F + 1)
    td, rsd = table.cuda(), rs.cuda()
    for M in STREAM_M + (1500,):
        idx, w = _padded_index(M, rows, F + M), R.weights(M, F + M + 1)
        i32, wd = idx.int().cuda(), w.cuda()
        for use_w, use_rs in ((0, 0), (1, 0), (0, 1), (1, 1)):
            out = gather_rows(td, i32, wd if use_w else None, rsd if use_rs else None)
            ref = R.gather_ref(table, idx, w if use_w else None, rs if use_rs else None)
            assert_same(out, ref, f"gather F{F} M{M} weight={use_w} row_scale={use_rs}")
            assert M < 2 or float(out[0].abs().sum()) == 0.0     # idx[0] is a padding entry


@pytest.mark.parametrize("F", F32_WIDTHS)
def test_f32_edge_dot_exact(F):
    for M in STREAM_M + (1500,):
        rows = max(M, 1) + 3
        A, B = R.features(rows, F, F + M), R.features(rows, F, F + M + 1)
        ai, bi = _padded_index(M, rows, F + M + 2), _padded_index(M, rows, F + M + 3)
        bi = bi.roll(2)
        Ad, Bd = A.cuda(), B.cuda()
        for ua, ub in ((1, 1), (0, 1), (1, 0), (0, 0)):
            out = edge_dot(Ad, ai.int().cuda() if ua else None, Bd, bi.int().cuda() if ub else None, M)
            ref = R.edge_dot_ref(A[:M] if not ua else A, ai if ua else None, B[:M] if not ub else B, bi if ub else None)
            assert_same(out, ref[:M], f"edge_dot F{F} M{M} gathered A={ua} B={ub}")


@pytest.mark.parametrize("F", BF16_WIDTHS)
def test_bf16_spread_gather_exact(F):
    for i, chunk in enumerate((0, 1)):
        ends = R.ENDS[(F + i) % 3]
        g, plan = graph(ends, chunk), plan_for(ends, chunk, "shuf")
        table, w = R.features(g.N, F, F + i, torch.bfloat16), R.weights(g.M, F + i + 1)
        assert_same(spread_rows(plan, table.cuda()), R.spread_ref(table, g.shuf), f"bf16 spread F{F} c{chunk}")
        assert_same(spread_rows(plan, table.cuda(), w.cuda()), R.spread_ref(table, g.shuf, w),
                    f"bf16 spread weighted F{F} c{chunk}")
    rows = 97
    table = R.features(rows, F, F, torch.bfloat16)
    for M in STREAM_M + (1500,):
        idx, w = _padded_index(M, rows, F + M), R.weights(M, F + M + 1)
        for use_w in (0, 1):
            out = gather_rows(table.cuda(), idx.int().cuda(), w.cuda() if use_w else None)
            assert_same(out, R.gather_ref(table, idx, w if use_w else None), f"bf16 gather F{F} M{M} weight={use_w}")


def test_streaming_kernels_second_grid_trip():
    """gather / edge dot launch at most 8192 blocks of 4 waves: more than 8192 * 256 rows (vector kernels, 64 rows
    per wave) or 8192 * 4 rows (scalar kernels, one row per wave) take the grid-stride loop round again"""
    for F, M in ((4, 8192 * 256 + 65), (3, 8192 * 4 + 65)):
        rows = 1000
        table, B = R.features(rows, F, 1), R.features(M, F, 2)
        idx, w = _padded_index(M, rows, 3), R.weights(M, 4)
        i32 = idx.int().cuda()
        assert_same(gather_rows(table.cuda(), i32, w.cuda()), R.gather_ref(table, idx, w), f"gather F{F} M{M}")
        assert_same(edge_dot(table.cuda(), i32, B.cuda(), None, M), R.edge_dot_ref(table, idx, B, None),
                    f"edge_dot F{F} M{M}")
    F, M = 8, 8192 * 256 + 65
    table = R.features(1000, F, 5, torch.bfloat16)
    idx = _padded_index(M, 1000, 6)
    assert_same(gather_rows(table.cuda(), idx.int().cuda()), R.gather_ref(table, idx), f"bf16 gather F{F} M{M}")


# ------------------------------------------------------------------ backward kernels through autograd
@pytest.mark.parametrize("F", F32_WIDTHS)
def test_f32_backward_exact(F):
    """gradients of scatter_add (k_spread_rows, k_edge_dot with an identity operand) and of gather_scale_scatter
    (the reduce on the transposed plan, k_edge_dot with two gathered operands) on grid-valued upstream gradients"""
    import hierarchicalgnn_amd as H
    ends = R.ENDS[F % 3]
    g, plan = graph(ends, 0), plan_for(ends, 0, "shuf")
    src, w, gout = R.features(g.M, F, F), R.weights(g.M, F + 1), R.features(g.N, F, F + 2)
    idx_d = g.dev["shuf"]
    # scatter_add, plain: the gradient is a gather
    s = src.cuda().requires_grad_(True)
    H.scatter_add(s, idx_d, dim=0, dim_size=g.N, plan=plan).backward(gout.cuda())
    assert_same(s.grad, gout[g.shuf], f"d scatter_add / d src, F{F}")
    # scatter_add, weighted
    s, wd = src.cuda().requires_grad_(True), w.view(-1, 1).cuda().requires_grad_(True)
    out = H.scatter_add(s, idx_d, dim=0, dim_size=g.N, plan=plan, weight=wd)
    assert_same(out, R.scatter_ref(src, g.shuf, g.N, weight=w), f"weighted scatter_add, F{F}", g.lengths)
    out.backward(gout.cuda())
    assert_same(s.grad, R.spread_ref(gout, g.shuf, w), f"d weighted scatter_add / d src, F{F}")
    assert_same(wd.grad, R.edge_dot_ref(src, None, gout, g.shuf).view(-1, 1), f"d weighted scatter_add / d weight, F{F}")
    # gather_scale_scatter with row_scale: short gather lists keep the eager row sum of grad_rs exact
    gl = R.lengths_filling(g.M)
    gi, _ = R.index_with_lengths(gl, seed=F + 3)
    n_src = len(gl)
    X, rs = R.features(n_src, F, F + 4), R.row_scales(n_src, F + 5)
    Xd, wd, rsd = (t.cuda().requires_grad_(True) for t in (X, w, rs))
    out = H.gather_scale_scatter(Xd, gi.cuda(), idx_d, g.N, wd, row_scale=rsd)
    assert_same(out, R.scatter_ref(X, g.shuf, g.N, weight=w, gather=gi, row_scale=rs), f"gss, F{F}", g.lengths)
    out.backward(gout.cuda())
    T = R.scatter_ref(gout, gi, n_src, weight=w, gather=g.shuf).double()     # sum_b w[b] * gout[dst[b]] per source row
    assert float((T.abs() * X.double().abs()).sum(1).max()) * 2 < R.EXACT_LIMIT     # units of 1/2
    assert_same(Xd.grad, (T * rs.double().view(-1, 1)).float(), f"d gss / d X, F{F}", gl)
    assert_same(rsd.grad, (T * X.double()).sum(1).float(), f"d gss / d row_scale, F{F}", gl)
    assert_same(wd.grad, (R.edge_dot_ref(gout, g.shuf, X, gi).double() * rs.double()[gi]).float(),
                f"d gss / d weight, F{F}")


def test_edge_dot_operator_both_index_forms():
    """ops.edge_dot (two gathered operands) and its gradients (weighted gathered reduces)"""
    from hierarchicalgnn_amd import ops
    F, rows = 68, 211
    gl = R.lengths_filling(1500)
    ai, _ = R.index_with_lengths(gl, seed=1)
    bi = torch.randint(0, rows, (ai.numel(),), generator=torch.Generator().manual_seed(2))
    A, B, gout = R.features(len(gl), F, 3), R.features(rows, F, 4), R.weights(ai.numel(), 5)
    Ad, Bd = A.cuda().requires_grad_(True), B.cuda().requires_grad_(True)
    out = ops.edge_dot(Ad, ai.cuda(), Bd, bi.cuda())
    assert_same(out, R.edge_dot_ref(A, ai, B, bi), "edge_dot")
    out.backward(gout.cuda())
    assert_same(Ad.grad, R.scatter_ref(B, ai, len(gl), weight=gout, gather=bi), "d edge_dot / d A", gl)
    assert_same(Bd.grad, R.scatter_ref(A, bi, rows, weight=gout, gather=ai), "d edge_dot / d B")


def test_spread_on_an_unvalidated_plan_zeroes_the_rows_it_skips():
    """a plan built with validate=False keeps out-of-range rows out of every list: the reduce ignores them and the
    spread must leave their output rows ZERO (ops._spread_rows allocates zeros, not empty, for such a plan)"""
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd.ops import _seg_reduce, _spread_rows
    F = 36
    g = graph("one", 5)
    index = g.shuf.clone()
    index[::11] = g.N + 3
    index[5::13] = -1
    ok = (index >= 0) & (index < g.N)
    plan = H.GraphPlan(index.cuda(), g.N, chunk=5, validate=False)
    assert not plan.validated and plan.counts_host()["err"] == 1 and plan.counts_host()["valid"] == int(ok.sum())
    src, table = R.features(g.M, F, 1), R.features(g.N, F, 2)
    assert_same(_seg_reduce(plan, src.cuda(), None, None), R.scatter_ref(src[ok], index[ok], g.N), "reduce")
    for _ in range(2):                                       # the second call lands on recycled, dirty memory
        out = _spread_rows(plan, table.cuda())
        assert_same(out, R.spread_ref(table, torch.where(ok, index, torch.full_like(index, -1))), "spread")
        out.fill_(float("nan"))
        del out


def test_unsupported_forms_raise():
    """widths / forms the kernels do not implement are errors, not fallbacks"""
    import hierarchicalgnn_amd as H
    g, plan = graph("one", 5), plan_for("one", 5, "shuf")
    for F in (12, 520):
        with pytest.raises(RuntimeError, match="multiple of 8"):
            H.scatter_add(R.features(g.M, F, 1, torch.bfloat16).cuda(), g.dev["shuf"], dim_size=g.N, plan=plan)
        with pytest.raises(RuntimeError, match="multiple of 8"):
            spread_rows(plan, R.features(g.N, F, 1, torch.bfloat16).cuda())
        with pytest.raises(RuntimeError, match="multiple of 8"):
            gather_rows(R.features(g.N, F, 1, torch.bfloat16).cuda(), g.dev["shuf"].int())
    for dtype in (torch.float32, torch.bfloat16):
        with pytest.raises(RuntimeError, match="row_scale requires weight"):
            seg_reduce(plan_for("one", 5, "gss"), R.features(g.n_src, 64, 1, dtype).cuda(), None,
                       R.row_scales(g.n_src, 2).cuda())


# ------------------------------------------------------------------ repeatability
_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
_ALL_WIDTHS = [("f32", F) for F in F32_WIDTHS] + [("bf16", F) for F in BF16_WIDTHS]


@pytest.mark.parametrize("kind,F", _ALL_WIDTHS)
def test_chunking_does_not_change_grid_results(kind, F):
    """the same grid data through plans with different chunk: bitwise the same output (and the reference)"""
    import hierarchicalgnn_amd as H
    dtype = _DTYPES[kind]
    g = graph("split", 100)
    src, w = R.features(g.M, F, F, dtype), R.weights(g.M, F + 1)
    ref = R.scatter_ref(src, g.shuf, g.N, weight=w)
    sd, wd = src.cuda(), w.cuda()
    for chunk in (0, 1, 5, 64, 100):
        key = ("split", 100, f"rechunk{chunk}")
        if key not in _PLANS:
            _PLANS[key] = H.GraphPlan(g.dev["shuf"], g.N, chunk=chunk)
        assert_same(seg_reduce(_PLANS[key], sd, wd), ref, f"F{F} chunk {chunk}", g.lengths)


@pytest.mark.parametrize("kind,F", _ALL_WIDTHS)
def test_same_plan_twice_is_bitwise_repeatable_on_random_data(kind, F):
    """determinism on data that is NOT exactly summable: one case per dispatch branch, plain and weighted"""
    dtype = _DTYPES[kind]
    g, plan = graph("split", 5), plan_for("split", 5, "shuf")
    gen = torch.Generator().manual_seed(F)
    src = torch.randn(g.M, F, generator=gen).to(dtype).cuda()
    w = (torch.rand(g.M, generator=gen) + 0.1).cuda()
    for weight in (None, w):
        a = seg_reduce(plan, src, weight).clone()
        b = seg_reduce(plan, src, weight)
        assert torch.equal(a.view(torch.int32 if dtype == torch.float32 else torch.int16),
                           b.view(torch.int32 if dtype == torch.float32 else torch.int16))
        assert bool(torch.isfinite(a.float()).all())


# ------------------------------------------------------------------ headline shape, every row
def _device_features(rows, F, seed, dtype=torch.float32):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    mag = torch.randint(1, R.FEATURE_MAX + 1, (rows, F), device="cuda", generator=gen, dtype=torch.int8)
    sign = torch.randint(0, 2, (rows, F), device="cuda", generator=gen, dtype=torch.int8) * 2 - 1
    return (mag * sign).to(dtype)


def _device_reference(src, index, N):
    """fp32 index_add_ on the device: exact on grid data in any order (tests/test_rows_ref.py), no host copy"""
    longest = int(torch.bincount(index, minlength=N).max())
    R.assert_exact(longest)
    return torch.zeros((N, src.shape[1]), dtype=torch.float32, device=src.device).index_add_(0, index, src.float()), longest


@pytest.fixture(scope="module")
def big():
    from hierarchicalgnn_amd import synth
    x, ei = synth.trackml_event(120_000, 1_000_000, seed=1234)
    return synth.directed(ei)[1].cuda().contiguous()


@pytest.mark.parametrize("layout,nt", [("given", 1), ("given", 0), ("sorted", 1), ("sorted", 0)])
def test_headline_all_rows(big, layout, nt):
    """N=120,000, M=2,000,000, F=256: all 120,000 x 256 elements against the exact device-side reference"""
    import hierarchicalgnn_amd as H
    N, F = 120_000, 256
    idx = big if layout == "given" else torch.sort(big).values
    assert idx.numel() == 2_000_000
    src = _device_features(idx.numel(), F, 77)
    ref, _ = _device_reference(src, idx, N)
    plan = H.get_plan(idx, N)
    assert plan.sorted == (layout == "sorted")
    with nt_loads(nt):
        out = H.scatter_add(src, idx, dim=0, dim_size=N, plan=plan)
    assert torch.equal(out, ref), f"{int((out != ref).sum())} of {ref.numel()} elements differ"


def test_headline_bf16_all_rows(big):
    """bf16 rows at F=512 (a 1-KiB row again): the rounded exact sum at every element, plain and weighted (plain
    sums of ~17 rows stay below 256 and need no rounding; weighted ones reach past it and hit ties)"""
    import hierarchicalgnn_amd as H
    N, F = 120_000, 512
    src = _device_features(big.numel(), F, 78, torch.bfloat16)
    w = torch.tensor(R.WEIGHTS, device="cuda")[torch.randint(0, 4, (big.numel(),), device="cuda",
                                                             generator=torch.Generator(device="cuda").manual_seed(82))]
    for weight in (None, w):
        terms = src.float() if weight is None else src.float() * weight.view(-1, 1)
        ref, _ = _device_reference(terms, big, N)
        del terms
        out = H.scatter_add(src, big, dim=0, dim_size=N, weight=weight)
        assert out.dtype == torch.bfloat16
        ref16 = ref.bfloat16()
        assert weight is None or int((ref16.float() != ref).sum()) > 0       # the rounding is exercised
        assert torch.equal(out, ref16), f"{int((out != ref16).sum())} of {ref.numel()} elements differ"


def test_pooling_skew_all_rows():
    """K3 at the BASELINE HGNN shape: B=600k -> S=10k, heavy fan-in skew (longest list ~12k rows < 32768)"""
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import synth
    bg, _ = synth.bipartite_assignment(120_000, 10_000, 5)
    bg = bg.cuda()
    B, F = bg.shape[1], 64
    X = _device_features(120_000, F, 79)
    w = torch.tensor(R.WEIGHTS, device="cuda")[torch.randint(0, 4, (B,), device="cuda",
                                                             generator=torch.Generator(device="cuda").manual_seed(80))]
    rs = torch.tensor(R.ROW_SCALES, device="cuda")[torch.randint(0, 4, (120_000,), device="cuda",
                                                                 generator=torch.Generator(device="cuda").manual_seed(81))]
    gi, di = bg[0].contiguous(), bg[1].contiguous()
    for row_scale in (None, rs):
        terms = w.view(-1, 1) * (X if row_scale is None else X * row_scale.view(-1, 1))[gi]
        ref, longest = _device_reference(terms, di, 10_000)
        assert 64 < longest < R.MAX_LIST
        out = H.gather_scale_scatter(X, gi, di, 10_000, w, row_scale=row_scale)
        assert torch.equal(out, ref), f"{int((out != ref).sum())} of {ref.numel()} elements differ"
