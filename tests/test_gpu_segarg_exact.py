"""Exact conformance of csrc/segminmax.hip through the C ABI: hgnn_segment_reduce_ex (scatter_min / scatter_max with
arg, wrapping integer sums) and hgnn_segment_arg_backward, at every kernel instantiation and every list-length edge.

Min, max, arg and a wrapping integer sum involve no rounding: every comparison is ``torch.equal`` on the bits of
``out`` and on ``arg`` against tests/segarg_ref.py (proven on the CPU by tests/test_segarg_ref.py, which also checks
that every case below holds its planted conditions: ties away from the first row, all-NaN lists and chunks, +-0.0
ties both ways, denormal winners, ties and winners across the chunks of a split list, integers 1 apart at 2^24 /
2^53, overflowing sums, winners beyond row 64).

``out``, ``arg``, ``partial`` and ``partial_arg`` live inside poisoned buffers with 64 guard elements on either side
(``GuardedBuf``; int32 / int64 too).  After each call the guards must be intact -- a 16-byte ``st4`` or the 32-byte
``st4_arg`` past a column tail or the last row shows there without a fault -- and every ``out`` / ``arg`` element must
be written.  Each case runs with ``partial_arg`` pre-filled with 0 (a valid position) and with 0x7FC0BEEF, twice
each (the second call onto the dirty buffers of the first): the four results must be the reference's bits.  For a SUM
the ``arg`` / ``partial_arg`` buffers are handed over all the same and must stay untouched.

Indices: those of tests/test_gpu_rows_exact.py (``Graph`` / ``plan_for``): list lengths 0..193 at every loop edge
(the inner step G*U of k_seg_arg is 64, 32, 16, 8, 16 (8 for int64), 4, 2 rows; the outer step 64), the chunk edges
c-1 .. 3c+1, 64c+1 (more than 64 partial rows), runs of empty destinations, first / last destination empty / one row
/ split.

Pruning rule of the cross product (20 widths x 10 (dtype, op) pairs x 5 chunks x 2 index kinds x 3 end placements):
  A  every width x every pair at the default chunk; the index kind (shuffled / sorted) and the end placement rotate
     with (width + pair)
  B  every width x every explicit chunk (1, 5, 64, 100; F >= 516: 1 and 5 only), the pair rotating with
     (width + chunk)
  C  every pair at chunk 100 at F in {3, 16, 32, 64, 128, 252, 260, 516} (the narrow kernel and one width of each
     row shape): only a chunk above 64 hands a wave more than 64 rows, the second trip of the kernels' outer loop.
     Rule B stops at chunk 5 for F >= 516, so the widest row shape (RL 64, VPL 4) meets chunk 100 through F = 516
     only; the narrow kernel meets it at F = 1, 3 and 6 (rule B, one pair each) and with every pair only at F = 3,
     never at F = 1028 / 1100

Kernel instantiation -> test id that reaches it (DT in f32, bf16, i32, i64; OP in min, max, and sum for i32 / i64):

  hgnn_segment_reduce_ex, main pass; ids are F{F}-{DT}-{OP}-c{chunk}-{ends}-{shuf|srt}
    k_seg_arg_narrow<DT,OP>            F%4, F>1024, or a misaligned pointer
                                                       test_segarg_exact[F{1,3,6,1028,1100}-*], test_alignment_fallback
    k_seg_arg<DT,OP,4,1,4,4>           nvec<=4         test_segarg_exact[F{4,16}-*]
    k_seg_arg<DT,OP,8,1,4,4>           nvec<=8         test_segarg_exact[F{20,32}-*]
    k_seg_arg<DT,OP,16,1,4,4>          nvec<=16        test_segarg_exact[F{36,64}-*]
    k_seg_arg<DT,OP,32,1,4,4>          nvec<=32        test_segarg_exact[F{68,128}-*]
    k_seg_arg<DT,OP,64,1,16,16>        nvec<=64        test_segarg_exact[F{132,252,256}-{f32,bf16,i32}-*]
    k_seg_arg<i64,OP,64,1,8,16>        nvec<=64        test_segarg_exact[F{132,252,256}-i64-*]
    k_seg_arg<DT,OP,64,2,4,4>          nvec<=128       test_segarg_exact[F{260,512}-*]
    k_seg_arg<DT,OP,64,4,2,4>          nvec<=256       test_segarg_exact[F{516,1024}-*]
      perm = plan.perm  *-shuf        perm = NULL (sorted index)  *-srt
    k_arg_combine<DT,OP>: every case (all have split lists, one with more than 64 partial rows), test_launch_edges
  hgnn_segment_arg_backward
    k_arg_scatter<float>, <uint16_t>   test_arg_backward_exact[*]; second grid-stride trip: test_arg_backward_second_trip
  refusals (nothing written)           test_refusals_write_nothing
  scatter_min / scatter_max / integer scatter_add on views, int32 index, wrong plan   test_wrappers_*

Wall time of this file on an MI355X: 6.9 s for the 397 tests (272 cases of rules A and B, 73 of rule C, 52 others);
the slowest case 0.36 s (test_segarg_exact[F4-f32-min-cdefault-empty-shuf], the first one, which carries the
warm-up), every other one at most 0.07 s (test_segarg_exact[F1100-i64-min-cdefault-one-srt]).
"""
import ctypes

import pytest
import torch

import rows_ref as R
import segarg_ref as S
import test_gpu_rows_exact as X

pytestmark = pytest.mark.gpu

POISON = {torch.int16: 0x7FC1, torch.int32: 0x7FC0BEEF, torch.int64: 0x7FC0BEEF7FC0BEEF}
ERR_INVALID_ARG, ERR_UNSUPPORTED = 1, 4          # HGNN_ERR_*


@pytest.fixture(scope="module", autouse=True)
def lib():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from hierarchicalgnn_amd import _lib
    import hierarchicalgnn_amd as H
    yield _lib.load()
    X._GRAPHS.clear()
    X._PLANS.clear()
    S._INDEX.clear()
    H.clear_plan_cache()


def _L():
    from hierarchicalgnn_amd import _lib
    return _lib


def _codes():
    L = _L()
    return ({"sum": L.RED_SUM, "min": L.RED_MIN, "max": L.RED_MAX},
            {"f32": L.DT_F32, "bf16": L.DT_BF16, "i32": L.DT_I32, "i64": L.DT_I64})


class GuardedBuf:
    """``n`` elements of ``dtype`` (float or integer) inside a poisoned buffer with 64 guard elements on either side;
    ``offset`` further leading elements move the payload off its 16-byte alignment by that many elements"""

    def __init__(self, n, dtype, offset=0):
        bt = S.BITS[dtype]
        self.n, self.lo, self.poison = int(n), 64 + offset, POISON[bt]
        self.bits = torch.empty(self.lo + self.n + 64, dtype=bt, device="cuda")
        self.bits.fill_(self.poison)
        self.data = self.bits[self.lo:self.lo + self.n]
        assert offset or self.data.data_ptr() % 16 == 0

    def addr(self):
        return self.data.data_ptr()

    def ptr(self):
        return ctypes.c_void_p(self.addr())

    def guards_intact(self, what):
        assert bool((self.bits[:self.lo] == self.poison).all()), f"{what}: wrote BEFORE the buffer"
        assert bool((self.bits[self.lo + self.n:] == self.poison).all()), f"{what}: wrote PAST the buffer"

    def all_written(self, what):
        n = int((self.data == self.poison).sum())
        assert n == 0, f"{what}: {n} elements never written"

    def untouched(self, what):
        assert bool((self.bits == self.poison).all()), f"{what}: written to"


class Buffers:
    """the four output / scratch buffers of one hgnn_segment_reduce_ex call, guarded; ``off``: names to misalign"""

    def __init__(self, plan, F, dtype, off=()):
        n_part = max(int(plan.c.max_partial), 1) * F
        self.out = GuardedBuf(plan.N * F, dtype, int("out" in off))
        self.arg = GuardedBuf(plan.N * F, torch.int64, int("arg" in off))
        self.partial = GuardedBuf(n_part, dtype, int("partial" in off))
        self.partial_arg = GuardedBuf(n_part, torch.int32, int("partial_arg" in off))

    def all(self):
        return (("out", self.out), ("arg", self.arg), ("partial", self.partial), ("partial_arg", self.partial_arg))


def call_ex(plan_c, op, dtype_code, src_ptr, F, b, arg_null=False):
    """the raw status of hgnn_segment_reduce_ex on the buffers ``b``"""
    L = _L()
    return L.load().hgnn_segment_reduce_ex(
        ctypes.byref(plan_c), op, dtype_code, src_ptr, F, b.out.ptr(), ctypes.c_void_p(0) if arg_null else b.arg.ptr(),
        b.partial.ptr(), b.partial_arg.ptr(), L.current_stream(torch.device("cuda")))


def first_difference(out_bits, arg, ref_out, ref_arg, what, lengths):
    """bitwise equality of out (and arg) at every element; on failure name the first wrong (row, column)"""
    ref_bits = ref_out.contiguous().view(S.BITS[ref_out.dtype])
    assert out_bits.shape == ref_bits.shape and out_bits.dtype == ref_bits.dtype, what
    bad = out_bits != ref_bits
    if ref_arg is not None:
        bad |= arg != ref_arg
    if not bool(bad.any()):
        return
    r, c = (int(v) for v in torch.nonzero(bad)[0])
    msg = (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at row {r} (list of {lengths[r]} rows), "
           f"column {c}: out bits {int(out_bits[r, c]):#x}, want {int(ref_bits[r, c]):#x}")
    if ref_arg is not None:
        msg += f"; arg {int(arg[r, c])}, want {int(ref_arg[r, c])}"
    raise AssertionError(msg)


def run_exact(plan, src_dev, dt, op, ref, what, lengths, off=()):
    """both partial_arg fills x two calls each, every result against ``ref``; returns the bits of the first result.
    ``off``: the buffers to misalign by one element (a misaligned ``src_dev`` is the caller's)"""
    ops, dts = _codes()
    dtype, F = S.DTYPES[dt], int(src_dev.shape[1])
    ref_out, ref_arg = ref
    first = None
    for fill in (0, POISON[torch.int32]):
        b = Buffers(plan, F, dtype, off)
        b.partial_arg.data.fill_(fill)
        addr = dict(src=src_dev.data_ptr(), out=b.out.addr(), partial=b.partial.addr(), arg=b.arg.addr(),
                    partial_arg=b.partial_arg.addr())
        assert S.is_wide(F, dt, **addr) == (S.row_class(F) != 0 and not off and src_dev.data_ptr() % 16 == 0), what
        for call in range(2):
            tag = f"{what}, partial_arg filled with {fill:#x}, call {call + 1}"
            rc = call_ex(plan.c, ops[op], dts[dt], ctypes.c_void_p(src_dev.data_ptr()), F, b)
            _L().check(rc, "hgnn_segment_reduce_ex")
            for name, buf in b.all():
                buf.guards_intact(f"{tag}: {name}")
            b.out.all_written(f"{tag}: out")
            if op == "sum":
                b.arg.untouched(f"{tag}: arg of a sum")
                assert bool((b.partial_arg.data == fill).all()), f"{tag}: partial_arg of a sum written to"
                arg = None
            else:
                b.arg.all_written(f"{tag}: arg")
                arg = b.arg.data.view(plan.N, F).cpu()
            out_bits = b.out.data.view(plan.N, F).cpu()
            first_difference(out_bits, arg, ref_out, ref_arg, tag, lengths)
            first = first if first is not None else (out_bits, arg)
    return first


# ------------------------------------------------------------------ every instantiation x every list-length edge
@pytest.mark.parametrize("case", S.cases(), ids=repr)
def test_segarg_exact(case):
    case.build()
    g = X.graph(case.ends, case.chunk)
    assert g.lengths == case.lengths and torch.equal(g.shuf if case.kind == "shuf" else g.srt, case.index)
    plan = X.plan_for(case.ends, case.chunk, case.kind)
    assert plan.counts_host()["split"] > 0 and (plan.c.src_row is None) == (case.kind == "srt")
    try:
        run_exact(plan, case.src.cuda(), case.dt, case.op, case.reference(), case.id, case.lengths)
    finally:
        case.src = case._ref = None


def test_case_list_is_the_rows_file_widths():
    assert sorted(S.WIDE_WIDTHS) == sorted(X.F32_VECTOR) and S.NARROW_WIDTHS == X.F32_SCALAR
    assert S.CHUNKS == X.CHUNKS


# ------------------------------------------------------------------ alignment fallback
def _misaligned_copy(t):
    """the same values, one element off the allocation's alignment"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0
    return view


@pytest.mark.parametrize("dt", ("f32", "bf16", "i32", "i64"))
@pytest.mark.parametrize("F", (8, 64, 256))
def test_alignment_fallback(F, dt):
    """a call is `wide` only if src, out, partial, arg and partial_arg are all aligned: with any of them one element
    off, the narrow kernel must give the bits of the aligned call (and stay inside the guards)"""
    names = ("src", "out", "arg", "partial", "partial_arg")
    for op in ("min", "max") + (() if S.is_float(dt) else ("sum",)):
        case = S.Case(F, dt, op, 5, "split", "shuf").build()
        plan = X.plan_for("split", 5, "shuf")
        ref = case.reference()
        src = case.src.cuda()
        aligned = run_exact(plan, src, dt, op, ref, f"{case.id} aligned", case.lengths)
        moved = _misaligned_copy(src)
        for off in [(n,) for n in names] + [names]:
            got = run_exact(plan, moved if "src" in off else src, dt, op, ref, f"{case.id} misaligned {off}",
                            case.lengths, off=tuple(n for n in off if n != "src"))
            assert torch.equal(got[0], aligned[0]) and (op == "sum" or torch.equal(got[1], aligned[1]))


# ------------------------------------------------------------------ launch edges
def _plan_of(lengths, chunk, seed=3):
    import hierarchicalgnn_amd as H
    shuf, _ = R.index_with_lengths(lengths, seed=seed)
    return shuf, H.GraphPlan(shuf.cuda(), len(lengths), chunk=chunk)


def _grid_values(M, F, dt, seed):
    grid = S.GRIDS[dt]
    return grid[torch.randint(0, len(grid), (M, F), generator=torch.Generator().manual_seed(seed))]


@pytest.mark.parametrize("dt,op", S.PAIRS, ids=lambda v: str(v))
def test_launch_edges(dt, op):
    ops, dts = _codes()
    dtype = S.DTYPES[dt]
    for F in (3, 8, 260):
        # N = 0: out == NULL is accepted and nothing is written
        index, plan = _plan_of([], 5)
        b = Buffers(plan, F, dtype)
        L = _L()
        rc = L.load().hgnn_segment_reduce_ex(ctypes.byref(plan.c), ops[op], dts[dt], None, F, None, b.arg.ptr(),
                                             b.partial.ptr(), b.partial_arg.ptr(), L.current_stream(torch.device("cuda")))
        L.check(rc, "hgnn_segment_reduce_ex at N = 0")
        for name, buf in b.all():
            buf.untouched(f"N = 0, F{F}: {name}")
        # M = 0, N = 5: out all 0, arg all 0 (= M); then N = 1 (one row, unsplit, split) and a hub destination
        for lengths in ([0] * 5, [1], [5], [16], [2, 64 * 5 + 7, 0, 1]):
            index, plan = _plan_of(lengths, 5)
            M, N = int(index.numel()), len(lengths)
            what = f"lengths {lengths}, F{F}"
            if max(lengths) > 5:
                n_part = -(-max(lengths) // 5)
                assert plan.counts_host()["partial"] == n_part and (n_part > 64) == (len(lengths) == 4)
            src = _grid_values(M, F, dt, 7 * F + M)
            ref = S.segarg_ref(src, index, N, op)
            ref = (ref, None) if op == "sum" else ref
            src_dev = src.cuda() if M else torch.empty((1, F), dtype=dtype, device="cuda")
            out_bits, arg = run_exact(plan, src_dev, dt, op, ref, what, lengths)
            if M == 0:
                assert not bool(out_bits.any()) and (arg is None or not bool(arg.any()))


# ------------------------------------------------------------------ refusals
def test_refusals_write_nothing():
    ops, dts = _codes()
    L = _L()
    F = 8
    g, plan = X.graph("one", 5), X.plan_for("one", 5, "shuf")
    src = _grid_values(g.M, F, "f32", 1).cuda()
    isrc = _grid_values(g.M, F, "i32", 1).cuda()
    gss = X.plan_for("one", 5, "gss")
    gsrc = _grid_values(g.n_src, F, "f32", 2).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                 # noqa: E731
    refused = [
        ("unknown op", plan, 7, dts["f32"], p(src), F, False, ERR_INVALID_ARG),
        ("negative op", plan, -1, dts["i32"], p(isrc), F, False, ERR_INVALID_ARG),
        ("float64 dtype", plan, ops["min"], L.DT_F64, p(src), F, False, ERR_INVALID_ARG),
        ("unknown dtype", plan, ops["max"], 99, p(src), F, False, ERR_INVALID_ARG),
        ("fp32 sum", plan, ops["sum"], dts["f32"], p(src), F, False, ERR_UNSUPPORTED),
        ("bf16 sum", plan, ops["sum"], dts["bf16"], p(src), F, False, ERR_UNSUPPORTED),
        ("gather plan", gss, ops["min"], dts["f32"], p(gsrc), F, False, ERR_INVALID_ARG),
        ("gather plan, sum", gss, ops["sum"], dts["i32"], p(isrc), F, False, ERR_INVALID_ARG),
        ("F = 0", plan, ops["min"], dts["f32"], p(src), 0, False, ERR_INVALID_ARG),
        ("F < 0", plan, ops["sum"], dts["i32"], p(isrc), -4, False, ERR_INVALID_ARG),
        ("NULL arg for min", plan, ops["min"], dts["f32"], p(src), F, True, ERR_INVALID_ARG),
        ("NULL arg for max", plan, ops["max"], dts["i32"], p(isrc), F, True, ERR_INVALID_ARG),
    ]
    for what, pl, op, dtc, sp, width, arg_null, want in refused:
        b = Buffers(pl, F, torch.float32)
        rc = call_ex(pl.c, op, dtc, sp, width, b, arg_null=arg_null)
        assert rc == want, f"{what}: status {rc}, want {want}"
        assert L.load().hgnn_last_error(), what
        torch.cuda.synchronize()
        for name, buf in b.all():
            buf.untouched(f"{what}: {name}")
    # the same calls are accepted once the offending argument is put right
    b = Buffers(plan, F, torch.float32)
    assert call_ex(plan.c, ops["min"], dts["f32"], p(src), F, b) == 0
    b.out.all_written("accepted call")


# ------------------------------------------------------------------ hgnn_segment_arg_backward
def _backward_inputs(N, F, dtype, seed):
    """arg with valid positions (distinct within a column, as a real arg is), M, -1 and M + 7; grad_out bits; the
    expected grad_src bits: zeros plus the exact assignments"""
    g = torch.Generator().manual_seed(seed)
    M = N + 3
    perm = torch.randperm(M, generator=g)
    arg = perm[(torch.arange(N).view(-1, 1) + torch.arange(F).view(1, -1)) % M]
    r = torch.randint(0, 12, (N, F), generator=g)
    arg = torch.where(r == 0, torch.full_like(arg, M), arg)
    arg = torch.where(r == 1, torch.full_like(arg, -1), arg)
    arg = torch.where(r == 2, torch.full_like(arg, M + 7), arg)
    bt = S.BITS[dtype]
    gbits = torch.randint(1, 1 << (15 if bt == torch.int16 else 31), (N, F), generator=g).to(bt)
    want = torch.zeros((M, F), dtype=bt)
    ok = (arg >= 0) & (arg < M)
    cols = torch.arange(F).view(1, -1).expand(N, F)
    want[arg[ok], cols[ok]] = gbits[ok]
    assert int(ok.sum()) < N * F or N * F < 12
    return M, arg, gbits, want


def _run_backward(N, F, dt):
    L = _L()
    _, dts = _codes()
    dtype = S.DTYPES[dt]
    M, arg, gbits, want = _backward_inputs(N, F, dtype, 31 * N + F)
    arg_d, g_d = arg.cuda(), gbits.cuda()
    out = GuardedBuf(M * F, dtype)
    for call in range(2):
        L.check(L.load().hgnn_segment_arg_backward(L.ptr(arg_d), N, F, M, dts[dt], L.ptr(g_d), out.ptr(),
                                                   L.current_stream(torch.device("cuda"))), "hgnn_segment_arg_backward")
        out.guards_intact(f"arg_backward N{N} F{F} {dt}")
        got = out.data.view(M, F).cpu()
        if not torch.equal(got, want):
            r, c = (int(v) for v in torch.nonzero(got != want)[0])
            raise AssertionError(f"arg_backward N{N} F{F} {dt}, call {call + 1}: {int((got != want).sum())} elements "
                                 f"differ; first at grad_src[{r}, {c}]: bits {int(got[r, c]):#x}, want {int(want[r, c]):#x}")


@pytest.mark.parametrize("dt", ("f32", "bf16"))
@pytest.mark.parametrize("N,F", S.BACKWARD_SHAPES)
def test_arg_backward_exact(N, F, dt):
    """N * F at 255 / 256 / 257 (one 256-thread block, and one element into the next) for F in {1, 3, 4, 256}"""
    _run_backward(N, F, dt)


@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_arg_backward_second_trip(dt):
    """the grid is capped at 8192 blocks x 256 threads = 2,097,152: N = 8193 x F = 256 = 2,097,408 elements send the
    first 256 threads round the grid-stride loop a second time"""
    N, F = S.BACKWARD_SECOND_TRIP
    assert S.scatter_trips(N, F) == (8192, 2)
    _run_backward(N, F, dt)


def test_arg_backward_refuses_integer_rows_and_writes_nothing():
    L = _L()
    _, dts = _codes()
    arg = torch.zeros((4, 4), dtype=torch.int64, device="cuda")
    grad = torch.ones((4, 4), dtype=torch.int32, device="cuda")
    out = GuardedBuf(7 * 4, torch.int32)
    for what, dtc, F in (("int32 rows", dts["i32"], 4), ("int64 rows", dts["i64"], 4), ("F = 0", dts["f32"], 0)):
        rc = L.load().hgnn_segment_arg_backward(L.ptr(arg), 4, F, 7, dtc, L.ptr(grad), out.ptr(),
                                                L.current_stream(torch.device("cuda")))
        assert rc == ERR_INVALID_ARG, what
        torch.cuda.synchronize()
        out.untouched(what)


# ------------------------------------------------------------------ the Python operators
@pytest.mark.parametrize("dt", ("f32", "bf16", "i32", "i64"))
def test_wrappers_on_views_and_an_int32_index(dt):
    """scatter_min / scatter_max / integer scatter_add on a column slice and on a transposed src equal the call on a
    contiguous clone (and the reference); an int32 index is accepted"""
    import hierarchicalgnn_amd as H
    F = 20
    g = X.graph("split", 5)
    fns = [("min", H.scatter_min), ("max", H.scatter_max)] + ([] if S.is_float(dt) else [("sum", H.scatter_add)])
    wide = _grid_values(g.M, 2 * F + 1, dt, 11).cuda()
    tall = _grid_values(F, g.M, dt, 12).cuda()
    views = (("column slice", wide[:, 1:1 + F]), ("transposed", tall.t()))
    for what, view in views:
        assert not view.is_contiguous() and tuple(view.shape) == (g.M, F)
        clone = view.contiguous().clone()
        for op, fn in fns:
            ref = S.segarg_ref(clone.cpu(), g.shuf, g.N, op)
            ref = (ref, None) if op == "sum" else ref
            for index in (g.dev["shuf"], g.dev["shuf"].int()):
                results = [fn(src, index, dim=0, dim_size=g.N) for src in (view, clone)]
                for res in results:
                    out, arg = (res, None) if op == "sum" else res
                    assert out.dtype == S.DTYPES[dt] and out.is_contiguous()
                    first_difference(out.cpu().view(S.BITS[out.dtype]), None if arg is None else arg.cpu(), ref[0],
                                     ref[1], f"{what} {dt} {op} index {index.dtype}", g.lengths)


def test_wrappers_refuse_a_plan_of_another_index():
    import hierarchicalgnn_amd as H
    g, plan = X.graph("split", 5), X.plan_for("split", 5, "shuf")
    other = X.graph("one", 5)
    assert other.M != g.M
    src, other_src = _grid_values(g.M, 4, "i32", 1).cuda(), _grid_values(other.M, 4, "i32", 1).cuda()
    for fn in (H.scatter_min, H.scatter_max, H.scatter_add):
        fn(src, g.dev["shuf"], dim=0, dim_size=g.N, plan=plan)                  # the matching call is accepted
        with pytest.raises(RuntimeError, match="plan does not match"):          # another number of rows
            fn(other_src, other.dev["shuf"], dim=0, dim_size=other.N, plan=plan)
        with pytest.raises(RuntimeError, match="plan does not match"):          # another dim_size
            fn(src, g.dev["shuf"], dim=0, dim_size=g.N + 1, plan=plan)
        with pytest.raises(RuntimeError, match="plan does not match"):          # a gather plan
            fn(src, g.dev["shuf"], dim=0, dim_size=g.N, plan=X.plan_for("split", 5, "gss"))
