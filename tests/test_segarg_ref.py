"""CPU checks of tests/segarg_ref.py: the proof that a red test in test_gpu_segarg_exact.py is the kernel's fault.

* the reference against independent computations (a per-element Python loop, torch.scatter_reduce, np.add.at);
* mutants: each plausible wrong kernel differs from the reference at the destination that claims the matching
  condition, on every (dtype, op) x chunk x index-kind family;
* ``conditions()`` holds on every case the GPU file runs (the same list, ``segarg_ref.cases()``);
* the width list and the pruned cross product reach every kernel instantiation of csrc/segminmax.hip.
"""
import numpy as np
import pytest
import torch

import rows_ref as R
import segarg_ref as S


# ------------------------------------------------------------------ reference against independent computations
def _small(dt, seed, M=70, N=9, F=3):
    g = torch.Generator().manual_seed(seed)
    grid = S.GRIDS[dt]
    src = grid[torch.randint(0, len(grid), (M, F), generator=g)]
    index = torch.randint(0, N - 2, (M,), generator=g)           # the last destinations stay empty
    index[index == 3] = 4                                        # and one in the middle
    return src, index, N


def _naive(src, index, N, op):
    M, F = src.shape
    vals = S.compare_view(src).tolist()                          # python floats / ints: exact for every type here
    bits = src.contiguous().view(S.BITS[src.dtype])
    out = torch.zeros((N, F), dtype=bits.dtype)
    arg = torch.full((N, F), M, dtype=torch.int64)
    idx = index.tolist()
    for d in range(N):
        for f in range(F):
            best = None
            for p in range(M):
                x = vals[p][f]
                if idx[p] != d or x != x:
                    continue
                if best is None or (x < vals[best][f] if op == "min" else x > vals[best][f]):
                    best = p
            if best is not None:
                out[d, f], arg[d, f] = bits[best, f], best
    return out.view(src.dtype), arg


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(S.BITS[a.dtype]),
                                                                     b.contiguous().view(S.BITS[b.dtype]))


@pytest.mark.parametrize("dt,op", S.PAIRS, ids=lambda v: str(v))
def test_reference_equals_a_per_element_loop(dt, op):
    for seed in range(4):
        src, index, N = _small(dt, seed)
        if op == "sum":
            mod = 1 << (32 if dt == "i32" else 64)
            want = [[0] * src.shape[1] for _ in range(N)]
            for p, d in enumerate(index.tolist()):
                for f, x in enumerate(src[p].tolist()):
                    want[d][f] = (want[d][f] + x) % mod
            want = [[x - mod if x >= mod // 2 else x for x in row] for row in want]
            assert S.segarg_ref(src, index, N, op).tolist() == want
            continue
        out, arg = S.segarg_ref(src, index, N, op)
        want_out, want_arg = _naive(src, index, N, op)
        assert _same(out, want_out) and torch.equal(arg, want_arg)
        assert bool((arg[-2:] == src.shape[0]).all()) and not bool(out[-2:].view(S.BITS[out.dtype]).any())


@pytest.mark.parametrize("dt", ("f32", "bf16"))
@pytest.mark.parametrize("op", ("min", "max"))
def test_reference_values_equal_torch_scatter_reduce(dt, op):
    g = torch.Generator().manual_seed(5)
    M, N, F = 3000, 60, 20
    finite = S.GRIDS[dt][:-1]                                    # everything but NaN
    src = finite[torch.randint(0, len(finite), (M, F), generator=g)]
    index = torch.randint(0, N, (M,), generator=g)
    out, arg = S.segarg_ref(src, index, N, op)
    assert bool((arg < M).all())
    t = torch.zeros(N, F).scatter_reduce(0, index.view(-1, 1).expand(M, F), src.float(),
                                         "amin" if op == "min" else "amax", include_self=False)
    assert torch.equal(out.float(), t)                           # values (a zero's sign is the reference's own rule)
    assert torch.equal(src[arg, torch.arange(F)].float(), out.float())


@pytest.mark.parametrize("dt", ("i32", "i64"))
def test_reference_sum_equals_numpy_where_nothing_overflows(dt):
    g = torch.Generator().manual_seed(6)
    M, N, F = 3000, 60, 20
    src = torch.randint(-1000, 1000, (M, F), generator=g).to(S.DTYPES[dt])
    index = torch.randint(0, N, (M,), generator=g)
    want = np.zeros((N, F), np.int64)
    np.add.at(want, index.numpy(), src.numpy().astype(np.int64))
    out = S.segarg_ref(src, index, N, "sum")
    assert out.dtype == src.dtype and np.array_equal(out.numpy().astype(np.int64), want)


def test_reference_sum_wraps():
    for dt, top in (("i32", S.I32_MAX), ("i64", S.I64_MAX)):
        src = torch.tensor([[top], [top], [1], [top]], dtype=S.DTYPES[dt])
        out = S.segarg_ref(src, torch.tensor([0, 0, 1, 1]), 3, "sum")
        assert out.view(-1).tolist() == [-2, -top - 1, 0]


def test_named_outcomes():
    inf, nan = float("inf"), float("nan")
    src = torch.tensor([nan, 0.0, -0.0, nan, nan, -0.0, 0.0, inf, 1e-45, 0.0]).view(-1, 1)
    index = torch.tensor([0, 0, 0, 1, 1, 2, 2, 3, 4, 4])
    out, arg = S.segarg_ref(src, index, 6, "min")
    assert arg.view(-1).tolist() == [1, 10, 5, 7, 9, 10]
    assert out.view(torch.int32).view(-1).tolist() == [0, 0, -(1 << 31), 0x7F800000, 0, 0]
    out, arg = S.segarg_ref(src, index, 6, "max")
    assert arg.view(-1).tolist() == [1, 10, 5, 7, 8, 10]
    assert out.view(torch.int32).view(-1).tolist() == [0, 0, -(1 << 31), 0x7F800000, 1, 0]
    big = torch.tensor([[1 << 53], [(1 << 53) + 1], [1 << 53]])
    assert S.segarg_ref(big, torch.zeros(3, dtype=torch.int64), 1, "max")[1].item() == 1


def test_reference_is_quick_at_the_largest_shape():
    """F = 1024 with about 10^4 rows (the chunk-100 index; int64, the widest element): under a second"""
    import time
    c = S.Case(1024, "i64", "max", 100, "split", "shuf").build()
    assert c.M > 9000 and c.src.shape == (c.M, 1024)
    t0 = time.perf_counter()
    S.segarg_ref(c.src, c.index, c.N, "max")
    assert time.perf_counter() - t0 < 1.0


# ------------------------------------------------------------------ mutants
def _mutant(case, name):
    """what a kernel with the named defect would give: (out, arg), or out for a sum"""
    src, index, N, op, c = case.src, case.index, case.N, case.op, case.c
    M, F = src.shape
    order, rowptr = S.list_rows(index, N)
    if op == "sum":
        assert name == "sum_saturates"
        lo, hi = (S.I32_MIN, S.I32_MAX) if case.dt == "i32" else (S.I64_MIN, S.I64_MAX)
        out = torch.zeros((N, F), dtype=src.dtype)
        for d in range(N):
            rows = order[rowptr[d]:rowptr[d + 1]].tolist()
            for f in range(F):
                out[d, f] = min(max(sum(int(src[p, f]) for p in rows), lo), hi)
        return out
    key, bits = S.compare_view(src), src.contiguous().view(S.BITS[src.dtype])
    fl = S.is_float(case.dt)
    if name == "int_via_float":
        key = key.to(torch.float32 if case.dt == "i32" else torch.float64)
    out = torch.zeros((N, F), dtype=bits.dtype)
    arg = torch.full((N, F), M, dtype=torch.int64)
    cols = torch.arange(F)
    if name == "empty_extreme":
        ident = S.GRIDS[case.dt][(-2 if fl else -1) if op == "min" else 0]       # the identity of the fold
        out[:] = ident.view(1).view(bits.dtype)
    if name == "empty_arg_minus_1":
        arg[:] = -1
    if name == "empty_arg_last_row":
        arg[:] = M - 1                                                           # a valid position: the dangerous one
    better = (lambda a, b: a < b) if op == "min" else (lambda a, b: a > b)

    def winner(blk):
        n = blk.shape[0]
        has, first = S.first_winner(blk, op)
        if name == "last_tie":
            _, last = S.first_winner(blk.flip(0), op)
            first = n - 1 - last
        if name == "signed_zero" and fl:
            m = blk[first, cols]
            want = torch.signbit(blk) if op == "min" else ~torch.signbit(blk)
            pref = (blk == 0) & want & ~torch.isnan(blk)
            alt = pref.to(torch.uint8).argmax(0)
            first = torch.where(has & (m == 0) & pref.any(0), alt, first)
        if name == "nan_propagates" and fl:
            nan = torch.isnan(blk)
            first = torch.where(nan.any(0), nan.to(torch.uint8).argmax(0), first)
            has = has | nan.any(0)
        return has, first

    for d in range(N):
        rows = order[rowptr[d]:rowptr[d + 1]]
        n = rows.numel()
        if n == 0:
            continue
        if name == "first_64_rows":
            rows = rows[:64]
        nch, ln = S.chunk_of(n, c)
        if name == "drops_last_chunk" and nch > 1:
            rows = rows[:(nch - 1) * ln]
        if name == "combine_reversed" and nch > 1:
            # chunks folded last to first, a later one replacing the running one only when strictly better
            has = torch.zeros(F, dtype=torch.bool)
            pos = torch.zeros(F, dtype=torch.int64)
            for k in reversed(range(nch)):
                r = rows[k * ln:(k + 1) * ln]
                h, first = winner(key[r])
                p = r[first]
                take = h & (~has | better(key[p, cols], key[pos, cols]))
                pos, has = torch.where(take, p, pos), has | h
        else:
            has, first = winner(key[rows])
            pos = rows[first]
        arg[d] = torch.where(has, pos, arg[d])
        out[d] = torch.where(has, bits[pos, cols], out[d])
    return out.view(src.dtype), arg


# mutant -> the conditions whose destination it must get wrong, per (float?, op)
def _claims(name, dt, op):
    fl = S.is_float(dt)
    table = {
        "last_tie": ("a", "e"),
        "nan_propagates": ("b", "c", "g") if fl else (),
        "empty_extreme": ("empty", "b") if fl else ("empty",),
        "empty_arg_minus_1": ("empty", "b") if fl else ("empty",),
        "empty_arg_last_row": ("empty", "b") if fl else ("empty",),
        "int_via_float": () if fl else ("h",),
        "signed_zero": (("d_pos_first",) if op == "min" else ("d_neg_first",)) if fl else (),
        "combine_reversed": ("e",),
        "first_64_rows": ("j",),
        "drops_last_chunk": ("f",),
    }
    if op == "sum":
        return ("i", "i_split") if name == "sum_saturates" else ()
    return table.get(name, ())


MUTANTS = ("last_tie", "nan_propagates", "empty_extreme", "empty_arg_minus_1", "empty_arg_last_row",
           "int_via_float", "sum_saturates", "signed_zero", "combine_reversed", "first_64_rows", "drops_last_chunk")


def _families():
    out = []
    for pi, (dt, op) in enumerate(S.PAIRS):
        for ci, chunk in enumerate((0,) + S.CHUNKS):
            for ki, kind in enumerate(S.KINDS):
                out.append(S.Case(3, dt, op, chunk, R.ENDS[(pi + ci + ki) % 3], kind))
    return out


@pytest.mark.parametrize("case", _families(), ids=repr)
def test_every_mutant_fails_where_its_condition_is_planted(case):
    case.build()
    ref_out, ref_arg = case.reference()
    assert all(S.conditions(case).values())
    hit = set()
    for name in MUTANTS:
        claims = _claims(name, case.dt, case.op)
        if not claims:
            continue
        got = _mutant(case, name)
        out, arg = (got, None) if case.op == "sum" else got
        for cond in claims:
            d = case.planted[cond]
            differs = not _same(out[d], ref_out[d]) or (arg is not None and not torch.equal(arg[d], ref_arg[d]))
            assert differs, f"mutant {name} passes at destination {d} ({case.lengths[d]} rows), condition {cond}"
            hit.add(cond)
    # 'denormal' has a test of its own below; of the two zero ties, the one whose first zero the mutant would keep
    other_tie = "d_neg_first" if case.op == "min" else "d_pos_first"
    assert hit == set(S.required_conditions(case.dt, case.op)) - {"denormal", other_tie}, hit


def test_denormal_is_told_from_zero():
    """a compare that flushes denormals ties the denormal with the zeros of its list: another arg"""
    for dt in ("f32", "bf16"):
        for op in ("min", "max"):
            case = S.Case(4, dt, op, 5, "one", "shuf").build()
            d = case.planted["denormal"]
            rows = case.rows_of(d)
            flushed = case.src.clone()
            v = S.compare_view(flushed)
            flushed[(v.abs() > 0) & (v.abs() < 2.0 ** -126)] = 0
            out, arg = S.segarg_ref(flushed, case.index, case.N, op)
            ref_out, ref_arg = case.reference()
            assert not _same(out[d], ref_out[d])
            assert op == "min" or not torch.equal(arg[d], ref_arg[d])
            assert bool(torch.isin(ref_arg[d], rows).all())


# ------------------------------------------------------------------ the GPU file's cases
_CASES = S.cases()


def test_case_ids_are_unique_and_sizes_small():
    ids = [c.id for c in _CASES]
    assert len(set(ids)) == len(ids)
    for c in _CASES:
        lengths, idx, _ = S.case_index(c.ends, c.chunk)
        M = int(idx[c.kind].numel())
        assert M * c.F * S.ELEM_BYTES[c.dt] <= 10_500 * 1024 * 8 and M <= 10_500
        assert max(lengths) > 64 * c.c                              # a destination with more than 64 partial rows


@pytest.mark.parametrize("F", S.WIDTHS)
def test_conditions_hold_on_every_gpu_case(F):
    mine = [c for c in _CASES if c.F == F]
    assert len(mine) >= len(S.PAIRS) + 2
    for c in mine:
        got = S.conditions(c)
        assert set(got) == set(S.required_conditions(c.dt, c.op)), c.id
        assert all(got.values()), (c.id, got)
        # every case has split lists (64c + 1 rows at the least): none is exempt from e .. g
        assert c.op == "sum" or all(c.lengths[c.planted[k]] > c.c for k in ("e", "f"))
        c.src = None                                                 # free the inputs


# ------------------------------------------------------------------ coverage of the dispatch
def test_widths_reach_every_row_shape_full_and_partly_filled():
    assert S.row_class(4) == 1 and S.row_class(16) == 1 and S.row_class(20) == 2 and S.row_class(1024) == 7
    assert S.row_class(1028) == 0 and S.row_class(6) == 0 and S.row_class(516) == 7 and S.row_class(512) == 6
    by_class = {}
    for F in S.WIDE_WIDTHS:
        by_class.setdefault(S.row_class(F), set()).add(S.last_group_full(F))
    assert by_class == {cls: {True, False} for cls in range(1, 8)}, by_class
    narrow = [F for F in S.NARROW_WIDTHS if S.row_class(F) == 0]
    assert narrow == list(S.NARROW_WIDTHS)
    assert any(F % 4 == 0 and F > 1024 for F in narrow) and any(F % 4 and F > 4 for F in narrow) and 1 in narrow
    # rows per inner trip: 64, 32, 16, 8 for classes 1-4, then 16 (8 for int64), 4 and 2
    assert [S.inner_step(k, "f32") for k in range(1, 8)] == [64, 32, 16, 8, 16, 4, 2]
    assert [S.inner_step(k, "i64") for k in range(1, 8)] == [64, 32, 16, 8, 8, 4, 2]
    steps = {S.inner_step(k, dt) for k in range(1, 8) for dt in S.ELEM_BYTES}
    assert all({s - 1, s, s + 1} <= set(R.BASE_LENGTHS) for s in steps)      # every G*U +- 1 is a list length


def test_wide_rule_mirror():
    for dt, eb in S.ELEM_BYTES.items():
        al = min(4 * eb, 16)
        base = dict(src=4096, out=8192, partial=12288, arg=16384, partial_arg=20480)
        assert S.is_wide(64, dt, **base) and S.is_wide(64, dt, 4096, 8192)       # NULL partials / arg (a sum)
        assert not S.is_wide(66, dt, **base) and not S.is_wide(1028, dt, **base)
        for k, step in (("src", eb), ("out", eb), ("partial", eb), ("arg", 8), ("partial_arg", 4)):
            assert not S.is_wide(64, dt, **dict(base, **{k: base[k] + step})), (dt, k)
        assert S.is_wide(64, dt, **dict(base, src=base["src"] + al))


def test_backward_shapes_reach_the_block_edges_and_the_second_trip():
    """k_arg_scatter: N * F at 255 / 256 / 257 for every F that can reach them, and one shape past the capped grid"""
    by_F = {}
    for N, F in S.BACKWARD_SHAPES:
        by_F.setdefault(F, set()).add(N * F)
        assert S.scatter_trips(N, F)[1] == 1
    assert set(by_F) == {1, 3, 4, 256}
    assert by_F[1] == {255, 256, 257} and by_F[3] == {255, 258} and by_F[4] == {252, 256, 260} and 256 in by_F[256]
    assert {S.scatter_trips(N, F)[0] for N, F in S.BACKWARD_SHAPES} == {1, 2}
    N, F = S.BACKWARD_SECOND_TRIP
    assert S.scatter_trips(N, F) == (8192, 2) and N * F - 8192 * 256 == 256
    assert S.scatter_trips(8192, 256) == (8192, 1)


def test_every_pair_meets_every_class_kind_and_chunk():
    kernels = set()
    for dt, op in S.PAIRS:
        mine = [c for c in _CASES if (c.dt, c.op) == (dt, op)]
        assert {S.row_class(c.F) for c in mine} == set(range(8)), (dt, op)
        for cls in range(8):
            assert {c.kind for c in mine if S.row_class(c.F) == cls} == set(S.KINDS), (dt, op, cls)
        assert {c.chunk for c in mine} == {0} | set(S.CHUNKS), (dt, op)
        assert {c.kind for c in mine} == set(S.KINDS) and {c.ends for c in mine} == set(R.ENDS)
        kernels |= {S.kernel_name(c.F, dt, op) for c in mine}
        # a work item of more than 64 rows (chunk 100: a second trip of the 64-row outer loop) in every kernel
        assert {S.row_class(c.F) for c in mine if c.chunk == 100} == set(range(8)), (dt, op)
    # 10 pairs x (7 row shapes + the narrow kernel)
    assert len(kernels) == 80, sorted(kernels)
    assert [S.row_class(F) for F in S.LONG_ITEM_WIDTHS] == list(range(8))
    assert {(c.F, c.chunk) for c in _CASES} == {(F, ch) for F in S.WIDTHS for ch in (0,) + S.CHUNKS
                                                if not (F >= 516 and ch > 5)} | {(516, 100)}
    assert {(c.F, c.dt, c.op) for c in _CASES if c.chunk == 0} == {(F, d, o) for F in S.WIDTHS for d, o in S.PAIRS}
