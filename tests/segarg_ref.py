"""CPU reference and case list for the exact conformance of csrc/segminmax.hip (scatter_min / scatter_max with arg,
wrapping integer sums).  tests/test_segarg_ref.py proves this file; tests/test_gpu_segarg_exact.py runs the cases.

Definition (``segarg_ref``).  MIN / MAX: of the rows p with index[p] == d, in increasing p, drop NaN; m is the IEEE
min / max of the rest compared in the element's own type (bf16 widens exactly to fp32, int64 stays int64);
arg[d, f] is the smallest p with src[p, f] == m and out[d, f] = src[arg, f] bit for bit, so the sign of a zero is
that of its first occurrence.  No candidate: out = 0, arg = M.  SUM (int32 / int64): two's-complement wrapping
addition, computed on the unsigned view.  Nothing rounds, so every comparison with a kernel is bitwise.

Cases.  Indices are those of tests/test_gpu_rows_exact.py (``rows_ref.standard_lengths`` with the same seeds: every
loop edge 0..193, the chunk edges c-1 .. 3c+1, 64c+1, runs of empty destinations, first / last destination empty /
one row / split).  Values come from tie-heavy grids of at most nine values (``GRIDS``), and the conditions a min /
max / sum kernel goes wrong on are PLANTED, one destination each, in every column of that destination:

  a            the winner occurs at least twice and its first occurrence is not the first row of the list
  b            a float list of at least one row that is all NaN
  c            a float list whose first row is NaN and which has a finite candidate
  d_neg_first  a -0.0 / +0.0 tie whose first zero is -0.0      d_pos_first  ... whose first zero is +0.0
  denormal     (float) the winner is the smallest denormal (MAX: over +-0.0, which a flushing compare would tie)
  e            a split destination whose winner ties between an earlier and a later chunk
  f            a split destination whose unique winner is in its last chunk
  g            (float) a split destination with one chunk all NaN
  h            (int) the two best candidates of one list differ by 1 at 2^24 / 2^53 (equal in float32 / float64)
  i, i_split   (SUM) an unsplit-or-any / a split list whose true sum overflows the type
  j            a list longer than 64 rows whose winner lies beyond row 64 of the list
  empty        a destination without rows

``conditions(case)`` evaluates each of them on the case's inputs (not on what was planted), at every column.
"""
import numpy as np
import torch

import rows_ref as R

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "i32": torch.int32, "i64": torch.int64}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int32: torch.int32, torch.int64: torch.int64}
PAIRS = tuple((d, o) for d in ("f32", "bf16", "i32", "i64") for o in ("min", "max")) + (("i32", "sum"), ("i64", "sum"))
WIDE_WIDTHS = (4, 16, 20, 32, 36, 64, 68, 128, 132, 252, 256, 260, 512, 516, 1024)
NARROW_WIDTHS = (1, 3, 6, 1028, 1100)
WIDTHS = WIDE_WIDTHS + NARROW_WIDTHS
LONG_ITEM_WIDTHS = (3, 16, 32, 64, 128, 252, 260, 516)      # the narrow kernel and one width of each row shape
CHUNKS = (1, 5, 64, 100)          # explicit GraphPlan(chunk=); 0 = the default (32 at these sizes)
KINDS = ("shuf", "srt")
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _from_bits(bits, dtype):
    return torch.tensor(bits, dtype=BITS[dtype]).view(dtype)


# ascending, NaN last; 1 = the smallest denormal of either float type
GRIDS = {
    "f32": _from_bits([-0x00800000, -0x40000000, -0x80000000, 0, 1, 0x3F000000, 0x40400000, 0x7F800000, 0x7FC00000],
                      torch.float32),
    "bf16": _from_bits([-0x0080, -0x4000, -0x8000, 0, 1, 0x3F00, 0x4040, 0x7F80, 0x7FC0], torch.bfloat16),
    "i32": torch.tensor([I32_MIN, -1, 0, 1, 1 << 24, (1 << 24) + 1, I32_MAX], dtype=torch.int32),
    "i64": torch.tensor([I64_MIN, -(1 << 53) - 1, -(1 << 53), 0, 1 << 53, (1 << 53) + 1, 1 << 62, I64_MAX],
                        dtype=torch.int64),
}
# grid positions by name (float grids)
_NINF, _M2, _NZ, _PZ, _DEN, _HALF, _THREE, _PINF, _NAN = range(9)


def is_float(dt):
    return dt in ("f32", "bf16")


# ------------------------------------------------------------------ the reference
def list_rows(index, N):
    """(order, rowptr): the rows of destination d, in increasing position, are order[rowptr[d]:rowptr[d + 1]]"""
    order = torch.sort(index, stable=True).indices
    counts = torch.bincount(index, minlength=N) if index.numel() else torch.zeros(N, dtype=torch.int64)
    rowptr = [0] + torch.cumsum(counts, 0).tolist()
    return order, rowptr


def compare_view(src):
    """the tensor the comparisons run on: the element's own type, bf16 widened (exactly) to fp32"""
    return src.float() if src.dtype == torch.bfloat16 else src


def first_winner(blk, op):
    """blk [n, F] (n >= 1), rows in list order: (has [F], first [F]) -- whether the column has a candidate, and the
    list offset of the first row holding the min / max of the candidates"""
    if blk.dtype.is_floating_point:
        valid = ~torch.isnan(blk)
        worst = float("inf") if op == "min" else float("-inf")
        filled = torch.where(valid, blk, torch.full_like(blk, worst))
    else:
        valid, filled = torch.ones_like(blk, dtype=torch.bool), blk
    m = filled.amin(0) if op == "min" else filled.amax(0)
    eq = valid & (blk == m)
    return eq.any(0), eq.to(torch.uint8).argmax(0)          # argmax: the first of equal maxima


def segarg_ref(src, index, N, op):
    """(out [N, F] of src.dtype, arg [N, F] int64) for op 'min' / 'max'; out for 'sum' (int32 / int64 only)"""
    assert src.dim() == 2 and index.dim() == 1 and index.numel() == src.shape[0] and op in ("min", "max", "sum")
    M, F = int(src.shape[0]), int(src.shape[1])
    order, rowptr = list_rows(index, N)
    if op == "sum":
        assert src.dtype in (torch.int32, torch.int64), "floating-point sums are the K1 kernels'"
        u = np.uint32 if src.dtype == torch.int32 else np.uint64
        a = src.contiguous().numpy().view(u)
        out = np.zeros((N, F), dtype=u)
        o = order.numpy()
        for d in range(N):
            if rowptr[d + 1] > rowptr[d]:
                out[d] = np.add.reduce(a[o[rowptr[d]:rowptr[d + 1]]], axis=0, dtype=u)      # wraps: unsigned
        return torch.from_numpy(out.view(np.int32 if src.dtype == torch.int32 else np.int64))
    key, bits = compare_view(src), src.contiguous().view(BITS[src.dtype])
    out = torch.zeros((N, F), dtype=bits.dtype)
    arg = torch.full((N, F), M, dtype=torch.int64)
    cols = torch.arange(F)
    for d in range(N):
        rows = order[rowptr[d]:rowptr[d + 1]]
        if rows.numel() == 0:
            continue
        has, first = first_winner(key[rows], op)
        pos = rows[first]
        arg[d] = torch.where(has, pos, arg[d])
        out[d] = torch.where(has, bits[pos, cols], out[d])
    return out.view(src.dtype), arg


# ------------------------------------------------------------------ the dispatch of segminmax.hip, mirrored
ROW_SHAPES = {1: (4, 1), 2: (8, 1), 3: (16, 1), 4: (32, 1), 5: (64, 1), 6: (64, 2), 7: (64, 4)}   # class: (RL, VPL)
ELEM_BYTES = {"f32": 4, "bf16": 2, "i32": 4, "i64": 8}


def row_class(F):
    """0: k_seg_arg_narrow; 1..7: the class of for_row_shape<256>(F / 4) (rows_common.h)"""
    if F % 4 or F > 1024:
        return 0
    nvec = F // 4
    for cls, limit in ((1, 4), (2, 8), (3, 16), (4, 32), (5, 64), (6, 128)):
        if nvec <= limit:
            return cls
    return 7


def last_group_full(F):
    """whether every lane of the row's last column group holds a column (no lane with cv >= nvec)"""
    RL, VPL = ROW_SHAPES[row_class(F)]
    return F // 4 == RL * VPL


def rows_in_flight(cls, dt):
    RL, VPL = ROW_SHAPES[cls]
    return 4 if RL < 64 else ((8 if dt == "i64" else 16) if VPL == 1 else 4 if VPL == 2 else 2)


def inner_step(cls, dt):
    """rows per inner trip of k_seg_arg: G * U"""
    return 64 // ROW_SHAPES[cls][0] * rows_in_flight(cls, dt)


def is_wide(F, dt, src=0, out=0, partial=0, arg=0, partial_arg=0):
    """the `wide` rule of hgnn_segment_reduce_ex on the five addresses (0 = NULL)"""
    al = min(4 * ELEM_BYTES[dt], 16)
    return (F % 4 == 0 and F <= 1024 and src % al == 0 and out % al == 0 and partial % al == 0 and arg % 16 == 0 and
            partial_arg % 16 == 0)


def kernel_name(F, dt, op):
    cls = row_class(F)
    if cls == 0:
        return f"k_seg_arg_narrow<{dt},{op}>"
    RL, VPL = ROW_SHAPES[cls]
    return f"k_seg_arg<{dt},{op},{RL},{VPL},{rows_in_flight(cls, dt)}>"


# hgnn_segment_arg_backward: one thread per (destination, column), 256-thread blocks, the grid capped (capped_grid)
BACKWARD_SHAPES = ((255, 1), (256, 1), (257, 1), (85, 3), (86, 3), (63, 4), (64, 4), (65, 4), (1, 256), (2, 256))
BACKWARD_SECOND_TRIP = (8193, 256)


def scatter_trips(N, F):
    """(blocks launched, grid-stride trips of the busiest thread) of k_arg_scatter on N x F elements"""
    total, block, cap = N * F, 256, 256 * 8 * 4
    blocks = min(max(-(-total // block), 1), cap)
    return blocks, -(-total // (blocks * block))


# ------------------------------------------------------------------ indices: those of test_gpu_rows_exact.Graph
_INDEX = {}


def case_index(ends, chunk):
    """(lengths, shuffled, sorted) of test_gpu_rows_exact.Graph(ends, chunk), without touching a device"""
    key = (ends, chunk)
    if key not in _INDEX:
        c = chunk or 32
        lengths = R.standard_lengths(c, ends, seed=17 * c + R.ENDS.index(ends))
        shuf, srt = R.index_with_lengths(lengths, seed=c + 5)
        assert chunk or R.default_chunk(int(shuf.numel())) == 32
        rows = {"shuf": list_rows(shuf, len(lengths)), "srt": list_rows(srt, len(lengths))}
        _INDEX[key] = (lengths, {"shuf": shuf, "srt": srt}, rows)
    return _INDEX[key]


def chunk_of(n, c):
    """(number of chunks, rows per chunk) the plan gives a list of n rows (rows_ref.plan_reference)"""
    nch = -(-n // c) if n > c else 1
    return nch, max(-(-n // nch), 1)


# ------------------------------------------------------------------ cases
class Case:
    def __init__(self, F, dt, op, chunk, ends, kind):
        self.F, self.dt, self.op, self.chunk, self.ends, self.kind = F, dt, op, chunk, ends, kind
        self.c = chunk or 32
        self.id = f"F{F}-{dt}-{op}-c{chunk or 'default'}-{ends}-{kind}"
        self.src = self._ref = None

    def __repr__(self):
        return self.id

    # ---- inputs
    def build(self):
        if self.src is not None:
            return self
        self.lengths, idx, rows = case_index(self.ends, self.chunk)
        self.index = idx[self.kind]
        self.order, self.rowptr = rows[self.kind]
        self.N, self.M = len(self.lengths), int(self.index.numel())
        self.grid = GRIDS[self.dt]
        seed = 100_000 * PAIRS.index((self.dt, self.op)) + 20 * self.F + self.chunk % 17
        self.gen = torch.Generator().manual_seed(seed)
        codes = torch.randint(0, len(self.grid), (self.M, self.F), generator=self.gen)
        self.src = self.grid[codes]
        self.planted, self._used = {}, {0, self.N - 1}
        self._plant()
        return self

    def rows_of(self, d):
        return self.order[self.rowptr[d]:self.rowptr[d + 1]]

    def _pick(self, name, ok, prefer=None):
        for want in ((prefer, None) if prefer is not None else (None,)):
            for d, n in enumerate(self.lengths):
                if d not in self._used and ok(n) and (want is None or want(n)):
                    self._used.add(d)
                    self.planted[name] = d
                    return d, n
        raise AssertionError(f"{self.id}: no destination left for condition {name}")

    def _fill(self, d, codes_allowed, fixed=()):
        """the rows of destination d: random grid values among ``codes_allowed``, then ``fixed`` = (offset, code)"""
        rows = self.rows_of(d)
        allowed = torch.tensor(codes_allowed)
        pick = allowed[torch.randint(0, len(allowed), (rows.numel(), self.F), generator=self.gen)]
        for off, code in fixed:
            pick[off] = code
        self.src[rows] = self.grid[pick]

    def _plant(self):
        c, op, dt = self.c, self.op, self.dt
        G = len(self.grid)
        split = lambda n: n > c                                              # noqa: E731
        if op == "sum":
            top = G - 1                                                      # INT_MAX
            d, n = self._pick("i", lambda n: n >= 2, lambda n: not split(n))
            self._fill(d, [top])
            d, n = self._pick("i_split", split)
            self._fill(d, [top])
            return
        fl = is_float(dt)
        if fl:
            best = _NINF if op == "min" else _PINF
            rest = [k for k in range(G) if k not in (best, _NAN)]            # worse than best, never NaN
        else:
            best = 0 if op == "min" else G - 1
            rest = [k for k in range(G) if k != best]
        d, n = self._pick("j", lambda n: n >= 65, lambda n: not split(n))
        self._fill(d, rest, [(64 + (n - 65) // 2, best)])
        d, n = self._pick("e", split)
        nch, ln = chunk_of(n, c)
        self._fill(d, rest, [(min(1, ln - 1), best), (n - 1, best)])
        d, n = self._pick("f", split)
        self._fill(d, rest, [(n - 1, best)])
        d, n = self._pick("a", lambda n: n >= 3, lambda n: not split(n))
        self._fill(d, rest, [(1, best), (n - 1, best)])
        if fl:
            d, n = self._pick("g", split)
            nch, ln = chunk_of(n, c)
            self._fill(d, rest, [(k, _NAN) for k in range(ln)])
            d, n = self._pick("b", lambda n: n >= 1, lambda n: n >= 2)
            self._fill(d, [_NAN])
            d, n = self._pick("c", lambda n: n >= 2, lambda n: n >= 3)
            self._fill(d, [_M2, _NZ, _PZ, _DEN, _HALF, _THREE], [(0, _NAN), (1, _HALF)])
            worse = [_HALF, _THREE, _PINF, _NAN] if op == "min" else [_NINF, _M2, _NAN]
            d, n = self._pick("d_neg_first", lambda n: n >= 2, lambda n: n >= 4)
            self._fill(d, worse + [_NZ, _PZ], [(0, worse[0]), (1, _NZ), (n - 1, _PZ)] if n >= 3 else [(0, _NZ), (1, _PZ)])
            d, n = self._pick("d_pos_first", lambda n: n >= 2, lambda n: n >= 4)
            self._fill(d, worse + [_NZ, _PZ], [(0, worse[0]), (1, _PZ), (n - 1, _NZ)] if n >= 3 else [(0, _PZ), (1, _NZ)])
            d, n = self._pick("denormal", lambda n: n >= 3)
            if op == "min":
                self._fill(d, [_HALF, _THREE], [(1, _DEN)])
            else:
                self._fill(d, [_NZ, _PZ, _M2], [(0, _PZ), (n - 1, _DEN)])
        else:
            # the better of the pair comes second, so a comparison through float (a tie) names the wrong row
            if op == "max":
                lo, hi = (4, 5)                                              # 2^24 / 2^53, then + 1
                worse = [0, 1, 2, 3]
            elif dt == "i32":
                lo, hi = (5, 4)                                              # 2^24 + 1, then 2^24
                worse = [6]
            else:
                lo, hi = (2, 1)                                              # -2^53, then -2^53 - 1
                worse = [3, 4, 5, 6, 7]
            d, n = self._pick("h", lambda n: n >= 3, lambda n: n >= 65)
            self._fill(d, worse, [(n // 3, lo), (2 * n // 3, hi)])
        zeros = [d for d, n in enumerate(self.lengths) if n == 0]
        self.planted["empty"] = zeros[len(zeros) // 2]

    # ---- reference, computed once per case
    def reference(self):
        self.build()
        if self._ref is None:
            r = segarg_ref(self.src, self.index, self.N, self.op)
            self._ref = (r, None) if self.op == "sum" else r
        return self._ref


def required_conditions(dt, op):
    if op == "sum":
        return ("i", "i_split")
    common = ("a", "e", "f", "j", "empty")
    return common + (("b", "c", "d_neg_first", "d_pos_first", "denormal", "g") if is_float(dt) else ("h",))


def _true_sums_overflow(blk, dt):
    """whether the true (unbounded) sum of every column of blk [n, F] leaves the type; exact: the upper and the lower
    32 bits are summed apart in int64 (n < 2^31 rows) and put together as Python integers"""
    hi = (blk.long() >> 32).sum(0).tolist()
    low = (blk.long() & 0xFFFFFFFF).sum(0).tolist()
    lo, top = (I32_MIN, I32_MAX) if dt == "i32" else (I64_MIN, I64_MAX)
    return all(not lo <= (h << 32) + l <= top for h, l in zip(hi, low))


def conditions(case):
    """{condition: bool}: each condition of ``required_conditions`` evaluated on the inputs of ``case`` -- at the
    destination that claims it, at every column"""
    case.build()
    c, op, dt = case.c, case.op, case.dt
    out = {}
    for name in required_conditions(dt, op):
        d = case.planted[name]
        n = case.lengths[d]
        blk = compare_view(case.src[case.rows_of(d)])
        assert blk.shape[0] == n
        nch, ln = chunk_of(n, c)
        if name == "empty":
            out[name] = n == 0
            continue
        if name in ("i", "i_split"):
            out[name] = _true_sums_overflow(blk, dt) and (name == "i" or n > c)
            continue
        nan = torch.isnan(blk) if is_float(dt) else torch.zeros_like(blk, dtype=torch.bool)
        if name == "b":
            out[name] = n >= 1 and bool(nan.all())
            continue
        has, first = first_winner(blk, op)
        m = blk[first, torch.arange(case.F)]
        eq = ~nan & (blk == m)
        chunk_id = (torch.arange(n) // ln).view(-1, 1).expand(n, case.F)
        if name == "a":
            ok = has & (eq.sum(0) >= 2) & (first > 0)
        elif name == "c":
            ok = nan[0] & torch.isfinite(blk).any(0) & has
        elif name in ("d_neg_first", "d_pos_first"):
            zeros = eq & (blk == 0)
            neg = zeros & torch.signbit(blk)
            ok = has & (m == 0) & neg.any(0) & (zeros & ~neg).any(0) & \
                (torch.signbit(m) if name == "d_neg_first" else ~torch.signbit(m))
        elif name == "denormal":
            tiny = 2.0 ** -126
            ok = has & (m > 0) & (m < tiny)
            if op == "max":
                ok = ok & (blk == 0).any(0)
        elif name == "e":
            big = torch.full_like(chunk_id, 1 << 30)
            lo = torch.where(eq, chunk_id, big).amin(0)
            hi = torch.where(eq, chunk_id, -big).amax(0)
            ok = has & (lo < hi) & (n > c)
        elif name == "f":
            ok = has & (eq.sum(0) == 1) & (first // ln == nch - 1) & (nch >= 2)
        elif name == "g":
            all_nan = torch.stack([nan[k * ln:(k + 1) * ln].all(0) for k in range(nch)]).any(0)
            ok = all_nan & (n > c)
        elif name == "h":
            worst = torch.full_like(blk, (I64_MAX if dt == "i64" else I32_MAX) if op == "min" else
                                    (I64_MIN if dt == "i64" else I32_MIN))
            second = torch.where(eq, worst, blk)
            m2 = second.amin(0) if op == "min" else second.amax(0)
            through = torch.float32 if dt == "i32" else torch.float64
            ok = ((m - m2).abs() == 1) & (m.to(through) == m2.to(through)) & (n >= 3)
        elif name == "j":
            ok = has & (first >= 64) & (n > 64)
        else:
            raise AssertionError(name)
        out[name] = bool(ok.all())
    return out


def cases():
    """the pruned cross product the GPU file runs.
    A: every width x every (dtype, op) pair at the default chunk; the index kind rotates with (width + pair) and so
       does the end placement.
    B: every width x every explicit chunk (F >= 516: chunks 1 and 5 only), the pair rotating with (width + chunk).
    C: every pair at chunk 100 at one width per kernel (``LONG_ITEM_WIDTHS``): only a chunk above 64 hands a wave
       more than 64 rows, i.e. a second trip of the 64-row outer loop of k_seg_arg / k_seg_arg_narrow (below chunk
       65 every list of more than 64 rows is split).  Rule B stops at chunk 5 for F >= 516, so the widest row shape
       (RL 64, VPL 4) meets chunk 100 through F = 516 only; the narrow kernel meets it at F = 1, 3 and 6 (rule B, one
       pair each) and with every pair at F = 3, never at F = 1028 / 1100."""
    out = []
    for wi, F in enumerate(WIDTHS):
        for pi, (dt, op) in enumerate(PAIRS):                                # A
            out.append(Case(F, dt, op, 0, R.ENDS[(wi + pi) % 3], KINDS[(wi + pi) % 2]))
        for ci, chunk in enumerate(CHUNKS):                                  # B
            if F >= 516 and chunk > 5:
                continue
            dt, op = PAIRS[(wi + ci) % len(PAIRS)]
            out.append(Case(F, dt, op, chunk, R.ENDS[(wi + ci + 1) % 3], KINDS[(wi + ci + 1) % 2]))
    have = {(c.F, c.dt, c.op, c.chunk) for c in out}
    for wi, F in enumerate(LONG_ITEM_WIDTHS):                                # C
        for pi, (dt, op) in enumerate(PAIRS):
            if (F, dt, op, 100) not in have:
                out.append(Case(F, dt, op, 100, R.ENDS[(wi + pi) % 3], KINDS[(wi + pi + 1) % 2]))
    return out
