"""Exact-arithmetic reference for the HBM-bound row kernels (segmented reduce, spread, gather, edge dot).

Every input is taken from a small dyadic grid, so every product and every partial sum -- in ANY order, with or
without FMA contraction -- is exactly representable in fp32, and a kernel's result must equal an integer
reference bit for bit:

    features    integers in +-{1..8}            (never 0: a dropped row always changes the sum; exact in bf16)
    weights     {0.5, 1, 2, 4}
    row scales  {0.25, 0.5, 1, 2}

A term weight * row_scale * feature is a multiple of UNIT = 1/8 of magnitude <= 64, i.e. <= MAX_TERM_UNITS = 512
units.  A partial sum of a list of l rows is below 2^24 units (the integers fp32 holds exactly) as long as
l * 512 < 2^24, i.e. l < 32768: ``assert_exact`` checks that bound on every case handed out.

The references are plain torch on the CPU in int64 (scale by 8, sum, scale back).  bf16 outputs are the exact sum
rounded to bf16 ONCE, round-to-nearest-even.
"""
import torch

UNIT_INV = 8                    # terms are multiples of 1/8
FEATURE_MAX = 8
WEIGHTS = (0.5, 1.0, 2.0, 4.0)
ROW_SCALES = (0.25, 0.5, 1.0, 2.0)
MAX_TERM_UNITS = int(FEATURE_MAX * max(WEIGHTS) * max(ROW_SCALES) * UNIT_INV)   # 512
EXACT_LIMIT = 1 << 24           # every integer of magnitude <= 2^24 is an fp32 number
MAX_LIST = EXACT_LIMIT // MAX_TERM_UNITS    # 32768: list lengths must stay BELOW this

# list lengths at the loop edges of the reduce kernels (rows per inner trip G*U in {2..64}, 64-row index batches,
# VPL = 2 / 4 rows) -- the chunk-dependent ones are added by ``standard_lengths``
BASE_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193)
ENDS = ("empty", "one", "split")


def assert_exact(max_list_len: int, max_term_units: int = MAX_TERM_UNITS):
    """the condition under which 'bitwise' is a fair demand: no partial sum can leave the exact integers of fp32"""
    assert int(max_list_len) * int(max_term_units) < EXACT_LIMIT, \
        f"list of {max_list_len} rows x {max_term_units} units is not exactly summable in fp32"


# ------------------------------------------------------------------ value grids
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def features(rows: int, F: int, seed: int, dtype=torch.float32) -> torch.Tensor:
    g = _gen(seed)
    mag = torch.randint(1, FEATURE_MAX + 1, (rows, F), generator=g)
    sign = torch.randint(0, 2, (rows, F), generator=g) * 2 - 1
    return (mag * sign).to(dtype)


def _pick(values, n, seed):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), (n,), generator=_gen(seed))]


def weights(n: int, seed: int) -> torch.Tensor:
    return _pick(WEIGHTS, n, seed)


def row_scales(n: int, seed: int) -> torch.Tensor:
    return _pick(ROW_SCALES, n, seed)


# ------------------------------------------------------------------ indices with prescribed list lengths
def default_chunk(n_rows: int) -> int:
    """the chunk ``hgnn_plan_dims`` picks for chunk <= 0"""
    share = n_rows // 4096 // 4
    return 32 if share < 32 else (512 if share > 512 else share)


def standard_lengths(chunk: int, ends: str, seed: int = 0):
    """the standard list-length set for a plan with chunk ``chunk``: BASE_LENGTHS, the chunk edges
    c-1, c, c+1, 2c-1, 2c, 2c+1, 3c+1, 64c+1 (more than 64 partial rows), two runs of consecutive empty destinations,
    in seeded random order, with the FIRST and the LAST destination both empty / one row / split (``ends``)."""
    c = int(chunk)
    assert c >= 1 and ends in ENDS
    body = list(BASE_LENGTHS) + [c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 3 * c + 1, 64 * c + 1]
    order = torch.randperm(len(body), generator=_gen(seed)).tolist()
    body = [body[i] for i in order]
    cut = len(body) // 3
    body = body[:cut] + [0, 0, 0] + body[cut:2 * cut] + [0, 0] + body[2 * cut:]
    end = {"empty": 0, "one": 1, "split": 2 * c + 1}[ends]
    lengths = [end] + body + [end]
    assert_exact(max(lengths))
    return lengths


def lengths_filling(total: int, pattern=(0, 1, 2, 3, 5, 8, 1, 20, 0, 0, 4, 16)):
    """list lengths cycling through ``pattern`` until they sum to ``total`` (the last one is trimmed)"""
    out, left, i = [], int(total), 0
    while left > 0:
        n = min(pattern[i % len(pattern)], left)
        out.append(n)
        left -= n
        i += 1
    return out


def index_with_lengths(lengths, seed: int):
    """(shuffled, sorted) int64 indices over N = len(lengths) destinations: destination d has exactly lengths[d]
    rows.  ``sorted`` is the same multiset in destination order, ``shuffled`` a seeded permutation of it."""
    n = torch.tensor(list(lengths), dtype=torch.int64)
    srt = torch.repeat_interleave(torch.arange(len(lengths), dtype=torch.int64), n)
    shuf = srt[torch.randperm(srt.numel(), generator=_gen(seed))] if srt.numel() else srt.clone()
    return shuf.contiguous(), srt.contiguous()


def plan_reference(lengths, chunk: int):
    """closed form of what ``hgnn_plan_build`` must produce for lists of these lengths: rowptr, the work items
    (begin, end, dst, target; target >= 0 is an output row, ~target a partial row), the split destinations with the
    first partial row of each (+ the total), and the counts."""
    c = int(chunk)
    rowptr = [0]
    for n in lengths:
        rowptr.append(rowptr[-1] + int(n))
    wb, we, wd, wt, sd, sp = [], [], [], [], [], []
    n_partial = 0
    for d, deg in enumerate(lengths):
        deg = int(deg)
        split = deg > c
        nch = -(-deg // c) if split else 1
        ln = -(-deg // nch)
        if split:
            sd.append(d)
            sp.append(n_partial)
        for k in range(nch):
            b = min(rowptr[d] + k * ln, rowptr[d + 1])
            wb.append(b)
            we.append(min(b + ln, rowptr[d + 1]))
            wd.append(d)
            wt.append(~(n_partial + k) if split else d)
        if split:
            n_partial += nch
    sp.append(n_partial)
    return dict(rowptr=rowptr, wi_begin=wb, wi_end=we, wi_dst=wd, wi_target=wt, split_dst=sd, split_pbegin=sp,
                work=len(wb), split=len(sd), partial=n_partial, valid=rowptr[-1])


# ------------------------------------------------------------------ exact references (CPU, int64)
def _units(t: torch.Tensor) -> torch.Tensor:
    """t (fp64, multiples of 1/8) as int64 units; asserts that nothing was lost"""
    u = (t * UNIT_INV).round()
    assert torch.equal(u / UNIT_INV, t), "value off the 1/8 grid"
    return u.long()


def _finish(units: torch.Tensor, dtype) -> torch.Tensor:
    assert units.numel() == 0 or int(units.abs().max()) <= EXACT_LIMIT, "sum leaves the exact range of fp32"
    f = (units.double() / UNIT_INV).float()          # exact: |units| <= 2^24
    return f if dtype == torch.float32 else f.to(dtype)   # bf16: ONE round-to-nearest-even


def edge_terms(src, weight=None, gather=None, row_scale=None) -> torch.Tensor:
    """fp64 [M, F]: weight[e] * row_scale[g[e]] * src[g[e]]  (g = identity without ``gather``)"""
    t = src.double()
    if row_scale is not None:
        t = t * row_scale.double().view(-1, 1)
    if gather is not None:
        t = t[gather]
    if weight is not None:
        t = t * weight.double().view(-1, 1)
    return t


def scatter_ref(src, index, dim_size, weight=None, gather=None, row_scale=None, out_dtype=None) -> torch.Tensor:
    """out[d] = sum_{e: index[e]=d} weight[e] * row_scale[g[e]] * src[g[e]], summed in int64"""
    u = _units(edge_terms(src, weight, gather, row_scale))
    if index.numel():
        assert_exact(int(torch.bincount(index, minlength=1).max()), int(u.abs().max()) if u.numel() else 0)
    out = torch.zeros((int(dim_size), src.shape[1]), dtype=torch.int64).index_add_(0, index, u)
    return _finish(out, out_dtype or src.dtype)


def gather_ref(table, idx, weight=None, row_scale=None) -> torch.Tensor:
    """out[e] = weight[e] * row_scale[idx[e]] * table[idx[e]]; a negative (padding) idx gives a zero row"""
    ok = idx >= 0
    safe = idx.clamp_min(0)
    t = edge_terms(table, weight, safe, row_scale) * ok.double().view(-1, 1)
    return _finish(_units(t), table.dtype)


def spread_ref(table, index, weight=None) -> torch.Tensor:
    """out[e] = weight[e] * table[index[e]]: the gradient of scatter_add w.r.t. src"""
    return gather_ref(table, index, weight)


def edge_dot_ref(A, ai, B, bi) -> torch.Tensor:
    """out[e] = <A[ai[e]], B[bi[e]]> in int64 (integer-valued rows); identity index for None; negative -> 0"""
    M = int(ai.numel() if ai is not None else bi.numel() if bi is not None else min(A.shape[0], B.shape[0]))
    ia = torch.arange(M) if ai is None else ai
    ib = torch.arange(M) if bi is None else bi
    ok = (ia >= 0) & (ib >= 0)
    a, b = A.double()[ia.clamp_min(0)], B.double()[ib.clamp_min(0)]
    assert torch.equal(a.round(), a) and torch.equal(b.round(), b), "edge_dot_ref wants integer-valued rows"
    s = (a.long() * b.long()).abs().sum(1)
    assert s.numel() == 0 or int(s.max()) < EXACT_LIMIT, "dot product leaves the exact range of fp32"
    d = (a.long() * b.long()).sum(1) * ok.long()
    return d.double().float()


# ------------------------------------------------------------------ bf16 rounding, bit level
def bf16_bits_rne(x: torch.Tensor) -> torch.Tensor:
    """int16 bit patterns of fp32 ``x`` rounded to bf16, round-to-nearest-even, by integer arithmetic on the fp32
    pattern (finite inputs): add 0x7FFF plus the lowest kept bit, keep the upper half."""
    bits = x.contiguous().view(torch.int32).long() & 0xFFFFFFFF
    lsb = (bits >> 16) & 1
    up = ((bits + 0x7FFF + lsb) >> 16) & 0xFFFF
    return torch.where(up >= 0x8000, up - 0x10000, up).to(torch.int16)
