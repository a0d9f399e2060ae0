"""Exact-arithmetic reference for the matrix kernels of the training path: the split-K weight gradients
(hgnn_wgrad_bf16, hgnn_wgrad_f32_split3), the data gradient of the bf16 backward layer (input form of
hgnn_mlp_backward_layer_bf16) and the split-bf16 fp32 GEMMs (hgnn_linear_f32_split3, hgnn_project_f32_split3).

Modelled on tests/rows_ref.py: every operand comes from a small integer grid, so every product and every partial sum
-- in ANY order -- is an integer multiple of one unit (1.0) of magnitude below EXACT_LIMIT = 2^22 units, and a
kernel's fp32 result must equal the integer reference bit for bit.  2^22 is TWO BITS under the 2^24 that fp32 holds
exactly and that rows_ref uses: how v_mfma_f32_16x16x32_bf16 aligns the 32 terms of its dot product before it adds
them to the accumulator has not been measured here; the margin keeps "bitwise" from depending on whether the
instruction carries guard bits below the accumulator's last place.  ``assert_exact`` guards every case handed out.

Grids (operand pairs a [M, K] . b [K, N], reduction over K; for the weight gradients a = dz^T):

    small      both operands integers +-{1..8}, never 0: exact in bf16; 64 * n < 2^22 terms allows n <= 65,535
    mid_a      a: odd integers of 9-10 significant bits (+-{257..1023}; 9 bits, +-{257..511}, for long reductions), so
               bf16(x) != x and x = hi + mid exactly with mid = +-1;  b: integers +-{1..4}      -> isolates mid.hi
    mid_b      the mirror image                                                                   -> isolates hi.mid
    mid_both   a: +-257 * 2^k, k in {0, 1} (hi = 256 * 2^k, mid = 2^k), at most MID_BOTH_NNZ non-zeros along the
               reduction (zeros are allowed here and only here; the first, the middle and the last position of every
               reduction are always non-zero);  b: +-257, dense                                            -> isolates mid.mid

References are float64 / int64 matmuls (exact: everything is an integer below 2^22); on the device the same
float64 expressions are used.  tests/test_gemm_ref.py proves them, and proves with mutants of the reference's own
arithmetic that every case of tests/test_gpu_gemm_exact.py would turn red on a subtly wrong kernel.
"""
import torch

import rows_ref as R

EXACT_LIMIT = 1 << 22           # two bits under fp32's 2^24: see the module docstring
KT = 32                         # rows per step of the weight-gradient kernel = k depth of one bf16 MFMA
SMALL_MAX = 8
PARTNER_MAX = 4                 # |partner| of a mid_* operand
MID_BOTH_NNZ = 16               # non-zero terms per dot product on mid_both
MID_BOTH_TERM = (257 * 2) * 257  # 132,098 units
GRIDS = ("small", "mid_a", "mid_b", "mid_both")


def assert_exact(n_terms: int, max_term_units: int):
    """the condition under which 'bitwise' is a fair demand: no partial sum of ``n_terms`` terms of at most
    ``max_term_units`` units each can reach 2^22 units"""
    assert int(n_terms) * int(max_term_units) < EXACT_LIMIT, \
        f"{n_terms} terms x {max_term_units} units is not inside the 2^22 exactness bound"


def cdiv(a: int, b: int) -> int:
    return -(-int(a) // int(b))


# ------------------------------------------------------------------ value grids
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def small(rows: int, cols: int, seed: int, max_mag: int = SMALL_MAX) -> torch.Tensor:
    g = _gen(seed)
    mag = torch.randint(1, max_mag + 1, (rows, cols), generator=g)
    sign = torch.randint(0, 2, (rows, cols), generator=g) * 2 - 1
    return (mag * sign).float()


def mid(rows: int, cols: int, seed: int, bits: int = 10) -> torch.Tensor:
    """odd integers +-{257 .. 2^bits - 1}: 9 to ``bits`` significant bits with the lowest one set, so the bf16 part
    (8 bits) differs from the value and the remainder is +-1"""
    assert bits in (9, 10)
    g = _gen(seed)
    m = 2 * torch.randint(128, 1 << (bits - 1), (rows, cols), generator=g) + 1
    sign = torch.randint(0, 2, (rows, cols), generator=g) * 2 - 1
    return (m * sign).float()


def both_dense(rows: int, cols: int, seed: int) -> torch.Tensor:
    return (257 * (torch.randint(0, 2, (rows, cols), generator=_gen(seed)) * 2 - 1)).float()


def both_sparse(rows: int, cols: int, seed: int, dim: int) -> torch.Tensor:
    """+-257 * 2^{0,1} at no more than MID_BOTH_NNZ positions along ``dim`` (the reduction), always at its first,
    middle and last position; 0 elsewhere"""
    g = _gen(seed)
    if dim == 1:
        return both_sparse(cols, rows, seed, 0).t().contiguous()
    val = 257 * (torch.randint(0, 2, (rows, cols), generator=g) * 2 - 1) * (1 << torch.randint(0, 2, (rows, cols), generator=g))
    rank = torch.rand((rows, cols), generator=g).argsort(0).argsort(0)         # a random permutation down each column
    keep = rank < MID_BOTH_NNZ - 3
    keep[0] = True
    keep[rows // 2] = True
    keep[rows - 1] = True
    return (val * keep).float()


def split(x: torch.Tensor):
    """(hi, mid) as the kernels form them: hi = bf16(x), mid = bf16(x - hi), both returned in float64"""
    x = x.float()
    hi = x.bfloat16().float()
    md = (x - hi).bfloat16().float()
    return hi.double(), md.double()


def operands(grid: str, M: int, K: int, N: int, seed: int):
    """a [M, K], b [K, N] (fp32, CPU) of one grid, checked against the exactness bound"""
    assert grid in GRIDS
    if grid == "small":
        assert_exact(K, SMALL_MAX * SMALL_MAX)
        return small(M, K, seed), small(K, N, seed + 1)
    if grid == "mid_both":
        assert_exact(MID_BOTH_NNZ, MID_BOTH_TERM)
        return both_sparse(M, K, seed, 1), both_dense(K, N, seed + 1)
    bits = 10 if K * (1 << 10) * PARTNER_MAX < EXACT_LIMIT else 9
    assert_exact(K, (1 << bits) * PARTNER_MAX)       # |hi| can round up to 2^bits
    if grid == "mid_a":
        return mid(M, K, seed, bits), small(K, N, seed + 1, PARTNER_MAX)
    return small(M, K, seed, PARTNER_MAX), mid(K, N, seed + 1, bits)


def wgrad_operands(grid: str, M: int, Ho: int, Hi: int, seed: int):
    """dz [M, Ho], rows [M, Hi]: the reduction runs over the M rows (a = dz^T)"""
    a, b = operands(grid, Ho, M, Hi, seed) if M else (torch.zeros(Ho, 0), torch.zeros(0, Hi))
    return a.t().contiguous(), b.contiguous()


# ------------------------------------------------------------------ references (float64; int64 on request, CPU only)
def _mm(a, b, int64=False):
    if int64:
        assert torch.equal(a.double().round(), a.double()) and torch.equal(b.double().round(), b.double())
        return (a.double().long() @ b.double().long()).double()
    return a.double() @ b.double()


def wgrad_ref(dz, rows, int64=False):
    """(dz^T . rows, dz.sum(0)) in float64"""
    return _mm(dz.t(), rows, int64), dz.double().sum(0)


def split3_ref(a, b, four: bool):
    """a . b as the sum of exactly the products a split-bf16 kernel forms: hi.hi + hi.mid + mid.hi (+ mid.mid)"""
    ah, am = split(a)
    bh, bm = split(b)
    s = ah @ bh + ah @ bm + am @ bh
    return s + am @ bm if four else s


def round_bf16_bits(s: torch.Tensor, truncate: bool = False) -> torch.Tensor:
    """int16 bf16 patterns of the float64 integers ``s`` (|s| < 2^24: exact in fp32), rounded ONCE to nearest even"""
    f = s.float()
    assert torch.equal(f.double(), s)
    if truncate:
        return (f.contiguous().view(torch.int32) >> 16).to(torch.int16)
    return R.bf16_bits_rne(f)


def bits_to_float(bits: torch.Tensor) -> torch.Tensor:
    return (bits.to(torch.int32) << 16).view(torch.float32)


def dgrad_ref(dz, W, skip=None, int64=False) -> torch.Tensor:
    """dz . W (+ skip), rounded to bf16 once: int16 bit patterns"""
    s = _mm(dz, W, int64)
    if skip is not None:
        s = s + skip.double()
    return round_bf16_bits(s)


# ------------------------------------------------------------------ wg::shape_for, restated (wgrad_bf16.hip)
def shape_for(M: int, Ho: int, Hi: int) -> dict:
    to = 256 if Ho > 128 else 128
    ti = 256 if (Ho > 128 and Hi > 128) else 128
    tiles = cdiv(Ho, to) * cdiv(Hi, ti)
    want = cdiv(512, tiles)
    want = max(1, min(want, cdiv(M, KT * 8)))
    rps = max(KT, cdiv(cdiv(M, want), KT) * KT)
    slices = cdiv(M if M > 0 else 1, rps)
    return dict(to=to, ti=ti, tiles=tiles, rows_per_slice=rps, slices=slices)


def slice_ranges(M: int, Ho: int, Hi: int):
    s = shape_for(M, Ho, Hi)
    return [(k * s["rows_per_slice"], min(M, (k + 1) * s["rows_per_slice"])) for k in range(s["slices"])]


def workspace_bytes(M: int, Ho: int, Hi: int) -> int:
    return shape_for(M, Ho, Hi)["slices"] * (Ho * Hi + Ho) * 4


def _first_m(Ho, Hi, pred, lo=257, hi=8192):
    for M in range(lo, hi):
        r = slice_ranges(M, Ho, Hi)
        if pred(r, shape_for(M, Ho, Hi)):
            return M
    raise AssertionError(f"no M in [{lo}, {hi}) for ({Ho}, {Hi})")


def m_edges(Ho: int, Hi: int):
    """the M values at the edges of the split-K decomposition of a [Ho, Hi] gradient: none / one row, a 32-row step and
    its neighbours, the 256 rows below which there is one slice and their neighbours, a last slice of exactly 1 row,
    of exactly 32 rows, a full last slice (several slices each), and the smallest M with >= 5 slices (four reduce
    chains + the remainder loop)"""
    last = lambda r: r[-1][1] - r[-1][0]
    one = _first_m(Ho, Hi, lambda r, s: len(r) >= 2 and last(r) == 1)
    step = _first_m(Ho, Hi, lambda r, s: len(r) >= 2 and last(r) == KT)
    full = _first_m(Ho, Hi, lambda r, s: len(r) >= 2 and last(r) == s["rows_per_slice"])
    five = _first_m(Ho, Hi, lambda r, s: len(r) >= 5)
    return sorted({0, 1, 31, 32, 33, 255, 256, 257, one, step, full, five})


WGRAD_SHAPES = (   # (Ho, Hi) -> the (TO, TI) instantiation it reaches
    ((8, 24), (128, 128)), ((64, 64), (128, 128)), ((128, 128), (128, 128)), ((128, 512), (128, 128)),
    ((24, 264), (128, 128)),
    ((136, 128), (256, 128)), ((256, 128), (256, 128)), ((520, 8), (256, 128)),
    ((264, 136), (256, 256)), ((512, 256), (256, 256)),
)
# thinned for the fp32 split kernel: one partial and one full shape per instantiation
WGRAD_S3_SHAPES = ((24, 264), (128, 128), (520, 8), (256, 128), (264, 136), (512, 256))


# seeds moved on until every mutant of tests/test_gemm_ref.py is caught on the case (at M = 1 the two columns that the
# column-swap mutant exchanges can coincide)
SEED_BUMP = {("small", 1, 128, 512): 1, ("mid_a", 1, 128, 128): 1, ("mid_both", 1, 128, 128): 1,
             ("mid_both", 1, 520, 8): 1, ("mid_both", 1, 256, 128): 1, ("mid_both", 1, 264, 136): 3,
             ("mid_both", 1, 512, 256): 1}


def wgrad_seed(grid, M, Ho, Hi):
    return 1000003 * GRIDS.index(grid) + 7919 * M + 31 * Ho + Hi + 100 * SEED_BUMP.get((grid, M, Ho, Hi), 0)


# ------------------------------------------------------------------ the row-tile kernels' cases
DGRAD_N = (128, 256, 512)
DGRAD_K = (128, 256, 1024)
TILE_M = (1, 63, 64, 65, 193)           # the 64-row tile: one row, its edges, three tiles + one row
LINEAR_N = (256, 512)
LINEAR_K = (128, 256, 512)


def dgrad_operands(M, K, N, seed, with_skip):
    """dz [M, K], W [K, N] (both bf16-exact integers), skip [M, N] or None"""
    assert_exact(K + 1, SMALL_MAX * SMALL_MAX)
    return small(M, K, seed), small(K, N, seed + 1), (small(M, N, seed + 2) if with_skip else None)


def dgrad_seed(M, K, N):
    return 104729 + 7919 * M + 31 * K + N


def linear_seed(grid, M, K, N):
    return 15485863 + 1000003 * GRIDS.index(grid) + 7919 * M + 31 * K + N


# ------------------------------------------------------------------ persistent tile loops
BWD_LAYER_BLOCKS = 512      # HGNN_MLP_BWD_BLOCKS: k_mlp_bwd_layer's grid does not depend on the device


def trip_rows(kernel: str, cus: int) -> int:
    """rows one trip of a persistent kernel's tile loop covers = workgroups x tile rows.  The split-bf16 forward runs
    ``cus`` x residency workgroups: two per CU at latent 128 (74 KB of LDS each), one at latent 256 on either tile."""
    return {"bwd_layer": BWD_LAYER_BLOCKS * 64,
            "split3_l128": cus * 2 * 64,
            "split3_l256_rows64": cus * 64,
            "split3_l256_rows128": cus * 128}[kernel]


def trip_first_row(kernel: str, t: int, cus: int) -> int:
    return t * trip_rows(kernel, cus)


def trip_of_row(kernel: str, row: int, cus: int):
    """(trip, workgroup, tile) that computes ``row``"""
    rows = 128 if kernel.endswith("rows128") else 64
    tile = row // rows
    wgs = trip_rows(kernel, cus) // rows
    return tile // wgs, tile % wgs, tile


# ------------------------------------------------------------------ mutants of the references' own arithmetic
def _last_step_begin(M, Ho, Hi):
    b, e = slice_ranges(M, Ho, Hi)[-1]
    return b + KT * ((e - b - 1) // KT)


def _colsum_shift(Ho, to):
    return to if Ho > to else (16 if Ho > 16 else 4)


def wgrad_mutants(dz, rows, s3_grid=None):
    """name -> (out, colsum) of a subtly wrong split-K weight gradient; ``s3_grid``: the fp32 split kernel on that
    grid (adds the mutants of its products)"""
    M, Ho, Hi = dz.shape[0], dz.shape[1], rows.shape[1]
    if M == 0:
        return {}
    ref, cs = wgrad_ref(dz, rows)
    sh = shape_for(M, Ho, Hi)
    keep = torch.ones(M, dtype=torch.bool)
    r = M // 2
    keep[r] = False
    out = {"dropped_row": wgrad_ref(dz[keep], rows[keep]),
           "duplicated_row": (ref + torch.outer(dz[r].double(), rows[r].double()), cs + dz[r].double())}
    b = slice_ranges(M, Ho, Hi)[-1][0]
    out["last_slice_skipped"] = wgrad_ref(dz[:b], rows[:b])
    b = _last_step_begin(M, Ho, Hi)
    out["last_step_skipped"] = wgrad_ref(dz[:b], rows[:b])
    c = Hi // 2 - 1
    sw = ref.clone()
    sw[:, [c, c + 1]] = ref[:, [c + 1, c]]
    out["columns_swapped"] = (sw, cs)
    out["colsum_wrong_tile"] = (ref, torch.roll(cs, _colsum_shift(Ho, sh["to"])))
    if s3_grid == "mid_both":
        out["mid_mid_dropped"] = (split3_ref(dz.t(), rows, four=False), cs)
    if s3_grid in ("mid_a", "mid_b"):
        b = KT * ((M - 1) // KT // 2)                      # one 32-row step
        ah, am = split(dz[b:b + KT].t())
        bh, bm = split(rows[b:b + KT])
        out["mid_hi_chunk_dropped"] = (ref - (am @ bh if s3_grid == "mid_a" else ah @ bm), cs)
    return out


def dgrad_mutants(dz, W, skip):
    """name -> int16 bits of a subtly wrong input-form backward layer"""
    K, N = W.shape
    k = K // 2
    keep = torch.ones(K, dtype=torch.bool)
    keep[k] = False
    s = _mm(dz, W)
    sk = skip.double() if skip is not None else 0
    c = N // 2 - 1
    perm = torch.arange(N)
    perm[c], perm[c + 1] = c + 1, c
    out = {"dropped_term": round_bf16_bits(_mm(dz[:, keep], W[keep]) + sk),
           "duplicated_term": round_bf16_bits(s + torch.outer(dz[:, k].double(), W[k].double()) + sk),
           "columns_swapped": round_bf16_bits(s[:, perm] + sk),
           "truncated": round_bf16_bits(s + sk, truncate=True)}
    if skip is not None:
        once = bits_to_float(round_bf16_bits(s)).double()
        out["skip_after_rounding"] = round_bf16_bits(once + sk)
    return out


def linear_mutants(a, b, grid, four):
    """name -> float64 result of a subtly wrong split-bf16 GEMM a . b (``four``: the kernel forms mid.mid too)"""
    K, N = b.shape
    k = K // 2
    keep = torch.ones(K, dtype=torch.bool)
    keep[k] = False
    ref = split3_ref(a, b, four)
    c = N // 2 - 1
    perm = torch.arange(N)
    perm[c], perm[c + 1] = c + 1, c
    out = {"dropped_term": split3_ref(a[:, keep], b[keep], four),
           "duplicated_term": ref + split3_ref(a[:, k:k + 1], b[k:k + 1], four),
           "columns_swapped": ref[:, perm]}
    if grid == "mid_both":
        out["mid_mid_dropped" if four else "mid_mid_added"] = split3_ref(a, b, not four)
    if grid in ("mid_a", "mid_b"):
        k0 = KT * (K // KT // 2)                           # one 32-wide k-chunk
        ah, am = split(a[:, k0:k0 + KT])
        bh, bm = split(b[k0:k0 + KT])
        out["mid_hi_chunk_dropped"] = ref - (am @ bh if grid == "mid_a" else ah @ bm)
    return out
