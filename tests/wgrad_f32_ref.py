"""Exact-arithmetic reference for hgnn_wgrad_f32, the fp32-MFMA weight gradient of the default training route
(csrc/wgrad_f32.hip), modelled on tests/gemm_ref.py and built on it.

* ``shape_for`` restates wgf::shape_for: tile, slices and rows per slice are a pure function of (M, Ho, Hi); KT = 16
  rows per step.  ``m_edges`` is gemm_ref.m_edges on this function and this KT.
* Grids: gemm_ref's small / mid_a / mid_b / mid_both, and one new pair.  wide_a / wide_b: one operand holds odd
  integers +-(2^17 + 2j + 1) < 2^18 -- 18 significant bits with the lowest one set, j restricted so that the remainder
  after bf16 has nine significant bits: neither bf16 (8 bits) nor hi + mid holds the value -- at no more than WIDE_NNZ = 15 positions along the reduction (always its first,
  middle and last position), the partner is dense +-1.  15 * 2^18 < 2^22: ``gemm_ref.assert_exact`` holds, and every
  kernel that forms exact fp32 products is bit-equal to the int64 product.  A split-bf16 kernel cannot be.
* ``emulate``: the kernel's own order in float32 on the CPU -- per slice a chain over its rows with one rounding per
  product-add (the fp32 MFMA is a k-ordered fmaf chain), then the partials in k_wgrad_f32_reduce's four-chain order.
* ``mutants``: subtly wrong weight gradients that every case of tests/test_gpu_wgrad_f32.py must tell from the truth.
* ``bar``: the a-priori element-wise error bound of that order for arbitrary data.
"""
import torch

import gemm_ref as G

KT = 16                          # rows per step of k_wgrad_f32 = four v_mfma_f32_16x16x4_f32 along k
MAX_WIDTH = 1024
WIDE_NNZ = 15
WIDE_MAX = 1 << 18
GRIDS = G.GRIDS + ("wide_a", "wide_b")
WIDE = ("wide_a", "wide_b")

# one partial and one full shape per instantiation, plus the widest
SHAPES = ((8, 24), (24, 264), (128, 128), (520, 8), (256, 128), (264, 136), (512, 256), (1024, 512))
FULL_SHAPES = ((128, 128), (256, 128), (512, 256))
TILE_OF = {(8, 24): (128, 128), (24, 264): (128, 128), (128, 128): (128, 128), (520, 8): (256, 128),
           (256, 128): (256, 128), (264, 136): (256, 256), (512, 256): (256, 256), (1024, 512): (256, 256)}
RANDOM_CASES = ((256, 128, 5000), (512, 256, 70001))


def cdiv(a, b):
    return G.cdiv(a, b)


# ------------------------------------------------------------------ wgf::shape_for, restated (wgrad_f32.hip)
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
    return shape_for(M, Ho, Hi)["slices"] * Ho * Hi * 4


def chain_and_slices(M: int, Ho: int, Hi: int):
    """(L, S): the longest fmaf chain of one slice and the slice count"""
    r = slice_ranges(M, Ho, Hi)
    return max(e - b for b, e in r), len(r)


def _first_m(Ho, Hi, pred, lo=KT * 8 + 1, hi=8192):
    for M in range(lo, hi):
        if pred(slice_ranges(M, Ho, Hi), shape_for(M, Ho, Hi)):
            return M
    raise AssertionError(f"no M in [{lo}, {hi}) for ({Ho}, {Hi})")


ONE_SLICE = KT * 8               # up to this many rows there is one slice


def m_edges(Ho: int, Hi: int):
    """the M values at the edges of the split-K decomposition: none / one row, a 16-row step and its neighbours, the 128
    rows up to which there is one slice and their neighbours, a last slice of exactly 1 row, of exactly one step, a
    full last slice (several slices each), and the smallest M with >= 5 slices (four reduce chains + the remainder)"""
    last = lambda r: r[-1][1] - r[-1][0]
    one = _first_m(Ho, Hi, lambda r, s: len(r) >= 2 and last(r) == 1)
    step = _first_m(Ho, Hi, lambda r, s: len(r) >= 2 and last(r) == KT)
    full = _first_m(Ho, Hi, lambda r, s: len(r) >= 2 and last(r) == s["rows_per_slice"])
    five = _first_m(Ho, Hi, lambda r, s: len(r) >= 5)
    return sorted({0, 1, KT - 1, KT, KT + 1, ONE_SLICE - 1, ONE_SLICE, ONE_SLICE + 1, one, step, full, five})


# ------------------------------------------------------------------ grids
def wide_sparse(n: int, cols: int, seed: int) -> torch.Tensor:
    """[n, cols]: odd +-(2^17 + 2j + 1) at no more than WIDE_NNZ positions down each column (the reduction), always at
    its first, middle and last position; 0 elsewhere"""
    g = torch.Generator().manual_seed(int(seed))
    # 2j + 1 = 1024 q + r with r odd in [257, 767]: bf16 (ulp 1024 here) leaves a remainder of 257 .. 511 in magnitude,
    # nine significant bits with the lowest set, which the mid part (8 bits) cannot hold either.  (An odd remainder
    # below 256 WOULD fit: hi + mid is exact for about half of all odd 18-bit integers.)
    val = (1 << 17) + 1024 * torch.randint(0, 128, (n, cols), generator=g) \
        + 257 + 2 * torch.randint(0, 256, (n, cols), generator=g)
    val = val * (torch.randint(0, 2, (n, cols), generator=g) * 2 - 1)
    rank = torch.rand((n, cols), generator=g).argsort(0).argsort(0)
    keep = rank < WIDE_NNZ - 3
    keep[0] = True
    keep[n // 2] = True
    keep[n - 1] = True
    assert int(keep.sum(0).max()) <= WIDE_NNZ and int(val.abs().max()) < WIDE_MAX
    return (val * keep).float()


def dense_pm1(n: int, cols: int, seed: int) -> torch.Tensor:
    return (torch.randint(0, 2, (n, cols), generator=torch.Generator().manual_seed(int(seed))) * 2 - 1).float()


def operands(grid: str, M: int, Ho: int, Hi: int, seed: int):
    """dz [M, Ho], rows [M, Hi] (fp32, CPU) of one grid, inside the exactness bound"""
    assert grid in GRIDS
    if grid not in WIDE:
        return G.wgrad_operands(grid, M, Ho, Hi, seed)
    if M == 0:
        return torch.zeros(0, Ho), torch.zeros(0, Hi)
    G.assert_exact(WIDE_NNZ, WIDE_MAX)
    if grid == "wide_a":
        return wide_sparse(M, Ho, seed), dense_pm1(M, Hi, seed + 1)
    return dense_pm1(M, Ho, seed), wide_sparse(M, Hi, seed + 1)


# seeds moved on until every mutant of tests/test_wgrad_f32_ref.py is caught on the case (at M = 1 the two +-1 columns
# that the column-swap mutant exchanges, or a 16 x 16 tile and its transpose, can coincide)
SEED_BUMP = {("wide_a", 1, 8, 24): 1, ("wide_a", 1, 24, 264): 5, ("mid_both", 1, 128, 128): 4,
             ("wide_a", 1, 264, 136): 2}


def seed_of(grid, M, Ho, Hi):
    return 2000003 * GRIDS.index(grid) + 7919 * M + 31 * Ho + Hi + 100 * SEED_BUMP.get((grid, M, Ho, Hi), 0)


def grids_of(shape):
    return GRIDS if tuple(shape) in FULL_SHAPES else ("small",) + WIDE


def integer_cases():
    """every (grid, M, Ho, Hi) that tests/test_gpu_wgrad_f32.py hands to the kernel"""
    for Ho, Hi in SHAPES:
        for grid in grids_of((Ho, Hi)):
            for M in m_edges(Ho, Hi):
                yield grid, M, Ho, Hi


def ref(dz, rows, int64=False):
    return G.wgrad_ref(dz, rows, int64)[0]


# ------------------------------------------------------------------ the kernel's order, in float32
def reduce_order(partials: torch.Tensor) -> torch.Tensor:
    """k_wgrad_f32_reduce: four chains over the slices k = 0, 1, 2, 3 mod 4, the remainder on chain 0, then
    (s0 + s1) + (s2 + s3); float32 throughout"""
    S = partials.shape[0]
    s = [torch.zeros_like(partials[0]) for _ in range(4)]
    k = 0
    while k + 3 < S:
        for c in range(4):
            s[c] = s[c] + partials[k + c]
        k += 4
    while k < S:
        s[0] = s[0] + partials[k]
        k += 1
    return (s[0] + s[1]) + (s[2] + s[3])


def emulate(dz: torch.Tensor, rows: torch.Tensor, ho=None, hi=None) -> torch.Tensor:
    """float32 result of hgnn_wgrad_f32's order (optionally of the output rows ``ho`` / columns ``hi`` only: the
    elements are independent).  One rounding per product-add: the product of two fp32 values is exact in float64, the
    sum is rounded to float64 and then to float32 -- an fmaf up to double rounding, and exactly an fmaf on the integer
    grids.  All slices advance together, one row of each per iteration; rows past the end are zeros (acc unchanged)."""
    M, Ho, Hi = dz.shape[0], dz.shape[1], rows.shape[1]
    sh = shape_for(M, Ho, Hi)
    S, rps = sh["slices"], sh["rows_per_slice"]
    a = dz.float() if ho is None else dz.float()[:, ho]
    b = rows.float() if hi is None else rows.float()[:, hi]
    pad = S * rps - M
    a = torch.cat([a, a.new_zeros(pad, a.shape[1])]).view(S, rps, -1).double()
    b = torch.cat([b, b.new_zeros(pad, b.shape[1])]).view(S, rps, -1).double()
    acc = torch.zeros(S, a.shape[2], b.shape[2], dtype=torch.float32)
    for r in range(min(rps, M)):
        acc = (acc.double() + a[:, r, :, None] * b[:, r, None, :]).float()
    return reduce_order(acc)


def bar(dz, rows, ho=None, hi=None) -> torch.Tensor:
    """(L + S + 2) * 2^-24 * (|dz|^T |rows|) in float64: the a-priori bound of a length-L fp32 chain followed by S adds
    (one half-ulp relative error per operation, first order, and 2 for the second-order terms); no measured constant"""
    L, S = chain_and_slices(dz.shape[0], dz.shape[1], rows.shape[1])
    a = dz.double().abs() if ho is None else dz.double().abs()[:, ho]
    b = rows.double().abs() if hi is None else rows.double().abs()[:, hi]
    return (L + S + 2) * 2.0 ** -24 * (a.t() @ b)


# ------------------------------------------------------------------ mutants
MUTANTS = ("dropped_row", "duplicated_row", "last_slice_skipped", "last_step_skipped", "columns_swapped",
           "tile_transposed")
WIDE_MUTANTS = ("split3_three_products", "split3_four_products")


def mutants(dz, rows, grid=None):
    """name -> float64 result of a subtly wrong split-K weight gradient (none at M == 0)"""
    M, Ho, Hi = dz.shape[0], dz.shape[1], rows.shape[1]
    if M == 0:
        return {}
    r0 = ref(dz, rows)
    keep = torch.ones(M, dtype=torch.bool)
    r = M // 2
    keep[r] = False
    out = {"dropped_row": ref(dz[keep], rows[keep]),
           "duplicated_row": r0 + torch.outer(dz[r].double(), rows[r].double())}
    b, e = slice_ranges(M, Ho, Hi)[-1]
    out["last_slice_skipped"] = ref(dz[:b], rows[:b])
    b = b + KT * ((e - b - 1) // KT)
    out["last_step_skipped"] = ref(dz[:b], rows[:b])
    c = Hi // 2 - 1
    sw = r0.clone()
    sw[:, [c, c + 1]] = r0[:, [c + 1, c]]
    out["columns_swapped"] = sw
    t = min(16, Ho, Hi)                    # the 16 x 16 MFMA tile (8 x 8 of it where a width is 8)
    tr = r0.clone()
    tr[:t, :t] = r0[:t, :t].t()
    out["tile_transposed"] = tr
    if grid in WIDE:
        out["split3_three_products"] = G.split3_ref(dz.t(), rows, four=False)
        out["split3_four_products"] = G.split3_ref(dz.t(), rows, four=True)
    return out
