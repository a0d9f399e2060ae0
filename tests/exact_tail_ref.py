"""Exact-arithmetic reference for the last kernels of the exact fp32 step: hgnn_project_f32 (csrc/project_f32.hip) and
the narrow products hgnn_linear_narrow_f32 / hgnn_outer_narrow_f32 / hgnn_wgrad_narrow_f32 (csrc/narrow_f32.hip),
modelled on tests/wgrad_f32_ref.py and built on it and on tests/gemm_ref.py.

* Restated shape functions: ``project_tiles`` (features per pass, passes, 64-row tiles) and ``wgrad_shape`` (slices and
  rows per slice of the narrow weight gradient), ``linear_lanes`` (lanes that share a row of the narrow Linear).
* Grids: gemm_ref.small, and wide_a / wide_b built from wgrad_f32_ref.wide_sparse (odd 18-bit integers at no more than
  15 positions along the reduction against dense +-1): every partial sum is an integer below 2^22
  (``gemm_ref.assert_exact``), so any kernel that forms exact fp32 products in ANY order is bit-equal to the float64
  product (exact on integers below 2^53); no split-bf16 kernel can be.
* ``emulate_*``: each order contract of include/hgnn_hip.h in float32 on the CPU, one rounding per product-add.
* ``bar_*``: the a-priori element-wise bounds for arbitrary data, no measured constant.  A chain of n fmaf plus a adds
  errs by at most (n + a) half-ulps of the running magnitude to first order; + 2 covers the second-order terms.  Any
  order of the same products sits inside them.
* ``*_mutants``: subtly wrong results that every case the GPU tests hand to the kernels must tell from the truth.
"""
import functools

import torch

import gemm_ref as G
import wgrad_f32_ref as F

GRIDS = ("small", "wide_a", "wide_b")
WIDE = ("wide_a", "wide_b")
NB = 8                                  # narrow columns a thread of k_wgrad_narrow carries
BIG_M = 70001

PROJECT_SHAPES = ((16, 32), (32, 64), (48, 96), (128, 256), (256, 512), (512, 1024))      # (K, N)
NARROW_N = (1, 2, 3, 6, 8, 31, 32)
NARROW_K = (4, 16, 60, 64, 256, 1024)


def cdiv(a, b):
    return G.cdiv(a, b)


# ------------------------------------------------------------------ shape functions, restated
def pass_width(N: int) -> int:
    """prj::pass_width: features per pass"""
    return 16 if N <= 16 else 32 if N <= 32 else 64 if N <= 64 else 128 if N <= 128 else 256


def project_tiles(M: int, N: int, blocks: int) -> dict:
    fp = pass_width(N)
    return dict(pass_width=fp, passes=cdiv(N, fp), row_tiles=cdiv(M, 64), grid=(cdiv(M, 64), blocks * cdiv(N, fp)))


def project_m(N: int):
    """one row, the 16-row wave and the 64-row tile with their neighbours, two tiles and theirs, one row past a full
    grid of 64 tiles, and a size past 4096"""
    past = 64 * 64 + 1
    assert project_tiles(past - 1, N, 1)["row_tiles"] == 64 and project_tiles(past, N, 1)["row_tiles"] == 65
    return (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, past, 4099)


def linear_lanes(K: int) -> int:
    """nrw::linear_lanes: the largest power of two <= min(K / 4, 64)"""
    p = 1
    while p * 2 <= K // 4 and p * 2 <= 64:
        p *= 2
    return p


def wgrad_shape(M: int, n: int, K: int) -> dict:
    """nrw::wgrad_shape"""
    want = cdiv(131072, (K // 4) * cdiv(n, NB))
    want = max(1, min(want, cdiv(M, 64)))
    rps = max(16, cdiv(cdiv(M, want), 16) * 16)
    return dict(rows_per_slice=rps, slices=cdiv(M if M > 0 else 1, rps))


def wgrad_slices(M, n, K):
    s = wgrad_shape(M, n, K)
    return [(k * s["rows_per_slice"], min(M, (k + 1) * s["rows_per_slice"])) for k in range(s["slices"])]


def wgrad_workspace_bytes(M, n, K) -> int:
    return wgrad_shape(M, n, K)["slices"] * n * (K + 1) * 4


def chain_and_slices(M, n, K):
    r = wgrad_slices(M, n, K)
    return max(e - b for b, e in r), len(r)


def _first_m(n, K, pred, lo=65, hi=8192):
    for M in range(lo, hi):
        if pred(wgrad_slices(M, n, K), wgrad_shape(M, n, K)):
            return M
    raise AssertionError(f"no M in [{lo}, {hi}) for n={n} K={K}")


@functools.lru_cache(maxsize=None)
def narrow_m(n: int, K: int):
    """0, 1, the 64 rows up to which there is one slice and their neighbours, every slice edge (a last slice of exactly
    one row, of exactly 16 rows, a full last slice), the first M with >= 5 slices, and 70,001"""
    last = lambda r: r[-1][1] - r[-1][0]
    one = _first_m(n, K, lambda r, s: len(r) >= 2 and last(r) == 1)
    step = _first_m(n, K, lambda r, s: len(r) >= 2 and last(r) == 16)
    full = _first_m(n, K, lambda r, s: len(r) >= 2 and last(r) == s["rows_per_slice"])
    five = _first_m(n, K, lambda r, s: len(r) >= 5)
    return tuple(sorted({0, 1, 63, 64, 65, one, step, full, five, BIG_M}))


# ------------------------------------------------------------------ grids
def _pair(grid, red, a_cols, b_cols, seed, max_mag=G.SMALL_MAX):
    """a [red, a_cols], b [red, b_cols] whose products a[r, i] * b[r, j] summed over r stay exact"""
    if red == 0 or a_cols == 0 or b_cols == 0:
        return torch.zeros(red, a_cols), torch.zeros(red, b_cols)
    if grid == "small":
        G.assert_exact(red, max_mag * max_mag)
        return G.small(red, a_cols, seed, max_mag), G.small(red, b_cols, seed + 1, max_mag)
    assert F.WIDE_NNZ * F.WIDE_MAX + 64 < G.EXACT_LIMIT          # + 64: room for a small `add` / bias term
    if grid == "wide_a":
        return F.wide_sparse(red, a_cols, seed), F.dense_pm1(red, b_cols, seed + 1)
    return F.dense_pm1(red, a_cols, seed), F.wide_sparse(red, b_cols, seed + 1)


# seeds moved on until every mutant of tests/test_exact_tail_ref.py is caught on the case (with one row and one narrow
# column a handful of small integers can cancel, or two swapped columns coincide)
SEED_BUMP = {
    ("linear", "wide_b", 1, 2, 4): 1, ("wgrad", "wide_a", 1, 2, 4): 2, ("wgrad", "wide_a", 1, 31, 4): 1,
    ("wgrad", "wide_a", 1, 32, 4): 1, ("wgrad", "wide_a", 1, 1, 60): 1, ("wgrad", "wide_a", 1, 2, 60): 1,
    ("wgrad", "wide_a", 1, 3, 60): 3, ("wgrad", "wide_a", 1, 6, 60): 2, ("wgrad", "wide_a", 1, 8, 60): 2,
    ("wgrad", "wide_a", 1, 1, 64): 1, ("wgrad", "wide_a", 1, 3, 64): 2, ("wgrad", "wide_a", 1, 6, 64): 2,
    ("wgrad", "wide_a", 1, 8, 64): 1, ("wgrad", "wide_a", 1, 31, 64): 1, ("wgrad", "wide_a", 1, 2, 256): 3,
    ("wgrad", "wide_a", 1, 3, 256): 2, ("wgrad", "small", 1, 8, 256): 1, ("wgrad", "wide_a", 1, 32, 256): 1,
    ("wgrad", "wide_a", 1, 1, 1024): 1, ("wgrad", "wide_a", 1, 2, 1024): 1, ("wgrad", "wide_a", 1, 6, 1024): 1,
    ("wgrad", "wide_a", 1, 8, 1024): 3, ("wgrad", "wide_a", 1, 32, 1024): 4,
}


def seed_of(kind, grid, M, a, b):
    """``a``, ``b``: (K, N) of a projection, (n, K) of a narrow product"""
    return 3000017 * ("project", "linear", "outer", "wgrad").index(kind) + 2000003 * GRIDS.index(grid) \
        + 7919 * M + 31 * a + b + 100 * SEED_BUMP.get((kind, grid, M, a, b), 0)


def project_operands(grid, M, K, N, seed):
    """x [M, K], w0, w1 [N, K]: the reduction runs over K"""
    xt, w = _pair(grid, K, M, 2 * N, seed)
    return xt.t().contiguous(), w[:, :N].t().contiguous(), w[:, N:].t().contiguous()


@functools.lru_cache(maxsize=3)
def big_wide(kind, K):
    """the [70,001, K] wide-side array of the small grid, magnitudes of at most 4 (16 x 70,001 < 2^22).  It depends on
    the kernel and K alone, so the callers that walk n inside K make the three of a K once"""
    G.assert_exact(BIG_M, 4 * 4)
    return G.small(BIG_M, K, seed_of(kind, "small", BIG_M, 0, K), 4)


def linear_operands(grid, M, K, n, seed):
    """x [M, K], W [n, K], bias [n]"""
    if M == BIG_M:
        G.assert_exact(K, 4 * G.SMALL_MAX)
        return big_wide("linear", K), G.small(n, K, seed), G.small(1, n, seed + 2)[0]
    xt, wt = _pair(grid, K, M, n, seed)
    return xt.t().contiguous(), wt.t().contiguous(), G.small(1, n, seed + 2)[0]


def outer_operands(grid, M, n, K, seed):
    """y [M, n], W [n, K], add [M, K]: the reduction runs over n"""
    if M == BIG_M:
        return G.small(M, n, seed), G.small(n, K, seed + 1), big_wide("outer", K)
    yt, W = _pair(grid, n, M, K, seed)
    return yt.t().contiguous(), W.contiguous(), G.small(M, K, seed + 2) if M else torch.zeros(0, K)


def wgrad_operands(grid, M, n, K, seed):
    """y [M, n], x [M, K]: the reduction runs over the M rows"""
    if M == BIG_M:
        return G.small(M, n, seed, 4), big_wide("wgrad", K)
    return _pair(grid, M, n, K, seed)


def grids_at(M):
    """70,001 rows: the small grid only, with magnitudes of at most 4"""
    return ("small",) if M == BIG_M else GRIDS


# ------------------------------------------------------------------ float64 references (exact on the integer grids)
def project_ref(x, w):
    return x.double() @ w.double().t()


def linear_ref(x, W, bias=None):
    r = x.double() @ W.double().t()
    return r if bias is None else r + bias.double()


def outer_ref(y, W, add=None):
    r = y.double() @ W.double()
    return r if add is None else r + add.double()


def wgrad_ref(y, x):
    """(y^T x, column sums of y)"""
    return y.double().t() @ x.double(), y.double().sum(0)


# ------------------------------------------------------------------ the kernels' orders, in float32
def _fma(acc, a, b):
    """one rounding per product-add: the product of two fp32 values is exact in float64, the sum is rounded to float64
    and then to float32 -- an fmaf up to double rounding, and exactly an fmaf on the integer grids"""
    return (acc.double() + a.double() * b.double()).float()


def emulate_project(x, w):
    """acc = 0; acc = fmaf(x[r, k], w[h, k], acc) for k ascending"""
    x, w = x.float(), w.float()
    acc = torch.zeros(x.shape[0], w.shape[0])
    for k in range(x.shape[1]):
        acc = _fma(acc, x[:, k, None], w[None, :, k])
    return acc


def emulate_linear(x, W, bias=None):
    """P lanes per row; lane t chains the k of its pieces t, t + P, ... ascending; a halving tree; the bias last"""
    x, W = x.float(), W.float()
    M, K = x.shape
    P = linear_lanes(K)
    nch = K // 4
    acc = torch.zeros(M, P, W.shape[0])
    for c in range(cdiv(nch, P)):
        lanes = min(P, nch - c * P)                       # lanes whose piece c * P + t exists
        for e in range(4):
            k = 4 * (c * P + torch.arange(lanes)) + e
            acc[:, :lanes] = _fma(acc[:, :lanes], x[:, k, None], W.t()[None, k, :])
    h = P // 2
    while h >= 1:
        acc = acc[:, :h] + acc[:, h:2 * h]
        h //= 2
    out = acc[:, 0]
    return out if bias is None else out + bias.float()


def emulate_outer(y, W, add=None):
    """acc = 0; acc = fmaf(y[m, j], W[j, k], acc) for j ascending; add last"""
    y, W = y.float(), W.float()
    acc = torch.zeros(y.shape[0], W.shape[1])
    for j in range(y.shape[1]):
        acc = _fma(acc, y[:, j, None], W[None, j, :])
    return acc if add is None else acc + add.float()


def emulate_wgrad(y, x, cols=None):
    """(out, colsum): per slice a chain over its rows in order, the slices in wgrad_f32_ref.reduce_order.  ``cols``:
    only these columns of x (the elements are independent); the slicing is the full shape's"""
    M, n, K = y.shape[0], y.shape[1], x.shape[1]
    sh = wgrad_shape(M, n, K)
    S, rps = sh["slices"], sh["rows_per_slice"]
    if M == 0:
        return torch.zeros(n, K if cols is None else len(cols)), torch.zeros(n)
    a = y.float()
    b = x.float() if cols is None else x.float()[:, cols]
    pad = S * rps - M
    a = torch.cat([a, a.new_zeros(pad, n)]).view(S, rps, n)
    b = torch.cat([b, b.new_zeros(pad, b.shape[1])]).view(S, rps, -1)
    acc = torch.zeros(S, n, b.shape[2])
    cs = torch.zeros(S, n)
    for r in range(min(rps, M)):
        acc = _fma(acc, a[:, r, :, None], b[:, r, None, :])
        cs = cs + a[:, r]
    return F.reduce_order(acc), F.reduce_order(cs)


# ------------------------------------------------------------------ a-priori bars
U = 2.0 ** -24


def bar_project(x, w):
    return (x.shape[1] + 2) * U * (x.double().abs() @ w.double().abs().t())


def bar_linear(x, W, bias=None):
    m = x.double().abs() @ W.double().abs().t()
    return (x.shape[1] + 3) * U * (m if bias is None else m + bias.double().abs())


def bar_outer(y, W, add=None):
    m = y.double().abs() @ W.double().abs()
    return (y.shape[1] + 3) * U * (m if add is None else m + add.double().abs())


def bar_wgrad(y, x):
    """((L + S + 2) 2^-24 |y|^T |x|, the same for the column sums against a column of ones)"""
    L, S = chain_and_slices(y.shape[0], y.shape[1], x.shape[1])
    return (L + S + 2) * U * (y.double().abs().t() @ x.double().abs()), (L + S + 2) * U * y.double().abs().sum(0)


# ------------------------------------------------------------------ mutants
def _swap_cols(r, c):
    sw = r.clone()
    sw[:, [c, c + 1]] = r[:, [c + 1, c]]
    return sw


def _split3(a, b, grid):
    if grid not in WIDE:
        return {}
    return {"split3_three_products": G.split3_ref(a, b, four=False), "split3_four_products": G.split3_ref(a, b, four=True)}


def project_mutants(x, w0, w1, grid=None):
    """name -> (out0, out1) of a subtly wrong projection (none at M == 0)"""
    M, K = x.shape
    if M == 0:
        return {}
    r0, r1 = project_ref(x, w0), project_ref(x, w1)
    m = M // 2
    out = {"last_16_k_skipped": (project_ref(x[:, :K - 16], w0[:, :K - 16]), project_ref(x[:, :K - 16], w1[:, :K - 16])),
           "columns_swapped": (_swap_cols(r0, w0.shape[0] // 2 - 1), _swap_cols(r1, w0.shape[0] // 2 - 1)),
           "block1_from_block0": (r0, r0)}
    d0, d1 = r0.clone(), r1.clone()
    d0[m], d1[m] = 0, 0
    out["dropped_row"] = (d0, d1)
    for name, res in _split3(x, w0.t(), grid).items():
        out[name] = (res, _split3(x, w1.t(), grid)[name])
    return out


def linear_mutants(x, W, bias, grid=None):
    M, K = x.shape
    if M == 0:
        return {}
    r = linear_ref(x, W, bias)
    out = {"bias_dropped": linear_ref(x, W)}
    d = r.clone()
    d[M // 2] = 0
    out["dropped_row"] = d
    out["last_piece_skipped"] = linear_ref(x[:, :K - 4], W[:, :K - 4], bias)
    if W.shape[0] > 1:
        out["columns_swapped"] = _swap_cols(r, W.shape[0] // 2 - 1 if W.shape[0] > 2 else 0)
    for name, res in _split3(x, W.t(), grid).items():
        out[name] = res + bias.double()
    return out


def outer_mutants(y, W, add, grid=None):
    M, n = y.shape
    if M == 0:
        return {}
    r = outer_ref(y, W, add)
    out = {"add_dropped": outer_ref(y, W), "columns_swapped": _swap_cols(r, W.shape[1] // 2 - 1)}
    d = r.clone()
    d[M // 2] = 0
    out["dropped_row"] = d
    if n > 1:
        out["last_j_skipped"] = outer_ref(y[:, :n - 1], W[:n - 1], add)
    for name, res in _split3(y, W, grid).items():
        out[name] = res + add.double()
    return out


def wgrad_mutants(y, x, grid=None, K=None):
    """name -> (out, colsum).  ``K``: the width of the full x when ``x`` holds only some of its columns (the columns are
    independent; the slices are the full shape's)"""
    M, n, K = y.shape[0], y.shape[1], x.shape[1] if K is None else K
    if M == 0:
        return {}
    r, cs = wgrad_ref(y, x)
    keep = torch.ones(M, dtype=torch.bool)
    keep[M // 2] = False
    out = {"dropped_row": wgrad_ref(y[keep], x[keep]), "columns_swapped": (_swap_cols(r, x.shape[1] // 2 - 1), cs)}
    b, _ = wgrad_slices(M, n, K)[-1]
    out["last_slice_skipped"] = wgrad_ref(y[:b], x[:b])
    for name, res in _split3(y.t(), x, grid).items():
        out[name] = (res, cs)
    return out
