"""CPU references of the hierarchy decision: fixed-radius kNN, the 2-component mixture, its cut, the components.

kNN (``knn_ref``) is an INTEGER reference on dyadic inputs: coordinates are integer multiples of 2^-4 in [-4, 4]
and D <= 16, so every t = q - p is a multiple of 2^-4 of magnitude <= 8 (128 units), every t*t a multiple of 2^-8
of at most 128^2 units, and every partial sum at most 16 * 128^2 = 262144 units < 2^24: ``fmaf(t, t, d2)`` is exact
in fp32 in any order, and so is r*r for a radius that is a multiple of 2^-4.  A kernel's (idx, d2) must therefore
equal the integer result bit for bit, ties included; ``assert_exact_knn`` checks the bound on every call.

The mixture (``gmm_ref``) restates ``hgnn_gmm2_fit_f32`` in float64 from the same deterministic start;
``gmm_f32_emulation`` is the same EM with the E step in numpy float32, which sizes the tolerance of the device
comparison (tests/test_gpu_hierarchy_decision.py).  tests/test_hierarchy_ref.py proves all of them.
"""
import math

import numpy as np
import torch

# ------------------------------------------------------------------ kNN on dyadic grids
COORD_UNIT_INV = 16             # coordinates and radii are multiples of 1/16
COORD_MAX_UNITS = 64            # |coordinate| <= 4
KNN_D_MAX = 16
EXACT_LIMIT = 1 << 24           # every integer of magnitude <= 2^24 is an fp32 number
D2_UNIT_INV = COORD_UNIT_INV * COORD_UNIT_INV   # squared distances are multiples of 1/256
KNN_INSTANCES = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 32)


def _units(x: torch.Tensor, what: str) -> torch.Tensor:
    xi = torch.round(x.double() * COORD_UNIT_INV)
    assert bool((xi == x.double() * COORD_UNIT_INV).all()), f"{what}: not on the 2^-4 grid"
    assert x.numel() == 0 or int(xi.abs().max()) <= COORD_MAX_UNITS, f"{what}: outside [-4, 4]"
    return xi.long()


def assert_exact_knn(D: int, r_units: int):
    """the condition under which 'bitwise' is a fair demand on the kernels"""
    assert 1 <= D <= KNN_D_MAX
    assert D * (2 * COORD_MAX_UNITS) ** 2 < EXACT_LIMIT, "a squared distance can leave the exact integers of fp32"
    assert 0 <= r_units and r_units * r_units < EXACT_LIMIT, "r*r is not exact in fp32"


def knn_ref(q: torch.Tensor, p: torch.Tensor, K: int, r: float, chunk: int = 2048):
    """the K smallest keys (d2, idx) with d2 < r^2 of every query, ascending; padding idx = -1, d2 = -1.
    Returns (idx int64 [nq, K], d2 float32 [nq, K])."""
    nq, D = int(q.shape[0]), int(q.shape[1])
    n_p = int(p.shape[0])
    r_units = r * COORD_UNIT_INV
    assert r_units == int(r_units), "radius not on the 2^-4 grid"
    r_units = int(r_units)
    assert_exact_knn(D, r_units)
    qi, pi = _units(q, "query"), _units(p, "points")
    r2 = r_units * r_units
    idx = torch.full((nq, K), -1, dtype=torch.int64)
    d2o = torch.full((nq, K), -1.0, dtype=torch.float32)
    if n_p == 0 or nq == 0:
        return idx, d2o
    BIG = 1 << 62
    kk = min(K, n_p)
    ar = torch.arange(n_p, dtype=torch.int64)
    for a in range(0, nq, chunk):
        b = min(a + chunk, nq)
        d2 = torch.zeros(b - a, n_p, dtype=torch.int64)
        for d in range(D):
            t = qi[a:b, d:d + 1] - pi[:, d].unsqueeze(0)
            d2 += t * t
        key = torch.where(d2 < r2, d2 * (1 << 31) + ar, torch.full_like(d2, BIG))
        key = torch.sort(key, dim=1).values[:, :kk]
        ok = key < BIG
        idx[a:b, :kk] = torch.where(ok, key % (1 << 31), torch.full_like(key, -1))
        d2o[a:b, :kk] = torch.where(ok, (key >> 31).double() / D2_UNIT_INV, torch.full(key.shape, -1.0,
                                                                                       dtype=torch.float64)).float()
    return idx, d2o


def knn_brute_f64(q: torch.Tensor, p: torch.Tensor, K: int, r: float):
    """float64 brute force with a stable argsort: what ``knn_ref`` is proven against"""
    nq, n_p = int(q.shape[0]), int(p.shape[0])
    idx = torch.full((nq, K), -1, dtype=torch.int64)
    d2o = torch.full((nq, K), -1.0, dtype=torch.float32)
    if n_p == 0 or nq == 0:
        return idx, d2o
    d2 = ((q.double().unsqueeze(1) - p.double().unsqueeze(0)) ** 2).sum(-1)
    order = torch.argsort(d2, dim=1, stable=True)
    for i in range(nq):
        o = order[i]
        o = o[d2[i, o] < float(r) * float(r)][:K]
        idx[i, :o.numel()] = o
        d2o[i, :o.numel()] = d2[i, o].float()
    return idx, d2o


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def grid_points(n: int, D: int, seed: int, step_units: int = 16, half_levels: int = 4) -> torch.Tensor:
    """n points with coordinates step_units/16 * {-half_levels..half_levels}: the default (9 levels of 1.0) gives mass
    ties; ``fine_points`` uses every grid value"""
    assert step_units * half_levels <= COORD_MAX_UNITS
    c = torch.randint(-half_levels, half_levels + 1, (n, D), generator=_gen(seed))
    return (c * step_units).float() / COORD_UNIT_INV


def tie_case(D: int):
    """(half_levels, r) of a tie-heavy grid for dimension D: integer coordinates (step 1.0), narrower as D grows so that
    a good share of the points stays within the radius, and a radius whose square IS a squared distance of the grid
    (integer differences: any integer r is a sum of D squares), so that d2 == r^2 candidates exist and must be
    excluded"""
    if D <= 4:
        return 4, {1: 2.0, 2: 3.0, 3: 3.0, 4: 4.0}[D]
    if D <= 8:
        return 2, 4.0 if D <= 5 else 5.0
    return 1, 3.0 if D <= 9 else 4.0


def tie_points(n: int, D: int, seed: int) -> torch.Tensor:
    return grid_points(n, D, seed, half_levels=tie_case(D)[0])


def d2_units(q: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    """int64 [nq, np] squared distances in units of 2^-8"""
    qi, pi = _units(q, "query"), _units(p, "points")
    return ((qi.unsqueeze(1) - pi.unsqueeze(0)) ** 2).sum(-1)


def thin_inside(q: torch.Tensor, p: torch.Tensor, K: int, r: float, queries) -> torch.Tensor:
    """make the STRICT radius cut observable.  A candidate with d2 == r^2 can only reach a kernel's output when the
    query has fewer than K points strictly inside the radius, and on a dense grid nearly every query has far more.
    For each listed query, all but (K - 1) // 2 of the points strictly inside are replaced by copies of the points
    exactly AT the radius: the correct result of that query is at most (K - 1) // 2 entries and padding, while a
    kernel that tests `d2 <= r^2` fills the padding with the at-radius points.  A query without an at-radius point gets
    one made for it (``at_radius_point``)."""
    p = p.clone()
    if p.shape[0] == 0:
        return p
    r2 = int(round(r * COORD_UNIT_INV)) ** 2
    for i in queries:
        d2 = d2_units(q[i:i + 1], p)[0]
        at, inside = torch.nonzero(d2 == r2).flatten(), torch.nonzero(d2 < r2).flatten()
        moved = inside[(K - 1) // 2:]
        if at.numel() > 0:
            p[moved] = p[at[torch.arange(moved.numel()) % at.numel()]]
        else:
            p[moved if moved.numel() > 0 else int(torch.argmax(d2))] = at_radius_point(q[i], r)
    return p


def at_radius_point(q_row: torch.Tensor, r: float) -> torch.Tensor:
    """a grid point at distance exactly r from q_row: r along one axis (3 and 4 along two axes for r = 5), each step
    taken towards the origin so that the point stays in [-4, 4]"""
    parts = {5.0: (3.0, 4.0)}.get(float(r), (float(r),))
    assert sum(t * t for t in parts) == r * r and len(parts) <= q_row.numel() and max(parts) <= 4.0
    out = q_row.clone()
    for d, t in enumerate(parts):
        out[d] = out[d] - t if out[d] >= 0 else out[d] + t
    return out


WITNESS_QUERIES = 4096      # the conditions below are evaluated on the first 4096 queries (all, but for BLOCK = 256)


def radius_counts(q, p, r):
    """(points strictly inside the radius, points exactly at it) of each of the first WITNESS_QUERIES queries"""
    r2 = int(round(r * COORD_UNIT_INV)) ** 2
    d2 = d2_units(q[:WITNESS_QUERIES], p)
    return (d2 < r2).sum(1), (d2 == r2).sum(1)


def strict_cut_witnesses(q, p, K, r) -> int:
    """queries with fewer than K points strictly inside the radius AND a point exactly at it: the only queries at
    which `d2 <= r^2` and `d2 < r^2` give different outputs"""
    if p.shape[0] == 0:
        return 0
    below, at = radius_counts(q, p, r)
    return int(((below < K) & (at > 0)).sum())


def truncating_queries(q, p, K, r) -> int:
    """queries with MORE than K points strictly inside the radius: there the list fills, later candidates are inserted
    into a full list and the selection drops keys"""
    if p.shape[0] == 0:
        return 0
    return int((radius_counts(q, p, r)[0] > K).sum())


def tie_inputs(nq, n_p, D, seed, K, dup=False, thin=True):
    """(q, p, r) of one kNN input: tie-heavy grid, optional exact duplicates, the tie radius of D, and two queries (the
    first and the middle one of the first WITNESS_QUERIES) thinned by ``thin_inside`` so that the input has witnesses
    of the strict cut, while the other queries keep more than K points inside the radius (the selection truncates).
    ``thin=False`` leaves every query dense."""
    q, p = tie_points(nq, D, seed), tie_points(n_p, D, seed + 1)
    if dup:
        p = with_duplicates(p, seed + 2)
    r = tie_case(D)[1]
    m = min(nq, WITNESS_QUERIES)
    return q, thin_inside(q, p, K, r, sorted({0, m // 2})) if thin else p, r


def tie_runs(nq, n_p, D, seed, K, dup=False):
    """the inputs one kNN arm is run on.  A single query is its own thinned witness: its correct row is a few entries
    and padding, so its list never fills and neither the truncation at K nor the stable insertion into a full list is
    exercised.  With nq = 1 the arm therefore runs a second time on the un-thinned points, where that one query has
    more than K points inside the radius."""
    runs = [tie_inputs(nq, n_p, D, seed, K, dup)]
    if nq == 1:
        dense = tie_inputs(nq, n_p, D, seed, K, dup, thin=False)
        if not torch.equal(dense[1], runs[0][1]):
            runs.append(dense)
    return runs


def fine_points(n: int, D: int, seed: int) -> torch.Tensor:
    return grid_points(n, D, seed, step_units=1, half_levels=COORD_MAX_UNITS)


def with_duplicates(p: torch.Tensor, seed: int, fraction: float = 0.5) -> torch.Tensor:
    """a `fraction` of the rows replaced by exact copies of other rows (at random places)"""
    n = int(p.shape[0])
    g = _gen(seed)
    out = p.clone()
    m = int(n * fraction)
    if n > 1 and m > 0:
        to = torch.randperm(n, generator=g)[:m]
        frm = torch.randint(0, n, (m,), generator=g)
        out[to] = p[frm]
    return out


def tie_shell(D: int, n_inner: int, n_shell: int, n_outer: int, seed: int):
    """one configuration around the origin: `n_inner` points strictly inside the shell, `n_shell` points at the
    SAME distance (sign flips and coordinate permutations of one vector), `n_outer` beyond it, in shuffled index
    order.  Returns (points, shell d2 in units of 2^-8)."""
    g = _gen(seed)
    base = torch.zeros(D)
    base[0] = 2.0
    if D > 1:
        base[1] = 1.0
    shell = torch.stack([base[torch.randperm(D, generator=g)] * (torch.randint(0, 2, (D,), generator=g) * 2 - 1).float()
                         for _ in range(n_shell)])
    shell_units = int(round(float((base * base).sum()) * D2_UNIT_INV))
    inner = torch.zeros(n_inner, D)
    inner[:, 0] = (torch.randint(-16, 17, (n_inner,), generator=g)).float() / COORD_UNIT_INV      # |x| <= 1 < shell
    outer = torch.zeros(n_outer, D)
    outer[:, 0] = (torch.randint(40, 65, (n_outer,), generator=g)).float() / COORD_UNIT_INV
    outer[:, 0] *= (torch.randint(0, 2, (n_outer,), generator=g) * 2 - 1).float()
    pts = torch.cat([inner, shell, outer])
    return pts[torch.randperm(pts.shape[0], generator=g)].contiguous(), shell_units


def far_apart(nq: int, n_p: int, D: int, seed: int):
    """queries with every coordinate in [-4, -3], points in [3, 4]: nothing within radius 1"""
    g = _gen(seed)
    q = -(torch.randint(48, 65, (nq, D), generator=g).float() / COORD_UNIT_INV)
    p = torch.randint(48, 65, (n_p, D), generator=g).float() / COORD_UNIT_INV
    return q, p


# the arms of tests/test_gpu_knn_exact.py (its docstring states the rotation rule); they live here so that
# tests/test_hierarchy_ref.py can assert their input conditions on the CPU
KNN_DS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16)
KNN_NQS = (1, 63, 64, 65)
NP_SPLIT = (512, 513, 1023, 1025, 700)
NP_NOWS = (512, 513, 1023, 1025)
NP_SMALL = (255, 256, 257, 511)


def kd_cases():
    """(K, D, form, nq, np, radius from the device, duplicates) of the K x D cross product"""
    cases = []
    for i, K in enumerate(KNN_INSTANCES):
        for j, D in enumerate(KNN_DS):
            s, h = i + j, (i + j) // 2
            if s % 2 == 0:
                form, n_p = "split", NP_SPLIT[h % len(NP_SPLIT)]
            elif s % 4 == 1:
                form, n_p = "nows", NP_NOWS[h % len(NP_NOWS)]
            else:
                form, n_p = "small", NP_SMALL[h % len(NP_SMALL)]
            r_dev = form != "nows" and h % 2 == 1
            cases.append((K, D, form, KNN_NQS[(i + 2 * j) % 4], n_p, r_dev, s % 3 == 0))
    return cases


def kd_runs(case):
    K, D, form, nq, n_p, r_dev, dup = case
    return tie_runs(nq, n_p, D, 1000 + 37 * K + D, K, dup)


def block256_case(i):
    """(K, D, nq, np) of the i-th BLOCK = 256 arm"""
    return KNN_INSTANCES[i], KNN_DS[(3 * i) % 10], 65536 + i % 2, (40, 270)[i % 2]


def block256_inputs(i):
    K, D, nq, n_p = block256_case(i)
    return tie_inputs(nq, n_p, D, 2000 + i, K, dup=i % 3 == 0)


NP_EDGES = ("0", "1", "K-1", "K", "255", "256", "257", "511", "512", "513", "1023", "1025")


def np_edge_case(n):
    """(K, np, nq, D) of the n-th point count of NP_EDGES"""
    e = NP_EDGES[n]
    K = {"K-1": 10, "K": 16}.get(e, KNN_INSTANCES[(5 * n + 3) % len(KNN_INSTANCES)])
    n_p = {"K-1": K - 1, "K": K}[e] if e in ("K-1", "K") else int(e)
    return K, n_p, KNN_NQS[n % 4], KNN_DS[(n + 2) % len(KNN_DS)]


def np_edge_runs(n):
    K, n_p, nq, D = np_edge_case(n)
    return tie_runs(nq, n_p, D, 3000 + n, K)


# (nq, np, expected slices): slice_len at its 256-multiple edges with want = 32 at the cap (1 query block), want = 16
# (128 query blocks) and want = ceil(2048 / 66) = 32 reached without the cap (66 query blocks)
SLICE_EDGE_CASES = [(64, 8191, 32), (64, 8192, 32), (64, 8193, 17), (8192, 4096, 16), (8192, 4097, 9), (4161, 600, 3)]
SLICE_EDGE_K = 5


def slice_edge_inputs(nq, n_p):
    return tie_inputs(nq, n_p, 3, 4000 + n_p, SLICE_EDGE_K)


RADIUS_FORMS_K = 8


def radius_forms_inputs():
    return tie_inputs(65, 700, 3, 5000, RADIUS_FORMS_K)


LARGE_KS, LARGE_DS = (33, 64, 100, 128), (1, 4, 7, 16)


def large_case(K, D, form):
    """(nq, np, duplicates) of one knn_large arm"""
    nq = (37, 16, 17, 64)[(K + D) % 4]
    n_p = ((1300, 513, 1025, 700) if form == "split" else (500, 1300, 257, 1025))[(K + D + 3) % 4]
    return nq, n_p, (K + D) % 3 == 0


def large_inputs(K, D, form):
    nq, n_p, dup = large_case(K, D, form)
    return tie_inputs(nq, n_p, D, 7000 + K + D, K, dup)


def edges_from_knn(idx: torch.Tensor, sym: bool, n: int) -> torch.Tensor:
    """the graph ``DynamicGraphConstruction.build_graph`` derives from a kNN result"""
    pos = idx >= 0
    ind = torch.arange(idx.shape[0]).unsqueeze(1).expand(idx.shape)
    s, d = ind[pos], idx[pos]
    if sym:
        key = torch.unique(torch.cat([s * n + d, d * n + s]))
        s, d = torch.div(key, n, rounding_mode="floor"), key % n
    return torch.stack([s, d], dim=0)


# ------------------------------------------------------------------ the mixture
EPS10 = 10.0 * 1.1920928955078125e-07       # sklearn: nk += 10 * eps(float32)
TWO_PI = 6.283185307179586
(S_W0, S_W1, S_MU0, S_MU1, S_VAR0, S_VAR1, S_PREV, S_CONV, S_ITERS, S_MIN, S_MAX, S_C0, S_C1, S_CUT, S_LOWER,
 S_SPARE) = range(16)


def _start(v32: np.ndarray):
    """min/max centres, 8 Lloyd passes (component 1 iff STRICTLY nearer to c1, compared in float32), hard M sums"""
    x = v32.astype(np.float64)
    lo, hi = float(x.min()), float(x.max())
    c0, c1 = lo, hi
    sums = None
    for it in range(9):                                      # 8 Lloyd updates, then the hard M step's assignment
        hard = np.abs(v32 - np.float32(c0)) > np.abs(v32 - np.float32(c1))
        x1, x0 = x[hard], x[~hard]
        sums = (float(x0.size), x0.sum(), (x0 * x0).sum(), float(x1.size), x1.sum(), (x1 * x1).sum())
        if it < 8:
            c0 = sums[1] / max(sums[0], 1.0)
            c1 = sums[4] / max(sums[3], 1.0)
    return lo, hi, c0, c1, sums


def _m_step(s, reg_covar):
    n0, n1 = s[0] + EPS10, s[3] + EPS10
    m0, m1 = s[1] / n0, s[4] / n1
    return [n0 / (n0 + n1), n1 / (n0 + n1), m0, m1, max(s[2] / n0 - m0 * m0, 0.0) + reg_covar, max(s[5] / n1 - m1 * m1, 0.0) + reg_covar]


def _e_step_f64(x, v32, p):
    w0, w1, mu0, mu1, var0, var1 = p
    lp0 = math.log(w0) - 0.5 * math.log(TWO_PI * var0) - 0.5 * (x - mu0) ** 2 / var0
    lp1 = math.log(w1) - 0.5 * math.log(TWO_PI * var1) - 0.5 * (x - mu1) ** 2 / var1
    m = np.maximum(lp0, lp1)
    e0, e1 = np.exp(lp0 - m), np.exp(lp1 - m)
    s = e0 + e1
    return e0 / s, m + np.log(s)


def _e_step_f32(x, v32, p):
    """the kernel's E step in numpy float32 (1/var, logf, exp and the log-sum-exp in float32; the fused multiply-add
    as a float64 product-sum rounded once)"""
    f = np.float32
    w0, w1, mu0, mu1, var0, var1 = [f(t) for t in p]
    iv0, iv1 = f(1.0) / var0, f(1.0) / var1
    k0 = np.log(w0) - f(0.5) * np.log(f(TWO_PI) * var0)
    k1 = np.log(w1) - f(0.5) * np.log(f(TWO_PI) * var1)
    d0, d1 = v32 - mu0, v32 - mu1
    lp0 = ((f(-0.5) * d0 * d0).astype(np.float64) * float(iv0) + float(k0)).astype(f)
    lp1 = ((f(-0.5) * d1 * d1).astype(np.float64) * float(iv1) + float(k1)).astype(f)
    m = np.maximum(lp0, lp1)
    e0, e1 = np.exp(lp0 - m), np.exp(lp1 - m)
    s = e0 + e1
    norm = m + np.log(s)
    assert norm.dtype == np.float32 and e0.dtype == np.float32
    return (e0 / s).astype(np.float64), norm.astype(np.float64)


def _gmm(v, max_iter, tol, reg_covar, e_step):
    v32 = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1))
    M = v32.size
    assert M > 0 and reg_covar > 0
    tol = float(np.float32(tol))
    reg_covar = float(np.float32(reg_covar))
    x = v32.astype(np.float64)
    lo, hi, c0, c1, sums = _start(v32)
    p = _m_step(sums, reg_covar)
    prev, conv, iters, lower = 0.0, 0.0, 0, 0.0
    deltas = []
    for it in range(int(max_iter)):
        with np.errstate(under="ignore", divide="ignore"):
            r0, norm = e_step(x, v32, p)
        r1 = 1.0 - r0
        lower = float(norm.sum() / M)
        if it > 0:
            deltas.append(abs(lower - prev))
        stop = it > 0 and abs(lower - prev) < tol
        prev, iters = lower, it + 1
        if stop:
            conv = 1.0
            break
        p = _m_step((r0.sum(), (r0 * x).sum(), (r0 * x * x).sum(), r1.sum(), (r1 * x).sum(), (r1 * x * x).sum()),
                    reg_covar)
    state = np.zeros(16, dtype=np.float64)
    state[:6] = p
    state[S_PREV], state[S_CONV], state[S_ITERS] = prev, conv, iters
    state[S_MIN], state[S_MAX], state[S_C0], state[S_C1], state[S_LOWER] = lo, hi, c0, c1, lower
    return state, deltas


def gmm_ref(v, max_iter=100, tol=1e-3, reg_covar=1e-6):
    """float64 restatement of ``hgnn_gmm2_fit_f32``: (state[16], [|delta lower| of pass 1, 2, ...])"""
    return _gmm(v, max_iter, tol, reg_covar, _e_step_f64)


def gmm_f32_emulation(v, max_iter=100, tol=1e-3, reg_covar=1e-6):
    return _gmm(v, max_iter, tol, reg_covar, _e_step_f32)


def gmm_start_ref(v):
    """(min, max, c0, c1) only: the deterministic start, exact on dyadic v"""
    lo, hi, c0, c1, _ = _start(np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1)))
    return lo, hi, c0, c1


def deltas_clear_of_tol(deltas, tol, factor=2.0):
    """the input condition of pass-count equality: no |delta lower| within a factor 2 of tol"""
    return all(not (tol / factor <= d <= tol * factor) for d in deltas)


GMM_QUANTITIES = ("w", "mu", "var", "lower")


def gmm_deviation(a, b):
    """largest deviation between two states, per quantity"""
    return {"w": float(np.abs(a[0:2] - b[0:2]).max()), "mu": float(np.abs(a[2:4] - b[2:4]).max()),
            "var": float(np.abs(a[4:6] - b[4:6]).max()), "lower": float(abs(a[S_LOWER] - b[S_LOWER]))}


# the EM cases of the device comparison: name -> (values float32, max_iter); tol = 1e-3, reg_covar = 1e-6
def _rng(seed):
    return np.random.default_rng(seed)


def _mix(seed, n0, mu0, sd0, n1, mu1, sd1):
    r = _rng(seed)
    v = np.concatenate([r.normal(mu0, sd0, n0), r.normal(mu1, sd1, n1)])
    return r.permutation(v).astype(np.float32)


def likelihood_like(seed, M):
    """atanh of clamped dots as the model produces them: a broad false-edge mode, a narrow true-edge mode near the
    clamp, and values AT both clamps (+-atanh(1 - 2^-23) ~ 8.3 as float32)"""
    r = _rng(seed)
    dots = np.concatenate([np.clip(r.normal(0.1, 0.14, M - M // 3), -1, 1), 1 - np.abs(r.normal(0, 0.02, M // 3))])
    dots[:7] = 1.0
    dots[7:11] = -1.0
    hi = np.float32(1 - 1e-7)
    dots = np.clip(dots.astype(np.float32), -hi, hi)
    return r.permutation(np.arctanh(dots.astype(np.float64))).astype(np.float32)


def em_cases():
    return {
        "balanced": (_mix(1, 20000, -1.0, 0.3, 20000, 1.4, 0.7), 100),
        "imbalanced_1000_1": (_mix(2, 100000, 0.0, 0.5, 100, 5.0, 0.3), 100),
        "overlapping": (_mix(3, 30000, 0.0, 1.0, 30000, 3.4, 1.0), 100),
        "collapsed": (np.concatenate([np.full(5000, 0.75, np.float32), _rng(4).normal(3.0, 0.5, 5000).astype(np.float32)]),
                      100),
        "likelihoods": (likelihood_like(5, 60000), 100),
        "one_block": (_mix(6, 600, -1.0, 0.4, 400, 0.5, 0.6), 100),
        "over_2p20": (_mix(7, 700000, 0.0, 0.6, (1 << 20) + 4097 - 700000, 2.3, 0.8), 100),
        "max_iter_1": (_mix(8, 20000, 0.0, 1.0, 20000, 0.6, 0.3), 1),
        "max_iter_3": (_mix(8, 20000, 0.0, 1.0, 20000, 0.6, 0.3), 3),
    }


# degenerate inputs of the fit: every responsibility is exactly 0 or 1
DEGENERATE = {
    "constant": np.full(5000, 0.75, np.float32),
    "constant_over_a_block": np.full(300001, -2.5, np.float32),
    "M1": np.array([2.5], np.float32),
    "two_values": np.array([-1.0, 3.0], np.float32),
    "two_distinct_repeated": np.array([3.0, 3.0, -1.0, -1.0, -1.0] * 200, np.float32),
}


def degenerate_lower_budget(x_max, reg_covar=1e-6):
    """float32 error budget of the lower bound on the degenerate inputs (|values| <= x_max), where it is ONE float32
    value per distinct data value, lp = fmaf(-0.5 d^2, 1/var, k) with k = logf(w) - 0.5 logf(2 pi var), repeated N
    times (the other component's term underflows, so the log-sum-exp adds exactly 0) -- its roundings do not average
    out.  With eps = 2^-24, reg_covar <= var and 2 pi var < 1:
      0.5 x 3 eps                  2 pi, var and their product rounded to float32: relative 3 eps in the log's argument
      0.5 x ulp(|log(2 pi var)|)   logf is accurate to 1 ulp of its result; |log(2 pi var)| <= |log(2 pi reg_covar)|
      2 eps                        w rounded to float32 and logf(w), |log w| < 1
      ulp(|k|) / 2, twice          the subtraction that forms k and the fused multiply-add that forms lp,
                                   |k| <= 0.5 |log(2 pi reg_covar)| + 1
      the quadratic term           nk += 10 eps(float32) = 20 eps pulls the mean of N copies of x to x (1 - 20 eps / N),
                                   so d = 20 eps x / N, but the kernel subtracts the mean rounded to float32 (error
                                   <= eps x): |d_f32^2 - d^2| <= eps^2 x^2 (40 / N + 1), times 0.5 / var with
                                   var = reg_covar + 20 eps x^2 / N.  Monotone in N: the larger of N = 1 and N -> inf.
    For reg_covar = 1e-6 and x_max = 3: 19.5 eps + 0.9 eps = 1.2e-6."""
    eps = 2.0 ** -24
    big = abs(math.log(TWO_PI * reg_covar))
    assert TWO_PI * (reg_covar + 20 * eps * x_max * x_max) < 1.0
    k = 0.5 * big + 1.0
    a = 0.5 * eps * eps * x_max * x_max
    quad = max(41 * a / (reg_covar + 20 * eps * x_max * x_max), a / reg_covar)
    return 0.5 * 3 * eps + 0.5 * float(np.spacing(np.float32(big))) + 2 * eps + float(np.spacing(np.float32(k))) + quad


def dyadic_values(M, seed):
    """multiples of 1/16 in [-8, 8]: sums of M of them (<= 2^7 * 2^22 units) are exact in float64 in any order"""
    return (_rng(seed).integers(-128, 129, M).astype(np.float32)) / np.float32(16)


# ------------------------------------------------------------------ the cut
def _posterior_logs(state, x):
    w, mu, var = state[0:2], state[2:4], state[4:6]
    return [math.log(w[k]) - 0.5 * ((x - mu[k]) ** 2 / var[k] + math.log(TWO_PI * var[k])) for k in (0, 1)]


def cut_function(state, granularity):
    """x -> sigmoid(r) P(left | x) - sigmoid(-r) P(right | x), and (left, right)"""
    mu = state[2:4]
    left, right = (0, 1) if mu[0] <= mu[1] else (1, 0)
    sr, sl = 1.0 / (1.0 + math.exp(-granularity)), 1.0 / (1.0 + math.exp(granularity))

    def f(x):
        lp = _posterior_logs(state, x)
        m = max(lp)
        p = [math.exp(lp[0] - m), math.exp(lp[1] - m)]
        s = p[0] + p[1]
        return sr * p[left] / s - sl * p[right] / s

    return f, left, right


def cut_ref(state, granularity):
    """(cut, has_root): root of the cut function between the two means by 200 float64 bisection steps; the midpoint of
    the means when the function does not change sign there"""
    f, left, right = cut_function(state, granularity)
    lo, hi = float(state[2 + left]), float(state[2 + right])
    if f(lo) * f(hi) > 0.0:
        return 0.5 * (lo + hi), False
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if f(lo) * f(mid) <= 0.0:
            hi = mid
        else:
            lo = mid
    return 0.5 * (lo + hi), True


def cut_log_ratio(state, granularity, x):
    """g(x) = log P(left | x) - log P(right | x) + r: the cut is its root; its evaluation error and slope size the
    allowance of a float64 root solve"""
    _, left, right = cut_function(state, granularity)
    lp = _posterior_logs(state, x)
    return lp[left] - lp[right] + granularity, abs(lp[left]) + abs(lp[right]) + abs(granularity)


def score_cut_forms(score_cut, cut, state, training, momentum=0.95):
    """the block's score_cut bookkeeping in float32: inf -> middle of the means; EMA only in training and only when
    the cut lies strictly between the means.  Returns the float32 results of the three ways a compiler may evaluate
    momentum * sc + (1 - momentum) * cut: unfused (both products rounded), and either product fused into the add.
    (A product of two float32 is exact in float64, and so is its sum with a float32 of comparable magnitude, so the
    fused forms round once.)"""
    f = np.float32
    mlo, mhi = min(state[2], state[3]), max(state[2], state[3])
    sc = f(score_cut)
    if np.isinf(sc):
        sc = f(0.5 * (mlo + mhi))
    if not (training and mlo < cut < mhi):
        return (f(sc),) * 3
    m, om, c = f(momentum), f(f(1.0) - f(momentum)), f(cut)
    a, b = f(m * sc), f(om * c)
    return f(a + b), f(float(m) * float(sc) + float(b)), f(float(om) * float(c) + float(a))


def score_cut_ref(score_cut, cut, state, training, momentum=0.95):
    """the unfused float32 form of ``score_cut_forms``"""
    return score_cut_forms(score_cut, cut, state, training, momentum)[0]


# ------------------------------------------------------------------ components
def kept_edges(src, dst, n, score=None, cut=None):
    """mask of the edges that count: both endpoints in [0, n) and, with a score, score >= cut (NaN >= x is False)"""
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    dst = np.asarray(dst, dtype=np.int64).reshape(-1)
    keep = (src >= 0) & (dst >= 0) & (src < n) & (dst < n)
    if score is not None:
        with np.errstate(invalid="ignore"):
            keep &= np.asarray(score, dtype=np.float32).reshape(-1) >= np.float32(cut)
    return keep


def components_ref(src, dst, n, score=None, cut=None):
    """plain union-find over the ``kept_edges``: (labels int32[n] = smallest vertex id of the component, present
    int32[n])"""
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    dst = np.asarray(dst, dtype=np.int64).reshape(-1)
    keep = kept_edges(src, dst, n, score, cut)
    parent = list(range(n))
    present = np.zeros(n, dtype=np.int32)
    for u, v in zip(src[keep].tolist(), dst[keep].tolist()):
        present[u] = 1
        present[v] = 1
        while parent[u] != u:
            parent[u] = parent[parent[u]]
            u = parent[u]
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        if u != v:
            if u < v:
                parent[v] = u
            else:
                parent[u] = v
    labels = np.empty(n, dtype=np.int32)
    for i in range(n):                      # parents have smaller ids: one ascending sweep resolves every root
        labels[i] = i if parent[i] == i else labels[parent[i]]
    return labels, present


def cluster_labels_ref(src, dst, n, min_cluster_size, score=None, cut=None):
    """``_cluster_labels``: (clusters int64[n], count).  -1 for vertices in no kept edge or in a component of fewer
    than `min_cluster_size` such vertices; the rest 0..C-1 in increasing order of the component's smallest id."""
    labels, present = components_ref(src, dst, n, score, cut)
    counts = np.bincount(labels[present > 0], minlength=n)
    keep_root = counts >= int(min_cluster_size)
    new_id = np.cumsum(keep_root) - 1
    keep = (present > 0) & keep_root[labels]
    clusters = np.where(keep, new_id[labels], -1).astype(np.int64)
    return clusters, int(keep_root.sum())


# ------------------------------------------------------------------ the whole decision
CLAMP = float(np.float32(1 - 1e-7))


def likelihood_ref(emb, graph):
    """atanh(clamp(<emb[g0], emb[g1]>)) in float64 (the clamp bounds are the float32 constants of the model)"""
    e = np.asarray(emb, dtype=np.float64)
    g = np.asarray(graph, dtype=np.int64)
    return np.arctanh(np.clip((e[g[0]] * e[g[1]]).sum(-1), -CLAMP, CLAMP))


def decision_ref(emb, graph, score_cut, hparams, training):
    """``gmm_edge_clustering`` in float64.  Returns a dict: clusters, count, score_cut (float32), host_reads,
    likelihood (float64), state, deltas, cut."""
    n = int(np.asarray(emb).shape[0])
    g = np.asarray(graph, dtype=np.int64)
    min_size = int(hparams["min_cluster_size"])
    if g.shape[1] == 0:
        return dict(clusters=np.full(n, -1, dtype=np.int64), count=0, score_cut=np.float32(score_cut), host_reads=0,
                    likelihood=np.zeros(0), state=None, deltas=[], cut=None)
    lik = likelihood_ref(emb, g)
    state, deltas = gmm_ref(lik.astype(np.float32))
    cut, _ = cut_ref(state, float(hparams.get("cluster_granularity", 0)))
    state[S_CUT] = cut
    sc = score_cut_ref(score_cut, cut, state, training)
    clusters, count = cluster_labels_ref(g[0], g[1], n, min_size, lik, float(sc))
    reads = 1
    if count <= 3:
        clusters, count = cluster_labels_ref(g[0], g[1], n, min_size)
        reads = 2
    return dict(clusters=clusters, count=count, score_cut=sc, host_reads=reads, likelihood=lik, state=state,
                deltas=deltas, cut=cut)


def likelihood_error_bound(D, max_abs_dot):
    """float32 error of atanh(<a, b>) for unit-norm rows of width D with |<a, b>| <= max_abs_dot: the dot product's
    D * eps * sum|a_i b_i| <= D * eps, amplified by atanh' = 1 / (1 - x^2), plus 4 ulp of the atanh itself"""
    eps = 2.0 ** -24
    return D * eps / (1.0 - max_abs_dot ** 2) + 4 * 2 * eps * math.atanh(max_abs_dot)


def decision_inputs(kind, seed=0):
    """synthetic embeddings (unit rows, D = 8) and a graph for the whole-decision tests.
    'normal': 150 tracks of 12 hits, dense edges inside a track, some between tracks;
    'fallback': 3 big tracks whose cut graph has 3 components (<= 3: the uncut graph is used instead);
    'empty': no edges."""
    r = _rng(100 + seed)
    D = 8
    n_tracks, per = (150, 12) if kind != "fallback" else (3, 300)
    centres = r.normal(size=(n_tracks, D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    track = np.repeat(np.arange(n_tracks), per)
    emb = centres[track] + 0.05 * r.normal(size=(n_tracks * per, D))
    emb = (emb / np.linalg.norm(emb, axis=1, keepdims=True)).astype(np.float32)
    n = emb.shape[0]
    if kind == "empty":
        return emb, np.zeros((2, 0), dtype=np.int64)
    n_in, n_out = (6 * n, 3 * n)
    a = r.integers(0, n, n_in)
    b = track[a] * per + r.integers(0, per, n_in)
    a, b = a[a != b], b[a != b]
    c, d = r.integers(0, n, 4 * n_out), r.integers(0, n, 4 * n_out)
    dots = (emb[c].astype(np.float64) * emb[d]).sum(-1)
    ok = (track[c] != track[d]) & (np.abs(dots) < 0.6)
    c, d = c[ok][:n_out], d[ok][:n_out]
    graph = np.stack([np.concatenate([a, c]), np.concatenate([b, d])]).astype(np.int64)
    return emb, graph[:, r.permutation(graph.shape[1])]


# ------------------------------------------------------------------ shared inputs of the CPU proof and the GPU tests
CUT_STATES = {
    "ordered": [0.6, 0.4, -1.0, 2.0, 0.25, 0.5],
    "swapped": [0.3, 0.7, 2.5, -0.5, 0.4, 0.2],
    "no_sign_change": [0.999, 0.001, 0.0, 0.1, 4.0, 0.01],
    "far": [0.5, 0.5, -3.0, 4.0, 0.25, 0.3],
}


def cc_inputs(n=50000, M=400000, seed=0, cut=0.9):
    """random graph with every edge class of the components test: scores equal to the cut, one ulp below, NaN; self
    loops; duplicated edges; endpoints -1 and n"""
    r = np.random.default_rng(seed)
    # about 0.6 n edges survive the cut: near the percolation threshold, so component sizes spread from 1 to hundreds
    src, dst = r.integers(0, n, M), r.integers(0, n, M)
    score = r.uniform(-1, 1, M).astype(np.float32)
    cutf = np.float32(cut)
    k = M // 40
    score[0 * k:1 * k] = cutf
    score[1 * k:2 * k] = np.nextafter(cutf, np.float32(-np.inf))
    score[2 * k:3 * k] = np.nan
    dst[3 * k:4 * k] = src[3 * k:4 * k]
    src[4 * k:5 * k], dst[4 * k:5 * k], score[4 * k:5 * k] = src[5 * k:6 * k], dst[5 * k:6 * k], score[5 * k:6 * k]
    src[6 * k:6 * k + 50] = -1
    dst[6 * k + 50:6 * k + 100] = n
    src[6 * k + 100:6 * k + 150] = n
    dst[6 * k + 150:6 * k + 200] = -1
    score[6 * k:6 * k + 200] = 1.0                                          # kept by the score: dropped by the ids
    p = r.permutation(M)
    return src[p], dst[p], score[p], float(cutf)


HPARAMS = {"min_cluster_size": 3, "cluster_granularity": 0.0}


# the allowance of the device cut in the whole-decision inputs: the EM allowance (16 x d_emul of the decision's own
# mixture, asserted below to stay under 2e-6 for w, mu and var) propagated through cut_ref (asserted below)
CUT_ALLOWANCE_DECISION = 2e-5


def cut_perturbation(state, granularity, allow):
    """largest change of cut_ref's root when w0 (and w1 = 1 - w0 against it), mu0, mu1, var0, var1 each move by
    +-allow[quantity]"""
    base, _ = cut_ref(state, granularity)
    worst = 0.0
    for bits in range(32):
        sg = [1 if bits >> i & 1 else -1 for i in range(5)]
        s = state.copy()
        s[0] += sg[0] * allow["w"]
        s[1] -= sg[0] * allow["w"]
        s[2] += sg[1] * allow["mu"]
        s[3] += sg[2] * allow["mu"]
        s[4] = max(s[4] + sg[3] * allow["var"], 1e-300)
        s[5] = max(s[5] + sg[4] * allow["var"], 1e-300)
        worst = max(worst, abs(cut_ref(s, granularity)[0] - base))
    return worst
