"""Grids, case lists and integer references for the exact conformance of the three scalar-result operators: the
pair hinge loss (csrc/pairloss.hip), the pT-weighted BCE (csrc/wbce.hip) and the attention weights of graph
construction (csrc/graphcon.hip, hgnn_graph_attention_*).

The inputs sit on grids where every float32 operation the header prescribes is exact, so the float64 sums are exact in
any order and the reference does not restate the reduction tree.  The references count in numpy int64:

  pt weighting   hparams weight_min 0.5, ptcut 1.0, pt_interval 0.5 (cut 0.5, cap 1.0, interval 0.5), weight_leak in
                 {0.25, 0, 1}; pt a multiple of 1/8 in [0, 3] or NaN.  32 ptw(pt) is the integer ``ptw32``.
  weighted BCE   scores in {0, 1}: l is exactly 0 or 100.  Sums in units of 1/32.
  pair hinge     integer points in [-3, 3]^D, pairs with a perfect-square squared distance >= 1, scale in {0.5, 1, 2},
                 integer margin: 2 l is an integer, raw l^2 a multiple of 1/128.
  attention      integer rows: x is the integer dot product; E a power of two in training mode.

``tests/test_scalar_ops_exact_ref.py`` proves the representability of every intermediate and that the cases are not
vacuous (``MUTANTS``); ``tests/test_gpu_scalar_ops_exact.py`` compares the kernels' bits with these references."""
import functools
import math

import numpy as np

BLOCK = 256                       # threads per workgroup (csrc/common.h kBlock)
MAX_GRID = 2048                   # csrc/det_reduce.h kDetMaxGrid
IDTS = (np.int32, np.int64)
VEC = {np.int32: 4, np.int64: 2}  # pairs per thread: 16 / sizeof(index)
HP = dict(weight_min=0.5, weight_leak=0.25, ptcut=1.0, pt_interval=0.5, log_weight_ratio=0.0)
LEAKS = (0.25, 0.0, 1.0)
DIMS = (1, 2, 3, 4, 5, 8, 12, 15, 16)
TINY = (0, 1, 2, 3, 4, 5, 7, 8, 9)
FAMILIES = ("tiny", "workgroup", "two_workgroups", "trip")
N_NODES = 64                      # rows of every node table of the size families
ST_BAD_ID, ST_BAD_SCORE = 1, 2    # HGNN_WB_ST_*; the pair hinge reports a bad id as 1 too

MUTANTS = ("last_dropped", "group_dropped", "counted_twice", "row_b_early", "keep_ignored", "true_as_false",
           "pt_a_both", "list_truncated_16", "empty_node_unwritten", "cap_branch_flipped", "leak_from_cut")


def sizes(idt, family, per_thread=None):
    """the pair counts of one launch-edge family.  ``per_thread``: pairs per thread (default VEC[idt]; the attention
    kernels take one edge per thread, so their own edges are ``sizes(idt, family, 1)``)"""
    v = VEC[idt] if per_thread is None else per_thread
    wg = BLOCK * v
    trip = MAX_GRID * wg
    return {"tiny": TINY, "workgroup": (wg - 1, wg, wg + 1), "two_workgroups": (2 * wg - 1, 2 * wg + 1),
            "trip": (trip - 1, trip, trip + 5)}[family]


def attention_sizes(idt, family):
    """the sizes of the pair operators for this index type, and the attention kernels' own edges (one edge per thread)"""
    own = sizes(idt, family, 1)
    both = set(sizes(idt, family)) | set(own)
    if family == "two_workgroups":                # the exact share too: a power of two, so the statistics are exact
        both |= {2 * BLOCK, 2 * BLOCK * VEC[idt]}
    return tuple(sorted(both))


def hp(leak=0.25):
    return dict(HP, weight_leak=leak)


# --------------------------------------------------------------------------------------------------- pt weighting
def _p8(pt):
    """8 pt as int64 with NaN read as 0 (ptw.h: ``if (p != p) p = 0``); the grid is checked"""
    p = np.asarray(pt, np.float64)
    p = np.where(np.isnan(p), 0.0, p)
    p8 = np.rint(p * 8).astype(np.int64)
    assert np.array_equal(p8, p * 8) and p8.min(initial=0) >= 0 and p8.max(initial=0) <= 24, "pt is off the grid"
    return p8


def ptw32(pt, leak, mutant=None):
    """32 ptw(pt) as int64: 16 (weight_min) + 16 min(2 max(pt - 1/2, 0), 1) + 32 leak max(pt - 1, 0)"""
    p8 = _p8(pt)
    leak4 = int(leak * 4)
    assert leak4 == leak * 4
    ramp = 2 * np.minimum(2 * np.maximum(p8 - 4, 0), 8)
    if mutant == "cap_branch_flipped":            # heaviside(pt - cap) taken as 1 at pt == cap: multiplies z = 0
        tail = np.where(p8 >= 8, p8 - 8, 0)
    elif mutant == "leak_from_cut":               # the leak term switched on from the cut, not from the cap
        tail = np.where(p8 > 4, p8 - 8, 0)
    else:
        tail = np.maximum(p8 - 8, 0)
    return 16 + ramp + leak4 * tail


def ptw_f32(pt, leak):
    """ptw.h's ph_ptw operation by operation in numpy float32 (no contraction: every product is exact on the grid)"""
    f = np.float32
    p = np.asarray(pt, np.float32).copy()
    p[np.isnan(p)] = 0
    cut, cap = f(HP["ptcut"] - HP["pt_interval"]), f(HP["ptcut"])
    interval = f(HP["ptcut"] - (HP["ptcut"] - HP["pt_interval"]))
    x, z = p - cut, p - cap
    r = np.minimum((x > 0).astype(f) * x / interval, f(1))
    t1 = f(1.0 - HP["weight_min"]) * r
    t2 = f(leak) * (z > 0).astype(f) * z
    return (f(HP["weight_min"]) + t1) + t2, (x, z, r, t1, t2)


def pt_table(n, rng):
    """n pt values on the 1/8 grid in [0, 3]: below the cut, between cut and cap, above the cap, exactly at both,
    and NaN.  Entries 0..5 are fixed (the builders rely on them): 0 -> 0 (weight 1/2), 1 -> 3, 2 -> cut, 3 -> cap,
    4 -> 3/4, 5 -> NaN"""
    pt = (rng.integers(0, 25, n) / 8.0).astype(np.float32)
    pt[6::11] = np.nan
    fixed = (0.0, 3.0, 0.5, 1.0, 0.75, np.nan)
    pt[:len(fixed)] = fixed[:n]
    return pt


def _bad_ids(idt, n):
    return (-1, n) + ((1 << 40,) if idt is np.int64 else ((1 << 31) - 1,))


def _stream_mutation(mutant, P, idt, graph):
    """(a, b, mult) of a mutated read of the [2, P] id rows; mult: how often pair i is counted"""
    g = np.asarray(graph).astype(np.int64)
    a, b = g[0].copy(), g[1].copy()
    mult = np.ones(P, np.int64)
    if mutant == "last_dropped":
        mult[P - 1:] = 0
    elif mutant == "group_dropped":
        mult[P - P % VEC[idt]:] = 0 if P % VEC[idt] else 1
    elif mutant == "counted_twice":
        mult[P // 3:P // 3 + 1] = 2
    elif mutant == "row_b_early":
        b = g.reshape(-1)[P - 1:2 * P - 1].copy() if P else b
    return a, b, mult


# --------------------------------------------------------------------------------------------------- weighted BCE
@functools.lru_cache(maxsize=None)
def wbce_case(P, idt, seed=0, combine="sum", two_tables=False, with_keep=True, leak=0.25, planted=True):
    """one case of the weighted BCE.  ``scores``: in {0, 1} (the exact forward); ``scores_q``: in {0, 1/4, 1/2, 3/4, 1}
    (the backward).  Planted (P >= 64): ids -1, N and 2^40 (int32: 2^31 - 1), scores NaN, 1.5, -0.25.  The mutants need
    a few fixed pairs: pair 0 is (2, 0), false and kept; pair P - 1 starts in a = 1 (two tables: 4), is true and kept;
    pair P // 3 is kept; pair P - 2 is dropped (P >= 4)."""
    rng = np.random.default_rng(1000 * seed + P % 9973)
    NA = N_NODES
    NB = 48 if two_tables else NA
    pt_a = pt_table(NA, rng)
    pt_b = pt_a
    if two_tables:
        pt_b = pt_table(NB, rng)
        pt_b[0], pt_b[1] = 3.0, 0.0               # against pt_a[0] = 0, pt_a[1] = 3: the tables differ where it shows
    graph = np.stack([rng.integers(0, NA, P), rng.integers(0, NB, P)]).astype(np.int64)
    y = rng.random(P) < 0.4
    keep = rng.random(P) < 0.8
    scores = rng.integers(0, 2, P).astype(np.float32)
    scores_q = (rng.integers(0, 5, P) / 4.0).astype(np.float32)
    if P:
        graph[0, P - 1], graph[1, 0] = 1, 0
        if two_tables:
            graph[0, P - 1] = 4                   # weight 3/4 on the a side: below pt_b[0]'s, above pt_a[0]'s
        y[0], y[P - 1] = False, True
        keep[P - 1] = True
        scores[0], scores[P - 1] = 1.0, 0.0       # l = 100 on both: the loss sees these pairs
    if P >= 2:
        graph[0, 0] = 2                           # weight 1/2: under max, pair 0's weight is its b end's
        keep[0] = keep[P // 3] = True
    if P >= 4:
        keep[P - 2] = False
    if planted and P >= 64:
        for pos, v in zip((10, 21, 30), _bad_ids(idt, NA)):
            graph[pos % 2, pos] = v if pos % 2 == 0 else (NB if v == NA else v)
        for pos, v in zip((11, 22, 31), (np.nan, 1.5, -0.25)):
            scores[pos] = scores_q[pos] = v
        keep[[10, 11, 21, 22]] = True
        keep[[30, 31]] = False                    # dropped before they are looked at: no status bit from these
    return dict(op="wbce", P=P, idt=idt, graph=graph.astype(idt), y=y, keep=keep if with_keep else None,
                scores=scores, scores_q=scores_q, pt_a=pt_a, pt_b=pt_b, NA=NA, NB=NB, combine=combine,
                two_tables=two_tables, leak=leak, hp=hp(leak), grad_out=0.125)


def wbce_terms(c, scores, mutant=None):
    """dict(live, y, raw32, mult, status): which pairs take part (wbce.hip wb_pair's order: keep, ids, score)"""
    P, idt = c["P"], c["idt"]
    a, b, mult = _stream_mutation(mutant, P, idt, c["graph"])
    y = np.asarray(c["y"], bool).copy()
    keep = c["keep"]
    if mutant == "keep_ignored":
        keep = None
    if mutant == "true_as_false" and y.any():
        y[np.flatnonzero(y)[-1]] = False
    pt_a, pt_b = c["pt_a"], c["pt_b"]
    if mutant == "pt_a_both":
        pt_b = pt_a
    NA, NB = len(pt_a), len(pt_b)
    live = np.ones(P, bool) if keep is None else np.asarray(keep, bool).copy()
    live &= mult > 0
    bad_id = live & ((a < 0) | (a >= NA) | (b < 0) | (b >= NB))
    live &= ~bad_id
    s = np.asarray(scores, np.float32)
    with np.errstate(invalid="ignore"):
        bad_sc = live & ~((s >= 0) & (s <= 1))
    live &= ~bad_sc
    status = (ST_BAD_ID if bad_id.any() else 0) | (ST_BAD_SCORE if bad_sc.any() else 0)
    pm = mutant if mutant in ("cap_branch_flipped", "leak_from_cut") else None
    wa = ptw32(pt_a[np.where(live, a, 0)], c["leak"], pm)
    wb = ptw32(pt_b[np.where(live, b, 0)], c["leak"], pm)
    raw32 = np.where(live, np.maximum(wa, wb) if c["combine"] == "max" else wa + wb, 0)
    return dict(live=live, y=y, raw32=raw32, mult=mult, status=status)


def _finish(ST32, SF32, LT, LF, unit):
    """det_reduce's finish in float64: the class sums S = S32 / 32, L = L / unit, kT = 0.5 / S_T (ONE division, 0 for a
    class without weight), loss = kT L_T + kF L_F"""
    assert max(ST32, SF32, LT, LF) < 2 ** 53
    ST, SF = np.float64(ST32) / 32.0, np.float64(SF32) / 32.0
    KT = np.float64(0.5) / ST if ST > 0 else np.float64(0.0)
    KF = np.float64(0.5) / SF if SF > 0 else np.float64(0.0)
    LTf, LFf = np.float64(LT) / unit, np.float64(LF) / unit
    loss = KT * LTf + KF * LFf
    return dict(ST32=int(ST32), SF32=int(SF32), LT=int(LT), LF=int(LF), ST=float(ST), SF=float(SF), KT=float(KT),
                KF=float(KF), LTf=float(LTf), LFf=float(LFf), LOSS=float(loss))


def wbce_exact(c, mutant=None):
    """the forward on ``scores`` in {0, 1}: l = 100 where the score is on the wrong side, 0 elsewhere"""
    t = wbce_terms(c, c["scores"], mutant)
    live, y, w = t["live"], t["y"], t["raw32"] * t["mult"]
    s = np.asarray(c["scores"])
    l100 = np.where(y, s == 0, s == 1) & live
    out = _finish(w[live & y].sum(), w[live & ~y].sum(), 100 * w[l100 & y].sum(), 100 * w[l100 & ~y].sum(), 32.0)
    out.update(status=t["status"], live=live)
    return out


def wbce_grad_f32(c, KT, KF, mutant=None):
    """wbce.hip k_wb_backward on ``scores_q``, operation by operation: the quotient and the clamp in float32, the
    coefficient in float64, one rounding.  A dropped or skipped pair gets exactly 0; a pair a mutant never visits
    stays unwritten (NaN here)"""
    f = np.float32
    t = wbce_terms(c, c["scores_q"], mutant)
    s = np.asarray(c["scores_q"], f)
    yf = t["y"].astype(f)
    with np.errstate(invalid="ignore", divide="ignore"):
        quot = (s - yf) / np.maximum((f(1) - s) * s, f(1e-12))
    k = np.where(t["y"], np.float64(c["grad_out"]) * np.float64(KT), np.float64(c["grad_out"]) * np.float64(KF))
    raw = (t["raw32"] / 32.0).astype(f)
    with np.errstate(invalid="ignore", over="ignore"):
        g = ((k * raw.astype(np.float64)) * quot.astype(np.float64)).astype(f)
    g[~t["live"]] = 0
    g[t["mult"] == 0] = np.nan
    return g


# --------------------------------------------------------------------------------------------------- pair hinge
HINGE_MARGIN = {0.5: 2.0, 1.0: 3.0, 2.0: 4.0}     # scale -> margin: a false pair sits ON the margin at d = 4, 3, 2


def hinge_points(D, rng, n=N_NODES):
    """n integer points in [-3, 3]^D: node 0 the origin, then the axis points k e_j (k = 1, 2, 3, -1, -2, -3), then
    random ones.  Node 1 is e_0: the pair (1, 0) has d = 1 in every D"""
    pts = rng.integers(-3, 4, (n, D)).astype(np.int64)
    pts[0] = 0
    i = 1
    for k in (1, 2, 3, -1, -2, -3):
        for j in range(D):
            if i < min(n, 40):
                pts[i] = 0
                pts[i, j] = k
                i += 1
    return pts


def hinge_pool(pts):
    """every ordered pair (i, j), i != j, whose squared distance is a perfect square >= 1, and that distance"""
    diff = pts[:, None, :] - pts[None, :, :]
    d2 = (diff * diff).sum(-1)
    d = np.rint(np.sqrt(d2)).astype(np.int64)
    ok = (d * d == d2) & (d2 >= 1)
    i, j = np.nonzero(ok)
    return np.stack([i, j]), d[i, j]


@functools.lru_cache(maxsize=None)
def hinge_case(P, idt, D=8, seed=0, scale=1.0, leak=0.25, planted=True):
    rng = np.random.default_rng(2000 * seed + 31 * D + P % 9973)
    N = N_NODES
    pts = hinge_points(D, rng)
    pool, _ = hinge_pool(pts)
    pt = pt_table(N, rng)
    graph = pool[:, rng.integers(0, pool.shape[1], P)].astype(np.int64)
    y = rng.random(P) < 0.4
    if P:
        to0 = pool[0, pool[1] == 0]
        from1 = pool[1, pool[0] == 1]
        graph[:, 0] = (to0[rng.integers(0, len(to0))], 0)
        graph[:, P - 1] = (1, from1[rng.integers(0, len(from1))])
        if P == 1:
            graph[:, 0] = (1, 0)
        y[0], y[P - 1] = False, True
    if planted and P >= 64:
        for pos, v in zip((10, 21, 30), _bad_ids(idt, N)):
            graph[pos % 2, pos] = v
    return dict(op="hinge", P=P, idt=idt, D=D, N=N, E=pts.astype(np.float32), pts=pts, graph=graph.astype(idt), y=y,
                pt=pt, scale=scale, margin=HINGE_MARGIN[scale], leak=leak, hp=hp(leak), grad_out=0.25)


def hinge_terms(c, mutant=None):
    """dict(live, y, raw32, mult, status, a, b, d2, d, l2): d2 the integer squared distance, d its integer root (-1
    off the grid: only a mutant gets there), l2 = 2 l"""
    P, idt, N = c["P"], c["idt"], c["N"]
    a, b, mult = _stream_mutation(mutant, P, idt, c["graph"])
    y = np.asarray(c["y"], bool).copy()
    if mutant == "true_as_false" and y.any():
        y[np.flatnonzero(y)[-1]] = False
    live = (mult > 0) & ~((a < 0) | (a >= N) | (b < 0) | (b >= N))
    status = 1 if ((mult > 0) & ~live).any() else 0
    sa, sb = np.where(live, a, 0), np.where(live, b, 0)
    pm = mutant if mutant in ("cap_branch_flipped", "leak_from_cut") else None
    raw32 = np.where(live, ptw32(c["pt"][sa], c["leak"], pm) + ptw32(c["pt"][sb], c["leak"], pm), 0)
    table = c["pts"][:, None, :] - c["pts"][None, :, :]               # N x N: the pairs only index it
    d2 = (table * table).sum(-1)[sa, sb]
    d = np.rint(np.sqrt(d2)).astype(np.int64)
    d = np.where((d * d == d2) & (d2 >= 1), d, -1)
    s2 = int(2 * c["scale"])
    m2 = int(2 * c["margin"])
    assert s2 == 2 * c["scale"] and m2 == 2 * c["margin"]
    l2 = np.where(y, s2 * d, np.maximum(m2 - s2 * d, 0))
    return dict(live=live, y=y, raw32=raw32, mult=mult, status=status, a=sa, b=sb, d2=d2, d=d, l2=l2)


def hinge_exact(c, mutant=None):
    """the forward: sums of raw in 1/32, of raw l^2 in 1/128.  Off the grid (mutants only) l comes from float64"""
    t = hinge_terms(c, mutant)
    live, y, w = t["live"], t["y"], t["raw32"] * t["mult"]
    on_grid = bool((t["d"][live] >= 1).all())
    if on_grid:
        rl = w * t["l2"] * t["l2"]
    else:
        assert mutant is not None, "a case of the exact family holds a pair off the grid"
        d = np.sqrt(t["d2"].astype(np.float64) + 1e-12)
        td = c["scale"] * d
        ell = np.where(y, td, np.maximum(c["margin"] - td, 0.0))
        rl = np.rint(w * 4 * ell * ell * 1024).astype(np.int64)     # mutants: any value that differs will do
    out = _finish(w[live & y].sum(), w[live & ~y].sum(), rl[live & y].sum(), rl[live & ~y].sum(), 128.0)
    out.update(status=t["status"], on_grid=on_grid, live=live)
    return out


def hinge_coef(c, KT, KF, mutant=None):
    """pairloss.hip k_ph_coef in float64 (every value is a short dyadic on the backward grid, so float64 is exact):
    c_i = 2 g kT scale^2 raw (true), -2 g kF scale raw l / d for a false pair inside the margin, else 0"""
    t = hinge_terms(c, mutant)
    g2 = 2.0 * c["grad_out"]
    raw = t["raw32"] / 32.0
    d = np.where(t["d"] >= 1, t["d"], 1).astype(np.float64)
    ell = c["margin"] - c["scale"] * d
    cf = np.where(t["y"], g2 * KT * c["scale"] * c["scale"] * raw,
                  np.where(ell > 0, -g2 * KF * c["scale"] * raw * ell / d, 0.0))
    cf = np.where(t["live"], cf, 0.0)
    return cf, t


def hinge_lists(c):
    """for every node its list in the plan's order (stable by position in cat(a, b)): (position in cat, pair, other)"""
    g = np.asarray(c["graph"]).astype(np.int64)
    P, N = c["P"], c["N"]
    dst = np.concatenate([g[0], g[1]])
    oth = np.concatenate([g[1], g[0]])
    valid = (dst >= 0) & (dst < N) & (oth >= 0) & (oth < N)
    pos = np.flatnonzero(valid)
    order = pos[np.argsort(dst[pos], kind="stable")]
    return dst[order], order % P if P else order, oth[order]


def hinge_grad_exact(c, KT, KF, mutant=None):
    """grad_E [N, D] in float64: grad[v] = sum over v's list of c_i (E[v] - E[o]).  ``list_truncated_16``: only the
    first 16 (n // 16) entries of each list; ``empty_node_unwritten``: a node without pairs keeps NaN"""
    cf, _ = hinge_coef(c, KT, KF, mutant if mutant not in ("list_truncated_16", "empty_node_unwritten") else None)
    v, pair, o = hinge_lists(c)
    N, D = c["N"], c["D"]
    use = np.ones(len(v), bool)
    counts = np.bincount(v, minlength=N)
    if mutant == "list_truncated_16":
        start = np.concatenate([[0], np.cumsum(counts)])[:-1]
        rank = np.arange(len(v)) - start[v]
        use = rank < 16 * (counts[v] // 16)
    E = c["pts"].astype(np.float64)
    term = cf[pair][:, None] * (E[v] - E[o])
    term[(o == v) | ~use] = 0
    grad = np.zeros((N, D), np.float64)
    for k in range(D):
        grad[:, k] = np.bincount(v, weights=term[:, k], minlength=N)
    if mutant == "empty_node_unwritten":
        grad[counts == 0] = np.nan
    return grad, term, v


def hinge_grad_is_exact(c, KT, KF):
    """True if float32 sums of every node's terms are exact in ANY order: all terms of a node are multiples of one
    quantum q (a power of two) and sum |term| < 2^24 q, so every partial sum is a multiple of q below 2^24 q"""
    _, term, v = hinge_grad_exact(c, KT, KF)
    if term.size == 0:
        return True
    scaled = term * 2.0 ** 60
    ints = np.rint(scaled)
    if not np.array_equal(ints, scaled) or np.abs(scaled).max(initial=0) >= 2.0 ** 62:
        return False
    ints = np.abs(ints.astype(np.int64))
    for node in np.unique(v):
        t = ints[v == node]
        nz = t[t > 0]
        if nz.size == 0:
            continue
        q = int(np.bitwise_or.reduce(nz.reshape(-1)))
        q &= -q                                                       # the lowest set bit of all terms
        if int(t.sum(axis=0).max()) >= (1 << 24) * q:
            return False
    return True


CENSUS = (1, 15, 16, 17, 32, 33)       # list entries of the census nodes; one more node has none
HINGE_BWD = {1.0: 3.0, 2.0: 4.0, 0.5: 2.0}


@functools.lru_cache(maxsize=None)
def hinge_backward_case(D, idt, seed=0, scale=1.0, n_flex=600, odd=True):
    """the backward grid.  Node 0 (the origin) is the hub.  Census nodes: axis points whose only pairs are with the
    hub, CENSUS[i] of them each; node N - 1 has no pair.  The other pairs are drawn so that each class's raw sum is a
    power of two (``top up``: 8 ptw is 2..5 per node, a pair gives 4..10, so n pairs reach every total in [4n, 10n])
    and every false pair inside the margin has d in {1, 2, 4}.  P = 114 + 2 n_flex + odd."""
    rng = np.random.default_rng(3000 * seed + D)
    N, leak = N_NODES, 0.25
    pts = hinge_points(D, rng)
    margin = HINGE_BWD[scale]
    pt = np.asarray([(0.0, 0.75, 1.0, 2.0)[i] for i in rng.integers(0, 4, N)], np.float32)
    pt[5::9] = np.nan
    pt[2], pt[3] = 0.5, 1.0
    w8 = ptw32(pt, leak) // 8
    assert np.array_equal(w8 * 8, ptw32(pt, leak)) and w8.min() >= 2 and w8.max() <= 5
    n_axis = min(6 * D, 39)
    axis = np.arange(1, 1 + n_axis)
    dist0 = np.abs(pts[axis]).sum(-1)                               # an axis point's distance from the hub
    ok = axis[(scale * dist0 >= margin) | np.isin(dist0, (1, 2, 4))]
    assert len(ok) >= len(CENSUS), "too few axis points for the census at this D and scale"
    census, counts = ok[:len(CENSUS)], CENSUS
    free = np.setdiff1d(np.arange(N - 1), census)                   # the hub among them; N - 1 stays empty
    pool, pool_d = hinge_pool(pts)
    keep = np.isin(pool[0], free) & np.isin(pool[1], free)
    pool, pool_d = pool[:, keep], pool_d[keep]
    contrib = w8[pool[0]] + w8[pool[1]]
    inside_ok = (scale * pool_d >= margin) | np.isin(pool_d, (1, 2, 4))
    pairs, ys = [], []
    for node, n in zip(census, counts):
        for i in range(n):
            pairs.append((node, 0) if i % 2 else (0, node))
            ys.append((i + int(node)) % 2 == 0)
    pairs, ys = np.asarray(pairs, np.int64).reshape(-1, 2), np.asarray(ys, bool)
    out_pairs, out_y = [pairs], [ys]
    for cls, n in ((True, n_flex), (False, n_flex + int(odd))):
        fixed = int((w8[pairs[ys == cls, 0]] + w8[pairs[ys == cls, 1]]).sum())
        target = 1 << int(math.floor(math.log2(fixed + 10 * n)))
        assert target >= fixed + 4 * n, "no power of two within reach of the top-up"
        q, r = divmod(target - fixed - 4 * n, n)
        want = np.full(n, 4 + q)
        want[:r] += 1
        rng.shuffle(want)
        sel = np.empty(n, np.int64)
        for cval in np.unique(want):
            cand = np.flatnonzero((contrib == cval) & (inside_ok | cls))
            hub = cand[(pool[0, cand] == 0) | (pool[1, cand] == 0)]
            assert cand.size, f"no pair of weight {cval} in the pool"
            m = want == cval
            pick = cand[rng.integers(0, cand.size, int(m.sum()))]
            if hub.size:                                              # every second one at the hub: a long list
                pick[::2] = hub[rng.integers(0, hub.size, len(pick[::2]))]
            sel[m] = pick
        out_pairs.append(pool[:, sel].T)
        out_y.append(np.full(n, cls))
    pairs, ys = np.concatenate(out_pairs), np.concatenate(out_y)
    perm = rng.permutation(len(ys))
    graph = pairs[perm].T.copy()
    return dict(op="hinge", P=graph.shape[1], idt=idt, D=D, N=N, E=pts.astype(np.float32), pts=pts,
                graph=graph.astype(idt), y=ys[perm], pt=pt, scale=scale, margin=margin, leak=leak, hp=hp(leak),
                grad_out=0.25, census=dict(zip((int(x) for x in census), counts)), empty=N - 1, hub=0)


# --------------------------------------------------------------------------------------------------- attention
@functools.lru_cache(maxsize=None)
def attn_case(E, idt, D=8, seed=0, training=None, fn="sigmoid", norm=True, momentum=0.25):
    """integer rows (in [-3, 3]; in [-1, 1] from 4096 edges on, where sum x^2 must leave room in the 53 bits).
    training defaults to "E is a power of two >= 2".  Dyadic BatchNorm state: running_mean 0.5, running_var 1024
    (eval mode: |z| stays below 7 for every integer x the rows can give, so exp does not overflow),
    num_batches_tracked 3, so that the cumulative average (momentum None) is 1 / 4 as well"""
    rng = np.random.default_rng(4000 * seed + 17 * D + E % 9973)
    Na, Nb = N_NODES, 48
    lim = 3 if E < 4096 else 1
    A = rng.integers(-lim, lim + 1, (Na, D)).astype(np.int64)
    B = rng.integers(-lim, lim + 1, (Nb, D)).astype(np.int64)
    A[1], B[0], B[1] = 1, 1, -1
    graph = np.stack([rng.integers(0, Na, E), rng.integers(0, Nb, E)]).astype(np.int64)
    if E:
        graph[0, E - 1], graph[1, 0] = 1, 0
    if E == 1:
        graph[:, 0] = (1, 0)
    if E >= 2:
        graph[:, E // 3 if E > 2 else 1] = (1, 1)     # x = -D there: counting that edge twice shows in the statistics
    if E >= 64:
        graph[0, 10], graph[1, 21] = -1, Nb           # x = 0 for an id out of range: no address is formed from it
    if training is None:
        training = E >= 2 and E & (E - 1) == 0
    return dict(op="attn", P=E, idt=idt, D=D, Na=Na, Nb=Nb, A=A, B=B, graph=graph.astype(idt), training=training,
                fn=fn, norm=norm, momentum=momentum, eps=1e-5, gamma=1.5, beta=-0.25, running_mean=0.5,
                running_var=1024.0, nbt=3)


def attn_exact(c, mutant=None):
    """x (int64), and in training mode the exact statistics: MEAN, VAR (float64, exactness asserted by the CPU test
    through ``fractions``), the running statistics after the header's one float32 rounding, num_batches_tracked"""
    E = c["P"]
    a, b, mult = _stream_mutation(mutant, E, c["idt"], c["graph"])
    live = (a >= 0) & (a < c["Na"]) & (b >= 0) & (b < c["Nb"])
    x = np.where(live, (c["A"][np.where(live, a, 0)] * c["B"][np.where(live, b, 0)]).sum(-1), 0)
    out = dict(x=x, mult=mult, E=E)
    if c["training"]:
        sx, sxx = int((x * mult).sum()), int((x * x * mult).sum())
        n = np.float64(E)
        mu = np.float64(sx) / n
        var = max(np.float64(sxx) / n - mu * mu, np.float64(0.0))
        m = np.float64(c["momentum"] if c["momentum"] is not None else 1.0 / (c["nbt"] + 1))
        rm = np.float32((1.0 - m) * np.float64(c["running_mean"]) + m * mu)
        rv = np.float32((1.0 - m) * np.float64(c["running_var"]) + m * (var * n / (n - 1.0)))
        out.update(sx=sx, sxx=sxx, MEAN=float(mu), VAR=float(var), running_mean=rm, running_var=rv, nbt=c["nbt"] + 1)
    else:
        out.update(MEAN=float(np.float32(c["running_mean"])), VAR=float(np.float32(c["running_var"])),
                   running_mean=np.float32(c["running_mean"]), running_var=np.float32(c["running_var"]),
                   nbt=c["nbt"])
    return out


# --------------------------------------------------------------------------------------------------- mutants
def applies(mutant, c):
    """whether a reference mutant can show on this case at all"""
    P, op = c["P"], c["op"]
    if mutant == "counted_twice":
        return P >= 1 and (op != "attn" or c["training"])
    if mutant in ("last_dropped", "row_b_early"):
        return P >= 1
    if mutant == "group_dropped":
        return op != "attn" and P % VEC[c["idt"]] != 0
    if mutant == "keep_ignored":
        return op == "wbce" and c["keep"] is not None and P >= 4
    if mutant == "true_as_false":
        return op != "attn" and P >= 1
    if mutant == "pt_a_both":
        return op == "wbce" and c["two_tables"] and c["combine"] == "max" and P >= 1
    if mutant in ("list_truncated_16", "empty_node_unwritten"):
        return op == "hinge" and "census" in c
    if mutant == "leak_from_cut":
        return op != "attn" and P >= 64 and c["leak"] != 0
    return False                                  # cap_branch_flipped: ptw is continuous at the cap, see the CPU test


def asserted(c, mutant=None, backward=True):
    """the tuple of everything the GPU test asserts on bits for this case, under a reference mutant (``backward``
    False: of the forward alone, which is cheaper and often enough to tell a mutant)"""
    if c["op"] == "wbce":
        r = wbce_exact(c, mutant)
        out = (r["ST32"], r["SF32"], r["LT"], r["LF"], r["status"])
        return out + (wbce_grad_f32(c, r["KT"], r["KF"], mutant).tobytes(),) if backward else out
    if c["op"] == "hinge":
        r = hinge_exact(c, mutant)
        out = (r["ST32"], r["SF32"], r["LT"], r["LF"], r["status"])
        if "census" in c and backward:
            out += (hinge_grad_exact(c, r["KT"], r["KF"], mutant)[0].tobytes(),)
        return out
    r = attn_exact(c, mutant)
    return (r["x"].tobytes(), r["MEAN"], r["VAR"], np.where(r["mult"] > 0, r["x"], -999).tobytes())


# --------------------------------------------------------------------------------------------------- case lists
OPS = ("wbce", "hinge", "attn")
_WB_MODES = (("sum", False, True), ("max", True, True), ("sum", True, False), ("max", False, True))
_SCALES = (1.0, 0.5, 2.0)


def cases(op, idt, family):
    """the cases of one size family: the modes (BCE), D and scale (pair hinge), D, function and norm (attention) are
    taken in turn, so that every family meets each of them"""
    out = []
    ps = attention_sizes(idt, family) if op == "attn" else sizes(idt, family)
    for i, P in enumerate(ps):
        if op == "wbce":
            combine, two, with_keep = _WB_MODES[i % 4]
            out.append(wbce_case(P, idt, seed=1, combine=combine, two_tables=two, with_keep=with_keep,
                                 leak=(0.25, 1.0, 0.0)[i % 3]))
        elif op == "hinge":
            out.append(hinge_case(P, idt, D=DIMS[(i + FAMILIES.index(family)) % len(DIMS)], seed=1,
                                  scale=_SCALES[i % 3], leak=(0.25, 1.0, 0.0)[i % 3]))
        else:
            out.append(attn_case(P, idt, D=DIMS[(i + 2 * FAMILIES.index(family)) % len(DIMS)], seed=1,
                                 fn=("sigmoid", "exp")[i % 2], norm=i % 3 != 1,
                                 momentum=None if i % 2 else 0.25))
    return out


def name(c):
    idt = "i32" if c["idt"] is np.int32 else "i64"
    if c["op"] == "wbce":
        return (f"wbce P={c['P']} {idt} {c['combine']} tables={1 + c['two_tables']} "
                f"keep={c['keep'] is not None} leak={c['leak']}")
    if c["op"] == "hinge":
        return f"hinge P={c['P']} {idt} D={c['D']} scale={c['scale']} margin={c['margin']} leak={c['leak']}"
    return f"attn E={c['P']} {idt} D={c['D']} train={c['training']} {c['fn']} norm={c['norm']}"


def backward_cases(idt):
    """the exact backward cases of the pair hinge: every D, the three scales in turn (D = 1: scale 1, the line has too
    few axis points for the census at scale 0.5)"""
    return [hinge_backward_case(D, idt, seed=1, scale=1.0 if D == 1 else _SCALES[i % 3])
            for i, D in enumerate(DIMS)]
