"""CPU restatement (numpy) of the reference's eval_metrics (Modules/tracking_utils.py:18-83) for the tracking
tests: the contract csrc/trackeval.hip implements, written out step by step.  Not collected by pytest.

track_eval(...) returns a dict with the four metrics, the counts behind them and ``no_match`` (the reference's
default_response).  Numerics as in DESIGN.md section 3 "Tracking metrics": the candidate size filter and the pt
cut compare in float32, everything after the contingency table in float64.
"""
import numpy as np

KEYS = ("track_eff", "track_pur", "hit_eff", "hit_pur")
# wrong readings of the contract, for tests/test_tracking_exact_ref.py: the six comparisons with the other sign, the
# hash tie to the lower label, duplicate pairs counted once, the size filter compared in float64
MUTANTS = ("size_gt", "col_gt", "row_gt", "kept_ge", "pt_ge", "nhits_gt", "tie_low", "dup_once", "size_f64")


def cluster_hash(C: int) -> np.ndarray:
    """numpy.linspace(1, 1 + 1e-12, C), restated: h_c = fl(fl(c * (delta / (C - 1))) + 1), h_{C-1} = stop"""
    stop = 1 + 1e-12
    if C == 1:
        return np.ones(1)
    delta = stop - 1.0
    step = delta / (C - 1)
    h = np.arange(C, dtype=np.float64) * step
    h += 1.0
    h[-1] = stop
    return h


def _default(C, P, n_match=0, n_kept=0):
    return dict(track_eff=0, track_pur=0, hit_eff=0, hit_pur=0, no_match=True, n_kept=n_kept, n_mask=0,
                n_truth=0, n_cand=C, n_part=P, n_match=n_match)


def track_eval(hit, cand, pid, pt, primary=None, pt_cut=1.0, nhits_cut=5, majority_cut=0.5, mutant=None):
    """primary: None (the reference's primary=False) or per-hit flags (primary=True).  A particle with a NaN pt has
    ptmin = NaN (np.minimum propagates it, as torch's amin does in the fixture generator) and is not
    reconstructable.  ``mutant``: one of MUTANTS (tests only)"""
    assert mutant is None or mutant in MUTANTS
    hit, cand = np.asarray(hit, np.int64), np.asarray(cand, np.int64)
    pid, pt = np.asarray(pid, np.int64), np.asarray(pt, np.float32)
    if hit.size and (hit.min() < 0 or hit.max() >= pid.size):
        raise ValueError("hit id out of range")
    # 1. candidate size filter (float32 comparison), dense relabel in ascending label order
    if hit.size and mutant == "dup_once":
        pairs = np.unique(np.stack([hit, cand], 1), axis=0)
        hit, cand = pairs[:, 0], pairs[:, 1]
    if hit.size:
        _, inv, cnt = np.unique(cand, return_inverse=True, return_counts=True)
        if mutant == "size_f64":
            keep = cnt[inv].astype(np.float64) >= nhits_cut * majority_cut
        elif mutant == "size_gt":
            keep = cnt[inv].astype(np.float32) > np.float32(nhits_cut * majority_cut)
        else:
            keep = cnt[inv].astype(np.float32) >= np.float32(nhits_cut * majority_cut)
        hit, cand = hit[keep], cand[keep]
    # 2. particles
    opid, p_of_hit, nhits = np.unique(pid, return_inverse=True, return_counts=True)
    P = opid.size
    if hit.size == 0:
        return _default(0, P)
    _, c_of_pair = np.unique(cand, return_inverse=True)
    C = int(c_of_pair.max()) + 1
    ptmin = np.full(P, np.inf, np.float32)
    with np.errstate(invalid="ignore"):
        np.minimum.at(ptmin, p_of_hit, pt)        # propagates NaN
    prim = np.zeros(P, bool)
    if primary is not None:
        prim[p_of_hit[np.asarray(primary) != 0]] = True
    # 3. contingency triples in row-major order; duplicates count
    key = p_of_hit[hit].astype(np.int64) * C + c_of_pair
    uk, n = np.unique(key, return_counts=True)
    rows, cols, n = uk // C, uk % C, n.astype(np.float64)
    col = np.bincount(c_of_pair, minlength=C).astype(np.float64)
    # 4-5. hashing tie-break and matching
    nh = n * (cluster_hash(C)[::-1] if mutant == "tie_low" else cluster_hash(C))[cols]
    rowmax = np.zeros(P)
    np.maximum.at(rowmax, rows, nh)
    nhits_f = nhits.astype(np.float64)
    by_col = n > majority_cut * col[cols] if mutant == "col_gt" else n >= majority_cut * col[cols]
    by_row = n > majority_cut * nhits_f[rows] if mutant == "row_gt" else n >= majority_cut * nhits_f[rows]
    match = by_col & by_row & (nh == rowmax[rows])
    n_match = int(match.sum())
    if n_match == 0:
        return _default(C, P)
    mr, mc, mn = rows[match], cols[match], n[match]
    # 6. match filter
    big = mn >= majority_cut * nhits_cut if mutant == "kept_ge" else mn > majority_cut * nhits_cut
    kf = big & (opid[mr] != 0)
    n_kept = int(kf.sum())
    if n_kept == 0:
        return _default(C, P, n_match)
    kr, kc, kn = mr[kf], mc[kf], mn[kf]
    # 7. metrics
    above = ptmin >= np.float32(pt_cut) if mutant == "pt_ge" else ptmin > np.float32(pt_cut)
    truth = above & (nhits > nhits_cut if mutant == "nhits_gt" else nhits >= nhits_cut)
    mask = truth[kr]
    if primary is not None:
        mask &= prim[kr]
        truth &= prim
    n_mask, n_truth = int(mask.sum()), int(truth.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        track_eff = np.float64(n_mask) / np.float64(n_truth)
        track_pur = np.float64(n_mask) / np.float64(C - (n_match - n_kept) - (n_kept - n_mask))
        hit_pur = np.sum(kn / col[kc]) / np.float64(n_kept)
        hit_eff = np.sum(kn[mask] / nhits_f[kr][mask]) / np.float64(n_mask)
    return dict(track_eff=float(track_eff), track_pur=float(track_pur), hit_eff=float(hit_eff),
                hit_pur=float(hit_pur), no_match=False, n_kept=n_kept, n_mask=n_mask, n_truth=n_truth,
                n_cand=C, n_part=P, n_match=n_match)


def same(a: float, b: float, rel: float = 0.0) -> bool:
    """equal (nan == nan), or within `rel` relative difference"""
    a, b = float(a), float(b)
    if np.isnan(a) or np.isnan(b):
        return np.isnan(a) and np.isnan(b)
    if np.isinf(a) or np.isinf(b) or rel == 0.0:
        return a == b
    return abs(a - b) <= rel * max(abs(a), abs(b))
