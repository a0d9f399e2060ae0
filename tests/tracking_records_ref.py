"""CPU restatement (numpy) of hgnn_track_records (csrc/trackeval_records.hip) for the tracking-records tests: the
steps of tests/tracking_ref.py, keeping the per-row (particle) and per-column (candidate) results and the binned
counts.  Not collected by pytest.

track_records(...) returns
  scalars     what tracking_ref.track_eval returns for the same inputs (its default on a no_match case)
  totals      the true integer sums P, n_truth, n_kept, n_mask, n_match, C behind the tables (on a no_match case
              tracking_ref defines no n_mask / n_truth; the tables always do)
  particles   {field: array[P]} in ascending pid; ``values`` is float32 [V, P]
  candidates  {field: array[C]} in ascending label
  hist        int64 [V, 66, 6]: slot = np.searchsorted(np.float32(edges), values, "right"), columns as BIN_COLUMNS
Also here: the two cases the exact-case set lacks (a hash collision that keeps two matches of one particle, two
particles holding one candidate), a 257-candidate case, and the binning variables every test uses for a case.
"""
import numpy as np

import tracking_exact_cases as X
import tracking_ref as T

MUTANTS = ("slot_left", "nan_skip")        # wrong readings of the slot rule and of the values reduction
BIN_COLUMNS = ("particles", "reconstructable", "n_kept", "n_mask", "masked_shared", "masked_nhits")
MAX_BINS = 64
PARTICLE_FIELDS = dict(pid=np.int64, nhits=np.int32, pt=np.float32, primary=np.uint8, reconstructable=np.uint8,
                       n_match=np.int32, n_kept=np.int32, n_mask=np.int32, cand_index=np.int32, shared=np.int32)
CANDIDATE_FIELDS = dict(label=np.int64, size=np.int32, n_kept=np.int32, n_mask=np.int32, particle=np.int32,
                        shared=np.int32)


def _nan_min(P, p_of_hit, x, skip_nan=False):
    """per-particle minimum of float32 x in which a NaN wins (np.minimum propagates it); skip_nan: the mutant.
    Which zero a minimum of 0.0 and -0.0 is depends on the order in numpy; the contract says -0.0 (the minimum of
    the total order), so the bits are defined"""
    x = np.asarray(x, np.float32)
    m = np.full(P, np.inf, np.float32)
    with np.errstate(invalid="ignore"):
        (np.fmin if skip_nan else np.minimum).at(m, p_of_hit, x)
    has_neg_zero = np.bincount(p_of_hit[(x == 0) & np.signbit(x)], minlength=P) > 0
    m[m == 0] = 0.0
    m[(m == 0) & has_neg_zero] = -0.0
    return m


def _first_by(group, n_groups, other, n):
    """for every group the smallest ``other`` among its entries and that entry's n, or (-1, 0)"""
    first = np.full(n_groups, -1, np.int64)
    shared = np.zeros(n_groups, np.int64)
    order = np.lexsort((other, group))
    g, o, nn = group[order], other[order], n[order]
    head = np.ones(g.size, bool)
    head[1:] = g[1:] != g[:-1]
    first[g[head]] = o[head]
    shared[g[head]] = nn[head]
    return first, shared


def track_records(hit, cand, pid, pt, primary=None, pt_cut=1.0, nhits_cut=5, majority_cut=0.5, values=None,
                  edges=(), mutant=None):
    """values: float32 [V, N] per-hit binning variables (or None), edges: V ascending sequences"""
    assert mutant is None or mutant in MUTANTS
    hit, cand = np.asarray(hit, np.int64), np.asarray(cand, np.int64)
    pid, pt = np.asarray(pid, np.int64), np.asarray(pt, np.float32)
    values = np.zeros((0, pid.size), np.float32) if values is None else np.asarray(values, np.float32)
    V = values.shape[0]
    assert V == len(edges) and values.shape[1:] == pid.shape
    if hit.size and (hit.min() < 0 or hit.max() >= pid.size):
        raise ValueError("hit id out of range")
    # 1. candidate size filter (float32 comparison), dense relabel in ascending label order
    if hit.size:
        _, inv, cnt = np.unique(cand, return_inverse=True, return_counts=True)
        keep = cnt[inv].astype(np.float32) >= np.float32(nhits_cut * majority_cut)
        hit, cand = hit[keep], cand[keep]
    label, c_of_pair, size = np.unique(cand, return_inverse=True, return_counts=True)
    C = label.size
    # 2. particles
    opid, p_of_hit, nhits = np.unique(pid, return_inverse=True, return_counts=True)
    P = opid.size
    ptmin = _nan_min(P, p_of_hit, pt)
    pvalues = np.stack([_nan_min(P, p_of_hit, values[v], mutant == "nan_skip") for v in range(V)]) if V else \
        np.zeros((0, P), np.float32)
    prim = np.zeros(P, bool)
    if primary is not None:
        prim[p_of_hit[np.asarray(primary) != 0]] = True
    with np.errstate(invalid="ignore"):
        recon = (ptmin > np.float32(pt_cut)) & (nhits >= nhits_cut)
    if primary is not None:
        recon &= prim
    # 3. contingency triples in row-major order; duplicates count
    if C:
        uk, n = np.unique(p_of_hit[hit].astype(np.int64) * C + c_of_pair, return_counts=True)
        rows, cols = uk // C, uk % C
        nf = n.astype(np.float64)
        col = size.astype(np.float64)
        # 4-5. hashing tie-break and matching
        nh = nf * T.cluster_hash(C)[cols]
        rowmax = np.zeros(P)
        np.maximum.at(rowmax, rows, nh)
        match = (nf >= majority_cut * col[cols]) & (nf >= majority_cut * nhits.astype(np.float64)[rows]) & \
            (nh == rowmax[rows])
        # 6. match filter, 7. mask
        kept = match & (nf > majority_cut * nhits_cut) & (opid[rows] != 0)
        mask = kept & recon[rows]
    else:
        rows = cols = n = np.zeros(0, np.int64)
        match = kept = mask = np.zeros(0, bool)
    cnt_p = lambda sel, w=None: np.bincount(rows[sel], None if w is None else w[sel], minlength=P).astype(np.int64)  # noqa: E731
    cnt_c = lambda sel: np.bincount(cols[sel], minlength=C).astype(np.int64)  # noqa: E731
    cand_index, p_shared = _first_by(rows[kept], P, cols[kept], n[kept])
    particle, c_shared = _first_by(cols[kept], C, rows[kept], n[kept])
    particles = dict(pid=opid, nhits=nhits, pt=ptmin, primary=prim, reconstructable=recon, n_match=cnt_p(match),
                     n_kept=cnt_p(kept), n_mask=cnt_p(mask), cand_index=cand_index, shared=p_shared)
    particles = {k: np.asarray(v).astype(PARTICLE_FIELDS[k]) for k, v in particles.items()}
    particles["values"] = pvalues
    candidates = dict(label=label, size=size, n_kept=cnt_c(kept), n_mask=cnt_c(mask), particle=particle,
                      shared=c_shared)
    candidates = {k: np.asarray(v).astype(CANDIDATE_FIELDS[k]) for k, v in candidates.items()}
    # binned counts
    masked_shared = cnt_p(mask, n)
    per_particle = np.stack([np.ones(P, np.int64), recon.astype(np.int64), particles["n_kept"].astype(np.int64),
                             particles["n_mask"].astype(np.int64), masked_shared,
                             nhits.astype(np.int64) * particles["n_mask"]], 1)
    hist = np.zeros((V, MAX_BINS + 2, len(BIN_COLUMNS)), np.int64)
    for v in range(V):
        e = np.asarray(edges[v], np.float64).astype(np.float32)
        assert 2 <= e.size <= MAX_BINS + 1 and np.all(np.isfinite(e)) and np.all(e[1:] > e[:-1])
        slot = np.searchsorted(e, pvalues[v], "left" if mutant == "slot_left" else "right")
        np.add.at(hist[v], slot, per_particle)
    totals = dict(n_part=P, n_cand=C, n_truth=int(recon.sum()), n_match=int(match.sum()), n_kept=int(kept.sum()),
                  n_mask=int(mask.sum()))
    # the scalars, from the tables' own sums, with tracking_ref's early returns
    if totals["n_match"] == 0 or totals["n_kept"] == 0:
        scalars = T._default(C, P, totals["n_match"] if C else 0, 0)
    else:
        t = totals
        with np.errstate(divide="ignore", invalid="ignore"):
            scalars = dict(
                track_eff=float(np.float64(t["n_mask"]) / np.float64(t["n_truth"])),
                track_pur=float(np.float64(t["n_mask"]) /
                                np.float64(C - (t["n_match"] - t["n_kept"]) - (t["n_kept"] - t["n_mask"]))),
                hit_eff=float(np.sum(nf[mask] / nhits.astype(np.float64)[rows[mask]]) / np.float64(t["n_mask"])),
                hit_pur=float(np.sum(nf[kept] / col[cols[kept]]) / np.float64(t["n_kept"])),
                no_match=False, n_kept=t["n_kept"], n_mask=t["n_mask"], n_truth=t["n_truth"], n_cand=C, n_part=P,
                n_match=t["n_match"])
    return dict(scalars=scalars, totals=totals, particles=particles, candidates=candidates, hist=hist)


# ---------------------------------------------------------------------------------------------- the added cases
def collision_case():
    """C = 8193 kept candidates with labels 0 .. C - 1 (dense index = label).  c0 is the first index whose hash
    equals its neighbour's; one particle of four hits has two in c0 and two in c0 + 1, majority_cut = 0.5: both
    triples have n * h == rowmax, both are matches and kept.  Terms 2/2 and 2/4 are dyadic."""
    C = 8193
    h = T.cluster_hash(C)
    same = np.flatnonzero(h[:-2] == h[1:-1])
    assert same.size
    c0 = int(same[0])
    ev = X.Event()
    split = ev.particle(70001, 4)
    for c in range(C):
        if c == c0:
            ev.pairs(split[:2], c)
        elif c == c0 + 1:
            ev.pairs(split[2:], c)
        else:
            ev.pairs(ev.particle(c + 1, 1), c)
    case = ev.case("records_hash_collision", "records", 8193, nhits_cut=1)
    return dict(case, c0=c0, split_pid=70001)


def shared_candidate_case():
    """two particles of two hits each hold exactly half of one candidate of four pairs, majority_cut = 0.5"""
    ev = X.Event()
    X._background(ev, nh=2)
    a, b = ev.particle(41, 2), ev.particle(43, 2)
    ev.pairs(list(a) + list(b), 7)
    return dict(ev.case("records_shared_candidate", "records", 2, nhits_cut=1), label=7, pids=(41, 43))


def many_candidates_case(C=257):
    """C kept candidates, one particle of two hits each: one block of the per-candidate kernels and one thread"""
    ev = X.Event()
    for c in range(C):
        ev.pairs(ev.particle(c + 1, 2, pt=(2.0, 0.5)[c % 2]), 3 * c - C)
    return ev.case(f"records_cands_{C}", "records", C, nhits_cut=1)


def _extra():
    out = {}
    for c in (collision_case(), shared_candidate_case(), many_candidates_case()):
        out[c["name"]] = c
    return out


EXTRA = _extra()
CASES = dict(X.CASES, **EXTRA)
NAMES = tuple(CASES)

PT_EDGES = (0.0, 0.5, 1.0, 2.0, 4.0)                     # the cases' pt values sit exactly on these
ETA_EDGES = tuple(np.linspace(-2.0, 2.0, 21))


def case_bins(case):
    """the binning variables the tests use for a case: ``pt`` itself against edges its values sit on, and ``eta``,
    seeded normal values rounded to eighths (so many sit on an edge) with a NaN and an infinity in some hits.
    Returns (names, float32 [2, N] values, edges)"""
    N = case["pid"].size
    rng = np.random.default_rng(7 + N)
    eta = (np.round(rng.normal(0.0, 1.2, N) * 8) / 8).astype(np.float32)
    eta[rng.random(N) < 0.08] = np.nan
    eta[rng.random(N) < 0.03] = np.inf
    eta[rng.random(N) < 0.03] = -np.inf
    return ("pt", "eta"), np.stack([case["pt"].astype(np.float32), eta]), (PT_EDGES, ETA_EDGES)


def restate(case, use_primary, with_bins=True, mutant=None):
    _, values, edges = case_bins(case)
    with np.errstate(all="ignore"):
        return track_records(case["hit"], case["cand"], case["pid"], case["pt"],
                             case["primary"] if use_primary else None, case["pt_cut"], case["nhits_cut"],
                             case["majority_cut"], values if with_bins else None, edges if with_bins else (),
                             mutant=mutant)
