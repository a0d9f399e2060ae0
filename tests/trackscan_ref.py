"""CPU restatement (numpy) of hgnn_track_scan (csrc/trackscan.hip) for the score-cut scan tests: the cuts sorted
descending, a plain sequential union-find carried from the highest cut to the lowest (EDGE) or the pair filter
(PAIR), the reference's none-pass rule, ``tracking_ref.track_eval`` on the resulting graph, and the integer edge
counts.  Not collected by pytest.

scan(...) returns one dict per cut, in the caller's cut order: the keys of ``tracking_ref.track_eval`` plus ``empty``
(no pair at that cut: the row hgnn_track_eval writes for n_pairs == 0, whose four ratios are NaN), ``hit`` / ``cand``
(the evaluated pairs) and ``n_pass`` / ``n_true_pass`` / ``n_true``.
"""
import numpy as np

import tracking_ref as T

ROW = T.KEYS + ("n_kept", "n_mask", "n_truth", "n_cand", "n_part", "no_match", "status", "n_match", "n_pass",
                "n_true_pass", "n_true")       # the order of HGNN_TE_* followed by HGNN_TS_N_*
# wrong kernels, for tests/test_trackscan_ref.py
MUTANTS = ("gt", "no_fallback", "no_carry", "no_present", "sorted_order", "dedup_cuts", "empty_as_run",
           "nan_in_fallback", "counts_no_keep")


class _UnionFind:
    def __init__(self, n):
        self.parent = np.arange(n)
        self.present = np.zeros(n, bool)

    def find(self, v):
        while self.parent[v] != v:
            v = self.parent[v]
        return v

    def hook(self, src, dst):
        n = self.parent.size
        for u, v in zip(src.tolist(), dst.tolist()):
            if u < 0 or v < 0 or u >= n or v >= n:      # skipped, as in k_cc_hook
                continue
            self.present[u] = self.present[v] = True
            a, b = self.find(u), self.find(v)
            if a != b:
                self.parent[max(a, b)] = min(a, b)      # the label of a component is its smallest vertex id

    def pairs(self, inverse_mask):
        v = np.flatnonzero(self.present)
        return inverse_mask[v], np.array([self.find(x) for x in v], np.int64)


def _n_truth(pid, pt, primary, pt_cut, nhits_cut):
    """reconstructable particles (tracking_ref step 7), for the empty_as_run mutant"""
    opid, inv, nhits = np.unique(pid, return_inverse=True, return_counts=True)
    ptmin = np.full(opid.size, np.inf, np.float32)
    with np.errstate(invalid="ignore"):
        np.minimum.at(ptmin, inv, pt)
        truth = (ptmin > np.float32(pt_cut)) & (nhits >= nhits_cut)
    if primary is not None:
        prim = np.zeros(opid.size, bool)
        prim[inv[np.asarray(primary) != 0]] = True
        truth &= prim
    return int(truth.sum())


def _evaluate(hit, cand, pid, pt, primary, pt_cut, nhits_cut, majority_cut, mutant):
    with np.errstate(all="ignore"):
        r = T.track_eval(hit, cand, pid, pt, primary, pt_cut, nhits_cut, majority_cut)
    r["empty"] = hit.size == 0
    if r["empty"]:
        nan = float("nan")
        r.update(track_eff=nan, track_pur=nan, hit_eff=nan, hit_pur=nan)
        if mutant == "empty_as_run":       # the pipeline run over nothing but dead pairs: the particles are counted
            r["n_truth"] = _n_truth(pid, pt, primary, pt_cut, nhits_cut)
            with np.errstate(all="ignore"):
                r["track_eff"] = float(np.float64(0) / np.float64(r["n_truth"]))
    r["status"] = 0
    r["hit"], r["cand"] = hit, cand
    return r


def scan(mode, a, b, score, cuts, inverse_mask, pid, pt, primary=None, pt_cut=1.0, nhits_cut=5, majority_cut=0.5,
         truth=None, keep=None, mutant=None):
    """mode "edge": a, b = src, dst over len(inverse_mask) vertices; mode "pair": a, b = hit, cand, inverse_mask or
    None.  cuts: any order, repeats allowed, no NaN; compared in float32"""
    assert mode in ("edge", "pair") and (mutant is None or mutant in MUTANTS)
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    score = np.asarray(score, np.float32)
    cuts = np.asarray(cuts, np.float64).astype(np.float32)
    pid, pt = np.asarray(pid, np.int64), np.asarray(pt, np.float32)
    Tn = cuts.size
    assert 1 <= Tn <= 64 and not np.isnan(cuts).any()
    order = np.argsort(-cuts.astype(np.float64), kind="stable")       # descending, stable
    with np.errstate(invalid="ignore"):
        passes = [(score > cuts[t]) if mutant == "gt" else (score >= cuts[t]) for t in order]   # NaN: never
    kept = np.ones(score.size, bool) if keep is None or mutant == "counts_no_keep" else np.asarray(keep) != 0
    args = (pid, pt, primary, pt_cut, nhits_cut, majority_cut, mutant)
    rows = []
    if mode == "edge":
        inverse_mask = np.asarray(inverse_mask, np.int64)
        uf = _UnionFind(inverse_mask.size)
        done = np.zeros(score.size, bool)
        for j in range(Tn):
            new = passes[j] & ~done
            done |= passes[j]
            if mutant == "no_carry":
                uf.parent = np.arange(inverse_mask.size)
            if mutant == "no_present":
                uf.present[:] = False
            uf.hook(a[new], b[new])
            rows.append(_evaluate(*uf.pairs(inverse_mask), *args))
        # none passes: all edges (with a comparable score) instead
        rest = ~done if mutant == "nan_in_fallback" else ~done & ~np.isnan(score)
        uf.hook(a[rest], b[rest])
        fallback = _evaluate(*uf.pairs(inverse_mask), *args)
        if mutant != "no_fallback":
            rows = [dict(fallback) if not passes[j].any() else rows[j] for j in range(Tn)]
    else:
        for j in range(Tn):
            hit, cand = a[passes[j]], b[passes[j]]
            if inverse_mask is not None:
                hit = np.asarray(inverse_mask, np.int64)[hit]
            rows.append(_evaluate(hit, cand, *args))
    for j in range(Tn):
        if truth is None:
            rows[j].update(n_pass=0, n_true_pass=0, n_true=0)
        else:
            y = np.asarray(truth) != 0
            rows[j].update(n_pass=int((kept & passes[j]).sum()), n_true_pass=int((kept & y & passes[j]).sum()),
                           n_true=int((kept & y).sum()))
    if mutant == "dedup_cuts":          # a repeated cut gets no row of its own
        blank = dict(_evaluate(np.zeros(0, np.int64), np.zeros(0, np.int64), *args), n_pass=0, n_true_pass=0,
                     n_true=0)
        rows = [rows[j] if j == 0 or cuts[order[j]] != cuts[order[j - 1]] else dict(blank) for j in range(Tn)]
    if mutant == "sorted_order":
        return rows
    out = [None] * Tn
    for j, t in enumerate(order):
        out[t] = rows[j]
    return out


def row_vector(r):
    """float64[15] in the order of ROW, and the entries that are compared: on a no_match row that is not the empty
    row the restatement defines neither n_mask / n_truth nor the raw ratios (eval_metrics returns default_response)"""
    vec = np.array([float(r.get(k, 0)) for k in ROW], np.float64)
    skip = set(T.KEYS) | {"n_mask", "n_truth"} if r["no_match"] and not r["empty"] else set()
    return vec, [i for i, k in enumerate(ROW) if k not in skip]
