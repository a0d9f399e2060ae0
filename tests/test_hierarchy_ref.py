"""Proof of tests/hierarchy_ref.py (CPU only), and every input-selection condition the GPU tests of the hierarchy
decision rely on, so that a bad seed fails here and not on the device.

Agreement observed when this file was written (float64 throughout, tol = 1e-12 on both sides):
  gmm_ref vs sklearn GaussianMixture(2, means_init = gmm_ref's own start), largest |difference| of (w, mu, var):
    balanced     1.7e-7     1000:1     5.9e-7     overlapping     3.6e-7
  (sklearn starts from the means only and takes its own path, so only the fixed point is compared; both sides stop
  when the lower bound moves by less than 1e-12, and at a maximum the bound is quadratic in the parameters, which
  leaves them undetermined to about sqrt(1e-12) = 1e-6).
The assertions use 5e-6: an EM whose update is off by any factor lands far outside it.
"""
import math

import numpy as np
import pytest
import torch

import hierarchy_ref as HR


# ------------------------------------------------------------------ kNN
KNN_PROOF_CASES = [
    # (nq, np, D, K, r, generator)
    (17, 300, 3, 5, 2.0, "grid"), (9, 700, 1, 10, 1.0, "grid"), (33, 257, 8, 32, 3.0, "grid"),
    (12, 500, 16, 16, 8.0, "fine"), (12, 400, 7, 100, 6.0, "fine"), (20, 600, 4, 128, 4.0, "dup"),
    (5, 3, 2, 8, 16.0, "grid"), (5, 0, 2, 3, 1.0, "grid"), (7, 200, 5, 4, 0.0, "grid"),
]


def _knn_inputs(nq, n_p, D, gen, seed):
    if gen == "fine":
        return HR.fine_points(nq, D, seed), HR.fine_points(n_p, D, seed + 1)
    q, p = HR.grid_points(nq, D, seed), HR.grid_points(n_p, D, seed + 1)
    if gen == "dup":
        p = HR.with_duplicates(p, seed + 2)
    return q, p


@pytest.mark.parametrize("case", KNN_PROOF_CASES, ids=lambda c: "q%d-p%d-D%d-K%d-r%g-%s" % c)
def test_knn_ref_equals_float64_brute_force(case):
    nq, n_p, D, K, r, gen = case
    q, p = _knn_inputs(nq, n_p, D, gen, 11)
    idx, d2 = HR.knn_ref(q, p, K, r)
    bidx, bd2 = HR.knn_brute_f64(q, p, K, r)
    assert torch.equal(idx, bidx) and torch.equal(d2, bd2)


@pytest.mark.parametrize("case", [c for c in KNN_PROOF_CASES if c[1] > 0], ids=lambda c: "q%d-p%d-D%d-K%d-r%g-%s" % c)
def test_knn_ref_agrees_with_oracle(case):
    from oracle.hgnn_oracle import knn_radius
    nq, n_p, D, K, r, gen = case
    q, p = _knn_inputs(nq, n_p, D, gen, 23)
    idx, d2 = HR.knn_ref(q, p, K, r)
    oidx, od2 = knn_radius(q, p, K, r)
    assert torch.equal(idx, oidx) and torch.equal(d2, od2)


def test_knn_float32_accumulation_is_exact_on_the_grid():
    """float32 accumulation in the kernels' order equals the int64 sums bit for bit at the extreme of the grid"""
    q, p = HR.fine_points(64, 16, 3), HR.fine_points(512, 16, 4)
    q[0], p[0] = 4.0, -4.0                                                  # the largest possible distance
    d2 = torch.zeros(64, 512, dtype=torch.float32)
    for d in range(16):
        t = q[:, d:d + 1] - p[:, d].unsqueeze(0)
        d2 = torch.addcmul(d2, t, t)
    qi, pi = (q * 16).long(), (p * 16).long()
    exact = ((qi.unsqueeze(1) - pi.unsqueeze(0)) ** 2).sum(-1)
    assert int(exact.max()) == 16 * 128 * 128 < HR.EXACT_LIMIT
    assert torch.equal(d2.double() * 256, exact.double())


def test_knn_ref_refuses_inexact_input():
    q = HR.grid_points(4, 3, 0)
    with pytest.raises(AssertionError):
        HR.knn_ref(q + 0.01, q, 2, 1.0)
    with pytest.raises(AssertionError):
        HR.knn_ref(q * 2, q, 2, 1.0)
    with pytest.raises(AssertionError):
        HR.knn_ref(q, q, 2, 0.3)


def test_knn_generators_have_the_advertised_ties():
    q, p = HR.grid_points(100, 3, 1), HR.grid_points(2000, 3, 2)
    qi, pi = (q * 16).long(), (p * 16).long()
    d2 = ((qi.unsqueeze(1) - pi.unsqueeze(0)) ** 2).sum(-1)
    assert torch.unique(d2).numel() <= 200, "the coarse grid should give mass ties"
    pts, shell = HR.tie_shell(4, 40, 400, 300, 5)
    d2 = ((pts * 16).long() ** 2).sum(-1)
    assert int((d2 == shell).sum()) == 400 and int((d2 < shell).sum()) == 40
    assert torch.unique(pts[d2 == shell], dim=0).shape[0] >= 24, "the shell should hold many DISTINCT points"
    q, p = HR.far_apart(10, 300, 3, 6)
    assert bool((HR.knn_ref(q, p, 5, 1.0)[0] == -1).all())


def _assert_strict_cut_arm(runs, K, what):
    """the two conditions that make an arm sensitive, over the inputs it runs on.  Strict cut (`d2 < r^2` against
    `d2 <= r^2`): some query has FEWER than K points strictly inside the radius and at least one exactly at it; only
    then can an at-radius candidate reach the K outputs, and the correct row ends in padding.  Truncation: ANOTHER
    query has MORE than K points strictly inside, so its list fills, later candidates are inserted into a full list
    and keys are dropped; its correct row has no padding.  No guard on the number of queries: a single query is run on
    two point sets (``hierarchy_ref.tie_runs``)."""
    witnesses = truncating = 0
    for n, (q, p, r) in enumerate(runs):
        below, at = HR.radius_counts(q, p, r)
        w, full = torch.nonzero((below < K) & (at > 0)).flatten(), torch.nonzero(below > K).flatten()
        assert w.numel() == HR.strict_cut_witnesses(q, p, K, r) and full.numel() == HR.truncating_queries(q, p, K, r)
        ref = HR.knn_ref(q[:HR.WITNESS_QUERIES], p, K, r)[0]
        assert bool((ref[w, K - 1] == -1).all()), "a witness row ends in padding"
        assert bool((ref[full] >= 0).all()), "a full row has no padding"
        witnesses += int(w.numel()) if n == 0 else 0            # the GPU tests look for the witness in the first run
        truncating += int(full.numel())
    assert witnesses >= 1, (what, "no strict-cut witness")
    assert truncating >= 1, (what, "no list fills")
    return witnesses


@pytest.mark.parametrize("case", HR.kd_cases(), ids=lambda c: "K%d-D%d-%s" % c[:3])
def test_knn_k_by_d_arms_see_the_strict_cut(case):
    """every case on its own, hence every k_knn_radius<K, DP, 64, SPLIT> arm and every k_knn_merge<K>"""
    runs = HR.kd_runs(case)
    assert len(runs) == (2 if case[3] == 1 else 1)
    _assert_strict_cut_arm(runs, case[0], case)


@pytest.mark.parametrize("i", range(len(HR.KNN_INSTANCES)))
def test_knn_block256_arms_see_the_strict_cut(i):
    K, D, nq, n_p = HR.block256_case(i)
    assert _assert_strict_cut_arm([HR.block256_inputs(i)], K, (K, D, nq, n_p)) >= 2, "queries share grid positions"


def test_knn_other_arms_see_the_strict_cut():
    _assert_strict_cut_arm([HR.radius_forms_inputs()], HR.RADIUS_FORMS_K, "radius forms")
    for nq, n_p, _ in HR.SLICE_EDGE_CASES:
        _assert_strict_cut_arm([HR.slice_edge_inputs(nq, n_p)], HR.SLICE_EDGE_K, ("slices", nq, n_p))
    for n in range(len(HR.NP_EDGES)):
        K, n_p, nq, D = HR.np_edge_case(n)
        if n_p >= 255:
            _assert_strict_cut_arm(HR.np_edge_runs(n), K, ("np edge", K, n_p, nq, D))
    for K in HR.LARGE_KS:
        for D in HR.LARGE_DS:
            for form in ("split", "unsplit"):
                _assert_strict_cut_arm([HR.large_inputs(K, D, form)], K, ("large", K, D, form))


def test_thin_inside_on_a_hand_example():
    """D = 1, r = 2, query at 0: points at -1, 0, 0, 1 are inside, 2 and -2 at the radius, 3 beyond"""
    q = torch.tensor([[0.0]])
    p = torch.tensor([[-1.0], [0.0], [2.0], [0.0], [1.0], [-2.0], [3.0]])
    assert HR.strict_cut_witnesses(q, p, 3, 2.0) == 0 and HR.strict_cut_witnesses(q, p, 5, 2.0) == 1
    t = HR.thin_inside(q, p, 3, 2.0, [0])                   # keeps (3 - 1) // 2 = 1 inside point, the first by index
    assert t.flatten().tolist() == [-1.0, 2.0, 2.0, -2.0, 2.0, -2.0, 3.0]
    assert HR.strict_cut_witnesses(q, t, 3, 2.0) == 1
    idx, d2 = HR.knn_ref(q, t, 3, 2.0)
    assert idx.tolist() == [[0, -1, -1]] and d2.tolist() == [[1.0, -1.0, -1.0]]


# ------------------------------------------------------------------ mixture
def _sklearn_fit(v, means_init):
    from sklearn.mixture import GaussianMixture
    gm = GaussianMixture(2, means_init=np.asarray(means_init).reshape(2, 1), tol=1e-12, reg_covar=1e-6, max_iter=5000)
    gm.fit(np.asarray(v, dtype=np.float64).reshape(-1, 1))
    assert gm.converged_
    return gm.weights_, gm.means_.ravel(), gm.covariances_.ravel()


@pytest.mark.parametrize("name,v", [
    ("balanced", HR._mix(11, 4000, -1.0, 0.5, 4000, 2.0, 0.7)),
    ("imbalanced_1000_1", HR._mix(12, 50000, 0.0, 0.5, 50, 5.0, 0.3)),
    ("overlapping", HR._mix(13, 5000, 0.0, 1.0, 5000, 2.5, 1.0)),
], ids=lambda t: t if isinstance(t, str) else "")
def test_gmm_ref_has_sklearn_fixed_point(name, v):
    state, _ = HR.gmm_ref(v, max_iter=1000, tol=1e-12, reg_covar=1e-6)
    assert state[HR.S_CONV] == 1.0
    w, mu, var = _sklearn_fit(v, state[2:4])
    dev = max(np.abs(state[0:2] - w).max(), np.abs(state[2:4] - mu).max(), np.abs(state[4:6] - var).max())
    print(f"gmm_ref vs sklearn, {name}: {dev:.3g}")
    assert dev < 5e-6, dev


def test_gmm_start_is_exact_on_dyadic_values():
    """Lloyd sums of dyadic values are exact in float64 in any order: c0 and c1 do not depend on the summation order"""
    v = HR.dyadic_values(100003, 1)
    lo, hi, c0, c1 = HR.gmm_start_ref(v)
    lo2, hi2, c02, c12 = HR.gmm_start_ref(v[::-1].copy())
    assert (lo, hi, c0, c1) == (lo2, hi2, c02, c12)
    assert lo == -8.0 and hi == 8.0 and c0 < 0 < c1


@pytest.mark.parametrize("name", sorted(HR.DEGENERATE))
def test_gmm_degenerate_inputs_meet_the_input_conditions(name):
    """finite, weights sum to 1, the populated component's mean is the data; and the conditions of the device
    comparison: pass counts can be compared (every |delta lower| clear of tol, reference and emulation stop at the same
    pass), and w, mu, var carry no float32 effect at all (d_emul = 0)"""
    v = HR.DEGENERATE[name]
    state, deltas = HR.gmm_ref(v)
    emu, deltas_e = HR.gmm_f32_emulation(v)
    assert np.isfinite(state).all() and np.isfinite(emu).all()
    assert abs(state[0] + state[1] - 1) < 1e-6
    assert HR.deltas_clear_of_tol(deltas, 1e-3) and HR.deltas_clear_of_tol(deltas_e, 1e-3), (deltas, deltas_e)
    assert state[HR.S_ITERS] == emu[HR.S_ITERS] and state[HR.S_CONV] == emu[HR.S_CONV] == 1.0
    d = HR.gmm_deviation(state, emu)
    print(f"d_emul {name:22s} passes {int(state[HR.S_ITERS])} " + " ".join(f"{q} {d[q]:.2e}" for q in HR.GMM_QUANTITIES))
    assert d["w"] == d["mu"] == d["var"] == 0.0, d
    assert d["lower"] <= HR.degenerate_lower_budget(float(np.abs(v).max())), d
    # a component of N identical values x sits at reg_covar + 20 eps x^2 / N (the pull of nk += 10 eps(float32))
    assert 1e-6 * (1 - 1e-7) <= min(state[4], state[5]) <= max(state[4], state[5]) < 1e-6 + 1.3e-6 * float(v.max()) ** 2
    if v.min() == v.max():
        # nk += 10 eps pulls the mean of M identical values x to x * M / (M + 10 eps)
        assert abs(state[HR.S_MU0] - float(v[0])) <= abs(float(v[0])) * HR.EPS10 / v.size + 2 * float(np.spacing(abs(v[0])))
        assert state[HR.S_W1] < 1e-5
    else:
        assert sorted([round(state[2], 5), round(state[3], 5)]) == [-1.0, 3.0]


EM_CASES = HR.em_cases()


@pytest.mark.parametrize("name", sorted(EM_CASES))
def test_em_cases_meet_the_input_conditions(name):
    """pass-count equality on the device needs every |delta lower| clear of tol by a factor 2, in the reference and
    in the float32 emulation, and both must stop at the same pass.  Prints d_emul (the table of
    tests/test_gpu_hierarchy_decision.py)."""
    v, max_iter = EM_CASES[name]
    ref, deltas = HR.gmm_ref(v, max_iter)
    emu, deltas_e = HR.gmm_f32_emulation(v, max_iter)
    assert HR.deltas_clear_of_tol(deltas, 1e-3) and HR.deltas_clear_of_tol(deltas_e, 1e-3), (deltas, deltas_e)
    assert ref[HR.S_ITERS] == emu[HR.S_ITERS] and ref[HR.S_CONV] == emu[HR.S_CONV]
    if max_iter < 100:
        assert ref[HR.S_CONV] == 0.0 and ref[HR.S_ITERS] == max_iter
    else:
        assert ref[HR.S_CONV] == 1.0 and 2 <= ref[HR.S_ITERS] < 100
    d = HR.gmm_deviation(ref, emu)
    print(f"d_emul {name:18s} passes {int(ref[HR.S_ITERS]):3d} " + " ".join(f"{q} {d[q]:.2e}" for q in HR.GMM_QUANTITIES))
    assert all(0 < d[q] < 1e-3 for q in HR.GMM_QUANTITIES), d
    if name == "collapsed":
        assert min(ref[4], ref[5]) < 2e-6, "one component should sit at reg_covar"
    if name == "imbalanced_1000_1":
        assert 500 < max(ref[0], ref[1]) / min(ref[0], ref[1]) < 2000
    if name == "likelihoods":
        assert abs(float(v.max()) - math.atanh(HR.CLAMP)) < 1e-3 and float(v.min()) == -float(v.max())
    if name == "one_block":
        assert v.size <= 1024
    if name == "over_2p20":
        assert v.size > 1 << 20


# ------------------------------------------------------------------ cut
def _state(six):
    s = np.zeros(16)
    s[:6] = six
    return s


@pytest.mark.parametrize("name", sorted(HR.CUT_STATES))
@pytest.mark.parametrize("granularity", [-5.0, 0.0, 0.5, 5.0, 40.0])
def test_cut_ref_solves_the_defining_equation(name, granularity):
    st = _state(HR.CUT_STATES[name])
    cut, has_root = HR.cut_ref(st, granularity)
    lo, hi = min(st[2], st[3]), max(st[2], st[3])
    f, _, _ = HR.cut_function(st, granularity)
    if not has_root:
        assert cut == 0.5 * (lo + hi) and f(lo) * f(hi) > 0
        return
    assert lo <= cut <= hi
    assert abs(f(cut)) < 1e-12
    g, _ = HR.cut_log_ratio(st, granularity, cut)        # the same root in the scale-free form
    assert abs(g) < 1e-9
    from scipy.optimize import brentq
    assert abs(brentq(f, lo, hi, xtol=1e-15, rtol=1e-15) - cut) < 1e-9 * (hi - lo) or abs(f(cut)) == 0.0


def test_cut_states_cover_both_branches():
    assert not HR.cut_ref(_state(HR.CUT_STATES["no_sign_change"]), 0.0)[1]
    assert HR.cut_ref(_state(HR.CUT_STATES["ordered"]), 0.0)[1] and HR.cut_ref(_state(HR.CUT_STATES["swapped"]), 0.0)[1]
    # at granularity 40 sigmoid(-r) = 4e-18: only far-apart components still have the sign change between the means
    assert HR.cut_ref(_state(HR.CUT_STATES["far"]), 40.0)[1] and not HR.cut_ref(_state(HR.CUT_STATES["ordered"]), 40.0)[1]


def test_score_cut_ref_bookkeeping():
    st = _state(HR.CUT_STATES["ordered"])
    f = np.float32
    assert HR.score_cut_ref(f("inf"), 0.3, st, False) == f(0.5)
    assert HR.score_cut_ref(f("inf"), 0.3, st, True) == f(f(f(0.95) * f(0.5)) + f(f(f(1) - f(0.95)) * f(0.3)))
    assert HR.score_cut_ref(f(1.25), 0.3, st, False) == f(1.25)
    assert HR.score_cut_ref(f(1.25), -1.0, st, True) == f(1.25)        # cut AT a mean: not strictly between
    assert HR.score_cut_ref(f(1.25), 2.0, st, True) == f(1.25)
    assert HR.score_cut_ref(f(1.25), 1.0, st, True) != f(1.25)
    # the fused forms round once: computed here with exact rationals
    from fractions import Fraction as Fr
    m, om = f(0.95), f(f(1) - f(0.95))
    for sc, cut in ((1.25, 0.3), (0.7, 1.9), (-0.3, 0.123456789)):
        forms = HR.score_cut_forms(f(sc), cut, st, True)
        a, b = f(m * f(sc)), f(om * f(cut))
        assert forms[0] == f(a + b)
        assert forms[1] == f(float(Fr(float(m)) * Fr(float(f(sc))) + Fr(float(b))))
        assert forms[2] == f(float(Fr(float(om)) * Fr(float(f(cut))) + Fr(float(a))))
    assert HR.score_cut_forms(f(1.25), 2.0, st, True) == (f(1.25),) * 3


# ------------------------------------------------------------------ components
def _scipy_components(src, dst, n, keep):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    s, d = src[keep], dst[keep]
    g = coo_matrix((np.ones(s.size), (s, d)), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    first = np.full(lab.max() + 1, n, dtype=np.int64)
    np.minimum.at(first, lab, np.arange(n))
    present = np.zeros(n, dtype=np.int32)
    present[s] = 1
    present[d] = 1
    return first[lab].astype(np.int32), present


@pytest.mark.parametrize("cut", [0.9, float("inf"), float("-inf"), None])
def test_components_ref_equals_scipy(cut):
    n = 50000
    src, dst, score, c = HR.cc_inputs(n)
    args = (score, c if cut == 0.9 else cut) if cut is not None else (None, None)
    labels, present = HR.components_ref(src, dst, n, *args)
    keep = HR.kept_edges(src, dst, n, *args)
    slab, spres = _scipy_components(src, dst, n, keep)
    assert np.array_equal(labels, slab) and np.array_equal(present, spres)
    if cut == float("inf"):
        assert keep.sum() == 0 and present.sum() == 0 and np.array_equal(labels, np.arange(n))


def test_cc_inputs_hold_every_edge_class():
    n = 50000
    src, dst, score, cut = HR.cc_inputs(n)
    cutf = np.float32(cut)
    valid = (src >= 0) & (dst >= 0) & (src < n) & (dst < n)
    assert (score == cutf).sum() >= 1000 and (score == np.nextafter(cutf, np.float32(-np.inf))).sum() >= 1000
    assert np.isnan(score).sum() >= 1000 and (src == dst).sum() >= 1000
    assert (src == -1).sum() >= 50 and (dst == n).sum() >= 50 and (src == n).sum() >= 50 and (dst == -1).sum() >= 50
    assert (~valid).sum() >= 200 and bool((score[~valid] >= cutf).all())
    pairs = src[valid] * n + dst[valid]
    assert pairs.size - np.unique(pairs).size >= 1000, "duplicated edges"
    # the boundary classes matter: edges AT the cut join components that `>` would leave apart, and the edges one ulp
    # below it would join more
    at = HR.components_ref(src, dst, n, score, cut)[0]
    strict = HR.components_ref(src, dst, n, score, float(np.nextafter(cutf, np.float32(np.inf))))[0]
    loose = HR.components_ref(src, dst, n, score, float(np.nextafter(cutf, np.float32(-np.inf))))[0]
    assert not np.array_equal(at, strict) and not np.array_equal(at, loose)
    # and the cut leaves a non-trivial partition with clusters on both sides of every size filter used
    sizes = np.bincount(at)
    assert (sizes == 1).sum() > 100 and (sizes == 2).sum() > 10 and (sizes >= 50).sum() >= 1
    for m in (1, 2, 3, 50):
        cl, cnt = HR.cluster_labels_ref(src, dst, n, m, score, cut)
        assert cnt >= 1 and cl.max() == cnt - 1 and (cl == -1).any()
        first = np.array([np.flatnonzero(cl == c)[0] for c in range(min(cnt, 50))])
        assert (np.diff(first) > 0).all(), "ids follow the smallest hit of each cluster"


def test_cluster_labels_ref_small_example():
    #   0-1-2   3-4   5(self loop)   6 isolated   7-8 below the cut
    src, dst = np.array([0, 1, 3, 5, 7]), np.array([1, 2, 4, 5, 8])
    score = np.array([1, 1, 1, 1, 0], np.float32)
    cl, cnt = HR.cluster_labels_ref(src, dst, 9, 1, score, 0.5)
    assert cl.tolist() == [0, 0, 0, 1, 1, 2, -1, -1, -1] and cnt == 3
    cl, cnt = HR.cluster_labels_ref(src, dst, 9, 2, score, 0.5)
    assert cl.tolist() == [0, 0, 0, 1, 1, -1, -1, -1, -1] and cnt == 2
    cl, cnt = HR.cluster_labels_ref(src, dst, 9, 3)
    assert cl.tolist() == [0, 0, 0, -1, -1, -1, -1, -1, -1] and cnt == 1


# ------------------------------------------------------------------ whole decision
def decision_margin(ref, D=8):
    """(delta, closest likelihood to the cut): delta = 100 x (cut allowance + float32 likelihood error bound); see
    tests/test_gpu_hierarchy_decision.py for the cut allowance (stated there as HR.CUT_ALLOWANCE_DECISION)"""
    lik = ref["likelihood"]
    bound = HR.likelihood_error_bound(D, float(np.tanh(np.abs(lik).max())))
    return 100.0 * (HR.CUT_ALLOWANCE_DECISION + bound), float(np.abs(lik - float(ref["score_cut"])).min())


@pytest.mark.parametrize("kind,training,start", [("normal", True, "inf"), ("normal", False, "inf"), ("normal", True, 1.0),
                                                 ("fallback", True, "inf")])
def test_decision_inputs_meet_the_conditions(kind, training, start):
    emb, graph = HR.decision_inputs(kind)
    ref = HR.decision_ref(emb, graph, np.float32(start), HR.HPARAMS, training)
    assert HR.deltas_clear_of_tol(ref["deltas"], 1e-3), ref["deltas"]
    emu, deltas_e = HR.gmm_f32_emulation(ref["likelihood"].astype(np.float32))
    assert HR.deltas_clear_of_tol(deltas_e, 1e-3) and emu[HR.S_ITERS] == ref["state"][HR.S_ITERS]
    d = HR.gmm_deviation(ref["state"], emu)
    allow = {q: 16 * d[q] for q in HR.GMM_QUANTITIES}
    assert max(allow["w"], allow["mu"], allow["var"]) < 2e-6, allow
    moved = HR.cut_perturbation(ref["state"], HR.HPARAMS["cluster_granularity"], allow)
    assert moved + allow["mu"] < HR.CUT_ALLOWANCE_DECISION, moved
    delta, closest = decision_margin(ref)
    print(f"decision {kind}: cut {ref['cut']:.6f} score_cut {float(ref['score_cut']):.6f} cut moves {moved:.2e} "
          f"delta {delta:.2e} closest likelihood {closest:.2e} clusters {ref['count']} reads {ref['host_reads']}")
    assert closest > delta, "an edge likelihood lies within delta of the cut: pick another seed (no mask)"
    assert np.abs(ref["likelihood"]).max() < math.atanh(0.9999)
    if kind == "normal":
        assert ref["host_reads"] == 1 and ref["count"] > 3
        assert (ref["clusters"] == -1).sum() < emb.shape[0]
    else:
        cut_count = HR.cluster_labels_ref(graph[0], graph[1], emb.shape[0], 3, ref["likelihood"],
                                          float(ref["score_cut"]))[1]
        assert cut_count in (2, 3) and ref["host_reads"] == 2
        assert ref["count"] == 1, "the uncut graph joins the tracks"


def test_decision_ref_empty_graph():
    emb, graph = HR.decision_inputs("empty")
    ref = HR.decision_ref(emb, graph, np.float32(0.5), HR.HPARAMS, True)
    assert ref["count"] == 0 and ref["host_reads"] == 0 and (ref["clusters"] == -1).all()
    assert ref["score_cut"] == np.float32(0.5)
