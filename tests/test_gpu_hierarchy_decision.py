"""Conformance of the hierarchy decision's device code (csrc/cluster.hip, hierarchicalgnn_amd/clustering.py) against
the float64 references of tests/hierarchy_ref.py: the mixture fit, its cut, the components, the whole decision.

Tolerances.  The E step of k_gmm_pass is float32 (1/var, logf, __expf, __logf); its sums are float64.  d_emul is the
deviation between ``gmm_ref`` (float64) and ``gmm_f32_emulation`` (the same EM with a numpy-float32 E step) per
quantity; the device is allowed 16 x d_emul and nothing more (the fast exp / log are a few ulp worse than libm; the
float64 sums add nothing).  d_emul is recomputed by the test on every run; the values when this file was written, with
the device deviation observed on an MI355X beside them ("dev", same units):

  case               passes  w d_emul   mu d_emul  var d_emul  lower d_emul | dev w     dev mu    dev var   dev lower
  balanced              4    4.2e-10    4.1e-09    1.4e-08     4.3e-09      | 4.5e-10   4.0e-09   1.4e-08   4.3e-09
  collapsed             4    2.8e-08    1.2e-07    2.7e-07     7.7e-08      | 2.8e-08   1.2e-07   2.7e-07   4.0e-07
  imbalanced_1000_1     2    7.4e-15    1.8e-11    4.5e-11     3.3e-09      | 7.4e-15   1.8e-11   4.5e-11   3.8e-09
  likelihoods           3    3.6e-10    2.3e-09    4.5e-09     3.0e-08      | 3.5e-10   2.3e-09   4.4e-09   3.0e-08
  max_iter_1            1    1.4e-08    4.2e-08    8.9e-09     7.7e-09      | 1.4e-08   3.8e-08   9.3e-09   7.3e-09
  max_iter_3            3    2.6e-09    1.9e-08    2.5e-08     1.8e-08      | 1.5e-08   6.1e-08   3.7e-08   6.8e-08
  one_block             3    2.3e-09    3.9e-09    4.8e-09     8.7e-09      | 4.0e-09   7.6e-09   7.1e-09   8.5e-09
  over_2p20             3    1.3e-08    5.1e-08    4.3e-08     6.9e-08      | 5.0e-09   1.6e-08   8.1e-09   3.9e-09
  overlapping           3    4.7e-09    2.1e-08    4.5e-08     1.0e-07      | 4.7e-09   2.3e-08   4.8e-08   4.1e-08

The largest device / d_emul ratio observed is 5.9 (w of max_iter_3) against the 16 allowed.

Degenerate inputs (constant, M = 1, two values): every responsibility is exactly 0 or 1, so d_emul of w, mu and var is
0 (asserted on the CPU) and 16 x d_emul would demand bitwise equality of float64 sums taken in different orders.
There, and only there, w, mu and var are allowed the summation-order floor M * 2^-53 * max(1, max x^2) (observed:
1e-16), and the lower bound -- one float32 value repeated M times -- the itemised float32 budget of
``hierarchy_ref.degenerate_lower_budget`` (20.4 x 2^-24 = 1.2e-6 at |x| <= 3; observed: up to 7.6e-7).

Pass counts are compared exactly; tests/test_hierarchy_ref.py asserts the input condition that makes this fair (no
|delta lower| of any case within a factor 2 of tol, in the reference and in the emulation).

The cut of a device-fitted mixture is allowed the EM allowance propagated through ``cut_ref`` (each of w, mu0, mu1,
var0, var1 moved by +-its allowance, largest change of the root) plus the allowance of the float64 root solve itself
(60 bisection steps: 2^-58 of the bracket; evaluation error of the log posterior ratio divided by its slope).

Whole decision: clusters are compared with ``torch.equal``.  The only mask-like construct is the margin around the
cut, asserted EMPTY on the CPU (tests/test_hierarchy_ref.py::test_decision_inputs_meet_the_conditions): no edge
likelihood within delta = 100 x (cut allowance + float32 atanh / dot error bound) of the reference cut.

Kernel -> test id that reaches it:
  k_gmm_pass<PASS_MINMAX>, <PASS_LLOYD>      test_fit_start_bitwise[M*] (grid-stride trip: M1048583, M3145729)
  k_gmm_pass<PASS_HARD_M>, <PASS_EM>         test_em_against_reference[*], test_em_degenerate_inputs[*]
    one block                                test_em_against_reference[one_block], test_fit_start_bitwise[M{1,2,1000}]
    grid capped at HGNN_GMM_BLOCKS           test_em_against_reference[over_2p20]
  k_gmm_reset                                every fit
  reg_covar = 0 refused                      test_reg_covar_zero_is_refused
  k_gmm_cut                                  test_cut_against_reference[*], test_cut_of_fitted_mixture
  k_cc_init, k_cc_hook, k_cc_compress        test_components_with_score_cut[*], test_components_edge_cases,
                                             test_cluster_labels_exact[*]
  gmm_edge_clustering                        test_whole_decision[*] (normal, c <= 3 fallback, empty graph)
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import hierarchy_ref as HR
from hierarchy_ref import CUT_STATES, HPARAMS, CUT_ALLOWANCE_DECISION, cc_inputs, cut_perturbation

pytestmark = pytest.mark.gpu

EM_CASES = HR.em_cases()


@pytest.fixture(scope="module", autouse=True)
def lib():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from hierarchicalgnn_amd import _lib
    return _lib.load()


def fit(v, max_iter=100, tol=1e-3, reg_covar=1e-6):
    from hierarchicalgnn_amd.clustering import gmm2_state
    st = gmm2_state(torch.from_numpy(np.ascontiguousarray(v)).cuda(), max_iter, tol, reg_covar)
    torch.cuda.synchronize()
    return st.cpu().numpy()


# ------------------------------------------------------------------ start of the fit
@pytest.mark.parametrize("M", [1, 2, 1000, 1024 * 1024 + 7, 3 * (1 << 20) + 1], ids=lambda m: f"M{m}")
def test_fit_start_bitwise(M):
    """min, max and the Lloyd centres on dyadic values: every sum is exact in float64 in any order, so the device's
    c0 and c1 equal the reference bit for bit (the last two sizes exceed the 1024-block cap: grid-stride trips)"""
    v = HR.dyadic_values(M, 40 + M % 7)
    lo, hi, c0, c1 = HR.gmm_start_ref(v)
    st = fit(v, max_iter=1)
    got = (st[HR.S_MIN], st[HR.S_MAX], st[HR.S_C0], st[HR.S_C1])
    assert got == (lo, hi, c0, c1), (got, (lo, hi, c0, c1))


# ------------------------------------------------------------------ EM
def allowance(ref, emu):
    d = HR.gmm_deviation(ref, emu)
    return {q: 16 * d[q] for q in HR.GMM_QUANTITIES}, d


@pytest.mark.parametrize("name", sorted(EM_CASES))
def test_em_against_reference(name):
    v, max_iter = EM_CASES[name]
    ref, _ = HR.gmm_ref(v, max_iter)
    emu, _ = HR.gmm_f32_emulation(v, max_iter)
    st = fit(v, max_iter)
    allow, d_emul = allowance(ref, emu)
    dev = HR.gmm_deviation(ref, st)
    print(f"\nEM {name:18s} passes dev {int(st[HR.S_ITERS])} ref {int(ref[HR.S_ITERS])} | " + " | ".join(
        f"{q}: d_emul {d_emul[q]:.2e} allowed {allow[q]:.2e} device {dev[q]:.2e}" for q in HR.GMM_QUANTITIES))
    assert np.isfinite(st).all()
    assert st[HR.S_ITERS] == ref[HR.S_ITERS], "pass count"
    assert st[HR.S_CONV] == ref[HR.S_CONV], "converged flag"
    if max_iter < 100:
        assert st[HR.S_CONV] == 0.0 and st[HR.S_ITERS] == max_iter
    assert st[HR.S_PREV] == st[HR.S_LOWER]
    for q in HR.GMM_QUANTITIES:
        assert dev[q] <= allow[q], f"{name}: {q} deviates by {dev[q]:.3g}, allowed {allow[q]:.3g} (d_emul {d_emul[q]:.3g})"


DEGENERATE = HR.DEGENERATE


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_em_degenerate_inputs(name):
    v = DEGENERATE[name]
    ref, _ = HR.gmm_ref(v)
    st = fit(v)
    assert np.isfinite(st).all(), st
    assert abs(st[0] + st[1] - 1.0) <= 1e-6
    # every responsibility is exactly 0 or 1 here: w, mu and var carry no float32 effect (d_emul = 0, asserted on the
    # CPU) and are allowed the float64 summation-order floor only; `lower` is one float32 value repeated M times and is
    # allowed the itemised float32 budget of that value (see the module docstring)
    floor = v.size * 2.0 ** -53 * max(1.0, float(np.max(v.astype(np.float64) ** 2)))
    allow = {q: floor for q in HR.GMM_QUANTITIES}
    allow["lower"] += HR.degenerate_lower_budget(float(np.abs(v).max()))
    dev = HR.gmm_deviation(ref, st)
    print(f"\nEM {name:22s} | " + " | ".join(f"{q}: allowed {allow[q]:.2e} device {dev[q]:.2e}" for q in HR.GMM_QUANTITIES))
    assert st[HR.S_ITERS] == ref[HR.S_ITERS] and st[HR.S_CONV] == ref[HR.S_CONV] == 1.0
    for q in HR.GMM_QUANTITIES:
        assert dev[q] <= allow[q], (q, dev[q], allow[q])
    if v.min() == v.max():                                   # all in component 0; nk += 10 eps pulls its mean by 10 eps / M
        x = float(v[0])
        assert abs(st[HR.S_MU0] - x) <= abs(x) * HR.EPS10 / v.size + 2 * float(np.spacing(abs(x)))
        assert st[HR.S_W1] < 1e-5
    else:                                                    # each value is one component's mean
        assert sorted([round(st[2], 5), round(st[3], 5)]) == [-1.0, 3.0]
    assert (st[HR.S_MIN], st[HR.S_MAX], st[HR.S_C0], st[HR.S_C1]) == \
        (ref[HR.S_MIN], ref[HR.S_MAX], ref[HR.S_C0], ref[HR.S_C1])


def test_reg_covar_zero_is_refused():
    """contract: a component of identical values has variance exactly reg_covar and the E step divides by it, so
    reg_covar must be positive; the entry point says so instead of returning a NaN mixture"""
    for v in (np.full(1000, 0.75, np.float32), HR.em_cases()["one_block"][0]):
        with pytest.raises(RuntimeError, match="reg_covar must be positive"):
            fit(v, reg_covar=0.0)


# ------------------------------------------------------------------ cut
def device_cut(state, granularity, training, score_cut, momentum=0.95):
    from hierarchicalgnn_amd import _lib as L
    st = torch.from_numpy(np.ascontiguousarray(state, dtype=np.float64)).cuda()
    sc = torch.tensor([score_cut], dtype=torch.float32, device="cuda")
    L.check(L.load().hgnn_gmm2_cut_f32(L.ptr(st), ctypes.c_float(granularity), 1 if training else 0,
                                       ctypes.c_float(momentum), L.ptr(sc), L.current_stream(st.device)),
            "hgnn_gmm2_cut_f32")
    torch.cuda.synchronize()
    return st.cpu().numpy(), np.float32(sc.cpu().numpy()[0])


def solve_allowance(state, granularity, cut):
    """what a float64 root solve of 60 bisection steps may miss: 2^-58 of the bracket, plus the evaluation error of the
    log posterior ratio (32 eps of the sum of its terms' magnitudes) divided by its slope at the root"""
    h = 1e-6 * abs(state[3] - state[2])
    g1, mag = HR.cut_log_ratio(state, granularity, cut + h)
    g0, _ = HR.cut_log_ratio(state, granularity, cut - h)
    slope = abs(g1 - g0) / (2 * h)
    return 2.0 ** -58 * abs(state[3] - state[2]) + 32 * 2.0 ** -52 * (mag + 1.0) / slope


@pytest.mark.parametrize("start", [float("inf"), 1.25], ids=["sc_inf", "sc_finite"])
@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("granularity", [-5.0, 0.0, 0.5, 5.0, 40.0])
@pytest.mark.parametrize("name", sorted(CUT_STATES))
def test_cut_against_reference(name, granularity, training, start):
    state = np.zeros(16)
    state[:6] = CUT_STATES[name]
    cut, has_root = HR.cut_ref(state, granularity)
    st, sc = device_cut(state, granularity, training, start)
    if has_root:
        assert abs(st[HR.S_CUT] - cut) <= solve_allowance(state, granularity, cut), (st[HR.S_CUT], cut)
    else:
        assert st[HR.S_CUT] == cut == 0.5 * (state[2] + state[3])
    assert np.array_equal(st[:13], state[:13]), "the cut kernel changes nothing but the cut slot"
    # the bookkeeping is float32 arithmetic on the device's own cut: momentum * sc + (1 - momentum) * cut evaluated
    # unfused, or with either product contracted into a fused multiply-add -- bitwise one of the three
    want = HR.score_cut_forms(start, st[HR.S_CUT], state, training)
    assert any(sc == w for w in want), (sc, want)
    lo, hi = min(state[2], state[3]), max(state[2], state[3])
    if not training or not (lo < st[HR.S_CUT] < hi):
        assert sc == (np.float32(0.5 * (lo + hi)) if math.isinf(start) else np.float32(start))


def test_cut_of_fitted_mixture():
    """fit + cut on the device against gmm_ref + cut_ref: the EM allowance propagated through the root"""
    for name in ("balanced", "overlapping", "likelihoods"):
        v, max_iter = EM_CASES[name]
        ref, _ = HR.gmm_ref(v, max_iter)
        emu, _ = HR.gmm_f32_emulation(v, max_iter)
        allow, _ = allowance(ref, emu)
        for g in (0.0, 0.5):
            cut, has_root = HR.cut_ref(ref, g)
            assert has_root
            bound = cut_perturbation(ref, g, allow) + solve_allowance(ref, g, cut)
            st, _ = device_cut(fit(v, max_iter), g, False, float("inf"))
            print(f"\ncut {name} r={g}: ref {cut:.9f} device {st[HR.S_CUT]:.9f} diff {abs(st[HR.S_CUT] - cut):.2e} "
                  f"allowed {bound:.2e}")
            assert abs(st[HR.S_CUT] - cut) <= bound


# ------------------------------------------------------------------ components
def device_cc(src, dst, n, score=None, cut=None):
    from hierarchicalgnn_amd.clustering import _cc
    s, d = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    sc = torch.from_numpy(score).cuda() if score is not None else None
    ct = torch.tensor([cut], dtype=torch.float32, device="cuda") if cut is not None else None
    labels, present = _cc(s, d, n, sc, ct)
    torch.cuda.synchronize()
    return labels.cpu(), present.cpu()


@pytest.mark.parametrize("cut", ["cut", "inf", "-inf", "none"])
def test_components_with_score_cut(cut):
    n = 50000
    src, dst, score, c = cc_inputs(n)
    args = {"cut": (score, c), "inf": (score, float("inf")), "-inf": (score, float("-inf")), "none": (None, None)}[cut]
    labels, present = device_cc(src, dst, n, *args)
    rl, rp = HR.components_ref(src, dst, n, *args)
    assert labels.dtype == torch.int32 and present.dtype == torch.int32
    assert torch.equal(present, torch.from_numpy(rp)), "present"
    assert torch.equal(labels, torch.from_numpy(rl)), "labels"
    if cut == "inf":
        assert int(present.sum()) == 0
    if cut == "-inf":                                        # NaN scores are still dropped: !(NaN >= -inf)
        assert HR.kept_edges(src, dst, n, *args).sum() + np.isnan(score).sum() >= HR.kept_edges(src, dst, n).sum() > \
            HR.kept_edges(src, dst, n, *args).sum()


def test_components_edge_cases():
    e = np.zeros(0, dtype=np.int64)
    labels, present = device_cc(e, e, 1000, np.zeros(0, np.float32), 0.5)                     # M = 0
    assert torch.equal(labels, torch.arange(1000, dtype=torch.int32)) and int(present.sum()) == 0
    z = np.zeros(5, dtype=np.int64)
    labels, present = device_cc(z, z, 1, np.ones(5, np.float32), 0.5)                         # n = 1, self loops
    assert labels.tolist() == [0] and present.tolist() == [1]
    labels, present = device_cc(z, z, 1, np.ones(5, np.float32), 1.5)
    assert labels.tolist() == [0] and present.tolist() == [0]
    bad = np.array([-1, 1, 0], dtype=np.int64), np.array([0, 0, 1], dtype=np.int64)           # ids outside [0, 1)
    labels, present = device_cc(bad[0], bad[1], 1)
    assert labels.tolist() == [0] and present.tolist() == [0]


@pytest.mark.parametrize("min_cluster_size", [1, 2, 3, 50])
def test_cluster_labels_exact(min_cluster_size):
    from hierarchicalgnn_amd.clustering import _cluster_labels, cluster_labels
    n = 50000
    src, dst, score, c = cc_inputs(n)
    s, d = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    cl, cnt = _cluster_labels(s, d, n, min_cluster_size, torch.from_numpy(score).cuda(),
                              torch.tensor([c], dtype=torch.float32, device="cuda"))
    rcl, rcnt = HR.cluster_labels_ref(src, dst, n, min_cluster_size, score, c)
    assert int(cnt) == rcnt and torch.equal(cl.cpu(), torch.from_numpy(rcl))
    # the public form (no score): a sparser graph, so that the size filter still has something to decide
    keep = HR.kept_edges(src, dst, n, score, c) | ~((src >= 0) & (dst >= 0) & (src < n) & (dst < n))
    s2, d2 = src[keep], dst[keep]
    cl = cluster_labels(torch.from_numpy(s2).cuda(), torch.from_numpy(d2).cuda(), n, min_cluster_size)
    rcl, rcnt = HR.cluster_labels_ref(s2, d2, n, min_cluster_size)
    assert rcnt > 1 and torch.equal(cl.cpu(), torch.from_numpy(rcl))
    empty = torch.zeros(0, dtype=torch.int64, device="cuda")
    assert bool((cluster_labels(empty, empty, 10, min_cluster_size) == -1).all())


# ------------------------------------------------------------------ the whole decision
@pytest.mark.parametrize("kind,training,start", [("normal", True, float("inf")), ("normal", False, float("inf")),
                                                 ("normal", True, 1.0), ("fallback", True, float("inf")),
                                                 ("empty", True, 0.5)],
                         ids=["normal-train", "normal-eval", "normal-train-finite", "fallback", "empty"])
def test_whole_decision(kind, training, start):
    from hierarchicalgnn_amd import clustering as C
    emb, graph = HR.decision_inputs(kind)
    ref = HR.decision_ref(emb, graph, np.float32(start), HPARAMS, training)
    if kind != "empty":                                      # the input condition, as asserted on the CPU: no mask
        delta = 100.0 * (CUT_ALLOWANCE_DECISION + HR.likelihood_error_bound(8, float(np.tanh(np.abs(ref["likelihood"]).max()))))
        assert float(np.abs(ref["likelihood"] - float(ref["score_cut"])).min()) > delta
    sc = torch.tensor([start], dtype=torch.float32, device="cuda")
    reads0 = C.stats["host_reads"]
    clusters, count = C.gmm_edge_clustering(torch.from_numpy(emb).cuda(), torch.from_numpy(graph).cuda(), sc, HPARAMS,
                                            training, return_count=True)
    torch.cuda.synchronize()
    assert C.stats["host_reads"] - reads0 == ref["host_reads"]
    assert count == ref["count"]
    assert clusters.dtype == torch.int64 and torch.equal(clusters.cpu(), torch.from_numpy(ref["clusters"]))
    got = float(sc.cpu()[0])
    if kind == "empty":
        assert got == start
    else:
        assert abs(got - float(ref["score_cut"])) <= CUT_ALLOWANCE_DECISION, (got, float(ref["score_cut"]))
        assert {"normal": 1, "fallback": 2}[kind] == ref["host_reads"]
