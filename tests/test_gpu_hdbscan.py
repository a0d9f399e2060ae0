"""GPU tests of hierarchicalgnn_amd.hdbscan (csrc/hdbscan.hip) against the numpy restatement's results stored in
tests/golden/hdbscan_cases.npz (tests/hdbscan_ref.py, tests/golden/make_hdbscan_golden.py).

Figures of one MI355X run: continuous case A = 0.959054 (sklearn against itself), ARI against sklearn 0.964693, ARI
against the restatement 1.0, sorted MST w2 equal to the restatement's to the bit; N = 20k: 6 rounds, 8 host reads."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdbscan_ref as R  # noqa: E402
from golden import make_hdbscan_golden as G  # noqa: E402

from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return load_golden("hdbscan_cases.npz")


@pytest.fixture(scope="module")
def H():
    import hierarchicalgnn_amd
    return hierarchicalgnn_amd


def _hdb():
    return importlib.import_module("hierarchicalgnn_amd.hdbscan")


def _x(cases, name):
    return torch.from_numpy(cases[name + "/q"].astype(np.float32) / np.float32(128.0)).cuda()


def _ari(a, b):
    """adjusted Rand index (noise is one more label, as sklearn.metrics.adjusted_rand_score counts it)"""
    a, b = np.unique(a, return_inverse=True)[1], np.unique(b, return_inverse=True)[1]
    m = np.zeros((a.max() + 1, b.max() + 1), np.float64)
    np.add.at(m, (a, b), 1)
    c2 = lambda v: (v * (v - 1) / 2).sum()  # noqa: E731
    s, sa, sb, n = c2(m), c2(m.sum(1)), c2(m.sum(0)), len(a) * (len(a) - 1) / 2
    e = sa * sb / n
    return (s - e) / (0.5 * (sa + sb) - e)


@pytest.mark.parametrize("name", list(G.EXACT))
def test_exact_cases(H, cases, name):
    mcs, ms = G.EXACT[name]
    labels, edges, w2, core2 = H.hdbscan_tree(_x(cases, name), mcs, None if ms == mcs else ms)
    assert labels.dtype == torch.int64 and labels.is_cuda and edges.dtype == torch.int64
    # core2 bit-equal
    assert np.array_equal(core2.cpu().numpy().view(np.uint32), cases[name + "/core2"].view(np.uint32))
    # MST edge set and w2, as sorted (min, max) pairs
    e, w = edges.cpu().numpy(), w2.cpu().numpy()
    assert (e[:, 0] < e[:, 1]).all()
    o = np.lexsort((e[:, 1], e[:, 0]))
    re, rw = cases[name + "/edges"].astype(np.int64), cases[name + "/w2"]
    ro = np.lexsort((re[:, 1], re[:, 0]))
    assert np.array_equal(e[o], re[ro])
    assert np.array_equal(w[o].view(np.uint32), rw[ro].view(np.uint32))
    # the library's own order is (w2, min, max), which is the restatement's
    assert np.array_equal(e, re) and np.array_equal(w, rw)
    # labels element for element (both are in the canonical numbering)
    got = labels.cpu().numpy()
    assert np.array_equal(got, R.canonical(got))
    assert np.array_equal(got, cases[name + "/labels"])


def test_default_min_samples_is_min_cluster_size(H, cases):
    x = _x(cases, "ms10")   # min_cluster_size 4: default min_samples 4 differs from the stored min_samples 10 run
    a = H.hdbscan_tree(x, 4)
    b = H.hdbscan_tree(x, 4, 4)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert not torch.equal(a[3], H.hdbscan_tree(x, 4, 10)[3])


def test_permutation_invariance(H, cases):
    """sklearn cannot pass this (its tie order follows the point order); this definition must"""
    x = _x(cases, "tracks300")
    base = cases["tracks300/labels"]
    for seed in (1, 2):
        p = np.random.default_rng(seed).permutation(len(base))
        lp = H.hdbscan(x[torch.from_numpy(p).cuda()], 5).cpu().numpy()
        back = np.empty_like(lp)
        back[p] = lp
        assert np.array_equal(R.canonical(back), base)


def test_continuous_case(H, cases):
    x = torch.from_numpy(cases["continuous/x"]).cuda()
    labels, edges, w2, core2 = H.hdbscan_tree(x, 5)
    a = float(cases["continuous/AB"][0])
    b = _ari(cases["continuous/sklearn_labels"], labels.cpu().numpy())
    w, rw = np.sort(w2.cpu().numpy()).astype(np.float64), np.sort(cases["continuous/w2"]).astype(np.float64)
    rel = float((np.abs(w - rw) / rw).max())
    print(f"continuous: A = {a:.6f}, ARI vs sklearn = {b:.6f}, ARI vs restatement = "
          f"{_ari(cases['continuous/labels'], labels.cpu().numpy()):.6f}, max rel w2 error = {rel:.3g}")
    assert a < 1.0
    assert 1 - b <= 2 * (1 - a)
    assert rel <= 4 * 2.0 ** -24   # float32 rounding of an 8-term sum; not tuned


def test_track_candidates_feed_eval_metrics(H, cases):
    name = "tracks300"
    x = _x(cases, name)
    ref = torch.from_numpy(cases[name + "/labels"].astype(np.int64)).cuda()
    n = ref.numel()
    g = torch.Generator().manual_seed(3)
    # truth: mostly the reference clusters, a fifth of the hits reassigned at random, noise = 0
    pid = ref + 1
    swap = torch.rand(n, generator=g) < 0.2
    pid = torch.where(swap.cuda(), torch.randint(0, int(ref.max()) + 2, (n,), generator=g).cuda(), pid)
    event = {"pid": pid, "pt": (0.5 + 2 * torch.rand(n, generator=g)).cuda()}
    inverse_mask = torch.randperm(n, generator=g).cuda()
    event = {"pid": torch.empty_like(pid).scatter_(0, inverse_mask, pid),
             "pt": torch.empty_like(event["pt"]).scatter_(0, inverse_mask, event["pt"])}
    graph = H.embedding_track_candidates(x, inverse_mask, 5)
    hits = torch.nonzero(ref >= 0).reshape(-1)
    expect = torch.stack([inverse_mask[hits], ref[hits]])
    assert graph.dtype == torch.int64 and torch.equal(graph, expect)
    plain = H.embedding_track_candidates(x, None, 5)
    assert torch.equal(plain, torch.stack([hits, ref[hits]]))
    got = H.eval_metrics(graph, event, pt_cut=1.0, nhits_cut=5, majority_cut=0.5, primary=False)
    want = H.eval_metrics(expect, event, pt_cut=1.0, nhits_cut=5, majority_cut=0.5, primary=False)
    assert got == want and set(got) == {"track_eff", "track_pur", "hit_eff", "hit_pur"}
    assert 0 < got["track_eff"] <= 1


def test_cuml_shim_fit_predict(H, cases):
    sys.path.insert(0, os.path.join(ROOT, "cuml_shim"))
    try:
        from cuml.cluster import HDBSCAN
    finally:
        sys.path.pop(0)
    x = _x(cases, "d3")
    model = HDBSCAN(min_cluster_size=5, metric="euclidean", cluster_selection_method="eom", verbose=0)
    out = model.fit_predict(x)
    assert np.array_equal(torch.as_tensor(out).long().cpu().numpy(), cases["d3/labels"])

    class Capsule:   # anything exposing DLPack
        def __init__(self, t):
            self.t = t

        def __dlpack__(self, stream=None):
            return self.t.__dlpack__()

        def __dlpack_device__(self):
            return self.t.__dlpack_device__()
    assert torch.equal(model.fit_predict(Capsule(x)), out)


def test_repeatability_and_host_reads(H):
    from hierarchicalgnn_amd import synth
    hdb = _hdb()
    x = synth.embedding_event(20_000, 8, seed=5)["embeddings"].cuda()
    r0 = hdb.stats["host_reads"]
    a = H.hdbscan_tree(x, 5)
    reads = hdb.stats["host_reads"] - r0
    print("N = 20k:", hdb.stats["last"])
    assert reads == hdb.stats["last"]["host_reads"] == hdb.stats["last"]["rounds"] + 2
    assert reads <= 24
    b = H.hdbscan_tree(x, 5)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    kept = a[0][a[0] >= 0]
    assert kept.numel() > 0 and int(torch.bincount(kept).min()) >= 5


def test_non_finite_points_are_an_error_not_a_fault(H):
    x = torch.full((300, 8), float("nan"), device="cuda")
    with pytest.raises(RuntimeError, match="joined nothing"):
        H.hdbscan(x, 5)


FULL_SIZE = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
import hierarchicalgnn_amd as H
from hierarchicalgnn_amd import synth
x = synth.embedding_event(120_000, 8)["embeddings"].cuda()
labels, edges, w2, core2 = H.hdbscan_tree(x, 5)
torch.cuda.synchronize()
kept = labels[labels >= 0]
counts = torch.bincount(kept)
assert labels.numel() == 120_000 and edges.shape == (119_999, 2)
assert kept.numel() > 0 and int(counts.min()) >= 5, int(counts.min())
assert int(edges.min()) >= 0 and int(edges.max()) < 120_000 and bool((edges[:, 0] < edges[:, 1]).all())
assert bool((w2[1:] >= w2[:-1]).all()) and bool(torch.isfinite(w2).all())
# the edges span: N - 1 edges that the tree stage accepted as acyclic
print("full size ok: clusters", int(counts.numel()), "noise", int((labels < 0).sum()))
"""


def test_full_size_event_completes():
    """N = 120k (N^2 > 2^32): guards workspace sizing and index arithmetic; compared to nothing.  A fresh child
    process under its own time limit."""
    r = subprocess.run([sys.executable, "-c", FULL_SIZE, ROOT], timeout=420, capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "full size ok" in r.stdout
