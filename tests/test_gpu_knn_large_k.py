"""GPU: fixed-radius kNN for 33 <= K <= 128 (csrc/knn_large.hip), the embedding stage's knn: 100.  The contract
does not depend on the algorithm: the K smallest (d2, idx) pairs with d2 < r^2, ascending, -1 padded, d2 from
k_knn_radius's arithmetic."""
import ctypes

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu


def _points(n, D, seed, dup_every=0):
    g = torch.Generator().manual_seed(seed)
    p = torch.nn.functional.normalize(torch.randn(n, D, generator=g))
    if dup_every:
        p[1::dup_every] = p[0::dup_every][: p[1::dup_every].shape[0]]
    return p


def _oracle(q, p, K, r):
    """the oracle's K + 1 nearest: the extra column tells whether slot K - 1 is a near-tie with the first point left
    out (the oracle sums t * t without fma, so such a pair may swap across the cut)"""
    from oracle import hgnn_oracle as O
    return O.knn_radius(q, p, K + 1, r)


def _gap_checked(idx, d2, idx_ref, d_ref):
    K = idx.shape[1]
    gap_ok = torch.ones_like(idx_ref, dtype=torch.bool)
    gap_ok[:, 1:] &= (d_ref[:, 1:] - d_ref[:, :-1]).abs() > 1e-5
    gap_ok[:, :-1] &= (d_ref[:, 1:] - d_ref[:, :-1]).abs() > 1e-5
    if idx_ref.shape[1] > K:
        idx_ref, d_ref, gap_ok = idx_ref[:, :K], d_ref[:, :K], gap_ok[:, :K]
    assert torch.equal(idx >= 0, idx_ref >= 0)
    assert rel_err(d2.numpy(), d_ref.numpy()) <= 1e-5
    assert torch.equal(idx[gap_ok], idx_ref[gap_ok])


@pytest.mark.parametrize("K", [33, 48, 64, 100, 128])
@pytest.mark.parametrize("D", [3, 8, 16])
@pytest.mark.parametrize("nq,np_,r", [(300, 700, 1.0), (90, 60, 1.5), (2000, 1500, 0.8)])
def test_large_k_vs_oracle(K, D, nq, np_, r):
    from hierarchicalgnn_amd.ops import knn_radius
    q = _points(nq, D, nq + K + D)
    p = _points(np_, D, np_ + 7 * K + D)
    idx_ref, d_ref = _oracle(q, p, K, r)
    radius = torch.tensor([r], device="cuda") if K % 2 else r      # both radius forms
    idx, d2 = knn_radius(q.cuda(), p.cuda(), K, radius, return_dist2=True)
    assert idx.shape == (nq, K)
    _gap_checked(idx.cpu(), d2.cpu(), idx_ref, d_ref)


@pytest.mark.parametrize("nq,np_,K", [(100, 5000, 100), (700, 3000, 64), (40, 1025, 128)])
def test_split_path_equals_single_pass(nq, np_, K):
    """few queries: the candidates are split over workgroups and merged; same bits as one pass (no workspace)"""
    from hierarchicalgnn_amd import _lib
    from hierarchicalgnn_amd.ops import knn_radius
    pts = _points(np_, 8, np_ + K, dup_every=5).cuda()
    q = pts[:nq].clone()
    idx, d2 = knn_radius(q, pts, K, 1.2, return_dist2=True)
    ref_idx, ref_d2 = torch.empty_like(idx), torch.empty_like(d2)
    lib = _lib.load()
    _lib.check(lib.hgnn_knn_radius_f32(_lib.ptr(q), nq, _lib.ptr(pts), np_, 8, K, ctypes.c_float(1.2),
                                       _lib.ptr(ref_idx), _lib.ptr(ref_d2), _lib.current_stream(q.device)))
    assert torch.equal(idx, ref_idx) and torch.equal(d2, ref_d2)
    nbytes = ctypes.c_size_t(0)
    _lib.check(lib.hgnn_knn_workspace_bytes(nq, np_, K, ctypes.byref(nbytes)))
    assert nbytes.value > 0                                       # the split is actually exercised
    idx_ref, d_ref = _oracle(q.cpu(), pts.cpu(), K, 1.2)
    _gap_checked(idx.cpu(), d2.cpu(), idx_ref, d_ref)


def test_exact_duplicates_and_prefix_equals_k32():
    """exact duplicate points tie: the lower index comes first; the first 32 columns of K = 64 (and K = 100) equal
    the K = 32 kernel's result bit for bit"""
    from hierarchicalgnn_amd.ops import knn_radius
    pts = _points(3000, 8, 5, dup_every=3).cuda()
    i32, d32 = knn_radius(pts, pts, 32, 1.0, return_dist2=True)
    for K in (64, 100):
        iK, dK = knn_radius(pts, pts, K, 1.0, return_dist2=True)
        assert torch.equal(iK[:, :32], i32) and torch.equal(dK[:, :32], d32)
    i64, d64 = knn_radius(pts, pts, 64, 1.0, return_dist2=True)
    ok = i64 >= 0
    same = ok[:, 1:] & ok[:, :-1] & (d64[:, 1:] == d64[:, :-1])
    assert bool(same.any())                                       # ties exist
    assert bool((i64[:, 1:][same] > i64[:, :-1][same]).all())     # and go to the lower index
    dd = torch.where(ok, d64, torch.full_like(d64, 9.0))
    assert bool((dd[:, 1:] >= dd[:, :-1]).all())


def test_repeated_calls_are_bitwise_equal():
    from hierarchicalgnn_amd.ops import knn_radius
    pts = _points(20_000, 8, 9).cuda()
    a = knn_radius(pts, pts, 100, 1.0, return_dist2=True)
    for _ in range(2):
        b = knn_radius(pts, pts, 100, 1.0, return_dist2=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("K", [0, 129])
def test_out_of_range_k_is_rejected(K):
    from hierarchicalgnn_amd.ops import knn_radius
    pts = _points(100, 8, 1).cuda()
    with pytest.raises(RuntimeError, match=r"K must be in \[1, 128\]"):
        knn_radius(pts, pts, K, 1.0)


def test_full_size_clustered_k100():
    """N = 120k self-queries, D = 8, K = 100, r = 1 on clustered embeddings; sampled rows against the oracle"""
    from hierarchicalgnn_amd import synth
    from hierarchicalgnn_amd.ops import knn_radius
    emb = synth.embedding_event(120_000)["embeddings"]
    idx, d2 = knn_radius(emb.cuda(), emb.cuda(), 100, 1.0, return_dist2=True)
    idx, d2 = idx.cpu(), d2.cpu()
    ok = idx >= 0
    assert float(d2[ok].max()) < 1.0
    assert bool((idx[:, 0] == torch.arange(120_000)).float().mean() > 0.99)   # the point itself first (d2 = 0)
    g = torch.Generator().manual_seed(3)
    sel = torch.randint(0, 120_000, (64,), generator=g)
    idx_ref, d_ref = _oracle(emb[sel], emb, 100, 1.0)
    _gap_checked(idx[sel], d2[sel], idx_ref, d_ref)
