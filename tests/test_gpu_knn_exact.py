"""Exact conformance of the fixed-radius kNN kernels (csrc/knn.hip, csrc/knn_large.hip).

Inputs come from the dyadic grids of tests/hierarchy_ref.py (multiples of 2^-4 in [-4, 4], D <= 16, radius a multiple
of 2^-4), so every squared distance and r*r is exact in fp32 in any order: every comparison below is ``torch.equal``
on BOTH idx and d2 against the integer reference ``knn_ref``, ties included -- no tolerance, no gap mask.  The grids
are tie-heavy (a few dozen distinct distances) and a third of the cases carry exact duplicate points.  The radius is
one at which d2 == r^2 candidates exist, and every arm has both kinds of query.  At least one has FEWER than K points
strictly inside the radius (``hierarchy_ref.thin_inside``): there the correct row ends in padding, and a kernel that
keeps d2 == r^2 fills the padding instead.  At least one other has MORE than K points inside: its list fills, later
candidates are inserted into a full list and keys are dropped, so a wrong stable insertion, a wrong truncation at K or
a wrong merge of full slice lists shows.  A single query (nq = 1) cannot be both, so those arms run twice, on the
thinned and on the un-thinned points (``hierarchy_ref.tie_runs``).  The arms and their inputs are defined in
tests/hierarchy_ref.py; tests/test_hierarchy_ref.py proves the reference and asserts both conditions for every arm
without exception, and each test below asserts them again on the inputs it runs.

Outputs of the C ABI calls live inside poisoned buffers (guard elements before and after, which must be intact);
the workspace of the split forms is filled with a NaN pattern, so a partial list that is read but was never written
shows up as a garbage index.

Rotation rule of the K x D cross product (12 instantiations x 10 widths), i = index of K, j = index of D:
  launch form   split (np >= 512, workspace)  if (i + j) even, else BLOCK=64 unsplit -- through
                hgnn_knn_radius_f32 (no workspace, np >= 512) if (i + j) % 4 == 1, through np < 512 if == 3;
                every K meets both forms in each of the three D paddings
  np            rotates through the listed sizes of the form with (i + j) // 2
  nq            {1, 63, 64, 65} rotating with (i + 2 j); nq = 1 runs the thinned and the un-thinned points
  radius        by value / from a device tensor, alternating with (i + j) // 2
  duplicates    when (i + j) % 3 == 0
BLOCK=256: every K once, nq alternating 65536 / 65537, D rotating through all ten widths, np 40 / 270.

Kernel instantiation -> test id that reaches it:

  k_knn_radius<K, DP, BLOCK, SPLIT> (knn.hip), K in {1,2,3,4,5,6,8,10,12,16,20,32}
    <K, 4, 64, true>     HGNN_KNN_DP(4), split      test_k_by_d[K*-D{1,2,3,4}-split-*]
    <K, 8, 64, true>     HGNN_KNN_DP(8), split      test_k_by_d[K*-D{5,7,8}-split-*]
    <K, 16, 64, true>    HGNN_KNN_DP(16), split     test_k_by_d[K*-D{9,15,16}-split-*]
    <K, 4, 64, false>    HGNN_KNN_DP(4), unsplit    test_k_by_d[K*-D{1,2,3,4}-{nows,small}-*]
    <K, 8, 64, false>    HGNN_KNN_DP(8), unsplit    test_k_by_d[K*-D{5,7,8}-{nows,small}-*]
    <K, 16, 64, false>   HGNN_KNN_DP(16), unsplit   test_k_by_d[K*-D{9,15,16}-{nows,small}-*]
    <K, DP, 256, false>  nq >= 65536                test_block256[K*-*] (DP 4: D 1,2,3,4; DP 8: D 5,7,8; DP 16: D 9,15,16)
    the `d < D ? .. : 0` padding branch             every D that is not 4, 8 or 16
  k_knn_merge<K>                                    every *-split-* id above, test_np_edges[*-ws] with np >= 512,
                                                    test_slice_edges[*] (2 .. 32 slices, whole and ragged last slice)
  np = 0, 1, K-1, K, tile edges                     test_np_edges[*]
  radius 0 / beyond every distance / nothing near   test_radius_forms
  k_knn_large<DP, SPLIT> (knn_large.hip), K in 33..128
    <4, false> <8, false> <16, false>               test_large[K*-D{1,4}-unsplit], [K*-D7-unsplit], [K*-D16-unsplit]
    <4, true> <8, true> <16, true>                  test_large[K*-D{1,4}-split], [K*-D7-split], [K*-D16-split]
    lk_flush with hundreds of keys tied at thr      test_large_tied_threshold[*]
    np < K                                          test_large_np_below_k
  k_knn_large_merge                                 test_large[*-split], test_large_tied_threshold[*-split]
  knn_dispatch refusals                             test_unsupported
"""
import ctypes

import pytest
import torch

import hierarchy_ref as HR

pytestmark = pytest.mark.gpu

KS = HR.KNN_INSTANCES
DS = HR.KNN_DS
NQS = HR.KNN_NQS
POISON32 = 0x7FC0BEEF
POISON64 = 0x7FC0BEEF7FC0BEEF
ERR_INVALID_ARG, ERR_UNSUPPORTED = 1, 4


@pytest.fixture(scope="module", autouse=True)
def lib():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from hierarchicalgnn_amd import _lib
    return _lib.load()


def _L():
    from hierarchicalgnn_amd import _lib
    return _lib


class Guarded:
    """[nq, K] output inside a poisoned buffer with at least 64 guard elements on either side"""

    def __init__(self, nq, K, dtype):
        self.pad = K * -(-64 // K)
        n = nq * K
        wide = dtype == torch.int64
        self.buf = torch.empty(2 * self.pad + n, dtype=dtype, device="cuda")
        self.bits = self.buf if wide else self.buf.view(torch.int32)
        self.poison = POISON64 if wide else POISON32
        self.bits.fill_(self.poison)
        self.out = self.buf[self.pad:self.pad + n].view(nq, K)

    def ptr(self):
        return ctypes.c_void_p(self.out.data_ptr())

    def check(self, what):
        lo, hi = self.bits[:self.pad], self.bits[self.bits.numel() - self.pad:]
        assert bool((lo == self.poison).all()), f"{what}: wrote BEFORE the first output row"
        assert bool((hi == self.poison).all()), f"{what}: wrote PAST the last output row"
        n = int((self.bits[self.pad:self.bits.numel() - self.pad] == self.poison).sum())
        assert n == 0, f"{what}: {n} output elements never written"
        return self.out.cpu()


def workspace_bytes(nq, n_p, K):
    L = _L()
    nbytes = ctypes.c_size_t(0)
    L.check(L.load().hgnn_knn_workspace_bytes(nq, n_p, K, ctypes.byref(nbytes)), "hgnn_knn_workspace_bytes")
    return nbytes.value


def knn(q, p, K, r, ws=True, r_dev=False, expect_slices=None):
    """one C ABI call into guarded outputs.  ws=True: hgnn_knn_radius_ws_f32 with a NaN-filled workspace (the split form
    when the library wants slices); ws=False: hgnn_knn_radius_f32 (never splits)."""
    L = _L()
    qd, pd = q.cuda().contiguous(), p.cuda().contiguous()
    nq, D, n_p = int(q.shape[0]), int(q.shape[1]), int(p.shape[0])
    gi, gd = Guarded(nq, K, torch.int64), Guarded(nq, K, torch.float32)
    stream = L.current_stream(qd.device)
    if ws:
        nbytes = workspace_bytes(nq, n_p, K)
        if expect_slices is not None:
            assert nbytes == (nq * expect_slices * K * 8 if expect_slices > 1 else 0), (nbytes, expect_slices)
        wsb = None
        if nbytes:
            wsb = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda").fill_(POISON32)
        rd = torch.tensor([r], dtype=torch.float32, device="cuda") if r_dev else None
        rc = L.load().hgnn_knn_radius_ws_f32(L.ptr(qd), nq, L.ptr(pd), n_p, D, K, ctypes.c_float(-1.0 if r_dev else r),
                                             L.ptr(rd), gi.ptr(), gd.ptr(), L.ptr(wsb), nbytes, stream)
    else:
        assert not r_dev
        rc = L.load().hgnn_knn_radius_f32(L.ptr(qd), nq, L.ptr(pd), n_p, D, K, ctypes.c_float(r), gi.ptr(), gd.ptr(),
                                          stream)
    L.check(rc, "hgnn_knn_radius")
    torch.cuda.synchronize()
    return gi.check("knn idx"), gd.check("knn d2")


def assert_knn(out, ref, what):
    (idx, d2), (ridx, rd2) = out, ref
    assert idx.shape == ridx.shape and idx.dtype == ridx.dtype and d2.dtype == rd2.dtype
    if torch.equal(idx, ridx) and torch.equal(d2, rd2):
        return
    bad = torch.nonzero((idx != ridx) | (d2 != rd2))
    i, k = int(bad[0][0]), int(bad[0][1])
    raise AssertionError(f"{what}: {bad.shape[0]} of {idx.numel()} slots differ; first at query {i}, slot {k}: got "
                         f"({int(idx[i, k])}, {float(d2[i, k])}), want ({int(ridx[i, k])}, {float(rd2[i, k])})")


def expected_slices(nq, n_p):
    """knn_slices (knn.hip) restated"""
    if nq >= 65536 or n_p < 512:
        return 1
    want = min(-(-2048 // -(-nq // 64)), 32)
    if want <= 1:
        return 1
    ln = -(-(-(-n_p // want)) // 256) * 256
    return -(-n_p // ln)


def assert_cut_and_truncation_are_observable(runs, K):
    """over the runs of one arm: a witness of the strict cut, and a query whose list fills and drops keys"""
    q, p, r = runs[0]
    assert HR.strict_cut_witnesses(q, p, K, r) >= 1, "no query could tell d2 <= r^2 from d2 < r^2"
    assert sum(HR.truncating_queries(q, p, K, r) for q, p, r in runs) >= 1, "no query has more than K points inside"


def _kd_id(c):
    K, D, form, nq, n_p, r_dev, dup = c
    return f"K{K}-D{D}-{form}-q{nq}-p{n_p}-{'rdev' if r_dev else 'rval'}{'-dup' if dup else ''}"


@pytest.mark.parametrize("case", HR.kd_cases(), ids=_kd_id)
def test_k_by_d(case):
    K, D, form, nq, n_p, r_dev, dup = case
    runs = HR.kd_runs(case)
    assert len(runs) == (2 if nq == 1 else 1)
    assert_cut_and_truncation_are_observable(runs, K)
    slices = expected_slices(nq, n_p) if form == "split" else 1
    assert (slices > 1) == (form == "split")
    for n, (q, p, r) in enumerate(runs):
        out = knn(q, p, K, r, ws=form != "nows", r_dev=r_dev, expect_slices=slices if form != "nows" else None)
        assert_knn(out, HR.knn_ref(q, p, K, r), _kd_id(case) + ("", " (un-thinned)")[n])


def test_rotation_reaches_every_arm():
    """the pruning rule above leaves no (K, D padding, split / unsplit) arm out"""
    seen = {(K, 4 if D <= 4 else 8 if D <= 8 else 16, form == "split") for K, D, form, *_ in HR.kd_cases()}
    assert seen == {(K, dp, sp) for K in KS for dp in (4, 8, 16) for sp in (False, True)}
    assert {(K, D) for K, D, *_ in HR.kd_cases()} == {(K, D) for K in KS for D in DS}


@pytest.mark.parametrize("i", range(len(KS)), ids=lambda i: "K%d-D%d-q%d" % HR.block256_case(i)[:3])
def test_block256(i):
    K, D, nq, n_p = HR.block256_case(i)
    q, p, r = HR.block256_inputs(i)
    assert_cut_and_truncation_are_observable([(q, p, r)], K)
    out = knn(q, p, K, r, ws=i % 4 < 2, r_dev=i % 4 == 1, expect_slices=1 if i % 4 < 2 else None)
    assert_knn(out, HR.knn_ref(q, p, K, r), f"BLOCK=256 K{K} D{D}")


def test_block256_reaches_every_padding():
    assert {4 if DS[(3 * i) % 10] <= 4 else 8 if DS[(3 * i) % 10] <= 8 else 16 for i in range(len(KS))} == {4, 8, 16}


NP_EDGES = HR.NP_EDGES


@pytest.mark.parametrize("form", ["ws", "nows"])
@pytest.mark.parametrize("n", range(len(NP_EDGES)), ids=lambda n: f"np{NP_EDGES[n]}")
def test_np_edges(n, form):
    K, n_p, nq, D = HR.np_edge_case(n)
    runs = HR.np_edge_runs(n)
    if n_p >= 255:
        assert_cut_and_truncation_are_observable(runs, K)
    for q, p, r in runs:
        if n_p <= 16:
            r = 16.0                                        # everything inside: all np points must come back, then -1
        out = knn(q, p, K, r, ws=form == "ws", expect_slices=expected_slices(nq, n_p) if form == "ws" else None)
        ref = HR.knn_ref(q, p, K, r)
        if n_p <= 16:
            assert int((ref[0] >= 0).sum()) == nq * min(K, n_p)
        assert_knn(out, ref, f"np={n_p} K={K} D={D} nq={nq} {form}")


@pytest.mark.parametrize("nq,n_p,slices", HR.SLICE_EDGE_CASES)
def test_slice_edges(nq, n_p, slices):
    """slice_len at its 256-multiple edges, with want = 32 at the cap (1 query block), want = 16 (128 query blocks)
    and want = ceil(2048 / 66) = 32 reached without the cap (66 query blocks)"""
    assert expected_slices(nq, n_p) == slices
    K = HR.SLICE_EDGE_K
    q, p, r = HR.slice_edge_inputs(nq, n_p)
    assert_cut_and_truncation_are_observable([(q, p, r)], K)
    out = knn(q, p, K, r, ws=True, r_dev=True, expect_slices=slices)
    assert_knn(out, HR.knn_ref(q, p, K, r), f"slices nq={nq} np={n_p}")


def test_radius_forms():
    K = HR.RADIUS_FORMS_K
    q, p, r = HR.radius_forms_inputs()
    assert_cut_and_truncation_are_observable([(q, p, r)], K)
    at_radius = HR.knn_ref(q, p, K, r)
    assert bool((at_radius[0][:, K - 1] == -1).any()) and bool((at_radius[0][:, K - 1] >= 0).any())
    for ws, r_dev in ((True, False), (True, True), (False, False)):     # by value, from a device tensor, no workspace
        idx, d2 = knn(q, p, K, 0.0, ws=ws, r_dev=r_dev)
        assert bool((idx == -1).all()) and bool((d2 == -1).all()), "radius 0 keeps nothing (d2 = 0 is not < 0)"
        out = knn(q, p, K, 16.0, ws=ws, r_dev=r_dev)           # beyond every distance of the grid (max 3 * 64 < 256)
        ref = HR.knn_ref(q, p, K, 16.0)
        assert bool((ref[0] >= 0).all())
        assert_knn(out, ref, "radius beyond every distance")
        assert_knn(knn(q, p, K, r, ws=ws, r_dev=r_dev), at_radius, "radius at a grid distance")
    q, p = HR.far_apart(65, 700, 3, 5001)
    for K in (5, 64):
        idx, d2 = knn(q, p, K, 1.0)
        assert bool((idx == -1).all()) and bool((d2 == -1).all())


def test_unsupported():
    L = _L()
    q, p, r = HR.tie_inputs(8, 100, 3, 6000, 5)
    qd, pd = q.cuda(), p.cuda()
    stream = L.current_stream(qd.device)

    def call(K, D, radius):
        gi, gd = Guarded(8, max(K, 1), torch.int64), Guarded(8, max(K, 1), torch.float32)
        rc = L.load().hgnn_knn_radius_f32(L.ptr(qd), 8, L.ptr(pd), 100, D, K, ctypes.c_float(radius), gi.ptr(), gd.ptr(),
                                          stream)
        torch.cuda.synchronize()
        assert bool((gi.bits == POISON64).all()) and bool((gd.bits == POISON32).all()), "a refused call wrote output"
        return rc, (L.load().hgnn_last_error() or b"").decode()

    for K in (7, 9, 11, 24, 31):
        rc, msg = call(K, 3, r)
        assert rc == ERR_UNSUPPORTED and "1-6, 8, 10, 12, 16, 20, 32" in msg and f"K={K}" in msg, (rc, msg)
    for K in (0, 129):
        assert call(K, 3, r)[0] == ERR_INVALID_ARG
    for D in (0, 17):
        rc, msg = call(5, D, r)
        assert rc == ERR_INVALID_ARG and "D must be" in msg, (rc, msg)
    rc, msg = call(5, 3, -1.0)
    assert rc == ERR_INVALID_ARG and "negative radius" in msg, (rc, msg)


# ------------------------------------------------------------------ 33 <= K <= 128
@pytest.mark.parametrize("form", ["split", "unsplit"])
@pytest.mark.parametrize("D", HR.LARGE_DS)
@pytest.mark.parametrize("K", HR.LARGE_KS)
def test_large(K, D, form):
    nq, n_p, _ = HR.large_case(K, D, form)
    q, p, r = HR.large_inputs(K, D, form)
    assert_cut_and_truncation_are_observable([(q, p, r)], K)
    ws = form == "split" or n_p < 512
    out = knn(q, p, K, r, ws=ws, r_dev=ws and D == 7)
    if form == "split":
        assert workspace_bytes(nq, n_p, K) > 0
    ref = HR.knn_ref(q, p, K, r)
    assert_knn(out, ref, f"large K{K} D{D} {form}")
    out32 = knn(q, p, 32, r, ws=ws)
    assert torch.equal(out[0][:, :32], out32[0]) and torch.equal(out[1][:, :32], out32[1]), "K = 32 prefix"


@pytest.mark.parametrize("form", ["split", "unsplit"])
@pytest.mark.parametrize("K", [5, 32, 33, 64, 100, 128])
def test_large_tied_threshold(K, form):
    """400 candidates at ONE distance from the first query with 40 points strictly nearer: for K > 40 the K-th key lies
    inside the tie, the running threshold equals the tied distance, every later tied candidate passes `d2 <= thr` and
    the 256-entry buffer is re-sorted again and again; the lower indices of the tie must win"""
    D = 4
    pts, shell = HR.tie_shell(D, 40, 400, 300, 8000)
    q = torch.cat([torch.zeros(1, D), HR.tie_points(20, D, 8001)])
    r = 3.0                                                  # shell d2 = 5 < 9: the whole tie is inside the radius
    assert shell == 5 * HR.D2_UNIT_INV
    ref = HR.knn_ref(q, pts, K, r)
    if K > 40:
        assert float(ref[1][0, K - 1]) * HR.D2_UNIT_INV == shell and float(ref[1][0, 39]) * HR.D2_UNIT_INV < shell
    out = knn(q, pts, K, r, ws=form == "split")
    if form == "split":
        assert workspace_bytes(q.shape[0], pts.shape[0], K) > 0
    assert_knn(out, ref, f"tied threshold K{K} {form}")


def test_large_np_below_k():
    for K, n_p in ((33, 32), (64, 20), (128, 127), (100, 1)):
        q, p, _ = HR.tie_inputs(17, n_p, 3, 9000 + K, K)
        for ws in (True, False):
            out = knn(q, p, K, 16.0, ws=ws)
            ref = HR.knn_ref(q, p, K, 16.0)
            assert int((ref[0] >= 0).sum()) == 17 * n_p
            assert_knn(out, ref, f"np={n_p} < K={K}")


# ------------------------------------------------------------------ the module that uses it
@pytest.mark.parametrize("sym", [False, True])
def test_dynamic_graph_construction_on_dyadic_input(sym):
    from hierarchicalgnn_amd.graph_construction import DynamicGraphConstruction
    D, k = 8, 10
    half, r = HR.tie_case(D)
    n_src, n_dst = (600, 600) if sym else (700, 300)
    src, dst = HR.tie_points(n_src, D, 9100), HR.tie_points(n_dst, D, 9101)
    m = DynamicGraphConstruction("exp", {}).cuda().eval()
    m.knn_radius.fill_(r)
    graph, w = m(src.cuda(), dst.cuda(), sym=sym, k=k)
    ref = HR.edges_from_knn(HR.knn_ref(src, dst, k, r)[0], sym, max(n_src, n_dst))
    assert ref.shape[1] > 1000
    assert torch.equal(graph.cpu(), ref)
    assert w.shape == (ref.shape[1], 1) and bool(torch.isfinite(w).all())
    assert float(m.knn_radius) == r, "eval mode leaves the radius alone"
