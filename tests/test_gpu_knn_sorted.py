"""GPU: the spatially sorted fixed-radius kNN (csrc/knn_sorted.hip, ``knn_radius(..., method="sorted")``).

Its contract is the brute-force kernels': the K smallest (d2, idx) pairs with d2 < r^2, ascending, -1 padded, d2 from
the same fmaf chain.  So every comparison here is ``torch.equal`` on idx AND d2 -- against the brute-force kernel on
the same input, and against the integer reference ``hierarchy_ref.knn_ref`` on that file's exact-grid inputs.  Where
the brute-force kernels have no instantiation (K = 7, 9, 15, 31) the reference is the first K columns of the next
supported K: the result is a prefix of the (d2, idx) order, whatever K.
"""
import pytest
import torch

import hierarchy_ref as R

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 255, 256, 257, 1000, 4099)      # tile (256) and group (16, 64) edges
DS = (1, 3, 8, 16)
KS = (1, 7, 32, 33, 100, 128)


def _brute(q, p, K, r):
    """(idx, d2) of the brute-force kernel; an unsupported K <= 32 is the prefix of the next supported one"""
    from hierarchicalgnn_amd.ops import knn_radius
    Kb = K if K > 32 else min(k for k in R.KNN_INSTANCES if k >= K)
    idx, d2 = knn_radius(q, p, Kb, r, return_dist2=True)
    return idx[:, :K].contiguous(), d2[:, :K].contiguous()


def _sorted(q, p, K, r):
    from hierarchicalgnn_amd.ops import knn_radius
    return knn_radius(q, p, K, r, return_dist2=True, method="sorted")


def _assert_same(got, want, what=""):
    assert got[0].shape == want[0].shape and got[0].dtype == torch.int64 and got[1].dtype == torch.float32
    assert torch.equal(got[0].cpu(), want[0].cpu()), f"{what}: idx differs"
    assert torch.equal(got[1].cpu(), want[1].cpu()), f"{what}: d2 differs"


def _cloud(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, D, generator=g)


def _radius(n, D):
    """a radius whose ball holds a few hundred of n uniform points of [0, 1]^D at most: lists that fill (more than K
    inside) and lists that do not both occur"""
    return 0.5 * min(1.0, (200.0 / max(n, 1)) ** (1.0 / D)) * (D ** 0.5)


def _size_cases():
    cases = []
    for i, n in enumerate(SIZES):
        for j, K in enumerate(KS):
            D = DS[(i + j) % 4]
            cases.append((n, n, D, K, True))                          # self-search
            cases.append((SIZES[(i + 3 + j) % 8], n, D, K, False))    # its own query set, nq != np but for one rotation
    return cases


@pytest.mark.parametrize("nq,n_p,D,K,self_search", _size_cases())
def test_equals_brute_force_over_sizes(nq, n_p, D, K, self_search):
    """nq, np over the tile and group edges x D x K (K > np included: np = 1, 63, 64 with K = 100, 128)"""
    p = _cloud(n_p, D, 11 * n_p + D).cuda()
    q = p if self_search else _cloud(nq, D, 13 * nq + K).cuda()
    r = _radius(n_p, D)
    got = _sorted(q, p, K, r)
    assert got[0].shape == (nq, K)
    _assert_same(got, _brute(q, p, K, r), f"nq={nq} np={n_p} D={D} K={K}")
    if self_search:
        assert bool((got[0][:, 0] >= 0).all())                        # every point finds itself


def test_size_cases_cover_what_they_claim():
    cases = _size_cases()
    assert {c[0] for c in cases} == set(SIZES) == {c[1] for c in cases}
    assert {c[2] for c in cases} == set(DS) and {c[3] for c in cases} == set(KS)
    assert any(c[0] != c[1] for c in cases) and any(c[3] > c[1] for c in cases)
    assert any(c[0] == c[1] and not c[4] for c in cases)              # equal sizes, two arrays: two sorts


@pytest.mark.parametrize("K", [7, 9, 15, 31])
def test_every_k_prefix_of_next_supported(K):
    p = _cloud(1500, 3, K).cuda()
    q = _cloud(333, 3, K + 1).cuda()
    _assert_same(_sorted(q, p, K, 0.2), _brute(q, p, K, 0.2), f"K={K}")
    _assert_same(_sorted(p, p, K, 0.2), _brute(p, p, K, 0.2), f"K={K} self")


@pytest.mark.parametrize("nq,n_p,D,K,dup", [(65, 700, 3, 7, False), (64, 1025, 8, 33, True), (37, 513, 16, 100, False),
                                             (63, 257, 1, 9, True), (1, 1300, 4, 128, False), (300, 4099, 2, 32, True)])
def test_exact_grid_equals_integer_reference(nq, n_p, D, K, dup):
    """tie-heavy dyadic inputs (d2 == r^2 candidates, exact duplicates): the integer reference, bit for bit"""
    for q, p, r in R.tie_runs(nq, n_p, D, 9000 + K + D, K, dup):
        got = _sorted(q.cuda(), p.cuda(), K, r)
        _assert_same(got, R.knn_ref(q, p, K, r), f"grid D={D} K={K}")
        _assert_same(got, _brute(q.cuda(), p.cuda(), K, r), f"grid D={D} K={K} vs brute")


@pytest.mark.parametrize("D,K", [(3, 33), (8, 7), (16, 100)])
def test_mass_ties_on_the_unit_grid(D, K):
    """grid_points: 9 levels per dimension, many equal d2 decide the index order; fine_points: every grid value"""
    for gen, n in ((R.grid_points, 2000), (R.fine_points, 1000)):
        p = R.with_duplicates(gen(n, D, 50 + D), 51 + D)
        q = gen(130, D, 52 + D)
        r = R.tie_case(D)[1]
        got = _sorted(q.cuda(), p.cuda(), K, r)
        _assert_same(got, R.knn_ref(q, p, K, r), f"{gen.__name__} D={D}")


@pytest.mark.parametrize("K", [7, 33])
def test_all_points_identical(K):
    """a degenerate box in every dimension and one shared key: every candidate ties, index order decides"""
    p = torch.full((600, 3), 0.75).cuda()
    got = _sorted(p, p, K, 1.0)
    _assert_same(got, _brute(p, p, K, 1.0))
    assert torch.equal(got[0].cpu(), torch.arange(K).expand(600, K))
    assert bool((got[1] == 0).all())
    q = torch.tensor([[0.75, 0.75, 0.75], [0.75, 0.75, 1.25], [9.0, 9.0, 9.0]]).cuda()
    _assert_same(_sorted(q, p, K, 1.0), _brute(q, p, K, 1.0))


@pytest.mark.parametrize("K", [9, 100])
def test_duplicates_straddle_a_tile_boundary(K):
    """300 exact copies of one point share a key, so after sorting they are consecutive and cross a 256-point tile
    boundary wherever the run starts; their order in every list must still be the index order"""
    g = torch.Generator().manual_seed(77)
    p = R.fine_points(1200, 3, 78)
    where = torch.randperm(1200, generator=g)[:300]
    p[where] = p[int(where[0])].clone()
    q = torch.cat([p[where[:5]], R.fine_points(60, 3, 79)])
    for r in (0.5, 8.0):
        got = _sorted(q.cuda(), p.cuda(), K, r)
        _assert_same(got, R.knn_ref(q, p, K, r), f"r={r}")
        assert torch.equal(got[0][0, :K].cpu(), torch.sort(where).values[:K])
    _assert_same(_sorted(p.cuda(), p.cuda(), K, 0.5), _brute(p.cuda(), p.cuda(), K, 0.5))


@pytest.mark.parametrize("D,K", [(3, 8), (8, 33)])
def test_radius_forms(D, K):
    p = _cloud(3000, D, 5).cuda()
    q = _cloud(500, D, 6).cuda()
    idx, d2 = _sorted(q, p, K, 0.0)                                   # strict <: nothing, not even a coincident point
    assert bool((idx == -1).all()) and bool((d2 == -1).all())
    idx, d2 = _sorted(p, p, K, 0.0)
    assert bool((idx == -1).all())
    # cuts mid-list: the median over the queries of the distance to the K-th neighbour, so about half the rows fill
    r_mid = float(torch.cdist(q.cpu().double(), p.cpu().double()).kthvalue(K, dim=1).values.median())
    got = _sorted(q, p, K, r_mid)
    full = (got[0] >= 0).all(1)
    assert bool(full.any()) and not bool(full.all())
    _assert_same(got, _brute(q, p, K, r_mid), "mid")
    got = _sorted(q, p, K, 1e6)                                       # no radius pruning: the thr_q bound alone
    assert bool((got[0] >= 0).all())
    _assert_same(got, _brute(q, p, K, 1e6), "huge")
    r_dev = torch.tensor([r_mid], device="cuda")                      # the module's knn_radius buffer
    _assert_same(_sorted(q, p, K, r_dev), _brute(q, p, K, r_mid), "device radius")
    _assert_same(_sorted(q, p, K, r_dev), _brute(q, p, K, r_dev), "device radius, both")


@pytest.mark.parametrize("K", [5, 33])
def test_queries_far_outside_the_points_box(K):
    p = _cloud(2000, 3, 21).cuda()
    q = (_cloud(300, 3, 22) + torch.tensor([50.0, -20.0, 0.0])).cuda()
    idx, _ = _sorted(q, p, K, 1.0)
    assert bool((idx == -1).all())
    _assert_same(_sorted(q, p, K, 1.0), _brute(q, p, K, 1.0), "none in reach")
    r = 54.0                                                          # reaches part of the cloud
    got = _sorted(q, p, K, r)
    assert bool((got[0] >= 0).any())
    _assert_same(got, _brute(q, p, K, r), "far, in reach")
    mixed = torch.cat([q[:100], p[:100]])                             # near and far queries in one call
    _assert_same(_sorted(mixed, p, K, 0.3), _brute(mixed, p, K, 0.3), "mixed")
    fq, fp = R.far_apart(70, 900, 4, 23)
    got = _sorted(fq.cuda(), fp.cuda(), K, 1.0)
    assert bool((got[0] == -1).all())
    _assert_same(got, R.knn_ref(fq, fp, K, 1.0), "far_apart")


@pytest.mark.parametrize("D,K", [(3, 8), (8, 33), (16, 100)])
def test_non_finite_coordinates_equal_brute_force(D, K):
    """rows with NaN or +-inf in the points and in the queries: whatever the brute-force kernel makes of them"""
    nan, inf = float("nan"), float("inf")
    p = _cloud(1500, D, 31)
    q = _cloud(400, D, 32)
    g = torch.Generator().manual_seed(33)
    for t, rows in ((p, torch.randperm(1500, generator=g)[:40]), (q, torch.randperm(400, generator=g)[:24])):
        for n, i in enumerate(rows.tolist()):
            t[i, n % D] = (nan, inf, -inf, nan)[n % 4]
            if n % 5 == 0:
                t[i, (n + 1) % D] = (inf, -inf)[n % 2]
    p[7] = inf                                                        # whole rows
    p[8] = nan
    q[3] = -inf
    r = _radius(1500, D)
    for qq in (q.cuda(), p.cuda()):
        for rr in (r, 1e6, inf):
            _assert_same(_sorted(qq, p.cuda(), K, rr), _brute(qq, p.cuda(), K, rr), f"r={rr}")
    allnan = torch.full((300, D), nan).cuda()                         # no finite coordinate at all: an empty box
    _assert_same(_sorted(allnan, allnan, K, 1.0), _brute(allnan, allnan, K, 1.0), "all NaN")
    _assert_same(_sorted(q.cuda(), allnan, K, 1.0), _brute(q.cuda(), allnan, K, 1.0), "NaN points")


def test_two_calls_are_bitwise_equal_and_so_are_their_stats():
    from hierarchicalgnn_amd.ops import knn_radius_stats
    p = torch.nn.functional.normalize(_cloud(4099, 8, 41) - 0.5).cuda()
    a = _sorted(p, p, 100, 1.0)
    sa = knn_radius_stats()
    b = _sorted(p, p, 100, 1.0)
    sb = knn_radius_stats()
    _assert_same(a, b)
    assert sa == sb
    groups, tiles = -(-4099 // 16), -(-4099 // 256)
    assert sa[0] + sa[1] == groups * tiles and sa[0] >= groups


def test_radius_pruning_skips_the_other_cluster():
    """two clusters of 1024 points, spread <= 0.1, centres 100 apart along the diagonal (so the top bit of every
    dimension separates them and each 256-point tile lies in one cluster): with r = 1 every group must skip the other
    cluster's 4 of the 8 tiles"""
    from hierarchicalgnn_amd.ops import knn_radius_stats
    g = torch.Generator().manual_seed(61)
    a = torch.rand(1024, 8, generator=g) * 0.1 / 8 ** 0.5
    b = torch.rand(1024, 8, generator=g) * 0.1 / 8 ** 0.5 + 100.0 / 8 ** 0.5
    p = torch.cat([a, b])[torch.randperm(2048, generator=g)].cuda()
    got = _sorted(p, p, 33, 1.0)
    visited, skipped = knn_radius_stats()
    assert visited + skipped == (2048 // 16) * 8
    assert skipped >= visited, (visited, skipped)
    _assert_same(got, _brute(p, p, 33, 1.0))


def test_the_dynamic_bound_alone_prunes():
    """points on a line, r = 1e6 (every point is inside the radius): only thr_q can skip a tile"""
    from hierarchicalgnn_amd.ops import knn_radius_stats
    g = torch.Generator().manual_seed(62)
    t = torch.rand(4096, 1, generator=g) * 1000.0
    p = (t * torch.ones(1, 8)).cuda()
    got = _sorted(p, p, 33, 1e6)
    visited, skipped = knn_radius_stats()
    assert skipped > 0, (visited, skipped)
    assert visited + skipped == (4096 // 16) * 16
    _assert_same(got, _brute(p, p, 33, 1e6))


@pytest.mark.parametrize("K", [0, 129])
def test_out_of_range_k_is_rejected(K):
    p = _cloud(100, 8, 1).cuda()
    with pytest.raises(RuntimeError, match=r"K must be in \[1, 128\]"):
        _sorted(p, p, K, 1.0)


def test_empty_sides():
    p = _cloud(100, 3, 2).cuda()
    none = torch.empty(0, 3, device="cuda")
    idx, d2 = _sorted(p, none, 7, 1.0)                                # np == 0: all padding
    assert idx.shape == (100, 7) and bool((idx == -1).all()) and bool((d2 == -1).all())
    idx, d2 = _sorted(none, p, 7, 1.0)                                # nq == 0
    assert idx.shape == (0, 7) and d2.shape == (0, 7)


def test_frnn_graph_sorted_equals_default():
    import hierarchicalgnn_amd as H
    g = torch.Generator().manual_seed(71)
    emb = torch.nn.functional.normalize(torch.randn(3000, 8, generator=g)).cuda()
    want = H.frnn_graph(emb, 1.0, 100)
    got = H.frnn_graph(emb, 1.0, 100, method="sorted")
    assert want.shape[1] > 3000 and torch.equal(got, want)
    batch = {"modulewise_true_edges": torch.randint(0, 3000, (2, 500), generator=g).cuda(),
             "signal_mask": torch.ones(3000, dtype=torch.bool).cuda(), "pid": torch.arange(3000).cuda() // 10}
    hp = dict(train_r=1.0, knn=100, true_edges="modulewise_true_edges")
    a = H.training_samples(emb, batch, hp)
    b = H.training_samples(emb, batch, dict(hp, knn_method="sorted"))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_graph_construction_k7_is_the_prefix_of_k8():
    from hierarchicalgnn_amd.graph_construction import DynamicGraphConstruction, find_neighbors
    g = torch.Generator().manual_seed(72)
    x = torch.nn.functional.normalize(torch.randn(700, 8, generator=g)).cuda()
    y = torch.nn.functional.normalize(torch.randn(300, 8, generator=g)).cuda()
    m = DynamicGraphConstruction("exp", {"knn_method": "sorted"}).cuda().eval()
    graph = m.build_graph(x, y, k=7)
    idx8 = find_neighbors(x, y, r_max=m.knn_radius, k_max=8)
    assert bool((idx8[:, 7] >= 0).any())                              # the cut at 7 drops something
    want = R.edges_from_knn(idx8[:, :7].cpu(), False, 700)
    assert torch.equal(graph.cpu(), want)
    with pytest.raises(RuntimeError, match="no instantiation"):       # the brute-force kernels still refuse K = 7
        DynamicGraphConstruction("exp", {}).cuda().eval().build_graph(x, y, k=7)
    i9 = find_neighbors(x, y, r_max=1.0, k_max=9, method="sorted")
    i10 = find_neighbors(x, y, r_max=1.0, k_max=10)
    assert torch.equal(i9, i10[:, :9])
