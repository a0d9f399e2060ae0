"""scatter_min / scatter_max with arg output and the integer sums (hgnn_segment_reduce_ex) against a plain CPU
restatement of torch_scatter 2.0.9's semantics: first-occurrence ties, out = 0 / arg = M for empty segments,
NaN never selected.  Min, max and arg involve no rounding, so every comparison is bitwise."""
import importlib
import sys

import numpy as np
import pytest
import torch

import conftest

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.int32, torch.int64]
WIDTHS = [1, 2, 3, 4, 8, 64, 256, 300]


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import _lib
    _lib.load()
    return H


def _np(t):
    """CPU numpy view of a tensor; bf16 widens to float32 exactly"""
    t = t.detach().cpu()
    return (t.float() if t.dtype == torch.bfloat16 else t).numpy()


def ref_minmax(vals, idx, N, op):
    """vals [M, F] numpy, idx int64 [M]: (out [N, F], arg [N, F]) by the stated rules"""
    M, F = vals.shape
    out = np.zeros((N, F), vals.dtype)
    arg = np.full((N, F), M, np.int64)
    e = np.arange(M)
    for f in range(F):
        v = vals[:, f]
        keep = ~np.isnan(v) if v.dtype.kind == "f" else np.ones(M, bool)
        vv, ee, dd = v[keep], e[keep], idx[keep]
        if len(vv) == 0:
            continue
        key = vv if op == "min" else (-vv if vv.dtype.kind == "f" else ~vv)   # ~ reverses integer order exactly
        order = np.lexsort((ee, key, dd))        # by segment, then value, then position
        ds = dd[order]
        first = np.ones(len(order), bool)
        first[1:] = ds[1:] != ds[:-1]
        sel = order[first]
        out[dd[sel], f] = vv[sel]
        arg[dd[sel], f] = ee[sel]
    return out, arg


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 2: np.int16}[a.dtype.itemsize])


def assert_same(out, arg, ref_out, ref_arg, what=""):
    o = _np(out)
    assert o.shape == ref_out.shape, what
    assert np.array_equal(_bits(o.astype(ref_out.dtype)), _bits(ref_out)), f"{what}: values differ"
    assert np.array_equal(arg.cpu().numpy(), ref_arg), f"{what}: arg differs"


def _src(dtype, M, F, g):
    x = torch.randint(0, 4, (M, F), generator=g)         # few distinct values: ties everywhere
    return x.to(dtype)


def _index(M, N, g, shuffled):
    # destinations drawn from every third id below N - 5: gaps, and dim_size > max + 1
    idx = torch.randint(0, (N - 5) // 3, (M,), generator=g) * 3
    return idx if shuffled else torch.sort(idx).values


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_minmax_matches_cpu_restatement(H, dtype, F, shuffled):
    g = torch.Generator().manual_seed(1000 + F)
    M, N = 3000, 400
    x = _src(dtype, M, F, g)
    idx = _index(M, N, g, shuffled)
    xd, idd = x.cuda(), idx.cuda()
    vals = _np(x)
    for op, fn in (("min", H.scatter_min), ("max", H.scatter_max)):
        out, arg = fn(xd, idd, dim=0, dim_size=N)
        assert out.dtype == dtype and arg.dtype == torch.int64 and out.shape == (N, F) and arg.shape == (N, F)
        ro, ra = ref_minmax(vals, idx.numpy(), N, op)
        assert_same(out, arg, ro, ra, f"{op} {dtype} F={F}")
        if dtype.is_floating_point:
            # cross-check the restatement's values on non-empty segments against torch on the CPU
            t = torch.zeros(N, F, dtype=torch.float32).scatter_reduce(
                0, idx.view(-1, 1).expand(M, F), x.float(), "amin" if op == "min" else "amax", include_self=False)
            nonempty = ra < M
            assert np.array_equal(t.numpy()[nonempty], ro.astype(np.float32)[nonempty])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("F", [1, 8, 256])
def test_split_destinations_do_not_depend_on_chunk(H, dtype, F):
    from hierarchicalgnn_amd.plan import GraphPlan
    g = torch.Generator().manual_seed(7)
    M, N, hub = 45_000, 600, 5
    idx = torch.randint(0, N, (M,), generator=g)
    idx[torch.rand(M, generator=g) < 0.8] = hub          # one destination with tens of thousands of rows
    x = _src(dtype, M, F, g)
    xd, idd = x.cuda(), idx.cuda()
    results = []
    for chunk in (7, 1000):
        plan = GraphPlan(idd, N, chunk=chunk)
        assert plan.counts_host()["split"] > 0, "the hub destination was not split"
        for fn in (H.scatter_min, H.scatter_max):
            results.append(fn(xd, idd, dim=0, dim_size=N, plan=plan))
    for a, b in zip(results[:2], results[2:]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "result depends on the plan's chunk"
    vals = _np(x)
    for (out, arg), op in zip(results[:2], ("min", "max")):
        assert_same(out, arg, *ref_minmax(vals, idx.numpy(), N, op), f"split {op}")
    if not dtype.is_floating_point:
        s = H.scatter_add(xd, idd, dim=0, dim_size=N, plan=GraphPlan(idd, N, chunk=7))
        ref = np.zeros((N, F), np.int64)
        np.add.at(ref, idx.numpy(), vals.astype(np.int64))
        assert s.dtype == dtype and np.array_equal(s.cpu().numpy().astype(np.int64), ref)


def test_extreme_values(H):
    i64 = torch.tensor([2**53 + 1, 2**53, -(2**62), 2**63 - 1, -(2**63), 2**53 + 1, 5, -7], dtype=torch.int64)
    i32 = torch.tensor([2**31 - 1, -(2**31), 0, -(2**31), 2**31 - 1, 3, -3, 1], dtype=torch.int32)
    inf, nan = float("inf"), float("nan")
    f32 = torch.tensor([inf, -inf, nan, 1.0, -inf, nan, nan, inf], dtype=torch.float32)
    idx = torch.tensor([0, 0, 0, 1, 1, 2, 2, 3])
    for x in (i64, i32, f32, f32.bfloat16()):
        for F in (1, 4):
            xs = x.view(-1, 1).repeat(1, F)
            for op, fn in (("min", H.scatter_min), ("max", H.scatter_max)):
                for perm in (torch.arange(8), torch.tensor([7, 3, 5, 0, 6, 2, 4, 1])):
                    out, arg = fn(xs[perm].cuda(), idx[perm].cuda(), dim=0, dim_size=5)
                    assert_same(out, arg, *ref_minmax(_np(xs[perm]), idx[perm].numpy(), 5, op), f"{op} {x.dtype}")
    # named outcomes: NaN never wins, a NaN-only segment is empty, +-inf are ordinary values
    out, arg = H.scatter_min(f32.cuda(), idx.cuda(), dim=0, dim_size=5)
    assert out.tolist()[:2] == [-inf, -inf] and arg.tolist() == [1, 4, 8, 7, 8]
    assert out[2].item() == 0.0 and out[4].item() == 0.0
    out, arg = H.scatter_max(i64.cuda(), idx.cuda(), dim=0, dim_size=5)
    assert out.tolist()[:2] == [2**53 + 1, 2**63 - 1] and arg.tolist()[:2] == [0, 3]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("F", [1, 3, 64])
def test_gradient_goes_to_arg(H, dtype, F):
    g = torch.Generator().manual_seed(3)
    M, N = 2000, 300
    x = _src(dtype, M, F, g)
    idx = _index(M, N, g, True)
    w = torch.randn(N, F, generator=g).to(dtype)
    for op, fn in (("min", H.scatter_min), ("max", H.scatter_max)):
        xd = x.cuda().requires_grad_(True)
        out, arg = fn(xd, idx.cuda(), dim=0, dim_size=N)
        assert not arg.requires_grad
        (out * w.cuda()).sum().backward()
        _, ra = ref_minmax(_np(x), idx.numpy(), N, op)
        expect = torch.zeros(M, F, dtype=dtype)
        d, f = np.nonzero(ra < M)
        expect[torch.from_numpy(ra[d, f]), torch.from_numpy(f)] = w[torch.from_numpy(d), torch.from_numpy(f)]
        assert xd.grad.dtype == dtype and torch.equal(xd.grad.cpu(), expect), op


def test_dim_argument(H):
    g = torch.Generator().manual_seed(11)
    M, N = 500, 70
    idx = torch.randint(0, N - 3, (M,), generator=g)
    cases = [
        (torch.randint(0, 4, (6, M), generator=g).float(), -1),
        (torch.randint(0, 4, (6, M), generator=g).float(), 1),
        (torch.randint(0, 4, (M, 6), generator=g).float(), 0),
        (torch.randint(0, 4, (3, M, 5), generator=g).int(), 1),
        (torch.randint(0, 4, (3, M, 5), generator=g).long(), -2),
        (torch.randint(0, 4, (M, 3, 5), generator=g).float(), 0),
    ]
    for x, dim in cases:
        d = dim % x.dim()
        for op, fn in (("min", H.scatter_min), ("max", H.scatter_max)):
            out, arg = fn(x.cuda(), idx.cuda(), dim, dim_size=N) if dim != -1 else fn(x.cuda(), idx.cuda(),
                                                                                        dim_size=N)
            moved = x.movedim(d, 0)
            ro, ra = ref_minmax(moved.reshape(M, -1).numpy(), idx.numpy(), N, op)
            shape = (N,) + tuple(moved.shape[1:])
            ro = np.moveaxis(ro.reshape(shape), 0, d)
            ra = np.moveaxis(ra.reshape(shape), 0, d)
            assert out.shape == ro.shape and out.is_contiguous()
            assert_same(out, arg, ro, ra, f"{op} dim={dim} shape={tuple(x.shape)}")


def test_dim_size_as_tensor_and_repeat_runs(H):
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 4, (5000, 64), generator=g).float().cuda()
    idx = torch.randint(0, 900, (5000,), generator=g).cuda()
    first = H.scatter_max(x, idx, dim=0, dim_size=idx.max() + 1)
    assert first[0].shape[0] == int(idx.max()) + 1
    for _ in range(3):
        again = H.scatter_max(x, idx, dim=0, dim_size=idx.max() + 1)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_out_argument_raises(H):
    x, idx = torch.randn(10).cuda(), torch.zeros(10, dtype=torch.long).cuda()
    with pytest.raises(RuntimeError, match="out="):
        H.scatter_min(x, idx, out=torch.empty(1).cuda())
    with pytest.raises(RuntimeError, match="float64"):
        H.scatter_max(x.double(), idx)


@pytest.fixture()
def shim():
    sys.path.insert(0, conftest.ROOT + "/torch_scatter_shim")
    try:
        yield importlib.import_module("torch_scatter")
    finally:
        sys.path.pop(0)
        sys.modules.pop("torch_scatter", None)


def test_reference_call_shapes_through_the_shim(H, shim):
    """bipartite_classification_base.py:158 / tracking_utils.py:37,41"""
    g = torch.Generator().manual_seed(21)
    n_hits = 120_000
    pid_raw = torch.randint(0, 10_000, (n_hits,), generator=g) * 7919 + 100_003   # sparse particle ids
    pt = (torch.randint(1, 50, (n_hits,), generator=g).float() * 0.25)             # ties within particles
    primary = (torch.rand(n_hits, generator=g) < 0.3).long()
    pid_raw, pt, primary = pid_raw.cuda(), pt.cuda(), primary.cuda()
    original_pid, pid, nhits = torch.unique(pid_raw, return_inverse=True, return_counts=True)
    pt_min = shim.scatter_min(pt, pid, dim=0, dim_size=pid.max() + 1)[0]
    n = int(pid.max()) + 1
    ro, _ = ref_minmax(pt.cpu().numpy().reshape(-1, 1), pid.cpu().numpy(), n, "min")
    assert pt_min.shape == (n,) and np.array_equal(_bits(pt_min.cpu().numpy()), _bits(ro[:, 0]))
    s = shim.scatter_sum(primary, pid)
    assert s.dtype == torch.int64
    assert np.array_equal(s.cpu().numpy(), np.bincount(pid.cpu().numpy(), weights=primary.cpu().numpy(),
                                                       minlength=n).astype(np.int64))
    assert torch.equal(shim.scatter(pt, pid, reduce="min"), pt_min)
    assert torch.equal(shim.scatter(primary, pid, dim=0, reduce="sum"), s)


def test_integer_scatter_mean_floors(H, shim):
    idx = torch.tensor([0, 0, 1, 1, 1, 3, 3])
    for dtype in (torch.int32, torch.int64):
        x = torch.tensor([-3, 0, 7, 1, 1, 5, -6], dtype=dtype)
        m = shim.scatter_mean(x.cuda(), idx.cuda(), dim=0, dim_size=5)
        assert m.dtype == dtype and m.cpu().tolist() == [-2, 3, 0, -1, 0]   # floor(-1.5), floor(3), empty, floor(-0.5)
        x2 = x.view(-1, 1).repeat(1, 8)
        m2 = shim.scatter_mean(x2.cuda(), idx.cuda(), dim=0, dim_size=5)
        assert m2.cpu().tolist() == [[v] * 8 for v in [-2, 3, 0, -1, 0]]
