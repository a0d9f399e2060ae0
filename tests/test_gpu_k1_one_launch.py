"""Bitwise gate of hgnn_segment_reduce_f32_ex (csrc/segreduce.hip): one launch per call, work items longest-first.

In the one-launch form the chunk of a split destination that arrives last sums the partial rows of that destination
in chunk order, starting from 0, and no combine launch follows; ``arrive`` (one int32 per split destination) is zero
before and after every call.  ``hgnn_plan_item_order`` hands the work items out by non-increasing list length in
buckets of 8 rows.  Neither may change one bit of the result: every comparison is ``torch.equal`` against
``order_exact_sum`` of test_gpu_k1_window.py on randn data, through the C ABI (guarded output buffer, NaN-filled
partial buffer) with both entry points and both values of each option, and through ``scatter_add``.

``order_exact_sum`` states the order of the kernels that read one row per wave instruction (F > 128: k_seg_window
and the wide k_seg_reduce).  At F = 64 a wave instruction of k_seg_reduce reads G = 4 rows: lane group g adds the
elements g, g + G, .. of a list in list order, starting from 0, and the groups are then added pairwise
((S0 + S1) + (S2 + S3)); the combine pass does the same with the partial rows.  That order is as fixed as the other,
and it is what the library computed before the one-launch form existed.  ``grouped_exact_sum`` states it without the
kernel under test; with G = 1 it is ``order_exact_sum`` (``test_grouped_reference_on_the_cpu``).
"""
import contextlib
import ctypes
import functools

import pytest
import torch

from test_gpu_k1_window import LENGTHS, order_exact_sum

DEFAULT_CHUNK = 32  # what hgnn_plan_dims picks for the few thousand rows of these cases
DEGS = LENGTHS + LENGTHS[::-1] + (3, 0, 0, 17, 31, 32, 33, 47, 48, 49) + LENGTHS  # test_gpu_k1_window.test_list_lengths


def _grouped(rows_of, begin, length, G, F, dev):
    """sum of the elements begin[i] .. begin[i] + length[i] - 1 (fetched by rows_of(positions)) of every list i:
    group g adds elements g, g + G, .. in order from 0, then S[g] += S[g ^ h] for h = 1, 2, .. G / 2"""
    n = begin.numel()
    acc = torch.zeros(n, G, F, dtype=torch.float32, device=dev)
    for k in range(-(-int(length.max()) // G) if n else 0):
        for g in range(G):
            sel = torch.nonzero(length > k * G + g).squeeze(1)
            acc[sel, g] = acc[sel, g] + rows_of(begin[sel] + k * G + g)
    h = 1
    while h < G:
        acc[:, 0::2 * h] = acc[:, 0::2 * h] + acc[:, h::2 * h]
        h *= 2
    return acc[:, 0]


def grouped_exact_sum(src, index, N, chunk, G):
    """order_exact_sum for kernels that read G rows per wave instruction (module docstring); any device"""
    dev, F = src.device, src.shape[1]
    perm = torch.sort(index, stable=True).indices
    deg = torch.bincount(index, minlength=N)
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(deg, 0)
    nch = torch.clamp((deg + chunk - 1) // chunk, min=1)
    ln = (deg + nch - 1) // nch
    first = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    first[1:] = torch.cumsum(nch, 0)
    owner = torch.repeat_interleave(torch.arange(N, device=dev), nch)
    c = torch.arange(int(first[-1]), device=dev) - first[owner]
    lbegin = rowptr[owner] + c * ln[owner]
    llen = torch.minimum(lbegin + ln[owner], rowptr[owner + 1]) - lbegin
    part = _grouped(lambda p: src[perm[p]], lbegin, llen, G, F, dev)
    out = torch.zeros(N, F, dtype=torch.float32, device=dev)
    single = torch.nonzero(nch == 1).squeeze(1)
    out[single] = part[first[single]]
    split = torch.nonzero(nch > 1).squeeze(1)
    out[split] = _grouped(lambda p: part[p], first[split], nch[split], G, F, dev)
    return out


def rows_per_instruction(F):
    """G of the kernel that serves width F (for_row_shape in csrc/rows_common.h): 64 / RL lanes per row"""
    ncol = F // 4
    return 64 // next(rl for rl in (4, 8, 16, 32, 64) if ncol <= rl or rl == 64)


def exact_sum(src, index, N, chunk):
    G = rows_per_instruction(src.shape[1])
    return order_exact_sum(src, index, N, chunk) if G == 1 else grouped_exact_sum(src, index, N, chunk, G)


def test_grouped_reference_on_the_cpu():
    import numpy as np
    g = torch.Generator().manual_seed(4)
    N, F, chunk = 8, 3, 5
    degs = [0, 1, 4, 5, 6, 11, 23, 37]  # up to 8 partial rows
    index = torch.repeat_interleave(torch.arange(N), torch.tensor(degs))
    index = index[torch.randperm(index.numel(), generator=g)]
    src = torch.randn(index.numel(), F, generator=g)
    assert torch.equal(grouped_exact_sum(src, index, N, chunk, 1), order_exact_sum(src, index, N, chunk))

    def grouped(rows):  # plain float32 loop: four running sums, then (S0 + S1) + (S2 + S3)
        S = [np.zeros(F, dtype=np.float32) for _ in range(4)]
        for i, r in enumerate(rows):
            S[i % 4] = np.float32(S[i % 4] + r)
        return np.float32(np.float32(S[0] + S[1]) + np.float32(S[2] + S[3]))

    s, idx = src.numpy(), index.numpy()
    want = np.zeros((N, F), dtype=np.float32)
    for d in range(N):
        rows = [s[i] for i in range(len(idx)) if idx[i] == d]
        n_ch = max(1, -(-len(rows) // chunk))
        ln = -(-len(rows) // n_ch)
        parts = [grouped(rows[k * ln:(k + 1) * ln]) for k in range(n_ch)]
        want[d] = parts[0] if n_ch == 1 else grouped(parts)
    got = grouped_exact_sum(src, index, N, chunk, 4).numpy()
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() != order_exact_sum(src, index, N, chunk).numpy().tobytes()  # the order matters here
    assert [rows_per_instruction(F) for F in (64, 132, 252, 256, 512)] == [4, 1, 1, 1, 1]


@contextlib.contextmanager
def option(name, value):
    from hierarchicalgnn_amd import _lib as L
    was = L.get_option(name)
    try:
        L.check(L.load().hgnn_set_option(name.encode(), int(value)), "hgnn_set_option")
        yield
    finally:
        L.check(L.load().hgnn_set_option(name.encode(), was), "hgnn_set_option")


def seg_reduce_ex(plan, src, order=None):
    """hgnn_segment_reduce_f32_ex into a guarded buffer, with a NaN-filled partial buffer; arrive must stay zero"""
    from hierarchicalgnn_amd import _lib as L
    import test_gpu_rows_exact as X
    F = int(src.shape[1])
    g = X.Guarded(plan.N, F, src.dtype)
    partial = plan.partial(F)
    partial.fill_(float("nan"))
    assert not bool(plan.arrive.any()), "arrive is not zero before the call"
    L.check(L.load().hgnn_segment_reduce_f32_ex(
        ctypes.byref(plan.c), L.ptr(src), F, None, None, g.ptr(), L.ptr(partial), L.ptr(plan.arrive), L.ptr(order),
        L.current_stream(src.device)), "hgnn_segment_reduce_f32_ex")
    g.all_written("segment_reduce_f32_ex")
    out = g.check("segment_reduce_f32_ex")
    assert not bool(plan.arrive.any()), "arrive is not zero after the call"
    return out


def same(out, ref, what):
    bad = (out != ref).any(1).nonzero().squeeze(1)
    assert bad.numel() == 0, f"{what}: {bad.numel()} rows differ, first destination {int(bad[0])}"


def all_forms(plan, src, index, ref, what):
    """both entry points, both values of both options, C ABI and scatter_add"""
    import hierarchicalgnn_amd as H
    import test_gpu_rows_exact as X
    same(X.seg_reduce(plan, src), ref, f"{what} two-launch entry")
    order = plan.item_order()
    for one in (1, 0):
        for ordered in (1, 0):
            with option("k1_one_launch", one), option("k1_item_order", ordered):
                tag = f"{what} one_launch={one} item_order={ordered}"
                same(seg_reduce_ex(plan, src, order), ref, tag + " (C ABI)")
                same(seg_reduce_ex(plan, src, None), ref, tag + " (C ABI, order NULL)")
                same(H.scatter_add(src, index, dim_size=plan.N, plan=plan), ref, tag + " (scatter_add)")
                assert not bool(plan.arrive.any()), tag + ": arrive is not zero after scatter_add"


@functools.lru_cache(maxsize=None)
def length_case(layout, chunk, F):
    """index, src and the order-exact reference of one (layout, chunk, F); shared by everything that needs it"""
    c = chunk if chunk > 0 else DEFAULT_CHUNK
    degs = torch.tensor(DEGS + (64 * c + 1,))  # more than 64 partial rows for one destination
    N = degs.numel()
    index = torch.repeat_interleave(torch.arange(N), degs)
    if layout == "shuffled":
        index = index[torch.randperm(index.numel(), generator=torch.Generator().manual_seed(5))]
    index = index.cuda()
    torch.manual_seed(F)
    src = torch.randn(index.numel(), F, device="cuda")
    return index, N, src, exact_sum(src, index, N, c)


@pytest.mark.gpu
@pytest.mark.parametrize("F", (256, 252, 132, 64, 512))  # k_seg_window: 256, 252, 132; k_seg_reduce: 64, 512
@pytest.mark.parametrize("chunk", (1, 5, 64, 0))
@pytest.mark.parametrize("layout", ("shuffled", "sorted"))
def test_one_launch_against_order_exact_reference(layout, chunk, F):
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd.plan import GraphPlan
    import test_gpu_rows_exact as X
    index, N, src, ref = length_case(layout, chunk, F)
    plan = GraphPlan(index, N, chunk=chunk)
    assert plan.chunk == (chunk if chunk > 0 else DEFAULT_CHUNK)
    assert plan.sorted == (layout == "sorted")
    assert plan.counts_host()["partial"] > 64
    for nt in (1, 0):
        with X.nt_loads(nt):
            all_forms(plan, src, index, ref, f"{layout} chunk={chunk} F={F} nt={nt}")
    H.clear_plan_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("nt", (1, 0))
def test_many_splits_spread_over_the_chip(nt):
    """2048 destinations of 8 chunks each: about 16k items in about 2k workgroups, so the chunks of one destination
    run on different XCDs; three calls in a row on one plan, each on other data, the partial buffer NaN-filled and
    arrive checked in between (seg_reduce_ex)"""
    from hierarchicalgnn_amd.plan import GraphPlan
    import test_gpu_rows_exact as X
    N, deg, chunk, F = 2048, 40, 5, 256
    index = torch.repeat_interleave(torch.arange(N), deg)
    index = index[torch.randperm(index.numel(), generator=torch.Generator().manual_seed(11))].cuda()
    plan = GraphPlan(index, N, chunk=chunk)
    c = plan.counts_host()
    assert (c["work"], c["split"], c["partial"]) == (8 * N, N, 8 * N)
    torch.manual_seed(nt)
    src = torch.randn(index.numel(), F, device="cuda")
    with X.nt_loads(nt), option("k1_one_launch", 1):
        for call in range(3):
            ref = order_exact_sum(src, index, N, chunk)
            order = plan.item_order() if call == 1 else None
            same(seg_reduce_ex(plan, src, order), ref, f"call {call}")
            src = src.roll(1, 0) * 1.5


def check_order(plan):
    c = plan.counts_host()["work"]
    order = plan.item_order().cpu().long()
    assert order.numel() == int(plan.c.max_work)
    assert torch.equal(torch.sort(order[:c]).values, torch.arange(c)), "order[:work] is not a permutation"
    assert bool((order[c:] >= c).all()), "an entry past the count names a work item"
    length = (plan.wi_end[:c] - plan.wi_begin[:c]).cpu().long()
    bucket = length[order[:c]] >> 3
    assert bool((bucket[1:] <= bucket[:-1]).all()), "bucketed lengths increase somewhere"
    # stable inside a bucket: plan order is kept
    keep = bucket[1:] == bucket[:-1]
    assert bool((order[:c][1:][keep] > order[:c][:-1][keep]).all()), "plan order is not kept inside a bucket"


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", (5, 0))
def test_item_order_of_the_length_set(chunk):
    from hierarchicalgnn_amd.plan import GraphPlan
    index, N, src, ref = length_case("shuffled", chunk, 256)
    check_order(GraphPlan(index, N, chunk=chunk))


@pytest.mark.gpu
def test_item_order_of_an_event():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import synth
    from hierarchicalgnn_amd.plan import GraphPlan
    x, ei = synth.trackml_event(3000, 20000, seed=1)
    index = synth.directed(ei)[1].contiguous().cuda()
    plan = GraphPlan(index, 3000, chunk=0)
    check_order(plan)
    torch.manual_seed(2)
    src = torch.randn(index.numel(), 256, device="cuda")
    ref = order_exact_sum(src, index, 3000, plan.chunk)
    for ordered in (0, 1):
        with option("k1_item_order", ordered):
            same(seg_reduce_ex(plan, src, plan.item_order()), ref, f"item_order={ordered} (C ABI)")
            same(H.scatter_add(src, index, dim_size=3000, plan=plan), ref, f"item_order={ordered} (scatter_add)")
    H.clear_plan_cache()
