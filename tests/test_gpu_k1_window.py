"""Bitwise gate of the K1 rolling-window kernel (k_seg_window in csrc/segreduce.hip) on randn data.

The kernel adds the rows of a list one by one, in list order, with plain fp32 adds, starting from 0; a
destination with more than ``plan.chunk`` rows is cut into ``nch = ceil(deg / chunk)`` chunks of
``len = ceil(deg / nch)`` rows whose partial sums are then added in chunk order, again starting from 0.
``order_exact_sum`` states exactly that without the kernel under test: rows are sorted stably by destination and,
for k = 0, 1, .., the k-th row of every list that has one is added with one indexed fp32 add, so every list is
summed strictly in order.  ``test_reference_against_python_loop`` proves it on the CPU against a plain float32
loop.  On randn data any other summation order changes low bits, so ``torch.equal`` pins the order.

Every GPU case runs at nt_loads 0 and 1, through the C ABI into a NaN-poisoned buffer with guards and a
NaN-filled partial buffer (helpers of test_gpu_rows_exact.py), and once more through ``scatter_add``.
"""
import numpy as np
import pytest
import torch

W = 16  # window depth of the shipped kernel (launch_seg_headline in segreduce.hip)
LENGTHS = (0, 1, W - 1, W, W + 1, 63, 64, 65, 128, 129)


def order_exact_sum(src, index, N, chunk):
    """out[d] = the rows of d in stable order, summed as the plan prescribes; works on any device"""
    dev = src.device
    F = src.shape[1]
    perm = torch.sort(index, stable=True).indices
    deg = torch.bincount(index, minlength=N)
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(deg, 0)
    nch = torch.clamp((deg + chunk - 1) // chunk, min=1)            # lists per destination (1 if not split)
    ln = (deg + nch - 1) // nch                                      # rows per chunk, the last one may be shorter
    first = torch.zeros(N + 1, dtype=torch.int64, device=dev)        # first list of each destination
    first[1:] = torch.cumsum(nch, 0)
    n_lists = int(first[-1])
    owner = torch.repeat_interleave(torch.arange(N, device=dev), nch)
    c = torch.arange(n_lists, device=dev) - first[owner]             # chunk number inside the destination
    lbegin = rowptr[owner] + c * ln[owner]
    lend = torch.minimum(lbegin + ln[owner], rowptr[owner + 1])
    llen = lend - lbegin
    part = torch.zeros(n_lists, F, dtype=torch.float32, device=dev)
    for k in range(int(llen.max()) if n_lists else 0):
        sel = torch.nonzero(llen > k).squeeze(1)
        part[sel] = part[sel] + src[perm[lbegin[sel] + k]]
    out = torch.zeros(N, F, dtype=torch.float32, device=dev)
    single = torch.nonzero(nch == 1).squeeze(1)
    out[single] = part[first[single]]
    for k in range(int(nch.max()) if N else 0):
        sel = torch.nonzero((nch > 1) & (nch > k)).squeeze(1)
        out[sel] = out[sel] + part[first[sel] + k]
    return out


def test_reference_against_python_loop():
    g = torch.Generator().manual_seed(3)
    N, F, chunk = 9, 3, 4
    degs = [0, 1, 3, 4, 5, 8, 9, 13, 0]
    index = torch.repeat_interleave(torch.arange(N), torch.tensor(degs))
    index = index[torch.randperm(index.numel(), generator=g)]
    src = torch.randn(index.numel(), F, generator=g)
    want = np.zeros((N, F), dtype=np.float32)
    s, idx = src.numpy(), index.numpy()
    for d in range(N):
        rows = [i for i in range(len(idx)) if idx[i] == d]          # list order = original order (stable sort)
        n_ch = max(1, -(-len(rows) // chunk))
        ln = -(-len(rows) // n_ch)
        parts = []
        for c in range(n_ch):
            acc = np.zeros(F, dtype=np.float32)
            for i in rows[c * ln:(c + 1) * ln]:
                acc = np.float32(acc + s[i])
            parts.append(acc)
        if n_ch == 1:
            want[d] = parts[0]
        else:
            acc = np.zeros(F, dtype=np.float32)
            for p in parts:
                acc = np.float32(acc + p)
            want[d] = acc
    got = order_exact_sum(src, index, N, chunk).numpy()
    assert got.tobytes() == want.tobytes()
    # and the order matters on this data: a reversed list order gives other bits somewhere
    rev = order_exact_sum(src.flip(0), index.flip(0), N, chunk).numpy()
    assert rev.tobytes() != want.tobytes()


def _check(index, N, F, chunk, nt, seed=0):
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd.plan import GraphPlan
    import test_gpu_rows_exact as X
    torch.manual_seed(seed)
    src = torch.randn(index.numel(), F, device="cuda")
    plan = GraphPlan(index, N, chunk=chunk)
    ref = order_exact_sum(src, index, N, plan.chunk)
    with X.nt_loads(nt):
        out = X.seg_reduce(plan, src)
        bad = (out != ref).any(1).nonzero().squeeze(1)
        assert bad.numel() == 0, f"{bad.numel()} rows differ, first destination {int(bad[0])}"
        assert torch.equal(H.scatter_add(src, index, dim_size=N, plan=plan), ref)
    H.clear_plan_cache()
    return plan


@pytest.mark.gpu
@pytest.mark.parametrize("nt", (1, 0))
@pytest.mark.parametrize("layout", ("shuffled", "sorted"))
def test_headline_event(layout, nt):
    from hierarchicalgnn_amd import synth
    x, ei = synth.trackml_event()
    index = synth.directed(ei)[1].contiguous().cuda()
    assert index.numel() == 2_000_000
    if layout == "sorted":
        index = torch.sort(index).values
    plan = _check(index, 120_000, 256, 0, nt)
    assert plan.sorted == (layout == "sorted")


@pytest.mark.gpu
@pytest.mark.parametrize("nt", (1, 0))
@pytest.mark.parametrize("chunk", (1, 5, 64))
def test_forced_chunks(chunk, nt):
    from hierarchicalgnn_amd import synth
    x, ei = synth.trackml_event(3000, 20000, seed=1)
    index = synth.directed(ei)[1].contiguous().cuda()
    _check(index, 3000, 256, chunk, nt)


@pytest.mark.gpu
@pytest.mark.parametrize("nt", (1, 0))
@pytest.mark.parametrize("F", (256, 252, 132))
@pytest.mark.parametrize("chunk", (0, 256))
@pytest.mark.parametrize("layout", ("shuffled", "sorted"))
def test_list_lengths(layout, chunk, F, nt):
    """every length at both ends of the destination range and in the middle; chunk 256 keeps the 65..129-row
    lists whole (a second and third 64-row trip of one window), the default chunk splits them"""
    degs = torch.tensor(LENGTHS + LENGTHS[::-1] + (3, 0, 0, 17, 31, 32, 33, 47, 48, 49) + LENGTHS)
    N = degs.numel()
    index = torch.repeat_interleave(torch.arange(N), degs)
    if layout == "shuffled":
        index = index[torch.randperm(index.numel(), generator=torch.Generator().manual_seed(5))]
    _check(index.cuda(), N, F, chunk, nt, seed=F)
