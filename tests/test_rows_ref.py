"""CPU checks of tests/rows_ref.py: the proof that a red test in test_gpu_rows_exact.py is the kernel's fault.
The generator yields the requested lengths, the exactness bound holds, fp32 summation on the grid does not depend
on the order, the int64 reference agrees with the oracle, the bf16 reference is one round-to-nearest-even."""
import pytest
import torch

import rows_ref as R

CHUNKS = (1, 5, 32, 64, 100)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("ends", R.ENDS)
def test_generator_yields_the_requested_lengths(chunk, ends):
    lengths = R.standard_lengths(chunk, ends, seed=chunk)
    shuf, srt = R.index_with_lengths(lengths, seed=3)
    N = len(lengths)
    want = torch.tensor(lengths)
    assert torch.equal(torch.bincount(shuf, minlength=N), want)
    assert torch.equal(torch.bincount(srt, minlength=N), want)
    assert torch.equal(srt, torch.sort(shuf).values) and bool((srt[1:] >= srt[:-1]).all())
    assert not torch.equal(shuf, srt)
    # every length the kernels have a loop edge at is present; first and last destination as asked
    c = chunk
    for n in R.BASE_LENGTHS + (c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 3 * c + 1, 64 * c + 1):
        assert n in lengths, n
    end = {"empty": 0, "one": 1, "split": 2 * c + 1}[ends]
    assert lengths[0] == end and lengths[-1] == end
    runs = "".join("0" if n == 0 else "x" for n in lengths)
    assert "000" in runs
    # the exactness bound (max list length x max |term| in units < 2^24)
    assert max(lengths) < R.MAX_LIST == 32768
    R.assert_exact(max(lengths))
    assert R.MAX_TERM_UNITS == 512


def test_exactness_bound_refuses_long_lists():
    R.assert_exact(32767)
    with pytest.raises(AssertionError):
        R.assert_exact(32768)
    with pytest.raises(AssertionError):
        R.standard_lengths(512, "one")          # 64 * 512 + 1 rows


def test_value_grids():
    x = R.features(500, 24, seed=1)
    assert set(x.unique().tolist()) == {float(v) for v in range(-8, 9) if v != 0}
    assert torch.equal(x.bfloat16().float(), x)                      # exact in bf16
    assert set(R.weights(4000, 2).unique().tolist()) == set(R.WEIGHTS)
    assert set(R.row_scales(4000, 3).unique().tolist()) == set(R.ROW_SCALES)
    assert torch.equal(R.features(7, 5, 9), R.features(7, 5, 9))      # seeded


@pytest.mark.parametrize("chunk", CHUNKS)
def test_plan_reference_tiles_every_list_once(chunk):
    lengths = R.standard_lengths(chunk, "split", seed=11)
    p = R.plan_reference(lengths, chunk)
    deg = torch.tensor(lengths)
    nch = torch.where(deg > chunk, (deg + chunk - 1) // chunk, torch.ones_like(deg))
    assert p["work"] == int(nch.sum()) and p["split"] == int((deg > chunk).sum())
    assert p["partial"] == int(nch[deg > chunk].sum()) and p["valid"] == int(deg.sum())
    # the bounds hgnn_plan_dims allocates for
    M, N = int(deg.sum()), len(lengths)
    assert p["work"] <= N + M // chunk + 1 and p["split"] <= M // (chunk + 1) + 1
    assert p["partial"] <= 2 * (M // chunk) + 2
    pos = 0
    for b, e, d in zip(p["wi_begin"], p["wi_end"], p["wi_dst"]):
        assert b == pos and b <= e <= b + chunk and p["rowptr"][d] <= b and e <= p["rowptr"][d + 1]
        assert e > b or lengths[d] == 0
        pos = e
    assert pos == M
    assert max(n for n in nch.tolist()) > 64                           # a combine list with a second 64-row trip


def test_fp32_summation_on_the_grid_is_order_independent():
    """fp32 index_add_ in several random orders equals the int64 sum bitwise, lists up to 17k rows"""
    lengths = [0, 1, 17000, 3, 0, 64, 9000, 4097]
    shuf, srt = R.index_with_lengths(lengths, seed=5)
    M, N, F = shuf.numel(), len(lengths), 12
    src, w, rs = R.features(M, F, 6), R.weights(M, 7), R.row_scales(M, 8)
    ref = R.scatter_ref(src, shuf, N, weight=w, row_scale=rs)
    ref16 = R.scatter_ref(src.bfloat16(), shuf, N, weight=w, row_scale=rs)
    assert ref16.dtype == torch.bfloat16
    terms = (w * rs).view(-1, 1) * src
    for seed in (0, 1, 2):
        p = torch.randperm(M, generator=torch.Generator().manual_seed(seed))
        out = torch.zeros(N, F).index_add_(0, shuf[p], terms[p])
        assert torch.equal(out, ref)
        assert torch.equal(out.bfloat16(), ref16)                      # rounding the exact sum once
    # a plain running sum in fp32, forwards and backwards
    one = terms[shuf == 2]
    assert torch.equal(one.cumsum(0)[-1], ref[2]) and torch.equal(one.flip(0).cumsum(0)[-1], ref[2])


@pytest.mark.parametrize("F", [1, 6, 64])
def test_reference_agrees_with_the_oracle(F):
    from oracle import hgnn_oracle as O
    lengths = R.standard_lengths(5, "one", seed=F)
    shuf, srt = R.index_with_lengths(lengths, seed=F + 1)
    M, N = shuf.numel(), len(lengths)
    src, w = R.features(M, F, 2), R.weights(M, 3)
    assert torch.equal(R.scatter_ref(src, shuf, N), O.scatter_add(src, shuf, 0, N))
    assert torch.equal(R.scatter_ref(src, shuf, N, weight=w), O.scatter_add(w.view(-1, 1) * src, shuf, 0, N))
    Rn = 77
    X, rs = R.features(Rn, F, 4), R.row_scales(Rn, 5)
    gi = torch.randint(0, Rn, (M,), generator=torch.Generator().manual_seed(6))
    ref = O.scatter_add(w.view(-1, 1) * (rs.view(-1, 1) * X)[gi], srt, 0, N)
    assert torch.equal(R.scatter_ref(X, srt, N, weight=w, gather=gi, row_scale=rs), ref)
    # gather (negative index -> zero row), spread, edge dot
    idx = gi.clone()
    idx[::7] = -1
    g = R.gather_ref(X, idx, weight=w, row_scale=rs)
    want = (w.view(-1, 1) * (rs.view(-1, 1) * X)[idx.clamp_min(0)]) * (idx >= 0).view(-1, 1)
    assert torch.equal(g, want) and float(g[::7].abs().sum()) == 0.0
    assert torch.equal(R.spread_ref(X, gi, w), w.view(-1, 1) * X[gi])
    dot = R.edge_dot_ref(src, None, X, idx)
    assert torch.equal(dot, ((src.double() * X.double()[idx.clamp_min(0)]).sum(1) * (idx >= 0)).float())


def test_bf16_reference_is_one_round_to_nearest_even():
    # bf16 keeps 8 significant bits: spacing 2 in [256, 512), 8 in [1024, 2048).  257 lies halfway between 256 and
    # 258, 259 halfway between 258 and 260: ties go to the even mantissa (256, 260), whatever the sign
    x = torch.tensor([257.0, 259.0, 261.0, 263.0, -257.0, -259.0, 258.0, 0.125, 1027.0, 1028.0, 1036.0, 1029.0, 3.0e38])
    want = torch.tensor([256.0, 260.0, 260.0, 264.0, -256.0, -260.0, 258.0, 0.125, 1024.0, 1024.0, 1040.0, 1032.0,
                         3.0e38]).bfloat16()
    assert torch.equal(x.bfloat16(), want)
    assert torch.equal(R.bf16_bits_rne(x), x.bfloat16().view(torch.int16))
    # on sums of the grid: integer sums hit exact ties all the time
    lengths = R.standard_lengths(32, "split", seed=2)
    shuf, _ = R.index_with_lengths(lengths, seed=4)
    src = R.features(shuf.numel(), 16, 3, dtype=torch.bfloat16)
    w = R.weights(shuf.numel(), 5)
    exact = R.scatter_ref(src.float(), shuf, len(lengths), weight=w)
    ref16 = R.scatter_ref(src, shuf, len(lengths), weight=w)
    assert torch.equal(R.bf16_bits_rne(exact), ref16.view(torch.int16))
    low = exact.view(torch.int32) & 0xFFFF
    assert int((low == 0x8000).sum()) > 0, "the data never hits a rounding tie"
    assert int((ref16.float() != exact).sum()) > 0


def test_default_chunk_formula():
    assert R.default_chunk(0) == 32 and R.default_chunk(5000) == 32 and R.default_chunk(2_000_000) == 122
    assert R.default_chunk(600_000) == 36 and R.default_chunk(10 ** 8) == 512
