"""CPU checks of tests/gemm_ref.py: the proof that a red test in test_gpu_gemm_exact.py is the kernel's fault.
The grids are what they claim, fp32 / float64 products of grid data do not depend on the reduction order and equal
the int64 result, the restated wg::shape_for agrees with hand-computed cases of the C++ formula, and every MUTANT of
the reference's own arithmetic (a dropped or duplicated row, a skipped last slice or last 32-row step, swapped
columns, a dropped mid.mid / mid.hi product, truncation, the skip row added after the rounding, column sums of the
wrong tile) changes at least one element of every case the GPU file runs -- the condition that keeps a case from
being vacuous."""
import pytest
import torch

import gemm_ref as G


# ------------------------------------------------------------------ grids
def test_value_grids():
    s = G.small(300, 24, seed=1)
    assert set(s.unique().tolist()) == {float(v) for v in range(-8, 9) if v != 0}
    assert torch.equal(s.bfloat16().float(), s)                              # exact in bf16
    for bits in (9, 10):
        m = G.mid(200, 40, seed=2, bits=bits)
        hi, md = G.split(m)
        assert bool((m != 0).all()) and torch.equal(hi + md, m.double())
        assert bool((md != 0).all()) and bool((md.abs() == 1).all())         # bf16(x) != x everywhere
        assert float(m.abs().max()) < 2 ** bits and float(m.abs().min()) >= 257 and float(hi.abs().max()) <= 2 ** bits
    assert G.mid(2000, 8, seed=3).abs().max() > 512                          # 10 significant bits do occur
    d = G.both_dense(64, 40, seed=4)
    assert set(d.unique().tolist()) == {-257.0, 257.0}
    for dim, shape in ((0, (300, 24)), (1, (24, 300)), (0, (1, 8)), (0, (5, 8))):
        sp = G.both_sparse(*shape, seed=5, dim=dim)
        nnz = (sp != 0).sum(dim)
        assert int(nnz.max()) <= G.MID_BOTH_NNZ and int(nnz.min()) >= min(shape[dim], 2)
        first, last = sp.select(dim, 0), sp.select(dim, shape[dim] - 1)
        assert bool((first != 0).all()) and bool((last != 0).all())
        assert set(sp.abs().unique().tolist()) <= {0.0, 257.0, 514.0}
        hi, md = G.split(sp)
        assert torch.equal(hi + md, sp.double()) and torch.equal(md != 0, sp != 0)


@pytest.mark.parametrize("grid", G.GRIDS)
def test_operand_pairs_are_what_they_claim(grid):
    a, b = G.operands(grid, 70, 256, 48, seed=11)
    (ah, am), (bh, bm) = G.split(a), G.split(b)
    assert torch.equal(ah + am, a.double()) and torch.equal(bh + bm, b.double())
    assert bool((b != 0).all())
    if grid != "mid_both":
        assert bool((a != 0).all())                                          # zeros only on mid_both
    a_mid, b_mid = grid in ("mid_a", "mid_both"), grid in ("mid_b", "mid_both")
    assert bool((am != 0).any(1).all()) == a_mid and bool((bm != 0).any(0).all()) == b_mid
    if grid in ("mid_a", "mid_b"):
        assert bool((am != 0).any(0).all()) == a_mid and bool((bm != 0).any(1).all()) == b_mid
        assert float((b if a_mid else a).abs().max()) <= G.PARTNER_MAX
    if not a_mid:
        assert not bool((am != 0).any())
    if not b_mid:
        assert not bool((bm != 0).any())


def test_exactness_bound():
    G.assert_exact(65535, 64)
    with pytest.raises(AssertionError):
        G.assert_exact(65536, 64)
    with pytest.raises(AssertionError):
        G.operands("small", 4, 65536, 8, seed=0)
    with pytest.raises(AssertionError):
        G.operands("mid_a", 4, 2048, 8, seed=0)
    assert G.EXACT_LIMIT == 1 << 22
    assert G.MID_BOTH_NNZ * G.MID_BOTH_TERM < G.EXACT_LIMIT
    a, _ = G.operands("mid_a", 4, 1793, 8, seed=0)                           # long reductions fall back to 9 bits
    assert float(a.abs().max()) < 512


@pytest.mark.parametrize("grid", G.GRIDS)
def test_any_summation_order_in_fp32_or_fp64_equals_int64(grid):
    M, K, N = 33, 512, 40
    a, b = G.operands(grid, M, K, N, seed=7)
    want = G._mm(a, b, int64=True)
    assert float(want.abs().max()) < G.EXACT_LIMIT
    g = torch.Generator().manual_seed(1)
    for trial in range(4):
        p = torch.randperm(K, generator=g) if trial else torch.arange(K)
        ap, bp = a[:, p], b[p]
        assert torch.equal((ap @ bp).double(), want)                         # fp32, the library's order
        assert torch.equal(ap.double() @ bp.double(), want)
        seq = torch.zeros(M, N)                                              # fp32, one term at a time
        for k in range(0, K, 8):
            seq = seq + ap[:, k:k + 8] @ bp[k:k + 8]
        assert torch.equal(seq.double(), want)
        chains = [(ap[:, c::4] @ bp[c::4]) for c in range(4)]                # four chains, as the split-K reduce
        assert torch.equal(((chains[0] + chains[1]) + (chains[2] + chains[3])).double(), want)
    # the split parts are on the grid as well: each partial product alone is exact in fp32
    (ah, am), (bh, bm) = G.split(a), G.split(b)
    for x, y in ((ah, bh), (ah, bm), (am, bh), (am, bm)):
        assert torch.equal((x.float() @ y.float()).double(), x @ y)


def test_split3_ref_against_the_fp64_product():
    for grid in ("small", "mid_a", "mid_b"):
        a, b = G.operands(grid, 20, 256, 24, seed=5)
        full = a.double() @ b.double()
        assert torch.equal(G.split3_ref(a, b, four=False), full) and torch.equal(G.split3_ref(a, b, four=True), full)
    a, b = G.operands("mid_both", 20, 256, 24, seed=5)
    full = a.double() @ b.double()
    assert torch.equal(G.split3_ref(a, b, four=True), full)
    three = G.split3_ref(a, b, four=False)
    # every element carries mid.mid terms (+-1, +-2); they can cancel in one element, not in a whole row or column
    diff = three != full
    assert bool(diff.any(0).all()) and bool(diff.any(1).all()) and float(diff.double().mean()) > 0.5
    assert float((three - full).abs().max()) <= 2 * G.MID_BOTH_NNZ


def test_references_agree_with_int64():
    dz, rows = G.wgrad_operands("small", 1025, 24, 40, seed=3)
    out, cs = G.wgrad_ref(dz, rows)
    out_i, _ = G.wgrad_ref(dz, rows, int64=True)
    assert torch.equal(out, out_i) and torch.equal(cs, dz.long().sum(0).double())
    dz, W, skip = G.dgrad_operands(65, 1024, 128, seed=4, with_skip=True)
    assert torch.equal(G.dgrad_ref(dz, W, skip), G.dgrad_ref(dz, W, skip, int64=True))
    # one rounding, to nearest even: the same bits as torch's own fp32 -> bf16 conversion
    s = (dz.double() @ W.double() + skip.double()).float()
    assert torch.equal(G.dgrad_ref(dz, W, skip), s.bfloat16().view(torch.int16))
    assert bool((G.bits_to_float(G.dgrad_ref(dz, W, skip)) != s).any())      # (and the rounding is not vacuous)


# ------------------------------------------------------------------ wg::shape_for
def test_shape_for_against_hand_computed_cases():
    """by hand from the C++ formula (wgrad_bf16.hip): want = ceil(512 / tiles) capped at ceil(M / 256),
    rows_per_slice = ceil(ceil(M / want) / 32) * 32 (at least 32), slices = ceil(max(M, 1) / rows_per_slice)"""
    table = {
        # (M, Ho, Hi): (to, ti, tiles, rows_per_slice, slices)
        (0, 64, 64): (128, 128, 1, 32, 1),
        (1, 64, 64): (128, 128, 1, 32, 1),
        (256, 128, 128): (128, 128, 1, 256, 1),
        (257, 128, 128): (128, 128, 1, 160, 2),             # want 2: ceil(257 / 2) = 129 -> 160
        (1025, 128, 512): (128, 128, 4, 224, 5),            # want 5: 205 -> 224; 4 x 224 = 896 < 1025
        (1793, 8, 24): (128, 128, 1, 256, 8),               # want 8: 225 -> 256; the last slice holds row 1792 alone
        (4097, 512, 256): (256, 256, 2, 256, 17),           # want min(256, 17): 241 -> 256
        (5000, 520, 8): (256, 128, 3, 256, 20),             # three ho tiles; want min(171, 20): 250 -> 256
        (5000, 136, 128): (256, 128, 1, 256, 20),
        (2_000_000, 512, 256): (256, 256, 2, 7840, 256),    # want 256: 7813 -> 7840; 255 x 7840 = 1,999,200
        (2_000_000, 1024, 512): (256, 256, 8, 31264, 64),   # want 64: 31250 -> 31264
    }
    for (M, Ho, Hi), (to, ti, tiles, rps, slices) in table.items():
        assert G.shape_for(M, Ho, Hi) == dict(to=to, ti=ti, tiles=tiles, rows_per_slice=rps, slices=slices), (M, Ho, Hi)
    for (Ho, Hi), (to, ti) in G.WGRAD_SHAPES:
        s = G.shape_for(1000, Ho, Hi)
        assert (s["to"], s["ti"]) == (to, ti)
        assert Ho % 8 == 0 and Hi % 8 == 0
    assert set(G.WGRAD_S3_SHAPES) <= {s for s, _ in G.WGRAD_SHAPES}
    assert {G.shape_for(9, *s)["to"] * 1000 + G.shape_for(9, *s)["ti"] for s in G.WGRAD_S3_SHAPES} == \
        {128128, 256128, 256256}


@pytest.mark.parametrize("shape", [s for s, _ in G.WGRAD_SHAPES], ids=lambda s: f"{s[0]}x{s[1]}")
def test_slices_tile_the_rows_and_the_edges_are_edges(shape):
    Ho, Hi = shape
    edges = G.m_edges(Ho, Hi)
    assert {0, 1, 31, 32, 33, 255, 256, 257} <= set(edges)
    lasts, counts = set(), set()
    for M in edges + [1000, 4097, 70001]:
        r = G.slice_ranges(M, Ho, Hi)
        s = G.shape_for(M, Ho, Hi)
        assert len(r) == s["slices"] and r[0][0] == 0 and r[-1][1] == M
        assert all(a[1] == b[0] for a, b in zip(r, r[1:]))                   # no gap, no overlap
        assert all(e - b == s["rows_per_slice"] for b, e in r[:-1]) and (M == 0 or 0 < r[-1][1] - r[-1][0] <= s["rows_per_slice"])
        assert s["rows_per_slice"] % G.KT == 0
        assert G.workspace_bytes(M, Ho, Hi) == s["slices"] * (Ho * Hi + Ho) * 4
        if M in edges and len(r) >= 2:
            lasts.add((r[-1][1] - r[-1][0], s["rows_per_slice"]))
            counts.add(len(r))
    assert any(n == 1 for n, _ in lasts) and any(n == G.KT for n, _ in lasts) and any(n == rps for n, rps in lasts)
    assert max(counts) >= 5 and any(c % 4 for c in counts if c >= 5)         # four chains AND the remainder loop
    assert max(edges) * G.SMALL_MAX ** 2 < G.EXACT_LIMIT


def test_trip_geometry():
    assert G.trip_rows("bwd_layer", 256) == G.trip_rows("bwd_layer", 304) == 32768
    assert G.trip_rows("split3_l128", 256) == 32768 and G.trip_rows("split3_l128", 304) == 38912
    assert G.trip_rows("split3_l256_rows64", 256) == 16384 and G.trip_rows("split3_l256_rows128", 256) == 32768
    assert G.trip_first_row("split3_l256_rows64", 2, 256) == 32768
    assert G.trip_of_row("bwd_layer", 32768 + 64, 256) == (1, 1, 513)
    assert G.trip_of_row("split3_l256_rows128", 2 * 32768 + 192, 256) == (2, 1, 513)


# ------------------------------------------------------------------ mutants
def _caught(kind, mutants, same, applicable, seen):
    for name, got in mutants.items():
        assert not same(got), f"{kind}: mutant {name} is NOT caught"
        seen[name] = seen.get(name, 0) + 1
    assert set(mutants) == set(applicable), (kind, sorted(mutants), sorted(applicable))


WGRAD_MUTANTS = {"dropped_row", "duplicated_row", "last_slice_skipped", "last_step_skipped", "columns_swapped",
                 "colsum_wrong_tile"}


@pytest.mark.parametrize("shape", [s for s, _ in G.WGRAD_SHAPES], ids=lambda s: f"{s[0]}x{s[1]}")
def test_mutants_are_caught_on_every_wgrad_bf16_case(shape):
    Ho, Hi = shape
    seen = {}
    for M in G.m_edges(Ho, Hi):
        dz, rows = G.wgrad_operands("small", M, Ho, Hi, G.wgrad_seed("small", M, Ho, Hi))
        ref, cs = G.wgrad_ref(dz, rows)
        assert M == 0 or bool((ref != 0).any())
        same = lambda got: torch.equal(got[0], ref) and torch.equal(got[1], cs)
        _caught(f"wgrad_bf16 {shape} M={M}", G.wgrad_mutants(dz, rows), same, WGRAD_MUTANTS if M else (), seen)
    print("\nwgrad_bf16", shape, "caught:", ", ".join(f"{k} x{v}" for k, v in sorted(seen.items())))
    assert set(seen) == WGRAD_MUTANTS


@pytest.mark.parametrize("grid", G.GRIDS)
@pytest.mark.parametrize("shape", G.WGRAD_S3_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mutants_are_caught_on_every_wgrad_f32_split3_case(shape, grid):
    Ho, Hi = shape
    extra = {"mid_both": {"mid_mid_dropped"}, "small": set()}.get(grid, {"mid_hi_chunk_dropped"})
    seen = {}
    for M in G.m_edges(Ho, Hi):
        dz, rows = G.wgrad_operands(grid, M, Ho, Hi, G.wgrad_seed(grid, M, Ho, Hi))
        ref, cs = G.wgrad_ref(dz, rows)
        assert torch.equal(G.split3_ref(dz.t(), rows, four=True), ref)       # the kernel forms all four products
        same = lambda got: torch.equal(got[0], ref) and torch.equal(got[1], cs)
        _caught(f"wgrad_f32_split3 {shape} {grid} M={M}", G.wgrad_mutants(dz, rows, s3_grid=grid), same,
                (WGRAD_MUTANTS | extra) if M else (), seen)
    print("\nwgrad_f32_split3", shape, grid, "caught:", ", ".join(f"{k} x{v}" for k, v in sorted(seen.items())))
    assert set(seen) == WGRAD_MUTANTS | extra


@pytest.mark.parametrize("N", G.DGRAD_N)
@pytest.mark.parametrize("K", G.DGRAD_K)
def test_mutants_are_caught_on_every_backward_layer_case(K, N):
    seen = {}
    base = {"dropped_term", "duplicated_term", "columns_swapped", "truncated"}
    for M in G.TILE_M:
        for with_skip in (False, True):
            dz, W, skip = G.dgrad_operands(M, K, N, G.dgrad_seed(M, K, N), with_skip)
            ref = G.dgrad_ref(dz, W, skip)
            _caught(f"backward layer K={K} N={N} M={M} skip={with_skip}", G.dgrad_mutants(dz, W, skip),
                    lambda got: torch.equal(got, ref), base | ({"skip_after_rounding"} if with_skip else set()), seen)
    print(f"\nbackward layer K={K} N={N} caught:", ", ".join(f"{k} x{v}" for k, v in sorted(seen.items())))
    assert set(seen) == base | {"skip_after_rounding"}


@pytest.mark.parametrize("N", G.DGRAD_N)
def test_mutants_are_caught_on_the_two_trip_backward_layer_case(N):
    """M = two full trips + 65 rows, K = 128: the mutants must show in the rows of trips 2 and 3 themselves (rows are
    independent: checked on the tiles at both ends of trip 2 and on trip 3)"""
    T = G.trip_rows("bwd_layer", 256)
    M, K = 2 * T + 65, 128
    dz, W, skip = G.dgrad_operands(M, K, N, G.dgrad_seed(M, K, N), True)
    rows = torch.cat([torch.arange(T, T + 128), torch.arange(2 * T - 64, M)])      # 192 rows of trip 2, the 65 of trip 3
    dz, skip = dz[rows], skip[rows]
    ref = G.dgrad_ref(dz, W, skip)
    for name, got in G.dgrad_mutants(dz, W, skip).items():
        bad = (got != ref).any(1)
        assert bool(bad[:192].any()) and bool(bad[192:].any()), f"two-trip case N={N}: {name} NOT caught in both trips"
    print(f"\nbackward layer two-trip N={N}: all mutants caught in trip 2 and in trip 3")


@pytest.mark.parametrize("grid", G.GRIDS)
@pytest.mark.parametrize("N", G.LINEAR_N)
@pytest.mark.parametrize("K", G.LINEAR_K)
def test_mutants_are_caught_on_every_linear_and_project_case(K, N, grid):
    """hgnn_linear_f32_split3 forms four products, hgnn_project_f32_split3 three: both reference flavours"""
    seen = {}
    base = {"dropped_term", "duplicated_term", "columns_swapped"}
    for M in G.TILE_M:
        a, b = G.operands(grid, M, K, N, G.linear_seed(grid, M, K, N))
        for four in (True, False):
            ref = G.split3_ref(a, b, four)
            extra = {"mid_both": {"mid_mid_dropped" if four else "mid_mid_added"}, "small": set()}.get(grid, {"mid_hi_chunk_dropped"})
            _caught(f"split3 GEMM K={K} N={N} {grid} M={M} four={four}", G.linear_mutants(a, b, grid, four),
                    lambda got: torch.equal(got, ref), base | extra, seen)
    print(f"\nsplit3 GEMM K={K} N={N} {grid} caught:", ", ".join(f"{k} x{v}" for k, v in sorted(seen.items())))
    assert base <= set(seen)
