"""tests/wgrad_f32_ref.py proves itself on the CPU: the float32 emulation of hgnn_wgrad_f32's order equals the int64
product on every integer case that tests/test_gpu_wgrad_f32.py hands to the kernel, every mutant differs from it on
every such case, and the a-priori error bar holds for the emulation on the random-data cases."""
import pytest
import torch

import gemm_ref as G
import wgrad_f32_ref as F


def test_shape_function_by_hand():
    """by hand from the C++ formula (wgrad_f32.hip): want = ceil(512 / tiles) capped at ceil(M / 128), rows per slice
    rounded up to 16"""
    assert F.shape_for(0, 512, 256) == dict(to=256, ti=256, tiles=2, rows_per_slice=16, slices=1)
    assert F.shape_for(128, 128, 128) == dict(to=128, ti=128, tiles=1, rows_per_slice=128, slices=1)
    assert F.shape_for(129, 128, 128) == dict(to=128, ti=128, tiles=1, rows_per_slice=80, slices=2)
    s = F.shape_for(2_000_000, 512, 256)
    assert (s["to"], s["ti"], s["tiles"], s["slices"], s["rows_per_slice"]) == (256, 256, 2, 256, 7824)
    s = F.shape_for(120_000, 512, 256)
    assert (s["slices"], s["rows_per_slice"]) == (250, 480)
    s = F.shape_for(2_000_000, 1024, 1024)
    assert (s["tiles"], s["slices"], s["rows_per_slice"]) == (16, 32, 62512)
    assert F.shape_for(5000, 256, 128)["to"] == 256 and F.shape_for(5000, 256, 128)["ti"] == 128
    for shape, tile in F.TILE_OF.items():
        s = F.shape_for(1000, *shape)
        assert (s["to"], s["ti"]) == tile


@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_m_edges_cover_the_decomposition(shape):
    Ho, Hi = shape
    edges = F.m_edges(Ho, Hi)
    assert {0, 1, 15, 16, 17, 127, 128, 129} <= set(edges)
    lasts = {M: F.slice_ranges(M, Ho, Hi) for M in edges}
    last = lambda r: r[-1][1] - r[-1][0]
    assert all(len(lasts[M]) == 1 for M in edges if M <= 128) and len(lasts[129]) == 2
    assert any(len(r) >= 2 and last(r) == 1 for r in lasts.values())
    assert any(len(r) >= 2 and last(r) == F.KT for r in lasts.values())
    assert any(len(r) >= 2 and last(r) == F.shape_for(M, Ho, Hi)["rows_per_slice"] for M, r in lasts.items())
    assert any(len(r) >= 5 for r in lasts.values())
    for M, r in lasts.items():                               # the slices tile [0, M) exactly, in order
        assert r[0][0] == 0 and r[-1][1] == M and all(a[1] == b[0] for a, b in zip(r, r[1:]))
        assert M == 0 or all(e > b for b, e in r)


def test_wide_grids_are_what_they_claim():
    for grid in F.WIDE:
        dz, rows = F.operands(grid, 301, 24, 40, 5)
        w, p = (dz, rows) if grid == "wide_a" else (rows, dz)
        nz = w[w != 0]
        assert int((w != 0).sum(0).max()) <= F.WIDE_NNZ
        assert bool((w[0] != 0).all()) and bool((w[150] != 0).all()) and bool((w[300] != 0).all())
        assert bool((nz.abs() > (1 << 17)).all()) and bool((nz.abs() < (1 << 18)).all())
        assert bool((nz.abs().long() % 2 == 1).all())
        assert bool((p.abs() == 1).all())
        hi, mid = G.split(nz)                                # neither bf16 nor hi + mid holds such a value
        assert bool((hi != nz.double()).all()) and bool((hi + mid != nz.double()).all())


def _same(a, b):
    return torch.equal(a.double(), b.double())


@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_emulation_is_exact_and_every_mutant_is_caught(shape):
    Ho, Hi = shape
    seen = set()
    for grid in F.grids_of(shape):
        for M in F.m_edges(Ho, Hi):
            dz, rows = F.operands(grid, M, Ho, Hi, F.seed_of(grid, M, Ho, Hi))
            assert dz.shape == (M, Ho) and rows.shape == (M, Hi)
            r64 = F.ref(dz, rows, int64=True)
            assert _same(F.ref(dz, rows), r64)
            assert float(r64.abs().max()) < G.EXACT_LIMIT if M else not r64.any()
            what = f"{grid} M={M} {Ho}x{Hi}"
            assert _same(F.emulate(dz, rows), r64), what
            mut = F.mutants(dz, rows, grid)
            want = (F.MUTANTS + (F.WIDE_MUTANTS if grid in F.WIDE else ())) if M else ()
            assert set(mut) == set(want), what
            for name, m in mut.items():
                assert not _same(m, r64), f"{what}: mutant {name} is not told from the reference"
                seen.add(name)
    assert seen == set(F.MUTANTS + F.WIDE_MUTANTS)


@pytest.mark.parametrize("case", F.RANDOM_CASES, ids=lambda c: f"{c[0]}x{c[1]}_M{c[2]}")
def test_bar_holds_for_the_emulation_on_random_data(case):
    """standard normal rows; the emulation runs on a strided sample of 32 x 32 output elements (the elements are
    independent chains), the bar is the a-priori one"""
    Ho, Hi, M = case
    g = torch.Generator().manual_seed(Ho + Hi + M)
    dz = torch.randn(M, Ho, generator=g)
    rows = torch.randn(M, Hi, generator=g)
    ho = torch.arange(0, Ho, Ho // 32)
    hi = torch.arange(0, Hi, Hi // 32)
    got = F.emulate(dz, rows, ho, hi).double()
    ref = F.ref(dz, rows)[ho][:, hi]
    ratio = float(((got - ref).abs() / F.bar(dz, rows, ho, hi)).max())
    L, S = F.chain_and_slices(M, Ho, Hi)
    print(f"wgrad_f32 emulation {Ho}x{Hi} M={M}: L={L} S={S} worst |err| / bar = {ratio:.4f}")
    assert ratio <= 1.0
