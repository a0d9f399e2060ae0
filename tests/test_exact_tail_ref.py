"""tests/exact_tail_ref.py proves itself on the CPU: the float32 emulation of each order contract equals the exact
product on every integer case that tests/test_gpu_exact_tail.py hands to the kernels, every mutant differs from it on
every case it applies to, and the a-priori bars hold for the emulations on random data."""
import pytest
import torch

import exact_tail_ref as T
import gemm_ref as G
import wgrad_f32_ref as F


def test_shape_functions_by_hand():
    """by hand from the C++ formulas (project_f32.hip, narrow_f32.hip)"""
    assert [T.pass_width(N) for N in (16, 32, 48, 64, 96, 128, 144, 256, 512, 1024)] == \
        [16, 32, 64, 64, 128, 128, 256, 256, 256, 256]
    assert T.project_tiles(120_000, 512, 2) == dict(pass_width=256, passes=2, row_tiles=1875, grid=(1875, 4))
    assert T.project_tiles(65, 96, 1)["grid"] == (2, 1) and T.project_tiles(4099, 1024, 2)["grid"] == (65, 8)
    assert [T.linear_lanes(K) for K in (4, 8, 12, 16, 60, 64, 128, 256, 260, 1024)] == [1, 2, 2, 4, 8, 16, 32, 64, 64, 64]
    # want = ceil(131072 / ((K / 4) * ceil(n / 8))) capped at ceil(M / 64); rows per slice rounded up to 16
    assert T.wgrad_shape(0, 3, 128) == dict(rows_per_slice=16, slices=1)
    assert T.wgrad_shape(64, 1, 256) == dict(rows_per_slice=64, slices=1)
    assert T.wgrad_shape(65, 1, 256) == dict(rows_per_slice=48, slices=2)
    assert T.wgrad_shape(2_000_000, 1, 256) == dict(rows_per_slice=992, slices=2017)
    assert T.wgrad_shape(2_000_000, 32, 1024) == dict(rows_per_slice=15632, slices=128)
    assert T.wgrad_shape(120_000, 3, 128) == dict(rows_per_slice=64, slices=1875)
    assert T.wgrad_workspace_bytes(120_000, 3, 128) == 1875 * 3 * 129 * 4


@pytest.mark.parametrize("K", T.NARROW_K)
def test_narrow_m_cover_the_decomposition(K):
    for n in T.NARROW_N:
        edges = T.narrow_m(n, K)
        assert {0, 1, 63, 64, 65, T.BIG_M} <= set(edges)
        lasts = {M: T.wgrad_slices(M, n, K) for M in edges}
        last = lambda r: r[-1][1] - r[-1][0]
        assert all(len(lasts[M]) == 1 for M in edges if M <= 64) and len(lasts[65]) == 2
        assert any(len(r) >= 2 and last(r) == 1 for r in lasts.values())
        assert any(len(r) >= 2 and last(r) == 16 for r in lasts.values())
        assert any(len(r) >= 2 and last(r) == T.wgrad_shape(M, n, K)["rows_per_slice"] for M, r in lasts.items())
        assert any(len(r) >= 5 for M, r in lasts.items() if M < T.BIG_M)
        for M, r in lasts.items():                           # the slices tile [0, M) exactly, in order
            assert r[0][0] == 0 and r[-1][1] == M and all(a[1] == b[0] for a, b in zip(r, r[1:]))
            assert M == 0 or all(e > b for b, e in r)


def test_wide_grids_are_what_they_claim():
    for grid in T.WIDE:
        x, w0, w1 = T.project_operands(grid, 40, 128, 32, 5)
        w, p = (x, torch.cat([w0, w1])) if grid == "wide_a" else (torch.cat([w0, w1]), x)
        nz = w[w != 0]
        assert int((w != 0).sum(1).max()) <= F.WIDE_NNZ      # along the reduction (k)
        assert bool((w[:, 0] != 0).all()) and bool((w[:, 64] != 0).all()) and bool((w[:, 127] != 0).all())
        assert bool((nz.abs() > (1 << 17)).all()) and bool((nz.abs() < (1 << 18)).all())
        assert bool((p.abs() == 1).all())
        hi, mid = G.split(nz)                                # neither bf16 nor hi + mid holds such a value
        assert bool((hi != nz.double()).all()) and bool((hi + mid != nz.double()).all())


def _same(a, b):
    return torch.equal(a.double(), b.double())


def _rows(M):
    """the rows the emulation runs on (the rows are independent): all of them up to 300, else both ends"""
    return torch.arange(M) if M <= 300 else torch.cat([torch.arange(100), torch.arange(M - 100, M)])


def _exact(r):
    assert float(r.abs().max()) < G.EXACT_LIMIT if r.numel() else True


PROJECT_MUTANTS = {"dropped_row", "last_16_k_skipped", "columns_swapped", "block1_from_block0"}
SPLIT3 = {"split3_three_products", "split3_four_products"}


@pytest.mark.parametrize("shape", T.PROJECT_SHAPES, ids=lambda s: f"K{s[0]}_N{s[1]}")
def test_projection_emulation_is_exact_and_every_mutant_is_caught(shape):
    K, N = shape
    for grid in T.GRIDS:
        for M in T.project_m(N):
            x, w0, w1 = T.project_operands(grid, M, K, N, T.seed_of("project", grid, M, K, N))
            assert x.shape == (M, K) and w0.shape == w1.shape == (N, K)
            r0, r1 = T.project_ref(x, w0), T.project_ref(x, w1)
            _exact(r0), _exact(r1)
            what = f"project {grid} M={M} K={K} N={N}"
            rows = _rows(M)
            assert _same(T.emulate_project(x[rows], w0), r0[rows]) and _same(T.emulate_project(x[rows], w1), r1[rows]), what
            mut = T.project_mutants(x, w0, w1, grid)
            assert set(mut) == ((PROJECT_MUTANTS | (SPLIT3 if grid in T.WIDE else set())) if M else set()), what
            for name, (m0, m1) in mut.items():
                if name == "block1_from_block0":
                    assert not _same(m1, r1), f"{what}: mutant {name} is not told from the reference"
                else:
                    assert not _same(m0, r0) and not _same(m1, r1), f"{what}: mutant {name} is not told from the reference"


@pytest.mark.parametrize("K", T.NARROW_K)
def test_narrow_emulations_are_exact_and_every_mutant_is_caught(K):
    seen = set()
    for n in T.NARROW_N:
        for M in T.narrow_m(n, K):
            for grid in T.grids_at(M):
                what = f"{grid} M={M} n={n} K={K}"
                big = M == T.BIG_M
                # at 70,001 rows linear and outer (independent rows) are proved on 201 rows -- both ends and the middle
                # one that the dropped-row mutant takes -- and wgrad (independent columns) on 8 columns of x
                keep = torch.cat([torch.arange(100), torch.tensor([M // 2]), torch.arange(M - 100, M)]) if big else None
                # linear
                x, W, bias = T.linear_operands(grid, M, K, n, T.seed_of("linear", grid, M, n, K))
                assert x.shape == (M, K) and W.shape == (n, K) and bias.shape == (n,)
                x = x[keep] if big else x
                rows = _rows(x.shape[0])
                r = T.linear_ref(x, W, bias)
                _exact(r)
                assert _same(T.emulate_linear(x[rows], W, bias), r[rows]), "linear " + what
                assert _same(T.emulate_linear(x[rows], W), T.linear_ref(x, W)[rows]), "linear " + what
                mut = T.linear_mutants(x, W, bias, grid)
                for name, m in mut.items():
                    assert not _same(m, r), f"linear {what}: mutant {name} is not told from the reference"
                    seen.add("linear/" + name)
                # outer
                y, W, add = T.outer_operands(grid, M, n, K, T.seed_of("outer", grid, M, n, K))
                assert y.shape == (M, n) and W.shape == (n, K) and add.shape == (M, K)
                y, add = (y[keep], add[keep]) if big else (y, add)
                r = T.outer_ref(y, W, add)
                _exact(r)
                assert _same(T.emulate_outer(y[rows], W, add[rows]), r[rows]), "outer " + what
                assert _same(T.emulate_outer(y[rows], W), T.outer_ref(y, W)[rows]), "outer " + what
                for name, m in T.outer_mutants(y, W, add, grid).items():
                    assert not _same(m, r), f"outer {what}: mutant {name} is not told from the reference"
                    seen.add("outer/" + name)
                # wgrad
                y, x = T.wgrad_operands(grid, M, n, K, T.seed_of("wgrad", grid, M, n, K))
                assert y.shape == (M, n) and x.shape == (M, K)
                cols = torch.arange(0, K, max(1, K // 8)) if big else None
                e, ecs = T.emulate_wgrad(y, x, cols)
                x = x[:, cols].contiguous() if big else x
                r, cs = T.wgrad_ref(y, x)
                _exact(r), _exact(cs)
                assert _same(e, r) and _same(ecs, cs), "wgrad " + what
                for name, (m, mcs) in T.wgrad_mutants(y, x, grid, K).items():
                    assert not _same(m, r), f"wgrad {what}: mutant {name} is not told from the reference"
                    seen.add("wgrad/" + name)
    assert {"linear/bias_dropped", "linear/dropped_row", "linear/last_piece_skipped", "linear/columns_swapped",
            "outer/add_dropped", "outer/dropped_row", "outer/columns_swapped", "outer/last_j_skipped",
            "wgrad/dropped_row", "wgrad/last_slice_skipped", "wgrad/columns_swapped"} <= seen
    assert {k + "/" + s for k in ("linear", "outer", "wgrad") for s in SPLIT3} <= seen


def _ratio(got, ref, bar):
    return float(((got.double() - ref).abs() / bar).max())


def test_bars_hold_for_the_emulations_on_random_data():
    """standard normal operands, the a-priori bars"""
    g = torch.Generator().manual_seed(11)
    x, w = torch.randn(200, 256, generator=g), torch.randn(512, 256, generator=g)
    ratios = {"project": _ratio(T.emulate_project(x, w), T.project_ref(x, w), T.bar_project(x, w))}
    W, b = torch.randn(6, 256, generator=g), torch.randn(6, generator=g)
    ratios["linear"] = _ratio(T.emulate_linear(x, W, b), T.linear_ref(x, W, b), T.bar_linear(x, W, b))
    y, add = torch.randn(200, 6, generator=g), torch.randn(200, 256, generator=g)
    ratios["outer"] = _ratio(T.emulate_outer(y, W, add), T.outer_ref(y, W, add), T.bar_outer(y, W, add))
    y, x = torch.randn(5000, 3, generator=g), torch.randn(5000, 128, generator=g)
    e, ecs = T.emulate_wgrad(y, x)
    (r, cs), (bar, bar_cs) = T.wgrad_ref(y, x), T.bar_wgrad(y, x)
    ratios["wgrad"], ratios["colsum"] = _ratio(e, r, bar), _ratio(ecs, cs, bar_cs)
    print("worst |err| / bar:", {k: round(v, 4) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0
