"""CPU proofs of tests/bf16_mlp_ref.py, the references of tests/test_gpu_bf16_mlp_exact.py.

  * every exact (selector) case of the GPU file: the integer closed form equals the float64 definition; layer by layer
    the bf16 bits of the output do not move under either statistics scheme emulated in float32 (one-pass; wave-local
    centred statistics pooled over 4 and over 8 waves), eps in {0, 1e-5, 1e-3}, mean and rstd each off by a relative
    +-2^-12 -- so the GPU comparison does not rest on a correctly rounded sqrtf or division;
  * the mutants (two hidden slots swapped, a tile's gamma / beta offset shifted by 16, a gather index off by one row,
    the skip row of row e - 1, the last row of a tile unwritten) change the expected bits;
  * the save_pre[0] references equal an int64 product, and the pre-projected form differs from the direct one;
  * the float32 emulation of the random networks against the float64 mirror: the figure behind the per-element bar
    bf16_mlp_ref.C_BAR, D_BAR.
"""
import itertools

import numpy as np
import pytest
import torch

import bf16_mlp_ref as B
import gemm_ref as G
import ln_ref as R

EXACT_CASES = [(cfg, M, acts) for cfg in sorted(B.EXACT_CONFIGS) for M in B.exact_ms(cfg) for acts in B.EXACT_ACTS]
PERTS = [(0.0, 0.0)] + [(a * B.PERT, b * B.PERT) for a, b in itertools.product((-1, 1), repeat=2)]
SCHEMES = (("onepass", 4), ("pooled", 4), ("pooled", 8))


@pytest.mark.parametrize("cfg", sorted(B.EXACT_CONFIGS))
def test_exact_cases_are_stable(cfg):
    worst_rows = 0
    for M in B.exact_ms(cfg):
        for acts in B.EXACT_ACTS:
            case = B.exact_case(cfg, M, acts)
            want = B.expected_bits(case)
            assert torch.equal(B.forward_f64(case["x"], case["layers"], case["skip"]), want), (cfg, M, acts, "float64")
            assert len(set(case["c_of_row"].tolist())) >= min(M, case["widths"][1] // 16)
            worst_rows = max(worst_rows, M)
            for z, gm, bt, act, sk, bits in B.exact_layers(case):
                for (scheme, nw), eps, (dm, dr) in itertools.product(SCHEMES, (0.0, 1e-5, 1e-3), PERTS):
                    got = B.layer_f32(z, gm, bt, act, sk, eps, scheme, nw, dm, dr)
                    assert torch.equal(got, bits), (cfg, M, acts, scheme, nw, eps, dm, dr)
    assert worst_rows == 193


def test_mutants_change_the_expected_bits():
    hits, applicable = {}, {}
    for cfg, M, acts in EXACT_CASES:
        if acts != B.EXACT_ACTS[sorted(B.EXACT_CONFIGS).index(cfg) % 2] or M not in (1, 65, 193):
            continue                              # a third of the cases: the float64 forwards of the widest are slow
        case = B.exact_case(cfg, M, acts)
        want = B.expected_bits(case)
        for name, bits in B.mutants(case).items():
            kind = name.rstrip("0123456789").replace("_seg", "").replace("_layer", "")
            applicable[kind] = applicable.get(kind, 0) + 1
            changed = not torch.equal(bits, want)
            hits[kind] = hits.get(kind, 0) + changed
            assert changed or M == 1, (cfg, M, acts, name)     # one row may happen to agree; several rows never do
    assert set(applicable) == {"hidden_slots_swapped", "ln_offset", "gather_off_by_one", "skip_from_previous_row",
                               "tile_last_row_unwritten"}
    assert all(hits[k] > 0 for k in applicable), hits


@pytest.mark.parametrize("name", sorted(B.PRE_CONFIGS))
def test_layer1_sum_reference(name):
    case = B.pre_case(name)
    x = torch.cat([t if i is None else t[i] for t, i in case["segments"]], dim=1)
    s = (x.long() @ case["W"].long().t() + case["b"].long()).double()
    assert float(s.abs().max()) < G.EXACT_LIMIT
    assert torch.equal(B.pre_ref_bits(case), G.round_bf16_bits(s))
    trunc = G.round_bf16_bits(s, truncate=True)
    assert not torch.equal(trunc, B.pre_ref_bits(case))                     # the sums do need rounding
    if case["pre"]:
        proj = [i for i, (_, idx) in enumerate(case["segments"]) if idx is not None][:2]
        assert not torch.equal(B.pre_ref_bits(case, proj), B.pre_ref_bits(case))   # and P's own rounding shows


def test_kernel_gelu_distance_from_erf_form():
    y = torch.linspace(-12, 12, 480001, dtype=torch.float64)
    d = float((B.gelu_kernel64(y) - R.act64(y, R.ACT_GELU)).abs().max())
    print(f"\nFIGURE gelu x sigmoid(2u) vs erf form: max |difference| = {d:.3e}")
    assert 1e-4 < d <= 5e-4


def test_boundary_rows():
    rows = B.boundary_rows(300, 128)
    assert rows[0] == 0 and rows[-1] == 299 and {15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 271, 272, 287, 288} <= set(rows)
    assert B.boundary_rows(1, 64) == [0]


def test_emulation_figure_behind_the_bar():
    """the float32 emulation (ln_ref.emul_net: one-pass + shift and centred statistics -- pooled over 8 slices at the
    feature-split kernel's widths --, both summation orders),
    its output rounded to bf16 like a kernel's, against the float64 mirror on every case of section 4: the worst
    per-element excess over one bf16 ulp.  D_BAR is twice that, C_BAR = 1 (the ulp itself)."""
    worst, where = -1.0, None
    with B.kernel_gelu():
        for cfg in sorted(B.BAR_CONFIGS):
            w_cfg = -1.0
            for M in B.bar_ms(cfg):
                case = B.bar_case(cfg, M)
                ref = B.mirror(case).numpy()
                rows = np.arange(M)
                second = "pooled" if B.BAR_CONFIGS[cfg][0] == "bf16_split" else "centred"   # (pooled: 8 slices, >= 128 wide)
                for mode, order in itertools.product(("onepass_shift", second), ("fwd", "rev")):
                    out = torch.from_numpy(R.emul_net(case, mode, order, rows)).bfloat16().double().numpy()
                    e = B.excess(out, ref)
                    w_cfg = max(w_cfg, e)
                    if e > worst:
                        worst, where = e, (cfg, M, mode, order)
            print(f"FIGURE emulation excess {cfg}: {w_cfg:.3e}")
    print(f"FIGURE worst emulation excess over one bf16 ulp: {worst:.4e} at {where}; D_BAR = {B.D_BAR:.4e}")
    assert B.C_BAR == 1.0
    assert worst <= B.D_BAR / 2 <= 1.05 * worst, (worst, B.D_BAR)
