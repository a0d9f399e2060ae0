"""The bars of tests/test_gpu_bwd_layer_f32.py, proven without a device: a float32 emulation of the arithmetic
hgnn_mlp_backward_layer_f32 is to perform -- da = dz W as a k-ordered chain of fused multiply-adds starting at 0, then
the centred LayerNorm / activation backward and forward -- stays at or below HALF of every bar of the project's fp32
parity (1e-4), in both summation orders, on every case of ln_ref.CASES at the five shapes the GPU file runs.

Worst figures of the emulation over all cases, shapes, activations and both orders: 4.7e-5 on a' (r256, normwise
only), 3.2e-5 on dz', 2.2e-5 on the column sums, 1e-6 on the const rows.
"""
import pytest

import bwd_layer_f32_ref as B
import ln_ref as R

HALF = 0.5 * R.F32_BAR


@pytest.mark.parametrize("K,N", B.BAR_SHAPES)
def test_emulation_stays_within_half_of_every_bar(K, N):
    worst = {}
    for act in B.BAR_ACTS:
        for name in R.CASES:
            rc, _, _, ref = B.bar_case(K, N, name, act)
            for order in ("fwd", "rev"):
                for what, v in B.errors(B.emulate(K, N, name, act, order), ref, rc).items():
                    key = (what, name, act, order)
                    worst[key] = v
    bad = {k: v for k, v in worst.items() if not v <= HALF}
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print(f"\nK={K} N={N}: worst emulation errors " + ", ".join(f"{k[0]} {k[1]} act{k[2]} {k[3]} {v:.2e}" for k, v in top))
    assert not bad, f"K={K} N={N}: the emulation exceeds half of the 1e-4 bar at {bad}"


def test_relu_rows_are_clear_of_zero_and_const_rows_stay_const():
    for K, N in B.BAR_SHAPES:
        for name in R.CASES:
            rc, _, _, _ = B.bar_case(K, N, name, R.ACT_RELU)
            plain = R.make_rows_case(name, N, seed=K)
            for r in rc["const_rows"]:
                assert bool((rc["z"][r] == plain["z"][r]).all())
            moved = int((rc["z"] != plain["z"]).sum())
            assert moved <= rc["z"].numel() // 100, (K, N, name, moved)
