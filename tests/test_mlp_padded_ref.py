"""The algebra hgnn_mlp_forward_f32_padded relies on, proved with the float32 emulations of tests/ln_ref.py (in the
manner of tests/test_ln_ref.py; no device involved):

  * a network whose parameters are ZERO PADDED to the next template width -- W rows / columns, b, ln_w, ln_b -- and
    whose LayerNorm statistics run over the real features only, the padded ones MASKED out of the centred pass
    (``ln_ref.emul_layer(..., n_real=)``), equals the float64 definition of the unpadded network within HALF of the
    fp32 bar on every ``ln_ref.CASES`` entry, in both summation orders, at 16 padded features (h = 240 on the 256-wide
    instantiation) and at 112 (h = 144 on the same one, 7 padded tiles); the padded activations are exactly 0;
  * the alternative the narrow-encoder path uses at <= 12 padded features -- sum the squared deviations over ALL stored
    features and subtract  pad * mean^2  afterwards -- does NOT pass at 112 padded features on an offset row (r256):
    pad * mean^2 is ~ pad r^2 / n times the sum it is subtracted from, and the subtraction cancels.

Offsets: every case runs at ``ln_ref.r_eff`` of its nominal r at the widest REAL GEMM width, exactly as in
tests/test_ln_ref.py (``make_case`` applies it): r64 at 16 (K = 216) / 8 (K = 360), r256 and const_c256 at 64 / 32.  No
case needed a lower offset than that for the masked statistics.
"""
import numpy as np
import pytest
import torch

import ln_ref as R
from test_ln_ref import EMUL_ROWS, ORDERS, _carries_elem_bar, _figures

# widths -> (2P, P) of the instantiation they run on
SHAPES = {
    "pad16": dict(widths=[360, 240, 120], stored=(256, 128)),
    "pad112x2": dict(widths=[216, 144, 72], stored=(256, 128)),
    "pad112x3": dict(widths=[216, 144, 144, 72], stored=(256, 128)),
}


def _pad(t, rows, cols=None):
    out = np.zeros((rows,) if t.ndim == 1 else (rows, cols if cols is not None else t.shape[1]), np.float32)
    if t.ndim == 1:
        out[:t.shape[0]] = t
    else:
        out[:t.shape[0], :t.shape[1]] = t
    return out


def _padded_layers(case, stored):
    """[(W, b, gamma, beta, act, n_real)] as the kernel stores them: hidden layers 2P wide, the last P wide, W[l >= 1]
    with 2P columns, every padded entry zero"""
    hid, last = stored
    n = len(case["layers"])
    out = []
    for l, (W, b, gm, bt, act) in enumerate(case["layers"]):
        rows = last if l == n - 1 else hid
        out.append((_pad(W.numpy(), rows, hid if l > 0 else None), _pad(b.numpy(), rows), _pad(gm.numpy(), rows),
                    _pad(bt.numpy(), rows), act, int(W.shape[0])))
    return out


def _ln_act_corrected(z, gamma, beta, act, eps, n_real, order):
    """float32 LayerNorm + activation over the first n_real of z's features the way the narrow-encoder path does it:
    the squared deviations of ALL stored features are summed (a padded feature is exactly 0 and adds mean^2), then
    (stored - n_real) * mean^2 is subtracted"""
    f = np.float32
    z = np.asarray(z, f)
    n = f(n_real)
    mean = R._seq_sum32(z, order) / n                    # padded features add exactly 0
    d = z - mean[:, None]
    q = R._seq_sum32(d * d, order)
    q = q - f(z.shape[1] - n_real) * mean * mean
    rstd = f(1.0) / np.sqrt(q / n + f(eps), dtype=f)
    y = (d * rstd[:, None]) * np.asarray(gamma, f) + np.asarray(beta, f)
    return R.act64(torch.from_numpy(y.astype(np.float64)), act).numpy().astype(f)


def _emul_padded(case, stored, order, rows, corrected=False):
    layers = _padded_layers(case, stored)
    h = case["x"][rows].numpy()
    for l, (W, b, gm, bt, act, n_real) in enumerate(layers):
        z = R.emul_gemm(h, W, b, order)
        assert not z[:, n_real:].any(), "a padded accumulator is not exactly 0"
        if corrected:
            h = _ln_act_corrected(z, gm, bt, act, case["eps"], n_real, order)
        else:
            h = R.emul_ln_act(z, gm, bt, act, case["eps"], "centred", order, n_real=n_real)
        assert not h[:, n_real:].any(), "a padded activation is not exactly 0"
    out = h[:, :layers[-1][5]]
    return out if case["skip"] is None else out + case["skip"][rows].numpy()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_masked_statistics_on_padded_parameters_equal_the_unpadded_definition(shape):
    cfg = SHAPES[shape]
    lines = []
    for name in R.CASES:
        case = R.case_for(dict(widths=cfg["widths"]), name)
        for order in ORDERS:
            f = _figures(case, _emul_padded(case, cfg["stored"], order, EMUL_ROWS))
            lines.append(f"{shape:9s} {name:11s} r={case['r']:<5g} masked/{order}: " + " ".join(f"{k} {v:.1e}" for k, v in f.items()))
            assert f["rel"] <= 0.5 * R.F32_BAR, lines[-1]
            assert not _carries_elem_bar(case) or f["elem"] <= 0.5 * R.F32_BAR, lines[-1]
            assert f.get("const", 0.0) <= 0.5 * R.F32_BAR, lines[-1]
    print("\n" + "\n".join(lines))


@pytest.mark.parametrize("shape", ["pad112x2", "pad112x3"])
def test_subtracting_pad_mean_squared_afterwards_fails_at_seven_padded_tiles(shape):
    cfg = SHAPES[shape]
    case = R.case_for(dict(widths=cfg["widths"]), "r256")
    assert case["r"] >= 32
    lines = []
    for order in ORDERS:
        f = _figures(case, _emul_padded(case, cfg["stored"], order, EMUL_ROWS, corrected=True))
        lines.append(f"{shape:9s} r256        r={case['r']:<5g} corrected/{order}: " + " ".join(f"{k} {v:.1e}" for k, v in f.items())
                     + "   (must fail)")
        assert f["rel"] > R.F32_BAR, lines[-1]
    print("\n" + "\n".join(lines))


def test_the_correction_is_harmless_where_the_narrow_encoder_uses_it():
    """the existing narrow-encoder kernels (at most 12 padded features) are left as they are: at r256 the corrected
    form stays inside the bar there"""
    case = R.case_for(R.F32_CONFIGS["narrow64"], "r256")
    layers = case["layers"]
    for order in ORDERS:
        h = case["x"][EMUL_ROWS].numpy()
        for l, (W, b, gm, bt, act) in enumerate(layers):
            if l < len(layers) - 1:
                h = R.emul_layer(h, W.numpy(), b.numpy(), gm.numpy(), bt.numpy(), act, case["eps"], "centred", order)
            else:
                z = R.emul_gemm(h, _pad(W.numpy(), 64), _pad(b.numpy(), 64), order)
                h = _ln_act_corrected(z, _pad(gm.numpy(), 64), _pad(bt.numpy(), 64), act, case["eps"], 56, order)[:, :56]
        assert R.rel_err(h, case["ref"][EMUL_ROWS].numpy()) <= R.F32_BAR
