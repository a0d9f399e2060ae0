"""The LayerNorm algebra of hgnn_mlp_forward_f32_split3_padded, proved with the float32 emulations of tests/ln_ref.py
(in the manner of tests/test_mlp_padded_ref.py; no device involved).

The 64-row split-bf16 kernel shares a layer's stored features among NW = 4 (P = 128) or 8 (P = 256) waves, wave w owning
the stored features [w S, (w + 1) S).  On zero-padded parameters only the first ``real`` of them exist, so the waves hold
UNEQUAL counts n_w = clamp(real - w S, 0, S) -- 64, 64, 64, 0 at h = 192, 32, 32, 8, 0 at o = 72 -- and

  * the COUNT-WEIGHTED pooling   mean = sum n_w m_w / n,   M2 = sum M2_w + sum n_w (m_w - mean)^2,   var = M2 / n
    (each wave centres its own real features on its own mean, padded quads selected out of both passes, a wave without a
    real feature contributing m_w = M2_w = 0) equals the float64 definition of the UNPADDED network within HALF of the
    fp32 bar on every ``ln_ref.CASES`` entry, in both summation orders, with the GEMMs in the matrix-pipe grouping;
  * the EQUAL-count formula of the native kernel (mean = avg m_w, M2 = sum M2_w + S sum (m_w - mean)^2 over all stored
    features, n = NW S) fails every one of those cases: it normalises over the zeros too;
  * padded accumulators and padded activations are exactly 0.

Not in the emulation: the ~2^-16 truncation of the split products (the device test carries the full bar for that).
"""
import numpy as np
import pytest
import torch

import ln_ref as R
from test_ln_ref import EMUL_ROWS, ORDERS, _carries_elem_bar, _figures

# widths -> (2P, P, NW) of the instantiation they run on
SHAPES = {
    "L96x2": dict(widths=[288, 192, 96], stored=(256, 128, 4)),
    "L72x2": dict(widths=[216, 144, 72], stored=(256, 128, 4)),
    "L72x3": dict(widths=[216, 144, 144, 72], stored=(256, 128, 4)),
    "L144x3": dict(widths=[432, 288, 288, 144], stored=(512, 256, 8)),
    "L120x2": dict(widths=[360, 240, 120], stored=(256, 128, 4)),
    "L192x2": dict(widths=[576, 384, 192], stored=(512, 256, 8)),
    "L64h192": dict(widths=[192, 192, 64], stored=(256, 128, 4)),
}


def _pad(t, rows, cols=None):
    out = np.zeros((rows,) if t.ndim == 1 else (rows, cols if cols is not None else t.shape[1]), np.float32)
    if t.ndim == 1:
        out[:t.shape[0]] = t
    else:
        out[:t.shape[0], :t.shape[1]] = t
    return out


def wave_counts(real, stored, nw):
    """n_w = clamp(real - w S, 0, S) with S = stored / nw"""
    S = stored // nw
    return [min(max(real - w * S, 0), S) for w in range(nw)]


def _lane_sum32(v, order):
    """ln_ref._seq_sum32 for any row length that is a multiple of 4 (a wave's real slice: 8, 16, 24, ... features)"""
    m, n = v.shape
    c = 16 if n % 16 == 0 else (8 if n % 8 == 0 else 4)
    p = v.reshape(m, n // c, c)
    s = np.zeros((m, n // c), np.float32)
    for k in (range(c) if order == "fwd" else range(c - 1, -1, -1)):
        s = s + p[:, :, k]
    while s.shape[1] > 1:
        if s.shape[1] % 2:
            s = np.concatenate([s, np.zeros((m, 1), np.float32)], axis=1)
        s = s[:, 0::2] + s[:, 1::2]
    return s[:, 0]


def ln_act_pooled(z, gamma, beta, act, eps, n_real, nw, order, weighted=True):
    """float32 LayerNorm + activation of the STORED rows z [M, NW S] the way the feature-split kernel forms them.
    ``weighted``: each wave over its n_w real features, pooled with the counts, n = n_real (the PAD kernels);
    otherwise each wave over its S stored features, pooled with equal counts, n = NW S (the native kernel)"""
    f = np.float32
    z = np.asarray(z, f)
    M, stored = z.shape
    S = stored // nw
    counts = wave_counts(n_real, stored, nw) if weighted else [S] * nw
    mw = np.zeros((M, nw), f)
    m2 = np.zeros((M, nw), f)
    for w, c in enumerate(counts):
        if c == 0:
            continue                                  # m_w = M2_w = 0
        part = z[:, w * S:w * S + c]
        mw[:, w] = _lane_sum32(part, order) / f(c)
        d = part - mw[:, w:w + 1]
        m2[:, w] = _lane_sum32(d * d, order)
    n = f(sum(counts))
    cw = np.asarray(counts, f)[None, :]
    ws = list(range(nw)) if order == "fwd" else list(range(nw - 1, -1, -1))
    s = np.zeros(M, f)
    q = np.zeros(M, f)
    for w in ws:
        s = s + cw[0, w] * mw[:, w]
        q = q + m2[:, w]
    mean = s / n
    c2 = np.zeros(M, f)
    for w in ws:
        d = mw[:, w] - mean
        c2 = c2 + (cw[0, w] * d) * d
    var = (c2 + q) / n
    rstd = f(1.0) / np.sqrt(var + f(eps), dtype=f)
    xh = (z - mean[:, None]) * rstd[:, None]
    y = (xh.astype(np.float64) * np.asarray(gamma, f).astype(np.float64) + np.asarray(beta, f).astype(np.float64)).astype(f)
    return R.act64(torch.from_numpy(y.astype(np.float64)), act).numpy().astype(f)


def emul_padded(case, stored, order, rows, weighted=True):
    """the padded network of a case through the emulation: hidden layers 2P wide, the last P wide, W[l >= 1] with 2P
    columns, every padded entry (ln_w included) zero; the result at the real width (+ skip)"""
    hid, last, nw = stored
    n = len(case["layers"])
    h = case["x"][rows].numpy()
    for l, (W, b, gm, bt, act) in enumerate(case["layers"]):
        rows_l = last if l == n - 1 else hid
        real = int(W.shape[0])
        z = R.emul_gemm(h, _pad(W.numpy(), rows_l, hid if l > 0 else None), _pad(b.numpy(), rows_l), order, case["group"])
        assert not z[:, real:].any(), "a padded accumulator is not exactly 0"
        h = ln_act_pooled(z, _pad(gm.numpy(), rows_l), _pad(bt.numpy(), rows_l), act, case["eps"], real, nw, order, weighted)
        assert not h[:, real:].any(), "a padded activation is not exactly 0"
    out = h[:, :int(case["layers"][-1][0].shape[0])]
    return out if case["skip"] is None else out + case["skip"][rows].numpy()


def test_wave_counts_cover_the_layouts_the_kernel_meets():
    assert wave_counts(192, 256, 4) == [64, 64, 64, 0]           # a wave with no real feature
    assert wave_counts(144, 256, 4) == [64, 64, 16, 0]           # a partly real slice: 16 of 64
    assert wave_counts(72, 128, 4) == [32, 32, 8, 0]             # 8 of 32
    assert wave_counts(88, 128, 4) == [32, 32, 24, 0]            # a multiple of 4 that is no multiple of 16
    assert wave_counts(288, 512, 8) == [64, 64, 64, 64, 32, 0, 0, 0]
    assert wave_counts(256, 256, 4) == [64] * 4 and wave_counts(256, 256, 8) == [32] * 8


def test_with_nothing_padded_the_weighted_pooling_is_the_native_one_bit_for_bit():
    """the counts are then the power of two S: scaling by them commutes with every rounding"""
    g = np.random.default_rng(5)
    z = (g.standard_normal((24, 256)) * 1.5 + 3.0).astype(np.float32)
    gm, bt = g.standard_normal(256).astype(np.float32), g.standard_normal(256).astype(np.float32)
    for nw in (4, 8):
        for order in ORDERS:
            a = ln_act_pooled(z, gm, bt, R.ACT_GELU, 1e-5, 256, nw, order, weighted=True)
            b = ln_act_pooled(z, gm, bt, R.ACT_GELU, 1e-5, 256, nw, order, weighted=False)
            assert np.array_equal(a, b)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_count_weighted_pooling_equals_the_unpadded_definition(shape):
    cfg = SHAPES[shape]
    lines = []
    for name in R.CASES:
        case = R.case_for(dict(widths=cfg["widths"]), name, matrix=True)
        for order in ORDERS:
            f = _figures(case, emul_padded(case, cfg["stored"], order, EMUL_ROWS))
            lines.append(f"{shape:8s} {name:11s} r={case['r']:<5g} weighted/{order}: " + " ".join(f"{k} {v:.1e}" for k, v in f.items()))
            assert f["rel"] <= 0.5 * R.F32_BAR, lines[-1]
            assert not _carries_elem_bar(case) or f["elem"] <= 0.5 * R.F32_BAR, lines[-1]
            assert f.get("const", 0.0) <= 0.5 * R.F32_BAR, lines[-1]
    print("\n" + "\n".join(lines))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_equal_count_formula_fails_on_padded_layouts(shape):
    """negative control: the native kernel's pooling on the same stored rows"""
    cfg = SHAPES[shape]
    lines = []
    for name in R.CASES:
        case = R.case_for(dict(widths=cfg["widths"]), name, matrix=True)
        for order in ORDERS:
            f = _figures(case, emul_padded(case, cfg["stored"], order, EMUL_ROWS, weighted=False))
            lines.append(f"{shape:8s} {name:11s} r={case['r']:<5g} equal/{order}: " + " ".join(f"{k} {v:.1e}" for k, v in f.items())
                         + "   (must fail)")
            assert f["rel"] > R.F32_BAR, lines[-1]
    print("\n" + "\n".join(lines))
