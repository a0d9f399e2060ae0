"""References and case builders of tests/test_gpu_bf16_mlp_exact.py: the bf16 fused MLP forward on the whole-wave kernel
(hgnn_mlp_forward_bf16, entry "bf16") and on the feature-split kernel (hgnn_mlp_forward_bf16_split, "bf16_split").
tests/test_bf16_mlp_ref.py proves everything here on the CPU.

1. SELECTOR NETWORKS -- expected bf16 bits known without any device arithmetic although every layer has a LayerNorm.
   Layer 1: weights in {-1, 0, +1}.  Every segment has one OFFSET column (weight column all ones, input mu in {-1, 0})
   and C >= width / 16 SIGN columns (weight column S[:, c], +-1, exactly half +1); row r puts its amplitude
   alpha in {1, 2, 4} into sign column c(r) of EVERY segment, so z = m_r + a_r S[:, c(r)] with a_r the sum of the
   segments' amplitudes and m_r = 1 (the bias) + the offsets, |m_r| <= a_r.  The other columns are fillers: non-zero
   inputs under zero weights, +-1 weights under zero inputs.  A gathered table row t has c = t mod C: the neighbouring
   table row selects another sign column.
   (A row's amplitude is thus a sum of one to three values of {1, 2, 4} -- every segment has to matter to the row, or a
   mis-gathered segment would go unseen -- and the offset stays within the amplitude: a mean off by 2^-12 relative then
   moves the normalised value by no more than 2^-12.)
   LayerNorm of a balanced two-valued row is +-1 up to rstd's relative error; gamma, beta are integers from families
   that keep every pre-activation at least 2 away from zero and every value that is kept well inside its bf16 rounding
   interval (``_margin`` asserts 2x room for: eps <= 1e-3, mean and rstd each off by a relative 2^-12):
       ReLU  A: gamma = +-6, beta in {11, 12, 13}     -> hidden in {5..7} / {17..19}
             B: gamma = +-g, g in {7..11}, beta = 12 - g -> hidden in {0, 12}
       none  gamma = +-6, beta in {0, +-11, +-12, +-13}
   so the two hidden values of a slot always differ by D = 12.  Layers 2 and 3: ONE +-1 per weight row -- output j reads
   hidden slot pi(j) with sign sigma_j -- and the bias that centres it: z_j = M_l + 6 v_j xhat[pi(j)].  The slots come
   in pairs of opposite sign pattern and a pair is selected (with one v) or dropped as a whole, so the row stays
   balanced and two-valued.  The output adds integer skip rows, 64 <= |skip| <= 200: |out| <= 256, an integer.
   ``expected_bits`` evaluates this in integers (and asserts the structure); ``layer_f32`` is the float32 emulation of
   one layer with either statistics scheme and perturbed statistics; ``forward_f64`` the float64 definition (used for mutants,
   whose rows are no longer two-valued).

2. integer-grid cases for the split kernel's save_pre[0] dump (``pre_case``, ``pre_ref_bits``).

3./4. random LayerNorm + GELU networks (``rand_case``) and the float64 mirror with the KERNELS' GELU
   x sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3) (``kernel_gelu``: swaps ln_ref.act64 for the block).
"""
import contextlib
import math

import numpy as np
import torch

import gemm_ref as G
import ln_ref as R
import rows_ref

ACT_NONE, ACT_GELU, ACT_TANH, ACT_RELU = R.ACT_NONE, R.ACT_GELU, R.ACT_TANH, R.ACT_RELU
POISON16 = 0x7FC1                 # test_gpu_rows_exact.POISON16
D_HID = 12                        # h(+1) - h(-1) of every hidden slot, in absolute value
A_HID = D_HID // 2                # amplitude of the pre-LayerNorm rows of layers 2 and 3
PERT = 2.0 ** -12                 # relative perturbation of mean and of rstd the expected bits must survive
EPS_MAX = 1e-3


# ---------------------------------------------------------------------------------------------------- bf16 helpers
def bits_of(t: torch.Tensor) -> torch.Tensor:
    """int16 bf16 patterns of float values, rounded once to nearest even"""
    return rows_ref.bf16_bits_rne(t.float())


def _tie_room(v: np.ndarray) -> np.ndarray:
    """distance from the bf16-exact values v to their nearest rounding tie (half an ulp on the tighter side)"""
    a = np.abs(v.astype(np.float64))
    out = np.full(a.shape, np.inf)
    nz = a > 0
    e = np.floor(np.log2(a[nz]))
    ulp = 2.0 ** (e - 7)
    out[nz] = np.where(a[nz] == 2.0 ** e, ulp / 4, ulp / 2)
    return out


def _margin(y, gamma_abs, a_min, what, relu=False):
    """every pre-activation y = gamma xhat + beta (an integer) keeps >= 2x room to zero and to its bf16 ties for an
    xhat off by (2 PERT + eps / (2 a^2)) relative"""
    err = np.asarray(gamma_abs, np.float64) * (2 * PERT + EPS_MAX / (2.0 * a_min * a_min))
    room = np.minimum(_tie_room(y), np.abs(y))
    if relu:                                   # a negative pre-activation only has to stay negative
        room = np.where(y < 0, np.abs(y), room)
    assert np.all(np.abs(y) >= 0.5) and np.all(room >= 2 * err), what


# ------------------------------------------------------------------------------------------- 1. selector networks
def _ln_params(n, act, rng, last):
    """integer gamma, beta of one layer from the families of the module docstring -> (gamma, beta, h_plus, h_minus)"""
    u = rng.choice([-1, 1], n)
    if act == ACT_RELU:
        typ_b = rng.random(n) < 0.5
        g = np.where(typ_b, rng.integers(7, 12, n), A_HID)
        beta = np.where(typ_b, D_HID - g, rng.integers(11, 14, n))
    else:
        g = np.full(n, A_HID)
        beta = rng.choice([0, 11, 12, 13, -11, -12, -13], n)
    gamma = u * g
    f = (lambda y: np.maximum(y, 0)) if act == ACT_RELU else (lambda y: y)
    hp, hm = f(gamma + beta), f(-gamma + beta)
    assert last or np.all(hp - hm == u * D_HID)
    return gamma, beta, hp, hm


def selector_case(widths, M, nseg, acts, seed, gathered=None, k_tab=3):
    """One exact case of a len(widths) - 1 layer net widths[0] -> ...; widths[0] = nseg * segment width.
    ``gathered``: per segment, whether it is a gathered table (default: all but the last).  Returns a dict:
    segments [(table, index or None)], x, layers [(W, b, gamma, beta, act)] (float32 tensors), skip, C, meta."""
    rng = np.random.default_rng(seed)
    K, n_layers = widths[0], len(widths) - 1
    assert K % nseg == 0
    sw, H = K // nseg, widths[1]
    gathered = [s < nseg - 1 for s in range(nseg)] if gathered is None else list(gathered)
    C = min(sw - 1, max(H // 16, 8))
    assert C >= H // 16, "fewer sign columns than 16-feature tiles"
    n_tab = C * k_tab
    # ---- layer 1 weights: pairs of features with opposite sign pattern
    match = rng.permutation(H).reshape(-1, 2)
    S = np.zeros((H, C), np.int64)
    S[match[:, 0]] = rng.choice([-1, 1], (H // 2, C))
    S[match[:, 1]] = -S[match[:, 0]]
    W1 = np.zeros((H, K), np.int64)
    c_of_row = rng.permutation(C)[np.arange(M) % C]
    segments, a_row, m_row = [], np.zeros(M, np.int64), np.ones(M, np.int64)
    for s in range(nseg):
        pos = rng.permutation(sw)
        off_col, sign_cols, rest = pos[0], pos[1:1 + C], pos[1 + C:]
        fill_x, fill_w = rest[:len(rest) // 2], rest[len(rest) // 2:]
        W1[:, s * sw + off_col] = 1
        W1[:, s * sw + sign_cols] = S
        W1[:, s * sw + fill_w] = rng.choice([-1, 1], (H, len(fill_w)))
        rows = n_tab if gathered[s] else M
        c_tab = (np.arange(rows) % C) if gathered[s] else c_of_row
        alpha = rng.choice([1, 2, 4], rows)
        mu = rng.choice([-1, 0], rows)
        t = np.zeros((rows, sw), np.int64)
        t[:, off_col] = mu
        t[np.arange(rows), sign_cols[c_tab]] = alpha
        t[:, fill_x] = rng.integers(-8, 9, (rows, len(fill_x)))
        if gathered[s]:
            idx = c_of_row + C * rng.integers(0, k_tab, M)
            a_row, m_row = a_row + alpha[idx], m_row + mu[idx]
            segments.append((torch.from_numpy(t).float(), torch.from_numpy(idx).to(torch.int64)))
        else:
            a_row, m_row = a_row + alpha, m_row + mu
            segments.append((torch.from_numpy(t).float(), None))
    assert np.all(np.abs(m_row) <= a_row)
    layers = []
    gm, bt, hp, hm = _ln_params(H, acts[0], rng, n_layers == 1)
    _margin(np.concatenate([gm + bt, -gm + bt]), np.abs(np.concatenate([gm, gm])), 1.0, "layer 1", acts[0] == ACT_RELU)
    layers.append([W1, np.ones(H, np.int64), gm, bt, acts[0]])
    pairs = match
    meta = dict(pairs=[match], perm=[None])
    for l in range(1, n_layers):
        n_in, n_out = widths[l], widths[l + 1]
        assert n_out % 2 == 0 and n_out <= n_in
        u_prev = np.sign(gm)
        chosen = pairs[rng.permutation(len(pairs))[:n_out // 2]]
        posn = rng.permutation(n_out).reshape(-1, 2)
        v = rng.choice([-1, 1], n_out // 2)
        pi, vj = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64)
        pi[posn[:, 0]], pi[posn[:, 1]] = chosen[:, 0], chosen[:, 1]
        vj[posn[:, 0]] = vj[posn[:, 1]] = v
        sigma = u_prev[pi] * vj
        assert np.all((hp + hm) % 2 == 0)
        M_l = int(rng.integers(-A_HID, A_HID + 1))
        W = np.zeros((n_out, n_in), np.int64)
        W[np.arange(n_out), pi] = sigma
        b = M_l - sigma * (hp[pi] + hm[pi]) // 2
        gm, bt, hp, hm = _ln_params(n_out, acts[l], rng, l == n_layers - 1)
        _margin(np.concatenate([gm + bt, -gm + bt]), np.abs(np.concatenate([gm, gm])), float(A_HID), f"layer {l + 1}",
                acts[l] == ACT_RELU)
        layers.append([W, b, gm, bt, acts[l]])
        pairs = posn
        meta["pairs"].append(posn)
        meta["perm"].append(pi)
    mag = rng.integers(64, 201, (M, widths[-1]))
    skip = mag * rng.choice([-1, 1], (M, widths[-1]))
    y_last = np.concatenate([hp, hm])                         # the activated last layer: out = that + skip
    lo = 64 - np.abs(y_last).max()
    assert lo >= 32 and 200 + np.abs(y_last).max() <= 256
    _margin(np.array([32.0]), np.abs(gm).max(), 1.0 if n_layers == 1 else float(A_HID), "output")   # the tightest value
    f32 = lambda a: torch.from_numpy(np.asarray(a)).float()   # noqa: E731
    layers = [(f32(W), f32(b), f32(g), f32(bb), act) for W, b, g, bb, act in layers]
    x = torch.cat([t if i is None else t[i] for t, i in segments], dim=1)
    return dict(segments=segments, x=x, layers=layers, skip=f32(skip), C=C, c_of_row=c_of_row, a_row=a_row,
                m_row=m_row, widths=list(widths), meta=meta, M=M)


def exact_layers(case):
    """per layer (z, gamma, beta, act, skip or None, bits): the pre-LayerNorm rows (float64 integers) and the int16
    bf16 patterns of the layer's output, in integer arithmetic: every pre-LayerNorm row is asserted balanced and
    two-valued, its normalised value is the SIGN of (z - mean), everything after it an integer"""
    h = case["x"].double()
    n = len(case["layers"])
    out = []
    for i, (W, b, gm, bt, act) in enumerate(case["layers"]):
        z = h @ W.double().t() + b.double()
        assert torch.equal(z, z.round())
        mean = z.mean(dim=1, keepdim=True)
        dev = z - mean
        amp = dev.abs()
        assert torch.equal(amp, amp[:, :1].expand_as(amp)) and bool((amp > 0).all()), f"layer {i + 1}: not two-valued"
        assert bool((dev.sign().sum(dim=1) == 0).all()), f"layer {i + 1}: not balanced"
        assert float(mean.abs().max()) <= float(amp.min()) or i > 0 and float(mean.abs().max()) <= A_HID
        y = dev.sign() * gm.double() + bt.double()
        assert act in (ACT_RELU, ACT_NONE)
        h = torch.clamp_min(y, 0.0) if act == ACT_RELU else y
        sk = case["skip"] if i == n - 1 else None
        if sk is not None:
            h = h + sk.double()
        assert torch.equal(h, h.round()) and float(h.abs().max()) <= 256
        out.append((z, gm, bt, act, sk, G.round_bf16_bits(h)))
    return out


def expected_bits(case) -> torch.Tensor:
    """int16 bf16 patterns of the output, known without floating-point arithmetic (``exact_layers``)"""
    return exact_layers(case)[-1][-1]


def _sum32(v):
    """float32 row sums, one value after the other"""
    return np.cumsum(v.astype(np.float32), axis=1, dtype=np.float32)[:, -1]


def stats_f32(z, eps, scheme, nw=4):
    """(mean, rstd) of float32 rows z in float32: ``onepass`` q / n - mean^2 (whole-wave kernel) or ``pooled`` --
    wave-local mean and centred M2 over each of nw feature slices, pooled (feature-split kernel)"""
    f = np.float32
    n = f(z.shape[1])
    if scheme == "onepass":
        mean = _sum32(z) / n
        q = _sum32((z.astype(np.float64) ** 2).astype(f)) / n
        var = np.maximum((q.astype(np.float64) - mean.astype(np.float64) ** 2).astype(f), f(0))
    else:
        parts = np.split(z, nw, axis=1)
        n_w = f(parts[0].shape[1])
        mw = np.stack([_sum32(p) / n_w for p in parts], axis=1)
        m2 = np.stack([_sum32(((p - mw[:, i:i + 1]).astype(f)) ** 2) for i, p in enumerate(parts)], axis=1)
        mean = _sum32(mw) / f(nw)
        dm = (mw - mean[:, None]).astype(f)
        var = ((_sum32(dm * dm) * n_w + _sum32(m2)) / n).astype(f)
    rstd = (f(1) / np.sqrt(var + f(eps), dtype=f)).astype(f)
    return mean.astype(f), rstd


def layer_f32(z, gm, bt, act, skip, eps, scheme, nw=4, dmean=0.0, drstd=0.0) -> torch.Tensor:
    """LayerNorm -> act (-> + skip) -> bf16 of the rows z in float32 with emulated statistics, mean and rstd each
    scaled by (1 + d) -> int16 patterns"""
    f = np.float32
    z = z.numpy().astype(f)
    mean, rstd = stats_f32(z, eps, scheme, nw)
    mean, rstd = (mean * f(1 + dmean)).astype(f), (rstd * f(1 + drstd)).astype(f)
    if scheme == "onepass":      # fma(z, rstd, -mean rstd)
        xh = (z.astype(np.float64) * rstd[:, None] - (mean * rstd).astype(f)[:, None]).astype(f)
    else:
        xh = ((z - mean[:, None]).astype(f) * rstd[:, None]).astype(f)
    y = (xh.astype(np.float64) * gm.numpy() + bt.numpy()).astype(f)
    a = np.maximum(y, f(0)) if act == ACT_RELU else y
    if skip is not None:
        a = (a + skip.numpy()).astype(f)
    return bits_of(torch.from_numpy(a))


def forward_f64(x, layers, skip, eps=1e-5) -> torch.Tensor:
    """the float64 definition with the documented roundings, the final one included -> int16 patterns"""
    out, _ = R.net_forward(x, layers, eps, skip, bf16=True)
    return bits_of(out)


def mutants(case):
    """name -> int16 output patterns of a subtly wrong kernel (float64 LayerNorm: a mutated row need not be two-valued).
    A mutant that does not apply to the case (no gathered segment, one row, one layer) is left out."""
    x, layers, skip, M = case["x"], case["layers"], case["skip"], case["M"]
    out = {}
    if len(layers) > 1:                       # two hidden slots swapped: two columns of W_2 that are both read
        W2 = layers[1][0]
        used = torch.nonzero(W2.abs().sum(0))[:, 0]
        f0, f1 = int(used[0]), int(used[len(used) // 2])
        Wm = W2.clone()
        Wm[:, [f0, f1]] = W2[:, [f1, f0]]
        out["hidden_slots_swapped"] = forward_f64(x, [layers[0], (Wm,) + tuple(layers[1][1:])] + layers[2:], skip)
    for l in range(len(layers)):              # tile t of layer l reads the gamma / beta of tile t + 1
        W, b, gm, bt, act = layers[l]
        t = (gm.numel() // 16) // 2 - 1
        g2, b2 = gm.clone(), bt.clone()
        g2[16 * t:16 * t + 16], b2[16 * t:16 * t + 16] = gm[16 * t + 16:16 * t + 32], bt[16 * t + 16:16 * t + 32]
        out[f"ln_offset_layer{l + 1}"] = forward_f64(x, layers[:l] + [(W, b, g2, b2, act)] + layers[l + 1:], skip)
    for s, (tab, idx) in enumerate(case["segments"]):
        if idx is None:
            continue
        i2 = idx.clone()
        r = M - 1
        i2[r] = idx[r] - 1 if idx[r] > 0 else idx[r] + 1
        segs = list(case["segments"])
        segs[s] = (tab, i2)
        xm = torch.cat([t if i is None else t[i] for t, i in segs], dim=1)
        out[f"gather_off_by_one_seg{s}"] = forward_f64(xm, layers, skip)
    if M > 1:
        sk = skip.clone()
        sk[M - 1] = skip[M - 2]
        out["skip_from_previous_row"] = forward_f64(x, layers, sk)
    unwritten = expected_bits(case).clone()
    unwritten[min(M, 64) - 1] = POISON16
    out["tile_last_row_unwritten"] = unwritten
    return out


# configurations of section 1: name -> (entry, widths without K, segment width, nseg).  The activation pairs of the
# runtime-switch instantiations: (hidden, output)
def _cfg(entry, tail, sw, nseg):
    return dict(entry=entry, widths=[sw * nseg] + tail, nseg=nseg)


EXACT_CONFIGS = {
    "wave_L32x2": _cfg("bf16", [64, 32], 32, 1), "wave_L32x3": _cfg("bf16", [64, 64, 32], 32, 3),
    "wave_L64x2": _cfg("bf16", [128, 64], 32, 2), "wave_L64x3": _cfg("bf16", [128, 128, 64], 64, 1),
    "wave_L128x2": _cfg("bf16", [256, 128], 32, 3), "wave_L128x3": _cfg("bf16", [256, 256, 128], 64, 2),
    "wave_L256x2": _cfg("bf16", [512, 256], 64, 2), "wave_L256x3": _cfg("bf16", [512, 512, 256], 64, 3),
    "split_L128x2": _cfg("bf16_split", [256, 128], 128, 3), "split_L128x3": _cfg("bf16_split", [256, 256, 128], 128, 2),
    "split_L256x2": _cfg("bf16_split", [512, 256], 128, 2), "split_L256x3": _cfg("bf16_split", [512, 512, 256], 128, 3),
    "split_L512x2": _cfg("bf16_split", [1024, 512], 128, 3), "split_L512x3": _cfg("bf16_split", [1024, 1024, 512], 256, 2),
    "split_o256": _cfg("bf16_split", [256], 128, 2), "split_o512": _cfg("bf16_split", [512], 128, 3),
    "split_o1024": _cfg("bf16_split", [1024], 128, 1),
}
EXACT_M = (1, 63, 65, 193)
EXACT_ACTS = ("relu_none", "none_relu")


def exact_ms(cfg):
    """the row counts of a configuration: the 64-row tile's edges and three tiles + one row; where a whole-wave
    workgroup holds 128 rows (EG = 2: first layer >= 256 wide) its edge too"""
    c = EXACT_CONFIGS[cfg]
    return EXACT_M + ((127, 129) if c["entry"] == "bf16" and c["widths"][1] >= 256 else ())


def exact_case(cfg, M, acts):
    c = EXACT_CONFIGS[cfg]
    n = len(c["widths"]) - 1
    hid, last = (ACT_RELU, ACT_NONE) if acts == "relu_none" else (ACT_NONE, ACT_RELU)
    seed = 7919 * sorted(EXACT_CONFIGS).index(cfg) + 31 * M + EXACT_ACTS.index(acts)
    k_tab = 1 if c["widths"][1] >= 512 else 3
    return selector_case(c["widths"], M, c["nseg"], [hid] * (n - 1) + [last], seed, k_tab=k_tab)


# ------------------------------------------------------------------------------- 2. layer-1 sums (save_pre[0])
# name -> (layer widths after K, segment widths, gathered?, pre-projected path forced)
PRE_CONFIGS = {
    "L128_1seg": ([256, 128], [128], [False], False),
    "L128_2seg_g": ([256, 128], [128, 256], [True, False], False),
    "L128_3seg_g": ([256, 128], [256, 128, 128], [True, True, False], False),
    "L256_3seg_direct": ([512, 256], [128, 128, 256], [False, False, False], False),
    "L256_2seg_pre": ([512, 256], [256, 128], [True, False], True),
    "L128_3seg_pre": ([256, 256, 128], [128, 128, 128], [True, True, False], True),
    "L512_3seg_pre": ([1024, 512], [128, 256, 128], [True, True, False], True),
    "L512_2seg_g": ([1024, 1024, 512], [256, 256], [False, True], False),
    "o256": ([256], [128, 128], [True, False], False),
    "o512": ([512], [256], [False], False),
    "o1024": ([1024], [128, 256, 128], [True, False, True], False),
}
PRE_M = 193
PRE_TAB = 41                      # 4 x 41 <= 193: small enough for fused._projected_segments


def pre_case(name):
    """integer-grid inputs, weights and bias (gemm_ref.small): every partial sum of b + W concat(x) is an integer
    below 2^22"""
    tail, sws, gathered, pre = PRE_CONFIGS[name]
    seed = 1009 * sorted(PRE_CONFIGS).index(name)
    K = sum(sws)
    G.assert_exact(K + 1, G.SMALL_MAX * G.SMALL_MAX)
    g = torch.Generator().manual_seed(seed)
    segments = []
    for s, (sw, ga) in enumerate(zip(sws, gathered)):
        if ga:
            segments.append((G.small(PRE_TAB, sw, seed + 10 + s), torch.randint(0, PRE_TAB, (PRE_M,), generator=g)))
        else:
            segments.append((G.small(PRE_M, sw, seed + 10 + s), None))
    W = G.small(tail[0], K, seed + 1)
    b = G.small(tail[0], 1, seed + 2)[:, 0].contiguous()
    return dict(segments=segments, W=W, b=b, tail=tail, pre=pre, sws=sws, name=name)


def pre_ref_bits(case, projected=()) -> torch.Tensor:
    """b + W concat(x) in float64, rounded ONCE to bf16 (int16 patterns).  ``projected``: the segments that enter as
    P = bf16(table W_s^T) rows (the pre-projected path rounds each P row once, to an integer)"""
    z = case["b"].double().expand(PRE_M, -1).clone()
    col = 0
    for s, ((tab, idx), sw) in enumerate(zip(case["segments"], case["sws"])):
        Ws = case["W"][:, col:col + sw].double()
        col += sw
        if s in projected:
            P = G.bits_to_float(G.round_bf16_bits(tab.double() @ Ws.t())).double()
            z = z + P[idx]
        else:
            z = z + (tab if idx is None else tab[idx]).double() @ Ws.t()
    return G.round_bf16_bits(z)


# --------------------------------------------------------------------- 3. / 4. random networks and the mirror
def gelu_kernel64(y):
    """the bf16 kernels' GELU in float64: x sigmoid(2u), u = sqrt(2 / pi) (x + 0.044715 x^3)"""
    u = math.sqrt(2.0 / math.pi) * (y + 0.044715 * y ** 3)
    return y * torch.sigmoid(2.0 * u)


@contextlib.contextmanager
def kernel_gelu():
    """inside the block ln_ref's float64 forward and float32 emulations evaluate GELU in the kernels' form"""
    old = R.act64
    R.act64 = lambda y, act: gelu_kernel64(y) if act == ACT_GELU else old(y, act)
    try:
        yield
    finally:
        R.act64 = old


def rand_case(widths, M, nseg, skip, seed, n_tab=97, acts=None):
    """a random bf16 case in ln_ref.make_case's distribution without its float64 forward (large M): -> dict(segments,
    x, layers, skip, eps, bf16, group, widths)"""
    g = torch.Generator().manual_seed(seed)
    K, n = widths[0], len(widths) - 1
    assert K % nseg == 0
    sw = K // nseg
    cast = lambda t: t.bfloat16().float()   # noqa: E731
    table = cast(torch.randn(n_tab, sw, generator=g))
    direct = cast(torch.randn(M, sw, generator=g))
    segments = [(table, torch.randint(0, n_tab, (M,), generator=g)) for _ in range(nseg - 1)] + [(direct, None)]
    if acts is None:
        acts = [ACT_GELU] * (n - 1) + [ACT_TANH if n == 2 else ACT_GELU]
    layers = []
    for l in range(n):
        layers.append((cast(torch.randn(widths[l + 1], widths[l], generator=g) / widths[l] ** 0.5),
                       0.2 * torch.randn(widths[l + 1], generator=g), 1 + 0.2 * torch.randn(widths[l + 1], generator=g),
                       0.2 * torch.randn(widths[l + 1], generator=g), acts[l]))
    sk = cast(torch.randn(M, widths[-1], generator=g)) if skip else None
    x = torch.cat([t if i is None else t[i] for t, i in segments], dim=1)
    return dict(segments=segments, x=x, layers=layers, skip=sk, eps=1e-5, bf16=True, group=R.GROUP_MATRIX,
                widths=list(widths), M=M)


def mirror(case) -> torch.Tensor:
    """float64 mirror (hidden rows rounded to bf16, the last value unrounded) with the kernels' GELU"""
    with kernel_gelu():
        return R.net_forward(case["x"], case["layers"], case["eps"], case["skip"], bf16=True)[0]


def boundary_rows(M, tile):
    """row 0, the rows either side of every 16 / 32 / 64 / 128-row boundary inside the first and the last ``tile``-row
    tile, the last row"""
    rows = {0, M - 1}
    for base in (0, (M - 1) // tile * tile):
        for step in (16, 32, 64, 128):
            for b in range(base, base + tile + 1, step):
                rows.update(r for r in (b - 1, b) if 0 <= r < M)
    return sorted(rows)


# per-element bar of section 4:  |out - ref| <= C_BAR 2^-8 |ref| + D_BAR max|ref|
def excess(out, ref):
    """worst over the elements of (|out - ref| - 2^-8 |ref|) / max|ref|: what an element is off beyond one bf16 ulp of
    its own magnitude, relative to the largest reference value"""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    return float(((np.abs(out - ref) - R.BF16_ULP * np.abs(ref)) / max(np.abs(ref).max(), 1e-30)).max())


def bar_ratio(out, ref, c, d):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(out - ref) / (c * R.BF16_ULP * np.abs(ref) + d * max(np.abs(ref).max(), 1e-30))).max())


# C_BAR: one bf16 ulp of the element itself.  D_BAR: twice the worst excess of the float32 emulation over that ulp on the
# cases below, 1.149e-3 (tests/test_bf16_mlp_ref.py::test_emulation_figure_behind_the_bar measures it and holds D_BAR to it)
C_BAR, D_BAR = 1.0, 2.3e-3
BAR_M_FULL = (1, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 193)
BAR_M_SUB = (1, 63, 65, 193)
# name -> (entry, widths after K, segment width).  The narrowest latent of each kernel runs BAR_M_FULL
BAR_CONFIGS = {
    "wave_L32x2": ("bf16", [64, 32], 32), "wave_L32x3": ("bf16", [64, 64, 32], 32),
    "wave_L64x2": ("bf16", [128, 64], 64), "wave_L64x3": ("bf16", [128, 128, 64], 64),
    "wave_L128x2": ("bf16", [256, 128], 128), "wave_L128x3": ("bf16", [256, 256, 128], 128),
    "wave_L256x2": ("bf16", [512, 256], 256), "wave_L256x3": ("bf16", [512, 512, 256], 256),
    "split_L128x2": ("bf16_split", [256, 128], 128), "split_L128x3": ("bf16_split", [256, 256, 128], 128),
    "split_L256x2": ("bf16_split", [512, 256], 256), "split_L256x3": ("bf16_split", [512, 512, 256], 256),
    "split_L512x2": ("bf16_split", [1024, 512], 512), "split_L512x3": ("bf16_split", [1024, 1024, 512], 512),
    "split_o256": ("bf16_split", [256], 256), "split_o512": ("bf16_split", [512], 512),
    "split_o1024": ("bf16_split", [1024], 1024),
}


def bar_ms(cfg):
    entry, tail, _ = BAR_CONFIGS[cfg]
    if cfg.startswith(("wave_L32", "split_L128")):
        return BAR_M_FULL
    return BAR_M_SUB + ((127, 129) if entry == "bf16" and tail[0] >= 256 else ())


def bar_case(cfg, M):
    """segments cycle 1..3 and the skip alternates with the position of M in the configuration's list; the segment
    width equals the output width so that a skip always fits"""
    entry, tail, sw = BAR_CONFIGS[cfg]
    i = bar_ms(cfg).index(M) + sorted(BAR_CONFIGS).index(cfg)
    nseg, skip = 1 + i % 3, i % 2 == 0
    return rand_case([sw * nseg] + tail, M, nseg, skip, seed=100003 * sorted(BAR_CONFIGS).index(cfg) + M,
                     n_tab=max(2, min(97, M)))
