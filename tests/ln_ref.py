"""float64 definition of one fused-MLP layer  Linear -> LayerNorm -> act (-> + skip)  and of its backward, two float32
EMULATIONS of the same layer, and the conformance cases of tests/test_gpu_mlp_layernorm.py.

Definition (the reference's formulas, Modules/utils.py make_mlp on torch.nn): z = x W^T + b; mean and BIASED variance
over the features; xhat = (z - mean) / sqrt(var + eps) with eps INSIDE the square root; y = xhat gamma + beta;
a = act(y) with the erf GELU; out = a (+ skip).  Backward of a = act(LN(z)) for an upstream gradient g:
dy = g act'(y); dgamma = sum_rows dy xhat; dbeta = sum_rows dy; gg = dy gamma;
dz = rstd (gg - mean(gg) - xhat mean(gg xhat)); dbias = sum_rows dz.

bf16 kernels -- the documented rounding points: inputs and weights are bf16-exact when they arrive; the hidden
activations of a multi-layer launch are rounded to bf16 between its layers; the result is rounded once, after the
skip add.  ``net_forward(..., bf16=True)`` applies the hidden roundings and returns the UNROUNDED last value: the
bounds of the GPU file account for the one final rounding themselves.

Emulations (float32, used only to size and to prove the tests, tests/test_ln_ref.py):
  * the GEMM the way the kernels accumulate it: the accumulator starts at the BIAS and takes one fused multiply-add
    per k (``order`` "fwd" or "rev" in K and in the features) -- every step rounds at the magnitude of the offset row, which is the
    error a CORRECT kernel has on an offset row and what sizes r per shape (``r_eff``); the matrix-pipe kernels round
    once per group of products (``group``); row sums are a lane's 16 values in sequence, then a halving tree;
  * ``centred``: mean, then sum((z - mean)^2), then (z - mean) rstd; ``pooled``: the same from 8 waves' (mean, M2) pairs;
  * ``onepass_shift``: var = max(E[z^2] - mean^2, 0), then fma(z, rstd, -mean rstd);
  * ``eps_mode``: "inside" (the definition), "omit" (no eps at all), "default" (1e-5 whatever the module says).
"""
import math

import numpy as np
import torch

ACT_NONE, ACT_GELU, ACT_TANH, ACT_RELU = 0, 1, 2, 3          # hgnn_hip.h HGNN_ACT_*
ACT_CODE = {None: 0, "GELU": 1, "Tanh": 2, "ReLU": 3}
F32_BAR = 1e-4                                               # the project's fp32 parity bar
BF16_ULP = 2.0 ** -8                                         # round-to-nearest to 8 significant bits: <= 2^-9 relative
M_ROWS = 193                                                 # three 64-row tiles + one row

CASES = ("r0", "r16", "r64", "r256", "s-8_r0", "s-8_r64", "s+8_r0", "s+8_r64", "eps1e-3", "const_c0.5", "const_c256")


def parse_case(name):
    """-> dict(r, scale_exp, eps, const)"""
    c = dict(r=0.0, scale_exp=0, eps=1e-5, const=None)
    if name == "eps1e-3":
        c.update(eps=1e-3, scale_exp=-4)
        return c
    if name.startswith("const_c"):
        c["const"] = float(name[len("const_c"):])
        return c
    for part in name.split("_"):
        if part.startswith("s"):
            c["scale_exp"] = int(part[1:])
        elif part.startswith("r"):
            c["r"] = float(part[1:])
        else:
            raise ValueError(name)
    return c


# The offset a CORRECT kernel can carry.  The kernels' accumulators start at the bias (r sigma) and round at that magnitude
# on every accumulation step: one step per k in the exact fp32 kernel (a chain of fused multiply-adds, GROUP = 1); the
# matrix-pipe kernels (split-bf16 fp32, bf16) add the products of a 32-wide k-chunk in 1 to 4 instructions, each rounding
# the accumulator once -- modelled as one rounding per GROUP = 8 products.  After K / GROUP steps z is off by
# ~ 0.29 ulp(r sigma) sqrt(K / GROUP) = 3.4e-8 r sqrt(K / GROUP) sigma rms, ~4x that at the worst of 193 x N elements, and
# d out / d z is ~ 1 / sigma, so
#     element-wise error (denominator |ref| + rms(ref) ~ 1)   ~ 1.4e-7 r sqrt(K / GROUP)
#     normwise error     (denominator max |ref| ~ 3..5)        ~ 4e-8 r sqrt(K / GROUP)
# "At or below HALF of the 1e-4 bar" then means r sqrt(K / GROUP) <= 300 for the cases that carry the element-wise bar
# (nominal r <= 64) and <= 1000 for the normwise-only case r256.  The bf16 single-layer bound leaves 1e-4 max|ref| ~ 4e-4
# absolute to the value that is rounded (zero violations asked, not half): <= 2800.  K is the widest GEMM of the launch.
# A case's nominal r is lowered to the largest power of two inside these limits; tests/test_ln_ref.py PROVES every
# resulting (case, shape) with the `centred` emulation in both summation orders -- the limits come from the arithmetic
# above, never from a device result.  (const_cC: every row of layer 1 sits at offset C / sigma, so C is lowered like r.)
# Entries that are handed z directly (the row kernels, the backward layer) have no GEMM in front of the statistics and
# keep the nominal r.
R_ELEM_LIMIT, R_NORM_LIMIT, R_BF16_LIMIT = 300.0, 1000.0, 2800.0
# The bf16 TRAINING path dumps the pre-LayerNorm rows z in bf16 (a design property): a row at offset
# r sigma is stored to 2^-9 r sigma, so the backward's xhat is off by ~ r 2^-9 / sqrt(3) = r 1.1e-3 rms, ~4x that at the
# worst element, whatever the kernel does afterwards.  Half of BF16_GRAD = 3e-2 leaves r <= 1.5e-2 / 4.5e-3 ~ 3.3: the
# bf16 training round trip runs its r64 case at r = 2 (the fp32 round trips dump fp32 rows and follow r_eff).
R_BF16_TRAIN = 2.0
GROUP_EXACT, GROUP_MATRIX = 1, 8


def r_eff(nominal, K, bf16=False, group=GROUP_EXACT):
    """the offset a case runs with at GEMM width K (see above): min(nominal, largest power of two within the limit)"""
    if nominal <= 0:
        return nominal
    limit = R_BF16_LIMIT if bf16 else (R_ELEM_LIMIT if nominal <= 64 else R_NORM_LIMIT)
    cap = 2.0 ** math.floor(math.log2(limit / math.sqrt(K / group)))
    return min(float(nominal), cap)


def bf16_round(t):
    """float64 -> nearest bf16 (ties to even), returned as float64"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def act64(y, act):
    if act == ACT_GELU:
        return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
    if act == ACT_TANH:
        return torch.tanh(y)
    if act == ACT_RELU:
        return torch.clamp_min(y, 0.0)
    return y


def act_grad64(y, act):
    if act == ACT_GELU:
        return 0.5 * (1.0 + torch.erf(y / math.sqrt(2.0))) + y * torch.exp(-0.5 * y * y) / math.sqrt(2.0 * math.pi)
    if act == ACT_TANH:
        return 1.0 - torch.tanh(y) ** 2
    if act == ACT_RELU:
        return (y > 0).to(y.dtype)
    return torch.ones_like(y)


def ln_stats64(z, eps, n_real=None):
    zz = z if n_real is None else z[:, :n_real]
    mean = zz.mean(dim=1, keepdim=True)
    var = ((zz - mean) ** 2).mean(dim=1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + eps)


def ln_act_forward(z, gamma, beta, act, eps):
    """a = act(LayerNorm(z)) in float64"""
    z, gamma, beta = z.double(), gamma.double(), beta.double()
    mean, rstd = ln_stats64(z, eps)
    return act64((z - mean) * rstd * gamma + beta, act)


def ln_act_backward(z, g, gamma, beta, act, eps):
    """(dz, dgamma, dbeta, dbias) of a = act(LayerNorm(z)) for the upstream gradient g, float64"""
    z, g, gamma, beta = z.double(), g.double(), gamma.double(), beta.double()
    mean, rstd = ln_stats64(z, eps)
    xh = (z - mean) * rstd
    dy = g * act_grad64(xh * gamma + beta, act)
    gg = dy * gamma
    dz = rstd * (gg - gg.mean(dim=1, keepdim=True) - xh * (gg * xh).mean(dim=1, keepdim=True))
    return dz, (dy * xh).sum(0), dy.sum(0), dz.sum(0)


def layer_forward(x, W, b, gamma, beta, act, eps, skip=None):
    """one layer in float64 -> (out, z)"""
    z = x.double() @ W.double().t() + b.double()
    a = z if gamma is None else ln_act_forward(z, gamma, beta, act, eps)   # gamma None: a plain last Linear (score head)
    return (a if skip is None else a + skip.double()), z


def net_forward(x, layers, eps, skip=None, bf16=False):
    """layers: [(W, b, gamma, beta, act)] -> (out, [z_l]); bf16: hidden activations rounded between the layers"""
    h, zs = x.double(), []
    for i, (W, b, gm, bt, act) in enumerate(layers):
        last = i == len(layers) - 1
        h, z = layer_forward(h, W, b, gm, bt, act, eps, skip if last else None)
        zs.append(z)
        if bf16 and not last:
            h = bf16_round(h)
    return h, zs


# ------------------------------------------------------------------------------------------------ float32 emulations
def emul_gemm(x, W, b, order="fwd", group=GROUP_EXACT):
    """z = b + sum_k x[:, k] W[:, k] in float32, the accumulator starting AT THE BIAS (what the kernels' accumulators
    do) and rounded once per `group` products (1: a chain of fused multiply-adds; the products and the sum inside a
    group are exact in float64); x [M, K], W [N, K], b [N] float32 arrays; `order`: "fwd" or "rev" in K."""
    x, W = np.asarray(x, np.float32), np.asarray(W, np.float32)
    acc = np.broadcast_to(np.asarray(b, np.float32), (x.shape[0], W.shape[0])).copy()
    starts = list(range(0, x.shape[1], group))
    xd, Wd = x.astype(np.float64), W.astype(np.float64)
    for k in (starts if order == "fwd" else starts[::-1]):
        acc = (acc.astype(np.float64) + xd[:, k:k + group] @ Wd[:, k:k + group].T).astype(np.float32)
    return acc


def _seq_sum32(v, order):
    """row sums of a float32 [M, N] array the way a wave forms them: a lane adds its own 16 (8 when N is no multiple
    of 16) values one by one in the given order, the lanes' partial sums are combined by a halving tree"""
    m, n = v.shape
    c = 16 if n % 16 == 0 else 8
    p = v.reshape(m, n // c, c)
    s = np.zeros((m, n // c), np.float32)
    for k in (range(c) if order == "fwd" else range(c - 1, -1, -1)):
        s = s + p[:, :, k]
    while s.shape[1] > 1:
        if s.shape[1] % 2:
            s = np.concatenate([s, np.zeros((m, 1), np.float32)], axis=1)
        s = s[:, 0::2] + s[:, 1::2]
    return s[:, 0]


def emul_ln_act(z, gamma, beta, act, eps, mode, order="fwd", eps_mode="inside", n_real=None):
    """float32 LayerNorm + activation of float32 rows z; mode in {"centred", "onepass_shift"}"""
    f = np.float32
    z = np.asarray(z, f)
    zz = z if n_real is None else z[:, :n_real]
    n = f(zz.shape[1])
    e = {"inside": f(eps), "omit": f(0.0), "default": f(1e-5)}[eps_mode]
    mean = _seq_sum32(zz, order) / n
    if mode == "centred":
        d = zz - mean[:, None]
        var = _seq_sum32(d * d, order) / n
        rstd = f(1.0) / np.sqrt(var + e, dtype=f)
        xh = (z - mean[:, None]) * rstd[:, None]
    elif mode == "pooled":
        # what the feature-split kernels do: 8 waves, each its own mean m_w and centred M2_w over its slice, pooled as
        # mean = avg(m_w), M2 = sum(M2_w) + n_w sum((m_w - mean)^2)
        nw = 8
        parts = np.split(zz, nw, axis=1)
        n_w = f(parts[0].shape[1])
        mw = np.stack([_seq_sum32(p, order) / n_w for p in parts], axis=1)
        m2 = np.stack([_seq_sum32((p - mw[:, i:i + 1]) ** 2, order) for i, p in enumerate(parts)], axis=1)
        mean = _seq_sum32(mw, order) / f(nw)
        dm = mw - mean[:, None]
        var = (_seq_sum32(m2, order) + n_w * _seq_sum32(dm * dm, order)) / n
        rstd = f(1.0) / np.sqrt(var + e, dtype=f)
        xh = (z - mean[:, None]) * rstd[:, None]
    elif mode == "onepass_shift":
        q = _seq_sum32((zz.astype(np.float64) ** 2).astype(f), order) / n
        var = np.maximum((q.astype(np.float64) - mean.astype(np.float64) ** 2).astype(f), f(0.0))   # fma(-mean, mean, q / n)
        with np.errstate(divide="ignore"):
            rstd = f(1.0) / np.sqrt(var + e, dtype=f)
        shift = -mean * rstd
        xh = (z.astype(np.float64) * rstd[:, None].astype(np.float64) + shift[:, None].astype(np.float64)).astype(f)
    else:
        raise ValueError(mode)
    y = (xh.astype(np.float64) * np.asarray(gamma, f).astype(np.float64) + np.asarray(beta, f).astype(np.float64)).astype(f)
    return act64(torch.from_numpy(y.astype(np.float64)), act).numpy().astype(f)


def emul_ln_act_backward(z, g, gamma, beta, act, eps, order="fwd"):
    """float32 backward of a = act(LayerNorm(z)) with centred statistics: (dz, dgamma, dbeta, dbias); the column sums
    add one row after the other in fp32, from the unrounded rows"""
    f = np.float32
    z, g, gamma, beta = (np.asarray(t, f) for t in (z, g, gamma, beta))
    n = f(z.shape[1])
    mean = _seq_sum32(z, order) / n
    d = z - mean[:, None]
    rstd = f(1.0) / np.sqrt(_seq_sum32(d * d, order) / n + f(eps), dtype=f)
    xh = d * rstd[:, None]
    y = xh * gamma + beta
    dy = g * act_grad64(torch.from_numpy(y.astype(np.float64)), act).numpy().astype(f)
    gg = dy * gamma
    mg, mgx = _seq_sum32(gg, order) / n, _seq_sum32(gg * xh, order) / n
    dz = rstd[:, None] * (gg - mg[:, None] - xh * mgx[:, None])
    col = lambda v: _seq_sum32(np.ascontiguousarray(v.T), order) if v.shape[0] % 8 == 0 else v.astype(f).cumsum(0, dtype=f)[-1]   # noqa: E731
    return dz, col(dy * xh), col(dy), col(dz)


def emul_layer(x, W, b, gamma, beta, act, eps, mode, order="fwd", eps_mode="inside", skip=None, n_real=None, z=None,
               group=GROUP_EXACT):
    z = emul_gemm(x, W, b, order, group) if z is None else z
    a = emul_ln_act(z, gamma, beta, act, eps, mode, order, eps_mode, n_real)
    return a if skip is None else (a + np.asarray(skip, np.float32))


# ------------------------------------------------------------------------------------------------------ error measures
def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def elem_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    rms = max(float(np.sqrt(np.mean(b * b))), 1e-30)
    return float((np.abs(a - b) / (np.abs(b) + rms)).max())


def rows_err(a, b, rows):
    """max |a - b| over `rows` alone / max |b| over everything: the const rows on their own"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a[rows] - b[rows]).max() / max(np.abs(b).max(), 1e-30))


def bf16_ratio(a, b):
    """worst |a - b| / (2^-8 |b| + 1e-4 max|b|): <= 1 on EVERY element is the bf16 single-layer bound -- one
    round-to-nearest to 8 significant bits (2^-9 |b|, doubled for the value that is rounded being off itself) of a
    value that meets the fp32 bar"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    bound = BF16_ULP * np.abs(b) + F32_BAR * max(np.abs(b).max(), 1e-30)
    return float((np.abs(a - b) / bound).max())


# --------------------------------------------------------------------------------------------------------------- cases
CONST_ROWS = lambda M: [0, M // 2, M - 1]   # noqa: E731


def make_case(name, widths, M=M_ROWS, seed=0, nseg=3, acts=None, skip=True, bf16=False, n_tab=97, r=None, head=0,
              cap=True, group=GROUP_EXACT, ref_device="cpu"):
    """One conformance case of a `len(widths) - 1`-layer net widths[0] -> ... -> widths[-1].

    Returns a dict: segments [(table, index or None)] (float32 CPU tensors; bf16-exact if ``bf16``), x (their
    concatenation), layers [(W, b, gamma, beta, act)] (float32 tensors; W bf16-exact if ``bf16``), eps, skip, ref
    (float64 result, hidden roundings applied if ``bf16``), zs (float64 pre-LayerNorm rows), r (the offset in use:
    ``r_eff`` of the case's nominal r at the widest GEMM unless ``r`` overrides it / ``cap`` is off), const_rows.
    ``ref_device``: where the float64 forward runs (a GPU for the 65,617-row case).  ``head``: append a plain Linear widths[-1] -> head (the last layer of a score head).

    r0: N(0,1) rows, randn / sqrt(K) weights, 0.2 randn biases and LayerNorm parameters (1 + 0.2 randn scale) --
    the distribution of every other MLP test.  rR: every Linear's bias += R sigma_l, sigma_l = the mean float64
    row std of that layer's z at r = 0 (a LayerNorm output does not depend on the offset of its input row, so
    sigma_l of a later layer is unchanged by the offsets below it).  sE: W and b of every layer x 2^E, sigma_l taken
    at that scale.  eps1e-3: eps = 1e-3 at scale 2^-4.  const_cC: the first, middle and last row of every segment (and
    of the gathered table rows they point to) are zero and the first layer's bias is the constant C, so those rows
    of z are exactly C in any arithmetic."""
    c = parse_case(name)
    kmax = max(widths[:-1])
    rr = (r_eff(c["r"], kmax, bf16, group) if cap else c["r"]) if r is None else float(r)
    if c["const"] is not None and cap:
        c["const"] = r_eff(c["const"], kmax, bf16, group)
    g = torch.Generator().manual_seed(1000 * seed + 7 * len(widths) + widths[0] + widths[-1])
    K, n_layers = widths[0], len(widths) - 1
    assert K % nseg == 0
    sw = K // nseg
    cast = (lambda t: t.bfloat16().float()) if bf16 else (lambda t: t)
    table = cast(torch.randn(n_tab, sw, generator=g))
    direct = cast(torch.randn(M, sw, generator=g))
    idx = [torch.randint(1, n_tab, (M,), generator=g) for _ in range(nseg - 1)]
    const_rows = CONST_ROWS(M) if c["const"] is not None else []
    if const_rows:
        table[0] = 0.0
        direct[const_rows] = 0.0
        for i in idx:
            i[const_rows] = 0
    segments = [(table, i.to(torch.int64)) for i in idx] + [(direct, None)]
    x = torch.cat([t if i is None else t[i] for t, i in segments], dim=1)
    if acts is None:
        acts = [ACT_GELU] * (n_layers - 1) + [ACT_TANH if n_layers == 2 else ACT_GELU]
    layers = []
    for l in range(n_layers):
        W = cast(torch.randn(widths[l + 1], widths[l], generator=g) / widths[l] ** 0.5)
        b = 0.2 * torch.randn(widths[l + 1], generator=g)
        gm = 1 + 0.2 * torch.randn(widths[l + 1], generator=g)
        bt = 0.2 * torch.randn(widths[l + 1], generator=g)
        layers.append([W, b, gm, bt, acts[l]])
    sk = direct if skip else None
    assert not skip or sw == widths[-1]
    if c["const"] is not None:
        layers[0][1] = torch.full_like(layers[0][1], c["const"])
    if c["scale_exp"]:
        s = 2.0 ** c["scale_exp"]
        for l in range(n_layers):
            layers[l][0] = layers[l][0] * s
            layers[l][1] = layers[l][1] * s
    if rr:   # sigma_l at r = 0 of THIS case (its scale and eps: near var ~ eps the hidden rows shrink)
        _, zs0 = _forward_on(ref_device, x, layers, c["eps"], sk, bf16)
        for l in range(n_layers):
            sigma = float(zs0[l].std(dim=1, unbiased=False).mean())
            layers[l][1] = (layers[l][1].double() + rr * sigma).float()
    if head:   # K -> H -> H -> head: a plain last Linear on the hidden rows (not offset, not scaled: it has no LayerNorm)
        layers.append([torch.randn(head, widths[-1], generator=g) / widths[-1] ** 0.5, 0.2 * torch.randn(head, generator=g),
                       None, None, ACT_NONE])
    layers = [tuple(t) for t in layers]
    ref, zs = _forward_on(ref_device, x, layers, c["eps"], sk, bf16)
    return dict(name=name, segments=segments, x=x, layers=layers, eps=c["eps"], skip=sk, ref=ref, zs=zs, r=rr,
                nominal_r=c["r"], const=c["const"], const_rows=const_rows, bf16=bf16, widths=list(widths), group=group)


def _forward_on(device, x, layers, eps, skip, bf16):
    """net_forward with the float64 arithmetic on `device` (large M), results back on the CPU"""
    mv = lambda t: None if t is None else t.to(device)   # noqa: E731
    out, zs = net_forward(mv(x), [(mv(W), mv(b), mv(g), mv(bt), a) for W, b, g, bt, a in layers], eps, mv(skip), bf16)
    return out.cpu(), [z.cpu() for z in zs]


def make_rows_case(name, W, M=M_ROWS, seed=0, bf16=False, r=None):
    """pre-LayerNorm rows given directly: z = 2^E sigma (randn + r) with sigma = 1.5, the const rows literal constants;
    bf16: z and the upstream gradient are rounded to bf16 first and the float64 definition gets the same values.
    -> dict(z, g, gamma, beta, eps, r, const_rows)"""
    c = parse_case(name)
    rr = c["r"] if r is None else float(r)
    g = torch.Generator().manual_seed(77 * seed + W)
    z = 1.5 * (torch.randn(M, W, generator=g) + rr) * 2.0 ** c["scale_exp"]
    const_rows = CONST_ROWS(M) if c["const"] is not None else []
    if const_rows:
        z[const_rows] = c["const"]
    go = torch.randn(M, W, generator=g)
    gm = 1 + 0.2 * torch.randn(W, generator=g)
    bt = 0.2 * torch.randn(W, generator=g)
    if bf16:
        z, go = z.bfloat16().float(), go.bfloat16().float()
    return dict(name=name, z=z, g=go, gamma=gm, beta=bt, eps=c["eps"], r=rr, const_rows=const_rows)


# ------------------------------------------------------------------------------- the launches of the GPU file, by name
# fp32 forward entries: name -> make_case arguments (+ "split": the split-bf16 kernel takes the shape too)
F32_CONFIGS = {
    "L128x2": dict(widths=[384, 256, 128], split=True),
    "L128x3": dict(widths=[384, 256, 256, 128], split=True),
    "L256x2": dict(widths=[768, 512, 256], split=True),
    "L256x3": dict(widths=[768, 512, 512, 256], split=True),
    "L32x2": dict(widths=[96, 64, 32], split=False),
    "head256": dict(widths=[256, 256, 256], nseg=2, skip=False, acts=[ACT_GELU, ACT_GELU], head=1, split=True),
    "narrow64": dict(widths=[64, 128, 128, 56], nseg=1, skip=False, split=False),          # LayerNorm over 56 < 64 features
    "single512": dict(widths=[128, 512], nseg=1, skip=False, acts=[ACT_GELU], split=False),
}
# bf16 forward entries
BF16_CONFIGS = {
    "wave_L32x2": dict(widths=[96, 64, 32], split=False),
    "wave_L128x2": dict(widths=[384, 256, 128], split=False),
    "split_L128x2": dict(widths=[384, 256, 128], split=True),
    "split_L128x3": dict(widths=[384, 256, 256, 128], split=True),
    "split_L256x2": dict(widths=[768, 512, 256], split=True),
    "split_L256x3": dict(widths=[768, 512, 512, 256], split=True),
    "split_L512x2": dict(widths=[1536, 1024, 512], split=True),
    "split_L512x3": dict(widths=[1536, 1024, 1024, 512], split=True),
}
# single-layer launches of the feature-split kernel: one direct segment -> o.  Without skip rows the activation is ReLU:
# the bf16 kernels evaluate GELU in its tanh form (documented in mlp_fused_bf16.hip: <= 5e-4 absolute), which an
# element-wise bound of 2^-8 |ref| + 1e-4 max|ref| does not admit on small outputs unless the skip rows raise max|ref| --
# a property of the activation, not of the statistics this file is about.
BF16_SINGLE = {
    "o256": dict(widths=[128, 256], nseg=1, skip=False, acts=[ACT_RELU]),
    "o256_skip": dict(widths=[256, 256], nseg=1, skip=True, acts=[ACT_GELU]),
    "o512": dict(widths=[128, 512], nseg=1, skip=False, acts=[ACT_RELU]),
    "o512_skip": dict(widths=[512, 512], nseg=1, skip=True, acts=[ACT_GELU]),
    "o1024": dict(widths=[128, 1024], nseg=1, skip=False, acts=[ACT_RELU]),
    "o1024_skip": dict(widths=[1024, 1024], nseg=1, skip=True, acts=[ACT_GELU]),
}


def case_for(config, name, bf16=False, matrix=False, **kw):
    """the case of a launch; ``matrix``: it runs on a matrix-pipe kernel (split-bf16 fp32, bf16) -- GROUP_MATRIX"""
    cfg = dict(config)
    cfg.pop("split", None)
    return make_case(name, bf16=bf16, group=GROUP_MATRIX if (matrix or bf16) else GROUP_EXACT, **cfg, **kw)


def emul_net(case, mode, order, rows, eps_mode="inside"):
    """the whole net of a case through the float32 emulation, on a subset of its rows (rows are independent)"""
    h = case["x"][rows].numpy()
    layers = case["layers"]
    for i, (W, b, gm, bt, act) in enumerate(layers):
        last = i == len(layers) - 1
        sk = case["skip"][rows].numpy() if (last and case["skip"] is not None) else None
        if gm is None:
            h = emul_gemm(h, W.numpy(), b.numpy(), order, case["group"])
            continue
        h = emul_layer(h, W.numpy(), b.numpy(), gm.numpy(), bt.numpy(), act, case["eps"], mode, order, eps_mode, sk,
                       group=case["group"])
        if case["bf16"] and not last:
            h = torch.from_numpy(h).bfloat16().float().numpy()
    return h
