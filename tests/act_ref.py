"""float64 definitions of the activations behind HGNN_ACT_SILU .. HGNN_ACT_SIGMOID (include/hgnn_hip.h) and of their
derivatives, a float32 EMULATION of the forms csrc/mlp_common.h evaluates them with, and the cases of
tests/test_gpu_mlp_activations.py / tests/test_gpu_mlp_plain.py (built on tests/ln_ref.py's case machinery).

Definition: torch.nn.SiLU / LeakyReLU / ELU / Sigmoid at their constructor defaults on float64 -- what the reference's
make_mlp instantiates (``getattr(nn, name)()``).  Codes 0..3 are ln_ref's.

Emulation (float32, used only to prove the stated bounds and to size the tests, tests/test_act_ref.py): every
operation of the device form in float32, fused multiply-adds rounded once; ``v_exp_f32`` and ``v_rcp_f32`` are modelled
at their documented accuracy of 1 ulp: the correctly rounded result moved by ``dexp`` / ``drcp`` in {-1, 0, +1} ulps, every
combination tried.

Stated bounds (``BOUNDS``; u = 2^-24; the comment in csrc/mlp_common.h carries the derivations):
    |device - definition| <= rel(x) |definition| + FLOOR max(1, |x|)   with   rel(x) = (1.25 |x| + c) u,
or for silu', whose value crosses zero, an absolute bound.  1.25 |x| u: the exponent x log2(e) is a rounded product
(|x| log2(e) u absolute, times ln 2 in the power: |x| u) with a rounded constant (float32 log2(e) is off by 0.22 u
relative: 0.22 |x| u).  FLOOR = 2^-125 covers results below the normal range (the power flushes to zero or overflows
there: sigmoid(-88) is 0 against 6e-39; SiLU multiplies that by |x|).
"""
import math

import numpy as np
import torch

import ln_ref as R

ACT_SILU, ACT_LEAKY_RELU, ACT_ELU, ACT_SIGMOID = 4, 5, 6, 7          # hgnn_hip.h HGNN_ACT_*
ACT_LAST = ACT_SIGMOID
NEW_CODES = (ACT_SILU, ACT_LEAKY_RELU, ACT_ELU, ACT_SIGMOID)
ACT_CODE = dict(R.ACT_CODE, SiLU=4, LeakyReLU=5, ELU=6, Sigmoid=7)
ACT_NAME = {v: k for k, v in ACT_CODE.items()}
U = 2.0 ** -24
FLOOR = 2.0 ** -125
LOG2E = np.float32(1.44269504088896341)
ELU_POLY_BELOW = 0.25                                                # |x| below which expm1 is the polynomial

_F = torch.nn.functional


def act64(y, act):
    y = y.double()
    if act == ACT_SILU:
        return _F.silu(y)
    if act == ACT_LEAKY_RELU:
        return _F.leaky_relu(y)           # negative_slope = 0.01
    if act == ACT_ELU:
        return _F.elu(y)                  # alpha = 1.0
    if act == ACT_SIGMOID:
        return torch.sigmoid(y)
    return R.act64(y, act)


def act_grad64(y, act):
    y = y.double()
    if act == ACT_SILU:
        s = torch.sigmoid(y)
        # s (1 - s) without the cancellation of 1 - s: sigmoid(y) sigmoid(-y)
        return s + y * s * torch.sigmoid(-y)
    if act == ACT_LEAKY_RELU:
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, 0.01))
    if act == ACT_ELU:
        return torch.where(y > 0, torch.ones_like(y), torch.exp(torch.clamp_max(y, 0.0)))
    if act == ACT_SIGMOID:
        return torch.sigmoid(y) * torch.sigmoid(-y)
    return R.act_grad64(y, act)


# ------------------------------------------------------------------------------------------------ float32 emulation
def _f(v):
    return np.asarray(v, np.float32)


def _nudge(v, ulps):
    v = _f(v)
    if ulps == 0:
        return v
    return np.nextafter(v, _f(np.inf if ulps > 0 else -np.inf))


def _exp2(x, d):
    """v_exp_f32: 2^x correctly rounded, moved by d ulps; results below the normal range flush to zero"""
    with np.errstate(over="ignore", under="ignore"):
        e = _f(np.exp2(_f(x).astype(np.float64)))
    e = np.where(np.isfinite(e) & (e > 0), _nudge(e, d), e)
    return _f(np.where(e < np.float32(2.0 ** -126), np.float32(0.0), e))


def _rcp(x, d):
    """v_rcp_f32: 1 / x correctly rounded, moved by d ulps; rcp(inf) = 0"""
    with np.errstate(divide="ignore", over="ignore"):
        r = _f(1.0 / _f(x).astype(np.float64))
    return _f(np.where(np.isfinite(r) & (r > 0), _nudge(r, d), r))


def _fma(a, b, c):
    """one rounding (the float64 product of two float32 is exact; the sum is rounded to float64 first, which at these
    magnitudes differs from a true fma by less than 2^-29 of an ulp of the float32 result)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return _f(_f(a).astype(np.float64) * _f(b).astype(np.float64) + _f(c).astype(np.float64))


def _mul(a, b):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return _f(_f(a) * _f(b))


def _sigmoid(x, dexp, drcp):
    return _rcp(_f(1.0) + _exp2(_mul(-LOG2E, x), dexp), drcp)


def _sigmoid_val_grad(x, dexp, drcp):
    e = _exp2(_mul(-LOG2E, np.abs(_f(x))), dexp)
    r = _rcp(_f(1.0) + e, drcp)
    er = _mul(e, r)
    return _f(np.where(_f(x) >= 0, r, er)), _mul(er, r)


def _elu_neg(xn, e):
    p = _fma(np.float32(1.0 / 720.0), xn, np.float32(1.0 / 120.0))
    p = _fma(p, xn, np.float32(1.0 / 24.0))
    p = _fma(p, xn, np.float32(1.0 / 6.0))
    p = _fma(p, xn, np.float32(0.5))
    p = _fma(p, xn, np.float32(1.0))
    return _f(np.where(xn > np.float32(-ELU_POLY_BELOW), _mul(xn, p), e - _f(1.0)))


def emul_act(x, act, dexp=0, drcp=0):
    """act_apply of csrc/mlp_common.h on float32 x, codes 4..7"""
    x = _f(x)
    if act == ACT_SILU:
        return _mul(x, _sigmoid(x, dexp, drcp))
    if act == ACT_LEAKY_RELU:
        return _f(np.where(x > 0, x, _mul(np.float32(0.01), x)))
    if act == ACT_ELU:
        xn = np.minimum(x, _f(0.0))
        return _f(np.where(x > 0, x, _elu_neg(xn, _exp2(_mul(LOG2E, xn), dexp))))
    if act == ACT_SIGMOID:
        return _sigmoid(x, dexp, drcp)
    raise ValueError(act)


def emul_act_grad(x, act, dexp=0, drcp=0):
    """act_grad (and the derivative half of act_val_grad: the same operations) on float32 x, codes 4..7"""
    x = _f(x)
    if act == ACT_SILU:
        s, ds = _sigmoid_val_grad(x, dexp, drcp)
        return _fma(x, ds, s)
    if act == ACT_LEAKY_RELU:
        return _f(np.where(x > 0, np.float32(1.0), np.float32(0.01)))
    if act == ACT_ELU:
        return _f(np.where(x > 0, np.float32(1.0), _exp2(_mul(LOG2E, np.minimum(x, _f(0.0))), dexp)))
    if act == ACT_SIGMOID:
        return _sigmoid_val_grad(x, dexp, drcp)[1]
    raise ValueError(act)


def emul_act_val(x, act, dexp=0, drcp=0):
    """the VALUE half of act_val_grad (the fused backward layers recompute activations with it): SiLU and Sigmoid use the
    |x|-side sigmoid there, LeakyReLU and ELU the operations of act_apply"""
    x = _f(x)
    if act == ACT_SILU:
        return _mul(x, _sigmoid_val_grad(x, dexp, drcp)[0])
    if act == ACT_SIGMOID:
        return _sigmoid_val_grad(x, dexp, drcp)[0]
    return emul_act(x, act, dexp, drcp)


# (kind, c): "rel": |err| <= (1.25 |x| + c) u |ref| + FLOOR max(1, |x|); "abs": |err| <= c u
BOUNDS = {
    ("val", ACT_SIGMOID): ("rel", 6.0), ("val", ACT_SILU): ("rel", 7.0), ("val", ACT_LEAKY_RELU): ("rel", 2.0),
    ("val", ACT_ELU): ("rel", 16.0),
    ("grad", ACT_SIGMOID): ("rel", 9.0), ("grad", ACT_SILU): ("abs", 12.0), ("grad", ACT_LEAKY_RELU): ("rel", 2.0),
    ("grad", ACT_ELU): ("rel", 3.0),
    # the |x|-side value forms of act_val_grad: one more multiplication on the negative side
    ("val2", ACT_SIGMOID): ("rel", 7.0), ("val2", ACT_SILU): ("rel", 8.0), ("val2", ACT_LEAKY_RELU): ("rel", 2.0),
    ("val2", ACT_ELU): ("rel", 16.0),
}


def bound(kind, act, x, ref):
    """the stated bound on |device - definition| at inputs x (float64 arrays)"""
    how, c = BOUNDS[(kind, act)]
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    if how == "abs":
        return np.full_like(x, c * U)
    # ELU / LeakyReLU are exact (one rounding) on the positive side, whatever |x|
    ax = np.where(x > 0, 0.0, np.abs(x)) if act in (ACT_ELU, ACT_LEAKY_RELU) else np.abs(x)
    return (1.25 * ax + c) * U * np.abs(ref) + FLOOR * np.maximum(1.0, np.abs(x))


def grid():
    """float32 inputs: a dense grid on [-30, 30], +-2^-20 .. +-2^-6 (ELU's cancelling range) with neighbours, +-0, the
    ELU threshold and its neighbours, and magnitudes where the power saturates"""
    g = [np.linspace(-30.0, 30.0, 24001), np.array([0.0, -0.0])]
    for e in range(-20, -5):
        for m in (1.0, 1.25, 1.5, 1.999):
            g.append(np.array([m * 2.0 ** e, -m * 2.0 ** e]))
    t = np.float32(ELU_POLY_BELOW)
    g.append(np.array([-t, np.nextafter(-t, np.float32(0)), np.nextafter(-t, np.float32(-1))], np.float64))
    g.append(np.array([2.0 ** -149, -2.0 ** -149, 2.0 ** -126, -2.0 ** -126, 2.0 ** -60, -2.0 ** -60]))
    g.append(np.array([87.0, -87.0, 88.0, -88.0, 88.8, -88.8, 89.0, -89.0, 100.0, -100.0, 104.0, -104.0, 1e4, -1e4, 1e30,
                       -1e30, 3.4e38, -3.4e38]))
    return _f(np.concatenate(g))


# --------------------------------------------------------------------------------------------- nets with any activation
def net_forward(x, layers, eps, skip=None, bf16=False):
    """ln_ref.net_forward for every activation code and for layers WITHOUT LayerNorm (gamma None: act(x W^T + b)):
    layers [(W, b, gamma or None, beta or None, act)] -> (out, [z_l]) in float64"""
    h, zs = x.double(), []
    for i, (W, b, gm, bt, act) in enumerate(layers):
        last = i == len(layers) - 1
        z = h @ W.double().t() + b.double()
        zs.append(z)
        if gm is not None:
            mean, rstd = R.ln_stats64(z, eps)
            z = (z - mean) * rstd * gm.double() + bt.double()
        h = act64(z, act)
        if last and skip is not None:
            h = h + skip.double()
        if bf16 and not last:
            h = R.bf16_round(h)
    return h, zs


def make_case(name, widths, acts, plain=False, **kw):
    """ln_ref.make_case with activation codes up to ACT_LAST; ``plain``: no layer has a LayerNorm.  ref and zs are
    recomputed here with this file's definitions (ln_ref knows codes 0..3)"""
    head = kw.get("head", 0)
    case = R.make_case(name, widths, acts=list(acts[:len(widths) - 1]), **kw)
    layers = [(W, b, None if plain else gm, None if plain else bt, a) for W, b, gm, bt, a in case["layers"]]
    if head:
        layers[-1] = case["layers"][-1]
    case["layers"] = layers
    dev = kw.get("ref_device", "cpu")                     # a GPU for the 65,617-row case
    mv = lambda t: None if t is None else t.to(dev)       # noqa: E731
    ref, zs = net_forward(mv(case["x"]), [(mv(W), mv(b), mv(g), mv(bt), a) for W, b, g, bt, a in layers], case["eps"],
                          mv(case["skip"]), case["bf16"])
    case["ref"], case["zs"] = ref.cpu(), [z.cpu() for z in zs]
    case["plain"] = plain
    return case


def emul_net(case, order="fwd", dexp=0, drcp=0):
    """float32 emulation of a case's net the way the exact fp32 kernel evaluates it: k-ascending fma chains starting at
    the bias (ln_ref.emul_gemm), centred LayerNorm statistics (ln_ref.emul_ln_act) or none, the device forms of the
    activations for codes 4..7 (ln_ref's float64-then-rounded ones for 0..3)"""
    h = case["x"].numpy()
    layers = case["layers"]
    for i, (W, b, gm, bt, act) in enumerate(layers):
        last = i == len(layers) - 1
        z = R.emul_gemm(h, W.numpy(), b.numpy(), order, case["group"])
        if gm is not None:
            z = R.emul_ln_act(z, gm.numpy(), bt.numpy(), R.ACT_NONE, case["eps"], "centred", order)
        if act in NEW_CODES:
            h = emul_act(z, act, dexp, drcp)
        else:
            h = R.act64(torch.from_numpy(z.astype(np.float64)), act).numpy().astype(np.float32)
        if last and case["skip"] is not None:
            h = h + case["skip"].numpy()
        if case["bf16"] and not last:
            h = torch.from_numpy(h).bfloat16().float().numpy()
    return h


# A LayerNorm-less layer has nothing that renormalises its rows, so the error of the k-ascending fma chain is carried at the
# magnitude of z: each of the K steps rounds the accumulator, 0.29 ulp rms, so z is off by ~ 0.29 u 2 sqrt(K) rms(z)
# ~ 3.4e-8 sqrt(K) rms(z), ~4x that at the worst element, and |act'| <= 1.1 for every code.  With randn / sqrt(K) weights
# rms(z) ~ 1 per layer and max|ref| >= 1 (the skip rows, or a Tanh / Sigmoid output near its asymptote, or a few sigma of
# a linear output), so three layers at K <= 768 stay below 3 * 4 * 3.4e-8 * sqrt(768) * 1.1 = 1.2e-5 normwise: an
# order of magnitude inside F32_BAR.  The plain route is therefore held to the SAME bars as the LayerNorm'ed kernels,
# normwise against max|ref| and element-wise in ln_ref's form; tests/test_act_ref.py proves every case at half the bar
# with ``emul_net``.
PLAIN_BAR = R.F32_BAR

# The GPU files' launches by name: widths, activation codes, make_case keywords
_S, _E, _T, _G, _L, _SG = ACT_SILU, ACT_ELU, R.ACT_TANH, R.ACT_GELU, ACT_LEAKY_RELU, ACT_SIGMOID
F32_ACT_CONFIGS = {
    # exact fp32 at its narrowest width: compile-time SiLU (+ SiLU / Tanh output) and the runtime switch (ELU output)
    "L32x2_silu_tanh": dict(widths=[96, 64, 32], acts=[_S, _T]),
    "L32x2_silu_elu": dict(widths=[96, 64, 32], acts=[_S, _E]),
    "L32x3_silu_silu": dict(widths=[96, 64, 64, 32], acts=[_S, _S, _S]),
    "L32x3_silu_elu": dict(widths=[96, 64, 64, 32], acts=[_S, _S, _E]),
    "L32x2_leaky_sigmoid": dict(widths=[96, 64, 32], acts=[_L, _SG]),
    "L32x3_elu_leaky": dict(widths=[96, 64, 64, 32], acts=[_E, _E, _L]),
    "head64_silu": dict(widths=[64, 64, 64], acts=[_S, _S], nseg=2, skip=False, head=1),
    "head64_elu": dict(widths=[64, 64, 64], acts=[_E, _E], nseg=2, skip=False, head=1),
    "enc3_silu": dict(widths=[3, 64, 64, 32], acts=[_S, _S, _S], nseg=1, skip=False),
    "enc6_elu_sigmoid": dict(widths=[6, 64, 32], acts=[_E, _SG], nseg=2, skip=False),
}
SPLIT3_ACT_CONFIGS = {
    "L128x2_silu_tanh": dict(widths=[384, 256, 128], acts=[_S, _T]),
    "L128x2_silu_elu": dict(widths=[384, 256, 128], acts=[_S, _E]),
    "L128x3_silu_silu": dict(widths=[384, 256, 256, 128], acts=[_S, _S, _S]),
    "L128x3_leaky_sigmoid": dict(widths=[384, 256, 256, 128], acts=[_L, _L, _SG]),
}
BF16_ACT_CONFIGS = {
    "wave_L32x2_silu_tanh": dict(widths=[96, 64, 32], acts=[_S, _T], split=False),
    "wave_L32x2_silu_elu": dict(widths=[96, 64, 32], acts=[_S, _E], split=False),
    "wave_L32x3_leaky_sigmoid": dict(widths=[96, 64, 64, 32], acts=[_L, _L, _SG], split=False),
    "split_L128x2_silu_tanh": dict(widths=[384, 256, 128], acts=[_S, _T], split=True),
    "split_L128x2_silu_elu": dict(widths=[384, 256, 128], acts=[_S, _E], split=True),
    "split_L128x3_elu_sigmoid": dict(widths=[384, 256, 256, 128], acts=[_E, _E, _SG], split=True),
}
PLAIN_CONFIGS = {
    "L32x2_silu_tanh": dict(widths=[96, 64, 32], acts=[_S, _T]),
    "L32x3_elu_leaky": dict(widths=[96, 64, 64, 32], acts=[_E, _E, _L]),
    "L32x3_gelu_sigmoid": dict(widths=[96, 64, 64, 32], acts=[_G, _G, _SG]),
    "L64x2_leaky_silu": dict(widths=[192, 128, 64], acts=[_L, _S]),
    "head64_silu": dict(widths=[64, 64, 64], acts=[_S, _S], nseg=2, skip=False, head=1),
    "head64_tanh_w8": dict(widths=[64, 64, 64], acts=[_T, _T], nseg=2, skip=False, head=8),
    "enc3_gelu": dict(widths=[3, 64, 64, 32], acts=[_G, _G, _G], nseg=1, skip=False),
    "enc6_elu": dict(widths=[6, 64, 32], acts=[_E, _E], nseg=2, skip=False),
    "narrow64_silu": dict(widths=[64, 128, 128, 56], acts=[_S, _S, _S], nseg=1, skip=False),
}


def case_for(cfg, name="r0", plain=False, bf16=False, matrix=False, **kw):
    c = dict(cfg)
    c.pop("split", None)
    return make_case(name, c.pop("widths"), c.pop("acts"), plain=plain, bf16=bf16,
                     group=R.GROUP_MATRIX if (matrix or bf16) else R.GROUP_EXACT, **c, **kw)


def tiny_rows(W, M=R.M_ROWS, seed=0):
    """rows for the row kernels: N(0, 1.5) values with the first rows replaced by ELU's cancelling range +-2^-20 .. +-2^-6,
    +-0 and the polynomial threshold, and an upstream gradient"""
    g = torch.Generator().manual_seed(31 * seed + W)
    z = 1.5 * torch.randn(M, W, generator=g)
    special = torch.tensor([s * 2.0 ** e for e in range(-20, -5) for s in (1.0, -1.0)] + [0.0, -0.0, -0.25, -0.2500001, -0.2499999])
    z[0, :special.numel()] = special
    if M > 1:
        z[1, -special.numel():] = special
    return z, torch.randn(M, W, generator=g)
