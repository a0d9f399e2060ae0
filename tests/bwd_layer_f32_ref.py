"""Cases, operands and float64 references of hgnn_mlp_backward_layer_f32 (the fused backward layer of the exact fp32
training path), shared by tests/test_bwd_layer_f32_api.py, tests/test_bwd_layer_f32_ref.py (CPU) and
tests/test_gpu_bwd_layer_f32.py.

Input form and the GEMM half of the LayerNorm form: the integer grids of tests/gemm_ref.py (``dgrad_operands``) --
every partial sum is an integer below EXACT_LIMIT, so the fp32 chain of fused multiply-adds is exact in any order and
the kernel's result must equal the float64 product bit for bit.  ``dgrad_mutants_f32`` are gemm_ref.dgrad_mutants without
the final bf16 rounding (its `truncated` and `skip_after_rounding` mutants are mutants OF that rounding and have no fp32
counterpart).

LayerNorm form, bars: dz = randn, W = randn / sqrt(K), rows from ln_ref.make_rows_case; the float64 definition is
ln_ref.ln_act_backward(z, dz W, ...) / ln_ref.ln_act_forward.  ReLU: its derivative jumps at 0 and the upstream
gradient da = dz W is formed inside the kernel, so it cannot be masked as tests/test_gpu_mlp_layernorm.py masks it;
instead the rows are moved until no pre-activation lies within 1e-3 of 0 (const rows excepted: their pre-activation is
beta exactly in any arithmetic).
"""
import functools

import numpy as np
import torch

import gemm_ref as G
import ln_ref as R

BLOCKS = 512                                       # HGNN_MLP_BWD_F32_BLOCKS
EXACT_N = (64, 128, 256, 512)
EXACT_K = (64, 128, 512, 1024)
EXACT_M = G.TILE_M                                 # one row, the 64-row tile's edges, three tiles + one row
FORMS = ("plain", "skip", "wslice")
CELL_LN = ((128, 256), (256, 256), (256, 512), (512, 512))      # (K, N) of the cell networks, LayerNorm form
CELL_INPUT = ((256, 128), (512, 256))                           # input form
BAR_SHAPES = CELL_LN + ((1024, 128),)
BAR_ACTS = (R.ACT_GELU, R.ACT_TANH, R.ACT_RELU)
RELU_GAP = 1e-3


def exact_case(M, K, N, form):
    """dz [M, K], W [K, N] (a column slice of a [K, 3N] weight for `wslice`), skip [M, N] or None; CPU fp32"""
    dz, W, skip = G.dgrad_operands(M, K, N, G.dgrad_seed(M, K, N), form == "skip")
    if form == "wslice":
        full = G.small(K, 3 * N, 21)
        full[:, N:2 * N] = W
        W = full[:, N:2 * N]
    return dz, W, skip


def dgrad_ref_f32(dz, W, skip=None):
    """dz . W (+ skip) in float64: exact integers, returned as fp32"""
    s = dz.double() @ W.double()
    if skip is not None:
        s = s + skip.double()
    return _f32_exact(s)


def _f32_exact(s):
    """the float64 integers ``s`` as fp32 (exact below 2^24)"""
    f = s.float()
    assert torch.equal(f.double(), s)
    return f


def dgrad_mutants_f32(dz, W, skip):
    """name -> fp32 result of a subtly wrong input-form backward layer (gemm_ref.dgrad_mutants, unrounded)"""
    K, N = W.shape
    k = K // 2
    keep = torch.ones(K, dtype=torch.bool)
    keep[k] = False
    s = dz.double() @ W.double()
    sk = skip.double() if skip is not None else 0
    c = N // 2 - 1
    perm = torch.arange(N)
    perm[c], perm[c + 1] = c + 1, c
    return {"dropped_term": _f32_exact(dz[:, keep].double() @ W[keep].double() + sk),
            "duplicated_term": _f32_exact(s + torch.outer(dz[:, k].double(), W[k].double()) + sk),
            "columns_swapped": _f32_exact(s[:, perm] + sk)}


def _relu_clear_of_zero(rc):
    """move z (not the const rows) until no pre-activation is within RELU_GAP of 0"""
    z = rc["z"].clone()
    free = torch.ones(z.shape[0], dtype=torch.bool)
    free[rc["const_rows"]] = False
    for _ in range(8):
        y = R.ln_act_forward(z, rc["gamma"], rc["beta"], R.ACT_NONE, rc["eps"])
        bad = (y.abs() < 2 * RELU_GAP) & free[:, None]
        if not bool(bad.any()):
            break
        _, rstd = R.ln_stats64(z.double(), rc["eps"])
        step = 8 * RELU_GAP / (rstd * rc["gamma"].double().abs().clamp_min(1e-2))
        z = torch.where(bad, (z.double() + torch.where(y >= 0, step, -step) * torch.sign(rc["gamma"].double())).float(), z)
    y = R.ln_act_forward(z, rc["gamma"], rc["beta"], R.ACT_NONE, rc["eps"])
    assert not bool(((y.abs() < RELU_GAP) & free[:, None]).any())
    rc["z"] = z
    return rc


@functools.lru_cache(maxsize=None)
def bar_operands(K, N):
    gen = torch.Generator().manual_seed(1000 * K + N)
    dz = torch.randn(R.M_ROWS, K, generator=gen)
    W = torch.randn(K, N, generator=gen) / K ** 0.5
    return dz, W, dz.double() @ W.double()


@functools.lru_cache(maxsize=None)
def bar_case(K, N, name, act):
    """(rows case, dz, W, float64 references dict) of one LayerNorm-form conformance case; computed once per session"""
    dz, W, da = bar_operands(K, N)
    rc = R.make_rows_case(name, N, seed=K)
    if act == R.ACT_RELU:
        rc = _relu_clear_of_zero(rc)
    a = R.ln_act_forward(rc["z"], rc["gamma"], rc["beta"], act, rc["eps"])
    dzp, dg, db, dbias = R.ln_act_backward(rc["z"], da, rc["gamma"], rc["beta"], act, rc["eps"])
    ref = dict(a=a.numpy(), dz=dzp.numpy(), dgamma=dg.numpy(), dbeta=db.numpy(), dbias=dbias.numpy())
    return rc, dz, W, ref


def emulate(K, N, name, act, order):
    """the arithmetic the kernel is to perform, in float32 on the CPU: da as a k-ordered chain of fused multiply-adds
    starting at 0, then the centred LayerNorm / activation backward and forward of tests/ln_ref.py"""
    rc, dz, W, _ = bar_case(K, N, name, act)
    da = emul_da(K, N, order)
    dzp, dg, db, dbias = R.emul_ln_act_backward(rc["z"].numpy(), da, rc["gamma"].numpy(), rc["beta"].numpy(), act,
                                                rc["eps"], order)
    a = R.emul_ln_act(rc["z"].numpy(), rc["gamma"].numpy(), rc["beta"].numpy(), act, rc["eps"], "centred", order)
    return dict(a=a, dz=dzp, dgamma=dg, dbeta=db, dbias=dbias)


@functools.lru_cache(maxsize=None)
def emul_da(K, N, order):
    dz, W, _ = bar_operands(K, N)
    return R.emul_gemm(dz.numpy(), W.t().contiguous().numpy(), np.zeros(N, np.float32), order)


def errors(out, ref, rc):
    """name -> (value, is it asserted) of the project's fp32 bars for one case: rel always, elem for nominal r <= 64,
    const rows on their own, column sums normwise"""
    e = {}
    for what in ("a", "dz"):
        e[what + ".rel"] = R.rel_err(out[what], ref[what])
        if rc["r"] <= 64:
            e[what + ".elem"] = R.elem_err(out[what], ref[what])
        if len(rc["const_rows"]):
            e[what + ".const"] = R.rows_err(out[what], ref[what], list(rc["const_rows"]))
    for what in ("dgamma", "dbeta", "dbias"):
        e[what] = R.rel_err(out[what], ref[what])
    return e


def trip_rows():
    return BLOCKS * 64
