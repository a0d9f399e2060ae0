"""float64 mirror of the bf16 training route (fused._FusedMLPTrainBf16: forward dumps + hand-written backward), its
float32 emulation, and the cases of tests/test_gpu_bf16_train_mirror.py.  tests/test_bf16_train_ref.py proves everything
here on the CPU.

The mirror rounds to bf16 (round to nearest even, ln_ref.bf16_round) exactly where the route stores bf16 and nowhere
else; what remains between mirror and device is fp32 summation order, the fast erf / tanh / exp forms, and single bf16
ulps on elements whose fp32 value sits on the other side of a rounding tie.

FORWARD (``forward_mirror``; csrc/mlp_split_bf16.hip:393-439, csrc/mlp_split_common.h gelu_t).  The kernel keeps every
layer's pre-LayerNorm rows in its fp32 accumulators, DUMPS their bf16 rounding (dump_pre) and normalises the
accumulators themselves, not the dump; the hidden activations are rounded to bf16 on their way into the next GEMM and the
result once, after the skip add.  So with zhat the unrounded rows:
    zhat_0 = b_0 + bf16(W_0) concat(x)            z_l   = bf16(zhat_l)                       (the dump)
    a_l    = bf16(act(LN(zhat_l)))                zhat_{l+1} = b_{l+1} + bf16(W_{l+1}) a_l
    out    = bf16(act(LN(zhat_{n-1})) (+ skip))
with the kernel's GELU x sigmoid(2u), u = sqrt(2 / pi)(x + 0.044715 x^3).  (A mirror that normalised the DUMP z_l would
be off by the dump's own rounding, 2^-9 |z| / sigma per element of LN(z): not what the forward computes.)

BACKWARD (``mirror``; line numbers of hierarchicalgnn_amd/fused.py).  Inputs: the device's dumps z_l (saved_tensors), the
tables, the fp32 master parameters, grad_out.  The backward differentiates act(LN(z_l)) at the DUMPED rows (erf GELU,
csrc/mlp_common.h act_grad / act_val_grad).
    g = bf16(grad_out)                                                                        :1954
    last layer (:1959, csrc/ln_act.hip:164-176): dz_{n-1} = bf16(dLN(act'(y) g)); dgamma, dbeta and dbias are fp32 sums
        of the UNROUNDED values (s_dz += o before st_row4 rounds)
    boundary l, fused (:1967-1973, csrc/mlp_bwd_bf16.hip:241-320): da = dz_l bf16(W_l) stays in the accumulators;
        a_{l-1} = bf16(act(LN(z_{l-1}))) (pack4(av), :270); dz_{l-1} = bf16(dLN(act'(y) da)) (pack4(o), :320);
        dW_l = dz_l^T a_{l-1} (:1971); db_l = wgrad_bf16's colsum: column sums of the ROUNDED dz_l (:1984) -- unless the
        boundary above was unfused and the row kernel already delivered it
    boundary l, unfused (:1975-1982): da = bf16(dz_l bf16(W_l)) (library GEMM, :1978); a_{l-1} from the row kernel;
        db_{l-1} from the row kernel, unrounded (:1988); the rest the same
    layer 0, gathered segment (:2001-2006): S = bf16(segment sum of dz_0) (csrc/segreduce_bf16.hip: fp32 sums, one
        rounding; column blocks of 512 above that width, :1722); dW[:, cols] = S^T table; d_table += bf16(S bf16(W_0)[:, cols]);
        a table used by two segments: autograd adds the two bf16 tensors in bf16
    layer 0, direct segment (:2007-2023): dW[:, cols] = dz_0^T table; db_0 = the colsum of the first direct segment
        (:2011) or else dz_0.float().sum(0) (:2026); d_direct = bf16(dz_0 bf16(W_0)[:, cols] (+ g when the skip is folded))
        (mlp_bwd_bf16.hip:168-170: one rounding after the add)
    a skip tensor that is not a segment gets g (:2028)
Every bf16 output comes with a SCALE array: |ref|, or the sum of the absolute values of the terms that met in bf16 (the
two gathers of one table, the folded skip).

Error measures and bars.  Parameter gradients: ln_ref.rel_err (normwise) and ln_ref.elem_err.  bf16 rows: the excess
    worst over elements of (|a - ref| - 2^-8 scale) / max|ref|.
Each bar is TWICE the worst figure of the float32 emulation (``emulate`` / ``emulate_forward``: ln_ref's emulated GEMM
with one rounding per 8 products, its emulated LayerNorm kernels, both summation orders) against the mirror over all cases
below -- the device's tie flips are another draw of the same process and the matrix instruction's internal alignment is
not measured.  Measured on the CPU (tests/test_bf16_train_ref.py::test_emulation_within_half_of_every_bar prints them):
    P_NORM_BAR  parameter gradient, normwise       worst 1.276e-3 (L512_unfused, L0.dW, order rev)   -> 2.56e-3
    P_ELEM_BAR  parameter gradient, element-wise   worst 7.07e-3  (L512_wide, L0.dW, order rev)      -> 1.42e-2
    D_ROW_BAR   bf16 row output, excess            worst 2.903e-3 (L512_wide, dT, order rev)         -> 5.81e-3
                (the forward alone: 1.97e-3, no_skip, out, order rev)
P_NORM_BAR is within the cap BF16_GRAD / 10 = 3e-3.  The two latent-512 cases run on seed 1: on seed 0 one tie flip on a
large element of dz_0 puts L512_unfused's L0.dW at 2.08e-3, outside what the cap allows the reference (1.5e-3); seeds
1..6 give 1.0e-3 .. 1.5e-3, seed 1 (1.28e-3) is their median.  At latent 128 the figure is 3e-4 .. 1e-3.
(tests/test_bf16_train_ref.py holds each bar to its figure from both sides: worst <= bar / 2 <= 1.05 worst.)
dgamma and dbeta of EVERY layer and dbias of the last layer are fp32 sums that never see a rounded row of their own layer
(the hidden layers' only feel the tie flips of the rows above through da).  Each (case, quantity) is held to
ln_ref.F32_BAR = 1e-4 wherever both emulation orders stay within half of it: everywhere (worst 3.9e-5, relu L0.dbeta; the
last layer's 5.5e-7) except the quantities of ``CLASS_BAR_QUANTS``, which fall under the class bars: relu L0.dgamma
(7.7e-5) and, on the unfused route, whose da is rounded once more, L512_unfused L0 / L1 dgamma and dbeta (0.9e-4 .. 4.7e-4).
The eps1e-3 case is cell2 with eps 1e-3 AND every W and b scaled by 2^-4 (ln_ref's eps1e-3 case does the same): at unit
scale the row variances are ~1 and eps 1e-3 against 1e-5 moves rstd by 5e-4 relative, which no bar rejects twofold: the
"eps_default" mutant would not be live.
"Bias from the rounded against the unrounded rows" (wgrad_bf16's colsum against the row kernel's sum) differs by 0.6e-3 ..
2.6e-3 normwise on these cases (2^-9 / sqrt 3 per row, which a sum of signed rows does not average out relative to
itself): around P_NORM_BAR at the most (silu_elu 2.58e-3 against 2.56e-3) and far inside P_ELEM_BAR, so it cannot be
rejected by a factor of 2 and is NOT a mutant; the mutants of ``MUTANTS`` are.
"""
import contextlib

import numpy as np
import torch

import act_ref as A
import bf16_mlp_ref as B
import ln_ref as R

P_NORM_BAR, P_ELEM_BAR, D_ROW_BAR = 2.56e-3, 1.42e-2, 5.81e-3
P_NORM_CAP = 3e-2 / 10                      # BF16_GRAD / 10 (tests/test_gpu_bf16_train.py)
F32_BAR = R.F32_BAR
N_TAB = 97
GELU, TANH, RELU, SILU, ELU, SIGMOID = R.ACT_GELU, R.ACT_TANH, R.ACT_RELU, A.ACT_SILU, A.ACT_ELU, A.ACT_SIGMOID
RELU_GUARD = 1e-3

_r_act64, _r_act_grad64 = R.act64, R.act_grad64


def act64(y, act, kernel_gelu=False):
    if act in A.NEW_CODES:
        return A.act64(y, act)
    if act == GELU and kernel_gelu:
        return B.gelu_kernel64(y)
    return _r_act64(y, act)


def act_grad64(y, act):
    return A.act_grad64(y, act) if act in A.NEW_CODES else _r_act_grad64(y, act)


@contextlib.contextmanager
def _emul_acts(kernel_gelu):
    """inside the block ln_ref's float32 emulations know every activation code (and the forward kernel's GELU)"""
    R.act64 = lambda y, act: act64(y, act, kernel_gelu)
    R.act_grad64 = act_grad64
    try:
        yield
    finally:
        R.act64, R.act_grad64 = _r_act64, _r_act_grad64


def ln_act_forward64(z, gm, bt, act, eps, kernel_gelu=False):
    mean, rstd = R.ln_stats64(z, eps)
    return act64((z - mean) * rstd * gm + bt, act, kernel_gelu)


def ln_act_backward64(z, g, gm, bt, act, eps):
    """(dz, dgamma, dbeta, rows dz for the bias sum) of act(LN(z)), float64"""
    mean, rstd = R.ln_stats64(z, eps)
    xh = (z - mean) * rstd
    dy = g * act_grad64(xh * gm + bt, act)
    gg = dy * gm
    dz = rstd * (gg - gg.mean(dim=1, keepdim=True) - xh * (gg * xh).mean(dim=1, keepdim=True))
    return dz, (dy * xh).sum(0), dy.sum(0)


# --------------------------------------------------------------------------------------------------------------- cases
def _spec(widths, segs, skip, acts, eps=1e-5, M=R.M_ROWS, no_grad=(), wide=None, ones=False, autocast=False, scale_exp=0, seed=0):
    return dict(seed=seed, widths=list(widths), segs=list(segs), skip=skip, acts=list(acts), eps=eps, M=M, no_grad=tuple(no_grad),
                wide=wide, ones=ones, autocast=autocast, scale_exp=scale_exp)


_CELL = [("T", "i0"), ("T", "i1"), ("D", None)]
_W2, _W3 = [384, 256, 128], [384, 256, 256, 128]
SPECS = {
    "cell2": _spec(_W2, _CELL, "D", [GELU, TANH]),
    "cell3": _spec(_W3, _CELL, "D", [GELU, GELU, GELU]),
    "m_edges_M1": _spec(_W2, _CELL, "D", [GELU, TANH], M=1),
    "m_edges_M63": _spec(_W2, _CELL, "D", [GELU, TANH], M=63),
    "m_edges_M64": _spec(_W2, _CELL, "D", [GELU, TANH], M=64),
    "m_edges_M65": _spec(_W2, _CELL, "D", [GELU, TANH], M=65),
    "no_skip": _spec(_W2, _CELL, None, [GELU, TANH]),
    "foreign_skip": _spec(_W2, _CELL, "S", [GELU, TANH]),
    "all_gathered": _spec([256, 256, 128], [("T", "i0"), ("U", "i1")], None, [GELU, TANH]),
    "direct_first": _spec([256, 256, 128], [("D", None), ("T", "i0")], "D", [GELU, TANH]),
    "no_grad_inputs": _spec(_W2, _CELL, "D", [GELU, TANH], no_grad=("T", "D")),
    "single256": _spec([256, 256], [("D", None)], "D", [GELU]),
    "eps1e-3": _spec(_W2, _CELL, "D", [GELU, TANH], eps=1e-3, scale_exp=-4),
    "relu": _spec(_W3, _CELL, "D", [RELU, RELU, GELU]),
    "silu_elu": _spec(_W3, _CELL, "D", [SILU, ELU, SIGMOID]),
    "L512_unfused": _spec([1536, 1024, 1024, 512], _CELL, "D", [GELU, GELU, GELU], wide=False, seed=1),
    "L512_wide": _spec([1536, 1024, 1024, 512], _CELL, "D", [GELU, GELU, GELU], wide=True, seed=1),
    "L256": _spec([768, 512, 256], _CELL, "D", [GELU, TANH]),
    "ones_grad": _spec(_W2, _CELL, "D", [GELU, TANH], ones=True),
    "autocast": _spec(_W2, _CELL, "D", [GELU, TANH], autocast=True),
}
CASES = tuple(SPECS)
# the bit equalities of the case table: name -> the case whose inputs and parameters it shares
SAME_BITS_AS = {"no_grad_inputs": "cell2", "autocast": "cell2"}

_built = {}


def build(name):
    """the tensors of a case (float32 CPU; tables and rows bf16-exact, parameters fp32 masters that are NOT bf16-exact),
    seeded by the widths and M alone so that cases sharing both share every tensor.  Biases carry the offset
    ln_ref.R_BF16_TRAIN sigma_l as ln_ref.make_case's rR cases do.  -> dict(spec fields, tables {key: rows}, idx {key:
    int64}, layers [(W, b, gamma, beta, act)], r: the fp32 upstream gradient before ``grad_out`` masks it)"""
    if name in _built:
        return _built[name]
    s = SPECS[name]
    widths, M = s["widths"], s["M"]
    n = len(widths) - 1
    sw = widths[0] // len(s["segs"])
    assert sw * len(s["segs"]) == widths[0] and sw % 128 == 0
    g = torch.Generator().manual_seed(100003 * n + 131 * widths[0] + widths[-1] + 7 * M + 1000003 * s["seed"])
    cast = lambda t: t.bfloat16().float()   # noqa: E731
    tables = {"T": cast(torch.randn(N_TAB, sw, generator=g)), "U": cast(torch.randn(N_TAB, sw, generator=g)),
              "D": cast(torch.randn(M, sw, generator=g)), "S": cast(torch.randn(M, widths[-1], generator=g))}
    idx = {"i0": torch.randint(0, N_TAB, (M,), generator=g), "i1": torch.randint(0, N_TAB, (M,), generator=g)}
    layers = []
    for l in range(n):
        W = torch.randn(widths[l + 1], widths[l], generator=g) / widths[l] ** 0.5
        b = 0.2 * torch.randn(widths[l + 1], generator=g)
        gm = 1 + 0.2 * torch.randn(widths[l + 1], generator=g)
        bt = 0.2 * torch.randn(widths[l + 1], generator=g)
        sc = 2.0 ** s["scale_exp"]
        layers.append([W * sc, b * sc, gm, bt, s["acts"][l]])
    r = torch.randn(M, widths[-1], generator=g)
    case = dict(s, name=name, tables=tables, idx=idx, layers=layers, r=r, sw=sw, n=n)
    assert s["skip"] is None or tables[s["skip"]].shape[1] == widths[-1]
    # the offset: sigma_l = the mean row std of layer l's rows at offset 0 (a LayerNorm output does not depend on the
    # offset of its input row, so the layers above are unchanged by the offsets below)
    _, _, zhat = forward_mirror(case)
    for l in range(n):
        sigma = float(zhat[l].std(dim=1, unbiased=False).mean())
        layers[l][1] = (layers[l][1].double() + R.R_BF16_TRAIN * sigma).float()
    case["layers"] = [tuple(t) for t in layers]
    _built[name] = case
    return case


def concat(case):
    return torch.cat([case["tables"][k] if i is None else case["tables"][k][case["idx"][i]] for k, i in case["segs"]], dim=1)


def needs_grad(case, key):
    return key not in case["no_grad"]


def skip_folded(case):
    """the index of the direct segment the skip gradient is folded into (fused.py:1924-1930), or -1"""
    if case["skip"] is None or not needs_grad(case, case["skip"]):
        return -1
    for s_i, (k, i) in enumerate(case["segs"]):
        if i is None and k == case["skip"]:
            return s_i
    return -1


def bwd_layer_supported(K, N, wide):
    """hgnn_mlp_backward_layer_supported_bf16's rule and fused._bwd_layer_supported's switch, restated"""
    return K > 0 and K % 128 == 0 and N in (128, 256, 512, 1024) and (N != 1024 or bool(wide))


def fused_flags(case):
    """[l] -> boundary l (between layers l - 1 and l) takes the fused backward layer; entry 0 is unused"""
    w = case["widths"]
    return [False] + [bwd_layer_supported(w[l + 1], w[l], case["wide"]) for l in range(1, case["n"])]


def branches(case):
    """the branches of fused._FusedMLPTrainBf16._backward a case reaches, from its widths and switches alone"""
    w, flags, out = case["widths"], fused_flags(case), set()
    n = case["n"]
    out.update("fused_boundary" for f in flags[1:] if f)
    out.update("unfused_boundary" for f in flags[1:] if not f)
    for l in range(1, n):
        if flags[l]:
            out.add({128: "bwd_N128", 256: "bwd_N256", 512: "bwd_N512", 1024: "bwd_N1024"}[w[l]])
    direct = [s_i for s_i, (_, i) in enumerate(case["segs"]) if i is None]
    gathered = [s_i for s_i, (_, i) in enumerate(case["segs"]) if i is not None]
    bias0_from_rows = n == 1 or not flags[1]            # the row kernel of layer 0 delivered it
    if not bias0_from_rows:
        out.add("colsum_bias0" if direct else "fallback_bias")
    if gathered and w[1] > 512:
        out.add("column_blocks")
    if skip_folded(case) >= 0:
        out.add("folded_skip")
    if case["skip"] is None:
        out.add("no_skip")
    elif case["skip"] == "S":
        out.add("foreign_skip")
    if n == 1:
        out.add("n1")
    if direct and direct[0] != len(case["segs"]) - 1:
        out.add("direct_not_last")
    if len({k for k, i in case["segs"] if i is not None}) > 1:
        out.add("two_tables")
    tabs = [k for k, i in case["segs"] if i is not None]
    if any(tabs.count(k) > 1 and needs_grad(case, k) for k in tabs):
        out.add("two_gathers_one_table")
    if case["no_grad"]:
        out.add("no_grad")
    if case["ones"]:
        out.add("stride0_grad")
    if case["autocast"]:
        out.add("autocast")
    if case["eps"] != 1e-5:
        out.add("eps")
    return out


def routing(case):
    """the counter deltas of ONE forward + backward: fused.stats["fused_train_calls"], ["bwd_layer_calls"],
    ["library_dgrad_calls"] (fused.py:1709, :1979, :2015-2023: a direct segment that needs a gradient takes the input form of
    the backward layer wherever (H0, w_s) is supported, which holds for every case here)"""
    flags = fused_flags(case)
    direct = sum(1 for k, i in case["segs"] if i is None and needs_grad(case, k))
    assert all(bwd_layer_supported(case["widths"][1], case["sw"], case["wide"]) for _ in range(direct))
    return dict(fused_train_calls=1, bwd_layer_calls=sum(flags[1:]) + direct,
                library_dgrad_calls=sum(1 for f in flags[1:] if not f))


def grad_out(case, zs):
    """the fp32 upstream gradient of a case given the dumps it will be differentiated at: ones (``ones``), else the
    seeded rows; ReLU / LeakyReLU' jump at 0, so a row with a hidden pre-activation within RELU_GUARD of 0 gets no upstream
    gradient (rows are independent all the way down; the last layer's elements are masked one by one)"""
    if case["ones"]:
        return torch.ones_like(case["r"])
    r = case["r"].clone()
    for l, (W, b, gm, bt, act) in enumerate(case["layers"]):
        if act != RELU:
            continue
        y = ln_act_forward64(zs[l].double(), gm.double(), bt.double(), R.ACT_NONE, case["eps"])
        near = y.abs() < RELU_GUARD
        if l == case["n"] - 1:
            r[near] = 0.0
        else:
            r[near.any(dim=1)] = 0.0
    return r


# ------------------------------------------------------------------------------------------------------ forward mirror
def forward_mirror(case, rounding=True, kernel_gelu=True):
    """-> (out, [z_l], [zhat_l]) in float64: the result and the dumps as stored (rounded if ``rounding``) and the
    unrounded pre-LayerNorm rows (module docstring)"""
    rb = R.bf16_round if rounding else (lambda t: t)
    h = concat(case).double()
    zhat = []
    for l, (W, b, gm, bt, act) in enumerate(case["layers"]):
        z = h @ rb(W.double()).t() + b.double()
        zhat.append(z)
        a = ln_act_forward64(z, gm.double(), bt.double(), act, case["eps"], kernel_gelu)
        if l == case["n"] - 1:
            if case["skip"] is not None:
                a = a + case["tables"][case["skip"]].double()
            return rb(a), [rb(t) for t in zhat], zhat
        h = rb(a)


def emulate_forward(case, order):
    """the forward in float32 the way the feature-split kernel evaluates it -> (out, [z_l]) as stored"""
    r32 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).bfloat16().float().numpy()   # noqa: E731
    h = concat(case).numpy()
    zs = []
    with _emul_acts(True):
        for l, (W, b, gm, bt, act) in enumerate(case["layers"]):
            z = R.emul_gemm(h, r32(W.numpy()), b.numpy(), order, R.GROUP_MATRIX)
            zs.append(r32(z))
            a = R.emul_ln_act(z, gm.numpy(), bt.numpy(), act, case["eps"], "pooled", order)
            if l == case["n"] - 1:
                if case["skip"] is not None:
                    a = a + case["tables"][case["skip"]].numpy()
                return r32(a), zs
            h = r32(a)


# ----------------------------------------------------------------------------------------------------- backward mirror
MUTANTS = ("bias_sum_last_row_missing", "gathered_row_missing", "skip_omitted", "skip_twice", "col_not_advanced",
           "second_gather_overwrites", "eps_default", "a_prev_from_next_layer_ln")


def mutant_live(case, mutant, g):
    """the branch a mutant breaks is taken by the case (g: its upstream gradient -- the two mutants that lose the LAST
    row need that row to carry one, which the ReLU case's guard may have taken away)"""
    gathered = [(k, i) for k, i in case["segs"] if i is not None]
    last_row = bool(g[-1].abs().sum() > 0)
    if mutant == "bias_sum_last_row_missing":           # a bias from wgrad_bf16's colsum or from the fallback sum
        return last_row and bool(branches(case) & {"fused_boundary", "colsum_bias0", "fallback_bias"})
    if mutant == "gathered_row_missing":
        return bool(gathered) and last_row
    if mutant in ("skip_omitted", "skip_twice"):
        return skip_folded(case) >= 0
    if mutant == "col_not_advanced":
        return any(needs_grad(case, k) for k, _ in case["segs"][1:])
    if mutant == "second_gather_overwrites":
        return "two_gathers_one_table" in branches(case)
    if mutant == "eps_default":
        return case["eps"] != 1e-5
    if mutant == "a_prev_from_next_layer_ln":
        return any(case["widths"][l] == case["widths"][l + 1] for l in range(1, case["n"]))
    raise ValueError(mutant)


def _segsum64(dz, idx, rows, drop_last=False):
    S = torch.zeros(rows, dz.shape[1], dtype=torch.float64)
    if drop_last:
        dz, idx = dz[:-1], idx[:-1]
    return S.index_add_(0, idx, dz)


def mirror(case, zs, g, flags, rounding=True, mutant=None):
    """float64 mirror of the backward (module docstring).  zs: the dumps; g: grad_out before its rounding; flags:
    ``fused_flags``.  -> (params {"L<l>.dW" | ".db" | ".dgamma" | ".dbeta": tensor},
                          rows {"d<table key>": (ref, scale)}; a table that needs no gradient has no entry)"""
    rb = R.bf16_round if rounding else (lambda t: t)
    n, eps, layers = case["n"], case["eps"], case["layers"]
    if mutant == "eps_default":
        eps = 1e-5
    zs = [z.double() for z in zs]
    Wb = [rb(L[0].double()) for L in layers]
    gm = [L[2].double() for L in layers]
    bt = [L[3].double() for L in layers]
    acts = [L[4] for L in layers]
    g = rb(g.double())
    P, rows = {}, {}
    # the mutant loses the last row in wgrad_bf16's colsum and in the dz.float().sum(0) fallback, not in the row kernel
    colsum = (lambda t: t[:-1].sum(0)) if mutant == "bias_sum_last_row_missing" else (lambda t: t.sum(0))
    dzu, P[f"L{n - 1}.dgamma"], P[f"L{n - 1}.dbeta"] = ln_act_backward64(zs[n - 1], g, gm[n - 1], bt[n - 1], acts[n - 1], eps)
    P[f"L{n - 1}.db"] = dzu.sum(0)                        # the row kernel: unrounded rows
    dz = rb(dzu)
    for l in range(n - 1, 0, -1):
        da = dz @ Wb[l]
        if not flags[l]:
            da = rb(da)
        src = l if (mutant == "a_prev_from_next_layer_ln" and gm[l].numel() == gm[l - 1].numel()) else l - 1
        a_prev = rb(ln_act_forward64(zs[l - 1], gm[src], bt[src], acts[l - 1], eps))
        P[f"L{l}.dW"] = dz.t() @ a_prev
        if f"L{l}.db" not in P:
            P[f"L{l}.db"] = colsum(dz)                    # wgrad_bf16's colsum: rounded rows
        dzu, P[f"L{l - 1}.dgamma"], P[f"L{l - 1}.dbeta"] = ln_act_backward64(zs[l - 1], da, gm[l - 1], bt[l - 1], acts[l - 1], eps)
        if not flags[l]:
            P[f"L{l - 1}.db"] = dzu.sum(0)                # the row kernel again
        dz = rb(dzu)
    dW = torch.zeros_like(Wb[0])
    folded = skip_folded(case)
    col = 0
    first_gather = True
    for s_i, (key, ik) in enumerate(case["segs"]):
        tab = case["tables"][key].double()
        w_s = tab.shape[1]
        wc = 0 if (mutant == "col_not_advanced" and s_i > 0) else col
        W_s = Wb[0][:, wc:wc + w_s]
        if ik is not None:
            S = rb(_segsum64(dz, case["idx"][ik], tab.shape[0], mutant == "gathered_row_missing" and first_gather))
            first_gather = False
            dW[:, col:col + w_s] = S.t() @ tab
            if needs_grad(case, key):
                gt = rb(S @ W_s)
                if f"d{key}" in rows and mutant != "second_gather_overwrites":
                    prev, sc = rows[f"d{key}"]
                    rows[f"d{key}"] = (rb(prev + gt), sc + gt.abs())
                else:
                    rows[f"d{key}"] = (gt, gt.abs())
        else:
            dW[:, col:col + w_s] = dz.t() @ tab
            if "L0.db" not in P:
                P["L0.db"] = colsum(dz)
            if needs_grad(case, key):
                v = dz @ W_s
                sc = v.abs()
                if folded == s_i and mutant != "skip_omitted":
                    v, sc = v + g * (2 if mutant == "skip_twice" else 1), sc + g.abs()
                assert f"d{key}" not in rows
                rows[f"d{key}"] = (rb(v), sc)
        col += w_s
    if "L0.db" not in P:
        P["L0.db"] = colsum(dz)                           # dz.float().sum(0): the same rows, another order
    P["L0.dW"] = dW
    if case["skip"] is not None and folded < 0 and needs_grad(case, case["skip"]):
        rows[f"d{case['skip']}"] = (g, g.abs())
    return P, rows


def bias_from_unrounded_rows(case, zs, g, flags):
    """NOT a mutant (module docstring): every colsum bias gradient taken from the unrounded rows -> {name: tensor}"""
    n, eps = case["n"], case["eps"]
    L = case["layers"]
    gd = R.bf16_round(g.double())
    out = {}
    dzu = ln_act_backward64(zs[n - 1].double(), gd, L[n - 1][2].double(), L[n - 1][3].double(), L[n - 1][4], eps)[0]
    for l in range(n - 1, 0, -1):
        dz = R.bf16_round(dzu)
        da = dz @ R.bf16_round(L[l][0].double())
        if not flags[l]:
            da = R.bf16_round(da)
        out[f"L{l}.db"] = dzu.sum(0)
        dzu = ln_act_backward64(zs[l - 1].double(), da, L[l - 1][2].double(), L[l - 1][3].double(), L[l - 1][4], eps)[0]
    out["L0.db"] = dzu.sum(0)
    return out


# ---------------------------------------------------------------------------------------------------- float32 emulation
def _r32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def _mm32(x, w, order):
    """x [M, K] w [K, N] -> [M, N] the way the matrix-pipe kernels accumulate: from zero, one rounding per 8 products"""
    return R.emul_gemm(x, np.ascontiguousarray(w.T), np.zeros(w.shape[1], np.float32), order, R.GROUP_MATRIX)


def _colsum32(v, order):
    v = np.asarray(v, np.float32)
    return (v if order == "fwd" else v[::-1]).cumsum(0, dtype=np.float32)[-1]


def _segsum32(dz, idx, rows, order):
    S = np.zeros((rows, dz.shape[1]), np.float32)
    ii = idx.numpy()
    rng = range(len(ii)) if order == "fwd" else range(len(ii) - 1, -1, -1)
    for r in rng:
        S[ii[r]] += dz[r]
    return S


def emulate(case, zs, g, flags, order):
    """the same chain in float32 (ln_ref's emulated kernels), ``order`` in ("fwd", "rev") -> (params, rows) of arrays"""
    assert order in ("fwd", "rev")
    n, eps, layers = case["n"], case["eps"], case["layers"]
    zs = [z.float().numpy() for z in zs]
    Wb = [_r32(L[0].numpy()) for L in layers]
    gm = [L[2].numpy() for L in layers]
    bt = [L[3].numpy() for L in layers]
    acts = [L[4] for L in layers]
    g = _r32(g.float().numpy())
    P, rows = {}, {}
    with _emul_acts(False):
        dzu, P[f"L{n - 1}.dgamma"], P[f"L{n - 1}.dbeta"], P[f"L{n - 1}.db"] = \
            R.emul_ln_act_backward(zs[n - 1], g, gm[n - 1], bt[n - 1], acts[n - 1], eps, order)
        dz = _r32(dzu)
        for l in range(n - 1, 0, -1):
            da = _mm32(dz, Wb[l], order)
            if not flags[l]:
                da = _r32(da)
            a_prev = _r32(R.emul_ln_act(zs[l - 1], gm[l - 1], bt[l - 1], acts[l - 1], eps,
                                        "pooled" if flags[l] else "centred", order))
            P[f"L{l}.dW"] = _mm32(dz.T, a_prev, order)
            if f"L{l}.db" not in P:
                P[f"L{l}.db"] = _colsum32(dz, order)
            dzu, P[f"L{l - 1}.dgamma"], P[f"L{l - 1}.dbeta"], dbias = \
                R.emul_ln_act_backward(zs[l - 1], da, gm[l - 1], bt[l - 1], acts[l - 1], eps, order)
            if not flags[l]:
                P[f"L{l - 1}.db"] = dbias
            dz = _r32(dzu)
    dW = np.zeros(Wb[0].shape, np.float32)
    folded = skip_folded(case)
    col = 0
    for s_i, (key, ik) in enumerate(case["segs"]):
        tab = case["tables"][key].numpy()
        w_s = tab.shape[1]
        W_s = Wb[0][:, col:col + w_s]
        if ik is not None:
            S = _r32(_segsum32(dz, case["idx"][ik], tab.shape[0], order))
            dW[:, col:col + w_s] = _mm32(S.T, tab, order)
            if needs_grad(case, key):
                gt = _r32(_mm32(S, W_s, order))
                rows[f"d{key}"] = _r32(rows[f"d{key}"] + gt) if f"d{key}" in rows else gt
        else:
            dW[:, col:col + w_s] = _mm32(dz.T, tab, order)
            if "L0.db" not in P:
                P["L0.db"] = _colsum32(dz, order)
            if needs_grad(case, key):
                v = _mm32(dz, W_s, order)
                rows[f"d{key}"] = _r32(v + g if folded == s_i else v)
        col += w_s
    if "L0.db" not in P:
        P["L0.db"] = _colsum32(dz, order)
    P["L0.dW"] = dW
    if case["skip"] is not None and folded < 0 and needs_grad(case, case["skip"]):
        rows[f"d{case['skip']}"] = g
    return P, rows


# ------------------------------------------------------------------------------------------------------------ measures
def row_excess(a, ref, scale):
    """worst over the elements of (|a - ref| - 2^-8 scale) / max|ref|"""
    a, ref, scale = (np.asarray(t, np.float64) for t in (a, ref, scale))
    return float(((np.abs(a - ref) - R.BF16_ULP * scale) / max(np.abs(ref).max(), 1e-30)).max())


# (case, quantity) pairs of the fp32-sum candidates whose emulation leaves half of F32_BAR: decided on the CPU
# (tests/test_bf16_train_ref.py::test_f32_held_split asserts this very table), held to the class bars instead
CLASS_BAR_QUANTS = {"relu": ("L0.dgamma",), "L512_unfused": ("L0.dbeta", "L0.dgamma", "L1.dbeta", "L1.dgamma")}


def f32_candidate(case, name):
    """dgamma and dbeta of every layer, dbias of the last: fp32 sums of values no rounding of their own layer touched"""
    return name.endswith((".dgamma", ".dbeta")) or name == f"L{case['n'] - 1}.db"


def f32_held(case, name):
    """held to F32_BAR: a candidate that is not in the case's CLASS_BAR_QUANTS"""
    return f32_candidate(case, name) and name not in CLASS_BAR_QUANTS.get(case["name"], ())


def compare(case, got_P, got_rows, ref_P, ref_rows):
    """every quantity of a backward against the mirror -> [(name, measure, value, bar)]"""
    out = []
    assert set(got_P) == set(ref_P) and set(got_rows) == set(ref_rows), (sorted(got_P), sorted(ref_P), sorted(got_rows), sorted(ref_rows))
    for name in sorted(ref_P):
        a, b = np.asarray(got_P[name], np.float64), ref_P[name].numpy()
        assert a.shape == b.shape, (name, a.shape, b.shape)
        if f32_held(case, name):
            out.append((name, "rel", R.rel_err(a, b), F32_BAR))
        else:
            out.append((name, "rel", R.rel_err(a, b), P_NORM_BAR))
            out.append((name, "elem", R.elem_err(a, b), P_ELEM_BAR))
    for name in sorted(ref_rows):
        ref, scale = ref_rows[name]
        a = np.asarray(got_rows[name], np.float64)
        assert a.shape == tuple(ref.shape), (name, a.shape, ref.shape)
        out.append((name, "excess", row_excess(a, ref.numpy(), scale.numpy()), D_ROW_BAR))
    return out


def compare_forward(got_out, got_zs, ref_out, ref_zs):
    """out and every dump against the forward mirror, every element, at the row-output bar"""
    out = [("out", "excess", row_excess(got_out, ref_out.numpy(), ref_out.abs().numpy()), D_ROW_BAR)]
    for l, (a, b) in enumerate(zip(got_zs, ref_zs)):
        out.append((f"z{l}", "excess", row_excess(a, b.numpy(), b.abs().numpy()), D_ROW_BAR))
    return out


# ------------------------------------------------------------------------------- float64 autograd through torch.nn
_ACT_MOD = {GELU: torch.nn.GELU, TANH: torch.nn.Tanh, RELU: torch.nn.ReLU, SILU: torch.nn.SiLU, ELU: torch.nn.ELU,
            SIGMOID: torch.nn.Sigmoid}


def autograd64(case, g):
    """float64 torch autograd of net(concat(x)) (+ skip) through torch.nn modules for the upstream gradient g ->
    (params, rows {"d<key>": tensor}, [z_l]) -- the derivative the mirror without roundings must equal"""
    mods, lins, lns = [], [], []
    for W, b, gm, bt, act in case["layers"]:
        lin = torch.nn.Linear(W.shape[1], W.shape[0]).double()
        ln = torch.nn.LayerNorm(W.shape[0], eps=case["eps"]).double()
        with torch.no_grad():
            lin.weight.copy_(W)
            lin.bias.copy_(b)
            ln.weight.copy_(gm)
            ln.bias.copy_(bt)
        lins.append(lin)
        lns.append(ln)
        mods += [lin, ln, _ACT_MOD[act]()]
    net = torch.nn.Sequential(*mods)
    leaves = {k: t.double().requires_grad_(needs_grad(case, k)) for k, t in case["tables"].items()}
    x = torch.cat([leaves[k] if i is None else leaves[k][case["idx"][i]] for k, i in case["segs"]], dim=1)
    zs = []
    hooks = [lin.register_forward_hook(lambda m, i, o: zs.append(o.detach())) for lin in lins]
    out = net(x)
    for h in hooks:
        h.remove()
    if case["skip"] is not None:
        out = out + leaves[case["skip"]]
    out.backward(g.double())
    P = {}
    for l, (lin, ln) in enumerate(zip(lins, lns)):
        P[f"L{l}.dW"], P[f"L{l}.db"], P[f"L{l}.dgamma"], P[f"L{l}.dbeta"] = lin.weight.grad, lin.bias.grad, ln.weight.grad, ln.bias.grad
    rows = {f"d{k}": t.grad for k, t in leaves.items() if t.grad is not None}
    return P, rows, zs
