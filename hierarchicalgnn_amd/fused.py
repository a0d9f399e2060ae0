"""Fused gather -> concat -> [Linear -> LayerNorm -> act] x {2,3} -> (+skip) on MFMA:
``hgnn_mlp_forward_f32`` (csrc/mlp_fused.hip, fp32 rows) and ``hgnn_mlp_forward_bf16``
(csrc/mlp_fused_bf16.hip, bf16 rows).  Covers the cell networks, the encoders (small-K mode)
and the width-1 classifier heads; fp32 rows at every hidden width that is a multiple of 16 up to 512
(``hgnn_mlp_forward_f32_padded``: zero-padded parameters on the next instantiation of the template grid), networks
whose output is as wide as their hidden layers, single layers below 512 and networks of 4 to 8 layers
(``hgnn_mlp_forward_f32_square``, csrc/mlp_fused_square.hip; ``set_square``, ``_group_route``).
Activations: GELU, Tanh, ReLU, SiLU, LeakyReLU, ELU, Sigmoid at their constructor defaults (``_ACT``).  Networks without
LayerNorm (``layer_norm=False``): opt-in route ``f32_plain`` (``set_plain_layers``, ``hgnn_mlp_forward_f32_plain``).

``_route`` decides per call (``supported`` asks it); when it says no, ``concat_mlp`` evaluates the same
Sequential with HIP row gathers + library GEMMs (still on the GPU).  The fused kernel is
used whenever autograd is not recording: inference, and the first (no-grad) pass of every
reentrant ``torch.utils.checkpoint`` segment -- which is how the reference runs all of its
updates (Modules/gnn_utils.py:14-15).  When autograd records, the differentiable variant runs
(``_FusedMLPTrain``: the same kernel dumping the pre-LayerNorm outputs, backward = HIP
LayerNorm/activation row kernels + library GEMMs + segmented-reduce scatter; with ``set_bwd_layer_f32`` the data
gradients and the row passes of a layer boundary are one launch of ``hgnn_mlp_backward_layer_f32``); shapes it
does not cover take the library path.
"""
from __future__ import annotations

import contextlib
import contextvars
import ctypes
import os
import weakref
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib
from .plan import get_index32

# HGNN_ACT_* (include/hgnn_hip.h).  4..7 at their constructor defaults only (``_act_code``)
_ACT = {nn.GELU: 1, nn.Tanh: 2, nn.ReLU: 3, nn.SiLU: 4, nn.LeakyReLU: 5, nn.ELU: 6, nn.Sigmoid: 7}
_enabled = True
# The differentiable variant (kernel forward + hand-written backward).  With ATen elementwise kernels in
# the backward it was 2 % slower than autograd through the library path; with the one-pass HIP
# LayerNorm/activation kernels (csrc/ln_act.hip) and the first-layer gradients factored through a
# segment-reduced dz it is faster (L=256, M=2M cell step: 58 vs 122 ms checkpointed, 45 vs 92 ms
# without checkpointing) and is the default when autograd records.
_train_enabled = True
# library_calls: concat_mlp evaluated a Sequential with library GEMMs (no fused route); library_dgrad_calls: a data
# gradient of the bf16 training backward went through a library GEMM; bwd_layer_calls: launches of the fused backward
# layer; hybrid_train_calls: encoders under autograd on the fp32 first layer + bf16 tail (mlp.concat_mlp);
# bwd_layer_f32_calls: launches of the exact-fp32 fused backward layer (set_bwd_layer_f32).  Created on first use:
# split3_wgrad_calls / wgrad_f32_calls / narrow_wgrad_calls / library_wgrad_calls, the branch ``_atb`` took for a weight
# gradient; project_f32_calls / library_project_calls, the branch of a forward pre-projection; narrow_linear_calls /
# narrow_outer_calls / library_head_calls, a head's plain last Linear (``set_project_f32``, ``set_narrow_f32``).  While
# ``set_narrow_f32`` is on, library_dgrad_calls also counts a first-layer input gradient of the fp32 backward that stays
# on the library
# plain_calls: launches of hgnn_mlp_forward_f32_plain (``set_plain_layers``), no-grad and differentiable
# square_calls: launches of hgnn_mlp_forward_f32_square (hidden = output, single layers, the groups of a deep network)
stats = {"fused_calls": 0, "fused_train_calls": 0, "padded_calls": 0, "library_calls": 0, "library_dgrad_calls": 0,
         "bwd_layer_calls": 0, "hybrid_train_calls": 0, "bwd_layer_f32_calls": 0, "plain_calls": 0, "square_calls": 0}

# Dispatch switches.  The module-level ``_name`` variables below are the PROCESS DEFAULTS (what the ``set_*`` functions
# and the HGNN_* environment variables change).  ``options(...)`` overrides any of them for the current context only --
# a ``contextvars`` context, i.e. per thread / per asyncio task -- so two models served from two threads can run
# different arithmetic (``with fused.options(fp32_split3=False): model(x, g)``) without touching shared state.
_ctx_options = contextvars.ContextVar("hgnn_fused_options", default=None)
_ctx_training_forward = contextvars.ContextVar("hgnn_fused_training_forward", default=0)
_OPTION_NAMES = ("enabled", "train_enabled", "preproject", "preproject_bf16", "fp32_split3", "fp32_split3_train",
                 "bf16_split", "train_bf16_enabled", "strict", "split3_padded", "plain_layers", "square")


def _opt(name: str):
    o = _ctx_options.get()
    if o is not None and name in o:
        return o[name]
    return globals()["_" + name]


@contextlib.contextmanager
def options(**overrides):
    """Context-local dispatch overrides: ``enabled``, ``train_enabled``, ``preproject``, ``preproject_bf16``,
    ``fp32_split3``, ``fp32_split3_train``, ``bf16_split``, ``train_bf16_enabled``, ``strict``, ``split3_padded``,
    ``plain_layers`` (see ``set_plain_layers``), ``square`` (see ``set_square``).
    ``strict``: ``concat_mlp`` raises instead of evaluating a Sequential on the library path (see ``set_strict``).
    Nested contexts stack; nothing outside the ``with`` block (or in another thread) sees the change.
    NOTE for training: autograd runs the backward (and the recompute of reentrant checkpoints) on its own worker
    thread, which does NOT inherit this context -- switches that must hold during ``backward()`` (``fp32_split3_train``,
    ``train_enabled``, ``train_bf16_enabled``) are to be set as process defaults
    (``set_*`` functions / HGNN_* environment variables); ``options`` is for inference-side choices."""
    bad = set(overrides) - set(_OPTION_NAMES)
    if bad:
        raise TypeError(f"fused.options: unknown option(s) {sorted(bad)}; known: {_OPTION_NAMES}")
    merged = dict(_ctx_options.get() or {})
    merged.update(overrides)
    token = _ctx_options.set(merged)
    try:
        yield
    finally:
        _ctx_options.reset(token)


def set_enabled(flag: bool, train: bool = None):
    """switch the fused kernels off/on (A/B measurements, debugging); `train` separately switches the
    differentiable variant (default: follows `flag`)"""
    global _enabled, _train_enabled
    _enabled = bool(flag)
    _train_enabled = bool(train) if train is not None else bool(flag)


_strict = False


def set_strict(flag: bool) -> None:
    """Process default of the ``strict`` option: ``mlp.concat_mlp`` raises ``RuntimeError`` (naming the layer widths
    and dtypes) where it would otherwise leave the fused kernels and evaluate the Sequential with library GEMMs
    (counted in ``stats["library_calls"]``).  ``options(strict=True)`` is context-local and therefore covers the
    forwards of the calling thread; a backward -- and the recompute of a reentrant checkpoint -- runs on autograd's
    own thread, which only the process default set here reaches."""
    global _strict
    _strict = bool(flag)


def _act_code(act) -> int:
    """HGNN_ACT_* of an activation module at the parameters the kernels implement (the constructor defaults:
    erf GELU, LeakyReLU slope 0.01, ELU alpha 1.0), or 0"""
    code = _ACT.get(type(act), 0)
    if isinstance(act, nn.GELU) and getattr(act, "approximate", "none") != "none":
        return 0
    if isinstance(act, nn.LeakyReLU) and act.negative_slope != 0.01:
        return 0
    if isinstance(act, nn.ELU) and act.alpha != 1.0:
        return 0
    return code


def _parse(net: nn.Sequential):
    """[(Linear, LayerNorm or None, act_code)] or None if the Sequential is neither
    (Linear -> LayerNorm -> act) repeated nor -- the plain form, make_mlp with layer_norm=False -- (Linear -> act)
    repeated, either optionally ending in one plain Linear (a head).  A network that mixes the two is None"""
    mods = list(net)
    layers = []
    i = 0
    plain = len(mods) > 1 and not isinstance(mods[1], (nn.LayerNorm, nn.Linear))
    while i < len(mods):
        lin = mods[i]
        if not isinstance(lin, nn.Linear) or lin.bias is None:
            return None
        if i + 1 == len(mods):                       # plain last layer (output_activation=None)
            layers.append((lin, None, 0))
            break
        if plain:
            code = _act_code(mods[i + 1])
            if not code:
                return None
            layers.append((lin, None, code))
            i += 2
            continue
        if i + 2 >= len(mods):
            return None
        ln, act = mods[i + 1], mods[i + 2]
        if not isinstance(ln, nn.LayerNorm) or not _act_code(act):
            return None
        if not ln.elementwise_affine or ln.bias is None:
            return None
        layers.append((lin, ln, _ACT[type(act)]))
        i += 3
    return layers or None


def _is_plain(layers) -> bool:
    """``_parse``'s plain form: at least one activated layer, no LayerNorm anywhere"""
    return layers is not None and layers[0][2] != 0 and all(ln is None for _, ln, _ in layers)


_preproject = True
# bf16 split kernel: implemented and parity-tested, but measured SLOWER (L=256: 3.7 vs 2.7 ms; L=512: 9.6 vs
# 8.6 ms): the accumulator-layout gather of bf16 P rows is 32-byte pieces issued at the start of every
# 64-row tile, which costs more than the 2/3 of the first layer's MFMAs it saves at 16x the matrix rate.
_preproject_bf16 = None   # bf16 feature-split kernel: None = by shape (first-layer width >= 512, i.e. latent >= 256:
                          # kernel 2.33-2.42 vs 2.70-2.80 ms at latent 256, 7.1 vs 8.6 ms at latent 512 incl. the
                          # projection GEMMs; latent 128 is 7 % slower projected), True / False = forced (A/B, tests)


def set_preproject(flag: bool) -> None:
    """A/B switch: project gathered segments through their block of the first Linear before the kernel"""
    global _preproject
    _preproject = bool(flag)


def _projected_segments(segments, M):
    """which gathered segments to pre-project (hgnn_mlp_desc.n_pre): table[idx] enters the first Linear
    linearly, W_s table[idx[e]] = (table W_s^T)[idx[e]], so a table with few rows (nodes: N = M / 16.7) is
    projected once by an N-row GEMM and only gathered inside the kernel -- the edge network's first layer
    keeps K = L of its 3L input columns.  At least one segment must stay in the kernel's K loop."""
    if not _opt("preproject") or len(segments) < 2 or any(int(t.shape[1]) % 16 for t, _ in segments):
        return []
    cand = [i for i, (t, idx) in enumerate(segments) if idx is not None and 4 * int(t.shape[0]) <= M]
    cand = cand[:2]
    if len(cand) == len(segments):
        cand = cand[:-1]
    return cand


def _pad_rows(t: torch.Tensor, rows: int) -> torch.Tensor:
    """zero-pad the leading dimension to `rows` (padded parameters of a partial last layer)"""
    out = torch.zeros((rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    out[:t.shape[0]] = t
    return out


def _pad_grid(h: int) -> int:
    """the grid width P whose instantiation a hidden width ``h`` runs on (hgnn_mlp_forward_f32_padded): the smallest of
    32, 64, 128, 256 with 2P >= h; 0 = none"""
    if h % 16 or not 32 <= h <= 512:
        return 0
    return next(P for P in (32, 64, 128, 256) if 2 * P >= h)


def _square_grid(h: int) -> int:
    """the grid width P whose instantiation a square network of width ``h`` runs on (hgnn_mlp_forward_f32_square): the
    smallest of 32, 64, 128, 256 with P >= h; 0 = none"""
    if h % 16 or not 32 <= h <= 256:
        return 0
    return next(P for P in (32, 64, 128, 256) if P >= h)


def _padded_param(param, rows: int, cols: Optional[int] = None, kept_cols=None, k_cols: Optional[int] = None):
    """zero-padded copy of a Linear / LayerNorm parameter for hgnn_mlp_forward_f32_padded, cached per parameter object
    and version (``_cached``): a weight [out, in] -> [rows, cols] (first layer: only the column blocks ``kept_cols``,
    then ``k_cols`` = 16 columns in small-K mode), a vector [out] -> [rows]"""
    def make():
        t = param.detach()
        if t.dim() == 1:
            return _pad_rows(t, rows)
        if kept_cols is not None:
            t = torch.cat([t[:, c0:c1] for c0, c1 in kept_cols], dim=1)
        width = cols if cols is not None else (k_cols if k_cols is not None else int(t.shape[1]))
        out = torch.zeros((rows, width), dtype=t.dtype, device=t.device)
        out[:t.shape[0], :t.shape[1]] = t
        return out
    return _cached(param, ("f32_padded", rows, cols, kept_cols, k_cols), make)


# One function per kernel: the weight layout of layer ``l`` of ``n`` (modules ``lin``, ``ln``; ``raw``: their W, b, ln_w,
# ln_b, the Parameters themselves).  ``cols``: the column blocks that stay in the kernel's K loop (first layer with
# pre-projected segments, else None), ``K`` wide (= width[0]); ``small_k``: first layer, K <= 16 stored as one 16-column
# chunk; ``hidden``: the first layer's output width; ``P_grid`` (f32_padded): the grid width the network runs on.
# Returns (w0_cols, w_last_rows, make) -- the descriptor fields the layout implies (0 = none) and ``make()`` -> the
# prepared (W, b, ln_w, ln_b), which a dry descriptor skips -- or None when the kernel has no such layer.  Plain
# arguments and no work outside ``make``: this runs for every layer of every call.
def _layout_f32(l, n, lin, ln, raw, cols, K, small_k, hidden, P_grid):
    """fp32 weights as they are; zero padded where the kernel wants more than the layer has"""
    o, last, rows = int(lin.out_features), l == n - 1, 0
    if last and ln is None:
        # head (width-1 classifiers, emb_dim-wide embedding head): the plain last layer is stored zero-padded as 32 rows
        if o > 32:
            return None
        rows = 32
    elif last and n == 3 and o not in (32, 64, 128, 256) and hidden % 2 == 0:
        # narrower than its tile row (supernode encoder, L - emb_dim outputs): Linear / LayerNorm parameters
        # zero-padded to P = hidden / 2 rows; the kernel normalises over the real width
        rows = hidden // 2
        if not (rows - 16 < o < rows) or o % 4:
            return None
    elif n == 1 and ln is not None and 496 < o < 512 and o % 4 == 0:
        # the narrow last layer of a chain (supernode encoder at latent 512, 504 outputs): one single-layer launch on
        # parameters zero-padded to 512 rows, statistics and stores over the real width
        rows = 512

    return 16 if small_k else 0, rows, lambda: _f32_params(raw, cols, K, small_k, rows)


def _f32_params(raw, cols, K, small_k, rows):
    """the (W, b, ln_w, ln_b) the exact fp32 kernel reads (``_layout_f32``, ``_layout_f32_plain``): the kept column
    blocks of the first layer, small-K padding, a last layer zero padded to ``rows`` rows"""
    if not (cols or small_k or rows):
        return raw
    W = raw[0].detach()
    if cols:
        W = torch.cat([W[:, c0:c1] for c0, c1 in cols], dim=1).contiguous()
    if small_k:
        # small-K mode (encoders, K = 3 / 6): one zero-padded 16-column chunk
        W = torch.nn.functional.pad(W, (0, 16 - K)).contiguous()
    ps = (W,) + raw[1:]
    return ps if not rows else [p if p is None else _pad_rows(p.detach(), rows) for p in ps]


def _layout_f32_padded(l, n, lin, ln, raw, cols, K, small_k, hidden, P_grid):
    """widths between the grid's: every parameter zero padded to the instantiation of P_grid (layout:
    hgnn_mlp_supported_f32_padded in include/hgnn_hip.h); cached copies, the kernel's statistics, dumps and stores use
    the real widths in d.width"""
    last = l == n - 1
    rows = 32 if ln is None else (P_grid if last else 2 * P_grid)

    def make():
        W = _padded_param(lin.weight, rows, 2 * P_grid if l > 0 else None, cols, 16 if small_k else None)
        lnp = (None, None) if ln is None else (_padded_param(ln.weight, rows), _padded_param(ln.bias, rows))
        return (W, _padded_param(lin.bias, rows)) + lnp
    return 16 if small_k else 0, rows if last else 0, make


def _layout_f32_split3(l, n, lin, ln, raw, cols, K, small_k, hidden, P_grid):
    """the bf16 split stream of the fp32 weight"""
    if ln is None or small_k:
        return None
    return 0, 0, lambda: (_split3_weight(lin.weight, cols, l == 0),) + raw[1:]


def _layout_bf16(l, n, lin, ln, raw, cols, K, small_k, hidden, P_grid):
    """bf16 [out][in], layers >= 1 in k-slot column order"""
    if l > 0 and lin.in_features % 32:
        return None

    def make():
        W = raw[0].detach()
        return ((W[:, _kslot_perm(lin.in_features, W.device)] if l > 0 else W).to(torch.bfloat16).contiguous(),) + raw[1:]
    return 0, 0, make


def _layout_bf16_split(l, n, lin, ln, raw, cols, K, small_k, hidden, P_grid):
    """bf16 in A-fragment order"""
    if (K if cols else lin.in_features) % 32 or lin.out_features % 64:
        return None
    return 0, 0, lambda: (_prepared_weight(lin.weight, cols),) + raw[1:]


def _layout_f32_split3_padded(l, n, lin, ln, raw, cols, K, small_k, hidden, P_grid):
    """widths between the split-bf16 kernel's: the split stream of the weight zero padded to the instantiation of P_grid
    (layout: hgnn_mlp_supported_f32_split3_padded in include/hgnn_hip.h), zero-padded vectors; cached copies.  ``cols``:
    the column blocks of the kept segments (always given for the first layer: each is padded to whole panels)"""
    if ln is None or small_k:
        return None
    last = l == n - 1
    rows = P_grid if last else 2 * P_grid

    def make():
        W = _split3_padded_weight(lin.weight, rows, 2 * P_grid if l > 0 else None, cols)
        return (W, _padded_param(lin.bias, rows), _padded_param(ln.weight, rows), _padded_param(ln.bias, rows))
    return 0, rows if last else 0, make


def _layout_f32_plain(l, n, lin, ln, raw, cols, K, small_k, hidden, P_grid):
    """no LayerNorm on any layer (hgnn_mlp_forward_f32_plain): ``_layout_f32``'s storage -- a head's last Linear as 32
    rows, the narrow encoder's as hidden / 2 rows (here only a store mask)"""
    if ln is not None:
        return None
    o, last, rows = int(lin.out_features), l == n - 1, 0
    if last and n == 3 and hidden != 2 * o:
        if o <= 32:
            rows = 32
        elif hidden % 2 == 0 and hidden // 2 - 16 < o < hidden // 2 and o % 4 == 0:
            rows = hidden // 2
        else:
            return None
    return 16 if small_k else 0, rows, lambda: _f32_params(raw, cols, K, small_k, rows)


def _layout_f32_square(l, n, lin, ln, raw, cols, K, small_k, hidden, P_grid):
    """hidden = output (hgnn_mlp_supported_f32_square in include/hgnn_hip.h).  On the grid (hidden == P_grid) a layer as
    wide as the hidden ones is read as it is; every other layer -- all of them between the grid widths, the narrow last
    layer of the supernode encoder -- zero padded to P_grid rows, W[l >= 1] to P_grid columns (``_padded_param``)"""
    if ln is None:
        return None
    o, last = int(lin.out_features), l == n - 1
    if o != hidden and not (last and n == 3 and hidden - 16 < o < hidden and o % 4 == 0):
        return None
    if hidden == P_grid and o == hidden:
        return 16 if small_k else 0, 0, lambda: _f32_params(raw, cols, K, small_k, 0)

    def make():
        W = _padded_param(lin.weight, P_grid, P_grid if l > 0 else None, cols, 16 if small_k else None)
        return (W, _padded_param(lin.bias, P_grid), _padded_param(ln.weight, P_grid), _padded_param(ln.bias, P_grid))
    return 16 if small_k else 0, P_grid if last else 0, make


_LAYOUTS = {"f32": _layout_f32, "f32_square": _layout_f32_square, "f32_plain": _layout_f32_plain, "f32_padded": _layout_f32_padded, "f32_split3": _layout_f32_split3,
            "f32_split3_padded": _layout_f32_split3_padded, "bf16": _layout_bf16, "bf16_split": _layout_bf16_split}


def _preprojections(tables, cols, proj, lin0, bf16: bool, split_proj: bool, width: int):
    """{i: tables[i] W_i^T  [rows, H]} for i in ``proj`` (W_i: columns ``cols[i]`` of the first Linear), zero padded to
    ``width`` columns (f32_padded, f32_split3_padded: the padded W[0] rows).  ``split_proj``: by ``_split3_project`` where it has the shape;
    with ``set_project_f32`` fp32 tables go to ``_exact_project`` (hgnn_project_f32); what is left is ``torch.matmul``"""
    P = {}
    if split_proj and proj:
        # both segments of one table (nodes[graph[0]], nodes[graph[1]]) in one launch
        t0 = tables[proj[0]]
        same = len(proj) == 2 and tables[proj[1]].data_ptr() == t0.data_ptr() and tables[proj[1]].shape == t0.shape
        for grp in ([proj] if same else [[i] for i in proj]):
            res = _split3_project(tables[grp[0]].detach(), lin0.weight, [cols[i] for i in grp])
            if res is not None:
                P.update(zip(grp, res))
    if _project_f32_on and not bf16:
        # set_project_f32: the exact route's projections on hgnn_project_f32 (fp32 MFMA, k-ordered chains), both
        # segments of one table in one launch; the split-bf16 projection above keeps precedence
        rest = [i for i in proj if i not in P]
        same = len(rest) == 2 and tables[rest[1]].data_ptr() == tables[rest[0]].data_ptr() \
            and tables[rest[1]].shape == tables[rest[0]].shape
        for grp in ([rest] if same else [[i] for i in rest]):
            res = _exact_project(tables[grp[0]].detach(), lin0.weight, [cols[i] for i in grp], width)
            if res is not None:
                P.update(zip(grp, res))
    for i in proj:
        if i in P:
            continue
        stats["library_project_calls"] = stats.get("library_project_calls", 0) + 1
        W_s = lin0.weight.detach()[:, cols[i][0]:cols[i][1]]
        with torch.autocast("cuda", enabled=False):
            # the kernel reads P in its row dtype; bf16: bf16 operands, fp32 accumulation, one rounding -- the
            # arithmetic the kernel's own MFMAs would do
            P[i] = torch.matmul(tables[i].detach(), (W_s.to(torch.bfloat16) if bf16 else W_s).t())
        if width and int(P[i].shape[1]) < width:
            P[i] = torch.nn.functional.pad(P[i], (0, width - int(P[i].shape[1])))
    return P


def _descriptor(net, segments, skip, entry: str = "f32", split_proj: bool = False, dry: bool = False, layers=None):
    """(descriptor, keep-alive list, M, n_out) for ``hgnn_mlp_forward_<entry>`` (``entry`` in f32, f32_padded, f32_square,
    f32_split3, f32_split3_padded, bf16, bf16_split), or None.  ``layers``: ``_parse(net)`` when the caller has it (then ``net`` is not read).

    One walk for every kernel: the segments (one row count M, int32 gather indices, pre-projected segments
    ``hgnn_mlp_desc.n_pre`` vs the ones kept in the kernel's K loop), the layers (chained widths, one LayerNorm eps)
    and the skip rows.  What depends on the kernel: the row dtype, which segments are pre-projected (fp32: by
    ``_projected_segments``; bf16: only for the split kernel, by ``preproject_bf16``, P rounded once to bf16) and the
    weight layout of each layer (``_LAYOUTS[entry]``).  ``dry``: only decide supportability (no projection GEMM or
    weight preparation runs: the tables and the module's own parameters stand in; the descriptor must not be launched).
    ``split_proj`` (f32_split3): the N-row projection GEMMs use the consuming kernel's arithmetic
    (hgnn_project_f32_split3, three products) instead of the library's fp32 GEMM."""
    bf16 = entry.startswith("bf16")
    dt = torch.bfloat16 if bf16 else torch.float32
    layers = _parse(net) if layers is None else layers
    if layers is None or not (1 <= len(layers) <= 3 and 1 <= len(segments) <= 3):
        return None
    if (entry != "f32_plain" and any(ln is None for _, ln, _ in (layers if bf16 else layers[:-1]))) \
            or any(t.dim() != 2 or not t.is_cuda or t.dtype != dt for t, _ in segments):
        return None
    M, *more = {int(i.numel()) if i is not None else int(t.shape[0]) for t, i in segments}
    ws = [int(t.shape[1]) for t, _ in segments]
    lin0 = layers[0][0]
    if more or lin0.in_features != sum(ws) or not lin0.weight.is_cuda:
        return None
    hidden = int(lin0.out_features)
    padded = entry in ("f32_padded", "f32_split3_padded")
    P_grid = _pad_grid(hidden) if padded else 0
    if padded and (P_grid == 0 or len(layers) < 2):
        return None
    pre_width = 2 * P_grid                     # columns of a pre-projected segment's rows: the padded W[0] rows
    if entry == "f32_square":
        pre_width = P_grid = _square_grid(hidden)
        if P_grid == 0:
            return None
    if bf16:
        pre = _opt("preproject_bf16")
        pre = entry == "bf16_split" and (len(layers) > 1 and hidden >= 512 if pre is None else pre)
    else:
        pre = layers[0][1] is not None or entry == "f32_plain"
    proj = _projected_segments(segments, M) if pre else []
    tables = [t if t.is_contiguous() else t.contiguous() for t, _ in segments]
    cols = [(sum(ws[:i]), sum(ws[:i + 1])) for i in range(len(ws))]
    pre_rows = _preprojections(tables, cols, proj, lin0, bf16, split_proj, pre_width) if proj and not dry else {}
    d = _lib.HgnnMlpDesc()
    keep = []
    n_kept = n_pre = 0
    for i, (t, (_, index)) in enumerate(zip(tables, segments)):
        i32 = None if index is None else get_index32(index, int(t.shape[0]))
        i_ptr = i32.data_ptr() if i32 is not None and i32.numel() else None
        keep += [t] if i32 is None else [t, i32]
        if i in proj:
            P = pre_rows.get(i, t)
            keep.append(P)
            d.pre_table[n_pre], d.pre_index[n_pre] = P.data_ptr(), i_ptr
            n_pre += 1
        else:
            d.seg_table[n_kept], d.seg_index[n_kept], d.seg_width[n_kept] = t.data_ptr(), i_ptr, ws[i]
            n_kept += 1
    d.n_seg, d.n_pre = n_kept, n_pre
    # the kernel's K loop only sees the kept segments
    # (f32_split3_padded pads every kept segment's block to whole panels: it is told the blocks in any case)
    kept_cols = tuple(c for i, c in enumerate(cols) if i not in proj) if proj or entry == "f32_split3_padded" else None
    n = d.n_layers = len(layers)
    o_l = K = d.width[0] = sum(ws) - sum(ws[i] for i in proj)
    small_k = not bf16 and any(w % 16 for w in ws)
    if small_k and K > 16:
        return None
    eps = None
    for l, (lin, ln, act) in enumerate(layers):
        if l > 0 and lin.in_features != o_l:
            return None
        # the Parameters themselves: only a layout that re-lays one out detaches it
        raw = (lin.weight, lin.bias) + ((None, None) if ln is None else (ln.weight, ln.bias))
        if not raw[0].is_cuda:
            return None
        for p in () if bf16 else raw:             # fp32 kernels: the parameters as they are
            if p is not None and (not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous()):
                return None
        if bf16:                                  # the bf16 kernels read bias and LayerNorm parameters in fp32
            raw = raw[:1] + tuple(p.detach().float().contiguous() for p in raw[1:])
        lay = _LAYOUTS[entry](l, n, lin, ln, raw, kept_cols if l == 0 else None, K, small_k and l == 0, hidden, P_grid)
        if lay is None:
            return None
        if lay[0]:
            d.w0_cols = lay[0]
        if lay[1]:
            d.w_last_rows = lay[1]
        W, b, lnw, lnb = raw if dry else lay[2]()
        keep += [W, b, lnw, lnb]
        d.W[l], d.b[l] = W.data_ptr(), b.data_ptr()
        if ln is not None:
            d.ln_w[l], d.ln_b[l] = lnw.data_ptr(), lnb.data_ptr()
            if eps is None:
                eps = ln.eps
            elif eps != ln.eps:
                return None
        o_l = d.width[l + 1] = int(lin.out_features)
        d.act[l] = act
    d.ln_eps = float(eps) if eps is not None else 0.0     # f32_plain: not read
    n_out = int(d.width[n])
    if skip is not None:
        if tuple(skip.shape) != (M, n_out) or not skip.is_cuda or skip.dtype != dt:
            return None
        sk = skip if skip.is_contiguous() else skip.contiguous()
        keep.append(sk)
        d.skip = sk.data_ptr()
    d.M = M
    return d, keep, M, n_out


def _kslot_perm(k: int, device) -> torch.Tensor:
    """column order of W_{l>=1} for the bf16 kernel: slot 32c+8g+j <- feature 32c+(j<4 ? 4g+j : 16+4g+j-4)"""
    c = torch.arange(k // 32, device=device).view(-1, 1, 1) * 32
    g = torch.arange(4, device=device).view(1, -1, 1)
    j = torch.arange(8, device=device).view(1, 1, -1)
    feat = c + torch.where(j < 4, 4 * g + j, 16 + 4 * g + j - 4)
    return feat.reshape(-1)


def _fragment_order(W: torch.Tensor) -> torch.Tensor:
    """bf16 W[F, K] in MFMA A-fragment order (include/hgnn_hip.h, hgnn_mlp_forward_bf16_split):
    [k-chunk c][16-feature tile T][lane = 16*(k-group) + row][8 values]"""
    F, K = W.shape
    return W.view(F // 16, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4).contiguous()


class _WeightCache:
    """prepared (re-laid-out / bf16 / split) copies of Linear weights, one per (weight object, layout).

    Validity = same Parameter OBJECT (held by weak reference: a deleted model frees its entries), same storage
    address and same in-place version counter.  ``optimizer.step()``, ``load_state_dict`` and every other in-place op
    on the parameter bump that counter.  Writes through ``param.data`` (``p.data.normal_()``, hand-written
    ``p.data -= lr * g``, EMA / SWA swaps) do NOT -- PyTorch gives ``.data`` a version counter of its own -- so:
      * the Sequentials built by ``utils.make_mlp`` drop their entries in ``train()`` / ``eval()`` / ``to()`` /
        ``load_state_dict`` (``FusedMLPSequential``), and
      * code that edits ``.data`` between two forwards without any of these calls ``fused.clear_weight_cache()``.
    """

    def __init__(self):
        self._d = {}

    def get(self, weight, tag):
        try:
            ver = weight._version
        except RuntimeError:              # inference tensors carry no version counter: never cached
            return None
        e = self._d.get((id(weight), tag))
        if e is not None and e[0]() is weight and e[1] == ver and e[2] == weight.data_ptr():
            return e[3]
        return None

    def put(self, weight, tag, value):
        try:
            ver = weight._version
        except RuntimeError:
            return
        key = (id(weight), tag)
        try:
            ref = weakref.ref(weight, lambda _r, k=key, d=self._d: d.pop(k, None))
        except TypeError:
            return
        self._d[key] = (ref, ver, weight.data_ptr(), value)

    def drop(self, weights):
        ids = {id(w) for w in weights}
        for k in [k for k in self._d if k[0] in ids]:
            self._d.pop(k, None)

    def clear(self):
        self._d.clear()

    def __len__(self):
        return len(self._d)


_wcache = _WeightCache()


def clear_weight_cache(module: Optional[nn.Module] = None) -> None:
    """forget the prepared weight copies (of ``module``'s parameters, or all).  Needed only after editing weights
    through ``param.data`` -- every in-place op on the parameter itself is detected (see ``_WeightCache``)."""
    if module is None:
        _wcache.clear()
    else:
        _wcache.drop(list(module.parameters()))


def _cached(weight, tag, make):
    """``make()``, cached per weight object, version and layout ``tag`` (``_WeightCache``): an inference forward
    re-lays out nothing, a training step once per optimizer update instead of once per call (forward + checkpoint
    recompute); a new version replaces the old copy"""
    hit = _wcache.get(weight, tag)
    if hit is None:
        hit = make()
        _wcache.put(weight, tag, hit)
    return hit


def _prepared_weight(weight, kept_cols):
    """bf16 copy of a Linear weight (optionally only the column blocks of the segments that stay in the kernel's K
    loop) in the kernel's fragment order"""
    def make():
        W = weight.detach()
        if kept_cols is not None:
            W = torch.cat([W[:, c0:c1] for c0, c1 in kept_cols], dim=1)
        return _fragment_order(W.to(torch.bfloat16).contiguous())
    return _cached(weight, ("_fragment_order", kept_cols), make)


_fp32_split3 = os.environ.get("HGNN_FP32_SPLIT3", "1") != "0"


_fp32_split3_train = os.environ.get("HGNN_FP32_SPLIT3_TRAIN", "0") == "1"


def set_fp32_split3_training(flag: bool) -> None:
    """OPT-IN (HGNN_FP32_SPLIT3_TRAIN=1): the split-bf16 arithmetic also under autograd -- the differentiable forward
    with its pre-LayerNorm dumps (hgnn_mlp_forward_f32_split3), the M-row data gradients dz.W (hgnn_linear_f32_split3,
    four products) and weight gradients dz^T a (hgnn_wgrad_f32_split3) of the backward.  EC-IN fp32 training step at
    latent 256: 883 -> 568 ms, latent 128 285 -> 235 ms, config 3 744 -> 486 ms.  Every gradient bar of the GPU suite
    holds with it on (269 passed), normwise with >= 6x margin, but the ELEMENT-WISE 1e-4 bar only by 3-7 % on two
    fixtures (9.3e-5 on one weight gradient of the latent-256 HGNN cell, 7.8e-5 on config 2's input gradient): by
    default gradients are therefore computed on the exact fp32 path and only no-grad forwards (inference, and the
    no-grad pass of a reentrant checkpoint) use split-bf16."""
    global _fp32_split3_train
    _fp32_split3_train = bool(flag)


def set_fp32_split3(flag: bool) -> None:
    """The forwards of the fp32 MLPs at latent 128 / 256 (node / edge / supernode / superedge networks, the hidden layers
    of the score heads; inference and the forward passes of a training step) evaluate their GEMMs as split-bf16
    products on the bf16 matrix pipe (hgnn_mlp_forward_f32_split3: hi.hi + mid.hi + hi.mid, exact products, fp32
    accumulation; rows, LayerNorm, activations, skip in fp32): <= 1.6e-5 against the reference at every checked stage
    of BASELINE configs 2 and 3, inside north_star's 1e-4, and the whole GPU parity suite holds with it on.
    DEFAULT ON for no-grad forwards (set_fp32_split3_training switches it on under autograd too); ``set_fp32_split3(False)``, ``HGNN_FP32_SPLIT3=0`` or ``hparams["fp32_gemm"] = "exact"`` select the
    exact fp32 matrix instruction (fmaf-chain arithmetic) instead."""
    global _fp32_split3
    _fp32_split3 = bool(flag)


class training_forward:
    """context: the enclosed no-grad evaluation belongs to a TRAINING step (the first pass of a reentrant
    ``torch.utils.checkpoint`` segment, gnn_utils._maybe_checkpoint).  The split-bf16 evaluation of the fp32 MLPs is an
    INFERENCE default; inside this context a no-grad forward uses exactly what the recompute under autograd will use
    (the exact fp32 kernels, or split-bf16 everywhere with set_fp32_split3_training(True)): forward values and the
    point the gradients are taken at agree bitwise, as with the reference's own recompute.  Context-local
    (``contextvars``): a training step in one thread does not change what an inference call in another thread runs."""

    def __enter__(self):
        self._token = _ctx_training_forward.set(_ctx_training_forward.get() + 1)

    def __exit__(self, *exc):
        _ctx_training_forward.reset(self._token)
        return False


def _split3(net, train: bool = False) -> bool:
    """the GEMMs of the fp32 MLP ``net`` are evaluated as split-bf16 products (hgnn_*_f32_split3).  ``train``: the
    differentiable forward and the backward GEMMs.  First match wins:
      1. under autograd (``train``) and in the no-grad pass of a checkpointed training step (``training_forward``): off
         unless ``fp32_split3_train`` (set_fp32_split3_training, HGNN_FP32_SPLIT3_TRAIN=1);
      2. an ``fp32_split3`` override of the current ``options`` context;
      3. the module's own mark, ``hparams["fp32_gemm"]`` (``net._hgnn_split3``, models._mark_split3);
      4. the process default (set_fp32_split3, HGNN_FP32_SPLIT3)."""
    if (train or _ctx_training_forward.get() > 0) and not _opt("fp32_split3_train"):
        return False
    o = _ctx_options.get()
    if o is not None and "fp32_split3" in o:
        return bool(o["fp32_split3"])
    flag = getattr(net, "_hgnn_split3", None)
    return _fp32_split3 if flag is None else bool(flag)


def _split3_stream(W: torch.Tensor) -> torch.Tensor:
    """fp32 W [F, K] (F % 16 == 0, K % 32 == 0) as its bf16 split stream in A-fragment order"""
    hi = W.to(torch.bfloat16)
    mid = (W - hi.float()).to(torch.bfloat16)
    F, K = W.shape
    # per 32-wide k-chunk: the chunk's W_hi columns, then its W_mid columns (virtual chunks 2c, 2c + 1)
    Wv = torch.stack([hi.view(F, K // 32, 32), mid.view(F, K // 32, 32)], dim=2).reshape(F, 2 * K)
    return _fragment_order(Wv.contiguous())


def _split3_weight(weight, kept_cols, panels: bool, transpose: bool = False):
    """bf16 split stream of an fp32 Linear weight (per 32-wide k-chunk of the kept columns: W_hi, then W_mid) in
    A-fragment order, cached per weight object and version (``_cached``)"""
    def make():
        W = weight.detach().float()
        if kept_cols is not None:
            W = torch.cat([W[:, c0:c1] for c0, c1 in kept_cols], dim=1)
        if transpose:
            W = W.t().contiguous()
        return _split3_stream(W)
    return _cached(weight, ("split3", kept_cols, panels, transpose), make)


def _split3_padded_weight(weight, rows: int, cols: Optional[int], kept_cols):
    """``_split3_weight``'s stream of the zero-padded weight (hgnn_mlp_forward_f32_split3_padded): [out, in] -> ``rows``
    rows; first layer (``kept_cols``): every kept column block padded to the next multiple of 128 columns; other layers:
    ``cols`` columns.  Cached per weight object and version under its own key"""
    def make():
        W = weight.detach().float()
        if kept_cols is not None:
            W = torch.cat([torch.nn.functional.pad(W[:, c0:c1], (0, -(c1 - c0) % 128)) for c0, c1 in kept_cols], dim=1)
        width = cols if cols is not None else int(W.shape[1])
        out = torch.zeros((rows, width), dtype=W.dtype, device=W.device)
        out[:W.shape[0], :W.shape[1]] = W
        return _split3_stream(out)
    return _cached(weight, ("split3_padded", rows, cols, kept_cols), make)


_plain_layers = os.environ.get("HGNN_MLP_PLAIN", "0") == "1"


def set_plain_layers(flag: bool) -> None:
    """OPT-IN (HGNN_MLP_PLAIN=1, ``options(plain_layers=True)``): fp32 networks WITHOUT LayerNorm (make_mlp with
    layer_norm=False, ``layernorm: False`` in a config) run on the exact fp32 kernel's plain form
    (hgnn_mlp_forward_f32_plain: each layer act(x W^T + b)) at the shapes the LayerNorm'ed networks have there -- cell
    networks and encoders at latent 32 / 64 / 128 / 256, the K -> H -> H -> w heads, the narrow supernode encoder.
    Under autograd the same kernel dumps the pre-activation rows and the backward uses hgnn_act_rows_backward_f32 and
    the GEMMs of the LayerNorm'ed path (``set_wgrad_f32`` / ``set_narrow_f32`` apply; ``set_bwd_layer_f32`` does not:
    the fused backward layer has no plain form).  bf16 rows, the padded widths, latent 512 and the split-bf16
    arithmetic have no plain form and keep the library path.  A backward and the recompute of a reentrant checkpoint run
    on autograd's own thread, which only the process default set here reaches.  Default off."""
    global _plain_layers
    _plain_layers = bool(flag)


def _plain_layers_on() -> bool:
    return bool(_opt("plain_layers"))


_split3_padded = os.environ.get("HGNN_SPLIT3_PADDED", "0") == "1"


def set_split3_padded(flag: bool) -> None:
    """OPT-IN (HGNN_SPLIT3_PADDED=1, ``options(split3_padded=True)``): no-grad forwards of the fp32 cell networks at
    widths BETWEEN the split-bf16 kernel's (hidden width in (128, 512], e.g. latent 96, 144, 160, 192) run the split-bf16
    arithmetic on zero-padded parameters (hgnn_mlp_forward_f32_split3_padded) instead of the exact fp32 kernel on them
    (hgnn_mlp_forward_f32_padded).  Only where the split-bf16 arithmetic applies at all (``_split3``): a module pinned
    with ``hparams["fp32_gemm"] = "exact"``, a ``training_forward`` and every call autograd records keep the exact
    kernel.  Default off."""
    global _split3_padded
    _split3_padded = bool(flag)


def _split3_linear(x: torch.Tensor, weight, cols, net) -> Optional[torch.Tensor]:
    """x [M, K] . W[:, cols]  for a Linear weight W [K, in] (``cols`` = (c0, c1) or None): the data gradient dz . W of
    the fp32 training backward as ONE split-bf16 GEMM (hgnn_linear_f32_split3), or None when the split-bf16 mode is
    off / the shape has no instantiation (the caller then uses the library's fp32 GEMM)"""
    K = int(x.shape[1])
    N = int(weight.shape[1]) if cols is None else cols[1] - cols[0]
    if not _split3(net, train=True) or x.dtype != torch.float32 or not x.is_cuda or K % 128 or N not in (256, 512) \
            or int(x.shape[0]) == 0:
        return None
    # the kernel wants the weight of the Linear that maps K -> N, i.e. W[:, cols]^T  [N, K]
    Wv = _split3_weight(weight, None if cols is None else (tuple(cols),), False, transpose=True)
    xc = x if x.is_contiguous() else x.contiguous()
    out = torch.empty((int(x.shape[0]), N), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().hgnn_linear_f32_split3(_lib.ptr(xc), int(x.shape[0]), K, _lib.ptr(Wv), N, None,
                                                      _lib.ptr(out), _lib.current_stream(x.device)),
                   "hgnn_linear_f32_split3")
    stats["split3_linear_calls"] = stats.get("split3_linear_calls", 0) + 1
    return out


def _split3_project(table: torch.Tensor, weight, cols_list):
    """[table [R, w] . W[:, cols]^T -> [R, H] for cols in cols_list] (one or two column blocks of the first Linear over
    the SAME table): the pre-projections of the gathered segments (``_projected_segments``) in the split-bf16 arithmetic
    of the kernel that consumes them (three products), ONE launch (hgnn_project_f32_split3); None when the shape has no
    instantiation"""
    R, K = int(table.shape[0]), int(table.shape[1])
    N = int(weight.shape[0])
    if R == 0 or K % 128 or N not in (256, 512) or table.dtype != torch.float32 or not table.is_cuda \
            or not 1 <= len(cols_list) <= 2:
        return None
    # the kernel wants the weight of the Linear that maps K -> N: W[:, cols]  [N, K]
    Wv = [_split3_weight(weight, (tuple(c),), False) for c in cols_list]
    tc = table if table.is_contiguous() else table.contiguous()
    outs = [torch.empty((R, N), dtype=torch.float32, device=table.device) for _ in cols_list]
    with torch.cuda.device(table.device):
        _lib.check(_lib.load().hgnn_project_f32_split3(
            _lib.ptr(tc), R, K, _lib.ptr(Wv[0]), _lib.ptr(Wv[1]) if len(Wv) > 1 else None, N, _lib.ptr(outs[0]),
            _lib.ptr(outs[1]) if len(outs) > 1 else None, _lib.current_stream(table.device)), "hgnn_project_f32_split3")
    stats["split3_project_calls"] = stats.get("split3_project_calls", 0) + 1
    return outs


def _exact_project(table: torch.Tensor, weight, cols_list, width: int):
    """``_split3_project``'s job in EXACT fp32 (ops.project_f32 / hgnn_project_f32): [table . W[:, cols]^T for cols in
    cols_list] from one launch, the column blocks of ``weight`` read in place, zero padded to ``width`` columns; None
    when the entry does not take the shape (K a multiple of 16 up to 512, N a multiple of 16 up to 1024)"""
    K, N = int(table.shape[1]), int(weight.shape[0])
    if table.dtype != torch.float32 or weight.dtype != torch.float32 or not table.is_cuda or not weight.is_cuda \
            or K % 16 or not 16 <= K <= 512 or N % 16 or not 16 <= N <= 1024 or not 1 <= len(cols_list) <= 2:
        return None
    from .ops import project_f32
    Wd = weight.detach()
    res = project_f32(table, *[Wd[:, c0:c1] for c0, c1 in cols_list], width=width if width and N < width else None)
    stats["project_f32_calls"] = stats.get("project_f32_calls", 0) + 1
    return list(res)


_bf16_split = True


def set_bf16_split(flag: bool) -> None:
    """use the feature-split bf16 kernel for the wide layers (L >= 128) when it supports the shape"""
    global _bf16_split
    _bf16_split = bool(flag)


def _wants_split(net, segments, layers=None) -> bool:
    """the bf16 feature-split kernel's shapes (switch ``bf16_split``); ``layers``: ``_parse(net)`` when the caller has
    it"""
    layers = _parse(net) if layers is None else layers
    if not _opt("bf16_split") or layers is None or len(layers) not in (1, 2, 3):
        return False
    if any(int(t.shape[1]) % 128 for t, _ in segments):
        return False
    o = layers[-1][0].out_features
    if len(layers) == 1:
        return layers[0][1] is not None and o in (256, 512, 1024)        # single layers (chains)
    return o in (128, 256, 512) and all(lin.out_features == 2 * o for lin, _, _ in layers[:-1])


def _is_bf16(segments) -> bool:
    return all(t.dtype == torch.bfloat16 for t, _ in segments)


def _narrow_encoder(layers) -> bool:
    """the supernode encoder's shape (``_layout_f32``'s rule): three layers whose last is up to 15 features narrower than
    half the hidden width.  It stays on the exact kernels when ``split3_padded`` is on"""
    h, o = layers[0][0].out_features, layers[-1][0].out_features
    return len(layers) == 3 and h // 2 - 16 < o < h // 2


class _Route(NamedTuple):
    """what ``_run`` launches for one call (``_route``)"""
    net: nn.Module
    layers: list               # _parse(net)
    entry: str                 # each launch calls hgnn_mlp_forward_<entry>: f32, f32_split3, bf16, bf16_split, f32_padded,
                               # f32_split3_padded, f32_plain or f32_square (with ``groups``: each group's own entry)
    split_proj: bool = False   # f32_split3: pre-projections in the kernel's arithmetic (``_descriptor``)
    chain: bool = False        # one launch per LayerNorm'ed layer (+ a trailing plain Linear)
    head: bool = False         # score head: the plain last Linear runs outside the kernel, on the hidden rows
    train: bool = False        # the differentiable variants (``_FusedMLPTrain``, ``_FusedMLPTrainBf16``)
    groups: tuple = ()         # 4 to 8 layers: the routes of consecutive launches of at most three layers (``_group_route``)


_square = os.environ.get("HGNN_MLP_SQUARE", "1") != "0"


def set_square(flag: bool) -> None:
    """Process default of the ``square`` option (HGNN_MLP_SQUARE=0 switches it off): fp32 networks whose output is as
    wide as their hidden layers (``hidden_ratio: 1``, ``hidden == latent``; widths: multiples of 16 in [32, 256]), single
    Linear -> LayerNorm -> act layers of those widths and networks of 4 to 8 layers run on the exact fp32 kernel's square
    instantiations (hgnn_mlp_forward_f32_square), no-grad and under autograd.  Asked only after every other fp32 route
    has declined, so no call that had a kernel before changes.  Off: these shapes take the library path (counted in
    ``stats["library_calls"]``).  A backward and the recompute of a reentrant checkpoint run on autograd's own thread,
    which only the process default set here reaches.  Default on."""
    global _square
    _square = bool(flag)


_GROUP_NETS = weakref.WeakKeyDictionary()   # net -> the Sequentials of its groups (sharing its modules)


def _group_nets(net, sizes):
    """``net``'s modules as consecutive Sequentials of ``sizes`` modules, built once per network (again when one of its
    modules has been replaced)"""
    mods = list(net)
    hit = _GROUP_NETS.get(net)
    if hit is None or hit[0] != sizes or len(hit[2]) != len(mods) or any(a is not b for a, b in zip(hit[2], mods)):
        subs, i = [], 0
        for k in sizes:
            subs.append(nn.Sequential(*mods[i:i + k]))
            i += k
        hit = (sizes, subs, mods)
        _GROUP_NETS[net] = hit
    for sub in hit[1]:
        sub._hgnn_split3 = getattr(net, "_hgnn_split3", None)   # models._mark_split3 may run after the first call
    return hit[1]


def _group_route(net, layers, segments, skip, train: bool) -> Optional[_Route]:
    """Networks of 4 to 8 layers with one hidden width, LayerNorm on every layer, optionally ending in a plain head
    Linear at most 32 wide: consecutive launches of at most three layers each, the hidden rows between two groups making
    one trip through HBM.  The first group K -> h -> h -> h carries the segments (square entry), middle groups are
    square on one direct segment, the last group takes whatever entry accepts its shape and carries ``skip``; a head's
    plain Linear is a product over the last hidden rows (as for the chains).  Under autograd each group is its own
    differentiable call.  None: the library path."""
    plain_last = layers[-1][1] is None
    body = layers[:-1] if plain_last else layers
    h = int(layers[0][0].out_features)
    if not 4 <= len(layers) <= 8 or len(body) < 4 or any(ln is None for _, ln, _ in body) \
            or any(int(lin.out_features) != h for lin, _, _ in body[:-1]) or not _square_grid(h) \
            or not isinstance(net, nn.Sequential) or _is_bf16(segments) or not all(t.is_cuda for t, _ in segments):
        return None
    if plain_last and (skip is not None or layers[-1][0].out_features > 32 or int(body[-1][0].out_features) != h):
        return None
    counts = [3] * ((len(body) - 1) // 3) + [len(body) - 3 * ((len(body) - 1) // 3)]
    subs = _group_nets(net, tuple(3 * c for c in counts))
    dev = segments[0][0].device
    probe = [(torch.empty((0, h), dtype=torch.float32, device=dev), None)]
    routes = []
    for i, sub in enumerate(subs):
        last = i == len(subs) - 1
        sk = None
        if last and skip is not None:
            M = {int(x.numel()) if x is not None else int(t.shape[0]) for t, x in segments}
            if len(M) != 1 or tuple(skip.shape) != (M.pop(), int(body[-1][0].out_features)) or not skip.is_cuda \
                    or skip.dtype != torch.float32:
                return None
            sk = torch.empty((0, int(skip.shape[1])), dtype=torch.float32, device=dev)
        r = _route(sub, segments if i == 0 else probe, sk, train=train, allow_groups=False)
        if r is None or r.chain or (not last and r.entry != "f32_square"):
            return None
        routes.append(r)
    return _Route(net, layers, "f32_square", head=plain_last, train=train, groups=tuple(routes))


def _route(net, segments, skip, *, train: bool, allow_chain: bool = True, allow_square: bool = True,  # noqa: C901
           allow_groups: bool = True) -> Optional[_Route]:
    """The one dispatch decision: which fused kernel evaluates ``net`` on these arguments, or None (library path).
    Parses ``net`` once and asks each kernel's own ``hgnn_mlp_supported*`` check at most once, on a dry descriptor.

    ``train=False``: a forward autograd does not record (no grad mode, or nothing requires grad).  fp32 rows: the whole
    network in one launch (hgnn_mlp_forward_f32), else -- ``allow_chain`` -- one launch per layer (latent 512; a caller
    with a cheaper alternative, the bf16 tail of the encoders, passes False), else -- widths between the kernel's
    template grid -- one launch on zero-padded parameters (hgnn_mlp_forward_f32_padded, exact fp32 only), else --
    ``allow_square``, option ``square`` -- hidden = output, single layers and (``allow_groups``) 4 to 8 layers on
    hgnn_mlp_forward_f32_square (``square_route``; under autograd too, after f32 and f32_padded).  Among these, with the split-bf16
    arithmetic on (``_split3``): score heads K -> H -> H -> w (H in 256, 512) run their hidden layers on
    hgnn_mlp_forward_f32_split3 and the last Linear as a product over the hidden rows; networks of its shapes run whole
    on it.  bf16 rows: the feature-split kernel where it wants the shape (``bf16_split``) else the plain bf16 kernel,
    else the single-layer chain on the split kernel.
    ``train=True``: autograd records.  fp32: the kernel's shapes with LayerNorm on every layer (f32_split3 when
    ``_split3(net, train=True)``), and score heads (dumps of their hidden layers); the padded widths with LayerNorm on
    every layer (their heads train on the library path); bf16: the feature-split kernel."""
    if train:
        if not _opt("train_enabled") or not torch.is_grad_enabled():
            return None
    else:
        if not _opt("enabled"):
            return None
        if torch.is_grad_enabled():
            tensors = [t for t, _ in segments] + ([skip] if skip is not None else []) + list(net.parameters())
            if any(t.requires_grad for t in tensors):
                return None
    layers = _parse(net)
    if layers is None:
        return None
    lib = _lib.load()
    bf16 = _is_bf16(segments)
    if _is_plain(layers):
        # no LayerNorm anywhere (layernorm: False): opt-in, fp32 rows, the exact kernel's plain form -- inference and
        # training alike; everything else (bf16 rows, shapes off its grid) is the library path's
        if not _plain_layers_on() or bf16 or len(layers) < 2:
            return None
        try:
            desc = _descriptor(net, segments, skip, "f32_plain", dry=True, layers=layers)
        except RuntimeError:
            return None
        if desc is None or not lib.hgnn_mlp_supported_f32_plain(ctypes.byref(desc[0])):
            return None
        if train and int(desc[0].w_last_rows) != 0 and not (layers[-1][2] == 0 and layers[-1][0].out_features <= 32):
            # a last layer narrower than its storage that is no head (the supernode encoder): its dumps are refused by
            # the entry, so it trains on the library path (counted in library_calls)
            return None
        return _Route(net, layers, "f32_plain", train=train)

    def dry(entry, lays=layers, sk=skip):
        """(dry descriptor or None, whether the kernel's own check accepts it)"""
        try:
            desc = _descriptor(net, segments, sk, entry, dry=True, layers=lays)
        except RuntimeError:
            return None, False
        check = getattr(lib, "hgnn_mlp_supported" + ("" if entry == "f32" else "_" + entry))
        return desc, desc is not None and bool(check(ctypes.byref(desc[0])))

    def chain_ok():
        """fp32 MLPs too wide for one launch (latent 512: a 1024-wide hidden layer is 256 accumulators per lane) and the
        bf16 heads: the LayerNorm'ed layers one launch each, the rows of a plain last Linear (the width-1 heads) an
        M x 1024 x w product"""
        if len(layers) < 2 or any(ln is None for _, ln, _ in layers[:-1]):
            return False
        fused_layers = layers if layers[-1][1] is not None else layers[:-1]
        # fp32: the chain may END in a LayerNorm'ed layer narrower than its 512-row storage (504: supernode encoder)
        o_last = layers[-1][0].out_features
        narrow = not bf16 and layers[-1][1] is not None and skip is None and 496 < o_last < 512 and o_last % 4 == 0
        wide = fused_layers[1:-1] if narrow else fused_layers[1:]
        if any(lin.out_features not in (512, 1024) or lin.in_features % 16 for lin, _, _ in wide) \
                or (narrow and fused_layers[-1][0].in_features % 16) \
                or fused_layers[0][0].out_features not in (512, 1024):
            return False
        if bf16 and not _wants_split(None, segments, fused_layers[:1]):
            return False
        first, ok = dry("bf16_split" if bf16 else "f32", fused_layers[:1], None)
        if not ok or (len(fused_layers) < len(layers) and skip is not None):
            return False                                      # heads have no skip connection
        dt = torch.bfloat16 if bf16 else torch.float32
        return skip is None or (skip.is_cuda and skip.dtype == dt
                                and tuple(skip.shape) == (first[2], layers[-1][0].out_features))

    plain_last = layers[-1][1] is None

    def square_route():
        """asked last, after f32, the chain and f32_padded have declined: hidden = output and single layers on
        hgnn_mlp_forward_f32_square (the exact kernel also for a module marked for split-bf16), 4 to 8 layers as groups
        (``_group_route``).  The narrow square encoder has no dumps: it trains on the library path"""
        if not allow_square or not _opt("square"):
            return None
        if len(layers) > 3:
            return _group_route(net, layers, segments, skip, train) if allow_groups else None
        if plain_last or not dry("f32_square")[1]:
            return None
        if train and layers[-1][0].out_features != layers[0][0].out_features:
            return None
        return _Route(net, layers, "f32_square", train=train)

    split3_shape = len(layers) in (2, 3) and all(ln is not None for _, ln, _ in layers) and \
        all(t.dtype == torch.float32 and int(t.shape[1]) % 128 == 0 for t, _ in segments)
    if split3_shape:
        o = layers[-1][0].out_features
        split3_shape = (len(layers) == 2 and layers[0][0].out_features == o and o in (256, 512)) or \
            (o in (128, 256) and all(lin.out_features == 2 * o for lin, _, _ in layers[:-1]))     # head body or cell
    if train:
        if bf16:
            if not _opt("train_bf16_enabled") or not _wants_split(net, segments, layers) \
                    or any(lin.out_features not in (64, 128, 256, 512, 1024) for lin, _, _ in layers):
                return None                               # widths of the bf16 LayerNorm / activation row kernels
            return _Route(net, layers, "bf16_split", train=True) if dry("bf16_split")[1] else None
        desc, ok = dry("f32")
        # narrow encoders (zero-padded LayerNorm'ed last layer) have no dumps; the small-K encoders (w0_cols = 16: the
        # kernel-side zero padding of W[0]) do -- their backward uses the unpadded parameters; score heads (plain last
        # layer stored as 32 rows) dump their two hidden layers
        head = len(layers) == 3 and plain_last
        if not ok and not plain_last and dry("f32_padded")[1]:
            # widths between the grid's: the same kernel on zero-padded parameters, dumps at the real widths; the
            # backward takes any width (ATen rows where the HIP row kernels have no instantiation)
            return _Route(net, layers, "f32_padded", train=True)
        if not ok:
            return square_route()
        if int(desc[0].w_last_rows) != 0 and not head:
            return None
        if head and (skip is not None or any(lin.out_features not in (64, 128, 256, 512) for lin, _, _ in layers[:2])):
            return None                                   # widths of the LayerNorm / activation row kernels
        split3 = not head and split3_shape and _split3(net, train=True)
        return _Route(net, layers, "f32_split3" if split3 else "f32", head=head, train=True)
    if bf16:
        entry = "bf16_split" if _wants_split(net, segments, layers) else "bf16"
        if dry(entry)[1]:
            return _Route(net, layers, entry)
        return _Route(net, layers, "bf16_split", chain=True) if allow_chain and chain_ok() else None
    desc, ok = dry("f32")
    chain = not ok and allow_chain and chain_ok()
    if not ok and not chain:
        # widths between the grid's (latent 48, 96, 160, 192, hidden_ratio 3, ...): zero-padded parameters on the next
        # grid instantiation of the exact fp32 kernel
        if not dry("f32_padded")[1]:
            return square_route()
        if _opt("split3_padded") and _split3(net) and not _narrow_encoder(layers) and dry("f32_split3_padded")[1]:
            # opt-in: the split-bf16 arithmetic on the same zero padding (cell networks with a hidden width above 128)
            return _Route(net, layers, "f32_split3_padded")
        return _Route(net, layers, "f32_padded")
    if _split3(net) and skip is None and len(layers) == 3 and plain_last \
            and layers[0][0].out_features in (256, 512) and layers[1][0].out_features == layers[0][0].out_features \
            and all(t.dtype == torch.float32 and int(t.shape[1]) % 128 == 0 for t, _ in segments):
        # score heads (K -> H -> H -> w, IN.py:107-115, HGNN_GMM.py:313-321): the two LayerNorm'ed hidden layers on
        # hgnn_mlp_forward_f32_split3, the plain last Linear a trailing matrix-vector product over the hidden rows
        return _Route(net, layers, "f32_split3", split_proj=True, head=True)
    if desc is not None and split3_shape and _split3(net):
        return _Route(net, layers, "f32_split3", split_proj=True)
    return _Route(net, layers, "f32", chain=chain)


def supported(net, segments, skip, allow_chain: bool = True) -> bool:
    """a fused kernel evaluates this no-grad call (``_route``).  ``allow_chain``: accept fp32 MLPs that run as one launch
    per layer (latent 512); a caller that has a cheaper alternative for them (bf16 tail of the encoders in bf16 mode)
    passes False"""
    return _route(net, segments, skip, train=False, allow_chain=allow_chain) is not None


def supported_train(net, segments, skip) -> bool:
    """differentiable fused path (``_route``): cell networks (LayerNorm on every layer, 16-aligned segments) and score
    heads; bf16 rows: the feature-split kernel's shapes at latent 128 / 256 (``_FusedMLPTrainBf16``)"""
    return _route(net, segments, skip, train=True) is not None


def _out_buffer(out, M, n_out, dtype, dev):
    """caller-supplied output rows (a contiguous [M, n_out] row block, e.g. a slice of a larger edge table) or a
    fresh tensor"""
    if out is None:
        return torch.empty((M, n_out), dtype=dtype, device=dev)
    if tuple(out.shape) != (M, n_out) or out.dtype != dtype or out.device != dev or not out.is_contiguous():
        raise RuntimeError(f"fused_concat_mlp: out must be a contiguous {dtype} [{M}, {n_out}] tensor on {dev}")
    return out


def _forward(entry, d, out, dev):
    """launch hgnn_mlp_forward_<entry> on a ready descriptor"""
    name = "hgnn_mlp_forward_" + entry
    _lib.check(getattr(_lib.load(), name)(ctypes.byref(d), _lib.ptr(out), _lib.current_stream(dev)), name)
    if entry == "f32_split3":
        stats["split3_calls"] = stats.get("split3_calls", 0) + 1
    elif entry == "f32_padded":
        stats["padded_calls"] += 1
    elif entry == "f32_split3_padded":
        stats["split3_padded_calls"] = stats.get("split3_padded_calls", 0) + 1
    elif entry == "f32_plain":
        stats["plain_calls"] += 1
    elif entry == "f32_square":
        stats["square_calls"] += 1


def _launch(layers, segments, skip, entry, split_proj=False, out=None):
    """one no-grad launch of hgnn_mlp_forward_<entry>"""
    desc = _descriptor(None, segments, skip, entry, split_proj, layers=layers)
    if desc is None:
        raise RuntimeError("fused_concat_mlp: unsupported arguments (call supported() first)")
    d, keep, M, n_out = desc
    dev = segments[0][0].device
    out = _out_buffer(out, M, n_out, torch.bfloat16 if entry.startswith("bf16") else torch.float32, dev)
    if M == 0:
        return out
    with torch.cuda.device(dev):
        _forward(entry, d, out, dev)
    del keep
    stats["fused_calls"] += 1
    return out


def _run(r: _Route, segments, skip, out=None):
    """evaluate ``net`` (+ ``skip``) on ``segments`` the way route ``r`` says.  ``out``: write the result rows into this
    tensor (no-grad callers that assemble one edge table from several calls -- the interior / boundary split of a sharded
    edge update -- avoid a 2 GB concatenation); only the single-launch paths write into it directly"""
    layers = r.layers
    if r.groups:
        # 4 to 8 layers: one launch (under autograd: one differentiable call) per group, the hidden rows between two
        # groups make one trip through HBM; the last group carries the skip rows
        y = None
        for i, g in enumerate(r.groups):
            y = _run(g, segments if i == 0 else [(y, None)], skip if i == len(r.groups) - 1 else None)
        if r.head:
            hidden, lin = y, layers[-1][0]
            y = _head_linear(hidden, lin, r.train)
            if y is None:
                y = torch.nn.functional.linear(hidden, lin.weight, lin.bias)
        return y if out is None else out.copy_(y)
    if r.train and r.entry == "f32_plain":
        tables, indices = [t for t, _ in segments], tuple(i for _, i in segments)
        params = [p for lin, _, _ in layers for p in (lin.weight, lin.bias)]
        return _PlainMLPTrain.apply(r, indices, skip is not None, *tables, *([skip] if skip is not None else []), *params)
    if r.train:
        tables, indices = [t for t, _ in segments], tuple(i for _, i in segments)
        params = []
        for lin, ln, _ in layers[:2] if r.head else layers:
            params += [lin.weight, lin.bias, ln.weight, ln.bias]
        if r.head:
            # score heads (IN.py:107-115,126-127; HGNN_GMM.py:313-321,342-344) under autograd: the two LayerNorm'ed
            # hidden layers on the differentiable fused kernel (dumps + hand-written backward), the plain last Linear --
            # an [M, H] x [H, w<=32] product -- applied to the returned hidden rows
            hidden = _FusedMLPTrain.apply(r, indices, False, *tables, *params)
            stats["fused_head_train_calls"] = stats.get("fused_head_train_calls", 0) + 1
            y = _head_linear(hidden, layers[2][0], True)
            if y is not None:
                return y
            return torch.nn.functional.linear(hidden, layers[2][0].weight, layers[2][0].bias)
        fn = _FusedMLPTrainBf16 if r.entry == "bf16_split" else _FusedMLPTrain
        return fn.apply(r, indices, skip is not None, *tables, *([skip] if skip is not None else []), *params)
    if r.head:
        hidden = _launch(layers[:2], segments, None, r.entry, r.split_proj)
        y = _head_linear(hidden, layers[2][0], False)
        if y is None:
            y = torch.nn.functional.linear(hidden, layers[2][0].weight, layers[2][0].bias)
    elif r.chain:
        # one launch per layer; the hidden rows make one trip through HBM (fp32 at latent 512)
        y = None
        for i, layer in enumerate(layers):
            if layer[1] is None:                          # the plain last Linear of a head
                hidden, y = y, _head_linear(y, layer[0], False)
                if y is None:
                    y = torch.nn.functional.linear(hidden, layer[0].weight.to(hidden.dtype),
                                                   layer[0].bias.to(hidden.dtype))
            else:
                y = _launch([layer], segments, skip if i == len(layers) - 1 else None, r.entry)
                segments = [(y, None)]
    else:
        return _launch(layers, segments, skip, r.entry, r.split_proj, out)
    return y if out is None else out.copy_(y)


def fused_concat_mlp(net, segments, skip: Optional[torch.Tensor], out: Optional[torch.Tensor] = None):
    """no-grad evaluation on the kernel ``_route`` picks.  ``out``: see ``_run``"""
    r = _route(net, segments, skip, train=False)
    if r is None:
        raise RuntimeError("fused_concat_mlp: unsupported arguments (call supported() first)")
    return _run(r, segments, skip, out)


# --------------------------------------------------------------------------- training variant
def _ln_act_forward(z, gamma, beta, act, eps):
    """act(LayerNorm(z)) in one HIP pass (csrc/ln_act.hip)"""
    out = torch.empty_like(z)
    M, W = int(z.shape[0]), int(z.shape[1])
    if M:
        lib = _lib.load()
        fn = lib.hgnn_ln_act_forward_bf16 if z.dtype == torch.bfloat16 else lib.hgnn_ln_act_forward_f32
        with torch.cuda.device(z.device):
            _lib.check(fn(
                _lib.ptr(z), M, W, _lib.ptr(gamma.detach().float().contiguous()),
                _lib.ptr(beta.detach().float().contiguous()),
                int(act), float(eps), _lib.ptr(out), _lib.current_stream(z.device)), "hgnn_ln_act_forward")
    return out


def _ln_act_backward(z, grad_out, gamma, beta, act, eps):
    """(grad_z, grad_gamma, grad_beta, grad_bias) of a = act(LayerNorm(z)), z = x W^T + bias, in one HIP pass"""
    M, W = int(z.shape[0]), int(z.shape[1])
    dz = torch.empty_like(z)
    partials = torch.empty((_lib.LN_ACT_BLOCKS, 3, W), dtype=torch.float32, device=z.device)
    go = grad_out.contiguous().to(z.dtype)
    lib = _lib.load()
    fn = lib.hgnn_ln_act_backward_bf16 if z.dtype == torch.bfloat16 else lib.hgnn_ln_act_backward_f32
    with torch.cuda.device(z.device):
        _lib.check(fn(
            _lib.ptr(z), _lib.ptr(go), M, W, _lib.ptr(gamma.detach().float().contiguous()),
            _lib.ptr(beta.detach().float().contiguous()), int(act), float(eps), _lib.ptr(dz), _lib.ptr(partials),
            _lib.current_stream(z.device)), "hgnn_ln_act_backward")
    sums = partials.sum(dim=0)
    return dz, sums[0], sums[1], sums[2]


def _atb(A: torch.Tensor, B: torch.Tensor, net=None) -> torch.Tensor:
    """A^T B for tall A [n, p], B [n, q] with a small [p, q] result: a weight gradient.  With the split-bf16 mode on
    (``net`` given) and fp32 operands of at least 4096 rows: the hand-written split-K kernel on the bf16 matrix pipe
    (ops.wgrad_f32_split3: ~1.7 ms where the library paths below need 3.6-4 ms at n = 2M).  With ``set_wgrad_f32`` and
    fp32 device operands whose widths are multiples of 8 up to 1024: the exact fp32-MFMA split-K kernel (ops.wgrad_f32:
    fixed order, the same bits on every device; 4.05 against 3.59 ms at n = 2M, profiles/wgrad_f32.json).  With
    ``set_narrow_f32`` and one width <= 32 (the other a multiple of 4 up to 1024) that the kernel above does not take:
    ops.wgrad_narrow_f32 (profiles/exact_tail.json).  Otherwise
    (``stats["library_wgrad_calls"]``): the library picks
    a small output tile without split-K for these (p*q/1024 workgroups walking all n rows: 1.2 ms for the
    8 GFLOP of n = 120k, ~110 TFLOP/s at n = 2M); a batched product over row blocks plus one sum fills the
    chip (fixed summation order: deterministic).  EC-IN training step 368 -> 306 ms."""
    n = int(A.shape[0])
    if net is not None and _split3(net, train=True) and n >= 4096 and A.dtype == torch.float32 and B.dtype == torch.float32 \
            and A.is_cuda and int(A.shape[1]) % 8 == 0 and int(B.shape[1]) % 8 == 0:
        from .ops import wgrad_f32_split3
        stats["split3_wgrad_calls"] = stats.get("split3_wgrad_calls", 0) + 1
        return wgrad_f32_split3(A, B)
    # set_wgrad_f32: the exact route's weight gradients on hgnn_wgrad_f32 (fp32 MFMA, fixed order) instead of the library
    if _wgrad_f32_on and n >= 1 and A.dtype == torch.float32 and B.dtype == torch.float32 and A.is_cuda and B.is_cuda \
            and int(A.shape[1]) % 8 == 0 and int(B.shape[1]) % 8 == 0 \
            and 0 < int(A.shape[1]) <= 1024 and 0 < int(B.shape[1]) <= 1024:
        from .ops import wgrad_f32
        stats["wgrad_f32_calls"] = stats.get("wgrad_f32_calls", 0) + 1
        return wgrad_f32(A, B)
    # set_narrow_f32: one width <= 32 (the encoders' 3- and 6-wide tables) on hgnn_wgrad_narrow_f32, the other a multiple
    # of 4 up to 1024; the narrow side goes first, so a [q <= 32] B gives the transposed result
    if _narrow_f32_on and A.dtype == torch.float32 and B.dtype == torch.float32 and A.is_cuda and B.is_cuda \
            and not (net is not None and _split3(net, train=True)):
        p, q = int(A.shape[1]), int(B.shape[1])
        if _narrow_widths(p, q) or _narrow_widths(q, p):
            from .ops import wgrad_narrow_f32
            stats["narrow_wgrad_calls"] = stats.get("narrow_wgrad_calls", 0) + 1
            return wgrad_narrow_f32(A, B) if _narrow_widths(p, q) else wgrad_narrow_f32(B, A).t().contiguous()
    stats["library_wgrad_calls"] = stats.get("library_wgrad_calls", 0) + 1
    chunks = max(16, min(256, n // 8192))   # 4096 / 8192 rows per block measured equal, 32768 6 % slower
    c = n // chunks
    if c < 256:
        return A.t() @ B
    main = c * chunks
    out = torch.bmm(A[:main].reshape(chunks, c, A.shape[1]).transpose(1, 2),
                    B[:main].reshape(chunks, c, B.shape[1])).sum(dim=0)
    if main < n:
        out += A[main:].t() @ B[main:]
    return out


_ATEN_ACT = {1: torch.nn.functional.gelu, 2: torch.tanh, 3: torch.relu, 4: torch.nn.functional.silu,
             5: torch.nn.functional.leaky_relu, 6: torch.nn.functional.elu, 7: torch.sigmoid}


def _aten_act(y, code: int):
    """act(y) with ATen kernels: rows of a width the HIP row kernels have no instantiation for"""
    return _ATEN_ACT[code](y) if code else y


def _aten_act_backward(da, y, code: int):
    """da * act'(y) through ATen's own derivative of the activation (same widths as ``_aten_act``)"""
    if not code:
        return da
    with torch.enable_grad():
        yy = y.detach().requires_grad_(True)
        return torch.autograd.grad(_ATEN_ACT[code](yy), yy, da)[0]


def _zero_grads(ctx, tables, params, grad_out, n_seg):
    """backward of an MLP that was called on M == 0 rows (a shard without edges, an empty super graph): every
    parameter and table gradient is zero; no kernel is launched"""
    gt = [torch.zeros_like(t) if ctx.needs_input_grad[3 + i] else None for i, t in enumerate(tables)]
    gs = [grad_out] if ctx.has_skip else []
    return (None, None, None, *gt, *gs, *[torch.zeros_like(p) for p in params])


def _train_forward(ctx, route, indices, has_skip, tensors):
    """the forward of both differentiable variants (``tensors`` = tables, the skip rows if any, then W, b, ln_w, ln_b
    of every layer): the kernel of ``route.entry`` dumping each layer's pre-LayerNorm rows z_l (``save_pre``) in the
    row dtype; fills ``ctx`` for the backward.  Returns (out, tables, skip, [z_l])"""
    n_seg = len(indices)
    tables = list(tensors[:n_seg])
    skip = tensors[n_seg] if has_skip else None
    params = tensors[n_seg + (1 if has_skip else 0):]
    bf16 = route.entry.startswith("bf16")
    desc = _descriptor(route.net, list(zip(tables, indices)), skip, route.entry, layers=route.layers)
    if desc is None:
        raise RuntimeError(f"fused_concat_mlp_train{' (bf16)' if bf16 else ''}: unsupported arguments "
                           "(call supported_train() first)")
    d, keep, M, n_out = desc
    # a score head: the LayerNorm'ed hidden layers are differentiated here, the plain last Linear is applied by the
    # caller on the returned hidden rows (``_run``)
    n = int(d.n_layers) - (1 if route.head else 0)
    dt, dev = torch.bfloat16 if bf16 else torch.float32, tables[0].device
    zs = [torch.empty((M, int(d.width[l + 1])), dtype=dt, device=dev) for l in range(n)]
    for l in range(n):
        d.save_pre[l] = zs[l].data_ptr() if M else None
    out = torch.empty((M, n_out), dtype=dt, device=dev)
    if M:
        with torch.cuda.device(dev):
            # f32_split3 (opt-in): the forward and its dumps on the split-bf16 kernel; the backward is unchanged
            _forward(route.entry, d, out, dev)
    del keep
    stats["fused_train_calls"] += 1
    ctx.indices, ctx.has_skip, ctx.n, ctx.net, ctx.layers = indices, has_skip, n, route.net, route.layers
    ctx.acts, ctx.eps = [int(d.act[l]) for l in range(n)], float(d.ln_eps)
    ctx.save_for_backward(*tables, *params, *zs)
    return out, tables, skip, zs


def _skip_segment(ctx, indices, tables, skip) -> int:
    """the direct (un-gathered) segment that is the same tensor as the skip rows (``edges + MLP(..., edges)``) when both
    need a gradient, or -1: the backward can then return the two gradients as one, added in a kernel's epilogue"""
    n_seg = len(indices)
    for s_i in range(n_seg):
        t = tables[s_i]
        if indices[s_i] is None and ctx.needs_input_grad[3 + s_i] and ctx.needs_input_grad[3 + n_seg] \
                and t.data_ptr() == skip.data_ptr() and t.shape == skip.shape and t.stride() == skip.stride():
            return s_i
    return -1


class _FusedMLPTrain(torch.autograd.Function):
    """Differentiable fused MLP.  Forward = the same MFMA kernel, additionally dumping each layer's
    pre-LayerNorm output z_l (``save_pre``).  Backward is written out by hand: LayerNorm / activation
    are re-derived from z_l with elementwise ATen kernels, data and weight gradients are library
    GEMMs (data gradients: the fused fp32 backward layer with ``set_bwd_layer_f32``), and the gradients of
    gathered segments go back through the atomics-free segmented reduce.
    Compared with autograd through the unfused path this skips the second forward's GEMMs,
    the [M,3L] concat and the gathered copies; with 288 GB of HBM the reference's checkpointing can
    also be switched off (hparams["checkpointing"]=False) and the dumps kept instead."""

    @staticmethod
    def forward(ctx, route, indices, has_skip, *tensors):
        out, tables, skip, zs = _train_forward(ctx, route, indices, has_skip, tensors)
        ctx.skip_seg = _skip_segment(ctx, indices, tables, skip) if has_skip else -1
        if route.head:
            # the hidden rows feeding the plain last Linear: one LayerNorm / activation row pass over the last dump
            ln = route.layers[ctx.n - 1][1]
            return _ln_act_forward(zs[-1], ln.weight, ln.bias, ctx.acts[-1], ctx.eps)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        with torch.autocast("cuda", enabled=False):   # fp32 GEMMs whatever the caller's autocast state
            return _FusedMLPTrain._backward(ctx, grad_out.float())

    @staticmethod
    def _backward(ctx, grad_out):
        from .ops import _seg_reduce
        from .plan import get_plan
        n, indices = ctx.n, ctx.indices
        n_seg = len(indices)
        saved = ctx.saved_tensors
        tables = saved[:n_seg]
        params = saved[n_seg:n_seg + 4 * n]
        zs = saved[n_seg + 4 * n:]
        if int(grad_out.shape[0]) == 0:
            return _zero_grads(ctx, tables, params, grad_out, n_seg)
        W = [params[4 * l] for l in range(n)]
        lw = [lin.weight for lin, _, _ in ctx.layers[:n]]   # the Parameter objects themselves (weight-prep cache keys)
        lnw = [params[4 * l + 2] for l in range(n)]
        lnb = [params[4 * l + 3] for l in range(n)]
        aten = torch.ops.aten
        g = grad_out.contiguous()
        hip_rows = all(int(z.shape[1]) in (64, 128, 256, 512, 1024) for z in zs)
        # set_bwd_layer_f32: the exact route's data gradients on hgnn_mlp_backward_layer_f32 (the opt-in split-bf16
        # training route keeps precedence).  fuse[l]: dz_l . W_l, the LayerNorm / activation backward of layer l - 1 and
        # its recomputed activations are ONE launch
        f32_layer = hip_rows and _bwd_layer_f32_on and not _split3(ctx.net, train=True) and g.dtype == torch.float32
        fuse = [bool(f32_layer and l > 0 and _bwd_layer_f32_supported(int(W[l].shape[0]), int(W[l].shape[1])))
                for l in range(n)]
        ys, means, rstds, outs = [], [], [], []
        if hip_rows:
            # hidden activations a_l = act(LN(z_l)) for the weight gradients: one HIP pass per layer
            outs = [_ln_act_forward(zs[l], lnw[l], lnb[l], ctx.acts[l], ctx.eps) if l < n - 1 and not fuse[l + 1]
                    else None for l in range(n)]
        else:
            # re-derive y_l = LN(z_l) (+ statistics) and a_l = act(y_l) with ATen elementwise kernels
            for l in range(n):
                y, mean, rstd = torch.native_layer_norm(zs[l], [zs[l].shape[1]], lnw[l], lnb[l], ctx.eps)
                ys.append(y)
                means.append(mean)
                rstds.append(rstd)
                code = ctx.acts[l]
                if l < n - 1 or code == 2:
                    outs.append(_aten_act(y, code))
                else:
                    outs.append(None)
        grads_params = [None] * (4 * n)
        grads_tables = [None] * n_seg
        da = g
        below = None          # (dz, dgamma, dbeta, dbias) of layer l, when the fused layer of l + 1 has produced them
        folded_skip = False
        for l in range(n - 1, -1, -1):
            code = ctx.acts[l]
            if below is not None:
                dz, dlw, dlb, dbias = below
                below = None
                grads_params[4 * l + 1] = dbias
            elif hip_rows:
                # act' -> LayerNorm backward -> dgamma / dbeta / dbias in ONE pass over (z_l, da)
                dz, dlw, dlb, dbias = _ln_act_backward(zs[l], da, lnw[l], lnb[l], code, ctx.eps)
                grads_params[4 * l + 1] = dbias
            else:
                if code == 1:
                    dy = aten.gelu_backward(da, ys[l], approximate="none")
                elif code == 2:
                    dy = aten.tanh_backward(da, outs[l])
                elif code == 3:
                    dy = da * (ys[l] > 0)
                elif code >= 4:
                    dy = _aten_act_backward(da, ys[l], code)
                else:
                    dy = da
                dz, dlw, dlb = aten.native_layer_norm_backward(dy, zs[l], [zs[l].shape[1]], means[l], rstds[l],
                                                               lnw[l], lnb[l], [True, True, True])
                ys[l] = None
                grads_params[4 * l + 1] = dz.sum(dim=0)
            grads_params[4 * l + 2] = dlw
            grads_params[4 * l + 3] = dlb
            if l > 0 and fuse[l]:
                dz_prev, a_prev, dlw_p, dlb_p, dbias_p = _bwd_layer_f32(
                    dz, W[l], zs[l - 1], lnw[l - 1], lnb[l - 1], ctx.acts[l - 1], ctx.eps, want_a=True, weight=lw[l])
                grads_params[4 * l] = _atb(dz, a_prev, ctx.net)
                del a_prev
                below = (dz_prev, dlw_p, dlb_p, dbias_p)
            elif l > 0:
                grads_params[4 * l] = _atb(dz, outs[l - 1], ctx.net)
                da = _split3_linear(dz, lw[l], None, ctx.net)
                if da is None:
                    da = dz @ W[l]
                outs[l - 1] = None
            else:
                # First layer.  A gathered segment x_s = table[idx] enters linearly, so both of its
                # gradients factor through S = segment_reduce(dz, idx)  ([table rows, H], one HBM pass):
                #   dW[:, s] = dz^T table[idx] = S^T table        (K = table rows instead of M)
                #   d table  = scatter(dz W_s, idx) = S W_s
                # i.e. for nodes[graph[k]] the two M-row GEMMs (and the gathered copy / the [M,K]
                # concat they would read) become two N-row GEMMs: 16x fewer FLOPs at M/N = 16.7.
                # Only a direct segment (the edge rows themselves) keeps M-row GEMMs.
                dW_cols = []
                col = 0
                split3_train = _split3(ctx.net, train=True)   # keeps precedence over set_narrow_f32
                for s_i in range(n_seg):
                    idx = indices[s_i]
                    tab = tables[s_i].contiguous()
                    w_s = int(tab.shape[1])
                    W_s = W[0][:, col:col + w_s]
                    if idx is not None:
                        S = _seg_reduce(get_plan(idx, int(tab.shape[0])), dz, None, None)
                        dW_cols.append(_atb(S, tab, ctx.net))
                        if ctx.needs_input_grad[3 + s_i]:
                            if f32_layer and int(S.shape[0]) and _bwd_layer_f32_supported(int(W_s.shape[0]), w_s):
                                grads_tables[s_i] = _bwd_layer_f32(S, W_s, None, None, None, 0, ctx.eps, weight=lw[0],
                                                                   cols=(col, col + w_s))[0]
                            else:
                                gt = None if split3_train else _narrow_dgrad(S, W_s, lw[0], (col, col + w_s))
                                grads_tables[s_i] = gt if gt is not None else S @ W_s
                        del S
                    else:
                        dW_cols.append(_atb(dz, tab, ctx.net))
                        if ctx.needs_input_grad[3 + s_i]:
                            if f32_layer and _bwd_layer_f32_supported(int(W_s.shape[0]), w_s):
                                # edges + MLP(..., edges): the skip connection's gradient is added in the epilogue and
                                # returned once, as this segment's (other direct segments leave folded_skip alone)
                                fold = ctx.skip_seg == s_i
                                grads_tables[s_i] = _bwd_layer_f32(dz, W_s, None, None, None, 0, ctx.eps,
                                                                   skip=g if fold else None, weight=lw[0],
                                                                   cols=(col, col + w_s))[0]
                                folded_skip = folded_skip or fold
                            else:
                                gt = _split3_linear(dz, lw[0], (col, col + w_s), ctx.net)
                                if gt is None and not split3_train:
                                    gt = _narrow_dgrad(dz, W_s, lw[0], (col, col + w_s))
                                grads_tables[s_i] = gt if gt is not None else dz @ W_s
                    col += w_s
                grads_params[0] = dW_cols[0] if n_seg == 1 else torch.cat(dW_cols, dim=1)
        grad_skip = [None if folded_skip else g] if ctx.has_skip else []
        return (None, None, None, *grads_tables, *grad_skip, *grads_params)


def fused_concat_mlp_train(net, segments, skip: Optional[torch.Tensor]):
    """differentiable evaluation on the kernel ``_route`` picks"""
    r = _route(net, segments, skip, train=True)
    if r is None:
        raise RuntimeError("fused_concat_mlp_train: unsupported arguments (call supported_train() first)")
    return _run(r, segments, skip)


# --------------------------------------------------------------------------- LayerNorm-less training variant
_ROW_WIDTHS = (64, 128, 256, 512, 1024)


def _act_rows_forward(z, act: int):
    """act(z) in one HIP pass (hgnn_act_rows_forward_f32); ATen at a width without instantiation"""
    M, W = int(z.shape[0]), int(z.shape[1])
    if W not in _ROW_WIDTHS or z.dtype != torch.float32:
        return _aten_act(z, act)
    out = torch.empty_like(z)
    if M:
        zc = _aligned16(z.contiguous())
        with torch.cuda.device(z.device):
            _lib.check(_lib.load().hgnn_act_rows_forward_f32(_lib.ptr(zc), M, W, int(act), _lib.ptr(out),
                                                             _lib.current_stream(z.device)), "hgnn_act_rows_forward_f32")
    return out


def _act_rows_backward(z, grad_out, act: int):
    """(grad_z, grad_bias) of a = act(z), z = x W^T + bias, in one HIP pass (hgnn_act_rows_backward_f32)"""
    M, W = int(z.shape[0]), int(z.shape[1])
    if W not in _ROW_WIDTHS or z.dtype != torch.float32:
        dz = _aten_act_backward(grad_out, z, act)
        return dz, dz.sum(dim=0)
    dz = torch.empty_like(z)
    partials = torch.empty((_lib.LN_ACT_BLOCKS, W), dtype=torch.float32, device=z.device)
    go = _aligned16(grad_out.contiguous().to(z.dtype))
    zc = _aligned16(z.contiguous())
    with torch.cuda.device(z.device):
        _lib.check(_lib.load().hgnn_act_rows_backward_f32(_lib.ptr(zc), _lib.ptr(go), M, W, int(act), _lib.ptr(dz),
                                                          _lib.ptr(partials), _lib.current_stream(z.device)),
                   "hgnn_act_rows_backward_f32")
    return dz, partials.sum(dim=0)


class _PlainMLPTrain(torch.autograd.Function):
    """Differentiable fused MLP without LayerNorm (route ``f32_plain``).  Forward: hgnn_mlp_forward_f32_plain dumping
    each activated layer's pre-activation rows z_l; a last layer without activation (a head's plain Linear) needs no
    dump, its dz is the incoming gradient.  Backward: dz_l = da_l * act'(z_l) with the bias gradient in one row pass
    (hgnn_act_rows_backward_f32), hidden activations recomputed from z_l (hgnn_act_rows_forward_f32), weight and data
    gradients exactly as in ``_FusedMLPTrain`` (``_atb``, gathered segments through the segmented reduce)."""

    @staticmethod
    def forward(ctx, route, indices, has_skip, *tensors):
        n_seg = len(indices)
        tables = list(tensors[:n_seg])
        skip = tensors[n_seg] if has_skip else None
        params = tensors[n_seg + (1 if has_skip else 0):]
        desc = _descriptor(route.net, list(zip(tables, indices)), skip, "f32_plain", layers=route.layers)
        if desc is None:
            raise RuntimeError("fused_concat_mlp_train (plain): unsupported arguments (call supported_train() first)")
        d, keep, M, n_out = desc
        n, dev = int(d.n_layers), tables[0].device
        acts = [int(d.act[l]) for l in range(n)]
        zs = [torch.empty((M, int(d.width[l + 1])), dtype=torch.float32, device=dev)
              for l in range(n) if l < n - 1 or acts[l] != 0]
        for l, z in enumerate(zs):
            d.save_pre[l] = z.data_ptr() if M else None
        out = torch.empty((M, n_out), dtype=torch.float32, device=dev)
        if M:
            with torch.cuda.device(dev):
                _forward("f32_plain", d, out, dev)
        del keep
        stats["fused_train_calls"] += 1
        ctx.indices, ctx.has_skip, ctx.n, ctx.net, ctx.layers, ctx.acts = indices, has_skip, n, route.net, route.layers, acts
        ctx.save_for_backward(*tables, *params, *zs)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        with torch.autocast("cuda", enabled=False):
            return _PlainMLPTrain._backward(ctx, grad_out.float())

    @staticmethod
    def _backward(ctx, grad_out):
        from .ops import _seg_reduce
        from .plan import get_plan
        n, indices, acts = ctx.n, ctx.indices, ctx.acts
        n_seg = len(indices)
        saved = ctx.saved_tensors
        tables = saved[:n_seg]
        params = saved[n_seg:n_seg + 2 * n]
        zs = saved[n_seg + 2 * n:]
        if int(grad_out.shape[0]) == 0:
            return _zero_grads(ctx, tables, params, grad_out, n_seg)
        W = [params[2 * l] for l in range(n)]
        lw = [lin.weight for lin, _, _ in ctx.layers]
        g = grad_out.contiguous()
        grads_params = [None] * (2 * n)
        grads_tables = [None] * n_seg
        da = g
        for l in range(n - 1, -1, -1):
            if acts[l] != 0:
                dz, dbias = _act_rows_backward(zs[l], da, acts[l])
            else:
                dz, dbias = da, da.sum(dim=0)
            grads_params[2 * l + 1] = dbias
            if l > 0:
                a_prev = _act_rows_forward(zs[l - 1], acts[l - 1])
                grads_params[2 * l] = _atb(dz, a_prev, ctx.net)
                del a_prev
                da = dz @ W[l]
                continue
            # first layer: gathered segments factor through S = segment_reduce(dz, idx) (see _FusedMLPTrain)
            dW_cols = []
            col = 0
            for s_i in range(n_seg):
                idx = indices[s_i]
                tab = tables[s_i].contiguous()
                w_s = int(tab.shape[1])
                W_s = W[0][:, col:col + w_s]
                src = dz if idx is None else _seg_reduce(get_plan(idx, int(tab.shape[0])), dz, None, None)
                dW_cols.append(_atb(src, tab, ctx.net))
                if ctx.needs_input_grad[3 + s_i]:
                    gt = _narrow_dgrad(src, W_s, lw[0], (col, col + w_s))
                    grads_tables[s_i] = gt if gt is not None else src @ W_s
                del src
                col += w_s
            grads_params[0] = dW_cols[0] if n_seg == 1 else torch.cat(dW_cols, dim=1)
        grad_skip = [g] if ctx.has_skip else []
        return (None, None, None, *grads_tables, *grad_skip, *grads_params)


# --------------------------------------------------------------------------- bf16 training variant
_train_bf16_enabled = True


def set_train_bf16(flag: bool) -> None:
    global _train_bf16_enabled
    _train_bf16_enabled = bool(flag)


# the fused backward layer at N = 1024 (hidden width of latent 512): default decided by tools/bench_bwd_layer.py --wide
# (DESIGN.md section 3); off = the unfused route (library GEMM + two HIP row passes).  Measured on 32-row tiles (the
# geometry without scratch): 8.9 against 8.0 ms at (512, 1024), 11.6 against 9.4 ms at (1024, 1024), M = 2M -- slower,
# so it ships OFF (profiles/bwd_layer_n1024.json)
_bwd_layer_wide = os.environ.get("HGNN_BWD_LAYER_WIDE", "0") == "1"


def set_bwd_layer_wide(flag: bool) -> None:
    """process default (the backward runs on autograd's thread, which no ``options`` context reaches): the bf16 training
    backward takes ``hgnn_mlp_backward_layer_bf16`` at N = 1024 too (HGNN_BWD_LAYER_WIDE=1)"""
    global _bwd_layer_wide
    _bwd_layer_wide = bool(flag)


def _bwd_layer_supported(K: int, N: int) -> bool:
    """the bf16 training backward routes this boundary to the fused backward layer"""
    if int(N) == 1024 and not _bwd_layer_wide:
        return False
    return bool(_lib.load().hgnn_mlp_backward_layer_supported_bf16(int(K), int(N)))


def _bwd_layer(dz, W, z_prev, gamma, beta, act, eps, skip=None, want_a=False):
    """``hgnn_mlp_backward_layer_bf16``.  W: the Linear's fp32 master weight [K, N] (or a column slice of it).
    LayerNorm form (z_prev given): returns (dz_prev, a_prev or None, dgamma, dbeta); input form: (dx,)."""
    M, K = int(dz.shape[0]), int(dz.shape[1])
    N = int(W.shape[1])
    dev = dz.device
    wt = _fragment_order(W.detach().t().to(torch.bfloat16).contiguous())      # W^T [N, K] in A-fragment order
    out = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    ln = z_prev is not None
    a_prev = torch.empty((M, N), dtype=torch.bfloat16, device=dev) if (ln and want_a) else None
    partials = torch.empty((_lib.MLP_BWD_BLOCKS, 2, N), dtype=torch.float32, device=dev) if ln else None
    gm = gamma.detach().float().contiguous() if ln else None
    bt = beta.detach().float().contiguous() if ln else None
    sk = skip.contiguous() if skip is not None else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().hgnn_mlp_backward_layer_bf16(
            _lib.ptr(dz.contiguous()), M, K, N, _lib.ptr(wt), _lib.ptr(z_prev), _lib.ptr(gm), _lib.ptr(bt), int(act),
            float(eps), _lib.ptr(sk), _lib.ptr(out), _lib.ptr(a_prev), _lib.ptr(partials),
            _lib.current_stream(dev)), "hgnn_mlp_backward_layer_bf16")
    stats["bwd_layer_calls"] += 1
    if not ln:
        return (out,)
    sums = partials.sum(dim=0)
    return out, a_prev, sums[0], sums[1]


def _seg_reduce_wide(plan, dz):
    """segmented reduce of bf16 rows wider than the bf16 row kernel's 512 columns: column blocks"""
    from .ops import _seg_reduce
    F = int(dz.shape[1])
    if F <= 512:
        return _seg_reduce(plan, dz, None, None)
    return torch.cat([_seg_reduce(plan, dz[:, c:c + 512].contiguous(), None, None) for c in range(0, F, 512)], dim=1)


# the fused backward layer of the EXACT fp32 route (hgnn_mlp_backward_layer_f32, csrc/mlp_bwd_f32.hip).  OFF: whether it
# beats the library GEMM + two HIP row passes is for tools/bench_bwd_layer.py --f32 to decide
_bwd_layer_f32_on = os.environ.get("HGNN_BWD_LAYER_F32", "0") == "1"


def set_bwd_layer_f32(flag: bool) -> None:
    """process default (the backward runs on autograd's thread, which no ``options`` context reaches): the exact fp32
    training backward forms its data gradients with ``hgnn_mlp_backward_layer_f32`` instead of library GEMMs + row
    passes, wherever the shape is supported (HGNN_BWD_LAYER_F32=1)"""
    global _bwd_layer_f32_on
    _bwd_layer_f32_on = bool(flag)


# the weight gradients of the EXACT fp32 route on hgnn_wgrad_f32 (csrc/wgrad_f32.hip) instead of the library's GEMMs.
# OFF: the default is decided by tools/bench_wgrad_f32.py and the 3 x spread rule
_wgrad_f32_on = os.environ.get("HGNN_WGRAD_F32", "0") == "1"


def set_wgrad_f32(flag: bool) -> None:
    """process default (the backward runs on autograd's thread, which no ``options`` context reaches): ``_atb`` -- every
    weight gradient dz^T a of the exact fp32 training backward, the N-row S^T table of gathered segments included --
    takes ``hgnn_wgrad_f32`` wherever both widths are multiples of 8 up to 1024 (HGNN_WGRAD_F32=1).  The opt-in
    split-bf16 route keeps precedence; independent of ``set_bwd_layer_f32``."""
    global _wgrad_f32_on
    _wgrad_f32_on = bool(flag)


# the forward pre-projections of the EXACT fp32 route on hgnn_project_f32 (csrc/project_f32.hip) instead of torch.matmul,
# and its products with one side at most 32 wide on the narrow kernels (csrc/narrow_f32.hip).  OFF: the defaults are
# decided by tools/bench_exact_tail.py and the 3 x spread rule
_project_f32_on = os.environ.get("HGNN_PROJECT_F32", "0") == "1"
_narrow_f32_on = os.environ.get("HGNN_NARROW_F32", "0") == "1"


def set_project_f32(flag: bool) -> None:
    """process default (the recompute of a checkpoint segment runs on autograd's thread, which no ``options`` context
    reaches): ``_preprojections`` takes ``hgnn_project_f32`` for fp32 tables whose (K, N) the entry accepts -- the
    no-grad exact route, both passes of a training step and the padded route (HGNN_PROJECT_F32=1).  bf16 rows and other
    shapes keep ``torch.matmul``; the split-bf16 projection keeps precedence; independent of the other switches."""
    global _project_f32_on
    _project_f32_on = bool(flag)


def set_narrow_f32(flag: bool) -> None:
    """process default: the exact fp32 route's narrow products leave the library (HGNN_NARROW_F32=1) -- the plain last
    Linear of a score head (forward ``hgnn_linear_narrow_f32``; backward ``hgnn_outer_narrow_f32`` +
    ``hgnn_wgrad_narrow_f32`` with its column sums), the weight gradients ``_atb`` with one width <= 32 that
    ``hgnn_wgrad_f32`` does not take, and the first layer's input gradients ``S @ W_s`` / ``dz @ W_s`` with w_s <= 32.
    The split-bf16 training route keeps precedence; independent of the other switches."""
    global _narrow_f32_on
    _narrow_f32_on = bool(flag)


def _narrow_widths(n: int, K: int) -> bool:
    """the narrow kernels' shapes: n the narrow width, K the wide one"""
    return 1 <= n <= 32 and 4 <= K <= 1024 and K % 4 == 0


def _count(name: str) -> None:
    stats[name] = stats.get(name, 0) + 1


class _NarrowLinear(torch.autograd.Function):
    """a head's plain last Linear ``hidden @ W^T + b`` with W [w <= 32, H] on the narrow kernels"""

    @staticmethod
    def forward(ctx, hidden, W, b):
        from .ops import linear_narrow_f32
        ctx.save_for_backward(hidden, W)
        ctx.has_bias = b is not None
        _count("narrow_linear_calls")
        return linear_narrow_f32(hidden.detach(), W.detach(), b.detach() if b is not None else None)

    @staticmethod
    def backward(ctx, dy):
        from .ops import outer_narrow_f32, wgrad_narrow_f32
        hidden, W = ctx.saved_tensors
        dy = dy.float()
        dh = None
        if ctx.needs_input_grad[0]:
            _count("narrow_outer_calls")
            dh = outer_narrow_f32(dy, W.detach())
        db = torch.empty(int(W.shape[0]), dtype=torch.float32, device=dy.device) if ctx.has_bias else None
        _count("narrow_wgrad_calls")
        dW = wgrad_narrow_f32(dy, hidden, colsum=db)
        return dh, dW, db


def _head_linear(hidden, lin, differentiable: bool):
    """the plain last Linear of a score head on the narrow kernels (``set_narrow_f32``), or None: the caller evaluates
    its library expression, counted here"""
    W, b = lin.weight, lin.bias
    if _narrow_f32_on and hidden.is_cuda and hidden.dtype == torch.float32 and W.dtype == torch.float32 \
            and (b is None or b.dtype == torch.float32) and _narrow_widths(int(W.shape[0]), int(W.shape[1])):
        if differentiable:
            return _NarrowLinear.apply(hidden, W, b)
        from .ops import linear_narrow_f32
        _count("narrow_linear_calls")
        return linear_narrow_f32(hidden, W.detach(), b.detach() if b is not None else None)
    _count("library_head_calls")
    return None


def _narrow_dgrad(x, W_s, weight, cols):
    """``x @ W_s`` for the first layer's W_s = weight[:, cols] [H, w_s <= 32] on ``hgnn_linear_narrow_f32`` (its weight
    is the small transposed copy W_s^T, cached per weight like ``_transposed_weight_f32``), or None: the caller's
    library expression, counted here while ``set_narrow_f32`` is on"""
    if not _narrow_f32_on:
        return None
    if x.is_cuda and x.dtype == torch.float32 and W_s.dtype == torch.float32 \
            and _narrow_widths(int(W_s.shape[1]), int(W_s.shape[0])):
        from .ops import linear_narrow_f32
        _count("narrow_linear_calls")
        return linear_narrow_f32(x, _transposed_weight_f32(W_s, weight, cols))
    stats["library_dgrad_calls"] += 1
    return None


def _bwd_layer_f32_supported(K: int, N: int) -> bool:
    """the exact fp32 training backward routes this boundary to the fused fp32 backward layer"""
    if not _bwd_layer_f32_on:
        return False
    return bool(_lib.load().hgnn_mlp_backward_layer_supported_f32(int(K), int(N)))


def _transposed_weight_f32(W, weight, cols):
    """W^T [N, K] row-major fp32 of W = weight[:, cols]; with the Parameter ``weight`` given the copy is cached per
    weight object and version (``_cached``), otherwise made from ``W`` itself"""
    if weight is None:
        return W.detach().float().t().contiguous()

    def make():
        Wd = weight.detach().float()
        if cols is not None:
            Wd = Wd[:, cols[0]:cols[1]]
        return Wd.t().contiguous()
    return _cached(weight, ("bwd_layer_f32", None if cols is None else tuple(cols)), make)


def _aligned16(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _bwd_layer_f32(dz, W, z_prev, gamma, beta, act, eps, skip=None, want_a=False, weight=None, cols=None):
    """``hgnn_mlp_backward_layer_f32``.  W: the Linear's fp32 weight [K, N] (or a column slice of it); ``weight`` /
    ``cols``: the Parameter W comes from and the column range taken, which let the W^T copy live in the weight cache.
    LayerNorm form (z_prev given): returns (dz_prev, a_prev or None, dgamma, dbeta, dbias); input form: (dx,)."""
    if not (dz.is_cuda and W.is_cuda):
        raise RuntimeError("_bwd_layer_f32 needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    if dz.dtype != torch.float32 or (z_prev is not None and z_prev.dtype != torch.float32) \
            or (skip is not None and skip.dtype != torch.float32):
        raise RuntimeError("_bwd_layer_f32: float32 rows only")
    M, K = int(dz.shape[0]), int(dz.shape[1])
    N = int(W.shape[1])
    dev = dz.device
    ln = z_prev is not None
    if M == 0:      # nothing to launch (an empty tensor has no address to tell the two forms apart by)
        zero = torch.zeros((0, N), dtype=torch.float32, device=dev)
        sums = torch.zeros((3, N), dtype=torch.float32, device=dev)
        return (zero, zero.clone() if want_a else None, sums[0], sums[1], sums[2]) if ln else (zero,)
    wt = _transposed_weight_f32(W, weight, cols)
    out = torch.empty((M, N), dtype=torch.float32, device=dev)
    a_prev = torch.empty((M, N), dtype=torch.float32, device=dev) if (ln and want_a) else None
    partials = torch.empty((_lib.MLP_BWD_F32_BLOCKS, 3, N), dtype=torch.float32, device=dev) if ln else None
    # the kernel reads 16-byte pieces: a view that starts off that grid (a slice of a flattened parameter buffer) is copied
    gm = _aligned16(gamma.detach().float().contiguous()) if ln else None
    bt = _aligned16(beta.detach().float().contiguous()) if ln else None
    zp = _aligned16(z_prev.contiguous()) if ln else None
    sk = _aligned16(skip.contiguous()) if skip is not None else None
    dzc = _aligned16(dz.contiguous())
    with torch.cuda.device(dev):
        _lib.check(_lib.load().hgnn_mlp_backward_layer_f32(
            _lib.ptr(dzc), M, K, N, _lib.ptr(wt), _lib.ptr(zp), _lib.ptr(gm), _lib.ptr(bt), int(act),
            float(eps), _lib.ptr(sk), _lib.ptr(out), _lib.ptr(a_prev), _lib.ptr(partials),
            _lib.current_stream(dev)), "hgnn_mlp_backward_layer_f32")
    stats["bwd_layer_f32_calls"] += 1
    if not ln:
        return (out,)
    sums = partials.sum(dim=0)
    return out, a_prev, sums[0], sums[1], sums[2]


class _FusedMLPTrainBf16(torch.autograd.Function):
    """Differentiable fused MLP on bf16 rows (BASELINE config 4 dtype; fp32 master weights).

    forward : the feature-split bf16-MFMA kernel, additionally dumping every layer's pre-LayerNorm rows
              z_l in bf16 (``hgnn_mlp_desc.save_pre``);
    backward: per layer ONE HIP row pass for activation' -> LayerNorm backward -> dgamma / dbeta / dbias
              (``hgnn_ln_act_backward_bf16``), the hidden activations recomputed from z_l in one more
              (``hgnn_ln_act_forward_bf16``), the WEIGHT gradients by the hand-written split-K bf16-MFMA
              kernel ``hgnn_wgrad_bf16`` (fp32 accumulation, deterministic: the library's TN GEMM reaches
              140-370 TFLOP/s on this tall reduction, 3.3-4.3x slower), the data gradients by bf16
              library GEMMs; gathered segments factor through the atomics-free segmented reduce exactly
              as in the fp32 variant (N-row products instead of M-row ones)."""

    @staticmethod
    def forward(ctx, route, indices, has_skip, *tensors):
        out, tables, skip, _ = _train_forward(ctx, route, indices, has_skip, tensors)
        # skip is the same tensor as a direct (un-gathered) segment: its gradient is folded into that segment's
        ctx.skip_seg = -1
        if has_skip:
            for s_i in range(len(indices)):
                t = tables[s_i]
                if indices[s_i] is None and ctx.needs_input_grad[3 + s_i] and ctx.needs_input_grad[3 + len(indices)] \
                        and t.data_ptr() == skip.data_ptr() and t.shape == skip.shape and t.stride() == skip.stride():
                    ctx.skip_seg = s_i
        return out

    @staticmethod
    def backward(ctx, grad_out):
        with torch.autocast("cuda", enabled=False):
            return _FusedMLPTrainBf16._backward(ctx, grad_out)

    @staticmethod
    def _backward(ctx, grad_out):
        from .ops import wgrad_bf16
        from .plan import get_plan
        n, indices = ctx.n, ctx.indices
        n_seg = len(indices)
        saved = ctx.saved_tensors
        tables = saved[:n_seg]
        params = saved[n_seg:n_seg + 4 * n]
        zs = saved[n_seg + 4 * n:]
        if int(grad_out.shape[0]) == 0:
            return _zero_grads(ctx, tables, params, grad_out, n_seg)
        W = [params[4 * l] for l in range(n)]
        lnw = [params[4 * l + 2] for l in range(n)]
        lnb = [params[4 * l + 3] for l in range(n)]
        bf = torch.bfloat16
        g = grad_out.contiguous().to(bf)
        grads_params = [None] * (4 * n)
        grads_tables = [None] * n_seg
        pdt = [params[4 * l].dtype for l in range(n)]
        # last layer: its LayerNorm / activation backward has no GEMM in front of it (one HIP row pass)
        dz, dlw, dlb, dbias = _ln_act_backward(zs[n - 1], g, lnw[n - 1], lnb[n - 1], ctx.acts[n - 1], ctx.eps)
        grads_params[4 * (n - 1) + 1] = dbias.to(pdt[n - 1])
        grads_params[4 * (n - 1) + 2] = dlw.to(pdt[n - 1])
        grads_params[4 * (n - 1) + 3] = dlb.to(pdt[n - 1])
        for l in range(n - 1, 0, -1):
            K, N = int(W[l].shape[0]), int(W[l].shape[1])
            need_bias = grads_params[4 * l + 1] is None
            colsum = torch.empty(K, dtype=torch.float32, device=dz.device) if need_bias else None
            if _bwd_layer_supported(K, N):
                # hand-written data gradient fused with the LayerNorm / activation backward of the layer below
                dz_prev, a_prev, dlw, dlb = _bwd_layer(dz, W[l], zs[l - 1], lnw[l - 1], lnb[l - 1], ctx.acts[l - 1],
                                                       ctx.eps, want_a=True)
                grads_params[4 * l] = wgrad_bf16(dz, a_prev, colsum=colsum).to(pdt[l])
                del a_prev
                dbias_prev = None                                         # comes out of layer l-1's weight gradient
            else:
                a_prev = _ln_act_forward(zs[l - 1], lnw[l - 1], lnb[l - 1], ctx.acts[l - 1], ctx.eps)
                grads_params[4 * l] = wgrad_bf16(dz, a_prev, colsum=colsum).to(pdt[l])
                del a_prev
                da = dz @ W[l].detach().to(bf)                            # data gradient: bf16 library GEMM
                stats["library_dgrad_calls"] += 1
                dz_prev, dlw, dlb, dbias_prev = _ln_act_backward(zs[l - 1], da, lnw[l - 1], lnb[l - 1],
                                                                 ctx.acts[l - 1], ctx.eps)
                del da
            if need_bias:
                grads_params[4 * l + 1] = colsum.to(pdt[l])
            grads_params[4 * (l - 1) + 2] = dlw.to(pdt[l - 1])
            grads_params[4 * (l - 1) + 3] = dlb.to(pdt[l - 1])
            if dbias_prev is not None:
                grads_params[4 * (l - 1) + 1] = dbias_prev.to(pdt[l - 1])
            dz = dz_prev
        # first layer: gathered segments factor through S = segment_reduce(dz, idx) (see _FusedMLPTrain)
        need_bias = grads_params[1] is None
        W0 = W[0].detach().to(bf)
        dW = torch.empty(tuple(W[0].shape), dtype=torch.float32, device=dz.device)
        H0 = int(W[0].shape[0])
        col = 0
        for s_i in range(n_seg):
            idx = indices[s_i]
            tab = tables[s_i].contiguous()
            w_s = int(tab.shape[1])
            W_s = W0[:, col:col + w_s]
            if idx is not None:
                S = _seg_reduce_wide(get_plan(idx, int(tab.shape[0])), dz)
                dW[:, col:col + w_s] = wgrad_bf16(S, tab)
                if ctx.needs_input_grad[3 + s_i]:
                    grads_tables[s_i] = S @ W_s
                del S
            else:
                colsum = torch.empty(H0, dtype=torch.float32, device=dz.device) if need_bias else None
                dW[:, col:col + w_s] = wgrad_bf16(dz, tab, colsum=colsum)
                if need_bias:
                    grads_params[1] = colsum.to(pdt[0])
                    need_bias = False
                if ctx.needs_input_grad[3 + s_i]:
                    folded = ctx.skip_seg == s_i          # edges + MLP(..., edges): both gradients in one epilogue
                    if _bwd_layer_supported(H0, w_s):
                        grads_tables[s_i] = _bwd_layer(dz, W[0][:, col:col + w_s], None, None, None, 0, ctx.eps,
                                                       skip=g if folded else None)[0]
                    elif folded:
                        grads_tables[s_i] = torch.addmm(g, dz, W_s)
                        stats["library_dgrad_calls"] += 1
                    else:
                        grads_tables[s_i] = dz @ W_s
                        stats["library_dgrad_calls"] += 1
            col += w_s
        if need_bias:
            grads_params[1] = dz.float().sum(dim=0).to(pdt[0])
        grads_params[0] = dW.to(pdt[0])
        grad_skip = [None if ctx.skip_seg >= 0 else g] if ctx.has_skip else []
        return (None, None, None, *grads_tables, *grad_skip, *grads_params)
