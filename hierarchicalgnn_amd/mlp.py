"""``concat -> make_mlp Sequential -> (+skip)`` evaluation for the cells.

Every MLP on the hot path has the shape  out = MLP(cat[seg_0, seg_1, seg_2]) + skip
where each segment is either a tensor or a row gather ``table[index]``
(Modules/gnn_utils.py:52-53, :61-62, :124-126, :134, :142-144, :152).

``concat_mlp`` is the single entry point the cells use.  Gathers run in the HIP
row-gather kernel (backward: atomics-free segmented reduce).  The dense layers
are evaluated by the fused fp32-MFMA kernel when the shape is supported
(``fused.py``: forward-only when autograd is off, a differentiable variant with a
hand-written backward when it records), otherwise by the library GEMM path (rocBLAS
through ATen) -- all on the GPU; none is a CPU fallback.  Every call that takes the library
path is counted in ``fused.stats["library_calls"]``; with the ``strict`` option
(``fused.options(strict=True)`` / ``fused.set_strict``) it raises instead.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from .ops import gather_rows

Segment = Tuple[torch.Tensor, Optional[torch.Tensor]]  # (table, index or None)


def _hybrid(net, segments, skip, train: bool):
    """the hybrid chain of the encoders in bf16 latent mode: the first Linear -> LayerNorm -> act on the fp32 rows,
    the cast, the rest on bf16 rows; None unless a fused route exists for both"""
    from . import fused
    if skip is not None or len(net) <= 3 or train != torch.is_grad_enabled() or not fused._opt("enabled") \
            or not all(t.dtype == torch.float32 and t.is_cuda for t, _ in segments):
        return None
    first, rest = nn.Sequential(*list(net)[:3]), nn.Sequential(*list(net)[3:])
    # (the square single layers below 512 are not asked: those encoders keep the routes they have)
    r_first = fused._route(first, segments, None, train=train, allow_square=False)
    probe = [(torch.empty((0, net[0].out_features), dtype=torch.bfloat16, device=segments[0][0].device), None)]
    r_rest = None if r_first is None else fused._route(rest, probe, None, train=train)
    if r_rest is None:
        return None
    if train:
        fused.stats["hybrid_train_calls"] += 1
    return fused._run(r_rest, [(fused._run(r_first, segments, None).to(torch.bfloat16), None)], None)


def concat_mlp(net: nn.Sequential, segments: Sequence[Segment], skip: Optional[torch.Tensor] = None,
               bf16_tail: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``bf16_tail`` (bf16 latent mode, encoders): when an fp32-input MLP has no fused kernel, keep its
    first Linear in fp32 (hit coordinates must not be rounded to 8 bits) and run the rest -- the wide
    GEMMs -- in bf16; the result is bf16."""
    from . import fused
    if out is not None:
        # caller-supplied output rows (no-grad only): straight into the fused kernel when it takes the shape,
        # otherwise evaluated as usual and copied
        if torch.is_grad_enabled() and any(t.requires_grad for t, _ in segments):
            raise RuntimeError("concat_mlp(out=...) is a no-grad path")
        r = None if bf16_tail else fused._route(net, segments, skip, train=False)
        if r is not None:
            return fused._run(r, segments, skip, out=out)
        return out.copy_(concat_mlp(net, segments, skip, bf16_tail))
    # bf16 latent mode, encoders: hybrid chain -- the first Linear (hit coordinates: must not be rounded to 8 bits) as
    # ONE fp32 fused layer, the wide tail on the bf16 feature-split kernel (edge encoder at latent 256, 2M rows: 3.0
    # instead of 5.6 ms for the all-fp32 fused kernel)
    y = _hybrid(net, segments, skip, train=False) if bf16_tail else None
    if y is not None:
        return y
    # (bf16 latent mode keeps its bf16 tail where the encoders have no kernel today: the square route is not asked)
    r = fused._route(net, segments, skip, train=False, allow_chain=not bf16_tail, allow_square=not bf16_tail) \
        or fused._route(net, segments, skip, train=True, allow_square=not bf16_tail)
    if r is not None:
        return fused._run(r, segments, skip)
    # the same hybrid chain under autograd (encoders at latent 512, whose 1024-wide hidden layers have no fp32 training
    # kernel): the first Linear as ONE differentiable fp32 layer (small-K, dump at its real width), the cast, the wide
    # tail on the differentiable bf16 feature-split kernel -- only when both routes exist
    y = _hybrid(net, segments, skip, train=True) if bf16_tail else None
    if y is not None:
        return y
    if not torch.is_grad_enabled() and fused._opt("enabled") and not bf16_tail \
            and fused._ctx_training_forward.get() == 0 \
            and all(t.dtype == torch.bfloat16 and t.is_cuda for t, _ in segments) \
            and (skip is None or skip.dtype == torch.bfloat16) and next(net.parameters()).dtype == torch.float32 \
            and not fused._is_plain(fused._parse(net)):    # bf16 rows without LayerNorm keep the library path
        # bf16 rows and a net no bf16 kernel accepts (the supernode encoder, latent - emb_dim outputs: the bf16 kernels
        # have no real-width LayerNorm): the fp32 kernels on the rows cast up, the result cast down -- a few thousand
        # pooled rows, the casts are noise.  Not in the no-grad pass of a checkpointed training step: its recompute
        # under autograd takes the library path, and the two must agree
        seg32 = [(t.float(), i) for t, i in segments]
        skip32 = None if skip is None else skip.float()
        r = fused._route(net, seg32, skip32, train=False, allow_square=False)   # bf16 rows at hidden = latent: library path
        if r is not None:
            return fused._run(r, seg32, skip32).to(torch.bfloat16)
    if fused._opt("strict"):
        widths = [m.in_features for m in net if isinstance(m, nn.Linear)][:1] + \
            [m.out_features for m in net if isinstance(m, nn.Linear)]
        raise RuntimeError(
            "concat_mlp (strict): no fused kernel for layer widths " + " -> ".join(str(w) for w in widths) +
            f", rows {[str(t.dtype) for t, _ in segments]} of widths {[int(t.shape[1]) for t, _ in segments]}"
            f", parameters {next(net.parameters()).dtype}, skip={skip is not None}, bf16_tail={bf16_tail}"
            f", autograd {'on' if torch.is_grad_enabled() else 'off'}: this call would run on library GEMMs")
    fused.stats["library_calls"] += 1
    parts: List[torch.Tensor] = []
    for table, index in segments:
        parts.append(table if index is None else gather_rows(table, index))
    x = parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)
    if bf16_tail and x.dtype == torch.float32 and x.is_cuda and isinstance(net[0], nn.Linear) and len(net) > 1:
        y = net[0](x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = net[1:](y)
        y = y.to(torch.bfloat16)
    elif x.dtype == torch.bfloat16 and next(net.parameters()).dtype == torch.float32:
        # bf16 feature rows with fp32 master weights (hparams["feature_dtype"] = "bf16"): library
        # GEMMs in bf16, LayerNorm statistics in fp32 -- what autocast does
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = net(x)
        y = y.to(torch.bfloat16)
    else:
        y = net(x)
    return y if skip is None else y + skip
