"""Operator-level drop-ins backed by libhgnn_hip.so.

``scatter_add(src, index, dim=0, dim_size=N)`` keeps torch_scatter's calling
convention exactly as the reference uses it (Modules/gnn_utils.py:50,124,125,
142,143; BipartiteClassification/Models/HGNN_GMM.py:269).  The fused forms
(``gather_scale_scatter``) compute ``scatter_add(w * X[g], d, dim_size)``
without materialising the ``[B, L]`` product the reference builds first.

All functions are ``torch.autograd.Function``s with hand-written HIP backward
kernels; they hold no per-call state and are safe under reentrant
``torch.utils.checkpoint`` recompute (gnn_utils.py:14-15).  fp32, HIP device
tensors only: anything else raises (there is no CPU fallback).
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib
from .plan import GraphPlan, get_plan


def _require_hip(t: torch.Tensor, name: str, allow_bf16: bool = False):
    if not t.is_cuda:
        raise RuntimeError(f"hierarchicalgnn_amd: `{name}` must be a HIP device tensor "
                           "(no CPU fallback; build + run on an MI355X)")
    if t.dtype != torch.float32 and not (allow_bf16 and t.dtype == torch.bfloat16):
        raise RuntimeError(f"hierarchicalgnn_amd: `{name}` must be float32"
                           + (" or bfloat16" if allow_bf16 else "") + f", got {t.dtype}")


def _f32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """weights / row scales are always handed to the kernels as fp32"""
    return None if t is None else (t if t.dtype == torch.float32 else t.float())


def _seg_reduce(plan: GraphPlan, src2d: torch.Tensor, weight: Optional[torch.Tensor],
                row_scale: Optional[torch.Tensor]) -> torch.Tensor:
    F = int(src2d.shape[1])
    out = torch.empty((plan.N, F), dtype=src2d.dtype, device=src2d.device)
    if plan.N == 0 or F == 0:
        return out
    lib = _lib.load()
    weight, row_scale = _f32(weight), _f32(row_scale)
    bf16 = src2d.dtype == torch.bfloat16
    if not bf16 and weight is None and row_scale is None:
        # plain fp32: one launch per call, work items in the plan's longest-first order where that is switched on
        order = plan.item_order() if _lib.get_option("k1_item_order") else None
        with torch.cuda.device(src2d.device):
            _lib.check(lib.hgnn_segment_reduce_f32_ex(
                ctypes.byref(plan.c), _lib.ptr(src2d), F, None, None, _lib.ptr(out), _lib.ptr(plan.partial(F)),
                _lib.ptr(plan.arrive), _lib.ptr(order), _lib.current_stream(src2d.device)),
                "hgnn_segment_reduce_f32_ex")
        return out
    fn = lib.hgnn_segment_reduce_bf16 if bf16 else lib.hgnn_segment_reduce_f32
    with torch.cuda.device(src2d.device):
        _lib.check(fn(ctypes.byref(plan.c), _lib.ptr(src2d), F, _lib.ptr(weight), _lib.ptr(row_scale),
                      _lib.ptr(out), _lib.ptr(plan.partial(F)), _lib.current_stream(src2d.device)),
                   "hgnn_segment_reduce_bf16" if bf16 else "hgnn_segment_reduce_f32")
    return out


def _gather_rows(table: torch.Tensor, idx32: torch.Tensor, M: int, weight: Optional[torch.Tensor] = None,
                 row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    F = int(table.shape[1])
    out = torch.empty((M, F), dtype=table.dtype, device=table.device)
    if M == 0 or F == 0:
        return out
    lib = _lib.load()
    weight, row_scale = _f32(weight), _f32(row_scale)
    with torch.cuda.device(table.device):
        if table.dtype == torch.bfloat16:
            if row_scale is not None:
                raise RuntimeError("gather_rows: row_scale is not implemented for bfloat16 tables")
            _lib.check(lib.hgnn_gather_rows_bf16(
                _lib.ptr(table), int(table.shape[0]), F, _lib.ptr(idx32), M, _lib.ptr(weight),
                _lib.ptr(out), _lib.current_stream(table.device)), "hgnn_gather_rows_bf16")
        else:
            _lib.check(lib.hgnn_gather_rows_f32(
                _lib.ptr(table), int(table.shape[0]), F, _lib.ptr(idx32), M, _lib.ptr(weight),
                _lib.ptr(row_scale), _lib.ptr(out), _lib.current_stream(table.device)),
                "hgnn_gather_rows_f32")
    return out


def _spread_rows(plan: GraphPlan, table: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[e] = w[e] * table[index[e]] walked in destination order (each table row read once)"""
    F = int(table.shape[1])
    alloc = torch.empty if plan.validated else torch.zeros
    out = alloc((plan.M, F), dtype=table.dtype, device=table.device)
    if plan.M == 0 or F == 0:
        return out
    lib = _lib.load()
    weight = _f32(weight)
    bf16 = table.dtype == torch.bfloat16
    fn = lib.hgnn_spread_rows_bf16 if bf16 else lib.hgnn_spread_rows_f32
    with torch.cuda.device(table.device):
        _lib.check(fn(ctypes.byref(plan.c), _lib.ptr(table), F, _lib.ptr(weight), _lib.ptr(out),
                      _lib.current_stream(table.device)),
                   "hgnn_spread_rows_bf16" if bf16 else "hgnn_spread_rows_f32")
    return out


def _edge_dot(A: torch.Tensor, ai: Optional[torch.Tensor], B: torch.Tensor, bi: Optional[torch.Tensor],
              M: int) -> torch.Tensor:
    F = int(A.shape[1])
    A, B = _f32(A), _f32(B)   # bf16 rows are widened once here (B <= 600k rows); the dot is fp32
    out = torch.empty((M,), dtype=torch.float32, device=A.device)
    if M == 0:
        return out
    lib = _lib.load()
    with torch.cuda.device(A.device):
        _lib.check(lib.hgnn_edge_dot_f32(
            _lib.ptr(A), _lib.ptr(ai), int(A.shape[0]), _lib.ptr(B), _lib.ptr(bi), int(B.shape[0]),
            F, M, _lib.ptr(out), _lib.current_stream(A.device)), "hgnn_edge_dot_f32")
    return out


# --------------------------------------------------------------------------- K1 / K4
class _ScatterAdd(torch.autograd.Function):
    """out[d] = sum_{e: index[e]=d} (w[e] *) src[e]"""

    @staticmethod
    def forward(ctx, src, weight, plan: GraphPlan):
        src_c = src.contiguous()
        w_c = weight.contiguous().view(-1) if weight is not None else None
        ctx.plan = plan
        ctx.has_w = weight is not None
        ctx.w_shape = weight.shape if weight is not None else None
        ctx.w_dtype = weight.dtype if weight is not None else None
        if ctx.has_w:
            ctx.save_for_backward(src_c, w_c)
        return _seg_reduce(plan, src_c, w_c, None)

    @staticmethod
    def backward(ctx, grad_out):
        plan = ctx.plan
        g = grad_out.contiguous()
        grad_src = grad_w = None
        if ctx.has_w:
            src_c, w_c = ctx.saved_tensors
            if ctx.needs_input_grad[0]:
                grad_src = _spread_rows(plan, g, weight=w_c)
            if ctx.needs_input_grad[1]:
                grad_w = _edge_dot(src_c, None, g, plan.dst32, plan.M).view(ctx.w_shape).to(ctx.w_dtype)
        elif ctx.needs_input_grad[0]:
            grad_src = _spread_rows(plan, g)
        return grad_src, grad_w, None


def scatter_add(src: torch.Tensor, index: torch.Tensor, dim: int = 0, dim_size: Optional[int] = None,
                out=None, plan: Optional[GraphPlan] = None, weight: Optional[torch.Tensor] = None,
                validate: bool = True) -> torch.Tensor:
    """torch_scatter.scatter_add for the call shape the reference uses.

    src   Tensor[M, ...] float32 / bfloat16, or int32 / int64 (exact, wrapping integer sum);
    index LongTensor[M] (broadcast along features).  ``dim`` other than 0 moves that dimension to the
    front and back again.  Returns a freshly allocated Tensor[dim_size, ...] with zero rows for absent
    destinations.  Differentiable w.r.t. floating-point ``src`` (and ``weight``).
    ``weight`` (Tensor[M] or [M,1]) is an extension: fused ``scatter_add(src*weight, ...)``
    as at Modules/gnn_utils.py:143.  ``validate=False`` (an index this package produced itself, known to
    be in range) skips the one host read a new plan makes to raise on out-of-range entries.
    """
    if out is not None:
        raise RuntimeError("hierarchicalgnn_amd.scatter_add: `out=` is not supported")
    if src.dtype in _INT_DTYPES:
        if weight is not None:
            raise RuntimeError("hierarchicalgnn_amd.scatter_add: `weight` needs floating-point src")
        return _scatter_ex(src, index, dim, dim_size, plan, validate, _lib.RED_SUM, "scatter_add")[0]
    d = _norm_dim(dim, src.dim(), "scatter_add")
    if d != 0:
        return scatter_add(src.movedim(d, 0), index, 0, dim_size, plan=plan, weight=weight,
                           validate=validate).movedim(0, d)
    _require_hip(src, "src", allow_bf16=True)
    if index.dim() != 1 or index.shape[0] != src.shape[0]:
        raise RuntimeError("hierarchicalgnn_amd.scatter_add: index must be 1-D with one entry per row of src")
    if index.device != src.device:
        raise RuntimeError("hierarchicalgnn_amd.scatter_add: index and src are on different devices")
    if dim_size is None:
        dim_size = int(index.max().item()) + 1 if index.numel() else 0
    dim_size = int(dim_size)
    if plan is None:
        plan = get_plan(index, dim_size, validate=validate)
    elif plan.M != index.numel() or plan.N != dim_size or plan.c.has_gather:
        raise RuntimeError("hierarchicalgnn_amd.scatter_add: plan does not match index/dim_size")
    trailing = tuple(src.shape[1:])
    width = 1
    for t in trailing:
        width *= int(t)
    src2d = src.reshape(src.shape[0], width)
    if weight is not None:
        _require_hip(weight, "weight", allow_bf16=True)
        if weight.numel() != src.shape[0]:
            raise RuntimeError("hierarchicalgnn_amd.scatter_add: weight must have one entry per row")
    res = _ScatterAdd.apply(src2d, weight, plan)
    return res.reshape((dim_size,) + trailing)


# --------------------------------------------------------------------------- scatter_min / scatter_max / integer sums
_INT_DTYPES = (torch.int32, torch.int64)
_EX_DTYPES = {torch.float32: _lib.DT_F32, torch.bfloat16: _lib.DT_BF16, torch.int32: _lib.DT_I32,
              torch.int64: _lib.DT_I64}


def _norm_dim(dim: int, ndim: int, what: str) -> int:
    d = int(dim) + ndim if int(dim) < 0 else int(dim)
    if not 0 <= d < ndim:
        raise RuntimeError(f"hierarchicalgnn_amd.{what}: dim {dim} out of range for a {ndim}-d src")
    return d


def _seg_ex(plan: GraphPlan, op: int, src2d: torch.Tensor):
    """hgnn_segment_reduce_ex over a contiguous [M, F] src: (out[N, F], arg[N, F] int64 or None for SUM)"""
    F = int(src2d.shape[1])
    out = torch.empty((plan.N, F), dtype=src2d.dtype, device=src2d.device)
    arg = None if op == _lib.RED_SUM else torch.empty((plan.N, F), dtype=torch.int64, device=src2d.device)
    if plan.N == 0 or F == 0:
        return out, arg
    lib = _lib.load()
    partial, partial_arg = plan.partial_ex(F, src2d.dtype)
    with torch.cuda.device(src2d.device):
        _lib.check(lib.hgnn_segment_reduce_ex(
            ctypes.byref(plan.c), op, _EX_DTYPES[src2d.dtype], _lib.ptr(src2d), F, _lib.ptr(out), _lib.ptr(arg),
            _lib.ptr(partial), None if op == _lib.RED_SUM else _lib.ptr(partial_arg),
            _lib.current_stream(src2d.device)), "hgnn_segment_reduce_ex")
    return out, arg


def _arg_backward(arg: torch.Tensor, grad_out: torch.Tensor, M: int) -> torch.Tensor:
    """grad_src[arg[d, f], f] = grad_out[d, f], zeros elsewhere"""
    N, F = int(arg.shape[0]), int(arg.shape[1])
    grad_src = torch.zeros((M, F), dtype=grad_out.dtype, device=grad_out.device)
    if M == 0 or F == 0:
        return grad_src
    lib = _lib.load()
    with torch.cuda.device(grad_out.device):
        _lib.check(lib.hgnn_segment_arg_backward(
            _lib.ptr(arg), N, F, M, _EX_DTYPES[grad_out.dtype], _lib.ptr(grad_out), _lib.ptr(grad_src),
            _lib.current_stream(grad_out.device)), "hgnn_segment_arg_backward")
    return grad_src


class _ScatterArgReduce(torch.autograd.Function):
    """(out, arg)[d] = min / max over {(src[e], e): index[e] = d}; the gradient goes to row arg only"""

    @staticmethod
    def forward(ctx, src2d, plan: GraphPlan, op: int):
        out, arg = _seg_ex(plan, op, src2d)
        ctx.mark_non_differentiable(arg)
        ctx.save_for_backward(arg)
        ctx.M = plan.M
        return out, arg

    @staticmethod
    def backward(ctx, grad_out, grad_arg):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        arg, = ctx.saved_tensors
        return _arg_backward(arg, grad_out.contiguous(), ctx.M), None, None


def _scatter_ex(src, index, dim, dim_size, plan, validate, op, what):
    """shared front end of the hgnn_segment_reduce_ex operators: returns (out, arg) shaped like torch_scatter's"""
    if src.dtype not in _EX_DTYPES:
        raise RuntimeError(f"hierarchicalgnn_amd.{what}: unsupported dtype {src.dtype} "
                           "(float32, bfloat16, int32 and int64 are implemented)")
    if not src.is_cuda or not index.is_cuda:
        raise RuntimeError(f"hierarchicalgnn_amd.{what}: src and index must be HIP device tensors "
                           "(no CPU fallback; build + run on an MI355X)")
    d = _norm_dim(dim, src.dim(), what)
    if index.dim() != 1 or index.numel() != src.shape[d]:
        raise RuntimeError(f"hierarchicalgnn_amd.{what}: index must be 1-D with one entry per element of src "
                           f"along dim {d} (got index {tuple(index.shape)}, src {tuple(src.shape)})")
    if index.device != src.device:
        raise RuntimeError(f"hierarchicalgnn_amd.{what}: index and src are on different devices")
    if index.dtype != torch.int64:
        index = index.long()
    if dim_size is None:
        dim_size = int(index.max().item()) + 1 if index.numel() else 0
    dim_size = int(dim_size)   # an int, or a 0-d tensor such as pid.max() + 1
    if plan is None:
        plan = get_plan(index, dim_size, validate=validate)
    elif plan.M != index.numel() or plan.N != dim_size or plan.c.has_gather:
        raise RuntimeError(f"hierarchicalgnn_amd.{what}: plan does not match index/dim_size")
    x = src.movedim(d, 0)
    rest = tuple(x.shape[1:])
    F = 1
    for t in rest:
        F *= int(t)
    x2 = x.reshape(int(x.shape[0]), F).contiguous()
    if op == _lib.RED_SUM:
        out, arg = _seg_ex(plan, op, x2)
    else:
        out, arg = _ScatterArgReduce.apply(x2, plan, op)
    shape = (dim_size,) + rest
    out = out.reshape(shape).movedim(0, d)
    arg = None if arg is None else arg.reshape(shape).movedim(0, d)
    if d != 0:
        out = out.contiguous()
        arg = None if arg is None else arg.contiguous()
    return out, arg


def scatter_min(src: torch.Tensor, index: torch.Tensor, dim: int = -1, out=None, dim_size=None,
                plan: Optional[GraphPlan] = None, validate: bool = True):
    """torch_scatter.scatter_min (2.0.9): ``(out, arg)`` with ``out[..., d, ...]`` the minimum of the elements of
    ``src`` whose position along ``dim`` has ``index == d``, and ``arg`` (int64) that position.

    ``index`` is 1-D (one entry per position along ``dim``) and broadcast along every other dimension.
    ``dim_size`` is an int or a 0-d tensor; ``None`` means ``index.max() + 1``.
    dtypes: float32, bfloat16, int32, int64 (values compared exactly in their own type).
    Ties: the first occurrence (smallest position) wins, as in torch_scatter's CPU kernel, independent of the
    plan's chunking (``plan=``, e.g. ``GraphPlan(index, N, chunk=c)``).
    NaN is never selected (strict comparisons): a segment holding only NaN counts as empty.  +-inf are ordinary
    values.  Empty segments: ``out = 0`` and ``arg = src.size(dim)``.
    Differentiable w.r.t. floating-point ``src``: the gradient of ``out[d, f]`` goes to ``src[arg[d, f], f]``
    only; empty segments contribute nothing.  ``out=`` (accumulation into a given tensor) is not supported and
    raises.  HIP device tensors only (no CPU fallback)."""
    if out is not None:
        raise RuntimeError("hierarchicalgnn_amd.scatter_min: `out=` is not supported")
    return _scatter_ex(src, index, dim, dim_size, plan, validate, _lib.RED_MIN, "scatter_min")


def scatter_max(src: torch.Tensor, index: torch.Tensor, dim: int = -1, out=None, dim_size=None,
                plan: Optional[GraphPlan] = None, validate: bool = True):
    """torch_scatter.scatter_max (2.0.9): as :func:`scatter_min` with the maximum (same tie, NaN, +-inf,
    empty-segment, gradient and ``out=`` rules)."""
    if out is not None:
        raise RuntimeError("hierarchicalgnn_amd.scatter_max: `out=` is not supported")
    return _scatter_ex(src, index, dim, dim_size, plan, validate, _lib.RED_MAX, "scatter_max")


def scatter_mean(src: torch.Tensor, index: torch.Tensor, dim: int = 0, out=None, dim_size=None,
                 plan: Optional[GraphPlan] = None, validate: bool = True) -> torch.Tensor:
    """torch_scatter.scatter_mean: the sum over the count (empty segments count 1); integer src is floored,
    as torch_scatter does.  Floating-point src: scatter_add of src and of a column of ones."""
    if out is not None:
        raise RuntimeError("hierarchicalgnn_amd.scatter_mean: `out=` is not supported")
    d = _norm_dim(dim, src.dim(), "scatter_mean")
    if dim_size is None:
        dim_size = int(index.max().item()) + 1 if index.numel() else 0
    dim_size = int(dim_size)
    if d != 0:
        return scatter_mean(src.movedim(d, 0), index, 0, None, dim_size, plan, validate).movedim(0, d)
    total = scatter_add(src, index, dim=0, dim_size=dim_size, plan=plan, validate=validate)
    view = (-1,) + (1,) * (src.dim() - 1)
    if src.dtype in _INT_DTYPES:
        ones = torch.ones(src.shape[0], dtype=src.dtype, device=src.device)
        count = scatter_add(ones, index, dim=0, dim_size=dim_size, plan=plan, validate=validate).clamp_(min=1)
        return total.div(count.view(view), rounding_mode="floor")
    ones = torch.ones(src.shape[0], 1, dtype=src.dtype, device=src.device)
    count = scatter_add(ones, index, dim=0, dim_size=dim_size).clamp_(min=1)
    return total / count.view(view)


_REDUCE_OPS = ("sum", "add", "mean", "min", "max")


def scatter(src: torch.Tensor, index: torch.Tensor, dim: int = -1, out=None, dim_size=None,
            reduce: str = "sum") -> torch.Tensor:
    """torch_scatter.scatter: ``reduce`` in sum / add / mean / min / max; min and max return the values only."""
    if reduce in ("sum", "add"):
        return scatter_add(src, index, dim=dim, dim_size=dim_size, out=out)
    if reduce == "mean":
        return scatter_mean(src, index, dim=dim, out=out, dim_size=dim_size)
    if reduce == "min":
        return scatter_min(src, index, dim=dim, out=out, dim_size=dim_size)[0]
    if reduce == "max":
        return scatter_max(src, index, dim=dim, out=out, dim_size=dim_size)[0]
    raise ValueError(f"hierarchicalgnn_amd.scatter: reduce must be one of {_REDUCE_OPS}, got {reduce!r}")


# --------------------------------------------------------------------------- K2 / K3 / K5
class _GatherScaleScatter(torch.autograd.Function):
    """out[d] = sum_{b: dst[b]=d} w[b] * rs[g[b]] * X[g[b]]"""

    @staticmethod
    def forward(ctx, X, weight, row_scale, plan_fwd: GraphPlan, plan_bwd: GraphPlan):
        X_c = X.contiguous()
        w_c = weight.contiguous().view(-1)
        rs_c = row_scale.contiguous().view(-1) if row_scale is not None else None
        ctx.plan_fwd, ctx.plan_bwd = plan_fwd, plan_bwd
        ctx.w_shape, ctx.w_dtype = weight.shape, weight.dtype
        ctx.rs_shape = row_scale.shape if row_scale is not None else None
        ctx.rs_dtype = row_scale.dtype if row_scale is not None else None
        ctx.save_for_backward(X_c, w_c, rs_c)
        return _seg_reduce(plan_fwd, X_c, w_c, rs_c)

    @staticmethod
    def backward(ctx, grad_out):
        X_c, w_c, rs_c = ctx.saved_tensors
        pf, pb = ctx.plan_fwd, ctx.plan_bwd
        g = grad_out.contiguous()
        grad_X = grad_w = grad_rs = None
        if ctx.needs_input_grad[0] or (rs_c is not None and ctx.needs_input_grad[2]):
            # T[s] = sum_{b: g[b]=s} w[b] * grad_out[dst[b]]   (transposed plan)
            T = _seg_reduce(pb, g, w_c, None)
            if rs_c is not None:
                if ctx.needs_input_grad[2]:
                    grad_rs = (T.float() * X_c.float()).sum(dim=1).view(ctx.rs_shape).to(ctx.rs_dtype)
                if ctx.needs_input_grad[0]:
                    grad_X = (T * rs_c.unsqueeze(1)).to(T.dtype)
            else:
                grad_X = T
        if ctx.needs_input_grad[1]:
            # dw[b] = rs[g[b]] * <grad_out[dst[b]], X[g[b]]>
            d = _edge_dot(g, pf.dst32, X_c, pb.dst32, pf.M)
            if rs_c is not None:
                d = d * rs_c[pb.dst32.long()[:pf.M]] if pf.M else d
            grad_w = d.view(ctx.w_shape).to(ctx.w_dtype)
        return grad_X, grad_w, grad_rs, None, None


def gather_scale_scatter(X: torch.Tensor, gather_index: torch.Tensor, dst_index: torch.Tensor, dim_size: int,
                         weight: torch.Tensor, row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused ``scatter_add(weight * (row_scale[:,None] * X)[gather_index], dst_index, dim=0, dim_size)``.

    K2: Modules/gnn_utils.py:124  (X=supernodes, gather=bipartite_graph[1], dst=bipartite_graph[0])
    K3: Modules/gnn_utils.py:142  (X=nodes,      gather=bipartite_graph[0], dst=bipartite_graph[1])
    K5: BipartiteClassification/Models/HGNN_GMM.py:269 (K3 with row_scale = 1/||nodes||_1)
    The [B, L] product is never written to HBM.  Differentiable w.r.t. X, weight, row_scale.
    """
    _require_hip(X, "X", allow_bf16=True)
    _require_hip(weight, "weight", allow_bf16=True)
    if X.dim() != 2:
        raise RuntimeError("gather_scale_scatter: X must be [rows, features]")
    if weight.numel() != gather_index.numel():
        raise RuntimeError("gather_scale_scatter: weight must have one entry per (gather, dst) pair")
    n_src = int(X.shape[0])
    plan_fwd = get_plan(dst_index, int(dim_size), gather_index, n_src)
    plan_bwd = get_plan(gather_index, n_src, dst_index, int(dim_size))
    if row_scale is not None:
        _require_hip(row_scale, "row_scale", allow_bf16=True)
        if row_scale.numel() != n_src:
            raise RuntimeError("gather_scale_scatter: row_scale must have one entry per row of X")
    return _GatherScaleScatter.apply(X, weight, row_scale, plan_fwd, plan_bwd)


# --------------------------------------------------------------------------- K6
class _GatherRows(torch.autograd.Function):
    """out[e] = table[index[e]]; backward = segmented reduce over the CSR by `index`"""

    @staticmethod
    def forward(ctx, table, plan: GraphPlan):
        ctx.plan = plan
        return _spread_rows(plan, table.contiguous())

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None
        return _seg_reduce(ctx.plan, grad_out.contiguous(), None, None), None


def gather_rows(table: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """``table[index]`` for a 2-D table and a 1-D int64 index (Modules/gnn_utils.py:61,134,152).
    Forward is a whole-row HIP gather; backward is the atomics-free segmented reduce."""
    _require_hip(table, "table", allow_bf16=True)
    if table.dim() != 2 or index.dim() != 1:
        raise RuntimeError("gather_rows: table must be 2-D and index 1-D")
    plan = get_plan(index, int(table.shape[0]))
    return _GatherRows.apply(table, plan)


def l1_row_scale(x: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """1 / max(||x_i||_1, eps): the per-row factor of F.normalize(x, p=1) (HGNN_GMM.py:269)"""
    return 1.0 / x.abs().sum(dim=1).clamp_min(eps)


# --------------------------------------------------------------------------- K11 per-edge dot products
class _EdgeDot(torch.autograd.Function):
    """out[e] = <A[ai[e]], B[bi[e]]>  (torch.einsum('ij,ij->i', A[ai], B[bi]), gnn_utils.py:208)"""

    @staticmethod
    def forward(ctx, A, B, ai, bi):
        from .plan import get_index32
        A_c, B_c = A.contiguous(), B.contiguous()
        ctx.save_for_backward(A_c, B_c)
        ctx.idx = (ai, bi)
        return _edge_dot(A_c, get_index32(ai, A_c.shape[0]), B_c, get_index32(bi, B_c.shape[0]), int(ai.numel()))

    @staticmethod
    def backward(ctx, g):
        A_c, B_c = ctx.saved_tensors
        ai, bi = ctx.idx
        g_c = g.contiguous()
        grad_A = grad_B = None
        if ctx.needs_input_grad[0]:   # dA[a] = sum_{e: ai[e]=a} g[e] * B[bi[e]]
            grad_A = _seg_reduce(get_plan(ai, int(A_c.shape[0]), bi, int(B_c.shape[0])), B_c, g_c, None)
        if ctx.needs_input_grad[1]:
            grad_B = _seg_reduce(get_plan(bi, int(B_c.shape[0]), ai, int(A_c.shape[0])), A_c, g_c, None)
        return grad_A, grad_B, None, None


def edge_dot(A: torch.Tensor, ai: torch.Tensor, B: torch.Tensor, bi: torch.Tensor) -> torch.Tensor:
    """per-edge dot product of two gathered rows without materialising the gathers; differentiable"""
    _require_hip(A, "A")
    _require_hip(B, "B")
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[1] or ai.shape != bi.shape or ai.dim() != 1:
        raise RuntimeError("edge_dot: A[*,F], B[*,F] and 1-D index tensors of equal length expected")
    return _EdgeDot.apply(A, B, ai, bi)


KNN_METHODS = ("brute", "sorted")
_knn_sorted_stats = None   # device int64[2] of the last method="sorted" call


def knn_radius(query: torch.Tensor, points: torch.Tensor, k: int, radius, return_dist2: bool = False,
               method: str = "brute"):
    """<=k nearest `points` of every `query` row with squared distance < radius^2, ascending,
    -1 padded: the idxs of frnn.frnn_grid_points (Modules/utils.py:232) for one batch.
    ``radius``: a float, or a 1-element float32 device tensor (the module's ``knn_radius`` buffer) that the
    kernel reads itself -- no host read of it.
    ``method``: "brute" compares every query with every point (k in 1-6, 8, 10, 12, 16, 20, 32 or 33..128);
    "sorted" sorts the points along a Morton curve and skips tiles that are provably too far (csrc/knn_sorted.hip):
    the same result bit for bit, for every k in 1..128."""
    if method not in KNN_METHODS:
        raise ValueError(f"knn_radius: method must be one of {KNN_METHODS}, got {method!r}")
    _require_hip(query, "query")
    _require_hip(points, "points")
    if query.dim() != 2 or points.dim() != 2 or query.shape[1] != points.shape[1]:
        raise RuntimeError("knn_radius: query[N,D] and points[S,D] expected")
    q, p = query.detach().contiguous(), points.detach().contiguous()
    nq, D = int(q.shape[0]), int(q.shape[1])
    r_dev, r_val = None, 0.0
    if torch.is_tensor(radius):
        if radius.numel() != 1 or radius.device != q.device:
            raise RuntimeError("knn_radius: a tensor radius must have one element on the queries' device")
        r_dev = radius.detach().reshape(1).float().contiguous()
    else:
        r_val = float(radius)
    idx = torch.empty((nq, int(k)), dtype=torch.int64, device=q.device)
    d2 = torch.empty((nq, int(k)), dtype=torch.float32, device=q.device) if return_dist2 else None
    lib = _lib.load()
    nbytes = ctypes.c_size_t(0)
    if method == "sorted":
        global _knn_sorted_stats
        _lib.check(lib.hgnn_knn_sorted_workspace_bytes(nq, int(p.shape[0]), D, int(k), ctypes.byref(nbytes)),
                   "hgnn_knn_sorted_workspace_bytes")
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=q.device)
        stats = (torch.empty if nq else torch.zeros)(2, dtype=torch.int64, device=q.device)   # nq == 0: not written
        with torch.cuda.device(q.device):
            _lib.check(lib.hgnn_knn_radius_sorted_f32(_lib.ptr(q), nq, _lib.ptr(p), int(p.shape[0]), D, int(k),
                                                      ctypes.c_float(r_val), _lib.ptr(r_dev), _lib.ptr(idx),
                                                      _lib.ptr(d2), _lib.ptr(ws), nbytes.value, _lib.ptr(stats),
                                                      _lib.current_stream(q.device)),
                       "hgnn_knn_radius_sorted_f32")
        _knn_sorted_stats = stats
        return (idx, d2) if return_dist2 else idx
    _lib.check(lib.hgnn_knn_workspace_bytes(nq, int(p.shape[0]), int(k), ctypes.byref(nbytes)),
               "hgnn_knn_workspace_bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=q.device) if nbytes.value else None
    with torch.cuda.device(q.device):
        _lib.check(lib.hgnn_knn_radius_ws_f32(_lib.ptr(q), nq, _lib.ptr(p), int(p.shape[0]), D, int(k),
                                              ctypes.c_float(r_val), _lib.ptr(r_dev), _lib.ptr(idx), _lib.ptr(d2),
                                              _lib.ptr(ws), nbytes.value, _lib.current_stream(q.device)),
                   "hgnn_knn_radius_ws_f32")
    return (idx, d2) if return_dist2 else idx


def knn_radius_stats():
    """(tiles visited, tiles skipped), summed over the workgroups, of the last ``knn_radius(..., method="sorted")``
    call.  One host read: for tests and tools, not for a training step."""
    if _knn_sorted_stats is None:
        raise RuntimeError("knn_radius_stats: no knn_radius(..., method=\"sorted\") call yet")
    v, s = _knn_sorted_stats.tolist()
    return int(v), int(s)


gc_stats = {"host_reads": 0}   # graph_construction.stats: the host reads of the device-side graph route


def knn_edges(idx: torch.Tensor, n_pts: int, sym: bool = False) -> torch.Tensor:
    """The edge list of a kNN result ``idx`` int64 [nq, K] (``knn_radius``'s: ids in [0, n_pts), -1 = empty slot) as
    ``DynamicGraphConstruction.build_graph`` forms it: the pairs (row, id) of the valid slots in row-major order, or
    with ``sym`` the union of both directions without duplicates in ascending (src, dst) order (``symmetrize`` with
    n = max(nq, n_pts)).  Built on the device (csrc/graphcon.hip) with ONE host read -- the edge count and the status
    word together, counted in ``graph_construction.stats["host_reads"]``.  Returns a contiguous int64 [2, B] tensor.
    ValueError if an id is >= n_pts or < -1."""
    if not torch.is_tensor(idx) or idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[1] < 1:
        raise ValueError("knn_edges: idx must be an int64 [nq, K >= 1] tensor")
    nq, K, n_pts = int(idx.shape[0]), int(idx.shape[1]), int(n_pts)
    if n_pts < 0 or max(nq, n_pts) > 2 ** 31:
        raise ValueError(f"knn_edges: n = max(nq, n_pts) = {max(nq, n_pts)} must be in [0, 2^31]")
    if nq * K >= 2 ** 30:
        raise ValueError(f"knn_edges: nq * K = {nq * K} must stay below 2^30")
    if not idx.is_cuda:
        raise RuntimeError("knn_edges needs a HIP device tensor: hierarchicalgnn_amd has no CPU path")
    dev = idx.device
    cap = (2 if sym else 1) * nq * K
    if cap == 0:
        return torch.empty((2, 0), dtype=torch.int64, device=dev)
    idx_c = idx.detach().contiguous()
    lib = _lib.load()
    ws, nbytes = _lib.workspace("hgnn_knn_edges_workspace_bytes", dev, nq, K, n_pts, int(bool(sym)))
    edges = torch.empty((2, cap), dtype=torch.int64, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.hgnn_knn_edges(_lib.ptr(idx_c), nq, K, n_pts, int(bool(sym)), _lib.ptr(edges), cap,
                                      _lib.ptr(info), _lib.ptr(ws), nbytes, _lib.current_stream(dev)),
                   "hgnn_knn_edges")
    gc_stats["host_reads"] += 1
    count, status = info.tolist()
    if status & _lib.GC_ST_BAD_ID:
        raise ValueError(f"knn_edges: a neighbour id is >= n_pts = {n_pts} or < -1")
    return edges[:, :count].contiguous()


def _wgrad_operand(t: torch.Tensor) -> torch.Tensor:
    """an operand of the weight-gradient kernels as they can read it: 16-byte pieces of row-major rows.  A view with a
    column stride, with a row stride that is no multiple of 16 bytes, or whose first element is not 16-byte aligned (a
    column slice at such an offset) is copied; every other column slice is read in place."""
    per16 = 16 // t.element_size()
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) % per16):
        t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def wgrad_bf16(dz: torch.Tensor, rows: torch.Tensor, out: Optional[torch.Tensor] = None,
               colsum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dz^T @ rows`` for bf16 ``dz[M, Ho]`` and ``rows[M, Hi]`` (row-major, possibly column slices of wider
    matrices) in fp32: the weight gradient of a Linear layer, by the hand-written split-K bf16-MFMA kernel
    (``hgnn_wgrad_bf16``; deterministic).  ``out`` (fp32 [Ho, Hi], possibly a column slice) is written in place;
    ``colsum`` (fp32 [Ho], optional) receives ``dz.sum(0)`` -- the Linear's bias gradient -- from the same pass."""
    _require_hip(dz, "dz", allow_bf16=True)
    _require_hip(rows, "rows", allow_bf16=True)
    if dz.dtype != torch.bfloat16 or rows.dtype != torch.bfloat16 or dz.dim() != 2 or rows.dim() != 2 \
            or dz.shape[0] != rows.shape[0]:
        raise RuntimeError("wgrad_bf16: bf16 dz[M, Ho] and rows[M, Hi] expected")
    dz, rows = _wgrad_operand(dz), _wgrad_operand(rows)
    M, Ho, Hi = int(dz.shape[0]), int(dz.shape[1]), int(rows.shape[1])
    if out is None:
        out = torch.empty((Ho, Hi), dtype=torch.float32, device=dz.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (Ho, Hi) or out.stride(1) != 1:
        raise RuntimeError("wgrad_bf16: out must be fp32 [Ho, Hi] with unit column stride")
    lib = _lib.load()
    nbytes = ctypes.c_size_t(0)
    _lib.check(lib.hgnn_wgrad_workspace_bytes(M, Ho, Hi, ctypes.byref(nbytes)), "hgnn_wgrad_workspace_bytes")
    ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=dz.device)
    lda = int(dz.stride(0)) if M > 1 else Ho
    ldb = int(rows.stride(0)) if M > 1 else Hi
    with torch.cuda.device(dz.device):
        if colsum is not None and (colsum.dtype != torch.float32 or colsum.numel() != Ho or not colsum.is_contiguous()):
            raise RuntimeError("wgrad_bf16: colsum must be a contiguous fp32 [Ho] tensor")
        _lib.check(lib.hgnn_wgrad_bf16(_lib.ptr(dz), lda, _lib.ptr(rows), ldb, M, Ho, Hi,
                                       ctypes.c_void_p(out.data_ptr()), int(out.stride(0)),
                                       ctypes.c_void_p(colsum.data_ptr()) if colsum is not None else None,
                                       _lib.ptr(ws), ws.numel(), _lib.current_stream(dz.device)), "hgnn_wgrad_bf16")
    return out


def wgrad_f32_split3(dz: torch.Tensor, rows: torch.Tensor, out: Optional[torch.Tensor] = None,
                     colsum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dz^T @ rows`` for FP32 ``dz[M, Ho]`` and ``rows[M, Hi]`` with the products evaluated as split-bf16
    (``hgnn_wgrad_f32_split3``: hi.hi + mid.hi + hi.mid on the bf16 matrix pipe, fp32 accumulation, deterministic):
    the M-row weight gradients of the fp32 training backward.  Same conventions as :func:`wgrad_bf16`."""
    _require_hip(dz, "dz")
    _require_hip(rows, "rows")
    if dz.dtype != torch.float32 or rows.dtype != torch.float32 or dz.dim() != 2 or rows.dim() != 2 \
            or dz.shape[0] != rows.shape[0]:
        raise RuntimeError("wgrad_f32_split3: fp32 dz[M, Ho] and rows[M, Hi] expected")
    dz, rows = _wgrad_operand(dz), _wgrad_operand(rows)
    M, Ho, Hi = int(dz.shape[0]), int(dz.shape[1]), int(rows.shape[1])
    if out is None:
        out = torch.empty((Ho, Hi), dtype=torch.float32, device=dz.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (Ho, Hi) or out.stride(1) != 1:
        raise RuntimeError("wgrad_f32_split3: out must be fp32 [Ho, Hi] with unit column stride")
    lib = _lib.load()
    nbytes = ctypes.c_size_t(0)
    _lib.check(lib.hgnn_wgrad_workspace_bytes(M, Ho, Hi, ctypes.byref(nbytes)), "hgnn_wgrad_workspace_bytes")
    ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=dz.device)
    lda = int(dz.stride(0)) if M > 1 else Ho
    ldb = int(rows.stride(0)) if M > 1 else Hi
    with torch.cuda.device(dz.device):
        if colsum is not None and (colsum.dtype != torch.float32 or colsum.numel() != Ho or not colsum.is_contiguous()):
            raise RuntimeError("wgrad_f32_split3: colsum must be a contiguous fp32 [Ho] tensor")
        _lib.check(lib.hgnn_wgrad_f32_split3(_lib.ptr(dz), lda, _lib.ptr(rows), ldb, M, Ho, Hi,
                                             ctypes.c_void_p(out.data_ptr()), int(out.stride(0)),
                                             ctypes.c_void_p(colsum.data_ptr()) if colsum is not None else None,
                                             _lib.ptr(ws), ws.numel(), _lib.current_stream(dz.device)),
                   "hgnn_wgrad_f32_split3")
    return out


def wgrad_f32(dz: torch.Tensor, rows: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dz^T @ rows`` for FP32 ``dz[M, Ho]`` and ``rows[M, Hi]`` in EXACT fp32 (``hgnn_wgrad_f32``: every product
    formed once from the fp32 operands on the fp32 MFMA, split-K in a fixed order, no atomics -- the same bits on every
    device and in every run): the weight gradients of the default fp32 training backward.  Widths: multiples of 8 up
    to 1024.  Same conventions as :func:`wgrad_f32_split3`, without ``colsum``."""
    _require_hip(dz, "dz")
    _require_hip(rows, "rows")
    if dz.dtype != torch.float32 or rows.dtype != torch.float32 or dz.dim() != 2 or rows.dim() != 2 \
            or dz.shape[0] != rows.shape[0]:
        raise RuntimeError("wgrad_f32: fp32 dz[M, Ho] and rows[M, Hi] expected")
    dz, rows = _wgrad_operand(dz), _wgrad_operand(rows)
    M, Ho, Hi = int(dz.shape[0]), int(dz.shape[1]), int(rows.shape[1])
    if out is None:
        out = torch.empty((Ho, Hi), dtype=torch.float32, device=dz.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (Ho, Hi) or out.stride(1) != 1:
        raise RuntimeError("wgrad_f32: out must be fp32 [Ho, Hi] with unit column stride")
    lib = _lib.load()
    nbytes = ctypes.c_size_t(0)
    _lib.check(lib.hgnn_wgrad_f32_workspace_bytes(M, Ho, Hi, ctypes.byref(nbytes)), "hgnn_wgrad_f32_workspace_bytes")
    ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=dz.device)
    lda = int(dz.stride(0)) if M > 1 else Ho
    ldb = int(rows.stride(0)) if M > 1 else Hi
    with torch.cuda.device(dz.device):
        _lib.check(lib.hgnn_wgrad_f32(_lib.ptr(dz), lda, _lib.ptr(rows), ldb, M, Ho, Hi,
                                      ctypes.c_void_p(out.data_ptr()), int(out.stride(0)),
                                      _lib.ptr(ws), ws.numel(), _lib.current_stream(dz.device)), "hgnn_wgrad_f32")
    return out


# ------------------------------------------------------------------ the exact route's projection and narrow products
def _narrow_operand(t: torch.Tensor) -> torch.Tensor:
    """a narrow-side operand ([M, n] rows, [n, K] weights) as the narrow kernels can read it: unit column stride and a
    row stride that covers the width (4-byte alignment is all they need, so tab[N, 3] is read in place)"""
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def _ld(t: torch.Tensor) -> int:
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def project_f32(x: torch.Tensor, w0: torch.Tensor, w1: Optional[torch.Tensor] = None, width: Optional[int] = None):
    """``x @ w0.T`` (and ``x @ w1.T``) for FP32 ``x[M, K]`` and ``w_b[N, K]`` in EXACT fp32 (``hgnn_project_f32``: every
    product formed once on the fp32 MFMA, each output element a fmaf chain over k ascending, no split-K): the forward
    pre-projection of the exact route, both segments of an edge update from one launch.  ``w0`` / ``w1`` may be column
    blocks of one first Linear, read in place; views the kernel cannot read are copied (:func:`_wgrad_operand`).
    ``width`` > N returns zero-filled ``[M, width]`` tensors with the product in the first N columns (the padded
    route).  Returns a tuple with one tensor per weight block."""
    _require_hip(x, "x")
    ws = [w0] if w1 is None else [w0, w1]
    for w in ws:
        _require_hip(w, "w")
    if x.dim() != 2 or any(w.dim() != 2 or w.shape[1] != x.shape[1] or w.shape != w0.shape for w in ws):
        raise RuntimeError("project_f32: fp32 x[M, K] and w[N, K] blocks of one shape expected")
    x = _wgrad_operand(x)
    ws = [_wgrad_operand(w) for w in ws]
    M, K, N = int(x.shape[0]), int(x.shape[1]), int(w0.shape[0])
    if len(ws) == 2 and N > 1 and ws[0].stride(0) != ws[1].stride(0):
        ws = [w.contiguous() for w in ws]
        ws = [w if w.data_ptr() % 16 == 0 else w.clone() for w in ws]
    cols = N if width is None else int(width)
    if cols < N:
        raise RuntimeError("project_f32: width must be at least N")
    make = torch.empty if cols == N else torch.zeros
    outs = [make((M, cols), dtype=torch.float32, device=x.device) for _ in ws]
    if M == 0:   # nothing to launch (and an empty tensor has no address to hand over)
        return tuple(outs)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().hgnn_project_f32(
            _lib.ptr(x), _ld(x), M, K, _lib.ptr(ws[0]), _lib.ptr(ws[1]) if len(ws) > 1 else None, _ld(ws[0]), N,
            _lib.ptr(outs[0]), _lib.ptr(outs[1]) if len(outs) > 1 else None, cols,
            _lib.current_stream(x.device)), "hgnn_project_f32")
    return tuple(outs)


def linear_narrow_f32(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x @ W.T + bias`` for FP32 ``x[M, K]`` and a NARROW ``W[n, K]``, n <= 32 (``hgnn_linear_narrow_f32``: fixed
    order, a function of K alone; the bias joins last): a head's last Linear, the encoders' input gradient."""
    _require_hip(x, "x")
    _require_hip(W, "W")
    if x.dim() != 2 or W.dim() != 2 or W.shape[1] != x.shape[1]:
        raise RuntimeError("linear_narrow_f32: fp32 x[M, K] and W[n, K] expected")
    x, W = _wgrad_operand(x), _narrow_operand(W)
    M, K, n = int(x.shape[0]), int(x.shape[1]), int(W.shape[0])
    if bias is not None:
        _require_hip(bias, "bias")
        if bias.numel() != n or not bias.is_contiguous():
            raise RuntimeError("linear_narrow_f32: bias must be a contiguous fp32 [n] tensor")
    out = torch.empty((M, n), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().hgnn_linear_narrow_f32(
            _lib.ptr(x), _ld(x), M, K, _lib.ptr(W), _ld(W), _lib.ptr(bias) if bias is not None else None, n,
            _lib.ptr(out), n, _lib.current_stream(x.device)), "hgnn_linear_narrow_f32")
    return out


def outer_narrow_f32(y: torch.Tensor, W: torch.Tensor, add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``y @ W (+ add)`` for a NARROW FP32 ``y[M, n]``, n <= 32, and ``W[n, K]`` (``hgnn_outer_narrow_f32``: a fmaf
    chain over j ascending, ``add`` joins last): a head's data gradient ``dy @ W``."""
    _require_hip(y, "y")
    _require_hip(W, "W")
    if y.dim() != 2 or W.dim() != 2 or W.shape[0] != y.shape[1]:
        raise RuntimeError("outer_narrow_f32: fp32 y[M, n] and W[n, K] expected")
    y, W = _narrow_operand(y), _narrow_operand(W)
    M, n, K = int(y.shape[0]), int(y.shape[1]), int(W.shape[1])
    if add is not None:
        _require_hip(add, "add")
        if tuple(add.shape) != (M, K):
            raise RuntimeError("outer_narrow_f32: add must be fp32 [M, K]")
        add = add.contiguous()   # it shares out's row stride
    out = torch.empty((M, K), dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        _lib.check(_lib.load().hgnn_outer_narrow_f32(
            _lib.ptr(y), _ld(y), M, n, _lib.ptr(W), _ld(W), K, _lib.ptr(add) if add is not None else None,
            _lib.ptr(out), K, _lib.current_stream(y.device)), "hgnn_outer_narrow_f32")
    return out


def wgrad_narrow_f32(y: torch.Tensor, x: torch.Tensor, colsum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``y^T @ x`` for a NARROW FP32 ``y[M, n]``, n <= 32, and ``x[M, K]`` (``hgnn_wgrad_narrow_f32``: split over the
    rows in a fixed order, no atomics); ``colsum`` (fp32 [n]) receives the column sums of ``y``.  A head's weight and
    bias gradient (``y = dy``, ``x = hidden``), the encoders' ``dW[:, cols]^T`` (``y = tab[N, 3]``, read in place)."""
    _require_hip(y, "y")
    _require_hip(x, "x")
    if y.dim() != 2 or x.dim() != 2 or y.shape[0] != x.shape[0]:
        raise RuntimeError("wgrad_narrow_f32: fp32 y[M, n] and x[M, K] expected")
    y, x = _narrow_operand(y), _wgrad_operand(x)
    M, n, K = int(y.shape[0]), int(y.shape[1]), int(x.shape[1])
    if colsum is not None:
        _require_hip(colsum, "colsum")
        if colsum.numel() != n or not colsum.is_contiguous():
            raise RuntimeError("wgrad_narrow_f32: colsum must be a contiguous fp32 [n] tensor")
    lib = _lib.load()
    nbytes = ctypes.c_size_t(0)
    _lib.check(lib.hgnn_wgrad_narrow_f32_workspace_bytes(M, n, K, ctypes.byref(nbytes)),
               "hgnn_wgrad_narrow_f32_workspace_bytes")
    ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=y.device)
    out = torch.empty((n, K), dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        _lib.check(lib.hgnn_wgrad_narrow_f32(
            _lib.ptr(y), _ld(y), n, _lib.ptr(x), _ld(x), K, M, _lib.ptr(out), K,
            _lib.ptr(colsum) if colsum is not None else None, _lib.ptr(ws), ws.numel(),
            _lib.current_stream(y.device)), "hgnn_wgrad_narrow_f32")
    return out
