"""Drop-in ``DynamicGraphConstruction`` (reference Modules/gnn_utils.py:171-218) and
``find_neighbors`` (Modules/utils.py:228-239): the per-forward kNN graph rebuild and the
attention weights of the hierarchical model.

Same constructor (``weighting_function`` name, ``hparams``), buffers (``knn_radius``) and
sub-module (``weight_normalization`` = ``BatchNorm1d(1)``), hence the same ``state_dict``
keys.  The neighbour search runs in the exact brute-force HIP kernel
(``hgnn_knn_radius_f32``; with ``hparams["knn_method"] = "sorted"`` in the spatially sorted
``hgnn_knn_radius_sorted_f32``, same result) instead of the un-vendored ``frnn`` grid search; the per-edge
dot products use ``hgnn_edge_dot_f32`` (no gathered copies), differentiable w.r.t. both
embeddings.  ``symmetrize`` restates cugraph's (union of both directions, duplicates
removed); cugraph does not document an edge order, ours is sorted by (src, dst).

``hparams["graph_construction"] = "fused"`` (default ``"torch"``: the route above) builds the edge list on the device
(``ops.knn_edges``: one host read, the edge count) and computes the weights with ``attention_weights``: dot product,
BatchNorm1d(1) with its running-statistics update, weighting function and mean normalisation as one operator with a
hand-written backward (csrc/graphcon.hip), no host read.  ``stats["host_reads"]`` counts that route's reads.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .ops import _f32, _seg_reduce, edge_dot, gc_stats as stats, knn_edges, knn_radius
from .plan import get_plan

GRAPH_CONSTRUCTION_ROUTES = ("torch", "fused")
_GA_FN = {"sigmoid": _lib.GA_FN_SIGMOID, "exp": _lib.GA_FN_EXP}


def find_neighbors(embedding1, embedding2, r_max=1.0, k_max=10, return_dist2=False, method=None):
    # method: ops.knn_radius's; None = "brute" (k_max in 1-6, 8, 10, 12, 16, 20, 32 or 33..128); "sorted": every k_max
    # a tensor radius (the knn_radius buffer) is read by the kernel itself: no .item() host read
    r = r_max if torch.is_tensor(r_max) and r_max.is_cuda else (float(r_max.item()) if torch.is_tensor(r_max)
                                                                 else float(r_max))
    return knn_radius(embedding1, embedding2, k_max, r, return_dist2=return_dist2,
                      method="brute" if method is None else method)


def symmetrize(src: torch.Tensor, dst: torch.Tensor, n: int):
    key = torch.cat([src * n + dst, dst * n + src])
    key = torch.unique(key)            # sorted
    return torch.div(key, n, rounding_mode="floor"), key % n


def batch_norm_1(bn: nn.BatchNorm1d, x: torch.Tensor, stat_reduce=None) -> torch.Tensor:
    """``bn(x.unsqueeze(1)).squeeze()`` for the one-channel BatchNorm of gnn_utils.py:179,209.  With ``stat_reduce``
    (a differentiable sum over the shards of ONE event, partition.allreduce_supernode_sums) and the module in
    training mode the batch statistics are those of the WHOLE event: every rank contributes (sum, sum of squares,
    count) of its own edges -- a synchronised BatchNorm; running statistics are updated exactly as nn.BatchNorm1d
    does (momentum, unbiased variance).  Gradients flow through the reduced statistics: the backward of the sum over
    ranks is again a sum over ranks, which is what makes d loss / d x_i see the other shards' loss terms."""
    if stat_reduce is None or not bn.training:
        return bn(x.unsqueeze(1)).squeeze(1)
    xd = x.double()
    stats = stat_reduce(torch.stack([xd.sum(), (xd * xd).sum(), xd.new_tensor(float(x.numel()))]))
    n = stats[2]
    mean = stats[0] / n
    var = (stats[1] / n - mean * mean).clamp(min=0)                 # biased, as the normalisation uses
    with torch.no_grad():
        if bn.track_running_stats and bn.running_mean is not None:
            bn.num_batches_tracked += 1
            m = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
            bn.running_mean.mul_(1 - m).add_(m * mean.to(bn.running_mean.dtype))
            bn.running_var.mul_(1 - m).add_(m * (var * n / (n - 1).clamp(min=1)).to(bn.running_var.dtype))
    y = ((xd - mean) * torch.rsqrt(var + bn.eps)).to(x.dtype)
    if bn.affine:
        y = y * bn.weight[0] + bn.bias[0]
    return y


class _GraphAttention(torch.autograd.Function):
    """(weights, logits, x, state) of hgnn_graph_attention_forward; backward: hgnn_graph_attention_backward for
    d/dx, d/dgamma, d/dbeta, then the weighted segmented reduce of ``_EdgeDot.backward`` for dA and dB"""

    @staticmethod
    def forward(ctx, A, B, gamma, beta, graph, bn, fn, flags):
        lib = _lib.load()
        dev = A.device
        e = int(graph.shape[1])
        idt = _lib.index_dtype(graph)
        A_c, B_c = _f32(A).contiguous(), _f32(B).contiguous()      # bf16 rows are widened once, as in _edge_dot
        x = torch.empty(e, dtype=torch.float32, device=dev)
        logits, weights = torch.empty_like(x), torch.empty_like(x)
        state = torch.empty(_lib.GA_STATE, dtype=torch.float64, device=dev)
        ws, nb = _lib.workspace("hgnn_graph_attention_workspace_bytes", dev, e, 0)
        momentum = -1.0 if bn.momentum is None else float(bn.momentum)
        with torch.cuda.device(dev):
            _lib.check(lib.hgnn_graph_attention_forward(
                _lib.ptr(A_c), int(A_c.shape[0]), _lib.ptr(B_c), int(B_c.shape[0]), int(A_c.shape[1]),
                _lib.ptr(graph), idt, e, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(bn.running_mean),
                _lib.ptr(bn.running_var), _lib.ptr(bn.num_batches_tracked), float(bn.eps), momentum, flags, fn,
                _lib.ptr(x), _lib.ptr(logits), _lib.ptr(weights), _lib.ptr(state), _lib.ptr(ws), nb,
                _lib.current_stream(dev)), "hgnn_graph_attention_forward")
        # the plans of the backward take int64 ids: an int32 graph is widened once, here
        graph64 = graph if graph.dtype == torch.int64 else graph.long()
        ctx.save_for_backward(A_c, B_c, gamma, beta, graph64, x, state)
        ctx.fn, ctx.flags = fn, flags
        ctx.in_dtypes = (A.dtype, B.dtype)
        ctx.mark_non_differentiable(x, state)
        ctx.set_materialize_grads(False)
        return weights, logits, x, state

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_w, g_logits, _gx, _gstate):
        A_c, B_c, gamma, beta, graph, x, state = ctx.saved_tensors
        lib = _lib.load()
        dev = x.device
        e = int(x.numel())
        if e == 0 or (g_w is None and g_logits is None):
            return None, None, None, None, None, None, None, None
        g_w = torch.zeros_like(x) if g_w is None else g_w.to(torch.float32).contiguous()
        g_l = None if g_logits is None else g_logits.to(torch.float32).contiguous()
        g_x = torch.empty_like(x)
        g_bn = torch.empty(2, dtype=torch.float32, device=dev)
        ws, nb = _lib.workspace("hgnn_graph_attention_workspace_bytes", dev, e, 1)
        with torch.cuda.device(dev):
            _lib.check(lib.hgnn_graph_attention_backward(
                _lib.ptr(x), e, _lib.ptr(gamma), _lib.ptr(beta), ctx.flags, ctx.fn, _lib.ptr(state), _lib.ptr(g_w),
                _lib.ptr(g_l), _lib.ptr(g_x), _lib.ptr(g_bn), _lib.ptr(ws), nb, _lib.current_stream(dev)),
                "hgnn_graph_attention_backward")
        ai, bi = graph[0], graph[1]
        na, nb_rows = int(A_c.shape[0]), int(B_c.shape[0])
        grad_A = grad_B = None
        if ctx.needs_input_grad[0]:   # dA[a] = sum_{e: a_e = a} g_x[e] * B[b_e]
            grad_A = _seg_reduce(get_plan(ai, na, bi, nb_rows), B_c, g_x, None).to(ctx.in_dtypes[0])
        if ctx.needs_input_grad[1]:
            grad_B = _seg_reduce(get_plan(bi, nb_rows, ai, na), A_c, g_x, None).to(ctx.in_dtypes[1])
        grad_gamma = g_bn[0:1] if ctx.needs_input_grad[2] else None
        grad_beta = g_bn[1:2] if ctx.needs_input_grad[3] else None
        return grad_A, grad_B, grad_gamma, grad_beta, None, None, None, None


def _weighting_name(weighting):
    name = weighting if isinstance(weighting, str) else {torch.sigmoid: "sigmoid", torch.exp: "exp"}.get(weighting)
    if name not in _GA_FN:
        raise ValueError(f"attention_weights: the weighting function must be 'sigmoid' or 'exp', got {weighting!r}")
    return name


def attention_weights(src, dst, graph, bn, weighting, norm=False, logits=False):
    """``DynamicGraphConstruction.edge_weights`` as one operator: ``weighting(bn(<src[graph[0]], dst[graph[1]]>))``,
    divided by its mean with ``norm``; returns ``weights [E, 1]`` (and ``logits [E]``).  ``bn`` is the module's
    ``BatchNorm1d(1)``: in training mode the batch statistics are float64 sums in a fixed order and the kernel updates
    ``running_mean``, ``running_var`` and ``num_batches_tracked`` as ``nn.BatchNorm1d`` does; in eval mode the running
    statistics are used.  ``weighting``: "sigmoid" or "exp" (or ``torch.sigmoid`` / ``torch.exp``).  Differentiable
    (once) w.r.t. ``src``, ``dst``, ``bn.weight`` and ``bn.bias``; no host read in either direction.
    Unlike ``edge_dot`` (whose int32 index copy is range-checked with a host read), the forward does not refuse a graph
    id outside its table: such an edge gets x = 0 -- no address is formed from the id -- and takes part in the
    statistics like any other; the backward's plan then raises on it.  ``knn_edges`` graphs hold no such id."""
    fn = _GA_FN[_weighting_name(weighting)]
    if not torch.is_tensor(src) or not torch.is_tensor(dst) or not torch.is_tensor(graph):
        raise ValueError("attention_weights: src, dst and graph must be tensors")
    if src.dim() != 2 or dst.dim() != 2 or src.shape[1] != dst.shape[1] or \
            not 1 <= src.shape[1] <= _lib.GA_MAX_DIM:
        raise ValueError(f"attention_weights: src [Na, D] and dst [Nb, D] with 1 <= D <= {_lib.GA_MAX_DIM} expected, "
                         f"got {tuple(src.shape)} and {tuple(dst.shape)}")
    if any(t.dtype not in (torch.float32, torch.bfloat16) for t in (src, dst)):
        raise ValueError(f"attention_weights: src and dst must be float32 or bfloat16, got {src.dtype}, {dst.dtype}")
    if graph.dim() != 2 or graph.shape[0] != 2 or graph.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"attention_weights: graph must be int64 or int32 [2, E], got {graph.dtype} "
                         f"{tuple(graph.shape)}")
    if not isinstance(bn, nn.BatchNorm1d) or bn.num_features != 1 or not bn.affine or not bn.track_running_stats:
        raise ValueError("attention_weights: bn must be an affine BatchNorm1d(1) that tracks running statistics")
    e = int(graph.shape[1])
    if bn.training and e <= 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size([e, 1])}")
    if not (src.is_cuda and dst.is_cuda and graph.is_cuda and bn.weight.is_cuda):
        raise RuntimeError("attention_weights needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    if any(t.device != src.device for t in (dst, graph, bn.weight)):
        raise ValueError("attention_weights: src, dst, graph and bn must be on one device")
    if e == 0:
        w = src.new_empty((0, 1), dtype=torch.float32)
        return (w, src.new_empty((0,), dtype=torch.float32)) if logits else w
    flags = (_lib.GA_TRAINING if bn.training else 0) | (_lib.GA_NORM if norm else 0)
    w, z, _, _ = _GraphAttention.apply(src, dst, bn.weight, bn.bias, graph.contiguous(), bn, fn, flags)
    w = w.unsqueeze(1)
    return (w, z) if logits else w


class DynamicGraphConstruction(nn.Module):
    def __init__(self, weighting_function, hparams):
        super().__init__()
        self.hparams = hparams
        self.weight_normalization = nn.BatchNorm1d(1)
        self.weighting_function = getattr(torch, weighting_function)
        self.register_buffer("knn_radius", torch.ones(1), persistent=True)
        # optional hparams["knn_method"]: "sorted" takes every k (a sparsity sweep at k = 7 or 9); absent: "brute"
        self.knn_method = hparams["knn_method"] if hparams is not None and "knn_method" in hparams else None
        # optional hparams["graph_construction"]: "fused" builds and weights the graph on the device; absent: "torch"
        route = hparams["graph_construction"] if hparams is not None and "graph_construction" in hparams else "torch"
        if route not in GRAPH_CONSTRUCTION_ROUTES:
            raise ValueError(f"graph_construction must be one of {GRAPH_CONSTRUCTION_ROUTES}, got {route!r}")
        self.fused = route == "fused"
        self._weighting_name = weighting_function

    def build_graph(self, src_embeddings, dst_embeddings, sym=False, k=10, fused=None):
        """gnn_utils.py:193-205 (no gradients): kNN within the tracked radius, optional symmetrisation,
        radius EMA in training mode.  ``fused`` (None: the module's route): the edge list by ``ops.knn_edges``"""
        fused = self.fused if fused is None else bool(fused)
        with torch.no_grad():
            idxs, d2 = find_neighbors(src_embeddings, dst_embeddings, r_max=self.knn_radius, k_max=k,
                                      return_dist2=True, method=self.knn_method)
            if fused:
                graph = knn_edges(idxs, int(dst_embeddings.shape[0]), sym=sym)
            else:
                positive = idxs >= 0
                ind = torch.arange(idxs.shape[0], device=idxs.device).unsqueeze(1).expand(idxs.shape)
                if sym:
                    s, d = symmetrize(ind[positive], idxs[positive],
                                      max(src_embeddings.shape[0], dst_embeddings.shape[0]))
                    graph = torch.stack([s, d], dim=0)
                else:
                    graph = torch.stack([ind[positive], idxs[positive]], dim=0)
            if self.training and graph.shape[1] > 0:
                maximum_dist = d2.max().clamp(min=0).sqrt()      # padding slots hold -1: max over the valid ones
                self.knn_radius = 0.9 * self.knn_radius + 0.11 * maximum_dist
        return graph

    def edge_weights(self, src_embeddings, dst_embeddings, graph, norm=False, logits=False, stat_reduce=None,
                     fused=None):
        """gnn_utils.py:208-216: dot product -> BatchNorm1d(1) -> weighting function (-> /mean).
        ``stat_reduce``: the edges are one shard of an event (partition.py): synchronised batch statistics.
        ``fused`` (None: the module's route): the whole chain as ``attention_weights``; not with ``stat_reduce``"""
        if self.fused if fused is None else bool(fused):
            if stat_reduce is not None:
                raise ValueError("edge_weights: the fused route has no synchronised BatchNorm; stat_reduce needs "
                                 "the torch route (graph_construction='torch' or fused=False)")
            return attention_weights(src_embeddings, dst_embeddings, graph, self.weight_normalization,
                                     self._weighting_name, norm=norm, logits=logits)
        likelihood = edge_dot(src_embeddings, graph[0], dst_embeddings, graph[1])
        edge_weights_logits = batch_norm_1(self.weight_normalization, likelihood, stat_reduce)
        edge_weights = self.weighting_function(edge_weights_logits)
        if norm:
            edge_weights = edge_weights / edge_weights.mean()
        edge_weights = edge_weights.unsqueeze(1)
        if logits:
            return edge_weights, edge_weights_logits
        return edge_weights

    def forward(self, src_embeddings, dst_embeddings, sym=False, norm=False, k=10, logits=False):
        graph = self.build_graph(src_embeddings, dst_embeddings, sym=sym, k=k)
        out = self.edge_weights(src_embeddings, dst_embeddings, graph, norm=norm, logits=logits)
        if logits:
            return graph, out[0], out[1]
        return graph, out
