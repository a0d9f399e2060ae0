"""The embedding stage's per-step pair construction on the GPU (reference GNNEmbedding/embedding_base.py).

Every training step of Embedding-IN / Embedding-HGNN-GMM calls ``get_training_samples`` (:109-135): a
fixed-radius kNN graph of the embeddings with knn = 100 (frnn, CUDA-only, there) and ``graph_intersection``
(utils.py:117-166, scipy CSR on the host there).  Here:

    frnn_graph(embeddings, r, k, method=None)        utils.FRNN_graph: ops.knn_radius (k <= 128, csrc/knn_large.hip
                                                     for k > 32, csrc/knn_sorted.hip with method="sorted"), [2, E]
                                                     int64, query ascending, then slot order
    graph_intersection(pred_graph, truth_graph, using_weights=False, weights_bidir=None)
                                                     utils.graph_intersection: one hgnn_graph_intersection call
                                                     (csrc/intersect.hip) and ONE host read (the count and status)
    training_samples(embeddings, batch, hparams, prediction_graph=None, fused=False)
                                                     EmbeddingBase.get_training_samples, both true_edges modes;
                                                     fused=True: knn_radius + training_pairs, the same bits
    training_pairs(knn_idx, batch, hparams)          the same from the kNN matrix [N, K <= 128], row by row
                                                     (csrc/trainpairs.hip): no [2, N*K] graph, no sort of the pairs,
                                                     ONE host read (the sizes and the status)
    training_weights(batch, graph, y, hparams)       pt_weighting + get_training_weight (:95-107, :137-146)
    hinge_distance(embeddings, graph, y)             get_hinge_distance (:148-155)
    pair_hinge_loss(embeddings, graph, y, batch, hparams, margin=None, scale=1.0)
                                                     the three lines above + hinge_embedding_loss(..)^2 . weights
                                                     (:167-168) as ONE operator, csrc/pairloss.hip: no [P, emb_dim]
                                                     tensor, no host read, bitwise reproducible forward and backward
    embedding_hgnn_training_loss(...) / embedding_in_training_loss(...)
                                                     training_step after the forward (:160-181 / :191-199)

Differences from the reference, all deliberate: results stay on the input's device (the reference returns CPU
tensors from graph_intersection and its callers move them), and an empty pred graph gives an empty result (the
reference raises on ``.max()`` of an empty tensor); in ``pair_hinge_loss`` a class of pairs without weight (an empty
class in particular) contributes nothing where the reference's 0/0 makes the loss NaN.  There is no CPU path: inputs must be HIP device tensors.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .ops import knn_radius
from .plan import GraphPlan, memo

stats = {"host_reads": 0}


def _field(batch, name):
    return batch[name] if isinstance(batch, dict) else getattr(batch, name)


# DESIGN.md section 3 "k_knn_sorted" records the measurement this default rests on
FRNN_DEFAULT_METHOD = "brute"


def frnn_graph(embeddings: torch.Tensor, r, k: int, method=None) -> torch.Tensor:
    """utils.FRNN_graph (utils.py:241-252): the pairs (query, neighbour) of the fixed-radius kNN of the embeddings
    among themselves, self pairs included, int64 [2, E] with the query ascending and then the neighbours in slot order
    (ascending distance, ties to the lower index).  ``method``: ops.knn_radius's ("brute" or "sorted": the same
    graph bit for bit); None = the default, FRNN_DEFAULT_METHOD."""
    if not embeddings.is_cuda:
        raise RuntimeError("frnn_graph needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    idx = knn_radius(embeddings, embeddings, int(k), r, method=FRNN_DEFAULT_METHOD if method is None else method)
    pos = idx >= 0
    ind = torch.arange(idx.shape[0], device=idx.device).unsqueeze(1).expand(idx.shape)
    return torch.stack([ind[pos], idx[pos]], dim=0)


def _as_graph(g, name):
    if not torch.is_tensor(g) or not g.is_cuda:
        raise RuntimeError(f"graph_intersection needs HIP device tensors ({name}): hierarchicalgnn_amd has no CPU path")
    if g.dim() != 2 or g.shape[0] != 2:
        raise ValueError(f"graph_intersection: {name} must be [2, E], got {tuple(g.shape)}")
    if g.dtype.is_floating_point or g.dtype == torch.bool:
        raise ValueError(f"graph_intersection: {name} must hold integer ids, got {g.dtype}")
    return g.to(torch.int64).contiguous()


def graph_intersection(pred_graph, truth_graph, using_weights=False, weights_bidir=None):
    """utils.graph_intersection: (new_pred_graph int64 [2, U], y bool [U]) -- and new_weights [U] with
    ``using_weights`` -- where new_pred_graph holds the distinct pred pairs in row-major order, y whether each also
    occurs in truth, new_weights the sum of ``weights_bidir`` over the truth copies of the pair (0 if none; float32 or
    float64 as given).  Pairs found only in truth are dropped.  Ids must lie in [0, 2^31): ValueError otherwise."""
    pred = _as_graph(pred_graph, "pred_graph")
    truth = _as_graph(truth_graph, "truth_graph")
    dev = pred.device
    if truth.device != dev:
        raise ValueError("graph_intersection: pred_graph and truth_graph must be on the same device")
    ep, et = int(pred.shape[1]), int(truth.shape[1])
    w, wdt = None, _lib.DT_F32
    if using_weights:
        if weights_bidir is None or not torch.is_tensor(weights_bidir) or not weights_bidir.is_cuda:
            raise RuntimeError("graph_intersection(using_weights=True) needs weights_bidir as a HIP device tensor")
        w = weights_bidir.reshape(-1)
        if w.numel() != et or w.device != dev:
            raise ValueError("graph_intersection: weights_bidir needs one entry per truth pair, on the graphs' device")
        if w.dtype == torch.float64:
            wdt = _lib.DT_F64
        elif w.dtype != torch.float32:
            raise ValueError(f"graph_intersection: weights_bidir must be float32 or float64, got {w.dtype}")
        w = w.contiguous()
    lib = _lib.load()
    ws, nb = _lib.workspace("hgnn_graph_intersection_workspace_bytes", dev, ep, et, 1 if using_weights else 0)
    out_graph = torch.empty((2, ep), dtype=torch.int64, device=dev)
    out_y = torch.empty(ep, dtype=torch.uint8, device=dev)
    out_w = torch.empty(ep, dtype=w.dtype, device=dev) if using_weights else None
    cs = torch.zeros(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.hgnn_graph_intersection(_lib.ptr(pred), ep, _lib.ptr(truth), et, _lib.ptr(w), wdt,
                                               _lib.ptr(out_graph), _lib.ptr(out_y), _lib.ptr(out_w), _lib.ptr(cs),
                                               _lib.ptr(ws), nb, _lib.current_stream(dev)),
                   "hgnn_graph_intersection")
    stats["host_reads"] += 1
    u, status = cs.tolist()
    if status != 0:
        raise ValueError("graph_intersection: a vertex id is negative or >= 2**31")
    new_graph, y = out_graph[:, :u], out_y[:u].view(torch.bool)
    if using_weights:
        return new_graph, y, out_w[:u]
    return new_graph, y


def _knn_method(hparams):
    """the optional hparams["knn_method"] (None: the default)"""
    return hparams["knn_method"] if "knn_method" in hparams else None


_TP_MODES = {"modulewise_true_edges": _lib.TP_MODE_MODULEWISE, "pid_true_edges": _lib.TP_MODE_PID}


def training_pairs(knn_idx, batch, hparams):
    """``training_samples`` from the kNN matrix itself: (graph int64 [2, P], y bool [P]), bit-equal to
    ``training_samples(..., prediction_graph=<the pairs (row, id) of the valid slots of knn_idx, row-major>)``, pair
    order included, in both ``hparams["true_edges"]`` modes -- without that [2, N*K] graph, without a sort of the
    pairs and with ONE host read (the sizes and the status, counted in ``stats["host_reads"]``); csrc/trainpairs.hip.

    ``knn_idx`` int64 [N, K], 1 <= K <= 128 (``ops.knn_radius``'s): ids in [0, N), -1 = an empty slot, anywhere in a
    row; duplicates within a row are allowed.  ``batch``: ``modulewise_true_edges`` int64 [2, T], ``signal_mask`` bool
    [N], ``pid`` int64 [N], on knn_idx's device.  Both results are contiguous and exactly sized.  ValueError for a
    wrong dtype or shape, tensors on different devices or an unknown mode (before any launch), and, after the read,
    for an entry of knn_idx outside [-1, N) or an id of modulewise_true_edges outside [0, N) (such an id is skipped by
    the kernels and never used as an address).  RuntimeError for CPU tensors: there is no CPU path."""
    mte = _field(batch, "modulewise_true_edges")
    signal_mask = _field(batch, "signal_mask")
    pid = _field(batch, "pid")
    for t, name in ((knn_idx, "knn_idx"), (mte, "modulewise_true_edges"), (signal_mask, "signal_mask"), (pid, "pid")):
        if not torch.is_tensor(t):
            raise ValueError(f"training_pairs: {name} must be a tensor")
    if knn_idx.dtype != torch.int64 or knn_idx.dim() != 2:
        raise ValueError(f"training_pairs: knn_idx must be int64 [N, K], got {knn_idx.dtype} {tuple(knn_idx.shape)}")
    n, k = int(knn_idx.shape[0]), int(knn_idx.shape[1])
    if not 1 <= k <= _lib.TP_MAX_K:
        raise ValueError(f"training_pairs: K = {k} must be in [1, {_lib.TP_MAX_K}]")
    if mte.dtype != torch.int64 or mte.dim() != 2 or mte.shape[0] != 2:
        raise ValueError(f"training_pairs: modulewise_true_edges must be int64 [2, T], got {mte.dtype} "
                         f"{tuple(mte.shape)}")
    if signal_mask.dtype != torch.bool or tuple(signal_mask.shape) != (n,):
        raise ValueError(f"training_pairs: signal_mask must be bool [N = {n}], got {signal_mask.dtype} "
                         f"{tuple(signal_mask.shape)}")
    if pid.dtype != torch.int64 or tuple(pid.shape) != (n,):
        raise ValueError(f"training_pairs: pid must be int64 [N = {n}], got {pid.dtype} {tuple(pid.shape)}")
    dev = knn_idx.device
    if mte.device != dev or signal_mask.device != dev or pid.device != dev:
        raise ValueError("training_pairs: knn_idx, modulewise_true_edges, signal_mask and pid must be on one device")
    mode = hparams["true_edges"]
    if mode not in _TP_MODES:
        raise ValueError(f"training_pairs: true_edges must be 'modulewise_true_edges' or 'pid_true_edges', "
                         f"got {mode!r}")
    t = int(mte.shape[1])
    if n * k + 2 * t >= 2 ** 31 or t >= 2 ** 29:
        raise ValueError(f"training_pairs: N * K + 2 T = {n * k + 2 * t} must stay below 2^31 (and T below 2^29)")
    if not knn_idx.is_cuda:
        raise RuntimeError("training_pairs needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    if n == 0:
        if t > 0:
            raise ValueError("training_pairs: an id of modulewise_true_edges is outside [0, N = 0)")
        return torch.empty((2, 0), dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.bool, device=dev)
    graph, y, info = _tp_launch(knn_idx.detach().contiguous(), mte.contiguous(),
                                signal_mask.contiguous().view(torch.uint8), pid.contiguous(), _TP_MODES[mode])
    return graph, y


def _tp_launch(idx, mte, sm8, pid, mode, check=True):
    """hgnn_training_pairs_count, the one host read, hgnn_training_pairs_fill on checked, contiguous device tensors:
    (graph, y, info).  ``check=False`` (tests): a bad-id status fills all the same -- the kernels skip such an id."""
    dev = idx.device
    n, k, t = int(idx.shape[0]), int(idx.shape[1]), int(mte.shape[1])
    lib = _lib.load()
    ws, nb = _lib.workspace("hgnn_training_pairs_workspace_bytes", dev, n, k, t, mode)
    info = torch.empty(_lib.TP_INFO, dtype=torch.int64, device=dev)
    args = (_lib.ptr(idx), n, k, _lib.ptr(mte), t, _lib.ptr(sm8), _lib.ptr(pid), mode)
    with torch.cuda.device(dev):
        _lib.check(lib.hgnn_training_pairs_count(*args, _lib.ptr(info), _lib.ptr(ws), nb, _lib.current_stream(dev)),
                   "hgnn_training_pairs_count")
        stats["host_reads"] += 1
        info = info.tolist()
        p, status = info[_lib.TP_P], info[_lib.TP_STATUS]
        if check and status & _lib.TP_ST_BAD_IDX:
            raise ValueError(f"training_pairs: an entry of knn_idx is outside [-1, N = {n})")
        if check and status & _lib.TP_ST_BAD_MTE:
            raise ValueError(f"training_pairs: an id of modulewise_true_edges is outside [0, N = {n})")
        graph = torch.empty((2, p), dtype=torch.int64, device=dev)
        y = torch.empty(p, dtype=torch.uint8, device=dev)
        _lib.check(lib.hgnn_training_pairs_fill(*args, _lib.ptr(graph), _lib.ptr(y), p, _lib.ptr(ws), nb,
                                                _lib.current_stream(dev)),
                   "hgnn_training_pairs_fill")
    return graph, y.view(torch.bool), info


def training_samples(embeddings, batch, hparams, prediction_graph=None, fused=False):
    """EmbeddingBase.get_training_samples (embedding_base.py:109-135) for both ``true_edges`` modes.  ``batch``:
    anything with ``modulewise_true_edges``, ``signal_mask`` and ``pid`` (attributes or keys) on the embeddings'
    device.  ``prediction_graph`` replaces the kNN graph when given (the reference always builds it); the optional
    ``hparams["knn_method"]`` is frnn_graph's ``method``.  ``fused=True``: the same result, bit for bit, from
    ``knn_radius`` and ``training_pairs`` -- one host read, no prediction graph (so none can be given)."""
    if fused:
        if prediction_graph is not None:
            raise ValueError("training_samples(fused=True) builds the pairs from the kNN matrix: it takes no "
                             "prediction_graph")
        if not torch.is_tensor(embeddings) or not embeddings.is_cuda:
            raise RuntimeError("training_samples(fused=True) needs HIP device tensors: hierarchicalgnn_amd has no "
                               "CPU path")
        method = _knn_method(hparams)
        idx = knn_radius(embeddings, embeddings, int(hparams["knn"]), hparams["train_r"],
                         method=FRNN_DEFAULT_METHOD if method is None else method)
        return training_pairs(idx, batch, hparams)
    dev = embeddings.device
    if prediction_graph is None:
        prediction_graph = frnn_graph(embeddings, hparams["train_r"], hparams["knn"], _knn_method(hparams))
    mte = _field(batch, "modulewise_true_edges")
    signal_mask = _field(batch, "signal_mask")
    pid = _field(batch, "pid")
    e_bidir = torch.cat([mte, mte.flip(0)], dim=1)
    e_bidir = e_bidir[:, signal_mask[e_bidir].all(0)]
    mode = hparams["true_edges"]
    if mode == "modulewise_true_edges":
        new_graph, y = graph_intersection(prediction_graph, e_bidir)
        fake_samples = new_graph[:, y == 0]
        pid_mask = (pid[fake_samples[0]] != pid[fake_samples[1]]) | (pid[fake_samples] == 0).any(0)
        fake_samples = fake_samples[:, pid_mask]
        new_graph = torch.cat([fake_samples, e_bidir], dim=1)
        y = torch.cat([torch.zeros(fake_samples.shape[1], device=dev),
                       torch.ones(e_bidir.shape[1], device=dev)], dim=0).bool()
    elif mode == "pid_true_edges":
        new_graph = torch.cat([prediction_graph, e_bidir], dim=1)
        y = (pid[new_graph[0]] == pid[new_graph[1]]) & (pid[new_graph] != 0).all(0)
        # embedding_base.py:131 as written: `|` binds tighter than `==`, so this is ((all | y) == 0)
        mask = (signal_mask[new_graph]).all(0) | y == 0
        new_graph = new_graph[:, mask]
        y = y[mask]
    else:
        raise ValueError(f"training_samples: true_edges must be 'modulewise_true_edges' or 'pid_true_edges', "
                         f"got {mode!r}")
    return new_graph, y


def pt_weighting(pt, hparams):
    """EmbeddingBase.pt_weighting (embedding_base.py:95-107) on a copy of ``pt``"""
    pt = pt.clone()
    pt[pt != pt] = 0
    h = lambda i: torch.heaviside(i, torch.zeros(1).to(pt))  # noqa: E731
    minimum = lambda i: torch.minimum(i, torch.ones(1).to(pt))  # noqa: E731
    eps = hparams["weight_leak"]
    cut = hparams["ptcut"] - hparams["pt_interval"]
    cap = hparams["ptcut"]
    min_weight = hparams["weight_min"]
    return min_weight + (1 - min_weight) * minimum(h(pt - cut) * (pt - cut) / (cap - cut)) + (eps * h(pt - cap) * (pt - cap))


def training_weights(batch, graph, y, hparams):
    """EmbeddingBase.get_training_weight (embedding_base.py:137-146); ``batch.pt`` is not written"""
    pt = _field(batch, "pt")
    dev = graph.device
    weights = pt_weighting(pt[graph[0]], hparams) + pt_weighting(pt[graph[1]], hparams)
    true_weights = weights[y].sum()
    fake_weights = weights[~y].sum()
    lwr = hparams["log_weight_ratio"]
    weights[y] = (weights[y] / true_weights) * torch.sigmoid(lwr * torch.ones(1, device=dev))
    weights[~y] = (weights[~y] / fake_weights) * torch.sigmoid(-lwr * torch.ones(1, device=dev))
    return weights.float()


def hinge_distance(embeddings, graph, y):
    """EmbeddingBase.get_hinge_distance (embedding_base.py:148-155): (hinge int64 +-1, distance)"""
    hinge = torch.ones(len(y), device=embeddings.device).long()
    hinge[~y] = -1
    dist = ((embeddings[graph[0]] - embeddings[graph[1]]).square().sum(-1) + 1e-12).sqrt()
    return hinge, dist


# --------------------------------------------------------------------------- the fused pair hinge loss
_ph_pending = _lib.PendingStatus(stats)


def _ph_scalars(hparams, margin, scale):
    h = _lib.pt_scalars(hparams)
    h[_lib.PH_MARGIN] = float(hparams["train_r"] if margin is None else margin)
    h[_lib.PH_SCALE] = float(scale)
    return h


def _ph_plan(graph, n, cache):
    """the destination-sorted plan over cat(a, b) with the other endpoint as its gather index: every pair sits in the
    list of both of its endpoints.  Unvalidated (no host read): ids out of range are dropped by the plan build.
    Costs beside the kernels, per call: the flipped copy of the graph (2P int64), an int64 copy of an int32 graph (the
    plan build takes int64), and the build itself (a radix sort of 2P keys) -- every step for the training samples,
    whose pairs change with the embeddings; once per event with ``cache`` (DESIGN.md section 3 "k_ph" has the times)."""
    g64 = graph if graph.dtype == torch.int64 else graph.long()
    build = lambda: GraphPlan(g64.reshape(-1), n, g64.flip(0).reshape(-1), n, validate=False)  # noqa: E731
    if cache and g64 is graph:
        # kept with the graph tensor (plan.memo), not in the shared plan cache: that cache's key does not tell an
        # unvalidated plan from a range-checked one
        return memo(graph, f"pair_hinge_plan/{n}", build)
    return build()


class _PairHinge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, graph, y8, pt, scalars, cache_plan):
        lib = _lib.load()
        dev = emb.device
        n, d, p = int(emb.shape[0]), int(emb.shape[1]), int(graph.shape[1])
        idt = _lib.index_dtype(graph)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        state = torch.empty(_lib.PH_STATE, dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        ws, nb = _lib.workspace("hgnn_pair_hinge_workspace_bytes", dev, p, n, d, 0)
        with torch.cuda.device(dev):
            _lib.check(lib.hgnn_pair_hinge_forward(_lib.ptr(emb), n, d, _lib.ptr(graph), idt, _lib.ptr(y8),
                                                   _lib.ptr(pt), p, scalars, _lib.ptr(loss), _lib.ptr(state),
                                                   _lib.ptr(status), _lib.ptr(ws), nb, _lib.current_stream(dev)),
                       "hgnn_pair_hinge_forward")
        ctx.plan = None
        if ctx.needs_input_grad[0]:
            # built once per call, next to the forward; the backward only walks it
            ctx.plan = _ph_plan(graph, n, cache_plan) if p > 0 and n > 0 else None
            ctx.save_for_backward(emb, graph, y8, pt, state)
            ctx.scalars, ctx.idt = scalars, idt
        ctx.mark_non_differentiable(status)
        return loss.reshape(()), status

    @staticmethod
    def backward(ctx, grad_loss, _grad_status):
        emb, graph, y8, pt, state = ctx.saved_tensors
        lib = _lib.load()
        dev = emb.device
        n, d, p = int(emb.shape[0]), int(emb.shape[1]), int(graph.shape[1])
        g = grad_loss.detach().reshape(1).to(torch.float32).contiguous()
        grad = torch.empty_like(emb)
        ws, nb = _lib.workspace("hgnn_pair_hinge_workspace_bytes", dev, p, n, d, 1)
        with torch.cuda.device(dev):
            _lib.check(lib.hgnn_pair_hinge_backward(ctypes.byref(ctx.plan.c) if ctx.plan is not None else None,
                                                    _lib.ptr(emb), n, d, _lib.ptr(graph), ctx.idt, _lib.ptr(y8),
                                                    _lib.ptr(pt), p, ctx.scalars, _lib.ptr(state), _lib.ptr(g),
                                                    _lib.ptr(grad), _lib.ptr(ws), nb, _lib.current_stream(dev)),
                       "hgnn_pair_hinge_backward")
        return grad, None, None, None, None, None


def pair_hinge_check(device=None):
    """Reads (ONE host read per device, counted in ``stats["host_reads"]``) and clears the status words of the
    ``pair_hinge_loss`` calls made since the last check: ValueError if any of them saw a pair id outside [0, N)."""
    if _ph_pending.take(device):
        raise ValueError("pair_hinge_loss: a pair id is negative or >= the number of embedding rows")


def pair_hinge_loss(embeddings, graph, y, batch, hparams, margin=None, scale=1.0, check=False, cache_plan=False):
    """sum_i w_i l_i^2 (0-d float32, differentiable in ``embeddings`` only) with w = training_weights(batch, graph, y,
    hparams), d = hinge_distance(embeddings, graph, y), l_i = scale d_i for a true pair and max(0, margin - scale d_i)
    for a false one: ``hinge_embedding_loss(scale * d, hinge, margin, 'none').square() . w`` of the reference's
    training steps.  ``margin`` defaults to ``hparams["train_r"]`` (the embedding stage: scale 1, margin train_r;
    ``bc_embedding_loss``: scale 1 / train_r, margin 1).

    ``embeddings`` float32 [N, D <= 16]; ``graph`` [2, P] int64 or int32; ``y`` [P] bool or uint8; ``batch.pt`` float32
    [N], not written.  The class sums and the loss are float64 sums in a fixed order and the gradient uses no
    atomics: two calls return the same bits.  A class of pairs whose weights sum to 0 contributes nothing.

    The call makes NO host read.  A pair id outside [0, N) is skipped by the kernels (never a fault) and recorded in a
    device status word; ``check=True`` reads it after the call (one host read, counted in ``stats["host_reads"]``) and
    raises ValueError, as does a later ``pair_hinge_check()``.  ``cache_plan=True`` keeps the backward's plan with the
    graph tensor (``plan.memo``), for a ``graph`` tensor that is reused from step to step (an event's input edges)."""
    if not torch.is_tensor(embeddings) or not embeddings.is_cuda or not torch.is_tensor(graph) or not graph.is_cuda:
        raise RuntimeError("pair_hinge_loss needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    dev = embeddings.device
    if embeddings.dim() != 2 or embeddings.dtype != torch.float32 or not 1 <= embeddings.shape[1] <= _lib.PH_MAX_DIM:
        raise ValueError(f"pair_hinge_loss: embeddings must be float32 [N, D <= {_lib.PH_MAX_DIM}], got "
                         f"{embeddings.dtype} {tuple(embeddings.shape)}")
    if graph.dim() != 2 or graph.shape[0] != 2 or graph.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"pair_hinge_loss: graph must be int64 or int32 [2, P], got {graph.dtype} {tuple(graph.shape)}")
    if not torch.is_tensor(y) or y.dtype not in (torch.bool, torch.uint8) or y.shape != (graph.shape[1],):
        raise ValueError("pair_hinge_loss: y must be bool or uint8 with one entry per pair")
    pt = _field(batch, "pt")
    if pt.dtype != torch.float32 or pt.numel() != embeddings.shape[0]:
        raise ValueError("pair_hinge_loss: batch.pt must be float32 with one entry per embedding row")
    if graph.device != dev or y.device != dev or pt.device != dev:
        raise ValueError("pair_hinge_loss: embeddings, graph, y and batch.pt must be on one device")
    y8 = y.contiguous().view(torch.uint8)
    loss, status = _PairHinge.apply(embeddings.contiguous(), graph.contiguous(), y8, pt.detach().reshape(-1).contiguous(),
                                    _ph_scalars(hparams, margin, scale), bool(cache_plan))
    _ph_pending.add(dev, status)
    if check:
        pair_hinge_check(dev)
    return loss


def embedding_in_training_loss(embeddings, batch, hparams, prediction_graph=None, fused_samples=False):
    """EmbeddingBase.training_step for Embedding-IN after the forward (embedding_base.py:191-199);
    ``fused_samples``: training_samples' ``fused``"""
    graph, y = training_samples(embeddings, batch, hparams, prediction_graph, fused=fused_samples)
    return pair_hinge_loss(embeddings, graph, y, batch, hparams)


def embedding_hgnn_training_loss(embeddings, intermediate_embeddings, batch, hparams, loss_schedule,
                                 prediction_graph=None, fused_samples=False):
    """EmbeddingBase.training_step for Embedding-HGNN-GMM after the forward (embedding_base.py:160-181):
    (loss, emb_loss, intermediate_loss) with loss = loss_schedule * intermediate_loss + (1 - loss_schedule) * emb_loss.
    The intermediate term is the PID truth on ``batch.edge_index`` with the intermediate embeddings, the second term
    ``training_samples`` with the final ones.  ``loss_schedule`` is the caller's (the reference takes it from hparams
    or from the epoch, :177-180).  ``fused_samples``: training_samples' ``fused``."""
    edge_index = _field(batch, "edge_index")
    pid = _field(batch, "pid")
    y_pid = pid[edge_index[0]] == pid[edge_index[1]]
    intermediate_loss = pair_hinge_loss(intermediate_embeddings, edge_index, y_pid, batch, hparams, cache_plan=True)
    graph, y = training_samples(embeddings, batch, hparams, prediction_graph, fused=fused_samples)
    emb_loss = pair_hinge_loss(embeddings, graph, y, batch, hparams)
    loss = (loss_schedule * intermediate_loss) + ((1 - loss_schedule) * emb_loss)
    return loss, emb_loss, intermediate_loss
