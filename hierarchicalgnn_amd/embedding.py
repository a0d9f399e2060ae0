"""The embedding stage's per-step pair construction on the GPU (reference GNNEmbedding/embedding_base.py).

Every training step of Embedding-IN / Embedding-HGNN-GMM calls ``get_training_samples`` (:109-135): a
fixed-radius kNN graph of the embeddings with knn = 100 (frnn, CUDA-only, there) and ``graph_intersection``
(utils.py:117-166, scipy CSR on the host there).  Here:

    frnn_graph(embeddings, r, k)                     utils.FRNN_graph: ops.knn_radius (k <= 128, csrc/knn_large.hip
                                                     for k > 32), [2, E] int64, query ascending, then slot order
    graph_intersection(pred_graph, truth_graph, using_weights=False, weights_bidir=None)
                                                     utils.graph_intersection: one hgnn_graph_intersection call
                                                     (csrc/intersect.hip) and ONE host read (the count and status)
    training_samples(embeddings, batch, hparams)     EmbeddingBase.get_training_samples, both true_edges modes
    training_weights(batch, graph, y, hparams)       pt_weighting + get_training_weight (:95-107, :137-146)
    hinge_distance(embeddings, graph, y)             get_hinge_distance (:148-155)

Differences from the reference, all deliberate: results stay on the input's device (the reference returns CPU
tensors from graph_intersection and its callers move them), and an empty pred graph gives an empty result (the
reference raises on ``.max()`` of an empty tensor).  There is no CPU path: inputs must be HIP device tensors.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .ops import knn_radius

stats = {"host_reads": 0}


def _field(batch, name):
    return batch[name] if isinstance(batch, dict) else getattr(batch, name)


def frnn_graph(embeddings: torch.Tensor, r, k: int) -> torch.Tensor:
    """utils.FRNN_graph (utils.py:241-252): the pairs (query, neighbour) of the fixed-radius kNN of the embeddings
    among themselves, self pairs included, int64 [2, E] with the query ascending and then the neighbours in slot order
    (ascending distance, ties to the lower index)."""
    if not embeddings.is_cuda:
        raise RuntimeError("frnn_graph needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    idx = knn_radius(embeddings, embeddings, int(k), r)
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
    nb = ctypes.c_size_t(0)
    _lib.check(lib.hgnn_graph_intersection_workspace_bytes(ep, et, 1 if using_weights else 0, ctypes.byref(nb)),
               "hgnn_graph_intersection_workspace_bytes")
    ws = torch.empty(max(int(nb.value), 1), dtype=torch.uint8, device=dev)
    out_graph = torch.empty((2, ep), dtype=torch.int64, device=dev)
    out_y = torch.empty(ep, dtype=torch.uint8, device=dev)
    out_w = torch.empty(ep, dtype=w.dtype, device=dev) if using_weights else None
    cs = torch.zeros(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.hgnn_graph_intersection(_lib.ptr(pred), ep, _lib.ptr(truth), et, _lib.ptr(w), wdt,
                                               _lib.ptr(out_graph), _lib.ptr(out_y), _lib.ptr(out_w), _lib.ptr(cs),
                                               _lib.ptr(ws), int(nb.value), _lib.current_stream(dev)),
                   "hgnn_graph_intersection")
    stats["host_reads"] += 1
    u, status = cs.tolist()
    if status != 0:
        raise ValueError("graph_intersection: a vertex id is negative or >= 2**31")
    new_graph, y = out_graph[:, :u], out_y[:u].view(torch.bool)
    if using_weights:
        return new_graph, y, out_w[:u]
    return new_graph, y


def training_samples(embeddings, batch, hparams, prediction_graph=None):
    """EmbeddingBase.get_training_samples (embedding_base.py:109-135) for both ``true_edges`` modes.  ``batch``:
    anything with ``modulewise_true_edges``, ``signal_mask`` and ``pid`` (attributes or keys) on the embeddings'
    device.  ``prediction_graph`` replaces the kNN graph when given (the reference always builds it)."""
    dev = embeddings.device
    if prediction_graph is None:
        prediction_graph = frnn_graph(embeddings, hparams["train_r"], hparams["knn"])
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
