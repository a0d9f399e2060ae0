"""Tracking-performance metrics on the GPU (reference Modules/tracking_utils.py:18-83, ``eval_metrics``).

The reference builds them with cupy / cupy.sparse, and its edge-classifier step builds the track candidates with
cugraph (EdgeClassifier/edge_classifier_base.py:157-168); neither exists on ROCm.  Here:

    eval_metrics(bipartite_graph, event, ...)      same signature and return dict as the reference; one call of
                                                   ``hgnn_track_eval`` (csrc/trackeval.hip) and ONE host read, the
                                                   12-double result vector
    edge_track_candidates(edge_index, scores, score_cut, inverse_mask)
                                                   edge_classifier_base.py:157-168: components of the edges above
                                                   the cut (all edges when none passes), lock-free union-find
    bipartite_track_candidates(bipartite_graph, scores, score_cut, inverse_mask)
                                                   bipartite_classification_base.py:262-263
    embedding_track_candidates(embeddings, inverse_mask, min_cluster_size)
                                                   embedding_base.py:267-272: HDBSCAN clusters of the embeddings
                                                   (hdbscan.py, csrc/hdbscan.hip), noise dropped

There is no CPU path: every input must be a HIP device tensor.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .clustering import _cc
from .hdbscan import hdbscan as _hdbscan

default_response = {
    "track_eff": 0,
    "track_pur": 0,
    "hit_eff": 0,
    "hit_pur": 0
}

stats = {"host_reads": 0}


def _field(event, name):
    return event[name] if isinstance(event, dict) else getattr(event, name)


def _has(event, name) -> bool:
    return name in event if isinstance(event, dict) or hasattr(event, "__contains__") else hasattr(event, name)


def track_eval(bipartite_graph: torch.Tensor, event, pt_cut: float = 1., nhits_cut=5, majority_cut: float = 0.5,
               primary: bool = True) -> torch.Tensor:
    """``hgnn_track_eval``: the float64[HGNN_TE_RESULT] device result vector (indices ``_lib.TE_*``), without a
    host read.  ``primary=True`` needs an ``event.primary`` field: any hit of a particle with primary != 0 makes
    the particle primary (what the reference's dead ``primary=True`` branch intends)."""
    pid, pt = _field(event, "pid"), _field(event, "pt")
    if not (bipartite_graph.is_cuda and pid.is_cuda and pt.is_cuda):
        raise RuntimeError("eval_metrics needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    if bipartite_graph.dim() != 2 or bipartite_graph.shape[0] != 2:
        raise ValueError(f"eval_metrics: bipartite_graph must be [2, B], got {tuple(bipartite_graph.shape)}")
    if not float(majority_cut) > 0:
        raise ValueError("eval_metrics: majority_cut must be > 0")
    prim = None
    if primary:
        if not _has(event, "primary"):
            raise ValueError("eval_metrics(primary=True): the event has no `primary` field "
                             "(pass primary=False, as every reference training base does)")
        prim = _field(event, "primary").reshape(-1).ne(0).to(torch.uint8)
    dev = bipartite_graph.device
    hit = bipartite_graph[0].to(torch.int64).contiguous()
    cand = bipartite_graph[1].to(torch.int64).contiguous()
    pid = pid.reshape(-1).to(torch.int64).contiguous()
    pt = pt.reshape(-1).to(torch.float32).contiguous()
    if pt.numel() != pid.numel() or (prim is not None and prim.numel() != pid.numel()):
        raise ValueError("eval_metrics: event.pid, event.pt (and event.primary) must have one entry per hit")
    lib = _lib.load()
    ws, nb = _lib.workspace("hgnn_track_eval_workspace_bytes", dev, hit.numel(), pid.numel())
    result = torch.empty(_lib.TE_RESULT, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.hgnn_track_eval(_lib.ptr(hit), _lib.ptr(cand), hit.numel(), _lib.ptr(pid), _lib.ptr(pt),
                                       _lib.ptr(prim) if prim is not None else None, pid.numel(), float(pt_cut),
                                       float(nhits_cut), float(majority_cut), _lib.ptr(result), _lib.ptr(ws),
                                       nb, _lib.current_stream(dev)), "hgnn_track_eval")
    return result


def read_result(result: torch.Tensor) -> list:
    """the one host read of an evaluation; raises on an out-of-range hit id"""
    stats["host_reads"] += 1
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode(0)
    try:
        r = result.cpu().tolist()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if r[_lib.TE_STATUS] != 0:
        raise ValueError("eval_metrics: a hit id of bipartite_graph[0] is outside [0, len(event.pid))")
    return r


def eval_metrics(bipartite_graph, event, pt_cut=1., nhits_cut=5, majority_cut=0.5, primary=True):
    """Evaluate tracking performance (reference tracking_utils.eval_metrics).

    bipartite_graph: int64 [2, B] device tensor, (i, j) = hit i is assigned to track candidate j
    event: dict or attribute object with ``pid`` (int64, 0 = noise), ``pt`` and, for ``primary=True``, ``primary``
    Returns {"track_eff", "track_pur", "hit_eff", "hit_pur"} as Python floats (nan / inf where numpy gives them), or
    ``default_response`` (int zeros) when no candidate matches a particle, before or after the match filter, or when
    no pair survives the candidate size filter."""
    r = read_result(track_eval(bipartite_graph, event, pt_cut, nhits_cut, majority_cut, primary))
    if r[_lib.TE_NO_MATCH] != 0:
        return dict(default_response)
    return {
        "track_eff": r[_lib.TE_TRACK_EFF],
        "track_pur": r[_lib.TE_TRACK_PUR],
        "hit_eff": r[_lib.TE_HIT_EFF],
        "hit_pur": r[_lib.TE_HIT_PUR],
    }


def edge_track_candidates(edge_index: torch.Tensor, scores: torch.Tensor, score_cut, inverse_mask: torch.Tensor):
    """Track candidates of the edge classifier (edge_classifier_base.py:157-168): the weakly connected components of
    the edges with ``scores >= score_cut``, or of all edges when none passes (decided on the device).  Returns the
    int64 [2, K] bipartite graph (inverse_mask[v], label[v]) over the vertices v that touch a kept edge, in
    ascending v; label = the smallest (masked) vertex id of v's component."""
    if not edge_index.is_cuda:
        raise RuntimeError("edge_track_candidates needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    dev = edge_index.device
    n = int(inverse_mask.numel())
    scores = scores.detach().reshape(-1).float().contiguous()
    if scores.numel() != edge_index.shape[1]:
        raise ValueError("edge_track_candidates: one score per edge expected")
    if edge_index.shape[1] == 0:
        return torch.empty((2, 0), dtype=torch.int64, device=dev)
    cut = torch.full((1,), float(score_cut), dtype=torch.float32, device=dev)
    # torch: float32 scores >= Python float compares in float32, as the cut kernel does
    cut = torch.where((scores >= cut).any(), cut, torch.full_like(cut, -math.inf))
    labels, present = _cc(edge_index[0], edge_index[1], n, scores, cut)
    v = torch.nonzero(present).reshape(-1)
    return torch.stack([inverse_mask.to(torch.int64)[v], labels[v].to(torch.int64)], dim=0)


def bipartite_track_candidates(bipartite_graph: torch.Tensor, scores: torch.Tensor, score_cut,
                               inverse_mask: torch.Tensor) -> torch.Tensor:
    """Track candidates of the bipartite classifier (bipartite_classification_base.py:262-263): the pairs with
    ``scores >= score_cut``, hit ids mapped through ``inverse_mask``."""
    if not bipartite_graph.is_cuda:
        raise RuntimeError("bipartite_track_candidates needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    g = bipartite_graph[:, scores.reshape(-1) >= score_cut]
    return torch.stack([inverse_mask.to(torch.int64)[g[0]], g[1].to(torch.int64)], dim=0)


def embedding_track_candidates(embeddings: torch.Tensor, inverse_mask: torch.Tensor = None,
                               min_cluster_size: int = 5) -> torch.Tensor:
    """Track candidates of the embedding models (embedding_base.py:267-272): HDBSCAN clusters of the embeddings
    (``inference_min_cluster_size``), noise dropped.  Returns the int64 [2, B] graph (hit, cluster label) over the
    clustered hits in ascending hit position, hit ids mapped through ``inverse_mask`` when it is given; ready for
    ``eval_metrics``."""
    if not embeddings.is_cuda:
        raise RuntimeError("embedding_track_candidates needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    clusters = _hdbscan(embeddings.detach().float(), min_cluster_size)
    hits = torch.nonzero(clusters >= 0).reshape(-1)
    labels = clusters[hits]
    if inverse_mask is not None:
        hits = inverse_mask.to(torch.int64)[hits]
    return torch.stack([hits, labels], dim=0)
