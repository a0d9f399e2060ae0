"""Tracking-performance metrics on the GPU (reference Modules/tracking_utils.py:18-83, ``eval_metrics``).

The reference builds them with cupy / cupy.sparse, and its edge-classifier step builds the track candidates with
cugraph (EdgeClassifier/edge_classifier_base.py:157-168); neither exists on ROCm.  Here:

    eval_metrics(bipartite_graph, event, ...)      same signature and return dict as the reference; one call of
                                                   ``hgnn_track_eval`` (csrc/trackeval.hip) and ONE host read, the
                                                   12-double result vector
    track_records(bipartite_graph, event, bins, ...)
                                                   the same metrics with the per-particle table, the per-candidate
                                                   table and integer histograms over chosen variables: one call of
                                                   ``hgnn_track_records`` (csrc/trackeval_records.hip), the same ONE
                                                   host read
    edge_track_candidates(edge_index, scores, score_cut, inverse_mask)
                                                   edge_classifier_base.py:157-168: components of the edges above
                                                   the cut (all edges when none passes), lock-free union-find
    bipartite_track_candidates(bipartite_graph, scores, score_cut, inverse_mask)
                                                   bipartite_classification_base.py:262-263
    embedding_track_candidates(embeddings, inverse_mask, min_cluster_size)
                                                   embedding_base.py:267-272: HDBSCAN clusters of the embeddings
                                                   (hdbscan.py, csrc/hdbscan.hip), noise dropped
    edge_score_scan(edge_index, scores, cuts, inverse_mask, event, ...)
    bipartite_score_scan(bipartite_graph, scores, cuts, inverse_mask, event, ...)
                                                   what edge_track_candidates / bipartite_track_candidates followed by
                                                   eval_metrics give at every one of up to 64 score cuts, and the
                                                   integer edge counts per cut: one call of ``hgnn_track_scan``
                                                   (csrc/trackscan.hip) and ONE host read for the whole list

There is no CPU path: every input must be a HIP device tensor.
"""
from __future__ import annotations

import ctypes
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


def _inputs(who: str, bipartite_graph: torch.Tensor, event, majority_cut, primary):
    """the checked operands of ``hgnn_track_eval`` / ``hgnn_track_records``: (hit, cand, pid, pt, prim or None)"""
    pid, pt = _field(event, "pid"), _field(event, "pt")
    if not (bipartite_graph.is_cuda and pid.is_cuda and pt.is_cuda):
        raise RuntimeError(f"{who} needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    if bipartite_graph.dim() != 2 or bipartite_graph.shape[0] != 2:
        raise ValueError(f"{who}: bipartite_graph must be [2, B], got {tuple(bipartite_graph.shape)}")
    if not float(majority_cut) > 0:
        raise ValueError(f"{who}: majority_cut must be > 0")
    prim = None
    if primary:
        if not _has(event, "primary"):
            raise ValueError(f"{who}(primary=True): the event has no `primary` field "
                             "(pass primary=False, as every reference training base does)")
        prim = _field(event, "primary").reshape(-1).ne(0).to(torch.uint8)
    hit = bipartite_graph[0].to(torch.int64).contiguous()
    cand = bipartite_graph[1].to(torch.int64).contiguous()
    pid = pid.reshape(-1).to(torch.int64).contiguous()
    pt = pt.reshape(-1).to(torch.float32).contiguous()
    if pt.numel() != pid.numel() or (prim is not None and prim.numel() != pid.numel()):
        raise ValueError(f"{who}: event.pid, event.pt (and event.primary) must have one entry per hit")
    return hit, cand, pid, pt, prim


def track_eval(bipartite_graph: torch.Tensor, event, pt_cut: float = 1., nhits_cut=5, majority_cut: float = 0.5,
               primary: bool = True) -> torch.Tensor:
    """``hgnn_track_eval``: the float64[HGNN_TE_RESULT] device result vector (indices ``_lib.TE_*``), without a
    host read.  ``primary=True`` needs an ``event.primary`` field: any hit of a particle with primary != 0 makes
    the particle primary (what the reference's dead ``primary=True`` branch intends)."""
    hit, cand, pid, pt, prim = _inputs("eval_metrics", bipartite_graph, event, majority_cut, primary)
    dev = bipartite_graph.device
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


PARTICLE_FIELDS = (("pid", torch.int64), ("nhits", torch.int32), ("pt", torch.float32), ("primary", torch.uint8),
                   ("reconstructable", torch.uint8), ("n_match", torch.int32), ("n_kept", torch.int32),
                   ("n_mask", torch.int32), ("cand_index", torch.int32), ("shared", torch.int32))
CANDIDATE_FIELDS = (("label", torch.int64), ("size", torch.int32), ("n_kept", torch.int32), ("n_mask", torch.int32),
                    ("particle", torch.int32), ("shared", torch.int32))
# the columns of a histogram slot, in order
BIN_COLUMNS = ("particles", "reconstructable", "n_kept", "n_mask", "masked_shared", "masked_nhits")
COUNT_KEYS = ("n_kept", "n_mask", "n_truth", "n_cand", "n_part", "n_match")


def _edges_f32(name, edges) -> torch.Tensor:
    """the edges of one variable as a host float32 tensor, rounded once, checked after the rounding"""
    e = torch.as_tensor(edges)
    if e.is_cuda:
        raise ValueError(f"track_records: the edges of bins[{name!r}] must be host values (a sequence or a CPU tensor)")
    e = e.detach().reshape(-1).to(torch.float64).to(torch.float32)
    if not 2 <= e.numel() <= _lib.TR_MAX_BINS + 1:
        raise ValueError(f"track_records: bins[{name!r}] needs 2..{_lib.TR_MAX_BINS + 1} edges, got {e.numel()}")
    if not bool(torch.isfinite(e).all()):
        raise ValueError(f"track_records: the edges of bins[{name!r}] must be finite in float32")
    if not bool((e[1:] > e[:-1]).all()):
        raise ValueError(f"track_records: the edges of bins[{name!r}] must be strictly ascending in float32")
    return e


def track_records(bipartite_graph, event, bins=None, pt_cut=1., nhits_cut=5, majority_cut=0.5, primary=True):
    """``eval_metrics`` with what it folds away (``hgnn_track_records``, csrc/trackeval_records.hip): the metrics, a
    per-particle table, a per-candidate table and integer histograms of the particles over chosen variables, from
    one call and ONE host read (the same 12-double result vector).

    bins: ``{name: (values, edges)}``, at most four.  ``values`` is a per-hit device tensor or the name of an event
    field; a particle's value is the minimum over its hits in which a NaN wins, as its ``pt`` is.  ``edges``: 2..65
    finite, strictly ascending host numbers, rounded to float32 once.  Slot = number of edges <= value in float32
    (``numpy.searchsorted(edges, x, "right")``): 0 is the underflow, nb + 1 the overflow, where a NaN lands.

    Returns ``{"metrics": what eval_metrics returns, "counts": the integer HGNN_TE_N_* entries,
    "particles": {field: tensor[P]} in ascending pid (PARTICLE_FIELDS and ``values``, float32 [V, P]),
    "candidates": {field: tensor[C]} in ascending label (CANDIDATE_FIELDS),
    "bins": {name: {"edges": float32[nb + 1], "counts": int64[nb + 2, 6]}}}`` (columns: BIN_COLUMNS); every tensor
    is on the device."""
    # the host-side argument checks come first (they need no device), then the device refusals
    bins = {} if bins is None else dict(bins)
    V = len(bins)
    if V > _lib.TR_MAX_VARS:
        raise ValueError(f"track_records: at most {_lib.TR_MAX_VARS} binning variables, got {V}")
    n_hits = _field(event, "pid").numel()
    edges_host = torch.zeros((max(V, 1), _lib.TR_MAX_BINS + 1), dtype=torch.float32)
    n_bins = (ctypes.c_int32 * max(V, 1))()
    columns = []
    for v, (name, spec) in enumerate(bins.items()):
        try:
            values, edges = spec
        except (TypeError, ValueError):
            raise ValueError(f"track_records: bins[{name!r}] must be (values, edges)") from None
        if isinstance(values, str):
            values = _field(event, values)
        if not isinstance(values, torch.Tensor):
            raise ValueError(f"track_records: the values of bins[{name!r}] must be a tensor or an event field name")
        if values.numel() != n_hits:
            raise ValueError(f"track_records: the values of bins[{name!r}] must have one entry per hit "
                             f"({n_hits}), got {values.numel()}")
        e = _edges_f32(name, edges)
        edges_host[v, :e.numel()] = e
        n_bins[v] = e.numel() - 1
        columns.append(values)
    hit, cand, pid, pt, prim = _inputs("track_records", bipartite_graph, event, majority_cut, primary)
    if not all(x.is_cuda for x in columns):
        raise RuntimeError("track_records needs HIP device tensors: hierarchicalgnn_amd has no CPU path "
                           "(the values of a binning variable are on the host)")
    dev = bipartite_graph.device
    B, N = hit.numel(), pid.numel()
    vars_ = torch.stack([x.detach().reshape(-1).to(torch.float32) for x in columns]).contiguous() if V else None
    lib = _lib.load()
    ws, nb = _lib.workspace("hgnn_track_records_workspace_bytes", dev, B, N, V)
    result = torch.empty(_lib.TE_RESULT, dtype=torch.float64, device=dev)
    ptab = {k: torch.empty(N, dtype=dt, device=dev) for k, dt in PARTICLE_FIELDS}
    ptab["values"] = torch.empty((V, N), dtype=torch.float32, device=dev)
    ctab = {k: torch.empty(B, dtype=dt, device=dev) for k, dt in CANDIDATE_FIELDS}
    hist = torch.empty((V, _lib.TR_MAX_BINS + 2, _lib.TR_COLUMNS), dtype=torch.int64, device=dev)
    cp = _lib.HgnnTrParticles(**{k: _lib.ptr(t) for k, t in ptab.items()})
    cc = _lib.HgnnTrCandidates(**{k: _lib.ptr(t) for k, t in ctab.items()})
    with torch.cuda.device(dev):
        _lib.check(lib.hgnn_track_records(
            _lib.ptr(hit), _lib.ptr(cand), B, _lib.ptr(pid), _lib.ptr(pt), _lib.ptr(prim) if prim is not None else None,
            N, _lib.ptr(vars_), V, ctypes.cast(edges_host.data_ptr(), ctypes.POINTER(ctypes.c_float)), n_bins,
            float(pt_cut), float(nhits_cut), float(majority_cut), _lib.ptr(result), ctypes.byref(cp), ctypes.byref(cc),
            _lib.ptr(hist), _lib.ptr(ws), nb, _lib.current_stream(dev)), "hgnn_track_records")
        edges_dev = edges_host.pin_memory().to(dev, non_blocking=True) if V else None
    r = read_result(result)
    P, C = int(r[_lib.TE_N_PART]), int(r[_lib.TE_N_CAND])
    if r[_lib.TE_NO_MATCH] != 0:
        metrics = dict(default_response)
    else:
        metrics = {"track_eff": r[_lib.TE_TRACK_EFF], "track_pur": r[_lib.TE_TRACK_PUR],
                   "hit_eff": r[_lib.TE_HIT_EFF], "hit_pur": r[_lib.TE_HIT_PUR]}
    counts = {k: int(r[getattr(_lib, "TE_" + k.upper())]) for k in COUNT_KEYS}
    particles = {k: (t[:, :P] if k == "values" else t[:P]) for k, t in ptab.items()}
    candidates = {k: t[:C] for k, t in ctab.items()}
    out_bins = {}
    for v, name in enumerate(bins):
        n = int(n_bins[v])
        out_bins[name] = {"edges": edges_dev[v, :n + 1], "counts": hist[v, :n + 2]}
    return {"metrics": metrics, "counts": counts, "particles": particles, "candidates": candidates, "bins": out_bins}


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


def _cuts_f32(who, cuts) -> torch.Tensor:
    """the score cuts as a host float32 tensor, rounded once, checked after the rounding"""
    c = torch.as_tensor(cuts)
    if c.is_cuda:
        raise ValueError(f"{who}: cuts must be host values (a sequence or a CPU tensor)")
    c = c.detach().reshape(-1).to(torch.float64).to(torch.float32)
    if not 1 <= c.numel() <= _lib.TS_MAX_CUTS:
        raise ValueError(f"{who}: 1..{_lib.TS_MAX_CUTS} cuts expected, got {c.numel()}")
    if bool(torch.isnan(c).any()):
        raise ValueError(f"{who}: a cut is NaN")
    return c


def _item_bytes(who, t, name, n):
    if not torch.is_tensor(t) or t.dtype not in (torch.bool, torch.uint8) or t.numel() != n:
        raise ValueError(f"{who}: {name} must be bool or uint8 with one entry per item ({n})")
    return t.reshape(-1).contiguous().view(torch.uint8)


def _score_scan(who, mode, graph, scores, cuts, inverse_mask, event, pt_cut, nhits_cut, majority_cut, primary, truth,
                keep):
    # the host-side argument checks come first (they need no device), then the device refusals
    c = _cuts_f32(who, cuts)
    if not torch.is_tensor(graph) or graph.dim() != 2 or graph.shape[0] != 2:
        raise ValueError(f"{who}: a [2, n] graph expected, got {tuple(getattr(graph, 'shape', ()))}")
    n_items = int(graph.shape[1])
    if not torch.is_tensor(scores) or scores.numel() != n_items:
        raise ValueError(f"{who}: one score per item expected ({n_items})")
    if keep is not None and truth is None:
        raise ValueError(f"{who}: keep needs truth")
    truth8 = None if truth is None else _item_bytes(who, truth, "truth", n_items)
    keep8 = None if keep is None else _item_bytes(who, keep, "keep", n_items)
    if mode == _lib.TS_EDGE and inverse_mask is None:
        raise ValueError(f"{who}: inverse_mask is needed")
    if not scores.is_cuda:
        raise RuntimeError(f"{who} needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    a, b, pid, pt, prim = _inputs(who, graph, event, majority_cut, primary)
    dev = graph.device
    mask = None if inverse_mask is None else inverse_mask.reshape(-1).to(torch.int64).contiguous()
    others = [scores] + [t for t in (mask, truth8, keep8) if t is not None]
    if any(t.device != dev for t in others):
        raise RuntimeError(f"{who} needs HIP device tensors on one device: hierarchicalgnn_amd has no CPU path")
    scores = scores.detach().reshape(-1).float().contiguous()
    T, n_vertices, N = c.numel(), 0 if mask is None else mask.numel(), pid.numel()
    lib = _lib.load()
    ws, nb = _lib.workspace("hgnn_track_scan_workspace_bytes", dev, mode, n_items, n_vertices, N, T)
    result = torch.empty((T, _lib.TS_ROW), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        cuts_dev = c.pin_memory().to(dev, non_blocking=True)
        _lib.check(lib.hgnn_track_scan(mode, _lib.ptr(a), _lib.ptr(b), n_items, _lib.ptr(scores), _lib.ptr(cuts_dev),
                                       T, _lib.ptr(mask), n_vertices, _lib.ptr(truth8), _lib.ptr(keep8), _lib.ptr(pid),
                                       _lib.ptr(pt), _lib.ptr(prim) if prim is not None else None, N, float(pt_cut),
                                       float(nhits_cut), float(majority_cut), _lib.ptr(result), _lib.ptr(ws), nb,
                                       _lib.current_stream(dev)), "hgnn_track_scan")
    # the one host read of the scan, made as read_result makes it
    stats["host_reads"] += 1
    sync_mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode(0)
    try:
        host = result.cpu()
    finally:
        torch.cuda.set_sync_debug_mode(sync_mode)
    rows = host.tolist()
    if any(r[_lib.TE_STATUS] == 2 for r in rows):
        raise ValueError(f"{who}: a candidate label equals the reserved value {_lib.TS_RESERVED_LABEL}")
    if any(r[_lib.TE_STATUS] != 0 for r in rows):
        raise ValueError(f"{who}: a hit id (after inverse_mask) is outside [0, len(event.pid)), or a hit id is "
                         "outside inverse_mask")
    metrics = []
    for r in rows:
        if r[_lib.TE_NO_MATCH] != 0:
            metrics.append(dict(default_response))
        else:
            metrics.append({"track_eff": r[_lib.TE_TRACK_EFF], "track_pur": r[_lib.TE_TRACK_PUR],
                            "hit_eff": r[_lib.TE_HIT_EFF], "hit_pur": r[_lib.TE_HIT_PUR]})
    edges = None
    if truth8 is not None:
        edges = {"pass": [int(r[_lib.TS_N_PASS]) for r in rows],
                 "true_pass": [int(r[_lib.TS_N_TRUE_PASS]) for r in rows],
                 "true": [int(r[_lib.TS_N_TRUE]) for r in rows]}
    return {"cuts": c.tolist(), "metrics": metrics, "result": host[:, :_lib.TE_RESULT].clone(), "edges": edges}


def edge_score_scan(edge_index, scores, cuts, inverse_mask, event, pt_cut=1., nhits_cut=5, majority_cut=0.5,
                    primary=True, truth=None, keep=None):
    """``eval_metrics(edge_track_candidates(edge_index, scores, cut, inverse_mask), event, ...)`` for every ``cut`` of
    ``cuts`` (1..64 host numbers, any order, repeats allowed, rounded to float32 once, none NaN) from one call of
    ``hgnn_track_scan`` and ONE host read: the union-find is carried from the highest cut to the lowest, the
    particle side of the evaluation runs once.  ``truth`` / ``keep``: per-edge bool or uint8 device tensors.

    Returns ``{"cuts": the float32-rounded cuts as Python floats, "metrics": per cut what eval_metrics returns,
    "result": the host float64 [T, 12] block of HGNN_TE_* rows, "edges": {"pass", "true_pass", "true"} as int lists
    (#{keep, score >= cut}, #{keep, truth, score >= cut}, #{keep, truth}; keep None = all), or None without
    truth}``, every list in the caller's cut order."""
    return _score_scan("edge_score_scan", _lib.TS_EDGE, edge_index, scores, cuts, inverse_mask, event, pt_cut,
                       nhits_cut, majority_cut, primary, truth, keep)


def bipartite_score_scan(bipartite_graph, scores, cuts, inverse_mask, event, pt_cut=1., nhits_cut=5, majority_cut=0.5,
                         primary=True, truth=None, keep=None):
    """``eval_metrics(bipartite_track_candidates(bipartite_graph, scores, cut, inverse_mask), event, ...)`` for every
    ``cut`` of ``cuts``; arguments and return value as for ``edge_score_scan`` (``inverse_mask`` None: hit ids are
    taken as they are).  The candidate label 2^63 - 1 is reserved: a passing pair that carries it raises."""
    return _score_scan("bipartite_score_scan", _lib.TS_PAIR, bipartite_graph, scores, cuts, inverse_mask, event,
                       pt_cut, nhits_cut, majority_cut, primary, truth, keep)
