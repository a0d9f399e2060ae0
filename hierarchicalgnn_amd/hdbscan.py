"""Deterministic HDBSCAN* on the GPU: the clustering call of the embedding stage's validation step (reference
GNNEmbedding/embedding_base.py:40-41,267-272, ``cuml.cluster.HDBSCAN(min_cluster_size, metric='euclidean',
cluster_selection_method='eom')``; cuml does not exist on ROCm).

    hdbscan(points, min_cluster_size=5, min_samples=None) -> labels
    hdbscan_tree(points, min_cluster_size=5, min_samples=None) -> (labels, mst_edges, mst_w2, core2)

One ``hgnn_hdbscan_f32`` call (csrc/hdbscan.hip): exact core distances, the minimum spanning tree of the
mutual-reachability graph by Boruvka rounds of a tiled all-pairs kernel, a device sort, and the sequential tree stage
(multi-way dendrogram, condensed tree, EOM) as host code inside the library.  The definition (DESIGN.md section 3,
"HDBSCAN") breaks no tie by arrival order, so -- unlike sklearn, the hdbscan package and cuml -- the partition does
not depend on the order of the points.  Fixed: Euclidean metric, EOM, alpha = 1, cluster_selection_epsilon = 0, no
single-cluster result.

The call synchronises: one host read per Boruvka round plus the two copies around the tree stage, counted in
``stats["host_reads"]`` (<= 24 per call).  ``stats["last"]`` holds the last call's rounds and per-stage times.
There is no CPU path: ``points`` must be a HIP device tensor.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib

stats = {"host_reads": 0, "calls": 0, "last": {}}

MAX_DIM, MAX_MIN_SAMPLES = 16, 128


def hdbscan_tree(points: torch.Tensor, min_cluster_size: int = 5, min_samples=None, stage_sync: bool = False):
    """(labels int64 [N], mst_edges int64 [N-1, 2] (min id first), mst_w2 float32 [N-1], core2 float32 [N]), all on
    the device; the edges are sorted by (w2, min, max).  ``stage_sync`` adds two stream synchronisations so that
    ``stats["last"]`` times the core-distance and sort stages on their own (measurement only)."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise RuntimeError("hdbscan needs a HIP device tensor: hierarchicalgnn_amd has no CPU path")
    if points.dim() != 2 or points.dtype != torch.float32:
        raise ValueError(f"hdbscan: points must be float32 [N, D], got {points.dtype} {tuple(points.shape)}")
    n, d = int(points.shape[0]), int(points.shape[1])
    mcs = int(min_cluster_size)
    ms = mcs if min_samples is None else int(min_samples)
    dev = points.device
    x = points.detach().contiguous()
    lib = _lib.load()
    ws, nb = _lib.workspace("hgnn_hdbscan_workspace_bytes", dev, n, d, mcs, ms)
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    edges = torch.empty((n - 1, 2), dtype=torch.int64, device=dev)
    w2 = torch.empty(n - 1, dtype=torch.float32, device=dev)
    core2 = torch.empty(n, dtype=torch.float32, device=dev)
    info = (ctypes.c_int64 * _lib.HDB_INFO)()
    info[_lib.HDB_STAGE_SYNC] = 1 if stage_sync else 0
    with torch.cuda.device(dev):
        _lib.check(lib.hgnn_hdbscan_f32(_lib.ptr(x), n, d, mcs, ms, _lib.ptr(labels), _lib.ptr(edges), _lib.ptr(w2),
                                        _lib.ptr(core2), info, _lib.ptr(ws), nb,
                                        _lib.current_stream(dev)), "hgnn_hdbscan_f32")
    rounds = int(info[_lib.HDB_ROUNDS])
    stats["calls"] += 1
    stats["host_reads"] += int(info[_lib.HDB_HOST_READS])
    stats["last"] = {
        "n": n, "rounds": rounds, "host_reads": int(info[_lib.HDB_HOST_READS]),
        "n_clusters": int(info[_lib.HDB_N_CLUSTERS]), "stage_sync": bool(stage_sync),
        "core_ms": info[_lib.HDB_T_CORE_NS] * 1e-6,
        "round_ms": [info[_lib.HDB_T_ROUND0_NS + r] * 1e-6 for r in range(rounds)],
        "sort_ms": info[_lib.HDB_T_SORT_NS] * 1e-6, "tree_ms": info[_lib.HDB_T_TREE_NS] * 1e-6,
    }
    return labels, edges, w2, core2


def hdbscan(points: torch.Tensor, min_cluster_size: int = 5, min_samples=None) -> torch.Tensor:
    """int64 [N] device labels: -1 is noise, clusters are numbered 0..C-1 by smallest member index."""
    return hdbscan_tree(points, min_cluster_size, min_samples)[0]
