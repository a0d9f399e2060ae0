"""hierarchicalgnn_amd -- MI355X-native message-passing engine for the Exa.TrkX
hierarchical GNN (reference: clairesonglee/HierarchicalGNN).

Drop-in surface (same names / signatures as the reference):
    scatter_add(src, index, dim=0, dim_size=N)          <- torch_scatter.scatter_add
    scatter_min / scatter_max / scatter_mean / scatter   <- torch_scatter (same names)
    InteractionGNNCell(hparams), HierarchicalGNNCell(hparams)   <- Modules/gnn_utils.py
    make_mlp(...)                                        <- Modules/utils.py
    eval_metrics(bipartite_graph, event, ...)            <- Modules/tracking_utils.py
    track_records(bipartite_graph, event, bins, ...)     eval_metrics plus per-particle / per-candidate tables and
                                                         binned counts (no counterpart in the reference)
    edge_score_scan(...), bipartite_score_scan(...), ec_score_scan(...), bc_score_scan(...)
                                                         the tracking metrics at every score cut of a list in one
                                                         device call (the reference evaluates one hard-coded cut)
    graph_intersection(...), frnn_graph(...)             <- Modules/utils.py (embedding stage)
    training_samples(...), training_pairs(knn_idx, ...)  <- EmbeddingBase.get_training_samples (the second: from the kNN matrix)
    bipartite_loss(...), bc_training_loss(...)           <- BipartiteClassificationBase.get_bipartite_loss / training_step
    pair_hinge_loss(...), embedding_hgnn_training_loss(...)   <- EmbeddingBase.training_step's weighted hinge loss
    weighted_bce_loss(...), ec_training_loss(...), ec_shared_evaluation(...)   <- EdgeClassifierBase.training_step / shared_evaluation
    hdbscan(points, min_cluster_size), embedding_track_candidates(...)   <- cuml.cluster.HDBSCAN (embedding validation)
    FusedAdamW(params, lr, ...), configure_optimizers(...), optimizer_step(...)   <- Trainer(gradient_clip_val) + AdamW(amsgrad) of every base
    knn_edges(idx, n_pts, sym), attention_weights(src, dst, graph, bn, weighting, ...)   <- DynamicGraphConstruction's edge list and weights
    prepare_event_device(event, hparams), particle_hit_counts(pid), TrackMLDataset(..., device)   <- TrackMLDataset.__getitem__ (Modules/utils.py)

Everything on the hot path runs in hand-written HIP kernels loaded from
libhgnn_hip.so through the C ABI of include/hgnn_hip.h; there is no CPU or
eager fallback.
"""
from .ops import scatter_add, gather_scale_scatter, gather_rows, l1_row_scale  # noqa: F401
from .ops import scatter, scatter_max, scatter_mean, scatter_min  # noqa: F401
from .plan import GraphPlan, get_plan, clear_plan_cache, plan_cache_stats  # noqa: F401
from .utils import make_mlp  # noqa: F401
from .gnn_utils import InteractionGNNCell, HierarchicalGNNCell  # noqa: F401
from .tracking import eval_metrics, edge_track_candidates, bipartite_track_candidates  # noqa: F401
from .tracking import embedding_track_candidates, track_records  # noqa: F401
from .tracking import edge_score_scan, bipartite_score_scan  # noqa: F401
from .hdbscan import hdbscan, hdbscan_tree  # noqa: F401  (the name `hdbscan` is the function; the module is
#                                             importlib.import_module("hierarchicalgnn_amd.hdbscan"))
from .embedding import frnn_graph, graph_intersection, training_samples, training_weights, hinge_distance  # noqa: F401
from .embedding import training_pairs  # noqa: F401
from .embedding import (pair_hinge_loss, pair_hinge_check, embedding_hgnn_training_loss,  # noqa: F401
                        embedding_in_training_loss)
from .assignment import (max_weight_matching, bipartite_loss, bc_embedding_loss, bc_training_loss,  # noqa: F401
                         gap_bound, bc_score_scan)
from .edge_classifier import (weighted_bce_loss, weighted_bce_check, ec_training_loss,  # noqa: F401
                              ec_shared_evaluation, ec_score_scan)
from .optim import FusedAdamW, configure_optimizers, optimizer_step  # noqa: F401
from .ops import knn_edges  # noqa: F401
from .graph_construction import attention_weights  # noqa: F401
from .dataset import TrackMLDataset, prepare_event_device, particle_hit_counts  # noqa: F401

__version__ = "0.1.0"
