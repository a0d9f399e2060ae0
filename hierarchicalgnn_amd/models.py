"""Model-level mirrors for the flat EC-IN model (BASELINE configs 1-2), so that the
``forward(x, edge_index)`` contract can be exercised end to end without the
reference's Lightning / PyG base classes (which are not needed for inference or
for a plain training loop).

    InteractionGNNBlock  <- EdgeClassifier/Models/IN.py:15-95
    EC_InteractionGNN    <- EdgeClassifier/Models/IN.py:97-128
    Embedding_InteractionGNN <- GNNEmbedding/Models/IN.py:99-118
    BC_MessagePassing    <- BipartiteClassification/Models/HGNN_GMM.py:300-346
    Embedding_HierarchicalGNN_GMM <- GNNEmbedding/Models/HGNN_GMM.py:278-301
    gMRT                 <- gMRT/Models/HGNN_GMM.py:276-356

Sub-module names (``ignn_block.node_encoder``, ``ignn_block.edge_encoder``,
``ignn_block.ignn_cells.{i}``, ``edge_classifier``) and therefore the
``state_dict`` keys are the reference's, so its checkpoints load with
``load_state_dict(ckpt["state_dict"])``.  In the reference these classes derive
from a LightningModule; to use the HIP cells inside the reference's own
training script, import-substitute ``gnn_utils`` instead.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .gnn_utils import InteractionGNNCell, _maybe_checkpoint
from .mlp import concat_mlp
from .plan import memo, stable_index
from .utils import make_mlp, match_dims, process_hparams


def _bf16_features(hparams) -> bool:
    """hparams["feature_dtype"] in ("bf16", "bfloat16"): an MI355X-side switch, absent = the reference's fp32"""
    return str(hparams.get("feature_dtype", "fp32")).lower() in ("bf16", "bfloat16")


def _mark_split3(module, hparams):
    """hparams["fp32_gemm"] (an MI355X-side key): "split_bf16" / "exact" pin this module's fp32 MLPs to the split-bf16
    evaluation of their GEMMs (fused.set_fp32_split3) or to the exact fp32 matrix instruction, whatever the
    process-wide default is; absent = the process-wide default (split-bf16, HGNN_FP32_SPLIT3=0 switches it off)"""
    mode = str(hparams.get("fp32_gemm", "")).lower()
    if mode in ("split_bf16", "split3", "exact", "fp32"):
        for m in module.modules():
            if isinstance(m, nn.Sequential):
                m._hgnn_split3 = mode in ("split_bf16", "split3")


def _head_input(t, hparams):
    """score heads in bf16 latent mode: from latent 256 on (hidden >= 512) the head runs as a chain of single-layer
    launches of the bf16 feature-split kernel on the bf16 rows; below that (no 256-wide single-layer instantiation)
    the rows are widened and the fused fp32 head kernel runs.  Either way no library MLP in an inference forward."""
    if t.dtype == torch.float32 or int(hparams["latent"]) >= 256:
        return t
    if torch.is_grad_enabled() and t.requires_grad:
        # training in bf16 mode: there is no differentiable fused head, so the head's wide GEMMs (1 TFLOP at
        # latent 256, E = 1M) would be fp32 library GEMMs; keep the rows in bf16 instead (library autocast)
        return t
    return t.float()


def _dst_sorted(graph):
    """(order, graph[:, order], inverse of order) for the stable sort of ``graph`` by destination"""
    order = torch.argsort(graph[1], stable=True)
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(order.numel(), device=order.device)
    return order, graph[:, order].contiguous(), inverse


class InteractionGNNBlock(nn.Module):
    def __init__(self, hparams, iterations, emb=True):
        super().__init__()
        hparams = process_hparams(hparams)
        act, ln = hparams["hidden_activation"], hparams["layernorm"]
        self.node_encoder = make_mlp(hparams["spatial_channels"], hparams["hidden"], hparams["latent"],
                                     hparams["nb_node_layer"], output_activation=act, hidden_activation=act,
                                     layer_norm=ln)
        self.edge_encoder = make_mlp(2 * hparams["spatial_channels"], hparams["hidden"], hparams["latent"],
                                     hparams["nb_edge_layer"], layer_norm=ln, output_activation=act,
                                     hidden_activation=act)
        if hparams["share_weight"]:                      # IN.py:51-56: one cell object reused
            cell = InteractionGNNCell(hparams)
            cells = [cell for _ in range(iterations)]
        else:
            cells = [InteractionGNNCell(hparams) for _ in range(iterations)]
        self.ignn_cells = nn.ModuleList(cells)
        if emb:
            self.output_layer = make_mlp(hparams["latent"], hparams["hidden"], hparams["emb_dim"],
                                         hparams["output_layers"], layer_norm=ln, output_activation=None,
                                         hidden_activation=hparams["hidden_output_activation"])
        self.emb = emb
        self.hparams = hparams
        self._ckpt = bool(hparams.get("checkpointing", True))
        _mark_split3(self, hparams)

    def _encode_nodes(self, x):
        return concat_mlp(self.node_encoder, [(x, None)], bf16_tail=_bf16_features(self.hparams))

    def _encode_edges(self, x, graph):
        return concat_mlp(self.edge_encoder, [(x, graph[0]), (x, graph[1])], bf16_tail=_bf16_features(self.hparams))

    def run(self, x, graph, restore_order=True):
        """The block on the destination-sorted layout.  Returns (emb or None, nodes, edges, graph_used,
        order): with ``restore_order`` the edges/graph come back in the caller's order (order=None);
        without it they stay destination-sorted and ``order`` maps sorted position -> original column
        (a caller that only needs node-level outputs, like the BC model, never pays the un-permute)."""
        if torch.is_grad_enabled() and x.is_leaf and not x.requires_grad:
            x.requires_grad = True                       # IN.py:82 (reentrant checkpoint needs a grad input)
        # MI355X layout choice, invisible through the interface: run the whole block on the
        # destination-sorted edge order.  The per-cell aggregation (gnn_utils.py:50) then reads
        # each node's incoming edge rows as ONE contiguous HBM stream instead of gathering 1-KiB
        # rows by edge id; the original order (which IN.py:126 relies on) is restored once at the end.
        order = None
        graph = stable_index(graph)
        graph_in = graph
        if self.hparams.get("sort_edges", True) and graph.is_cuda and graph.shape[1] > 0:
            order, graph, inverse = memo(graph, "dst_sorted", lambda g=graph: _dst_sorted(g))
        nodes = _maybe_checkpoint(self._ckpt, self._encode_nodes, x)              # IN.py:84
        edges = _maybe_checkpoint(self._ckpt, self._encode_edges, x, graph)       # IN.py:85
        if _bf16_features(self.hparams):
            # BASELINE config 4: latent rows in bf16 (fp32 master weights, fp32 accumulation and
            # LayerNorm inside the kernels); encoders, embeddings and heads stay fp32
            nodes, edges = nodes.bfloat16(), edges.bfloat16()
        for cell in self.ignn_cells:                                              # IN.py:87-88
            nodes, edges = cell(nodes, edges, graph)
        if order is not None and restore_order:
            from .ops import gather_rows
            edges = gather_rows(edges, inverse)
            graph, order = graph_in, None
        emb = None
        if self.emb:
            # HGNN_GMM.py:96-97: embedding head (plain emb_dim-wide last layer) on the fused kernel
            emb = nn.functional.normalize(concat_mlp(self.output_layer, [(nodes.float(), None)]))
        return emb, nodes, edges, graph, order

    def forward(self, x, graph):
        emb, nodes, edges, _, _ = self.run(x, graph, restore_order=True)
        if self.emb:
            return emb, nodes, edges
        return nodes, edges


class EC_InteractionGNN(nn.Module):
    """flat interaction-network edge classifier: forward(x[N,3], graph[2,E]) -> scores[E]"""

    def __init__(self, hparams):
        super().__init__()
        hparams = process_hparams(hparams)
        self.hparams = hparams
        self.ignn_block = InteractionGNNBlock(hparams, hparams["n_interaction_graph_iters"], emb=False)
        self.edge_classifier = make_mlp(2 * hparams["latent"], hparams["hidden"], 1, hparams["output_layers"],
                                        layer_norm=hparams["layernorm"], output_activation=None,
                                        hidden_activation=hparams["hidden_output_activation"])
        _mark_split3(self, hparams)

    def forward(self, x, graph):
        graph = stable_index(graph)
        directed_graph = memo(graph, "directed", lambda: torch.cat([graph, graph.flip(0)], dim=1))  # IN.py:122
        nodes, edges = self.ignn_block(x, directed_graph)
        edges = _head_input(edges, self.hparams)
        e = graph.shape[1]
        # IN.py:126 -- relies on the ORIGINAL edge order: edges[:E] pairs with edges[E:]
        scores = concat_mlp(self.edge_classifier, [(edges[:e], None), (edges[e:], None)]).squeeze(-1)
        return torch.sigmoid(scores.float())


class Embedding_InteractionGNN(nn.Module):
    """GNNEmbedding/Models/IN.py:99-118 without its Lightning base: forward(x[N,3], graph[2,E]) -> unit
    embeddings[N, emb_dim] of the doubled graph.  The pair construction of its training step is
    hierarchicalgnn_amd.embedding."""

    def __init__(self, hparams):
        super().__init__()
        hparams = process_hparams(hparams)
        self.hparams = hparams
        self.ignn_block = InteractionGNNBlock(hparams, hparams["n_interaction_graph_iters"], emb=True)
        _mark_split3(self, hparams)

    def forward(self, x, graph):
        graph = stable_index(graph)
        directed_graph = memo(graph, "directed", lambda: torch.cat([graph, graph.flip(0)], dim=1))  # IN.py:114
        embeddings, _, _ = self.ignn_block(x, directed_graph)
        return embeddings


class HierarchicalGNNBlock(nn.Module):
    """Message-passing part of BipartiteClassification/Models/HGNN_GMM.py:101-298.

    The reference's block first decides the hierarchy (GMM cut, connected components,
    kNN graphs: HGNN_GMM.py:244-260 -- host-side sklearn/scipy/cugraph/frnn calls, SURVEY
    section 8f "next" rows) and then runs the arithmetic mirrored here on the result:
    K5 pooling (:269), supernode / superedge encoders (:270-271) and the
    HierarchicalGNNCell loop (:275-284).  ``forward`` therefore takes the hierarchy
    (centroids ``means``, bipartite and super graphs with their weights) as inputs.
    Sub-module names match the reference, so its ``hgnn_block.*`` weights load
    (the graph-construction buffers it also holds are simply not used here).

    The embedding stage's block (GNNEmbedding/Models/HGNN_GMM.py:99-276) is the same block with two switches:
    ``l1_pool=False`` pools the node rows as they are (:256, no L1 row normalisation) and ``emb_head=True`` gives the
    block the ``output_layer`` (:149-157) whose normalised output is the model's final embedding (``embed_head``).
    """

    def __init__(self, hparams, l1_pool=True, emb_head=False):
        super().__init__()
        from .gnn_utils import HierarchicalGNNCell
        hparams = process_hparams(hparams)
        act, ln = hparams["hidden_activation"], hparams["layernorm"]
        self.supernode_encoder = make_mlp(hparams["latent"], hparams["hidden"],
                                          hparams["latent"] - hparams["emb_dim"], hparams["nb_node_layer"],
                                          output_activation=act, hidden_activation=act, layer_norm=ln)
        self.superedge_encoder = make_mlp(2 * hparams["latent"], hparams["hidden"], hparams["latent"],
                                          hparams["nb_edge_layer"], layer_norm=ln, output_activation=act,
                                          hidden_activation=act)
        n = hparams["n_hierarchical_graph_iters"]
        if hparams["share_weight"]:
            cell = HierarchicalGNNCell(hparams)
            cells = [cell for _ in range(n)]
        else:
            cells = [HierarchicalGNNCell(hparams) for _ in range(n)]
        self.hgnn_cells = nn.ModuleList(cells)
        if emb_head:
            self.output_layer = make_mlp(hparams["latent"], hparams["hidden"], hparams["emb_dim"],
                                         hparams["output_layers"], layer_norm=ln, output_activation=None,
                                         hidden_activation=hparams["hidden_output_activation"])
        self.l1_pool, self.emb_head = bool(l1_pool), bool(emb_head)
        # same names / buffers as the reference block (HGNN_GMM.py:155-157) so that its
        # state_dict loads strictly; `score_cut` belongs to the (host-side) GMM edge cut
        from .graph_construction import DynamicGraphConstruction
        self.super_graph_construction = DynamicGraphConstruction("sigmoid", hparams)
        self.bipartite_graph_construction = DynamicGraphConstruction("exp", hparams)
        self.register_buffer("score_cut", torch.tensor([float("inf")]))
        self.hparams = hparams
        self._ckpt = bool(hparams.get("checkpointing", True))
        _mark_split3(self, hparams)

    def clustering(self, embeddings, graph, return_count=False):
        """HGNN_GMM.py:184-234 on the GPU (clustering.py): cluster id per hit, -1 = unclustered"""
        from .clustering import gmm_edge_clustering
        return gmm_edge_clustering(embeddings, graph, self.score_cut, self.hparams, self.training,
                                   return_count=return_count)

    def hierarchy_from_clusters(self, embeddings, clusters, n_clusters=None, graphs=None):
        """HGNN_GMM.py:251-260 given the cluster label of every hit (-1 = unclustered): centroids
        (scatter_mean, K8), L2-normalise, kNN super graph (symmetrised, sigmoid weights) and
        bipartite graph (exp weights), both mean-normalised.  ``n_clusters`` (known from the clustering
        step's single host read) avoids a second read of ``clusters.max()``."""
        from .ops import scatter_add
        if n_clusters is None:
            n_clusters = int(clusters.max().item()) + 1
        # unclustered hits (-1) are summed into a dummy row that is dropped: no data-dependent compaction
        lab = torch.where(clusters >= 0, clusters, torch.full_like(clusters, n_clusters)).contiguous()
        sums = scatter_add(embeddings, lab, dim=0, dim_size=n_clusters + 1, validate=False)[:n_clusters]
        counts = scatter_add(torch.ones(embeddings.shape[0], 1, device=embeddings.device), lab, dim=0,
                             dim_size=n_clusters + 1, validate=False)[:n_clusters].clamp_(min=1)
        means = nn.functional.normalize(sums / counts)
        if graphs is not None:
            # a caller-supplied topology (bipartite_graph, super_graph): only the differentiable attention
            # weights are evaluated on it (gnn_utils.py:208-216)
            bip_graph, super_graph = graphs
            super_w = self.super_graph_construction.edge_weights(means, means, super_graph, norm=True)
            bip_w, bip_logits = self.bipartite_graph_construction.edge_weights(embeddings, means, bip_graph, norm=True,
                                                                              logits=True)
            return means, bip_graph, bip_w, super_graph, super_w, bip_logits
        super_graph, super_w = self.super_graph_construction(
            means, means, sym=True, norm=True, k=self.hparams["supergraph_sparsity"])
        bip_graph, bip_w, bip_logits = self.bipartite_graph_construction(
            embeddings, means, sym=False, norm=True, k=self.hparams["bipartitegraph_sparsity"], logits=True)
        return means, bip_graph, bip_w, super_graph, super_w, bip_logits

    def _encode_supernodes(self, pooled):
        return concat_mlp(self.supernode_encoder, [(pooled, None)])

    def _encode_superedges(self, supernodes, super_graph):
        return concat_mlp(self.superedge_encoder, [(supernodes, super_graph[0]), (supernodes, super_graph[1])])

    def forward(self, nodes, edges, graph, means, bipartite_graph, bipartite_edge_weights, super_graph,
                super_edge_weights):
        from .ops import gather_scale_scatter, l1_row_scale
        graph, bipartite_graph, super_graph = (stable_index(g) for g in (graph, bipartite_graph, super_graph))
        # HGNN_GMM.py:269 -- L1-normalised rows, weighted, summed per supernode (K5, one fused kernel); the embedding
        # stage's block pools the rows as they are (GNNEmbedding/Models/HGNN_GMM.py:256)
        pooled = gather_scale_scatter(nodes, bipartite_graph[0], bipartite_graph[1], means.shape[0],
                                      bipartite_edge_weights, row_scale=l1_row_scale(nodes) if self.l1_pool else None)
        supernodes = torch.cat([means.to(nodes.dtype),
                                _maybe_checkpoint(self._ckpt, self._encode_supernodes, pooled)], dim=-1)
        superedges = _maybe_checkpoint(self._ckpt, self._encode_superedges, supernodes, super_graph)
        for cell in self.hgnn_cells:                                              # HGNN_GMM.py:275-284
            nodes, edges, supernodes, superedges = cell(nodes, edges, supernodes, superedges, graph,
                                                        bipartite_graph, bipartite_edge_weights,
                                                        super_graph, super_edge_weights)
        return nodes, supernodes, edges, superedges

    def embed_head(self, nodes):
        """GNNEmbedding/Models/HGNN_GMM.py:273-274: the final unit embeddings from the block's node rows"""
        return nn.functional.normalize(concat_mlp(self.output_layer, [(nodes.float(), None)]))

    def decide(self, embeddings, directed_graph, hierarchy=None):
        """(clusters, means, bipartite graph, its weights, super graph, its weights): the GPU hierarchy decision, or
        -- ``hierarchy`` = (clusters, bipartite_graph, super_graph) -- a caller's topology with only the differentiable
        attention weights evaluated on it"""
        if hierarchy is None:
            clusters, n_clusters = self.clustering(embeddings, directed_graph, return_count=True)
            means, bg, bw, sg, sw, _ = self.hierarchy_from_clusters(embeddings, clusters, n_clusters)
        else:
            clusters, bg, sg = hierarchy
            means, bg, bw, sg, sw, _ = self.hierarchy_from_clusters(embeddings, clusters, graphs=(bg, sg))
        return clusters, means, bg, bw, sg, sw


class BC_MessagePassing(nn.Module):
    """BC_HierarchicalGNN_GMM (HGNN_GMM.py:300-346) without its Lightning base: IGNN block ->
    hierarchy decision (GPU clustering + kNN graphs) -> HGNN block -> bipartite head.  ``forward``
    runs all of it; ``embed`` / ``hgnn_block(...)`` / ``score`` expose the stages so that a caller
    can also supply its own hierarchy."""

    def __init__(self, hparams):
        super().__init__()
        hparams = process_hparams(hparams)
        self.hparams = hparams
        self.ignn_block = InteractionGNNBlock(hparams, hparams["n_interaction_graph_iters"], emb=True)
        self.hgnn_block = HierarchicalGNNBlock(hparams)
        self.bipartite_output_layer = make_mlp(2 * hparams["latent"], hparams["hidden"], 1,
                                               hparams["output_layers"], layer_norm=hparams["layernorm"],
                                               output_activation=None,
                                               hidden_activation=hparams["hidden_output_activation"])
        _mark_split3(self, hparams)

    def embed(self, x, graph, restore_order=False):
        """HGNN_GMM.py:328-331: returns (directed_graph, embeddings[N,emb_dim], nodes, edges, order).
        By default the directed graph and the edge latents stay in the destination-sorted layout
        (``order`` = sorted position -> column of cat([graph, graph.flip(0)])): the BC model only
        returns node-level quantities, so the HGNN block keeps streaming on that layout and the
        un-permute is never paid."""
        graph = stable_index(graph)
        directed_graph = memo(graph, "directed", lambda: torch.cat([graph, graph.flip(0)], dim=1))
        emb, nodes, edges, directed_graph, order = self.ignn_block.run(x, directed_graph, restore_order)
        return directed_graph, emb, nodes, edges, order

    def forward(self, x, graph):
        """HGNN_GMM.py:323-346: returns (bipartite_graph[2,B], bipartite_scores[B], embeddings[N,emb_dim])"""
        directed, emb, nodes, edges, _ = self.embed(x, graph)
        clusters, n_clusters = self.hgnn_block.clustering(emb, directed, return_count=True)
        means, bg, bw, sg, sw, _ = self.hgnn_block.hierarchy_from_clusters(emb, clusters, n_clusters)
        nodes, supernodes, _, _ = self.hgnn_block(nodes, edges, directed, means, bg, bw, sg, sw)
        return bg, self.score(nodes, supernodes, bg), emb

    def score(self, nodes, supernodes, bipartite_graph):
        """HGNN_GMM.py:342-344"""
        s = concat_mlp(self.bipartite_output_layer,
                       [(_head_input(nodes, self.hparams), bipartite_graph[0]),
                        (_head_input(supernodes, self.hparams), bipartite_graph[1])]).squeeze(-1)
        return torch.sigmoid(s.float())


class Embedding_HierarchicalGNN_GMM(nn.Module):
    """GNNEmbedding/Models/HGNN_GMM.py:278-301 without its Lightning base: IGNN block (intermediate embeddings) ->
    hierarchy decision on them -> HGNN block without the L1 pooling normalisation -> the block's own embedding head.
    ``forward(x, graph)`` returns (embeddings, intermediate_embeddings, clusters).  Runs on the destination-sorted
    layout without the un-permute, as BC_MessagePassing does.  The training step's loss is
    ``embedding.embedding_hgnn_training_loss``."""

    def __init__(self, hparams):
        super().__init__()
        hparams = process_hparams(hparams)
        self.hparams = hparams
        self.ignn_block = InteractionGNNBlock(hparams, hparams["n_interaction_graph_iters"], emb=True)
        self.hgnn_block = HierarchicalGNNBlock(hparams, l1_pool=False, emb_head=True)
        _mark_split3(self, hparams)

    def forward(self, x, graph, hierarchy=None):
        """``hierarchy`` = (clusters, bipartite_graph, super_graph) replaces the GPU hierarchy decision"""
        graph = stable_index(graph)
        directed_graph = memo(graph, "directed", lambda: torch.cat([graph, graph.flip(0)], dim=1))   # :295
        intermediate, nodes, edges, directed_graph, _ = self.ignn_block.run(x, directed_graph, restore_order=False)
        clusters, means, bg, bw, sg, sw = self.hgnn_block.decide(intermediate, directed_graph, hierarchy)
        nodes, _, _, _ = self.hgnn_block(nodes, edges, directed_graph, means, bg, bw, sg, sw)
        return self.hgnn_block.embed_head(nodes), intermediate, clusters


class gMRT(nn.Module):
    """gMRT/Models/HGNN_GMM.py:276-356 without its Lightning base: one-layer ``match_dims`` encoders and embedding
    head instead of an IGNN block, then the BC-style HGNN block (L1 pooling, :243-250) and the bipartite head.
    ``forward(x, graph)`` returns (bipartite_graph, bipartite_scores, embeddings); the training loss is
    ``assignment.bc_training_loss``.  The config keys ``data_dir`` / ``super_dir`` (the reference's supergraph dump
    directories) are accepted and ignored."""

    def __init__(self, hparams):
        super().__init__()
        hparams = process_hparams(hparams)
        self.hparams = hparams
        act, ln = hparams["hidden_activation"], hparams["layernorm"]
        self.node_encoder = match_dims(hparams["spatial_channels"], hparams["latent"], layer_norm=ln,
                                       output_activation=act)
        self.edge_encoder = match_dims(2 * hparams["spatial_channels"], hparams["latent"], layer_norm=ln,
                                       output_activation=act)
        self.output_layer = match_dims(hparams["latent"], hparams["emb_dim"], layer_norm=ln, output_activation=None)
        self.hgnn_block = HierarchicalGNNBlock(hparams)
        self.bipartite_output_layer = make_mlp(2 * hparams["latent"], hparams["hidden"], 1,
                                               hparams["output_layers"], layer_norm=ln, output_activation=None,
                                               hidden_activation=hparams["hidden_output_activation"])
        self._ckpt = bool(hparams.get("checkpointing", True))
        _mark_split3(self, hparams)

    def _encode_nodes(self, x):
        return concat_mlp(self.node_encoder, [(x, None)], bf16_tail=_bf16_features(self.hparams))

    def _encode_edges(self, x, graph):
        return concat_mlp(self.edge_encoder, [(x, graph[0]), (x, graph[1])], bf16_tail=_bf16_features(self.hparams))

    def embed(self, x, graph):
        """:339-344: (directed_graph, embeddings, nodes, edges) on the destination-sorted layout.  Like the reference
        (:337) and ``InteractionGNNBlock.run`` it sets ``requires_grad`` on the CALLER's leaf ``x`` when autograd
        records (the reentrant checkpoints need an input with a gradient): the caller's tensor is changed, and the
        backward computes a gradient for ``x`` that a training step never uses."""
        if torch.is_grad_enabled() and x.is_leaf and not x.requires_grad:
            x.requires_grad = True                                                               # :337
        graph = stable_index(graph)
        directed_graph = memo(graph, "directed", lambda: torch.cat([graph, graph.flip(0)], dim=1))
        if self.hparams.get("sort_edges", True) and directed_graph.is_cuda and directed_graph.shape[1] > 0:
            _, directed_graph, _ = memo(directed_graph, "dst_sorted", lambda g=directed_graph: _dst_sorted(g))
        nodes = _maybe_checkpoint(self._ckpt, self._encode_nodes, x)
        edges = _maybe_checkpoint(self._ckpt, self._encode_edges, x, directed_graph)
        emb = nn.functional.normalize(concat_mlp(self.output_layer, [(nodes.float(), None)]))
        if _bf16_features(self.hparams):
            nodes, edges = nodes.bfloat16(), edges.bfloat16()
        return directed_graph, emb, nodes, edges

    def forward(self, x, graph, hierarchy=None):
        """``hierarchy`` = (clusters, bipartite_graph, super_graph) replaces the GPU hierarchy decision"""
        directed_graph, emb, nodes, edges = self.embed(x, graph)
        _, means, bg, bw, sg, sw = self.hgnn_block.decide(emb, directed_graph, hierarchy)
        nodes, supernodes, _, _ = self.hgnn_block(nodes, edges, directed_graph, means, bg, bw, sg, sw)
        return bg, self.score(nodes, supernodes, bg), emb

    score = BC_MessagePassing.score


class GraphedInference:
    """Replay a model's no-grad ``forward(x, edge_index)`` from a captured HIP graph.

    Small events are launch-bound (a 2k-hit event is ~100 kernels of a few microseconds each behind
    Python / ctypes dispatch); the C ABI allocates nothing and never synchronises, so the whole
    forward is capturable once its per-event plans exist.  Usage:

        g = GraphedInference(model, x, edge_index)   # eager warm-up (builds the plans), then capture
        scores = g(x_new)                            # same topology, new hit features: replay

    The topology (``edge_index``) is baked in: a new event needs a new capture (or the eager path).
    Each call returns a fresh copy of the captured output buffer (a replay overwrites the buffer; pass
    ``clone=False`` to get the aliased buffer itself and save the copy).
    """

    def __init__(self, model, x, edge_index, warmup: int = 2):
        self.model = model
        self.x = x.clone()
        self.edge_index = stable_index(edge_index)      # an inference-tensor graph would be re-cloned (and re-planned) per call
        stream = torch.cuda.Stream(x.device)
        stream.wait_stream(torch.cuda.current_stream(x.device))
        with torch.no_grad(), torch.cuda.stream(stream):
            for _ in range(warmup):
                model(self.x, self.edge_index)
        torch.cuda.current_stream(x.device).wait_stream(stream)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.out = model(self.x, self.edge_index)

    def __call__(self, x=None, clone: bool = True):
        if x is not None:
            self.x.copy_(x)
        self.graph.replay()
        if not clone:
            return self.out
        if torch.is_tensor(self.out):
            return self.out.clone()
        return tuple(o.clone() if torch.is_tensor(o) else o for o in self.out)
