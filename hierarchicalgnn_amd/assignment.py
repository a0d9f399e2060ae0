"""The assignment loss of BC-HGNN-GMM and gMRT on the GPU (reference BipartiteClassification/
bipartite_classification_base.py:108-224; gmrt_base.py has the same methods).

Every training and validation step of the reference ends in ``get_bipartite_loss`` (:152-191): the B ~ N*k bipartite
scores go to the host, scipy builds a CSR matrix (summing the scores of each (particle, cluster) pair) and runs
``min_weight_full_bipartite_matching(maximize=True)``, and the matching comes back.  Here:

    max_weight_matching(row, col, score, n_rows, n_cols)   one hgnn_assign_match call (csrc/assign.hip): contraction
                                                           and an integer eps-scaled auction, all on the device
    gap_bound(n_rows, n_cols, w_max, grid_bits=None)       the documented bound on OPT - total(returned matching)
    bipartite_loss(bipartite_scores, bipartite_graph, batch, hparams)       get_bipartite_loss
    bc_embedding_loss(embeddings, edge_index, batch, hparams)               training_step :199-204
    bc_training_loss(bipartite_graph, bipartite_scores, embeddings, batch, hparams, loss_schedule)
                                                           training_step :196-213 after the forward
    bc_score_scan(bipartite_graph, bipartite_scores, batch, event, hparams, cuts)
                                                           the tracking metrics of shared_evaluation (:262-276) at every
                                                           score cut of a list: tracking.bipartite_score_scan

One stated difference from the reference: a pair's weight is the float64 sum of its float32 scores in position order
(scipy sums float32 in CSR order).  On scores that are multiples of 2^-12 both are exact and equal.  Weights that
quantise to 0 (below 2^-31) tie with the virtual column and which of them is matched is arbitrary.  pid 0 takes part
in the matching and is filtered afterwards, as in the reference.  ``batch.pt`` is not written.  There is no CPU path.

``stats``: ``host_reads`` of the LAST call of max_weight_matching / bipartite_loss (at most 64: the matching gives up
with a RuntimeError before it would read more than 48 times, the lines around it read 6 times), and the matching's
``phases``, ``grid_rounds``, ``tail_rounds`` and ``n_pairs``.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .embedding import _field, hinge_distance, pt_weighting, training_weights
from .ops import scatter_min

stats = {"host_reads": 0, "phases": 0, "grid_rounds": 0, "tail_rounds": 0, "n_pairs": 0}


def gap_bound(n_rows: int, n_cols: int, w_max: float, grid_bits=None) -> float:
    """G(P, C, w_max): an upper bound on OPT - total(returned matching), both totals in float64 over the contracted
    weights with HGNN_AM_FALLBACK_WEIGHT for every virtual column ("Assignment loss").  The
    auction is exact for the weights rint(w * 2^S), S = 30; a matching has at most min(P, C) real pairs, each off by
    at most 2^-(S+1) in either matching, and at most P virtual columns of weight 1e-12 < 2^-S that quantise to 0, so
    G = (P + C) * 2^-S.  ``grid_bits``: every score is a multiple of 2^-grid_bits; with grid_bits <= S the
    quantisation is exact and the bound on the total over the REAL pairs is 0.  Raises ValueError where the
    quantised weights would leave the range the kernel accepts (|rint(w * 2^S)| * (P + C + 1) <= 2^56)."""
    n = int(n_rows) + int(n_cols)
    if float(w_max) * 2.0 ** _lib.AM_SCALE_BITS * (n + 1) > 2.0 ** 56:
        raise ValueError(f"gap_bound: w_max {w_max} with {n} vertices exceeds the kernel's weight range")
    if grid_bits is not None and int(grid_bits) <= _lib.AM_SCALE_BITS:
        return 0.0
    return n * 2.0 ** -_lib.AM_SCALE_BITS


def _ids(t, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"max_weight_matching needs HIP device tensors ({name}): hierarchicalgnn_amd has no CPU path")
    if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"max_weight_matching: {name} must be a 1-D integer tensor")
    return t.to(torch.int64).contiguous()


def max_weight_matching(row, col, score, n_rows: int, n_cols: int):
    """(col_match int64 [n_rows], pair_row int64 [U], pair_col int64 [U], pair_weight float64 [U]), all on the device:
    the U distinct (row, col) pairs in row-major order with the float64 sum of their scores in position order, and a
    maximum-weight matching of them: ``col_match[r]`` is a real column of one of r's pairs, no column twice, or
    ``n_cols + r``, r's virtual column.  ValueError: empty input, an id out of range, a weight that is not finite or
    too large.  RuntimeError: CPU tensors, or the auction ran out of its round budget."""
    row, col = _ids(row, "row"), _ids(col, "col")
    if not torch.is_tensor(score) or not score.is_cuda:
        raise RuntimeError("max_weight_matching needs HIP device tensors (score): hierarchicalgnn_amd has no CPU path")
    score = score.detach().reshape(-1).float().contiguous()
    B, P, C = int(row.numel()), int(n_rows), int(n_cols)
    if B == 0 or P <= 0 or C <= 0:
        raise ValueError("max_weight_matching: empty bipartite graph")
    if col.numel() != B or score.numel() != B or col.device != row.device or score.device != row.device:
        raise ValueError("max_weight_matching: row, col and score need one entry per edge, on one device")
    dev = row.device
    lib = _lib.load()
    ws, nb = _lib.workspace("hgnn_assign_match_workspace_bytes", dev, B, P, C)
    col_match = torch.empty(P, dtype=torch.int64, device=dev)
    pair_row = torch.empty(B, dtype=torch.int64, device=dev)
    pair_col = torch.empty(B, dtype=torch.int64, device=dev)
    pair_w = torch.empty(B, dtype=torch.float64, device=dev)
    info = (ctypes.c_int64 * _lib.AM_INFO)()
    with torch.cuda.device(dev):
        _lib.check(lib.hgnn_assign_match(_lib.ptr(row), _lib.ptr(col), _lib.ptr(score), B, P, C, _lib.ptr(col_match),
                                         _lib.ptr(pair_row), _lib.ptr(pair_col), _lib.ptr(pair_w), info, _lib.ptr(ws),
                                         nb, _lib.current_stream(dev)), "hgnn_assign_match")
    stats.update(host_reads=int(info[_lib.AM_HOST_READS]), phases=int(info[_lib.AM_PHASES]),
                 grid_rounds=int(info[_lib.AM_GRID_ROUNDS]), tail_rounds=int(info[_lib.AM_TAIL_ROUNDS]),
                 n_pairs=int(info[_lib.AM_N_PAIRS]))
    status = int(info[_lib.AM_STATUS])
    if status & _lib.AM_ST_BAD_ID:
        raise ValueError(f"max_weight_matching: a row id is outside [0, {P}) or a col id outside [0, {C})")
    if status & _lib.AM_ST_BAD_WEIGHT:
        raise ValueError("max_weight_matching: a pair weight is not finite or too large for the int64 auction "
                         "(|w| * 2^30 * (n_rows + n_cols + 1) must stay below 2^56)")
    if status != 0:
        what = "a price left the int64 range" if status & _lib.AM_ST_OVERFLOW else "the round budget ran out"
        raise RuntimeError(f"max_weight_matching: {what} (status {status}, {stats['phases']} phases, "
                           f"{stats['tail_rounds']} tail rounds, {stats['host_reads']} host reads)")
    u = stats["n_pairs"]
    return col_match, pair_row[:u], pair_col[:u], pair_w[:u]


def _asgmt_weight(batch_pt, pt, bipartite_graph, n_cols, y_idx, not_y_idx, row_match, col_match, hparams):
    """get_asgmt_weight (:123-138); y_idx / not_y_idx are the positions weights[y] / weights[~y] select"""
    dev = bipartite_graph.device
    supernodes_pt = torch.zeros(n_cols, device=dev).float()
    supernodes_pt[col_match] = pt[row_match].float()
    weights = torch.maximum(pt_weighting(batch_pt[bipartite_graph[0]], hparams),
                            pt_weighting(supernodes_pt[bipartite_graph[1]], hparams))
    true_weights = weights[y_idx].sum()
    fake_weights = weights[not_y_idx].sum()
    lwr = hparams["log_weight_ratio"]
    weights[y_idx] = (weights[y_idx] / true_weights) * torch.sigmoid(lwr * torch.ones(1, device=dev))
    weights[not_y_idx] = (weights[not_y_idx] / fake_weights) * torch.sigmoid(-lwr * torch.ones(1, device=dev))
    return weights.float()


def _torch_tail(bipartite_scores, bipartite_graph, batch_pt, pt, original_pid, hit_row, col_match, n_cols, hparams,
                return_details):
    """everything of get_bipartite_loss after the matching as the reference writes it (:170-190): four ``nonzero()``
    host reads, get_asgmt_weight, binary_cross_entropy and the dot product"""
    dev = bipartite_scores.device
    n_rows = int(original_pid.numel())
    with torch.no_grad():
        row_match = torch.arange(n_rows, device=dev)
        noise_mask = (original_pid[row_match] != 0) & (col_match < n_cols)   # filter out noise and virtual tracks
        keep = noise_mask.nonzero().reshape(-1)                                               # read
        row_match, col_match = row_match[keep], col_match[keep]

        matched_particles = torch.zeros(n_rows, dtype=torch.bool, device=dev)
        matched_particles[row_match] = True
        matched_hits = matched_particles[hit_row].nonzero().reshape(-1)                       # read
        pid_assignments = torch.zeros(n_rows, device=dev).long()
        pid_assignments[row_match] = col_match
        truth = torch.zeros(len(bipartite_scores), dtype=torch.bool, device=dev)
        truth[matched_hits] = pid_assignments[hit_row[matched_hits]] == bipartite_graph[1][matched_hits]
        y_idx, not_y_idx = truth.nonzero().reshape(-1), (~truth).nonzero().reshape(-1)        # two reads
        stats["host_reads"] += 4
    weights = _asgmt_weight(batch_pt, pt, bipartite_graph, n_cols, y_idx, not_y_idx, row_match, col_match, hparams)
    asgmt_loss = torch.nn.functional.binary_cross_entropy(bipartite_scores, truth.float(), reduction="none")
    asgmt_loss = torch.dot(asgmt_loss, weights)   # weight by pT
    if return_details:
        return asgmt_loss, {"row_match": row_match, "col_match": col_match, "truth": truth, "weights": weights}
    return asgmt_loss


def _fused_tail(bipartite_scores, bipartite_graph, batch_pt, pt, original_pid, hit_row, col_match, n_cols, hparams,
                return_details):
    """everything of get_bipartite_loss after the matching without a host read: the truth and the supernodes' pt as
    elementwise index ops over the UNFILTERED matching, the loss as one ``weighted_bce_loss`` call (csrc/wbce.hip)"""
    from .edge_classifier import _wb_apply
    dev = bipartite_scores.device
    n_rows = int(original_pid.numel())
    with torch.no_grad():
        matched = (original_pid != 0) & (col_match < n_cols)            # filter out noise and virtual tracks
        cm = col_match[hit_row]
        truth = matched[hit_row] & (cm == bipartite_graph[1])
        # one scatter: a matched particle writes its pt to its column, every other one to its own virtual column
        # (col_match has no column twice, virtual ones included), and the virtual columns are sliced away
        slot = torch.where(matched, col_match, n_cols + torch.arange(n_rows, device=dev))
        supernodes_pt = torch.zeros(n_cols + n_rows, dtype=torch.float32, device=dev)
        supernodes_pt[slot] = pt.float()
        supernodes_pt = supernodes_pt[:n_cols]
    scores = bipartite_scores if bipartite_scores.dtype == torch.float32 else bipartite_scores.float()
    asgmt_loss, _, state = _wb_apply(scores.reshape(-1), bipartite_graph, truth, batch_pt.float(), hparams,
                                     supernodes_pt, "max", None)
    if not return_details:
        return asgmt_loss
    with torch.no_grad():
        keep = matched.nonzero().reshape(-1)                                                  # read
        stats["host_reads"] += 1
        raw = torch.maximum(pt_weighting(batch_pt[bipartite_graph[0]], hparams),
                            pt_weighting(supernodes_pt[bipartite_graph[1]], hparams))
        k = torch.where(truth, state[_lib.WB_KT], state[_lib.WB_KF])
        weights = (raw.double() * k).float()
    return asgmt_loss, {"row_match": keep, "col_match": col_match[keep], "truth": truth, "weights": weights}


def bipartite_loss(bipartite_scores, bipartite_graph, batch, hparams, return_details: bool = False,
                   fused: bool = False):
    """BipartiteClassificationBase.get_bipartite_loss / gMRTBase.get_bipartite_loss: the pT-weighted BCE between the
    scores and the truth a maximum-weight particle <-> cluster matching induces.  ``batch``: anything with ``pid``
    and ``pt`` (attributes or keys) on the scores' device; ``hparams``: weight_leak, ptcut, pt_interval, weight_min,
    log_weight_ratio.  The gradient reaches ``bipartite_scores`` through the BCE only.  With ``return_details`` also
    a dict of row_match, col_match (after the noise / virtual filter), truth and weights.  ``fused=True`` evaluates
    everything after ``max_weight_matching`` with no host read (four fewer than the default route): truth and the
    supernodes' pt by index ops, the weights, the BCE and the dot product as ``edge_classifier.weighted_bce_loss``
    (``combine="max"``); the weights are materialised only for ``return_details``, whose filter is then one read."""
    if not torch.is_tensor(bipartite_scores) or not bipartite_scores.is_cuda or not bipartite_graph.is_cuda:
        raise RuntimeError("bipartite_loss needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    if bipartite_graph.shape[1] == 0:
        raise ValueError("bipartite_loss: empty bipartite graph")
    batch_pid, batch_pt = _field(batch, "pid"), _field(batch, "pt")
    original_pid, pid, _ = torch.unique(batch_pid, return_inverse=True, return_counts=True)   # host read 1
    n_rows = int(original_pid.numel())
    pt = scatter_min(batch_pt, pid, dim=0, dim_size=n_rows)[0]
    with torch.no_grad():
        n_cols = int(bipartite_graph[1].max()) + 1                                            # host read 2
        hit_row = pid[bipartite_graph[0]]
        col_match = max_weight_matching(hit_row, bipartite_graph[1], bipartite_scores, n_rows, n_cols)[0]
        stats["host_reads"] += 2
    if fused:
        return _fused_tail(bipartite_scores, bipartite_graph, batch_pt, pt, original_pid, hit_row, col_match, n_cols,
                           hparams, return_details)
    return _torch_tail(bipartite_scores, bipartite_graph, batch_pt, pt, original_pid, hit_row, col_match, n_cols,
                       hparams, return_details)


def bc_embedding_loss(embeddings, edge_index, batch, hparams, fused=False):
    """the embedding loss of training_step (:199-204): PID truth on the input edges, get_emb_weight, get_hinge_distance
    and the squared hinge loss at margin 1 on dist / train_r, dotted with the weights.  ``fused=True`` evaluates the
    same quantity with ``embedding.pair_hinge_loss`` (one HIP operator, no host read, reproducible backward)."""
    if not torch.is_tensor(embeddings) or not embeddings.is_cuda or not edge_index.is_cuda:
        raise RuntimeError("bc_embedding_loss needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    batch_pid = _field(batch, "pid")
    y_pid = batch_pid[edge_index[0]] == batch_pid[edge_index[1]]
    if fused:
        from .embedding import pair_hinge_loss
        return pair_hinge_loss(embeddings, edge_index, y_pid, batch, hparams, margin=1.0,
                               scale=1.0 / hparams["train_r"], cache_plan=True)
    weights = training_weights(batch, edge_index, y_pid, hparams)
    hinge, dist = hinge_distance(embeddings, edge_index, y_pid)
    emb_loss = torch.nn.functional.hinge_embedding_loss(dist / hparams["train_r"], hinge, margin=1,
                                                        reduction="none").square()
    return torch.dot(emb_loss, weights)


def bc_training_loss(bipartite_graph, bipartite_scores, embeddings, batch, hparams, loss_schedule, fused=False):
    """training_step (:196-213) after the forward: (loss, emb_loss, asgmt_loss) with
    loss = loss_schedule * emb_loss + (1 - loss_schedule) * asgmt_loss.  ``batch`` also carries ``edge_index``.
    ``fused=True`` takes the fused route of both terms (``bc_embedding_loss``, ``bipartite_loss``)."""
    emb_loss = bc_embedding_loss(embeddings, _field(batch, "edge_index"), batch, hparams, fused=fused)
    asgmt_loss = bipartite_loss(bipartite_scores, bipartite_graph, batch, hparams, fused=fused)
    loss = (loss_schedule * emb_loss) + ((1 - loss_schedule) * asgmt_loss)
    return loss, emb_loss, asgmt_loss


def bc_score_scan(bipartite_graph, bipartite_scores, batch, event, hparams, cuts):
    """The tracking metrics of BC-HGNN-GMM's and gMRT's shared_evaluation (bipartite_classification_base.py:262-276,
    gmrt_base.py:269) at every score cut of ``cuts`` instead of at ``hparams["score_cut"]``
    (``tracking.bipartite_score_scan``: one device call, ONE host read).  ``batch`` carries ``inverse_mask``;
    ``event.pt`` is zeroed at ``pid == 0`` on a copy; ``hparams`` carries ptcut, n_hits and majority_cut."""
    from .tracking import bipartite_score_scan
    pid, pt = _field(event, "pid"), _field(event, "pt")
    ev = {"pid": pid, "pt": torch.where(pid == 0, torch.zeros_like(pt), pt)}
    return bipartite_score_scan(bipartite_graph, bipartite_scores, cuts, _field(batch, "inverse_mask"), ev,
                                pt_cut=hparams["ptcut"], nhits_cut=hparams["n_hits"],
                                majority_cut=hparams["majority_cut"], primary=False)
