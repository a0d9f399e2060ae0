"""The edge classifier's training and validation step on the GPU (reference EdgeClassifier/edge_classifier_base.py).

``EdgeClassifierBase.training_step`` (:113-132) and ``shared_evaluation`` (:135-191) end in the pT-weighted binary
cross-entropy: ``get_training_weight`` (:99-111, boolean indexing and a dozen elementwise kernels),
``binary_cross_entropy(reduction="none")`` and ``torch.dot``.  The assignment loss of BC-HGNN-GMM / gMRT ends in the
same arithmetic with the max of the two endpoint weights and a second pT table.  Here:

    weighted_bce_loss(scores, graph, y, pt_a, hparams, pt_b=None, combine="sum", keep=None, check=False)
                                                     the weights, the BCE and the dot product as ONE operator,
                                                     csrc/wbce.hip: no [P] weight vector, no host read, bitwise
                                                     reproducible forward and backward
    weighted_bce_check(device=None)                  reads the status words of the calls made since the last check
    ec_training_loss(scores, batch, hparams)         training_step after the forward (:115-128), both true_edges modes
    ec_shared_evaluation(scores, batch, event, hparams)
                                                     shared_evaluation after the forward: (bipartite_graph, loss,
                                                     metrics) with tracking.edge_track_candidates and eval_metrics
    ec_score_scan(scores, batch, event, hparams, cuts)
                                                     the metrics of shared_evaluation at every score cut of a list, and
                                                     the edge counts per cut: tracking.edge_score_scan

One stated difference from the reference: a class of pairs without weight (an empty class in particular) contributes
nothing where the reference's 0/0 makes the loss NaN.  There is no CPU path: inputs must be HIP device tensors.
"""
from __future__ import annotations

import torch

from . import _lib
from .embedding import _field

stats = {"host_reads": 0}

_wb_pending = _lib.PendingStatus(stats)
_COMBINE = {"sum": _lib.WB_COMBINE_SUM, "max": _lib.WB_COMBINE_MAX}


_wb_scalars = _lib.pt_scalars


class _WeightedBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, graph, y8, keep8, pt_a, pt_b, scalars, combine):
        lib = _lib.load()
        dev = scores.device
        p = int(scores.numel())
        idt = _lib.index_dtype(graph)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        state = torch.empty(_lib.WB_STATE, dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        ws, nb = _lib.workspace("hgnn_weighted_bce_workspace_bytes", dev, p, 0)
        with torch.cuda.device(dev):
            _lib.check(lib.hgnn_weighted_bce_forward(_lib.ptr(scores), _lib.ptr(graph), idt, _lib.ptr(y8),
                                                     _lib.ptr(keep8), _lib.ptr(pt_a), int(pt_a.numel()),
                                                     _lib.ptr(pt_b), int(pt_b.numel()), p, combine, scalars,
                                                     _lib.ptr(loss), _lib.ptr(state), _lib.ptr(status), _lib.ptr(ws),
                                                     nb, _lib.current_stream(dev)), "hgnn_weighted_bce_forward")
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(scores, graph, y8, pt_a, pt_b, state)
            ctx.keep8 = keep8
            ctx.scalars, ctx.idt, ctx.combine = scalars, idt, combine
        ctx.mark_non_differentiable(status, state)
        return loss.reshape(()), status, state

    @staticmethod
    def backward(ctx, grad_loss, _grad_status, _grad_state):
        scores, graph, y8, pt_a, pt_b, state = ctx.saved_tensors
        lib = _lib.load()
        dev = scores.device
        p = int(scores.numel())
        g = grad_loss.detach().reshape(1).to(torch.float32).contiguous()
        grad = torch.empty_like(scores)
        with torch.cuda.device(dev):
            _lib.check(lib.hgnn_weighted_bce_backward(_lib.ptr(scores), _lib.ptr(graph), ctx.idt, _lib.ptr(y8),
                                                      _lib.ptr(ctx.keep8), _lib.ptr(pt_a), int(pt_a.numel()),
                                                      _lib.ptr(pt_b), int(pt_b.numel()), p, ctx.combine, ctx.scalars,
                                                      _lib.ptr(state), _lib.ptr(g), _lib.ptr(grad),
                                                      _lib.current_stream(dev)), "hgnn_weighted_bce_backward")
        return grad, None, None, None, None, None, None, None


def weighted_bce_check(device=None):
    """Reads (ONE host read per device, counted in ``stats["host_reads"]``) and clears the status words of the
    ``weighted_bce_loss`` calls made since the last check: ValueError if any of them saw a pair id out of range or a
    score that is NaN or outside [0, 1]."""
    word = _wb_pending.take(device)
    if word & _lib.WB_ST_BAD_ID:
        raise ValueError("weighted_bce_loss: a pair id is negative or >= the length of its pt table")
    if word & _lib.WB_ST_BAD_SCORE:
        raise ValueError("weighted_bce_loss: a score is NaN or outside [0, 1]")


def _wb_bytes(t, name, p):
    if not torch.is_tensor(t) or t.dtype not in (torch.bool, torch.uint8) or t.shape != (p,):
        raise ValueError(f"weighted_bce_loss: {name} must be bool or uint8 with one entry per pair")
    return t.contiguous().view(torch.uint8)


def _wb_table(t, name):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 1:
        raise ValueError(f"weighted_bce_loss: {name} must be a float32 vector")
    return t.detach().contiguous()


def _wb_apply(scores, graph, y, pt_a, hparams, pt_b, combine, keep):
    """(loss, status, state) of one validated call; the status word joins the device's pending word"""
    if not torch.is_tensor(scores) or not torch.is_tensor(graph):
        raise ValueError("weighted_bce_loss: scores and graph must be tensors")
    if scores.dim() != 1 or scores.dtype != torch.float32:
        raise ValueError(f"weighted_bce_loss: scores must be float32 [P], got {scores.dtype} {tuple(scores.shape)}")
    p = int(scores.numel())
    if graph.dim() != 2 or graph.shape[0] != 2 or graph.dtype not in (torch.int64, torch.int32) or graph.shape[1] != p:
        raise ValueError(f"weighted_bce_loss: graph must be int64 or int32 [2, P = {p}], got {graph.dtype} "
                         f"{tuple(graph.shape)}")
    if combine not in _COMBINE:
        raise ValueError(f"weighted_bce_loss: combine must be 'sum' or 'max', got {combine!r}")
    y8 = _wb_bytes(y, "y", p)
    keep8 = None if keep is None else _wb_bytes(keep, "keep", p)
    pt_a = _wb_table(pt_a, "pt_a")
    pt_b = pt_a if pt_b is None else _wb_table(pt_b, "pt_b")
    if not scores.is_cuda or not graph.is_cuda:
        raise RuntimeError("weighted_bce_loss needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    dev = scores.device
    if any(t.device != dev for t in (graph, y8, pt_a, pt_b)) or (keep8 is not None and keep8.device != dev):
        raise ValueError("weighted_bce_loss: scores, graph, y, keep and the pt tables must be on one device")
    loss, status, state = _WeightedBCE.apply(scores.contiguous(), graph.contiguous(), y8, keep8, pt_a, pt_b,
                                             _wb_scalars(hparams), _COMBINE[combine])
    _wb_pending.add(dev, status)
    return loss, status, state


def weighted_bce_loss(scores, graph, y, pt_a, hparams, pt_b=None, combine="sum", keep=None, check=False):
    """sum_i w_i bce(s_i, y_i) (0-d float32, differentiable in ``scores`` only) with the reference's class-balanced
    pT weights: raw_i = combine(pt_weighting(pt_a[graph[0, i]]), pt_weighting(pt_b[graph[1, i]])), w_i = raw_i /
    S_T * sigmoid(lwr) for a true pair and raw_i / S_F * sigmoid(-lwr) for a false one, S_T / S_F the class sums of
    raw, and bce torch's ``binary_cross_entropy`` (logs clamped at -100).  ``combine="sum"`` with one table is the
    edge classifier's ``get_training_weight``, ``combine="max"`` with the supernodes' table as ``pt_b`` is
    ``get_asgmt_weight``.

    ``scores`` float32 [P] in [0, 1]; ``graph`` [2, P] int64 or int32; ``y`` [P] bool or uint8; ``pt_a`` float32 [NA],
    ``pt_b`` float32 [NB] (default: ``pt_a``), neither written; ``keep`` [P] bool or uint8 or None: a pair with
    keep == 0 contributes to nothing and gets gradient 0.  The class sums and the loss are float64 sums in a fixed
    order: two calls return the same bits.  A class of pairs whose weights sum to 0 contributes nothing.

    The call makes NO host read.  A pair with an id out of range, or a score that is NaN or outside [0, 1], is skipped
    by the kernels (never a fault) and recorded in a device status word; ``check=True`` reads it after the call (one
    host read, counted in ``stats["host_reads"]``) and raises ValueError, as does a later ``weighted_bce_check()``."""
    loss, _, _ = _wb_apply(scores, graph, y, pt_a, hparams, pt_b, combine, keep)
    if check:
        weighted_bce_check(scores.device)
    return loss


def _ec_truth(who, batch, hparams):
    """(y, keep or None) of the edge classifier's loss in the ``true_edges`` mode of ``hparams``"""
    mode = hparams["true_edges"]
    if mode not in ("modulewise_true_edges", "pid_true_edges"):
        raise ValueError(f"{who}: true_edges must be 'modulewise_true_edges' or 'pid_true_edges', "
                         f"got {mode!r}")
    if mode == "modulewise_true_edges":
        y, y_pid = _field(batch, "y"), _field(batch, "y_pid")
        return y.bool(), (y_pid == 0) | (y == 1)
    return _field(batch, "y_pid").bool(), None


def ec_training_loss(scores, batch, hparams):
    """EdgeClassifierBase.training_step after the forward (edge_classifier_base.py:115-128), and the loss of
    shared_evaluation (:143-154).  ``batch``: anything with ``edge_index``, ``y``, ``y_pid`` and ``pt`` (attributes or
    keys) on the scores' device.  With ``true_edges == "modulewise_true_edges"`` the neutral edges (PID-true but not
    modulewise) are dropped through a keep mask: no compaction, no host read."""
    y, keep = _ec_truth("ec_training_loss", batch, hparams)
    if not torch.is_tensor(scores) or not scores.is_cuda:
        raise RuntimeError("ec_training_loss needs HIP device tensors: hierarchicalgnn_amd has no CPU path")
    return weighted_bce_loss(scores, _field(batch, "edge_index"), y, _field(batch, "pt"), hparams, keep=keep)


def ec_shared_evaluation(scores, batch, event, hparams):
    """EdgeClassifierBase.shared_evaluation after the forward (edge_classifier_base.py:143-181): (bipartite_graph,
    loss, metrics).  ``batch`` as for ``ec_training_loss`` plus ``inverse_mask``; ``event``: the unmodified event with
    ``pid`` and ``pt`` on the device (not written: the reference's ``event.pt[event.pid == 0] = 0`` is applied to a
    copy); ``hparams`` also carries score_cut, ptcut, n_hits and majority_cut."""
    from .tracking import edge_track_candidates, eval_metrics
    loss = ec_training_loss(scores, batch, hparams)
    bipartite_graph = edge_track_candidates(_field(batch, "edge_index"), scores, hparams["score_cut"],
                                            _field(batch, "inverse_mask"))
    pid, pt = _field(event, "pid"), _field(event, "pt")
    ev = {"pid": pid, "pt": torch.where(pid == 0, torch.zeros_like(pt), pt)}
    metrics = eval_metrics(bipartite_graph, ev, pt_cut=hparams["ptcut"], nhits_cut=hparams["n_hits"],
                           majority_cut=hparams["majority_cut"], primary=False)
    return bipartite_graph, loss, metrics


def ec_score_scan(scores, batch, event, hparams, cuts):
    """The tracking metrics of ``ec_shared_evaluation`` at every score cut of ``cuts`` instead of at
    ``hparams["score_cut"]``, with the edge counts per cut (``tracking.edge_score_scan``: one device call, ONE host
    read).  Truth and keep are formed as ``ec_training_loss`` forms them in the ``true_edges`` mode of ``hparams``;
    ``event.pt`` is zeroed at ``pid == 0`` on a copy; ``hparams`` carries ptcut, n_hits and majority_cut."""
    from .tracking import edge_score_scan
    y, keep = _ec_truth("ec_score_scan", batch, hparams)
    pid, pt = _field(event, "pid"), _field(event, "pt")
    ev = {"pid": pid, "pt": torch.where(pid == 0, torch.zeros_like(pt), pt)}
    return edge_score_scan(_field(batch, "edge_index"), scores, cuts, _field(batch, "inverse_mask"), ev,
                           pt_cut=hparams["ptcut"], nhits_cut=hparams["n_hits"], majority_cut=hparams["majority_cut"],
                           primary=False, truth=y, keep=keep)
