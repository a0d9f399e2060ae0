"""float64 numpy restatement of the pT-weighted binary cross-entropy (include/hgnn_hip.h, "weighted BCE"; reference
EdgeClassifier/edge_classifier_base.py:99-111, :127-128 and bipartite_classification_base.py:123-138, :189-190): the
loss, its gradient in the scores, the weights and the class sums.  It reads the float32 inputs as they are and forms
1 - s in float32, as torch's binary_cross_entropy does; everything after that is float64."""
import numpy as np

from pairloss_ref import _sigmoid, pt_weighting


def raw_weights(pt_a, pt_b, graph, hp, combine="sum"):
    wa = pt_weighting(np.asarray(pt_a)[graph[0]], hp)
    wb = pt_weighting(np.asarray(pt_b)[graph[1]], hp)
    return wa + wb if combine == "sum" else np.maximum(wa, wb)


def weighted_bce(scores, graph, y, pt_a, hp, pt_b=None, combine="sum", keep=None):
    """(loss, grad_scores [P], w [P], (S_T, S_F)) in float64.  A dropped pair (keep == 0) has weight and gradient 0; a
    class whose raw weights sum to 0 (an empty class in particular) gets weight 0."""
    assert combine in ("sum", "max")
    graph = np.asarray(graph).astype(np.int64)
    y = np.asarray(y).astype(bool)
    s32 = np.asarray(scores, np.float32)
    keep = np.ones(y.shape, bool) if keep is None else np.asarray(keep).astype(bool)
    raw = raw_weights(pt_a, pt_a if pt_b is None else pt_b, graph, hp, combine)
    w = np.zeros(raw.shape, np.float64)
    sums = []
    for cls, sign in ((y & keep, 1.0), (~y & keep, -1.0)):
        tot = raw[cls].sum()
        sums.append(float(tot))
        if tot > 0:
            w[cls] = raw[cls] / tot * _sigmoid(sign * hp["log_weight_ratio"])
    s = s32.astype(np.float64)
    one_minus = (np.float32(1.0) - s32).astype(np.float64)
    with np.errstate(divide="ignore"):
        ell = -np.where(y, np.maximum(np.log(s), -100.0), np.maximum(np.log(one_minus), -100.0))
    loss = float((w * ell).sum())
    grad = w * (s - y) / np.maximum(one_minus * s, 1e-12)
    return loss, grad, w, tuple(sums)
