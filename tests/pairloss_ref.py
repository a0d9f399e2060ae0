"""float64 numpy restatement of the weighted pair hinge loss (include/hgnn_hip.h, "pair hinge"; reference
GNNEmbedding/embedding_base.py:95-107, :137-155, :167-168): the loss, its parts and the gradient in the embeddings."""
import numpy as np


def pt_weighting(pt, hp):
    p = np.asarray(pt, np.float64).copy()
    p[np.isnan(p)] = 0.0
    cut = hp["ptcut"] - hp["pt_interval"]
    cap = hp["ptcut"]
    h = lambda x: (x > 0).astype(np.float64)  # noqa: E731  heaviside(x, 0)
    ramp = np.minimum(h(p - cut) * (p - cut) / (cap - cut), 1.0)
    return hp["weight_min"] + (1 - hp["weight_min"]) * ramp + hp["weight_leak"] * h(p - cap) * (p - cap)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def weights(pt, graph, y, hp):
    """w_i; a class whose raw weights sum to 0 (an empty class in particular) gets weight 0"""
    y = np.asarray(y).astype(bool)
    raw = pt_weighting(np.asarray(pt)[graph[0]], hp) + pt_weighting(np.asarray(pt)[graph[1]], hp)
    w = np.zeros(raw.shape, np.float64)
    for cls, sign in ((y, 1.0), (~y, -1.0)):
        s = raw[cls].sum()
        if s > 0:
            w[cls] = raw[cls] / s * _sigmoid(sign * hp["log_weight_ratio"])
    return w


def distance(emb, graph):
    e = np.asarray(emb, np.float64)
    diff = e[graph[0]] - e[graph[1]]
    return np.sqrt((diff * diff).sum(-1) + 1e-12), diff


def pair_hinge(emb, graph, y, pt, hp, margin=None, scale=1.0):
    """(loss, grad_E [N, D], w [P], d [P]) in float64"""
    graph = np.asarray(graph).astype(np.int64)
    y = np.asarray(y).astype(bool)
    margin = hp["train_r"] if margin is None else margin
    e = np.asarray(emb, np.float64)
    w = weights(pt, graph, y, hp)
    d, diff = distance(e, graph)
    t = scale * d
    ell = np.where(y, t, np.maximum(0.0, margin - t))
    loss = float((w * ell * ell).sum())
    dl_dd = np.where(y, scale, np.where(margin - t > 0, -scale, 0.0))
    c = 2.0 * w * ell * dl_dd / d
    grad = np.zeros_like(e)
    np.add.at(grad, graph[0], c[:, None] * diff)
    np.add.at(grad, graph[1], -c[:, None] * diff)
    return loss, grad, w, d
