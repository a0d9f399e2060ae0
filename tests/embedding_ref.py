"""CPU restatement (numpy) of the embedding stage's pair construction for the tests: graph_intersection
(Modules/utils.py:117-166) on packed keys with np.unique instead of scipy, and get_training_samples
(GNNEmbedding/embedding_base.py:109-135).  Not collected by pytest."""
import numpy as np


def _keys(g):
    g = np.asarray(g, np.int64)
    return (g[0] << 31) | g[1]


def graph_intersection(pred, truth, weights=None):
    """(graph int64 [2, U], y bool [U]) and, with weights, the per-pair sum of the truth weights (0 if none), summed
    in truth order"""
    pk = np.unique(_keys(pred))
    tk = _keys(truth)
    graph = np.stack([pk >> 31, pk & ((1 << 31) - 1)]).astype(np.int64)
    y = np.isin(pk, tk)
    if weights is None:
        return graph, y
    weights = np.asarray(weights)
    out = np.zeros(pk.size, weights.dtype)
    order = np.argsort(tk, kind="stable")
    pos = np.searchsorted(pk, tk[order])
    for j, p in zip(order, pos):
        if p < pk.size and pk[p] == tk[j]:
            out[p] = out[p] + weights[j]
    return graph, y, out


def training_samples(pred, mte, signal_mask, pid, true_edges):
    e_bidir = np.concatenate([mte, mte[::-1]], axis=1)
    e_bidir = e_bidir[:, signal_mask[e_bidir].all(0)]
    if true_edges == "modulewise_true_edges":
        g, y = graph_intersection(pred, e_bidir)
        fake = g[:, ~y]
        m = (pid[fake[0]] != pid[fake[1]]) | (pid[fake] == 0).any(0)
        fake = fake[:, m]
        return np.concatenate([fake, e_bidir], 1), np.concatenate([np.zeros(fake.shape[1], bool),
                                                                   np.ones(e_bidir.shape[1], bool)])
    g = np.concatenate([pred, e_bidir], 1)
    y = (pid[g[0]] == pid[g[1]]) & (pid[g] != 0).all(0)
    mask = (signal_mask[g].all(0) | y) == 0
    return g[:, mask], y[mask]
