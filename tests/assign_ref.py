"""CPU restatement of the assignment loss (reference BipartiteClassification/bipartite_classification_base.py:
108-224): float64 contraction in position order, scipy's min_weight_full_bipartite_matching on the P x (C + P)
matrix with the virtual columns, and the reference's post-matching lines in torch on the CPU.  Shared by the CPU
and the GPU tests; nothing here touches the HIP library."""
import numpy as np
import torch
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import min_weight_full_bipartite_matching

FALLBACK = 1e-12


def contract(row, col, score, n_rows, n_cols):
    """distinct (row, col) pairs in row-major order and the float64 sum of their float32 scores in ascending
    original position: (pair_row, pair_col, pair_weight)"""
    row = np.asarray(row, np.int64)
    col = np.asarray(col, np.int64)
    score = np.asarray(score, np.float32)
    key = row * np.int64(n_cols) + col
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    w = np.zeros(start.size, np.float64)
    s64 = score[order].astype(np.float64)
    ends = np.concatenate([start[1:], [ks.size]])
    longest = int((ends - start).max())
    for t in range(longest):   # position order within a pair, one term at a time: a fixed summation order
        sel = start + t < ends
        w[sel] += s64[start[sel] + t]
    uk = ks[start]
    return uk // n_cols, uk % n_cols, w


def solve(pair_row, pair_col, pair_weight, n_rows, n_cols):
    """scipy on the P x (C + P) matrix: col_match int64 [n_rows] (>= n_cols: the row's virtual column)"""
    data = np.concatenate([pair_weight, np.full(n_rows, FALLBACK)])
    rows = np.concatenate([pair_row, np.arange(n_rows)])
    cols = np.concatenate([pair_col, n_cols + np.arange(n_rows)])
    m = csr_matrix((data, (rows, cols)), shape=(n_rows, n_cols + n_rows))
    rm, cm = min_weight_full_bipartite_matching(m, maximize=True)
    out = np.empty(n_rows, np.int64)
    out[rm] = cm
    return out


def pair_lookup(pair_row, pair_col, pair_weight, n_cols):
    return dict(zip((np.asarray(pair_row, np.int64) * n_cols + np.asarray(pair_col, np.int64)).tolist(),
                    np.asarray(pair_weight, np.float64).tolist()))


def totals(col_match, pair_row, pair_col, pair_weight, n_cols):
    """(float64 total over the matched REAL pairs, number of virtual matches); KeyError when a row is matched to a
    column that is none of its pairs"""
    col_match = np.asarray(col_match, np.int64)
    look = pair_lookup(pair_row, pair_col, pair_weight, n_cols)
    real = np.flatnonzero(col_match < n_cols)
    w = np.array([look[int(r) * n_cols + int(col_match[r])] for r in real], np.float64)
    return float(np.sum(np.sort(w))), int(col_match.size - real.size)


def check_valid(col_match, pair_row, pair_col, n_rows, n_cols):
    """every row matched to one of its own pairs or to its own virtual column, no real column twice"""
    col_match = np.asarray(col_match, np.int64)
    assert col_match.shape == (n_rows,)
    have = set((np.asarray(pair_row, np.int64) * n_cols + np.asarray(pair_col, np.int64)).tolist())
    real = col_match[col_match < n_cols]
    assert np.unique(real).size == real.size, "a real column is used twice"
    for r, c in enumerate(col_match.tolist()):
        assert c == n_cols + r or (0 <= c < n_cols and r * n_cols + c in have), (r, c)


def certify_unique(pair_row, pair_col, pair_weight, n_rows, n_cols, margin):
    """Solve once; then, for every row, re-solve with that row's matched edge removed (its virtual edge included).
    If every re-solve loses more than ``margin`` the optimum is unique by that margin: any different full matching
    omits at least one matched edge.  Returns (unique, smallest loss)."""
    pair_row, pair_col = np.asarray(pair_row, np.int64), np.asarray(pair_col, np.int64)
    pair_weight = np.asarray(pair_weight, np.float64)
    data = np.concatenate([pair_weight, np.full(n_rows, FALLBACK)])
    rows = np.concatenate([pair_row, np.arange(n_rows)])
    cols = np.concatenate([pair_col, n_cols + np.arange(n_rows)])

    def best(keep):
        m = csr_matrix((data[keep], (rows[keep], cols[keep])), shape=(n_rows, n_cols + n_rows))
        rm, cm = min_weight_full_bipartite_matching(m, maximize=True)
        out = np.empty(n_rows, np.int64)
        out[rm] = cm
        return out, float(np.asarray(m[rm, cm]).sum())

    everything = np.ones(data.size, bool)
    match, opt = best(everything)
    smallest = np.inf
    for r in range(n_rows):
        keep = everything.copy()
        keep[(rows == r) & (cols == match[r])] = False
        if not keep[rows == r].any():
            continue   # the row has no other edge: no full matching omits this one
        try:
            _, alt = best(keep)
        except ValueError:
            continue   # no full matching without this edge
        smallest = min(smallest, opt - alt)
    return bool(smallest > margin), float(smallest)


def pt_weighting(pt, hp):
    pt = pt.clone()
    pt[pt != pt] = 0
    h = lambda i: torch.heaviside(i, torch.zeros(1).to(pt))  # noqa: E731
    minimum = lambda i: torch.minimum(i, torch.ones(1).to(pt))  # noqa: E731
    eps = hp["weight_leak"]
    cut = hp["ptcut"] - hp["pt_interval"]
    cap = hp["ptcut"]
    mw = hp["weight_min"]
    return mw + (1 - mw) * minimum(h(pt - cut) * (pt - cut) / (cap - cut)) + (eps * h(pt - cap) * (pt - cap))


def bipartite_loss(bipartite_scores, bipartite_graph, batch_pid, batch_pt, hp):
    """get_bipartite_loss on the CPU with the float64 position-order contraction: (loss, details)"""
    original_pid, pid = torch.unique(batch_pid, return_inverse=True)
    n_rows = int(original_pid.numel())
    n_cols = int(bipartite_graph[1].max()) + 1
    pt = torch.full((n_rows,), float("inf")).to(batch_pt).scatter_reduce(0, pid, batch_pt, "amin", include_self=True)
    with torch.no_grad():
        hit_row = pid[bipartite_graph[0]]
        pr, pc, pw = contract(hit_row.numpy(), bipartite_graph[1].numpy(), bipartite_scores.detach().numpy(),
                              n_rows, n_cols)
        col_match = torch.from_numpy(solve(pr, pc, pw, n_rows, n_cols))
        row_match = torch.arange(n_rows)
        noise_mask = (original_pid[row_match] != 0) & (col_match < n_cols)
        row_match, col_match = row_match[noise_mask], col_match[noise_mask]
        matched_particles = torch.zeros(n_rows, dtype=torch.bool)
        matched_particles[row_match] = True
        matched_hits = matched_particles[hit_row]
        pid_assignments = torch.zeros(n_rows).long()
        pid_assignments[row_match] = col_match
        truth = torch.zeros(len(bipartite_scores), dtype=torch.bool)
        truth[matched_hits] = pid_assignments[hit_row[matched_hits]] == bipartite_graph[1][matched_hits]
    supernodes_pt = torch.zeros(n_cols).float()
    supernodes_pt[col_match] = pt[row_match].float()
    weights = torch.maximum(pt_weighting(batch_pt[bipartite_graph[0]], hp),
                            pt_weighting(supernodes_pt[bipartite_graph[1]], hp))
    tw, fw = weights[truth].sum(), weights[~truth].sum()
    weights[truth] = (weights[truth] / tw) * torch.sigmoid(hp["log_weight_ratio"] * torch.ones(1))
    weights[~truth] = (weights[~truth] / fw) * torch.sigmoid(-hp["log_weight_ratio"] * torch.ones(1))
    weights = weights.float()
    loss = torch.nn.functional.binary_cross_entropy(bipartite_scores, truth.float(), reduction="none")
    loss = torch.dot(loss, weights)
    return loss, {"row_match": row_match, "col_match": col_match, "truth": truth, "weights": weights,
                  "pairs": (pr, pc, pw), "n_rows": n_rows, "n_cols": n_cols}


def embedding_loss(embeddings, edge_index, batch_pid, batch_pt, hp):
    """training_step :199-204 on the CPU"""
    y = batch_pid[edge_index[0]] == batch_pid[edge_index[1]]
    weights = pt_weighting(batch_pt[edge_index[0]], hp) + pt_weighting(batch_pt[edge_index[1]], hp)
    tw, fw = weights[y].sum(), weights[~y].sum()
    weights[y] = (weights[y] / tw) * torch.sigmoid(hp["log_weight_ratio"] * torch.ones(1))
    weights[~y] = (weights[~y] / fw) * torch.sigmoid(-hp["log_weight_ratio"] * torch.ones(1))
    weights = weights.float()
    hinge = torch.ones(len(y)).long()
    hinge[~y] = -1
    dist = ((embeddings[edge_index[0]] - embeddings[edge_index[1]]).square().sum(-1) + 1e-12).sqrt()
    loss = torch.nn.functional.hinge_embedding_loss(dist / hp["train_r"], hinge, margin=1, reduction="none").square()
    return torch.dot(loss, weights)


HPARAMS = {"weight_leak": 0.1, "ptcut": 1.0, "pt_interval": 0.5, "weight_min": 0.1, "log_weight_ratio": 0.0,
           "train_r": 1.0}
