"""CPU restatement (numpy, row by row) of the row-local pair construction (hierarchicalgnn_amd.embedding.training_pairs,
csrc/trainpairs.hip): get_training_samples (GNNEmbedding/embedding_base.py:109-135) from the kNN matrix, without the
prediction graph and without a global sort.  Not collected by pytest."""
import numpy as np

MODES = ("modulewise_true_edges", "pid_true_edges")


def e_bidir(mte, signal_mask):
    """[mte, mte.flip(0)] restricted to the columns whose two ends pass signal_mask, original order"""
    e = np.concatenate([mte, mte[::-1]], axis=1).astype(np.int64)
    return e[:, signal_mask[e].all(0)]


def training_pairs(idx, mte, signal_mask, pid, mode, skip_bad=False):
    """(graph int64 [2, P], y bool [P]).  idx int64 [N, K]: ids in [0, N), -1 = an empty slot anywhere in a row.
    ``skip_bad``: an entry of idx outside [-1, N) counts as an empty slot and a column of mte with an id outside
    [0, N) is dropped (what the kernels do beside setting their status); otherwise such an id is an error."""
    idx, mte, pid = np.asarray(idx, np.int64), np.asarray(mte, np.int64), np.asarray(pid, np.int64)
    signal_mask = np.asarray(signal_mask, bool)
    n = idx.shape[0]
    if skip_bad:
        mte = mte[:, ((mte >= 0) & (mte < n)).all(0)]
    else:
        assert ((idx >= -1) & (idx < n)).all() and ((mte >= 0) & (mte < n)).all()
    eb = e_bidir(mte, signal_mask)
    if mode not in MODES:
        raise ValueError(mode)
    modulewise = mode == "modulewise_true_edges"
    truth = np.unique((eb[0] << 31) | eb[1])
    rows, cols = [], []
    for i in range(n):
        js = idx[i]
        js = js[(js >= 0) & (js < n)]                                         # the valid slots, in slot order
        if modulewise:
            js = np.unique(js)                                                # distinct, ascending
            keys = (i << 31) | js
            at = np.minimum(np.searchsorted(truth, keys), truth.size - 1)     # truth is sorted: a binary search
            in_truth = truth[at] == keys if truth.size else np.zeros(js.size, bool)
            keep = ~in_truth & ((pid[i] != pid[js]) | (pid[i] == 0) | (pid[js] == 0))
        else:                                                                 # duplicates kept
            keep = ~(signal_mask[i] & signal_mask[js]) & ~((pid[i] == pid[js]) & (pid[i] != 0) & (pid[js] != 0))
        cols.append(js[keep])
        rows.append(np.full(int(keep.sum()), i, np.int64))
    g = np.stack([np.concatenate(rows), np.concatenate(cols)]) if n else np.zeros((2, 0), np.int64)
    if not modulewise:
        return g, np.zeros(g.shape[1], bool)                                  # the e_bidir part is empty here
    return np.concatenate([g, eb], 1), np.concatenate([np.zeros(g.shape[1], bool), np.ones(eb.shape[1], bool)])


def idx_from_pairs(pairs, n, k=None, scatter=None):
    """The kNN matrix int64 [n, k] of a row-sorted pair list int64 [2, E] (row ascending; a row's ids keep their
    order): -1 padding at the tail of each row, or, with ``scatter`` (a numpy Generator), at random slots.  ``k``
    defaults to the longest row (at least 1)."""
    pairs = np.asarray(pairs, np.int64)
    assert (np.diff(pairs[0]) >= 0).all()
    deg = np.bincount(pairs[0], minlength=n)
    k = max(int(deg.max(initial=0)), 1) if k is None else k
    assert deg.max(initial=0) <= k
    idx = np.full((n, k), -1, np.int64)
    start = np.concatenate([[0], np.cumsum(deg)])
    for i in range(n):
        ids = pairs[1, start[i]:start[i + 1]]
        slots = np.arange(ids.size) if scatter is None else np.sort(scatter.choice(k, ids.size, replace=False))
        idx[i, slots] = ids
    return idx


def pairs_from_idx(idx):
    """frnn_graph's expansion: the pairs (row, id) of the valid slots, row-major"""
    idx = np.asarray(idx, np.int64)
    pos = idx >= 0
    rows = np.broadcast_to(np.arange(idx.shape[0])[:, None], idx.shape)
    return np.stack([rows[pos], idx[pos]])


def random_case(rng, n, k, n_truth, signal="mixed", pid_kind="mixed"):
    """idx with in-row duplicates, self pairs and scattered -1; pid with zeros; mte with duplicate columns, self
    loops and pairs present in both directions"""
    idx = rng.integers(0, n, (n, k))
    dup = rng.random((n, k)) < 0.2
    idx = np.where(dup, np.roll(idx, 1, axis=1), idx)                          # in-row duplicates
    self_rows = rng.random(n) < 0.5
    idx[self_rows, rng.integers(0, k, int(self_rows.sum()))] = np.nonzero(self_rows)[0]
    idx = np.where(rng.random((n, k)) < 0.25, -1, idx)
    if n > 2:
        idx[1] = -1                                                            # an empty row
        idx[2] = np.abs(idx[2])                                                # (mostly) full row
    pid = {"mixed": rng.integers(0, max(n // 4, 2), n), "one": np.full(n, 7), "zero": np.zeros(n, int)}[pid_kind]
    pid = pid.astype(np.int64)
    sm = {"mixed": rng.random(n) < 0.7, "all": np.ones(n, bool), "none": np.zeros(n, bool)}[signal]
    return idx.astype(np.int64), random_truth(rng, idx, n_truth), sm, pid


def random_truth(rng, idx, n_truth):
    """mte int64 [2, n_truth]: random pairs, a quarter of them pairs that the rows of idx hold, and (from 8 columns
    on) a duplicate column, a pair in both directions and a self loop"""
    n, k = idx.shape
    mte = rng.integers(0, max(n, 1), (2, n_truth))
    if n_truth >= 8:
        q = n_truth // 4
        mte[:, :q] = pairs_from_idx(np.maximum(idx, 0))[:, rng.integers(0, n * k, q)]
        mte[:, q] = mte[:, 0]                                                  # a duplicate column
        mte[:, q + 1] = mte[::-1, 1]                                           # a pair in both directions
        mte[:, q + 2] = mte[0, q + 2]                                          # a self loop
    return mte.astype(np.int64)


ROW_KINDS = ("empty", "full", "copies", "self", "all_self", "holes")


def grid_idx(rng, n, k):
    """(idx int64 [n, k], kinds [n]) hand-made for the launch edges.  Row i is of kind ROW_KINDS[(i + k) % 6]: all
    -1; all valid (distinct ids where n >= k); k copies of one id; random ids with -1 in arbitrary slots and the self
    pair in one slot; k copies of i itself; random ids with -1 in arbitrary slots"""
    idx = np.empty((n, k), np.int64)
    kinds = []
    for i in range(n):
        kind = ROW_KINDS[(i + k) % len(ROW_KINDS)]
        kinds.append(kind)
        holes = np.where(rng.random(k) < 0.3, -1, rng.integers(0, n, k))
        if kind == "empty":
            row = np.full(k, -1)
        elif kind == "full":
            row = rng.permutation(n)[:k] if n >= k else rng.integers(0, n, k)
        elif kind == "copies":
            row = np.full(k, rng.integers(0, n))
        elif kind == "self":
            row = holes
            row[rng.integers(0, k)] = i
        elif kind == "all_self":
            row = np.full(k, i)
        else:
            row = holes
        idx[i] = row
    return idx, np.array(kinds)
