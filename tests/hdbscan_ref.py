"""Plain numpy restatement of the project's deterministic HDBSCAN* ("HDBSCAN"): the contract
csrc/hdbscan.hip is tested against.

    core2[i]   the min_samples-th smallest squared distance from i, i itself counted (sklearn / cuml convention)
    w2(i, j)   max(core2[i], core2[j], d2(i, j)); d2 = float32 sum of squared float32 differences in dimension order
    MST        the unique minimum spanning tree under the strict total order (w2, min(i, j), max(i, j))
    hierarchy  all MST edges of equal w2 are ONE simultaneous multi-way merge.  Read top-down a level is a true
               split iff at least two of its parts hold >= min_cluster_size points (those become clusters, the
               smaller parts fall out of the parent there); otherwise the parts below min_cluster_size fall out of
               the continuing cluster at that level
    stability  lambda = 1 / sqrt(w2) in float64 (LAMBDA_DUP for w2 = 0), sum of (lambda_leave - lambda_birth) over
               the points of a cluster, float64; EOM: a cluster is selected iff its stability >= the sum of the
               selected stabilities below it; the root is never selected
    labels     -1 = noise, clusters numbered 0..C-1 by smallest member index

No tie is broken by arrival order anywhere, so the result does not depend on the order of the points.
"""
import numpy as np

LAMBDA_DUP = 2.0 ** 100   # HGNN_HDBSCAN_LAMBDA_DUP: above 1 / sqrt(smallest positive float32) = 2.7e22


def d2_rows(x, lo, hi):
    """float32 d2[lo:hi, :] with the contract's arithmetic (one rounded product and one rounded sum per dimension)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    acc = np.zeros((hi - lo, x.shape[0]), np.float32)
    for k in range(x.shape[1]):
        t = x[lo:hi, k][:, None] - x[None, :, k]
        acc = acc + t * t
    return acc


MUTANTS = ("rank_lo", "rank_hi", "tie_maxmin", "last_point", "last_slice", "binary", "lambda_denorm")


def slice_layout(n, tile=256):
    """(slices, slice_len) of the candidate slicing of one Boruvka round (csrc/hdbscan.hip hdb_layout): at most 16
    slices, each a whole number of 256-point tiles, enough of them for 1024 workgroups"""
    blocks = -(-n // tile)
    s = min(max(-(-1024 // blocks), 1), 16)
    slice_len = -(-(-(-n // s)) // tile) * tile
    return -(-n // slice_len), slice_len


def core2(x, min_samples, chunk=512, mutant=None):
    """``mutant`` (tests only, tests/test_hdbscan_exact_ref.py): rank_lo / rank_hi take rank k-2 / k instead of
    k-1; last_point never offers the point N-1 as a candidate (every rank is taken among the other N-1 values)"""
    n = x.shape[0]
    r = min_samples - 1 + {"rank_lo": -1, "rank_hi": 1}.get(mutant, 0)
    cols = n - 1 if mutant == "last_point" else n
    r = min(r, cols - 1)
    assert 0 <= r < cols, "the mutant does not apply"
    out = np.empty(n, np.float32)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        out[lo:hi] = np.partition(d2_rows(x, lo, hi)[:, :cols], r, axis=1)[:, r]
    return out


def mst(x, c2, mutant=None):
    """``mutant`` (tests only): tie_maxmin orders equal weights by (max, min); last_slice never offers the points of
    the last candidate slice (slice_layout), so an edge between two of them is never seen.

    Prim with every choice made under the strict total order (w2, min, max): the order is total, so the minimum
    spanning tree is unique and this is the tree Kruskal under the same order builds.  Returns (edges [N-1, 2] with
    min first, w2 [N-1]) sorted by (w2, min, max)."""
    n = x.shape[0]
    x = np.ascontiguousarray(x, dtype=np.float32)
    ids = np.arange(n, dtype=np.int64)
    in_tree = np.zeros(n, bool)
    bw = np.full(n, np.inf, np.float32)
    bk = np.full(n, np.iinfo(np.int64).max, np.int64)   # min * n + max of the best edge to the tree
    edges = np.empty((n - 1, 2), np.int64)
    w2 = np.empty(n - 1, np.float32)
    cur = 0
    in_tree[0] = True
    cutoff = n
    if mutant == "last_slice":
        slices, slice_len = slice_layout(n)
        cutoff = (slices - 1) * slice_len
        assert cutoff > 0, "the mutant does not apply"
    for e in range(n - 1):
        w = np.maximum(np.maximum(d2_rows(x, cur, cur + 1)[0], c2), c2[cur])
        if cur >= cutoff:
            w[cutoff:] = np.inf
        if mutant == "tie_maxmin":
            k = np.maximum(ids, cur) * n + np.minimum(ids, cur)
        else:
            k = np.minimum(ids, cur) * n + np.maximum(ids, cur)
        better = (w < bw) | ((w == bw) & (k < bk))
        better &= ~in_tree
        bw[better] = w[better]
        bk[better] = k[better]
        cand = np.where(in_tree, np.float32(np.inf), bw)
        m = cand.min()
        assert np.isfinite(m), "non-finite input"
        tie = np.flatnonzero(cand == m)
        nxt = tie[np.argmin(bk[tie])]
        edges[e] = sorted((bk[nxt] // n, bk[nxt] % n))
        w2[e] = m
        in_tree[nxt] = True
        cur = int(nxt)
    order = np.lexsort((edges[:, 1], edges[:, 0], w2))
    return edges[order], w2[order]


def _lambda(w, dup=LAMBDA_DUP):
    return 1.0 / np.sqrt(np.float64(w)) if w > 0 else dup


def tree_labels(edges, w2, n, min_cluster_size, return_info=False, mutant=None):
    """dendrogram with multi-way levels -> condensed tree -> EOM -> labels, from MST edges sorted by w2.
    ``mutant`` (tests only): binary makes every edge a level of its own; lambda_denorm takes lambda of w2 = 0 as
    1 / sqrt(smallest positive float32)"""
    dup = 1.0 / np.sqrt(np.float64(2.0 ** -149)) if mutant == "lambda_denorm" else LAMBDA_DUP
    mcs = int(min_cluster_size)
    m = len(w2)
    assert m == n - 1
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    node_of = list(range(n))          # dendrogram node of a union-find root
    children = {}                     # internal node -> list of child nodes
    size = [1] * n
    level = [0.0] * n
    e = 0
    while e < m:
        f = e
        while f < m and w2[f] == w2[e]:
            f += 1
        if mutant == "binary":
            f = e + 1
        old = {}
        for a, b in edges[e:f]:
            ra, rb = find(int(a)), find(int(b))
            old[ra] = node_of[ra]
            old[rb] = node_of[rb]
            assert ra != rb
            parent[max(ra, rb)] = min(ra, rb)
        groups = {}
        for r in sorted(old):
            groups.setdefault(find(r), []).append(old[r])
        for r in sorted(groups):
            nid = len(size)
            children[nid] = groups[r]
            size.append(sum(size[c] for c in groups[r]))
            level.append(float(w2[e]))
            node_of[r] = nid
        e = f
    root = len(size) - 1
    assert size[root] == n

    def leaves(node):
        out, stack = [], [node]
        while stack:
            v = stack.pop()
            if v < n:
                out.append(v)
            else:
                stack.extend(children[v])
        return out

    # condensed tree: cluster 0 is the root
    c_parent, c_birth, c_stab, c_kids = [-1], [0.0], [0.0], [[]]
    fell = np.full(n, -1, np.int64)   # the cluster a point fell out of
    stack = [(root, 0)]
    while stack:
        node, c = stack.pop()
        if node < n:                  # only when n == 1
            fell[node] = c
            continue
        lam = _lambda(level[node], dup)
        kids = children[node]
        big = [k for k in kids if size[k] >= mcs]
        for k in kids:
            if size[k] < mcs:
                c_stab[c] += size[k] * (lam - c_birth[c])
                fell[leaves(k)] = c
        if len(big) >= 2:
            for k in big:
                c_stab[c] += size[k] * (lam - c_birth[c])
                nc = len(c_parent)
                c_parent.append(c)
                c_birth.append(lam)
                c_stab.append(0.0)
                c_kids.append([])
                c_kids[c].append(nc)
                stack.append((k, nc))
        elif len(big) == 1:
            stack.append((big[0], c))
    assert (fell >= 0).all()

    nc = len(c_parent)
    selected = [False] * nc
    sub = [0.0] * nc
    margin = np.inf
    for c in range(nc - 1, 0, -1):    # children have larger ids than their parents
        if not c_kids[c]:
            selected[c], sub[c] = True, c_stab[c]
            continue
        s = sum(sub[k] for k in c_kids[c])
        margin = min(margin, abs(c_stab[c] - s) / max(c_stab[c], s, 1e-300))
        if c_stab[c] >= s:
            selected[c], sub[c] = True, c_stab[c]
        else:
            sub[c] = s
    # a selected cluster unselects everything below it: the label of a cluster is its highest selected ancestor
    lab_of = [-1] * nc
    for c in range(1, nc):
        p = c_parent[c]
        lab_of[c] = lab_of[p] if lab_of[p] >= 0 else (c if selected[c] else -1)
    raw = np.array(lab_of, np.int64)[fell]
    labels = canonical(raw)
    if return_info:
        return labels, {"eom_margin": float(margin), "n_condensed": nc}
    return labels


def canonical(raw):
    """relabel clusters 0..C-1 by smallest member index; negative stays -1"""
    raw = np.asarray(raw)
    out = np.full(raw.shape, -1, np.int64)
    seen = {}
    for i, r in enumerate(raw.tolist()):
        if r < 0:
            continue
        if r not in seen:
            seen[r] = len(seen)
        out[i] = seen[r]
    return out


def hdbscan(x, min_cluster_size=5, min_samples=None, return_all=False, mutant=None):
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[0]
    ms = int(min_cluster_size if min_samples is None else min_samples)
    assert n >= min_cluster_size and 1 <= ms <= n
    c2 = core2(x, ms, mutant=mutant)
    edges, w2 = mst(x, c2, mutant=mutant)
    labels, info = tree_labels(edges, w2, n, min_cluster_size, return_info=True, mutant=mutant)
    if return_all:
        return labels, edges, w2, c2, info
    return labels
