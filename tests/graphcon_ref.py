"""CPU references of the device-side graph construction (csrc/graphcon.hip): the edge list of a kNN result and the
attention weights as one operator.

``edges_ref`` restates ``hgnn_knn_edges`` slot by slot in plain Python; tests/test_graphcon_ref.py proves it equal to
``hierarchy_ref.edges_from_knn`` (the torch formulation ``build_graph`` uses).

``attention_ref`` restates ``hgnn_graph_attention_*``: x in float32, the sums in float64, the elementwise part in
float32 from the float64 scalars rounded once, and the closed-form backward.  With ``dtype=np.float64`` the same code is
the exact formula, which tests/test_graphcon_ref.py checks against autograd of ``oracle.hgnn_oracle.graph_edge_weights``;
with ``dtype=np.float32`` it is the emulation of the kernels that sizes the distance to the 1e-4 bar.  ``mutant`` breaks
one piece of the arithmetic on purpose: the tests show that the bar sees each of them.

``cases()`` is the list of attention cases that tests/test_gpu_graphcon.py runs on the device; the CPU file runs the
emulation on the same list.
"""
import numpy as np
import torch

MUTANTS = ("var_unbiased", "no_dgamma", "no_sgf", "exp_derivative", "running_var_biased")
K_CASE = 5                     # neighbours per query of the attention cases
N_PTS_CASE = 8                 # points of the small cases: every query's 5 nearest of 8
BIG_E = (105_000, 1000)        # (nq, n_pts): E = 525000 > one grid trip of 2048 workgroups x 256 threads = 524288


# ------------------------------------------------------------------ edge lists
def edges_ref(idx: torch.Tensor, n_pts: int, sym: bool, mutant: str = None) -> torch.Tensor:
    """``hgnn_knn_edges``: the valid slots (0 <= id < n_pts) in row-major order; with ``sym`` both directions of each,
    sorted by (src, dst), duplicates removed.  mutants: "drop_last_slot", "no_dedup" """
    nq, K = idx.shape
    rows = idx.tolist()
    pairs = []
    for r in range(nq):
        for j in range(K - 1 if mutant == "drop_last_slot" else K):
            v = rows[r][j]
            if v < -1 or v >= n_pts:
                raise ValueError("bad id")
            if v >= 0:
                pairs.append((r, v))
    if sym:
        both = pairs + [(d, s) for s, d in pairs]
        pairs = sorted(both) if mutant == "no_dedup" else sorted(set(both))
    if not pairs:
        return torch.empty((2, 0), dtype=torch.int64)
    return torch.tensor(pairs, dtype=torch.int64).t().contiguous()


def edge_cases():
    """(name, idx [nq, K], n_pts): rows with 0, 1 .. K valid slots, an empty slot before a valid one, nq != n_pts
    both ways, self-pairs and pairs present in both directions"""
    out = []
    K = 4
    rows = [[-1] * K]
    for c in range(1, K + 1):
        rows.append([(3 * c + j) % 7 for j in range(c)] + [-1] * (K - c))
    rows.append([-1, 2, -1, 5])                      # holes before valid slots
    rows.append([-1, -1, -1, 6])
    rows.append([8, 0, -1, 1])                       # row 8: a self-pair
    out.append(("counts_and_holes", torch.tensor(rows, dtype=torch.int64), 9))
    out.append(("nq_gt_npts", torch.tensor([[0, 1], [1, 0], [2, -1], [-1, 1], [0, 2]], dtype=torch.int64), 3))
    out.append(("nq_lt_npts", torch.tensor([[11, 0], [-1, 10], [1, 11]], dtype=torch.int64), 12))
    # (0,1)/(1,0) and (2,3)/(3,2) are each other's reverse; (1,1) and (3,3) are self-pairs
    out.append(("reverse_pairs", torch.tensor([[1, -1, -1], [0, 1, -1], [3, -1, 0], [2, 3, -1]], dtype=torch.int64), 4))
    out.append(("all_empty", torch.full((5, 3), -1, dtype=torch.int64), 5))
    out.append(("single", torch.tensor([[0]], dtype=torch.int64), 1))
    return out


def knn_pattern(nq: int, K: int, n_pts: int, fill: str, seed: int) -> torch.Tensor:
    """a kNN-shaped idx [nq, K] with distinct ids per row: "empty", "full", "prefix" (a random number of valid slots
    at the front of each row) or "holes" (each slot emptied with probability 1/3, wherever it sits)"""
    g = torch.Generator().manual_seed(seed)
    assert n_pts >= K
    base = torch.stack([torch.randperm(n_pts, generator=g)[:K] for _ in range(nq)]) if nq * n_pts <= 1 << 16 else \
        (torch.randint(0, n_pts, (nq, 1), generator=g) + torch.arange(K).unsqueeze(0) * (n_pts // K)) % n_pts
    base = base.to(torch.int64)
    if fill == "full":
        return base
    if fill == "empty":
        return torch.full_like(base, -1)
    if fill == "prefix":
        count = torch.randint(0, K + 1, (nq, 1), generator=g)
        return torch.where(torch.arange(K).unsqueeze(0) < count, base, torch.full_like(base, -1))
    assert fill == "holes"
    return torch.where(torch.rand(nq, K, generator=g) < 1.0 / 3.0, torch.full_like(base, -1), base)


# ------------------------------------------------------------------ attention weights
def dot_f32(A: np.ndarray, B: np.ndarray, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """x_e in float32 with ``hgnn_edge_dot_f32``'s summation tree (the products' rounding is the kernel's fused
    multiply-add; the difference is below one ulp of a term and irrelevant at the 1e-4 bar)"""
    D = A.shape[1]
    p = np.zeros((a.shape[0], 16), np.float32)
    p[:, :D] = A[a].astype(np.float32) * B[b].astype(np.float32)
    if D % 4 == 0:
        q = ((p[:, 0::4] + p[:, 1::4]) + p[:, 2::4]) + p[:, 3::4]
        return (q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])
    off = 1
    while off < 16:
        p[:, ::2 * off] = p[:, ::2 * off] + p[:, off::2 * off]
        off *= 2
    return p[:, 0].copy()


def _phi(z, fn, dt):
    z = z.astype(dt)
    return np.exp(z).astype(dt) if fn == "exp" else (dt(1) / (dt(1) + np.exp(-z))).astype(dt)


def attention_ref(A, B, graph, gamma, beta, running_mean, running_var, nbt, fn, norm, training, eps=1e-5, momentum=0.1,
                  g_w=None, g_logits=None, dtype=np.float32, mutant=None):
    """dict(x, logits, weights, running_mean, running_var, nbt[, dA, dB, dgamma, dbeta]).  ``dtype``: the elementwise
    precision (float32 = the kernels', float64 = the exact formula); sums are float64 either way."""
    dt = dtype
    a, b = np.asarray(graph[0]), np.asarray(graph[1])
    E = a.shape[0]
    if dt is np.float32:
        x = dot_f32(np.asarray(A, np.float32), np.asarray(B, np.float32), a, b)
    else:
        x = (np.asarray(A, np.float64)[a] * np.asarray(B, np.float64)[b]).sum(-1)
    out = {"x": x}
    x64 = x.astype(np.float64)
    rm, rv = float(running_mean), float(running_var)
    if training:
        mu = x64.sum() / E
        var = max((x64 * x64).sum() / E - mu * mu, 0.0) if dt is np.float32 else ((x64 - mu) ** 2).sum() / E
        var_used = var * E / (E - 1) if mutant == "var_unbiased" else var
        nbt = nbt + 1
        m = 1.0 / nbt if momentum is None else momentum
        rm = float(np.float32((1 - m) * rm + m * mu))
        rv = float(np.float32((1 - m) * rv + m * (var if mutant == "running_var_biased" else var * E / (E - 1))))
    else:
        mu, var_used = rm, rv
    rstd = 1.0 / np.sqrt(var_used + eps)
    out.update(running_mean=rm, running_var=rv, nbt=nbt)
    g, bt = dt(gamma), dt(beta)
    xh = ((x.astype(dt) - dt(mu)) * dt(rstd)).astype(dt)
    z = (g * xh + bt).astype(dt)
    f = _phi(z, fn, dt)
    sum_f = f.astype(np.float64).sum()
    w = (f * dt(E / sum_f)).astype(dt) if norm else f
    out.update(logits=z, weights=w)
    if g_w is None and g_logits is None:
        return out
    gw = np.zeros(E, dt) if g_w is None else np.asarray(g_w).astype(dt)
    if norm:
        mean_f = sum_f / E
        sgf = (gw.astype(np.float64) * f.astype(np.float64)).sum()
        c0 = 0.0 if mutant == "no_sgf" else sgf / (E * mean_f * mean_f)
        gf = (dt(1.0 / mean_f) * gw - dt(c0)).astype(dt)
    else:
        gf = gw
    dphi = f if (fn == "exp" or mutant == "exp_derivative") else (f * (dt(1) - f)).astype(dt)
    G = (gf * dphi).astype(dt)
    if g_logits is not None:
        G = (G + np.asarray(g_logits).astype(dt)).astype(dt)
    dbeta = G.astype(np.float64).sum()
    dgamma = (G.astype(np.float64) * xh.astype(np.float64)).sum()
    k = dt(g * dt(rstd))
    if training:
        mg = 0.0 if mutant == "no_dgamma" else dgamma / E
        gx = (k * (G - dt(dbeta / E) - xh * dt(mg))).astype(dt)
    else:
        gx = (k * G).astype(dt)
    # dA, dB: the segmented reduce sums float32 rows; float64 here (its own conformance tests bound that error)
    A64, B64 = torch.as_tensor(np.asarray(A, np.float64)), torch.as_tensor(np.asarray(B, np.float64))
    ta, tb, tg = torch.as_tensor(a).long(), torch.as_tensor(b).long(), torch.as_tensor(gx.astype(np.float64))
    dA = torch.zeros_like(A64).index_add_(0, ta, tg[:, None] * B64[tb]).numpy()
    dB = torch.zeros_like(B64).index_add_(0, tb, tg[:, None] * A64[ta]).numpy()
    out.update(dA=dA, dB=dB, dgamma=dgamma, dbeta=dbeta, gx=gx)
    return out


def oracle64(A, B, graph, gamma, beta, running_mean, running_var, fn, norm, training, eps=1e-5, g_w=None,
             g_logits=None, same=False):
    """autograd of ``oracle.hgnn_oracle.graph_edge_weights`` on float64 copies; ``same``: A is B (one leaf).
    Works on whatever device the inputs live on."""
    from oracle import hgnn_oracle as O
    A64 = torch.as_tensor(A).double().clone().requires_grad_(True)
    B64 = A64 if same else torch.as_tensor(B).double().clone().requires_grad_(True)
    dev = A64.device
    ga = torch.tensor([float(gamma)], dtype=torch.float64, device=dev, requires_grad=True)
    be = torch.tensor([float(beta)], dtype=torch.float64, device=dev, requires_grad=True)
    graph = torch.as_tensor(graph).to(dev).long()
    w, z = O.graph_edge_weights(A64, B64, graph, ga, be, torch.tensor(float(running_mean), dtype=torch.float64, device=dev),
                                torch.tensor(float(running_var), dtype=torch.float64, device=dev), fn, norm,
                                training=training, eps=eps)
    out = {"weights": w.squeeze(1).detach(), "logits": z.detach()}
    if g_w is None and g_logits is None:
        return out
    loss = 0.0
    if g_w is not None:
        loss = loss + (w.squeeze(1) * torch.as_tensor(g_w).to(dev).double()).sum()
    if g_logits is not None:
        loss = loss + (z * torch.as_tensor(g_logits).to(dev).double()).sum()
    loss.backward()
    out.update(dA=A64.grad, dB=None if same else B64.grad, dgamma=ga.grad[0], dbeta=be.grad[0])
    return out


MODES = [(training, fn, norm, gl) for training in (True, False) for fn in ("sigmoid", "exp") for norm in (False, True)
         for gl in (False, True)]
DIMS = (1, 3, 8, 16)
SIZES = (2, 63, 64, 65, 257, 4097)


def cases():
    """(name, D, E, seed, training, fn, norm, with_g_logits, same, backward): every D x E with the 16 modes taken in
    turn (E = 2: their eval-mode twins), all 16 modes at D = 8, E = 257, E = 2 in training mode at D = 1 and D = 8 (see
    ``gx_bar``), the super-graph form (A is B), and one E beyond a single grid trip."""
    out = []
    i = 0
    for D in DIMS:
        for E in SIZES:
            tr, fn, norm, gl = MODES[i % len(MODES)]
            if E == 2:
                tr = False
            out.append((f"D{D}_E{E}", D, E, 100 + i, tr, fn, norm, gl, False, True))
            i += 5                                    # 5 is coprime to 16: the modes cycle through all of them
    out.append(("D1_E2_train", 1, 2, 10100, True, "sigmoid", True, False, False, True))   # seed: x = (1, -1)
    out.append(("D8_E2_train", 8, 2, 151, True, "exp", False, True, False, True))
    for j, (tr, fn, norm, gl) in enumerate(MODES):
        out.append((f"mode{j}", 8, 257, 200 + j, tr, fn, norm, gl, False, True))
    out.append(("same_train", 8, 257, 300, True, "sigmoid", True, True, True, True))
    out.append(("same_eval", 3, 65, 301, False, "exp", True, False, True, True))
    out.append(("big", 8, BIG_E[0] * K_CASE, 400, True, "exp", True, True, False, True))
    return out


BAR = 1e-4
DBETA_ZERO_BOUND = 1e-6


def gx_bar(training, E, x, eps=1e-5):
    """The bar for dA and dB.  1e-4, except at E = 2 in training mode: two edges have xhat = +-c with
    c^2 = var / (var + eps), so g_x = gamma rstd (G1 - G2) / 2 (1 - c^2) is the difference of terms that agree to
    eps / (var + eps) of their size.  Each of the about 8 float32 roundings on the way (x, xhat, z, f, G, the two means,
    the difference) moves it by 2^-24 of those terms, i.e. by 2^-24 (var + eps) / eps of the result: the bar there is
    8 x 2^-24 (var + eps) / eps (0.048 at var = 1), if that is above 1e-4.  dgamma and dbeta do not suffer the
    cancellation and keep 1e-4."""
    if not (training and E == 2):
        return BAR
    var = float(np.var(np.asarray(x, np.float64)))
    return max(BAR, 8 * 2.0 ** -24 * (var + eps) / eps)


def dbeta_is_zero(fn, norm, gl):
    """exp(z + c) / mean exp(z + c) is free of c: with exp, norm and no g_logits the weights do not depend on beta and
    dbeta = sum G is 0 in exact arithmetic -- a rounding residue in any other, with nothing to be relative to"""
    return fn == "exp" and norm and not gl


def dbeta_scale(g_w, weights):
    """what the residue of a vanishing dbeta is measured against: G_e = g_w w_e - w_e (sum g_w w) / E is formed from
    the two terms g_w w_e and w_e mean(g_w w) by 4 float32 roundings (the two float64 coefficients rounded once, one
    product, one difference), each at most 2^-24 of the larger term.  So |dbeta| <= 4 x 2^-24 S = 2.4e-7 S with
    S = sum |g_w w| + |sum g_w w|; ``DBETA_ZERO_BOUND`` = 1e-6 leaves a factor 4."""
    gw = np.asarray(g_w, np.float64).reshape(-1)
    w = np.asarray(weights, np.float64).reshape(-1)
    return float(np.abs(gw * w).sum() + abs((gw * w).sum()))


def errors(got, ref, c, x, g_w):
    """{quantity: (normwise, element-wise)} of ``got`` against the float64 oracle ``ref``, each scaled so that ITS bar
    reads 1e-4: weights, logits, dgamma, dbeta at 1e-4 (``conftest.rel_err`` / ``elem_err``; dgamma and dbeta each on
    its own), dA and dB at ``gx_bar``, and in the modes where dbeta vanishes |dbeta| / S at ``DBETA_ZERO_BOUND``."""
    import conftest
    name, D, E, seed, training, fn, norm, gl, same, bw = c

    def num(t):
        return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, np.float64)
    out = {}
    for q in ("weights", "logits"):
        r = num(ref[q])
        g = num(got[q]).reshape(r.shape)
        out[q] = (conftest.rel_err(g, r), conftest.elem_err(g, r))
    if not bw:
        return out
    k = BAR / gx_bar(training, E, num(x))
    for q in ("dA", "dB"):
        if ref.get(q) is None:
            continue
        r = num(ref[q])
        g = num(got[q]).reshape(r.shape)
        out[q] = (k * conftest.rel_err(g, r), k * conftest.elem_err(g, r))
    r, g = num(ref["dgamma"]).reshape(1), num(got["dgamma"]).reshape(1)
    out["dgamma"] = (conftest.rel_err(g, r), conftest.elem_err(g, r))
    r, g = num(ref["dbeta"]).reshape(1), num(got["dbeta"]).reshape(1)
    if dbeta_is_zero(fn, norm, gl):
        e = abs(float(g[0])) / dbeta_scale(num(g_w), num(ref["weights"])) * (BAR / DBETA_ZERO_BOUND)
        out["dbeta"] = (e, e)
    else:
        out["dbeta"] = (conftest.rel_err(g, r), conftest.elem_err(g, r))
    return out


def case_shape(E, same):
    """(nq, n_pts) of a case: 5 neighbours per query out of n_pts points, the first E edges are kept"""
    if E == BIG_E[0] * K_CASE:
        return BIG_E
    nq = -(-E // K_CASE)
    return (max(nq, N_PTS_CASE), max(nq, N_PTS_CASE)) if same else (nq, N_PTS_CASE)


def case_inputs(D, E, seed, same):
    """unit-normalised Gaussian embeddings, BatchNorm parameters and state, upstream gradients (CPU tensors)"""
    g = torch.Generator().manual_seed(seed)
    nq, n_pts = case_shape(E, same)
    A = torch.nn.functional.normalize(torch.randn(nq, D, generator=g))
    B = A if same else torch.nn.functional.normalize(torch.randn(n_pts, D, generator=g))
    gamma = float(0.5 + torch.rand(1, generator=g))
    beta = float(torch.randn(1, generator=g) * 0.3)
    rm = float(0.5 + 0.2 * torch.randn(1, generator=g))
    rv = float(0.05 + 0.1 * torch.rand(1, generator=g))
    g_w = torch.randn(E, generator=g)
    g_l = torch.randn(E, generator=g)
    return dict(A=A, B=B, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, nbt=3, g_w=g_w, g_logits=g_l)


def knn_cpu(q, p, k, chunk=8192):
    """the k nearest points of every query (float64 distances), all within any radius > 2"""
    out = []
    p64 = p.double()
    for s in range(0, q.shape[0], chunk):
        d2 = torch.cdist(q[s:s + chunk].double(), p64) ** 2
        out.append(torch.topk(d2, k, dim=1, largest=False, sorted=True).indices)
    return torch.cat(out)


def case_graph(idx, E):
    """the first E edges of the (non-symmetrised) graph of a full kNN result"""
    nq, k = idx.shape
    src = torch.arange(nq, device=idx.device).unsqueeze(1).expand(nq, k).reshape(-1)
    return torch.stack([src, idx.reshape(-1)])[:, :E].contiguous()
