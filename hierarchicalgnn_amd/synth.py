"""Synthetic TrackML-1GeV-shaped events (no dataset is reachable offline).

Shape contract (SURVEY.md section 8d / BASELINE.md section 4): ``N`` hits on 10
concentric barrel layers with per-hit ``x = (r, phi, z)`` scaled to O(1);
``E`` undirected candidate edges joining hits on adjacent layers inside a
(delta-phi) window, mean directed in-degree 2E/N ~ 16.7 with a tail; the
columns of ``edge_index`` are SHUFFLED (stored TrackML graphs are not sorted by
destination).  The model doubles the graph to ``M = 2E`` directed rows
(reference EdgeClassifier/Models/IN.py:122).  Seeds: 1234 topology, 1235
features, 1236 weights.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch

N_LAYERS = 10


def trackml_event(n_hits: int = 120_000, n_edges: int = 1_000_000, seed: int = 1234,
                  hub_fraction: float = 0.01, hub_boost: int = 6) -> Tuple[torch.Tensor, torch.Tensor]:
    """returns (x[N,3] float32, edge_index[2,E] int64) on the CPU"""
    g = torch.Generator().manual_seed(seed)
    layer = torch.randint(0, N_LAYERS, (n_hits,), generator=g)
    phi = torch.rand(n_hits, generator=g) * 2 - 1
    z = torch.randn(n_hits, generator=g).clamp_(-3, 3) / 3
    x = torch.stack([(layer.float() + 1) / N_LAYERS, phi, z], dim=1).contiguous()

    n_src_hits = int((layer < N_LAYERS - 1).sum())
    mean_fanout = n_edges / max(n_src_hits, 1) * 1.15  # oversample, trimmed below
    srcs, dsts = [], []
    for l in range(N_LAYERS - 1):
        a = torch.nonzero(layer == l).squeeze(1)
        b = torch.nonzero(layer == l + 1).squeeze(1)
        if a.numel() == 0 or b.numel() == 0:
            continue
        b = b[torch.argsort(phi[b])]
        pos = torch.searchsorted(phi[b].contiguous(), phi[a].contiguous())
        # per-hit fan-out: Poisson-ish body plus a few "hub" hits (dense jets) for the degree tail
        fan = torch.poisson(torch.full((a.numel(),), mean_fanout), generator=g).long().clamp_(min=1)
        hub = torch.rand(a.numel(), generator=g) < hub_fraction
        fan = torch.where(hub, fan * hub_boost, fan).clamp_(max=b.numel())
        rep = torch.repeat_interleave(torch.arange(a.numel()), fan)
        start = torch.cumsum(fan, 0) - fan
        k = torch.arange(rep.numel()) - start[rep]                 # 0..fan-1 within each hit
        off = k - fan[rep] // 2                                    # window centred on the phi match
        partner = b[(pos[rep] + off) % b.numel()]
        srcs.append(a[rep])
        dsts.append(partner)
    src = torch.cat(srcs)
    dst = torch.cat(dsts)
    perm = torch.randperm(src.numel(), generator=g)
    if src.numel() >= n_edges:
        perm = perm[:n_edges]
    else:  # pad by repeating random edges (keeps shape exact)
        extra = torch.randint(0, src.numel(), (n_edges - src.numel(),), generator=g)
        perm = torch.cat([perm, extra])
    # random orientation so that both rows carry hubs, then the shuffle above is the column order
    flip = torch.rand(perm.numel(), generator=g) < 0.5
    s, d = src[perm], dst[perm]
    edge_index = torch.stack([torch.where(flip, d, s), torch.where(flip, s, d)]).contiguous()
    return x, edge_index


def directed(edge_index: torch.Tensor) -> torch.Tensor:
    """the doubling the model applies (IN.py:122 / HGNN_GMM.py:328)"""
    return torch.cat([edge_index, edge_index.flip(0)], dim=1)


def bipartite_assignment(n_hits: int, n_super: int = 10_000, k: int = 5, seed: int = 1234):
    """HGNN extras: B = N*k bipartite edges hit -> supernode with cluster-size skew,
    weights exp(N(0,1))/mean; returns (bipartite_graph[2,B] int64, weights[B,1] float32)"""
    g = torch.Generator().manual_seed(seed + 7)
    # heavy-tailed cluster popularity (Zipf-like) => supernode fan-in skew
    pop = 1.0 / torch.arange(1, n_super + 1, dtype=torch.float64) ** 0.7
    pop = pop[torch.randperm(n_super, generator=g)]
    sn = torch.multinomial(pop, n_hits * k, replacement=True, generator=g)
    hit = torch.arange(n_hits).repeat_interleave(k)
    w = torch.exp(torch.randn(n_hits * k, 1, generator=g))
    w = (w / w.mean()).float()
    shuffle = torch.randperm(n_hits * k, generator=g)
    return torch.stack([hit[shuffle], sn[shuffle]]).contiguous(), w[shuffle].contiguous()


def super_graph(n_super: int = 10_000, k: int = 10, seed: int = 1234):
    g = torch.Generator().manual_seed(seed + 11)
    s0 = torch.arange(n_super).repeat_interleave(k)
    s1 = torch.randint(0, n_super, (n_super * k,), generator=g)
    sg = torch.unique(torch.stack([torch.cat([s0, s1]), torch.cat([s1, s0])]), dim=1)
    sg = sg[:, torch.randperm(sg.shape[1], generator=g)].contiguous()
    w = torch.sigmoid(torch.randn(sg.shape[1], 1, generator=g))
    return sg, (w / w.mean()).float().contiguous()


def degree_stats(index: torch.Tensor, n: int):
    deg = torch.bincount(index, minlength=n)
    return dict(mean=float(deg.float().mean()), max=int(deg.max()), median=float(deg.float().median()),
                zero=int((deg == 0).sum()))


def tracking_event(n_hits: int = 120_000, hits_per_particle: int = 10, noise_fraction: float = 0.1,
                   primary_fraction: float = 0.9, seed: int = 1234):
    """TrackML-shaped truth for the tracking metrics (reference tracking_utils.eval_metrics): returns a dict
    {pid int64[N] (0 = noise, the rest large distinct ids), pt float32[N] (GeV, per particle with a small per-hit
    spread; 0 on noise, as the training bases set it), primary int64[N] (per particle)} on the CPU"""
    g = torch.Generator().manual_seed(seed + 13)
    n_noise = int(round(n_hits * noise_fraction))
    n_sig = n_hits - n_noise
    n_part = max(1, n_sig // hits_per_particle)
    part = torch.randint(0, n_part, (n_sig,), generator=g)          # ~Poisson(hits_per_particle) hits per particle
    ids = ((torch.randperm(n_part, generator=g) + 1) << 20) | torch.randint(0, 1 << 20, (n_part,), generator=g)
    pt_p = 0.2 - torch.log(torch.rand(n_part, generator=g).clamp_(min=1e-12))
    prim_p = (torch.rand(n_part, generator=g) < primary_fraction).long()
    pid = torch.cat([ids[part], torch.zeros(n_noise, dtype=torch.long)])
    pt = torch.cat([pt_p[part] * (1 + 0.02 * torch.rand(n_sig, generator=g)), torch.zeros(n_noise)]).float()
    primary = torch.cat([prim_p[part], torch.zeros(n_noise, dtype=torch.long)])
    perm = torch.randperm(n_hits, generator=g)
    return {"pid": pid[perm].contiguous(), "pt": pt[perm].contiguous(), "primary": primary[perm].contiguous()}


def track_candidates(pid: torch.Tensor, n_pairs: int = 600_000, n_candidates: int = 10_000,
                     clean_fraction: float = 0.8, hit_loss: float = 0.1, seed: int = 1234) -> torch.Tensor:
    """a hit -> track-candidate bipartite graph int64[2, ~n_pairs] for the event truth `pid`: clean candidates
    (a seed particle's hits, each lost with `hit_loss`, plus ~2 foreign hits; a particle may seed two) and large
    junk candidates that take the rest of the pair budget as random hits.  Labels are arbitrary vertex-like ids."""
    g = torch.Generator().manual_seed(seed + 17)
    n = pid.numel()
    uniq, q = torch.unique(pid, return_inverse=True)
    sig = torch.nonzero(pid != 0).reshape(-1)
    signal = torch.nonzero(uniq != 0).reshape(-1)
    n_clean = int(n_candidates * clean_fraction)
    seed_p = signal[torch.randint(0, signal.numel(), (n_clean,), generator=g)]
    cnt = torch.bincount(seed_p, minlength=uniq.numel())
    order = torch.argsort(seed_p, stable=True)
    off = torch.cumsum(cnt, 0) - cnt
    reps = cnt[q[sig]]
    h = torch.repeat_interleave(sig, reps)
    k = torch.arange(h.numel()) - torch.repeat_interleave(torch.cumsum(reps, 0) - reps, reps)
    c = order[off[q[h]] + k]
    keep = torch.rand(h.numel(), generator=g) >= hit_loss
    h, c = h[keep], c[keep]
    n_extra = 2 * n_clean
    h = torch.cat([h, torch.randint(0, n, (n_extra,), generator=g)])
    c = torch.cat([c, torch.randint(0, n_clean, (n_extra,), generator=g)])
    rest = n_pairs - h.numel()
    if rest > 0 and n_candidates > n_clean:
        h = torch.cat([h, torch.randint(0, n, (rest,), generator=g)])
        c = torch.cat([c, torch.randint(n_clean, n_candidates, (rest,), generator=g)])
    labels = torch.randperm(max(n, n_candidates), generator=g)[:n_candidates]
    perm = torch.randperm(h.numel(), generator=g)
    return torch.stack([h[perm], labels[c[perm]]]).contiguous()


def embedding_event(n_hits: int = 120_000, emb_dim: int = 8, hits_per_particle: int = 10, spread: float = 0.1,
                    noise_fraction: float = 0.1, seed: int = 1234):
    """An event for the embedding stage's pair construction (GNNEmbedding/embedding_base.py:109-146): returns a
    dict of CPU tensors {embeddings float32 [N, emb_dim] unit vectors clustered by particle (centre + spread * noise,
    normalised; noise hits uniform on the sphere), pid int64 [N] (0 = noise), pt float32 [N] (GeV; 0 on noise),
    signal_mask bool [N] (~95 % true), modulewise_true_edges int64 [2, E] (consecutive hits of every particle)}"""
    g = torch.Generator().manual_seed(seed + 19)
    n_noise = int(round(n_hits * noise_fraction))
    n_sig = n_hits - n_noise
    n_part = max(1, n_sig // hits_per_particle)
    part = torch.randint(0, n_part, (n_sig,), generator=g)
    centres = torch.nn.functional.normalize(torch.randn(n_part, emb_dim, generator=g), dim=1)
    sig = torch.nn.functional.normalize(centres[part] + spread * torch.randn(n_sig, emb_dim, generator=g), dim=1)
    noise = torch.nn.functional.normalize(torch.randn(n_noise, emb_dim, generator=g), dim=1)
    pt_p = 0.2 - torch.log(torch.rand(n_part, generator=g).clamp_(min=1e-12))
    emb = torch.cat([sig, noise])
    pid = torch.cat([part + 1, torch.zeros(n_noise, dtype=torch.long)])
    pt = torch.cat([pt_p[part], torch.zeros(n_noise)]).float()
    perm = torch.randperm(n_hits, generator=g)
    emb, pid, pt = emb[perm].contiguous(), pid[perm].contiguous(), pt[perm].contiguous()
    signal_mask = torch.rand(n_hits, generator=g) >= 0.05
    # truth: the hits of every particle in index order, consecutive ones joined
    order = torch.argsort(pid * n_hits + torch.arange(n_hits), stable=True)
    p_sorted = pid[order]
    same = (p_sorted[1:] == p_sorted[:-1]) & (p_sorted[1:] != 0)
    edges = torch.stack([order[:-1][same], order[1:][same]])
    return {"embeddings": emb, "pid": pid, "pt": pt, "signal_mask": signal_mask,
            "modulewise_true_edges": edges.contiguous()}


def assignment_event(n_hits: int = 120_000, n_super: int = 10_000, k: int = 5, seed: int = 1234, dyadic: bool = False):
    """An event for the assignment loss (BipartiteClassification/bipartite_classification_base.py:152-191): pid and
    pt from ``tracking_event``, the hit -> cluster graph from ``bipartite_assignment`` with the first edge of every
    signal hit rewired to its particle's home cluster, and scores in (0, 1] that favour the home cluster (0.5 .. 1
    there, below 0.6 elsewhere).  ``dyadic``: every score is a multiple of 2^-12 in [2^-12, 1], so that sums of
    scores are exact in float32 and float64 alike.  Returns a dict of CPU tensors {pid int64 [N], pt float32 [N],
    bipartite_graph int64 [2, N*k], scores float32 [N*k]}."""
    ev = tracking_event(n_hits, seed=seed)
    graph, _ = bipartite_assignment(n_hits, n_super, k, seed=seed)
    g = torch.Generator().manual_seed(seed + 23)
    uniq, pidx = torch.unique(ev["pid"], return_inverse=True)
    home = torch.randint(0, n_super, (uniq.numel(),), generator=g)
    first = torch.argsort(graph[0], stable=True)[::k]            # every hit has exactly k edges
    first = first[ev["pid"][graph[0][first]] != 0]
    col = graph[1].clone()
    col[first] = home[pidx[graph[0][first]]]
    u = torch.rand(n_hits * k, generator=g)
    scores = 0.6 * u
    scores[first] = 0.5 + 0.5 * u[first]
    if dyadic:
        scores = (torch.floor(scores * 4096) + 1).clamp_(1, 4096) / 4096
    else:
        scores = scores.clamp_(1e-6, 1 - 1e-6)
    return {"pid": ev["pid"], "pt": ev["pt"], "bipartite_graph": torch.stack([graph[0], col]).contiguous(),
            "scores": scores.float().contiguous()}
