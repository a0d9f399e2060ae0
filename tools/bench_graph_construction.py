#!/usr/bin/env python3
"""DynamicGraphConstruction's two routes against each other, in one process: "torch" (boolean-mask compaction,
torch.unique, edge_dot + BatchNorm1d + weighting as ATen launches -- the default) and "fused" (ops.knn_edges,
graph_construction.attention_weights; csrc/graphcon.hip).

    python tools/bench_graph_construction.py [--hits 120000] [--clusters 10000] [--rounds 15] [--warmup 3] [--out FILE]

Seeded inputs: `clusters` unit-normalised Gaussian centroids in 8 dimensions, `hits` points around them; radius 1.0, so
the bipartite graph (k = 5) has 5 `hits` edges and the super graph (k = 10, sym) is the union of both directions.

  build_graph      the whole call, neighbour search included (it is the same kernel in both routes), eval mode
  edges            the stage that differs: kNN result -> edge list, on a fixed kNN result
  weights_eval     edge_weights forward, eval mode, norm, on the fixed graph
  weights_train    edge_weights forward + backward (d/d both embeddings and the BatchNorm parameters), training mode

Each case: `warmup` untimed rounds, then `rounds` rounds with the two routes alternating inside every round.  Per call
and route the median and min .. max of the device-event time and of the wall time (host reads stall the host, which
only the wall time shows).  host_syncs: host reads of one call as torch.cuda.set_sync_debug_mode("warn") counts them;
fused_reads: what graph_construction.stats["host_reads"] counted.  gain_counts: the project's rule -- the difference
of the medians must exceed 3 x the larger min .. max spread, for the wall time."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
from hierarchicalgnn_amd import graph_construction as G
from hierarchicalgnn_amd.graph_construction import DynamicGraphConstruction, find_neighbors


def _timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end), (time.perf_counter() - t0) * 1e3


def _syncs(fn):
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    return sum("synchroniz" in str(w.message).lower() for w in rec)


def _summary(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def _compare(case, routes, rounds, warmup, extra):
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    times = {r: ([], []) for r in routes}
    reads = {}
    for _ in range(rounds):                              # alternate inside the round, so that drift hits both alike
        for r, fn in routes.items():
            before = G.stats["host_reads"]
            dev_ms, wall_ms = _timed(fn)
            reads[r] = G.stats["host_reads"] - before
            times[r][0].append(dev_ms)
            times[r][1].append(wall_ms)
    row = dict(case=case, rounds=rounds, **extra)
    for r in routes:
        row[r + "_device_ms"] = _summary(times[r][0])
        row[r + "_wall_ms"] = _summary(times[r][1])
        row[r + "_host_syncs"] = _syncs(routes[r])
    row["fused_reads"] = reads["fused"]
    t, f = row["torch_wall_ms"], row["fused_wall_ms"]
    spread = max(t["max"] - t["min"], f["max"] - f["min"])
    row["wall_gain_ms"] = t["median"] - f["median"]
    row["gain_counts"] = bool(row["wall_gain_ms"] > 3 * spread)
    print(json.dumps(row), flush=True)
    return row


def _modules(fn, dev, training):
    out = {}
    for route in ("torch", "fused"):
        m = DynamicGraphConstruction(fn, {"graph_construction": route}).to(dev).train(training)
        m.knn_radius.fill_(1.0)
        out[route] = m
    return out


def _graph_cases(name, src, dst, sym, k, fn, rounds, warmup):
    dev = src.device
    rows = []
    mods = _modules(fn, dev, False)
    with torch.no_grad():
        idx = find_neighbors(src, dst, r_max=mods["torch"].knn_radius, k_max=k)
        graph = mods["torch"].build_graph(src, dst, sym=sym, k=k)
        assert torch.equal(graph, mods["fused"].build_graph(src, dst, sym=sym, k=k))
    shape = dict(nq=int(src.shape[0]), n_pts=int(dst.shape[0]), k=k, sym=sym, edges=int(graph.shape[1]))

    def build(route):
        def fn_():
            with torch.no_grad():
                mods[route].build_graph(src, dst, sym=sym, k=k)
        return fn_

    rows.append(_compare(name + ".build_graph", {r: build(r) for r in mods}, rounds, warmup, shape))

    n = max(src.shape[0], dst.shape[0])

    def edges_torch():
        positive = idx >= 0
        ind = torch.arange(idx.shape[0], device=dev).unsqueeze(1).expand(idx.shape)
        if sym:
            return torch.stack(G.symmetrize(ind[positive], idx[positive], n), dim=0)
        return torch.stack([ind[positive], idx[positive]], dim=0)

    rows.append(_compare(name + ".edges", {"torch": edges_torch,
                                           "fused": lambda: G.knn_edges(idx, int(dst.shape[0]), sym=sym)},
                         rounds, warmup, shape))

    def weights_eval(route):
        def fn_():
            with torch.no_grad():
                mods[route].edge_weights(src, dst, graph, norm=True)
        return fn_

    rows.append(_compare(name + ".weights_eval", {r: weights_eval(r) for r in mods}, rounds, warmup, shape))

    train = _modules(fn, dev, True)
    a = src.clone().requires_grad_(True)
    b = a if sym else dst.clone().requires_grad_(True)
    up = torch.randn(graph.shape[1], 1, generator=torch.Generator().manual_seed(1)).to(dev)

    def weights_train(route):
        def fn_():
            a.grad = b.grad = None
            w = train[route].edge_weights(a, b, graph, norm=True)
            (w * up).sum().backward()
        return fn_

    rows.append(_compare(name + ".weights_train", {r: weights_train(r) for r in train}, rounds, warmup, shape))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=120_000)
    ap.add_argument("--clusters", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 9:
        raise SystemExit("bench_graph_construction: at least 9 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_graph_construction needs an MI355X: there is no CPU path and no fallback")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(a.hits + a.clusters)
    means = torch.nn.functional.normalize(torch.randn(a.clusters, 8, generator=g))
    member = torch.randint(0, a.clusters, (a.hits,), generator=g)
    hits = torch.nn.functional.normalize(means[member] + 0.1 * torch.randn(a.hits, 8, generator=g))
    means, hits = means.to(dev), hits.to(dev)
    rows = _graph_cases("bipartite", hits, means, False, 5, "exp", a.rounds, a.warmup)
    rows += _graph_cases("super", means, means, True, 10, "sigmoid", a.rounds, a.warmup)
    result = dict(tool="tools/bench_graph_construction.py", device=torch.cuda.get_device_name(0),
                  command="python tools/bench_graph_construction.py --hits %d --clusters %d --rounds %d --warmup %d"
                  % (a.hits, a.clusters, a.rounds, a.warmup), rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
