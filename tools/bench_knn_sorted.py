#!/usr/bin/env python3
"""The embedding stage's kNN by both methods of ops.knn_radius at the reference's size.

    python tools/bench_knn_sorted.py [--out profiles/knn_sorted_bench.json]

Inputs as tools/bench_embedding_samples.py: N = 120k self-queries, D = 8, K = 100, r = 1 on clustered
(synth.embedding_event) and on uniform unit embeddings.  Both methods run in ONE process, alternating; per method and
distribution the median device time of 7 calls after a warm-up and the spread (max - min) of those 7.  The sorted call
is timed whole: bounding box, keys, sort, gather and search.  `stats` = (tiles visited, tiles skipped) of the sorted
call summed over its workgroups; `equal` = the two methods' idx and d2 are bitwise equal.  One more shape, the
bipartite graph's: 120k queries against 10k points, K = 5.
`switch_default` applies the rule of DESIGN.md Appendix A to frnn_graph's default (K >= 33, nq >= 65536): the sorted
call beats the brute-force one at BOTH distributions by more than 3x the larger spread.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from hierarchicalgnn_amd import synth
from hierarchicalgnn_amd.ops import knn_radius, knn_radius_stats

REPS = 7


def _time_once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def _both(q, p, K, r):
    """{method: (median ms, spread ms)} with the two methods alternating, stats of the sorted call, equality"""
    fns = {m: (lambda m=m: knn_radius(q, p, K, r, return_dist2=True, method=m)) for m in ("brute", "sorted")}
    outs = {}
    for m, fn in fns.items():
        for _ in range(2):
            outs[m] = fn()
    torch.cuda.synchronize()
    stats = knn_radius_stats()
    equal = bool(torch.equal(outs["brute"][0], outs["sorted"][0]) and torch.equal(outs["brute"][1], outs["sorted"][1]))
    del outs
    times = {m: [] for m in fns}
    for _ in range(REPS):
        for m, fn in fns.items():
            times[m].append(_time_once(fn))
    res = {}
    for m, t in times.items():
        t.sort()
        res[f"{m}_ms"] = t[len(t) // 2]
        res[f"{m}_spread_ms"] = t[-1] - t[0]
    res["tiles_visited"], res["tiles_skipped"] = stats
    res["skipped_share"] = stats[1] / max(1, stats[0] + stats[1])
    res["equal"] = equal
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_sorted_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    n = 120_000
    clustered = synth.embedding_event(n)["embeddings"].to(dev)
    g = torch.Generator().manual_seed(2)
    uniform = torch.nn.functional.normalize(torch.randn(n, 8, generator=g)).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "N": n, "D": 8, "K": 100, "r": 1.0, "reps": REPS,
           "goal_frnn_ms": 8.0}
    for name, emb in (("clustered", clustered), ("uniform", uniform)):
        res[name] = _both(emb, emb, 100, 1.0)
    g = torch.Generator().manual_seed(3)
    sel = torch.randperm(n, generator=g)[:10_000].to(dev)
    res["bipartite_120k_x_10k_K5"] = _both(clustered, clustered[sel].contiguous(), 5, 1.0)
    big = ("clustered", "uniform")
    spread = max(res[d][f"{m}_spread_ms"] for d in big for m in ("brute", "sorted"))
    res["largest_spread_ms"] = spread
    res["goal_met_sorted"] = all(res[d]["sorted_ms"] <= 8.0 for d in big)
    res["goal_met_brute"] = all(res[d]["brute_ms"] <= 8.0 for d in big)
    res["switch_default"] = all(res[d]["brute_ms"] - res[d]["sorted_ms"] > 3 * spread for d in big)
    txt = json.dumps(res, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
