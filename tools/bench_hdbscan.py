#!/usr/bin/env python3
"""GPU HDBSCAN (hierarchicalgnn_amd.hdbscan, csrc/hdbscan.hip) on the synthetic event's embeddings:
synth.embedding_event(120k hits, 8-D unit vectors clustered by particle (--spread 0.02), 10 % noise).

    python tools/bench_hdbscan.py [--hits 120000] [--reps 5] [--sklearn-hits N] [--out FILE.json]

  call_ms        median wall time of one hdbscan() call, every host read and the host tree stage included
  stages         one extra call with stage synchronisation: core distances, every Boruvka round, sort (with the copy
                 of the edges to the host) and the host tree stage, host-clock milliseconds; rounds and host reads
  sklearn_ms     wall time of sklearn HDBSCAN(min_cluster_size=5, algorithm="kd_tree") on the first --sklearn-hits
                 points on this host (one run; 0 skips it), and our call on the SAME points (call_same_points_ms)
  goal_met       call_same_points_ms < sklearn_ms: faster than the host route on the same machine
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import importlib

import torch
import hierarchicalgnn_amd as H
from hierarchicalgnn_amd import synth

hdb = importlib.import_module("hierarchicalgnn_amd.hdbscan")


def _wall_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return sorted(out)[len(out) // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=120_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-cluster-size", type=int, default=5)
    ap.add_argument("--spread", type=float, default=0.02, help="width of a particle's cluster around its centre")
    ap.add_argument("--sklearn-hits", type=int, default=None, help="default: --hits; 0 skips sklearn")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    ev = synth.embedding_event(args.hits, 8, spread=args.spread)
    x = ev["embeddings"].to(dev)
    mcs = args.min_cluster_size
    res = {"device": torch.cuda.get_device_name(0), "hits": args.hits, "dim": 8, "min_cluster_size": mcs,
           "spread": args.spread, "reps": args.reps}
    res["call_ms"], res["call_all_ms"] = _wall_ms(lambda: H.hdbscan(x, mcs), args.reps)
    labels = hdb.hdbscan_tree(x, mcs, stage_sync=True)[0]
    torch.cuda.synchronize()
    res["stages"] = dict(hdb.stats["last"])
    res["noise_points"] = int((labels < 0).sum())
    n_sk = args.hits if args.sklearn_hits is None else args.sklearn_hits
    if n_sk > 0:
        try:
            from sklearn.cluster import HDBSCAN
        except ImportError:
            HDBSCAN = None
            res["sklearn_ms"] = None
        if HDBSCAN is not None:
            pts = ev["embeddings"][:n_sk].double().numpy()
            t = time.perf_counter()
            HDBSCAN(min_cluster_size=mcs, algorithm="kd_tree").fit_predict(pts)
            res["sklearn_ms"] = (time.perf_counter() - t) * 1e3
            res["sklearn_hits"] = n_sk
            xs = x[:n_sk].contiguous()
            res["call_same_points_ms"] = _wall_ms(lambda: H.hdbscan(xs, mcs), 3)[0]
            res["speedup"] = res["sklearn_ms"] / res["call_same_points_ms"]
            res["goal_met"] = res["call_same_points_ms"] < res["sklearn_ms"]
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
