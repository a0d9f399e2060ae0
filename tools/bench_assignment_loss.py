#!/usr/bin/env python3
"""The assignment loss (hierarchicalgnn_amd.assignment) at config-3 size: synth.assignment_event(120k hits, 10k
clusters, k = 5), about 12k particles and 290k distinct (particle, cluster) pairs.

    python tools/bench_assignment_loss.py [--reps 7] [--out FILE.json]

  loss_forward_ms    (a) median wall time of one bipartite_loss forward, all of its host reads included
  matching_ms        (b) median device-event time of one max_weight_matching call (contraction + auction)
  reference_route_ms (c) median wall time of the reference's route on this host: scores and ids .cpu(), scipy CSR
                     build, min_weight_full_bipartite_matching(maximize=True), the matching copied back
  speedup            (c) / (a); the goal is > 1, both measured in this one process
and the matching's phases, grid rounds (idle launches included), tail rounds and host reads.  One warm-up call before
every series.  Run under ``rocprofv3 --kernel-trace --stats`` for the per-kernel times.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import hierarchicalgnn_amd as H
from hierarchicalgnn_amd import assignment, synth

HP = {"weight_leak": 0.1, "ptcut": 1.0, "pt_interval": 0.5, "weight_min": 0.1, "log_weight_ratio": 0.0}


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _wall_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return _median(out), out


def _device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e))
    return _median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--hits", type=int, default=120_000)
    ap.add_argument("--clusters", type=int, default=10_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import min_weight_full_bipartite_matching
    dev = torch.device("cuda:0")
    ev = synth.assignment_event(args.hits, args.clusters, 5)
    batch = {"pid": ev["pid"].to(dev), "pt": ev["pt"].to(dev)}
    graph, scores = ev["bipartite_graph"].to(dev), ev["scores"].to(dev)
    original_pid, pid = torch.unique(batch["pid"], return_inverse=True)
    P, C = int(original_pid.numel()), int(graph[1].max()) + 1
    row = pid[graph[0]]
    res = {"device": torch.cuda.get_device_name(0), "hits": args.hits, "particles": P, "clusters": C,
           "edges": int(graph.shape[1]), "reps": args.reps}

    res["loss_forward_ms"], res["loss_forward_all_ms"] = _wall_ms(
        lambda: H.bipartite_loss(scores, graph, batch, HP), args.reps)
    res["loss_host_reads"] = assignment.stats["host_reads"]
    res["matching_ms"], res["matching_all_ms"] = _device_ms(
        lambda: H.max_weight_matching(row, graph[1], scores, P, C), args.reps)
    res.update({k: assignment.stats[k] for k in ("n_pairs", "phases", "grid_rounds", "tail_rounds")})
    res["matching_host_reads"] = assignment.stats["host_reads"]
    col_match = H.max_weight_matching(row, graph[1], scores, P, C)[0]

    def reference_route():
        # bipartite_classification_base.py:164-175
        m = csr_matrix(
            (torch.cat([scores, 1e-12 * torch.ones(P, device=dev)], dim=0).cpu().numpy(),
             (torch.cat([row, torch.arange(P, device=dev)], dim=0).cpu().numpy(),
              torch.cat([graph[1], torch.arange(C, C + P, device=dev)], dim=0).cpu().numpy())),
            shape=(P, C + P))
        rm, cm = min_weight_full_bipartite_matching(m, maximize=True)
        return torch.tensor(rm, device=dev).long(), torch.tensor(cm, device=dev).long(), m

    res["reference_route_ms"], res["reference_route_all_ms"] = _wall_ms(reference_route, max(3, args.reps // 2))
    rm, cm, m = reference_route()
    ours = np.array(col_match.cpu().numpy())
    res["total_ours"] = float(np.asarray(m[np.arange(P), ours]).sum())
    res["total_scipy"] = float(np.asarray(m[np.array(rm.cpu().numpy()), np.array(cm.cpu().numpy())]).sum())
    res["gap_bound"] = H.gap_bound(P, C, float(m.max()))
    res["speedup"] = res["reference_route_ms"] / res["loss_forward_ms"]
    res["goal_met"] = res["loss_forward_ms"] < res["reference_route_ms"]
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
