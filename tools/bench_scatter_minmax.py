#!/usr/bin/env python3
"""scatter_max / scatter_min (hgnn_segment_reduce_ex) on the headline event, with K1 (scatter_add) on the same plan.

    python tools/bench_scatter_minmax.py [--out FILE.json]

Cases:
  max_f32_L256   scatter_max of [M, 256] fp32 rows over graph[1] (M = 2 x 1M directed edges, N = 120k)
  max_bf16_L256  the same rows in bf16
  k1_f32_L256    scatter_add of the fp32 rows on the same plan (K1, for comparison)
  min_f32_bc     scatter_min(pt, pid) of the BC loss: 120k hits, ~10k particles, F = 1
Call time is the median of device-event timings around one call; run under
``rocprofv3 --kernel-trace --stats`` for kernel times.  Algorithmic bytes: src read + out write (+ int64 arg write
for min / max; + int32 index read for K1, as tools/bench_k1_widths.py counts it), share of an 8 TB/s HBM peak.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import hierarchicalgnn_amd as H
from hierarchicalgnn_amd import synth

PEAK = 8e12


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return ts[len(ts) // 2]


def row(ms, nbytes, **kw):
    return dict(kw, ms=ms, alg_bytes=nbytes, GBps=nbytes / ms / 1e6, frac_of_8TBps=nbytes / (ms * 1e-3) / PEAK)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    res = {"device": torch.cuda.get_device_name(0)}
    _, ei = synth.trackml_event()
    graph = synth.directed(ei).cuda()
    N, M, L = 120_000, int(graph.shape[1]), 256
    idx = graph[1]
    plan = H.get_plan(idx, N)
    res["event"] = dict(M=M, N=N, chunk=plan.chunk, **plan.counts_host())
    src = torch.randn(M, L, device="cuda")
    ms = timed(lambda: H.scatter_max(src, idx, dim=0, dim_size=N, plan=plan))
    res["max_f32_L256"] = row(ms, 4 * M * L + 4 * N * L + 8 * N * L)
    ms = timed(lambda: H.scatter_add(src, idx, dim_size=N, plan=plan))
    res["k1_f32_L256"] = row(ms, 4 * L * M + 4 * M + 4 * L * N)
    src = src.bfloat16()
    ms = timed(lambda: H.scatter_max(src, idx, dim=0, dim_size=N, plan=plan))
    res["max_bf16_L256"] = row(ms, 2 * M * L + 2 * N * L + 8 * N * L)
    del src
    g = torch.Generator().manual_seed(0)
    pid_raw = (torch.randint(0, 10_000, (120_000,), generator=g) * 7919).cuda()
    pt = torch.rand(120_000, generator=g).cuda()
    _, pid, _ = torch.unique(pid_raw, return_inverse=True, return_counts=True)
    n_p = int(pid.max()) + 1
    bc_plan = H.get_plan(pid, n_p)
    ms = timed(lambda: H.scatter_min(pt, pid, dim=0, dim_size=n_p, plan=bc_plan))
    res["min_f32_bc"] = row(ms, 4 * 120_000 + 4 * n_p + 8 * n_p, hits=120_000, particles=n_p)
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
