#!/usr/bin/env python3
"""eval_metrics (hgnn_track_eval, csrc/trackeval.hip) on the headline synthetic event, next to the CPU restatement.

    python tools/bench_tracking_eval.py [--reps 50] [--out FILE.json]

Event: synth.tracking_event (N = 120k hits, ~10 hits per particle, 10 % noise) and synth.track_candidates
(B = 600k pairs, 10k candidates), primary=False as every reference training base calls it.
  device_ms   median of device-event timings around one hgnn_track_eval launch sequence (no host read)
  call_ms     median wall time of one full H.eval_metrics call, including the workspace allocation and the one
              host read of the 12-double result (what a validation step pays)
  cpu_ms      one call of the numpy restatement (tests/tracking_ref.py) on the host, for scale
Run under ``rocprofv3 --kernel-trace --stats`` for the per-kernel times.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import hierarchicalgnn_amd as H
from hierarchicalgnn_amd import synth, tracking


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    ev_cpu = synth.tracking_event(120_000)
    bg_cpu = synth.track_candidates(ev_cpu["pid"], 600_000, 10_000)
    ev = {k: v.cuda() for k, v in ev_cpu.items()}
    bg = bg_cpu.cuda()
    kw = dict(pt_cut=1.0, nhits_cut=5, majority_cut=0.5, primary=False)
    res = {"device": torch.cuda.get_device_name(0), "N": 120_000, "B": int(bg.shape[1]),
           "candidates": int(torch.unique(bg[1]).numel())}
    for _ in range(5):
        out = H.eval_metrics(bg, ev, **kw)
    torch.cuda.synchronize()
    dev = []
    for _ in range(args.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        tracking.track_eval(bg, ev, 1.0, 5, 0.5, False)
        e.record()
        torch.cuda.synchronize()
        dev.append(s.elapsed_time(e))
    wall = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = H.eval_metrics(bg, ev, **kw)
        wall.append((time.perf_counter() - t) * 1e3)
    dev.sort()
    wall.sort()
    res["device_ms"] = dev[len(dev) // 2]
    res["call_ms"] = wall[len(wall) // 2]
    res["call_ms_min"] = wall[0]
    res["metrics"] = out
    import tracking_ref as T
    t = time.perf_counter()
    ref = T.track_eval(bg_cpu[0].numpy(), bg_cpu[1].numpy(), ev_cpu["pid"].numpy(), ev_cpu["pt"].numpy(), None,
                       1.0, 5, 0.5)
    res["cpu_ms"] = (time.perf_counter() - t) * 1e3
    res["cpu_metrics"] = {k: ref[k] for k in T.KEYS}
    res["goal_ms"] = 2.0
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
