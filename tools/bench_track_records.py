#!/usr/bin/env python3
"""track_records (hgnn_track_records, csrc/trackeval_records.hip) next to eval_metrics on the headline synthetic
event, and eval_metrics on the library of the commit before it.

    python tools/bench_track_records.py [--parent-lib PATH/libhgnn_hip.so] [--repeats 9] [--inner 20] [--out FILE]

Event: synth.tracking_event (N = 120k hits, ~10 hits per particle, 10 % noise) and synth.track_candidates
(B = 600k pairs, 10k candidates), primary=False as every reference training base calls it.  Variants, each ONE full
Python call including its workspace allocation and its one host read of the 12-double result (what a validation
step pays):
  eval_metrics           this commit
  eval_metrics_parent    the same Python call on the parent commit's library (``--parent-lib``, built from a checkout
                         of that commit; the binding is swapped in this process, so both run alternated).  The
                         Python wrapper of eval_metrics differs from the parent's only by a shared argument check
  track_records_v0       no binning variable
  track_records_v2       two variables (pt, eta) of 20 bins
Method: wall time around ``--inner`` back-to-back calls (every call ends in its host read, so the device is idle at
both ends), every variant warmed up first, the variants ALTERNATED inside each of ``--repeats`` rounds, one process;
per variant the median per-call time and the spread (min, max) over the rounds.  Verdicts by the project's rule: two
medians differ when they are more than 3 x the larger spread apart.  Writes profiles/track_records_bench.json.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import hierarchicalgnn_amd as H
from hierarchicalgnn_amd import _lib, synth, tracking


def _parent_handle(path):
    """the parent commit's library with the two entries eval_metrics uses bound as this commit binds them"""
    lib = ctypes.CDLL(path)
    for name in ("hgnn_track_eval_workspace_bytes", "hgnn_track_eval", "hgnn_last_error"):
        res, args = _lib._SIGNATURES[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_records_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    ev_cpu = synth.tracking_event(120_000)
    bg = synth.track_candidates(ev_cpu["pid"], 600_000, 10_000).cuda()
    ev = {k: v.cuda() for k, v in ev_cpu.items()}
    g = torch.Generator().manual_seed(5)
    ev["eta"] = (torch.randn(120_000, generator=g) * 1.5).cuda()
    kw = dict(pt_cut=1.0, nhits_cut=5, majority_cut=0.5, primary=False)
    bins = {"pt": ("pt", [0.25 * k for k in range(21)]), "eta": ("eta", [-4.0 + 0.4 * k for k in range(21)])}
    here = _lib.load()
    parent = _parent_handle(args.parent_lib) if args.parent_lib else None

    def on_parent():
        _lib._lib = parent
        try:
            return H.eval_metrics(bg, ev, **kw)
        finally:
            _lib._lib = here

    variants = {"eval_metrics": lambda: H.eval_metrics(bg, ev, **kw)}
    if parent is not None:
        variants["eval_metrics_parent"] = on_parent
    variants["track_records_v0"] = lambda: H.track_records(bg, ev, None, **kw)
    variants["track_records_v2"] = lambda: H.track_records(bg, ev, bins, **kw)

    last = {}
    for name, fn in variants.items():
        for _ in range(5):
            last[name] = fn()
    rounds = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(args.inner):
                fn()
            rounds[name].append((time.perf_counter() - t) * 1e3 / args.inner)
    res = {}
    for name, r in rounds.items():
        r = sorted(r)
        res[name] = dict(median_ms=round(r[len(r) // 2], 4), min_ms=round(r[0], 4), max_ms=round(r[-1], 4))

    def verdict(x, y):
        spread = max(res[x]["max_ms"] - res[x]["min_ms"], res[y]["max_ms"] - res[y]["min_ms"])
        diff = res[y]["median_ms"] - res[x]["median_ms"]
        return dict(y_minus_x_ms=round(diff, 4), larger_spread_ms=round(spread, 4),
                    differs_by_more_than_3_spreads=abs(diff) > 3 * spread)

    rec = last["track_records_v2"]
    same = all(tracking_same(last["eval_metrics"][k], out["metrics"][k])
               for out in (last["track_records_v0"], rec) for k in last["eval_metrics"])
    doc = dict(device=torch.cuda.get_device_name(0), N=120_000, B=int(bg.shape[1]), repeats=args.repeats,
               inner=args.inner,
               method="wall time per full Python call (allocation and the one host read included), variants "
                      "alternated inside each repeat, median (min, max) over the repeats",
               ms=res, metrics=last["eval_metrics"], counts=rec["counts"], metrics_equal=same,
               pt_efficiency=[None if x != x else round(x, 4) for x in
                              (rec["bins"]["pt"]["counts"][:, 3].double() /
                               rec["bins"]["pt"]["counts"][:, 1].double()).tolist()],
               cost_of_records={"v0_over_eval_metrics": verdict("eval_metrics", "track_records_v0"),
                                "v2_over_eval_metrics": verdict("eval_metrics", "track_records_v2")})
    if parent is not None:
        doc["eval_metrics_against_parent"] = verdict("eval_metrics_parent", "eval_metrics")
        doc["parent_metrics_equal"] = all(tracking_same(last["eval_metrics"][k], last["eval_metrics_parent"][k])
                                          for k in last["eval_metrics"])
    txt = json.dumps(doc, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


def tracking_same(a, b):
    return a == b or (a != a and b != b)


if __name__ == "__main__":
    main()
