#!/usr/bin/env python3
"""Sweep the K1 rolling-window kernel in one process, variants interleaved.

    python tools/tune_k1_window.py [--build-only] [--rounds R] [--json PATH]

The shipped library holds one variant (window depth, waves per workgroup); this tool builds a second library
from the same sources with -DHGNN_K1_SWEEP (every depth in {8,16,32} x waves in {4,8,16}, and as window 0 the
burst-then-drain kernel it replaced, picked through hgnn_set_option "k1_window" / "k1_waves") under build/,
rebuilt whenever a source is newer, and times every variant x nt_loads {0,1}
on the headline event in both layouts (shuffled edge order, destination-sorted).  Each round times every
variant once (20 launches between two events), so drift hits all variants alike; the table gives the median
and the min-max spread over rounds.  Every variant's output must equal the first variant's bit for bit.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SWEEP_LIB = os.path.join(ROOT, "build", "libhgnn_hip_k1sweep.so")
os.environ["HGNN_LIB"] = SWEEP_LIB  # read when the package is first imported


def build_sweep_lib():
    from hierarchicalgnn_amd import build as b
    b.build(verbose=False)
    os.makedirs(os.path.dirname(SWEEP_LIB), exist_ok=True)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    # the variants are in segreduce.hip, the options that pick one in capi.hip
    sweep = [os.path.join(b.CSRC, n) for n in ("segreduce.hip", "capi.hip")]
    objs = [s[:-4] + ".o" for s in b.sources() if s not in sweep]
    for src in sweep:
        objs.append(os.path.join(os.path.dirname(SWEEP_LIB), os.path.basename(src)[:-4] + "_k1sweep.o"))
        subprocess.check_call([hipcc, "-O3", "-std=c++17", f"--offload-arch={b.ARCH}", "-fPIC", "-DHGNN_K1_SWEEP",
                               "-c", src, "-o", objs[-1]])
    subprocess.check_call([hipcc, f"--offload-arch={b.ARCH}", "-shared", "-fPIC", "-o", SWEEP_LIB] + objs)
    return SWEEP_LIB


ap = argparse.ArgumentParser()
ap.add_argument("--build-only", action="store_true")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()
def stale():
    from hierarchicalgnn_amd import build as b
    return not os.path.exists(SWEEP_LIB) or not b.up_to_date() or \
        any(os.path.getmtime(d) > os.path.getmtime(SWEEP_LIB) for d in b._deps())


if args.build_only or stale():
    print(build_sweep_lib())
    if args.build_only:
        sys.exit(0)
import torch  # noqa: E402
import hierarchicalgnn_amd as H  # noqa: E402
from hierarchicalgnn_amd import _lib, synth  # noqa: E402

lib = _lib.load()
N, L, REPS = 120_000, 256, 20
x, ei = synth.trackml_event()
graph = synth.directed(ei).cuda()
M = graph.shape[1]
src = torch.randn(M, L, device="cuda")
layouts = {"shuffled": graph[1].contiguous(), "sorted": torch.sort(graph[1]).values}
plans = {k: H.get_plan(v, N) for k, v in layouts.items()}
assert plans["sorted"].sorted and not plans["shuffled"].sorted
nbytes = 4 * L * M + 4 * M + 4 * L * N
# window 0 = control: the burst-then-drain kernel k_seg_window replaced (16 waves only), with the same nt hint
variants = [(0, 16, nt) for nt in (1, 0)] + [(w, wpb, nt) for w in (8, 16, 32) for wpb in (4, 8, 16) for nt in (1, 0)]


def select(w, wpb, nt):
    for name, v in ((b"k1_window", w), (b"k1_waves", wpb), (b"nt_loads", nt)):
        _lib.check(lib.hgnn_set_option(name, v), "hgnn_set_option")


times = {(lay, v): [] for lay in layouts for v in variants}
first = {}
for rnd in range(args.rounds + 1):  # round 0 warms every variant up and checks its output
    for lay, index in layouts.items():
        for v in variants:
            select(*v)
            out = H.scatter_add(src, index, dim_size=N, plan=plans[lay])
            if rnd == 0:
                first.setdefault(lay, out)
                assert torch.equal(out, first[lay]), f"{lay} {v}: output differs from the first variant's"
                continue
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(REPS):
                H.scatter_add(src, index, dim_size=N, plan=plans[lay])
            e.record()
            torch.cuda.synchronize()
            times[(lay, v)].append(s.elapsed_time(e) / REPS * 1e3)
rows = []
for (lay, (w, wpb, nt)), t in times.items():
    t.sort()
    med = t[len(t) // 2]
    rows.append({"layout": lay, "window": w, "waves_per_workgroup": wpb, "nt_loads": nt, "median_us": med,
                 "min_us": t[0], "max_us": t[-1], "TBps": nbytes / med / 1e6})
rows.sort(key=lambda r: (r["layout"], r["median_us"]))
for r in rows:
    print(f"{r['layout']:9s} W={r['window']:2d} waves={r['waves_per_workgroup']:2d} nt={r['nt_loads']} "
          f"median {r['median_us']:.1f} us  [{r['min_us']:.1f}, {r['max_us']:.1f}]  {r['TBps']:.2f} TB/s")
if args.json:
    with open(args.json, "w") as f:
        json.dump({"shape": {"N": N, "M": M, "L": L}, "launches_per_sample": REPS, "rounds": args.rounds,
                   "what": "whole scatter_add call (main launch + combine launch), event-bracketed", "rows": rows},
                  f, indent=1)
