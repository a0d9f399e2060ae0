#!/usr/bin/env python3
"""What the ramp and the tail of the K1 launch cost, and what handing out the longest lists first recovers.

    python tools/bench_k1_tail.py [--root TREE] [--rounds R] [--json PATH]

One process, variants interleaved: each round times every variant once (20 scatter_add calls between two events),
so drift hits all variants alike; the table gives the median and the min-max spread over the rounds.  K1 at
M = 2M rows, N = 120k destinations, F = 256 on

  (a) the headline event (list lengths: median 16, p99 35, a few hundred of 64 rows and more), plan order;
  (b) a control without imbalance: every destination has 16 or 17 rows, same M and N, shuffled with a fixed seed;
  (c) the headline event with its work items handed out longest-first (option k1_item_order = 1).

(a) - (b) bounds what any reordering of (a) can recover.  Where the library has the one-launch entry point, (a),
(b) and (c) run with it and a fourth variant times (a) on the two-launch path (k1_one_launch = 0).  --root measures
the package of another source tree (an older build without those options: (a) and (b) only).
"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
import hierarchicalgnn_amd as H  # noqa: E402
from hierarchicalgnn_amd import _lib, synth  # noqa: E402

lib = _lib.load()
has_options = hasattr(lib, "hgnn_segment_reduce_f32_ex")
N, L, REPS = 120_000, 256, 20
x, ei = synth.trackml_event()
headline = synth.directed(ei)[1].contiguous().cuda()
M = headline.numel()
g = torch.Generator().manual_seed(7)
deg = torch.full((N,), M // N, dtype=torch.int64)
deg[torch.randperm(N, generator=g)[:M - N * (M // N)]] += 1          # 16 or 17 rows each, M in all
balanced = torch.repeat_interleave(torch.arange(N), deg)[torch.randperm(M, generator=g)].cuda()
assert balanced.numel() == M
src = torch.randn(M, L, device="cuda")
inputs = {"headline": headline, "balanced": balanced}
plans = {k: H.get_plan(v, N) for k, v in inputs.items()}

# (name, input, k1_one_launch, k1_item_order)
variants = [("a_headline", "headline", 1, 0), ("b_balanced", "balanced", 1, 0)]
if has_options:
    variants += [("c_headline_longest_first", "headline", 1, 1), ("b_balanced_longest_first", "balanced", 1, 1),
                 ("a_headline_two_launches", "headline", 0, 0)]


def select(one, ordered):
    if has_options:
        for name, v in ((b"k1_one_launch", one), (b"k1_item_order", ordered)):
            _lib.check(lib.hgnn_set_option(name, v), "hgnn_set_option")


times = {v[0]: [] for v in variants}
first = {}
for rnd in range(args.rounds + 1):  # round 0 warms every variant up and checks its output
    for name, inp, one, ordered in variants:
        select(one, ordered)
        index, plan = inputs[inp], plans[inp]
        out = H.scatter_add(src, index, dim_size=N, plan=plan)
        if rnd == 0:
            first.setdefault(inp, out)
            assert torch.equal(out, first[inp]), f"{name}: output differs from the first variant's on this input"
            continue
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(REPS):
            H.scatter_add(src, index, dim_size=N, plan=plan)
        e.record()
        torch.cuda.synchronize()
        times[name].append(s.elapsed_time(e) / REPS * 1e3)
select(1, 1)
rows = {}
for name, t in times.items():
    t.sort()
    rows[name] = {"median_us": t[len(t) // 2], "min_us": t[0], "max_us": t[-1], "spread_us": t[-1] - t[0]}
    print(f"{name:28s} median {t[len(t) // 2]:.1f} us  [{t[0]:.1f}, {t[-1]:.1f}]")
res = {"shape": {"N": N, "M": M, "L": L}, "launches_per_sample": REPS, "rounds": args.rounds,
       "what": "whole scatter_add call, event-bracketed", "has_one_launch_entry": has_options, "rows": rows,
       "gap_a_minus_b_us": rows["a_headline"]["median_us"] - rows["b_balanced"]["median_us"]}
if has_options:
    a, c = rows["a_headline"], rows["c_headline_longest_first"]
    res["gain_c_over_a_us"] = a["median_us"] - c["median_us"]
    res["three_spreads_us"] = 3 * max(a["spread_us"], c["spread_us"])
    res["longest_first_pays"] = res["gain_c_over_a_us"] > res["three_spreads_us"]
print(json.dumps({k: v for k, v in res.items() if k != "rows"}))
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
