#!/usr/bin/env python3
"""The score-cut scan (hgnn_track_scan, csrc/trackscan.hip) next to the loop of the existing single-cut functions.

    python tools/bench_score_scan.py [--repeats 7] [--inner 3] [--cuts 8 32] [--out FILE]

Event: synth.tracking_event (N = 120k hits).  EDGE: M = 1M edges over the N hits, chains along every particle's hits
(scores 0.35 .. 1) and random edges (scores 0 .. 0.6), so the components merge over the whole cut range.  PAIR:
synth.track_candidates (B = 600k pairs, 10k candidates) with uniform scores.  T cuts spread over (0.05, 0.95).
Variants, each ONE full Python call (allocations and host reads included: what a validation step pays):
  scan   edge_score_scan / bipartite_score_scan: one device call, one host read
  loop   for every cut: edge_track_candidates / bipartite_track_candidates, then eval_metrics (the existing
         functions, the same code as on the commit before the scan): T host reads and, in EDGE mode, T more host
         synchronisations (the nonzero of edge_track_candidates)
Method: first ``torch.equal`` of the scan's [T, 12] block and the loop's hgnn_track_eval vectors (NaNs compared as
equal); then wall time around ``--inner`` back-to-back calls (every call ends in a host read, so the device is idle at
both ends), every variant warmed up first, scan and loop ALTERNATED inside each of ``--repeats`` rounds, one process;
per variant the median per-call time and the spread (min, max) over the rounds.  Verdict by the project's rule: the
scan is faster only when the medians differ by more than 3 x the larger spread.  Writes
profiles/score_scan_bench.json.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import hierarchicalgnn_amd as H
from hierarchicalgnn_amd import synth, tracking

KW = dict(pt_cut=1.0, nhits_cut=5, majority_cut=0.5, primary=False)


def edges_of(pid, n_edges, seed=7):
    g = torch.Generator().manual_seed(seed)
    order = torch.argsort(pid, stable=True)
    same = (pid[order][1:] == pid[order][:-1]) & (pid[order][1:] != 0)
    src, dst = order[:-1][same], order[1:][same]
    s_true = 0.35 + 0.65 * torch.rand(src.numel(), generator=g)
    n_false = n_edges - src.numel()
    fs, fd = torch.randint(0, pid.numel(), (2, n_false), generator=g)
    s_false = 0.6 * torch.rand(n_false, generator=g)
    perm = torch.randperm(n_edges, generator=g)
    ei = torch.stack([torch.cat([src, fs]), torch.cat([dst, fd])])[:, perm].contiguous()
    return ei, torch.cat([s_true, s_false])[perm].float().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=120_000)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, default=600_000)
    ap.add_argument("--cuts", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_scan_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    ev_cpu = synth.tracking_event(args.hits)
    ev = {k: v.cuda() for k, v in ev_cpu.items()}
    mask = torch.arange(args.hits).cuda()
    ei, es = (x.cuda() for x in edges_of(ev_cpu["pid"], args.edges))
    bg = synth.track_candidates(ev_cpu["pid"], args.pairs, 10_000).cuda()
    ps = torch.rand(bg.shape[1], generator=torch.Generator().manual_seed(3)).cuda()

    def loop(kind, cuts):
        cand, graph, scores = (H.edge_track_candidates, ei, es) if kind == "edge" else \
            (H.bipartite_track_candidates, bg, ps)
        return [H.eval_metrics(cand(graph, scores, c, mask), ev, **KW) for c in cuts]

    def loop_vectors(kind, cuts):
        cand, graph, scores = (H.edge_track_candidates, ei, es) if kind == "edge" else \
            (H.bipartite_track_candidates, bg, ps)
        return torch.stack([tracking.track_eval(cand(graph, scores, c, mask), ev, **KW).cpu() for c in cuts])

    def scan(kind, cuts):
        if kind == "edge":
            return H.edge_score_scan(ei, es, cuts, mask, ev, **KW)
        return H.bipartite_score_scan(bg, ps, cuts, mask, ev, **KW)

    rows = []
    for kind in ("edge", "pair"):
        for T in args.cuts:
            cuts = [0.05 + 0.9 * (k + 0.5) / T for k in range(T)]
            out = scan(kind, cuts)
            want = loop_vectors(kind, cuts)
            equal = torch.equal(torch.nan_to_num(out["result"], nan=-1.0), torch.nan_to_num(want, nan=-1.0))
            assert equal, f"{kind} T={T}: the scan and the loop disagree"
            assert out["metrics"] == loop(kind, cuts) or all(
                a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)
                for a, b in zip(out["metrics"], loop(kind, cuts)))
            variants = {"scan": lambda: scan(kind, cuts), "loop": lambda: loop(kind, cuts)}
            for fn in variants.values():
                fn()
            reads = {}
            times = {name: [] for name in variants}
            for _ in range(args.repeats):
                for name, fn in variants.items():
                    torch.cuda.synchronize()
                    r0 = tracking.stats["host_reads"]
                    t = time.perf_counter()
                    for _ in range(args.inner):
                        fn()
                    times[name].append((time.perf_counter() - t) * 1e3 / args.inner)
                    reads[name] = (tracking.stats["host_reads"] - r0) // args.inner
            ms = {}
            for name, r in times.items():
                r = sorted(r)
                ms[name] = dict(median_ms=round(r[len(r) // 2], 4), min_ms=round(r[0], 4), max_ms=round(r[-1], 4))
            spread = max(ms[n]["max_ms"] - ms[n]["min_ms"] for n in ms)
            diff = ms["loop"]["median_ms"] - ms["scan"]["median_ms"]
            n_cand = out["result"][:, 7].tolist()
            rows.append(dict(mode=kind, cuts=T, items=int((ei if kind == "edge" else bg).shape[1]), result_equal=equal,
                             ms=ms, counted_host_reads_per_call=reads, loop_minus_scan_ms=round(diff, 4),
                             larger_spread_ms=round(spread, 4), scan_faster=bool(diff > 3 * spread),
                             loop_faster=bool(-diff > 3 * spread), candidates_first_last=[n_cand[0], n_cand[-1]]))
            print(json.dumps(rows[-1]), flush=True)
    doc = dict(tool="tools/bench_score_scan.py", device=torch.cuda.get_device_name(0), N=args.hits,
               repeats=args.repeats, inner=args.inner,
               method="wall time per full Python call (allocations and host reads included), scan and loop alternated "
                      "inside each repeat, median (min, max) over the repeats; faster = medians more than 3 x the "
                      "larger spread apart", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
