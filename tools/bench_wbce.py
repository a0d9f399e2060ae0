#!/usr/bin/env python3
"""The fused pT-weighted BCE (hierarchicalgnn_amd.weighted_bce_loss, csrc/wbce.hip) against the torch compositions it
replaces, loss + backward, on seeded inputs.

    python tools/bench_wbce.py [--hits 120000] [--pairs 1000000,2000000] [--bipartite 600000] [--reps 30] [--out FILE]

  edge classifier   N hits, P random edges (30 % true), int64 and int32 ids.  fused: weighted_bce_loss.  torch:
                    embedding.training_weights + F.binary_cross_entropy(reduction="none") + torch.dot (the torch side
                    always gets int64 ids).
  assignment tail   N hits, B = 5 N bipartite pairs, a seeded matching of 10 000 particles and 10 000 clusters: what
                    bipartite_loss does after max_weight_matching.  fused: assignment._fused_tail.  torch:
                    assignment._torch_tail (four nonzero() host reads, get_asgmt_weight, BCE, dot).

  fused_ms / torch_ms   median of device-event times of loss + backward, the two alternating, after --warmup rounds
  ratio                 torch_ms / fused_ms;  goal_met: fused_ms < torch_ms with zero host reads in the fused call
  fused_bytes_per_s     the algorithmic bytes of DESIGN.md section 3 "k_wb" over fused_ms: forward 2 ids + 4 (score) +
                        1 (y), backward the same + 4 (gradient).  A whole-call rate, not a kernel's share of peak.
  rel_diff              |fused - torch| / |torch| of the two float32 losses (fused_loss, torch_loss)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import hierarchicalgnn_amd as H
from hierarchicalgnn_amd import assignment

HP = dict(weight_leak=1.0, weight_min=0.5, pt_interval=0.5, ptcut=1.0, log_weight_ratio=0.3)


def _ms(fn):
    """device time of fn() between two events on the current stream; host reads inside fn are part of it"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end), out


def _compare(tag, fused, ref, reads_of, reps, warmup, bytes_per_pair, pairs, extra):
    for _ in range(warmup):
        lf, lt = fused(), ref()
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    tf, tt = [], []
    reads = None
    for _ in range(reps):                            # alternate, so that drift hits both alike
        before = reads_of()
        tf.append(_ms(fused)[0])
        reads = reads_of() - before
        tt.append(_ms(ref)[0])
    f, t = med(tf), med(tt)
    row = dict(case=tag, pairs=pairs, reps=reps, fused_ms=f, torch_ms=t, fused_min_ms=min(tf), fused_max_ms=max(tf),
               torch_min_ms=min(tt), torch_max_ms=max(tt), ratio=t / f, fused_host_reads=reads,
               goal_met=bool(f < t and reads == 0), fused_bytes_per_s=bytes_per_pair * pairs / (f * 1e-3),
               fused_loss=float(lf), torch_loss=float(lt), rel_diff=abs(float(lf) - float(lt)) / abs(float(lt)),
               **extra)
    print(json.dumps(row), flush=True)
    return row


def _edge_classifier(n, p, idt, dev, reps, warmup):
    g = torch.Generator().manual_seed(n + p)
    graph64 = torch.randint(0, n, (2, p), generator=g).to(dev)
    graph = graph64.to(idt)
    y = (torch.rand(p, generator=g) < 0.3).to(dev)
    pt = torch.empty(n).exponential_(1.0, generator=g).to(dev)
    scores = torch.sigmoid(3.0 * torch.randn(p, generator=g)).to(dev)
    batch = {"pt": pt}

    def fused():
        s = scores.detach().requires_grad_(True)
        loss = H.weighted_bce_loss(s, graph, y, pt, HP)
        loss.backward()
        return loss.detach()

    def ref():
        s = scores.detach().requires_grad_(True)
        w = H.training_weights(batch, graph64, y, HP)
        loss = torch.dot(torch.nn.functional.binary_cross_entropy(s, y.float(), reduction="none"), w)
        loss.backward()
        return loss.detach()

    isz = 8 if idt == torch.int64 else 4
    reads_of = lambda: (H.edge_classifier.stats["host_reads"] + H.embedding.stats["host_reads"]  # noqa: E731
                        + assignment.stats["host_reads"])
    return _compare("edge_classifier", fused, ref, reads_of, reps, warmup, 2 * (2 * isz + 5) + 4, p,
                    dict(hits=n, index_dtype=str(idt).replace("torch.", "")))


def _assignment_tail(n, b, dev, reps, warmup, n_rows=10_000, n_cols=10_000):
    g = torch.Generator().manual_seed(n + b)
    pid = torch.randint(0, n_rows, (n,), generator=g)                       # particle 0 is noise
    original_pid = torch.arange(n_rows).to(dev)
    graph = torch.stack([torch.randint(0, n, (b,), generator=g), torch.randint(0, n_cols, (b,), generator=g)]).to(dev)
    # a matching: 80 % of the particles hold a distinct real column, the rest their virtual one
    cols = torch.randperm(n_cols, generator=g)[:n_rows]
    virtual = torch.rand(n_rows, generator=g) < 0.2
    col_match = torch.where(virtual, n_cols + torch.arange(n_rows), cols).to(dev)
    # half of the pairs follow the matching, so that the true class is not nearly empty
    follow = (torch.rand(b, generator=g) < 0.5).to(dev)
    hit_row = pid.to(dev)[graph[0]]
    graph[1] = torch.where(follow & (col_match[hit_row] < n_cols), col_match[hit_row], graph[1])
    batch_pt = torch.empty(n).exponential_(1.0, generator=g).to(dev)
    pt = torch.empty(n_rows).exponential_(1.0, generator=g).to(dev)
    scores = torch.sigmoid(3.0 * torch.randn(b, generator=g)).to(dev)

    def run(tail):
        s = scores.detach().requires_grad_(True)
        loss = tail(s, graph, batch_pt, pt, original_pid, hit_row, col_match, n_cols, HP, False)
        loss.backward()
        return loss.detach()

    reads_of = lambda: assignment.stats["host_reads"] + H.edge_classifier.stats["host_reads"]  # noqa: E731
    return _compare("assignment_tail", lambda: run(assignment._fused_tail), lambda: run(assignment._torch_tail),
                    reads_of, reps, warmup, 2 * (16 + 5) + 4, b, dict(hits=n, particles=n_rows, clusters=n_cols))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=120_000)
    ap.add_argument("--pairs", default="1000000,2000000")
    ap.add_argument("--bipartite", type=int, default=600_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wbce needs an MI355X: there is no CPU path and no fallback")
    dev = torch.device("cuda:0")
    rows = []
    for p in (int(t) for t in a.pairs.split(",")):
        for idt in (torch.int64, torch.int32):
            rows.append(_edge_classifier(a.hits, p, idt, dev, a.reps, a.warmup))
    rows.append(_assignment_tail(a.hits, a.bipartite, dev, a.reps, a.warmup))
    H.weighted_bce_check()
    result = dict(tool="tools/bench_wbce.py", device=torch.cuda.get_device_name(0),
                  command="python tools/bench_wbce.py --reps %d" % a.reps, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
