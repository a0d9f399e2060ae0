#!/usr/bin/env python3
"""The pair construction of one embedding training step from a precomputed kNN matrix, two routes, on an MI355X.

    python tools/bench_training_pairs.py [--n 120000] [--k 100] [--reps 20] [--out profiles/training_pairs_bench.json]

Both routes start from the same ``idx = knn_radius(emb, emb, K, 1.0)`` of ``synth.embedding_event(N)`` (the kNN is not
timed), alternate within this one process, and are compared bit for bit before anything is timed:

  composition   the frnn_graph expansion of idx (two boolean-index compactions) plus
                ``training_samples(..., prediction_graph=...)``: graph_intersection's radix sort of the pairs and the
                compactions and cats behind it
  fused         ``training_pairs(idx, batch, hparams)`` (csrc/trainpairs.hip)

Per ``true_edges`` mode: the median, minimum, maximum and the spread (max - min of the middle half) of the wall time of
a whole call (host clock around a call that ends in a device synchronise), the host reads each route counts in
``embedding.stats`` (the composition's boolean indexing syncs more often than it counts: see its ``syncs`` note), and
the device time (events) of the ``count`` and of the ``fill`` launch sequence of the fused route.
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
from hierarchicalgnn_amd import _lib, embedding, synth
from hierarchicalgnn_amd.ops import knn_radius

MODES = ("modulewise_true_edges", "pid_true_edges")


def _summary(ms):
    s = sorted(ms)
    n = len(s)
    return {"median_ms": s[n // 2], "min_ms": s[0], "max_ms": s[-1], "spread_ms": s[(3 * n) // 4] - s[n // 4],
            "reps": n}


def _wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _device(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def _expand(idx):
    pos = idx >= 0
    ind = torch.arange(idx.shape[0], device=idx.device).unsqueeze(1).expand(idx.shape)
    return torch.stack([ind[pos], idx[pos]], dim=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=120_000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 repetitions"
    assert torch.cuda.is_available(), "needs an MI355X: there is no CPU path and no CPU timing"
    dev = torch.device("cuda:0")
    ev = synth.embedding_event(args.n)
    batch = {k: v.to(dev) for k, v in ev.items()}
    emb = batch["embeddings"]
    idx = knn_radius(emb, emb, args.k, 1.0)
    res = {"device": torch.cuda.get_device_name(0), "N": args.n, "K": args.k, "r": 1.0,
           "T": int(batch["modulewise_true_edges"].shape[1]), "valid_slots": int((idx >= 0).sum()), "modes": {}}
    lib = _lib.load()
    for mode in MODES:
        hp = dict(train_r=1.0, knn=args.k, true_edges=mode)
        composition = lambda: H.training_samples(emb, batch, hp, prediction_graph=_expand(idx))   # noqa: E731
        fused = lambda: H.training_pairs(idx, batch, hp)                                          # noqa: E731
        reads = {}
        for name, fn in (("composition", composition), ("fused", fused)):
            r0 = embedding.stats["host_reads"]
            out = fn()
            reads[name] = embedding.stats["host_reads"] - r0
            if name == "composition":
                ref = out
        assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1]), "the two routes disagree"
        for _ in range(2):
            composition(), fused()
        times = {"composition": [], "fused": []}
        for _ in range(args.reps):                                   # alternating, one process
            times["composition"].append(_wall(composition))
            times["fused"].append(_wall(fused))
        m = {"pairs": int(ref[0].shape[1]), "true_pairs": int(ref[1].sum()),
             "composition": dict(_summary(times["composition"]), host_reads_counted=reads["composition"],
                                 syncs="every boolean-index compaction synchronises as well: not counted"),
             "fused": dict(_summary(times["fused"]), host_reads_counted=reads["fused"])}
        # the two launch sequences of the fused route on their own
        mte, sm8, pid = batch["modulewise_true_edges"], batch["signal_mask"].view(torch.uint8), batch["pid"]
        n, k, t, code = args.n, args.k, int(mte.shape[1]), embedding._TP_MODES[mode]
        ws, nb = _lib.workspace("hgnn_training_pairs_workspace_bytes", dev, n, k, t, code)
        info = torch.empty(_lib.TP_INFO, dtype=torch.int64, device=dev)
        a = (_lib.ptr(idx), n, k, _lib.ptr(mte), t, _lib.ptr(sm8), _lib.ptr(pid), code)
        stream = _lib.current_stream(dev)
        count = lambda: _lib.check(lib.hgnn_training_pairs_count(*a, _lib.ptr(info), _lib.ptr(ws), nb, stream))  # noqa: E731
        count()
        p = int(info[_lib.TP_P])
        assert p == m["pairs"]
        graph = torch.empty((2, p), dtype=torch.int64, device=dev)
        y = torch.empty(p, dtype=torch.uint8, device=dev)
        fill = lambda: _lib.check(lib.hgnn_training_pairs_fill(*a, _lib.ptr(graph), _lib.ptr(y), p, _lib.ptr(ws), nb,  # noqa: E731
                                                               stream))
        for _ in range(3):
            count(), fill()
        m["fused"]["count_device"] = _summary([_device(count) for _ in range(args.reps)])
        m["fused"]["fill_device"] = _summary([_device(fill) for _ in range(args.reps)])
        assert torch.equal(graph, ref[0]) and torch.equal(y.view(torch.bool), ref[1])
        m["fused"]["workspace_bytes"] = nb
        diff = m["fused"]["median_ms"] - m["composition"]["median_ms"]
        spread = max(m["fused"]["spread_ms"], m["composition"]["spread_ms"])
        m["fused_minus_composition_ms"] = diff
        m["fused_not_slower_beyond_spread"] = diff <= spread
        res["modes"][mode] = m
    res["note"] = ("training_samples(fused=True) is opt-in; whether it becomes the default is decided from this file "
                   "by the 3 x spread rule, not here")
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
