#!/usr/bin/env python3
"""The embedding stage's per-step pair construction (hierarchicalgnn_amd.embedding) at the reference's sizes.

    python tools/bench_embedding_samples.py [--reps 20] [--out FILE.json]

  frnn_ms_*        median device time of one ops.knn_radius(N = 120k self-queries, D = 8, K = 100, r = 1) (the kNN
                   inside frnn_graph; goal <= 8 ms) on clustered (synth.embedding_event) and on uniform unit
                   embeddings, with the mean number of in-radius candidates per query
  frnn_graph_ms    median wall time of a whole frnn_graph call (kNN + the mask compaction, one host sync)
  intersection_ms  median device time of one hgnn_graph_intersection launch sequence, 12M pred / 300k truth pairs
                   (goal <= 2 ms); intersection_call_ms: the whole graph_intersection call with its host read
  samples_ms       median wall time of a whole training_samples call (modulewise_true_edges) on the clustered event
Run under ``rocprofv3 --kernel-trace --stats`` for the per-kernel times.
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
from hierarchicalgnn_amd import _lib, synth
from hierarchicalgnn_amd.ops import knn_radius


def _device_ms(fn, reps):
    for _ in range(3):
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
    out.sort()
    return out[len(out) // 2]


def _wall_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    out.sort()
    return out[len(out) // 2]


def _candidates(emb, r, n=256):
    q = emb[:n]
    return float(((torch.cdist(q, emb) ** 2) < r * r).sum(1).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    n = 120_000
    ev = synth.embedding_event(n)
    batch = {k: v.to(dev) for k, v in ev.items()}
    clustered = batch["embeddings"]
    g = torch.Generator().manual_seed(2)
    uniform = torch.nn.functional.normalize(torch.randn(n, 8, generator=g)).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "N": n, "D": 8, "K": 100, "r": 1.0}
    for name, emb in (("clustered", clustered), ("uniform", uniform)):
        res[f"frnn_ms_{name}"] = _device_ms(lambda: knn_radius(emb, emb, 100, 1.0), args.reps)
        res[f"candidates_per_query_{name}"] = _candidates(emb, 1.0)
    res["frnn_graph_ms"] = _wall_ms(lambda: H.frnn_graph(clustered, 1.0, 100), args.reps)

    rng = torch.Generator().manual_seed(4)
    pred = torch.randint(0, n, (2, 12_000_000), generator=rng).to(dev)
    truth = torch.cat([pred[:, torch.randint(0, 12_000_000, (150_000,), generator=rng).to(dev)],
                       torch.randint(0, n, (2, 150_000), generator=rng).to(dev)], 1)
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    _lib.check(lib.hgnn_graph_intersection_workspace_bytes(pred.shape[1], truth.shape[1], 0, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    og = torch.empty((2, pred.shape[1]), dtype=torch.int64, device=dev)
    oy = torch.empty(pred.shape[1], dtype=torch.uint8, device=dev)
    cs = torch.empty(2, dtype=torch.int64, device=dev)

    def launch():
        _lib.check(lib.hgnn_graph_intersection(_lib.ptr(pred), pred.shape[1], _lib.ptr(truth), truth.shape[1], None,
                                               0, _lib.ptr(og), _lib.ptr(oy), None, _lib.ptr(cs), _lib.ptr(ws),
                                               nb.value, _lib.current_stream(dev)))

    res["intersection_pairs"] = [int(pred.shape[1]), int(truth.shape[1])]
    res["intersection_ms"] = _device_ms(launch, args.reps)
    res["intersection_call_ms"] = _wall_ms(lambda: H.graph_intersection(pred, truth), args.reps)
    hp = dict(train_r=1.0, knn=100, true_edges="modulewise_true_edges")
    res["samples_ms"] = _wall_ms(lambda: H.training_samples(clustered, batch, hp), args.reps)
    gs, ys = H.training_samples(clustered, batch, hp)
    res["samples_pairs"] = int(gs.shape[1])
    res["goal_frnn_ms"], res["goal_intersection_ms"] = 8.0, 2.0
    res["frnn_goal_met"] = res["frnn_ms_clustered"] <= 8.0 and res["frnn_ms_uniform"] <= 8.0
    res["intersection_goal_met"] = res["intersection_ms"] <= 2.0
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
