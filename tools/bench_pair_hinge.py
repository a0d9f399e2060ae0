#!/usr/bin/env python3
"""The fused weighted pair hinge loss (hierarchicalgnn_amd.pair_hinge_loss, csrc/pairloss.hip) against the torch
composition it replaces (training_weights + hinge_distance + hinge_embedding_loss + dot), forward + backward, on
seeded inputs: N hits with unit embeddings in D dimensions and P random pairs, 30 % true.

    python tools/bench_pair_hinge.py [--hits 120000] [--dim 8] [--pairs 4000000,12000000] [--reps 20] [--out FILE.json]

  fused_ms / torch_ms   median wall time of loss + backward, alternating the two, each ending in a device synchronise
  fused_fwd_ms          the forward alone
  ratio                 torch_ms / fused_ms;  goal_met: fused_ms < torch_ms with zero host reads in the fused call
  fused_bytes_per_s     the algorithmic bytes of DESIGN.md section 3 "k_ph" (17 B/pair forward, 21 + 24 B/pair backward,
                        int64 ids) over fused_ms: a whole-call rate, plan build included, not a kernel's share of peak
  rel_diff              |fused - torch| / |torch| of the two losses at this size
  --model-steps H,E     also time one whole training step (forward, loss, backward; median wall time) of
                        models.Embedding_HierarchicalGNN_GMM and models.gMRT built from the shipped configs
                        (tests/golden/embedding_hgnn.npz holds the parsed YAMLs) on a synthetic event of H hits and E
                        edges, freshly initialised weights; recorded, not gated
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

HP = dict(train_r=1.0, weight_leak=1.0, weight_min=0.5, pt_interval=0.5, ptcut=1.0, log_weight_ratio=0.0)


def _case(n, d, p, dev):
    g = torch.Generator().manual_seed(n + p)
    emb = torch.nn.functional.normalize(torch.randn(n, d, generator=g)).to(dev)
    graph = torch.randint(0, n, (2, p), generator=g).to(dev)
    y = (torch.rand(p, generator=g) < 0.3).to(dev)
    pt = torch.empty(n).exponential_(1.0, generator=g).to(dev)
    return emb, graph, y, {"pt": pt}


def _fused(emb, graph, y, batch, backward=True):
    e = emb.detach().requires_grad_(backward)
    loss = H.pair_hinge_loss(e, graph, y, batch, HP)
    if backward:
        loss.backward()
    return loss.detach()


def _torch(emb, graph, y, batch):
    e = emb.detach().requires_grad_(True)
    w = H.training_weights(batch, graph, y, HP)
    hinge, dist = H.hinge_distance(e, graph, y)
    loss = torch.dot(torch.nn.functional.hinge_embedding_loss(dist, hinge, margin=HP["train_r"],
                                                             reduction="none").square(), w)
    loss.backward()
    return loss.detach()


def _ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _model_steps(hits, edges, reps, dev):
    import numpy as np
    from hierarchicalgnn_amd import models, synth
    z = np.load(os.path.join(ROOT, "tests", "golden", "embedding_hgnn.npz"), allow_pickle=False)
    x, ei = synth.trackml_event(hits, edges, seed=11)
    ev = synth.embedding_event(hits, seed=11)
    batch = {k: v.to(dev) for k, v in ev.items() if k != "embeddings"}
    batch["edge_index"] = ei.to(dev)
    x = x.to(dev)
    out = {}
    for tag, cls in (("emb", models.Embedding_HierarchicalGNN_GMM), ("gmrt", models.gMRT)):
        hp = json.loads(str(z[f"cfg/{tag}/yaml"]))
        hp.setdefault("true_edges", "modulewise_true_edges")
        torch.manual_seed(0)
        model = cls(hp).to(dev).train()

        def step():
            model.zero_grad(set_to_none=True)
            if tag == "emb":
                emb, inter, _ = model(x, batch["edge_index"])
                loss = H.embedding_hgnn_training_loss(emb, inter, batch, hp, 0.3)[0]
            else:
                bg, scores, emb = model(x, batch["edge_index"])
                loss = H.bc_training_loss(bg, scores, emb, batch, hp, 0.3)[0]
            loss.backward()
            return loss

        step()
        step()
        times = [_ms(step) for _ in range(reps)]
        out[tag] = dict(model=hp["model"], latent=hp["latent"], hits=hits, edges=edges, reps=reps,
                        step_ms=sorted(times)[len(times) // 2], min_ms=min(times), max_ms=max(times))
        print(json.dumps({tag: out[tag]}), flush=True)
        del model
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=120_000)
    ap.add_argument("--dim", type=int, default=8)
    ap.add_argument("--pairs", default="4000000,12000000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model-steps", default=None, help="HITS,EDGES: also time one training step of the two models")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pair_hinge needs an MI355X: there is no CPU path and no fallback")
    dev = torch.device("cuda:0")
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    rows = []
    for p in (int(t) for t in a.pairs.split(",")):
        emb, graph, y, batch = _case(a.hits, a.dim, p, dev)
        for _ in range(a.warmup):
            lf, lt = _fused(emb, graph, y, batch), _torch(emb, graph, y, batch)
        reads = H.embedding.stats["host_reads"]
        fused, ref, fwd = [], [], []
        for _ in range(a.reps):                      # alternate, so that drift hits both alike
            fused.append(_ms(lambda: _fused(emb, graph, y, batch)))
            ref.append(_ms(lambda: _torch(emb, graph, y, batch)))
            fwd.append(_ms(lambda: _fused(emb, graph, y, batch, backward=False)))
        zero_reads = H.embedding.stats["host_reads"] == reads
        f, t = med(fused), med(ref)
        rows.append(dict(hits=a.hits, dim=a.dim, pairs=p, reps=a.reps, fused_ms=f, torch_ms=t, fused_fwd_ms=med(fwd),
                         fused_min_ms=min(fused), fused_max_ms=max(fused), torch_min_ms=min(ref), torch_max_ms=max(ref),
                         ratio=t / f, zero_host_reads=zero_reads, goal_met=bool(f < t and zero_reads),
                         fused_bytes_per_s=(17 + 21 + 24) * p / (f * 1e-3),
                         rel_diff=abs(float(lf) - float(lt)) / abs(float(lt))))
        print(json.dumps(rows[-1]), flush=True)
    H.pair_hinge_check()
    result = dict(tool="tools/bench_pair_hinge.py", device=torch.cuda.get_device_name(0), rows=rows)
    if a.model_steps:
        hits, edges = (int(t) for t in a.model_steps.split(","))
        result["model_steps"] = _model_steps(hits, edges, max(3, a.reps // 4), dev)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
