#!/usr/bin/env python3
"""Secondary figures at the BASELINE shape: (a) one InteractionGNNCell forward+backward under
reentrant checkpointing (the way the reference trains), (b) one HierarchicalGNNCell inference
forward with the synthetic hierarchy (S=10k, B=600k, Q~200k).  Usage: bench_train_step.py [L]

bench_train_step.py 512 wide_ab [OUT.json]: instead, one EC-IN training step at latent 512 with bf16 rows (BASELINE
config 4's dtype; forward + BCE + backward, reentrant checkpointing) with the N = 1024 fused backward layer off and on
(fused.set_bwd_layer_wide), the two alternating step by step in one process: median and max - min of 5 steps each."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import hierarchicalgnn_amd as H
from hierarchicalgnn_amd import fused, synth

L = int(sys.argv[1]) if len(sys.argv) > 1 else 256


def wide_ab():
    from hierarchicalgnn_amd.models import EC_InteractionGNN
    torch.manual_seed(1236)
    hp = dict(spatial_channels=3, latent=L, hidden=2 * L, n_interaction_graph_iters=14, nb_node_layer=3,
              nb_edge_layer=2, output_layers=3, hidden_output_activation="GELU", hidden_activation="GELU",
              layernorm=True, share_weight=False, checkpointing=True, feature_dtype="bf16")
    model = EC_InteractionGNN(hp).cuda().train()
    x, ei = synth.trackml_event()
    x, ei = x.cuda(), ei.cuda()
    target = (torch.rand(ei.shape[1], device="cuda") < 0.3).float()

    def step():
        loss = torch.nn.functional.binary_cross_entropy(model(x, ei), target)
        loss.backward()
        model.zero_grad(set_to_none=True)

    res = {"model": "EC-IN", "latent": L, "feature_dtype": "bf16", "cells": 14, "checkpointing": True,
           "N": int(x.shape[0]), "E": int(ei.shape[1])}
    ts = {False: [], True: []}
    for flag in (False, True):
        fused.set_bwd_layer_wide(flag)
        step()
    torch.cuda.synchronize()
    for _ in range(5):
        for flag in (False, True):
            fused.set_bwd_layer_wide(flag)
            c0 = {k: fused.stats[k] for k in ("bwd_layer_calls", "library_dgrad_calls", "library_calls", "hybrid_train_calls")}
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            torch.cuda.synchronize()
            ts[flag].append(a.elapsed_time(b))
            res[f"counters_wide_{'on' if flag else 'off'}"] = {k: fused.stats[k] - v for k, v in c0.items()}
    for flag, v in ts.items():
        v.sort()
        name = "on" if flag else "off"
        res[f"train_step_wide_{name}_ms"] = round(v[len(v) // 2], 2)
        res[f"train_step_wide_{name}_spread_ms"] = round(v[-1] - v[0], 2)
    text = json.dumps(res, indent=1)
    out = [a for a in sys.argv[3:]]
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out[0])), exist_ok=True)
        with open(out[0], "w") as f:
            f.write(text + "\n")
    print(text)


if "wide_ab" in sys.argv[2:3]:
    wide_ab()
    sys.exit(0)
torch.manual_seed(0)
x, ei = synth.trackml_event()
graph = synth.directed(ei).cuda()
N, M = 120_000, graph.shape[1]
hp = dict(latent=L, hidden=2 * L, nb_edge_layer=2, nb_node_layer=3, layernorm=True, hidden_activation="GELU")


def timeit(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
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


res = {"L": L, "N": N, "M": M}
cell = H.InteractionGNNCell(hp).cuda()
nodes = torch.randn(N, L, device="cuda", requires_grad=True)
edges = torch.randn(M, L, device="cuda", requires_grad=True)


def train_step():
    on, oe = cell(nodes, edges, graph)
    (on.sum() + oe.sum()).backward()
    cell.zero_grad(set_to_none=True)
    nodes.grad = None
    edges.grad = None


for ckpt in (True, False):
    cell._ckpt = ckpt
    for name, fwd, trn in (("fused_fwd+fused_train", True, True), ("fused_fwd+library_bwd", True, False),
                           ("library_only", False, False)):  # noqa
        fused.set_enabled(fwd, train=trn)
        res[f"ignn_cell_fwd_bwd_{'checkpointed' if ckpt else 'no_checkpoint'}_{name}_ms"] = timeit(train_step, 3, 1)
        res[f"peak_mem_GB_{'ckpt' if ckpt else 'nockpt'}_{name}"] = torch.cuda.max_memory_allocated() / 2**30
        torch.cuda.reset_peak_memory_stats()
cell._ckpt = True
fused.set_enabled(True)

S = 10_000
bg, bw = synth.bipartite_assignment(N, S, 5)
sg, sw = synth.super_graph(S, 10)
bg, bw, sg, sw = bg.cuda(), bw.cuda(), sg.cuda(), sw.cuda()
hcell = H.HierarchicalGNNCell(hp).cuda()
sn = torch.randn(S, L, device="cuda")
se = torch.randn(sg.shape[1], L, device="cuda")
res["B"] = int(bg.shape[1])
res["Q"] = int(sg.shape[1])
with torch.no_grad():
    n0, e0 = nodes.detach(), edges.detach()
    for name, on in (("fused", True), ("library", False)):
        fused.set_enabled(on)
        res[f"hgnn_cell_forward_{name}_ms"] = timeit(lambda: hcell(n0, e0, sn, se, graph, bg, bw, sg, sw), 3, 1)
    fused.set_enabled(True)
print(json.dumps(res, indent=1))
