#!/usr/bin/env python3
"""Exact fp32-MFMA weight gradient (hgnn_wgrad_f32) vs the library route it replaces (fused._atb with the switch off:
a batched product over row blocks + one sum + a tail product).  Usage: bench_wgrad_f32.py [OUT.json] [--no-steps]

Kernel: (Ho, Hi) in {(512, 256), (256, 512), (512, 512), (256, 128), (128, 256)} at M = 2,000,000 and M = 120,000, the
two routes in the same process ALTERNATING call by call, median and max - min of 10 timed calls each after 3 warm-up
calls.  Then one whole EC-IN training step at latent 128 and 256 on the synthetic 120k-hit / 1M-edge event with
fused.set_wgrad_f32 off against on, with fused.set_bwd_layer_f32 both off and on: the four settings alternating step by
step (1 warm-up step each, median and max - min of 5).

The rule for a later flip of fused.set_wgrad_f32's default: ``default_on_by_rule`` is true only
if, at every shape and both M, the median gain exceeds three times the library route's own max - min spread."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from hierarchicalgnn_amd import fused
from hierarchicalgnn_amd.ops import wgrad_f32

SHAPES = ((512, 256), (256, 512), (512, 512), (256, 128), (128, 256))
ROWS = (2_000_000, 120_000)


def ab(library, kernel, reps=10, warm=3):
    """alternate the two routes call by call; (median, max - min) of each"""
    for _ in range(warm):
        library()
        kernel()
    torch.cuda.synchronize()
    ts = {"library": [], "kernel": []}
    for _ in range(reps):
        for name, fn in (("library", library), ("kernel", kernel)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ts[name].append(s.elapsed_time(e))
    r = {"calls": reps}
    for name, v in ts.items():
        v.sort()
        r[name + "_ms"] = round(v[len(v) // 2], 4)
        r[name + "_spread_ms"] = round(v[-1] - v[0], 4)
    r["gain_ms"] = round(r["library_ms"] - r["kernel_ms"], 4)
    r["passes_rule"] = bool(r["gain_ms"] > 3 * r["library_spread_ms"])
    return r


def kernel_cases(res):
    fused.set_wgrad_f32(False)            # fused._atb below is the library route
    for M in ROWS:
        for Ho, Hi in SHAPES:
            dz = torch.randn(M, Ho, device="cuda")
            a = torch.randn(M, Hi, device="cuda")
            r = ab(lambda: fused._atb(dz, a), lambda: wgrad_f32(dz, a))
            r["kernel_tflops"] = round(2.0 * M * Ho * Hi / (r["kernel_ms"] * 1e-3) / 1e12, 1)
            r["library_tflops"] = round(2.0 * M * Ho * Hi / (r["library_ms"] * 1e-3) / 1e12, 1)
            ref = fused._atb(dz, a)
            r["max_rel_diff_between_routes"] = float((wgrad_f32(dz, a) - ref).abs().max() / ref.abs().max())
            res["cases"][f"Ho{Ho}_Hi{Hi}_M{M}"] = r
            del dz, a, ref
            torch.cuda.empty_cache()
    res["default_on_by_rule"] = all(c["passes_rule"] for c in res["cases"].values())


def train_steps(res):
    from hierarchicalgnn_amd import synth
    from hierarchicalgnn_amd.models import EC_InteractionGNN
    x, ei = synth.trackml_event()
    x, ei = x.cuda(), ei.cuda()
    target = (torch.rand(ei.shape[1], device="cuda") < 0.3).float()
    settings = [(w, b) for b in (False, True) for w in (False, True)]      # (wgrad_f32, bwd_layer_f32)
    name = lambda w, b: f"wgrad_f32_{'on' if w else 'off'}__bwd_layer_f32_{'on' if b else 'off'}"
    for L in (128, 256):
        torch.manual_seed(1236)
        hp = dict(spatial_channels=3, latent=L, hidden=2 * L, n_interaction_graph_iters=14, nb_node_layer=3,
                  nb_edge_layer=2, output_layers=3, hidden_output_activation="GELU", hidden_activation="GELU",
                  layernorm=True, share_weight=False, checkpointing=True)
        model = EC_InteractionGNN(hp).cuda().train()

        def step():
            loss = torch.nn.functional.binary_cross_entropy(model(x, ei), target)
            loss.backward()
            model.zero_grad(set_to_none=True)

        def select(w, b):
            fused.set_wgrad_f32(w)
            fused.set_bwd_layer_f32(b)

        r = {"model": "EC-IN", "latent": L, "cells": 14, "checkpointing": True, "N": int(x.shape[0]),
             "E": int(ei.shape[1]), "settings": {}}
        ts = {s: [] for s in settings}
        counts = {}
        for s in settings:
            select(*s)
            step()
        torch.cuda.synchronize()
        for _ in range(5):
            for s in settings:
                select(*s)
                c0 = {k: fused.stats.get(k, 0) for k in ("wgrad_f32_calls", "library_wgrad_calls", "bwd_layer_f32_calls")}
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step()
                b.record()
                torch.cuda.synchronize()
                ts[s].append(a.elapsed_time(b))
                counts[s] = {k: fused.stats.get(k, 0) - v for k, v in c0.items()}
        for s, v in ts.items():
            v.sort()
            r["settings"][name(*s)] = dict(train_step_ms=round(v[len(v) // 2], 2),
                                           train_step_spread_ms=round(v[-1] - v[0], 2), **counts[s])
        res["train_steps"][f"ec_in_L{L}"] = r
        del model
        torch.cuda.empty_cache()
    select(False, False)


def main():
    res = {"kernel": "k_wgrad_f32 (v_mfma_f32_16x16x4_f32, split-K, 256x256 / 256x128 / 128x128 tiles, KT = 16) "
                     "+ k_wgrad_f32_reduce",
           "library": "fused._atb with set_wgrad_f32(False): torch.bmm over row blocks + sum + tail",
           "cases": {}, "train_steps": {}}
    kernel_cases(res)
    if "--no-steps" not in sys.argv[1:]:
        train_steps(res)
    text = json.dumps(res, indent=1)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
