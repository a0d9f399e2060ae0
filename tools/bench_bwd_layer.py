#!/usr/bin/env python3
"""Fused backward layer (hgnn_mlp_backward_layer_bf16) vs the unfused pieces it replaces (bf16 library GEMM + HIP
LayerNorm/activation row passes), M = 2M rows.  Usage: bench_bwd_layer.py [--wide [OUT.json] | --f32 [OUT.json]]

--wide: the N = 1024 instance (hidden width of latent 512) on GELU -- LayerNorm form (K, N) in {(512, 1024),
(1024, 1024)} at M = 2,000,000 and M = 120,000, input form (1024, 512) at M = 2,000,000 -- fused against unfused in
the same process, the two ALTERNATING call by call, median and max - min of 10 timed calls each after 3 warm-up calls.
The rule for the default of fused.set_bwd_layer_wide: on only if, at both M for both LayerNorm
shapes, the median gain exceeds three times the unfused route's own max - min spread.

--f32: the exact-fp32 fused backward layer (hgnn_mlp_backward_layer_f32) on GELU, same protocol -- LayerNorm form
(K, N) in {(256, 512), (512, 512), (128, 256), (256, 256)} at M = 2,000,000 and M = 120,000, input form (512, 256) with
skip at M = 2,000,000 -- against the unfused route of the same process (fp32 library GEMM + the two HIP row passes: what
the training backward runs with fused.set_bwd_layer_f32(False)); then one whole EC-IN training step at latent 128 and
256 on the synthetic 120k-hit / 1M-edge event with the switch off against on, alternating step by step (1 warm-up step,
median and max - min of 5).  The same rule decides a later flip of fused.set_bwd_layer_f32's default."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from hierarchicalgnn_amd import _lib, fused


def t(fn, reps=8):
    for _ in range(2):
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


def ab(unfused, fused_fn, reps=10, warm=3):
    """alternate the two routes call by call; (median, max - min) of each"""
    for _ in range(warm):
        unfused()
        fused_fn()
    torch.cuda.synchronize()
    ts = {"unfused": [], "fused": []}
    for _ in range(reps):
        for name, fn in (("unfused", unfused), ("fused", fused_fn)):
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
    r["gain_ms"] = round(r["unfused_ms"] - r["fused_ms"], 4)
    r["passes_rule"] = bool(r["gain_ms"] > 3 * r["unfused_spread_ms"])
    return r


def wide():
    res = {"kernel": "k_mlp_bwd_layer<8, EPI, 0, 1, 8, 2, true>  (N = 1024: 8 waves x 32-row tiles)", "act": "GELU",
           "tile_rows": _lib.MLP_BWD_TILE_ROWS_N1024, "cases": {}}
    fused.set_bwd_layer_wide(True)
    for K, N in ((512, 1024), (1024, 1024)):
        for M in (2_000_000, 120_000):
            dz = torch.randn(M, K, device="cuda").bfloat16()
            W = torch.randn(K, N, device="cuda") / K ** 0.5
            z = torch.randn(M, N, device="cuda").bfloat16()
            gm, bt = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
            Wb = W.bfloat16()

            def unfused():
                da = dz @ Wb
                return fused._ln_act_backward(z, da, gm, bt, 1, 1e-5), fused._ln_act_forward(z, gm, bt, 1, 1e-5)

            res["cases"][f"ln_form_K{K}_N{N}_M{M}"] = ab(
                unfused, lambda: fused._bwd_layer(dz, W, z, gm, bt, 1, 1e-5, want_a=True))
            del dz, z
            torch.cuda.empty_cache()
    M, K, N = 2_000_000, 1024, 512
    dz = torch.randn(M, K, device="cuda").bfloat16()
    W = torch.randn(K, N, device="cuda") / K ** 0.5
    skip = torch.randn(M, N, device="cuda").bfloat16()
    Wb = W.bfloat16()
    res["cases"][f"input_form_K{K}_N{N}_M{M}"] = ab(
        lambda: torch.addmm(skip, dz, Wb), lambda: fused._bwd_layer(dz, W, None, None, None, 0, 1e-5, skip=skip))
    res["default_on_by_rule"] = all(c["passes_rule"] for k, c in res["cases"].items() if k.startswith("ln_form"))
    text = json.dumps(res, indent=1)
    args = [a for a in sys.argv[1:] if a != "--wide"]
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write(text + "\n")
    print(text)


def f32_train_steps(res):
    from hierarchicalgnn_amd import synth
    from hierarchicalgnn_amd.models import EC_InteractionGNN
    x, ei = synth.trackml_event()
    x, ei = x.cuda(), ei.cuda()
    target = (torch.rand(ei.shape[1], device="cuda") < 0.3).float()
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

        r = {"model": "EC-IN", "latent": L, "cells": 14, "checkpointing": True, "N": int(x.shape[0]),
             "E": int(ei.shape[1])}
        ts = {False: [], True: []}
        for flag in (False, True):
            fused.set_bwd_layer_f32(flag)
            step()
        torch.cuda.synchronize()
        for _ in range(5):
            for flag in (False, True):
                fused.set_bwd_layer_f32(flag)
                c0 = fused.stats["bwd_layer_f32_calls"]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step()
                b.record()
                torch.cuda.synchronize()
                ts[flag].append(a.elapsed_time(b))
                r[f"bwd_layer_f32_calls_{'on' if flag else 'off'}"] = fused.stats["bwd_layer_f32_calls"] - c0
        for flag, v in ts.items():
            v.sort()
            name = "on" if flag else "off"
            r[f"train_step_{name}_ms"] = round(v[len(v) // 2], 2)
            r[f"train_step_{name}_spread_ms"] = round(v[-1] - v[0], 2)
        res["train_steps"][f"ec_in_L{L}"] = r
        del model
        torch.cuda.empty_cache()
    fused.set_bwd_layer_f32(False)


def f32():
    res = {"kernel": "k_mlp_bwd_f32 (fp32 MFMA, 4 waves x 16 rows, persistent on %d workgroups)" % _lib.MLP_BWD_F32_BLOCKS,
           "act": "GELU", "cases": {}, "train_steps": {}}
    fused.set_bwd_layer_f32(True)
    for K, N in ((256, 512), (512, 512), (128, 256), (256, 256)):
        for M in (2_000_000, 120_000):
            dz = torch.randn(M, K, device="cuda")
            W = torch.nn.Parameter(torch.randn(K, N, device="cuda") / K ** 0.5, requires_grad=False)
            z = torch.randn(M, N, device="cuda")
            gm, bt = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")

            def unfused():
                da = dz @ W
                return fused._ln_act_backward(z, da, gm, bt, 1, 1e-5), fused._ln_act_forward(z, gm, bt, 1, 1e-5)

            res["cases"][f"ln_form_K{K}_N{N}_M{M}"] = ab(
                unfused, lambda: fused._bwd_layer_f32(dz, W, z, gm, bt, 1, 1e-5, want_a=True, weight=W))
            del dz, z
            torch.cuda.empty_cache()
    M, K, N = 2_000_000, 512, 256
    dz = torch.randn(M, K, device="cuda")
    W = torch.nn.Parameter(torch.randn(K, N, device="cuda") / K ** 0.5, requires_grad=False)
    skip = torch.randn(M, N, device="cuda")
    res["cases"][f"input_form_K{K}_N{N}_M{M}"] = ab(
        lambda: torch.addmm(skip, dz, W), lambda: fused._bwd_layer_f32(dz, W, None, None, None, 0, 1e-5, skip=skip, weight=W))
    del dz, skip
    torch.cuda.empty_cache()
    res["default_on_by_rule"] = all(c["passes_rule"] for k, c in res["cases"].items() if k.startswith("ln_form"))
    f32_train_steps(res)
    fused.set_bwd_layer_f32(False)
    text = json.dumps(res, indent=1)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write(text + "\n")
    print(text)


if "--wide" in sys.argv[1:]:
    wide()
    sys.exit(0)
if "--f32" in sys.argv[1:]:
    f32()
    sys.exit(0)

M = 2_000_000
out = {}
lib = _lib.load()
for K, N in ((256, 512), (128, 256), (512, 512)):
    dz = torch.randn(M, K, device="cuda").bfloat16()
    W = torch.randn(K, N, device="cuda") / K ** 0.5
    z = torch.randn(M, N, device="cuda").bfloat16()
    gm, bt = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
    Wb = W.bfloat16()

    def unfused():
        da = dz @ Wb
        dzp = fused._ln_act_backward(z, da, gm, bt, 1, 1e-5)
        a = fused._ln_act_forward(z, gm, bt, 1, 1e-5)
        return dzp, a

    r = {"unfused_ms": t(unfused)}
    r["fused_ms"] = t(lambda: fused._bwd_layer(dz, W, z, gm, bt, 1, 1e-5, want_a=True))
    out[f"ln_form_K{K}_N{N}"] = r
    del dz, z
for K, N in ((512, 256), (256, 128)):
    dz = torch.randn(M, K, device="cuda").bfloat16()
    W = torch.randn(K, N, device="cuda") / K ** 0.5
    skip = torch.randn(M, N, device="cuda").bfloat16()
    Wb = W.bfloat16()
    out[f"input_form_K{K}_N{N}"] = {"unfused_addmm_ms": t(lambda: torch.addmm(skip, dz, Wb)),
                                    "fused_ms": t(lambda: fused._bwd_layer(dz, W, None, None, None, 0, 1e-5, skip=skip))}
print(json.dumps(out, indent=1))
