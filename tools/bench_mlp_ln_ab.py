#!/usr/bin/env python3
"""Kernel-level timing of the fused MLP entries whose LayerNorm epilogue computes pooled centred statistics: the edge
update K -> 2L -> (2L ->) L on the split-bf16 fp32 kernels and on the bf16 feature-split kernel, and the bf16 backward layer, median of 10 calls (ms)
between device events.  A/B of two builds: run once per library with HGNN_LIB=<path to libhgnn_hip.so>, alternating
(profiles/ln_stats_ab.json)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from hierarchicalgnn_amd import fused, make_mlp


def run(L, layers, M, bf16, iters=10):
    torch.manual_seed(L + layers)
    out_act = "Tanh" if layers == 2 else "GELU"
    net = make_mlp(3 * L, 2 * L, L, layers, layer_norm=True, output_activation=out_act, hidden_activation="GELU").cuda()
    dt = torch.bfloat16 if bf16 else torch.float32
    n_tab = M // 17
    table = torch.randn(n_tab, L, device="cuda").to(dt)
    i0 = torch.randint(0, n_tab, (M,), device="cuda")
    i1 = torch.sort(torch.randint(0, n_tab, (M,), device="cuda")).values
    direct = torch.randn(M, L, device="cuda").to(dt)
    segs = [(table, i0), (table, i1), (direct, None)]
    out = torch.empty(M, L, device="cuda", dtype=dt)
    with torch.no_grad():
        for _ in range(3):
            fused.fused_concat_mlp(net, segs, direct, out=out)
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fused.fused_concat_mlp(net, segs, direct, out=out)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def run_bwd(K, N, M, iters=10):
    """fused._bwd_layer, LayerNorm form (the N = 512 instantiation reloads z in every epilogue phase)"""
    g = torch.Generator(device="cuda").manual_seed(K + N)
    dz = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    W = torch.randn(K, N, device="cuda", generator=g) / K ** 0.5
    z = (1.5 * torch.randn(M, N, device="cuda", generator=g) + 0.2).bfloat16()
    gamma = 1 + 0.2 * torch.randn(N, device="cuda", generator=g)
    beta = 0.2 * torch.randn(N, device="cuda", generator=g)
    ts = []
    for i in range(3 + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fused._bwd_layer(dz, W, z, gamma, beta, 1, 1e-5, want_a=True)
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


res = {}
fused.set_fp32_split3(True)
res["f32_split3_L256x2_M2M"] = run(256, 2, 2_000_000, False)
res["f32_split3_L128x2_M2M"] = run(128, 2, 2_000_000, False)
res["f32_split3_L256x3_M1M"] = run(256, 3, 1_000_000, False)
res["bf16_split_L256x2_M2M"] = run(256, 2, 2_000_000, True)
res["bf16_split_L512x2_M1M"] = run(512, 2, 1_000_000, True)
res["bwd_layer_K1024_N512_M1M"] = run_bwd(1024, 512, 1_000_000)
res["bwd_layer_K512_N256_M1M"] = run_bwd(512, 256, 1_000_000)
print(json.dumps(res))
