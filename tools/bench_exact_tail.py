#!/usr/bin/env python3
"""The last kernels of the exact fp32 step against the library expressions they replace: hgnn_project_f32 against
torch.matmul, the narrow products against F.linear / ``@`` / fused._atb.  Usage: bench_exact_tail.py [OUT.json] [--no-steps]

Kernels, the two routes in the same process ALTERNATING call by call, median and max - min of 10 timed calls each after
3 warm-up calls:
  * N = 120,000 rows: the projection in two blocks at K/N = 128/256 and 256/512 (the library: two matmuls); the encoder
    products with n = 3 at H = 256 and 512 (weight gradient S^T tab, input gradient S W_s);
  * M = 2,000,000 rows: a head's forward (F.linear) and backward (dy W, dy^T hidden and the column sums of dy) with
    n = 1 at H = 256 and 512.
Then one whole EC-IN training step at latent 128 and 256 on the synthetic 120k-hit / 1M-edge event with all four
switches (set_bwd_layer_f32, set_wgrad_f32, set_project_f32, set_narrow_f32) off against all four on, alternating step
by step (1 warm-up step each, median and max - min of 5).

The rule for a later flip of a default: a switch earns "on" only if, in every case it serves, the
median gain exceeds three times the LARGER of the two routes' max - min spreads.  ``default_on_by_rule`` records the
verdict per switch; no default is flipped here."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from hierarchicalgnn_amd import fused, ops

F = torch.nn.functional


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
    r["passes_rule"] = bool(r["gain_ms"] > 3 * max(r["library_spread_ms"], r["kernel_spread_ms"]))
    return r


def _diff(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def kernel_cases(res):
    for s in (fused.set_project_f32, fused.set_narrow_f32, fused.set_wgrad_f32, fused.set_bwd_layer_f32):
        s(False)                                   # fused._atb below is the library route
    rn = lambda *shape: torch.randn(*shape, device="cuda")
    N, M = 120_000, 2_000_000
    for K, H in ((128, 256), (256, 512)):
        x, W = rn(N, K), rn(H, 3 * K)
        w0, w1 = W[:, :K], W[:, K:2 * K]
        r = ab(lambda: (torch.matmul(x, w0.t()), torch.matmul(x, w1.t())), lambda: ops.project_f32(x, w0, w1))
        r["max_rel_diff_between_routes"] = _diff(ops.project_f32(x, w0, w1)[1], torch.matmul(x, w1.t()))
        res["cases"][f"project_K{K}_N{H}_two_blocks_rows{N}"] = dict(r, switch="project_f32")
    for H in (256, 512):
        S, tab, W_s = rn(N, H), rn(N, 3), rn(H, 3)
        Wt = W_s.t().contiguous()
        r = ab(lambda: fused._atb(S, tab), lambda: ops.wgrad_narrow_f32(tab, S))
        r["max_rel_diff_between_routes"] = _diff(ops.wgrad_narrow_f32(tab, S).t(), fused._atb(S, tab))
        res["cases"][f"encoder_wgrad_n3_H{H}_rows{N}"] = dict(r, switch="narrow_f32")
        r = ab(lambda: S @ W_s, lambda: ops.linear_narrow_f32(S, Wt))
        r["max_rel_diff_between_routes"] = _diff(ops.linear_narrow_f32(S, Wt), S @ W_s)
        res["cases"][f"encoder_dgrad_n3_H{H}_rows{N}"] = dict(r, switch="narrow_f32")
        del S, tab
    for H in (256, 512):
        hidden, W, b, dy = rn(M, H), rn(1, H), rn(1), rn(M, 1)
        r = ab(lambda: F.linear(hidden, W, b), lambda: ops.linear_narrow_f32(hidden, W, b))
        r["max_rel_diff_between_routes"] = _diff(ops.linear_narrow_f32(hidden, W, b), F.linear(hidden, W, b))
        res["cases"][f"head_forward_n1_H{H}_rows{M}"] = dict(r, switch="narrow_f32")
        cs = torch.empty(1, device="cuda")
        r = ab(lambda: (dy @ W, dy.t() @ hidden, dy.sum(0)),
               lambda: (ops.outer_narrow_f32(dy, W), ops.wgrad_narrow_f32(dy, hidden, colsum=cs)))
        r["max_rel_diff_between_routes"] = max(_diff(ops.outer_narrow_f32(dy, W), dy @ W),
                                               _diff(ops.wgrad_narrow_f32(dy, hidden), dy.t() @ hidden))
        res["cases"][f"head_backward_n1_H{H}_rows{M}"] = dict(r, switch="narrow_f32")
        del hidden, dy
        torch.cuda.empty_cache()
    for sw in ("project_f32", "narrow_f32"):
        res["default_on_by_rule"][sw] = all(c["passes_rule"] for c in res["cases"].values() if c["switch"] == sw)


COUNTERS = ("project_f32_calls", "narrow_linear_calls", "narrow_outer_calls", "narrow_wgrad_calls", "wgrad_f32_calls",
            "bwd_layer_f32_calls", "library_project_calls", "library_head_calls", "library_dgrad_calls",
            "library_wgrad_calls")


def train_steps(res):
    from hierarchicalgnn_amd import synth
    from hierarchicalgnn_amd.models import EC_InteractionGNN
    x, ei = synth.trackml_event()
    x, ei = x.cuda(), ei.cuda()
    target = (torch.rand(ei.shape[1], device="cuda") < 0.3).float()

    def select(on):
        for s in (fused.set_project_f32, fused.set_narrow_f32, fused.set_wgrad_f32, fused.set_bwd_layer_f32):
            s(on)

    for L in (128, 256):
        torch.manual_seed(1236)
        hp = dict(spatial_channels=3, latent=L, hidden=2 * L, n_interaction_graph_iters=14, nb_node_layer=3,
                  nb_edge_layer=2, output_layers=3, hidden_output_activation="GELU", hidden_activation="GELU",
                  layernorm=True, share_weight=False, checkpointing=True)
        model = EC_InteractionGNN(hp).cuda().train()

        def step():
            loss = F.binary_cross_entropy(model(x, ei), target)
            loss.backward()
            model.zero_grad(set_to_none=True)

        ts, counts = {False: [], True: []}, {}
        for on in (False, True):
            select(on)
            step()
        torch.cuda.synchronize()
        for _ in range(5):
            for on in (False, True):
                select(on)
                c0 = {k: fused.stats.get(k, 0) for k in COUNTERS}
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step()
                b.record()
                torch.cuda.synchronize()
                ts[on].append(a.elapsed_time(b))
                counts[on] = {k: fused.stats.get(k, 0) - v for k, v in c0.items() if fused.stats.get(k, 0) != v}
        r = {"model": "EC-IN", "latent": L, "cells": 14, "checkpointing": True, "N": int(x.shape[0]), "E": int(ei.shape[1])}
        for on, v in ts.items():
            v.sort()
            r["all_four_on" if on else "all_four_off"] = dict(train_step_ms=round(v[len(v) // 2], 2),
                                                              train_step_spread_ms=round(v[-1] - v[0], 2), **counts[on])
        gain = r["all_four_off"]["train_step_ms"] - r["all_four_on"]["train_step_ms"]
        r["gain_ms"] = round(gain, 2)
        r["passes_rule"] = bool(gain > 3 * max(r["all_four_off"]["train_step_spread_ms"],
                                               r["all_four_on"]["train_step_spread_ms"]))
        res["train_steps"][f"ec_in_L{L}"] = r
        del model
        torch.cuda.empty_cache()
    select(False)


def main():
    res = {"kernels": "k_project_f32 (v_mfma_f32_16x16x4_f32, k ascending, no split-K); k_linear_narrow / k_outer_narrow / "
                      "k_wgrad_narrow + k_wgrad_narrow_reduce (fp32 VALU)",
           "library": "torch.matmul per block; F.linear; dy @ W, dy^T @ hidden, dy.sum(0); fused._atb and S @ W_s with "
                      "the switches off",
           "rule": "gain > 3 x the larger max - min spread, in every case a switch serves",
           "cases": {}, "default_on_by_rule": {}, "train_steps": {}}
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
