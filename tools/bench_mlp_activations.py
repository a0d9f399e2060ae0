#!/usr/bin/env python3
"""Fused fp32 MLP with the activations a config sweep reaches first: the latent-256 edge update
(3 x 256 -> 512 -> 256, Tanh output, skip) at M = 2M edges, N = 120k nodes, exact fp32 kernel.

  gelu_compile_time     hidden GELU: the instantiation every shipped config runs
  silu_compile_time     hidden SiLU: its own instantiation
  silu_runtime_switch   the SAME network forced through the runtime switch (ACT = -1) of the same kernel by
                        ``hgnn_set_option("mlp_act_switch", 1)``: same source arithmetic (exact kernel: same bits, recorded)
  gelu_runtime_switch   the GELU network forced likewise
  elu_runtime_switch    hidden ELU (has no instantiation)
  plain                 hidden SiLU, layer_norm=False, ``fused.options(plain_layers=True)``
  silu_library          the SiLU network with the fused kernels off: what it ran on before the code existed (baseline)
  (``--split3`` adds gelu / silu / silu-switch on the split-bf16 kernel, the no-grad default at this width)

Method (as tools/bench_mlp_widths.py): device events around ``--inner`` back-to-back calls, every variant warmed up
first, the variants ALTERNATED inside each of ``--repeats`` (>= 7) rounds, one process; per variant the median per-call
time and the spread (min, max) over the rounds.  ``verdict``: whether compile-time SiLU differs from the runtime switch
by more than 3 x the larger spread (the project's rule for keeping an instantiation).  Writes
profiles/mlp_activations.json (``--out``) and prints the document.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hierarchicalgnn_amd import _lib, fused, make_mlp, mlp, synth  # noqa: E402
from bench_mlp_widths import _alternate, _library  # noqa: E402

L = 256


def _net(hidden, out, layer_norm=True):
    torch.manual_seed(7)
    return make_mlp(3 * L, 2 * L, L, 2, layer_norm=layer_norm, output_activation=out, hidden_activation=hidden).cuda()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=120_000)
    ap.add_argument("--edges", type=int, default=1_000_000, help="undirected edges (the update runs on twice as many)")
    ap.add_argument("--split3", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "mlp_activations.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp_activations: needs a GPU (there is no CPU path to time)")
    if args.repeats < 7:
        raise SystemExit("bench_mlp_activations: at least 7 repeats")
    _, ei = synth.trackml_event(args.nodes, args.edges, seed=1)
    graph = synth.directed(ei.cuda()).cuda()
    M = int(graph.shape[1])
    nodes = torch.randn(args.nodes, L, device="cuda")
    edges = torch.randn(M, L, device="cuda")
    segs = [(nodes, graph[0]), (nodes, graph[1]), (edges, None)]

    def call(net, **opts):
        def run():
            with fused.options(**opts):
                return mlp.concat_mlp(net, segs, skip=edges)
        return run

    def switched(fn):
        def run():
            lib = _lib.load()
            _lib.check(lib.hgnn_set_option(b"mlp_act_switch", 1))
            try:
                return fn()
            finally:
                _lib.check(lib.hgnn_set_option(b"mlp_act_switch", 0))
        return run

    silu, gelu = _net("SiLU", "Tanh"), _net("GELU", "Tanh")
    variants = {
        "gelu_compile_time": call(gelu, fp32_split3=False, strict=True),
        "gelu_runtime_switch": switched(call(gelu, fp32_split3=False, strict=True)),
        "silu_compile_time": call(silu, fp32_split3=False, strict=True),
        "silu_runtime_switch": switched(call(silu, fp32_split3=False, strict=True)),
        "elu_runtime_switch": call(_net("ELU", "Tanh"), fp32_split3=False, strict=True),
        "plain": call(_net("SiLU", "Tanh", layer_norm=False), plain_layers=True, strict=True),
        "silu_library": _library(call(silu)),
    }
    if args.split3:
        variants.update({
            "split3_gelu_compile_time": call(gelu, fp32_split3=True, strict=True),
            "split3_silu_compile_time": call(silu, fp32_split3=True, strict=True),
            "split3_silu_runtime_switch": switched(call(silu, fp32_split3=True, strict=True)),
        })
    with torch.no_grad():
        p0, l0 = fused.stats["plain_calls"], fused.stats["library_calls"]
        variants["plain"]()
        variants["silu_library"]()
        ran = dict(plain_kernel_ran=fused.stats["plain_calls"] == p0 + 1,
                   library_path_ran=fused.stats["library_calls"] == l0 + 1)
        a, b = variants["silu_compile_time"](), variants["silu_library"]()
        err = float((a - b).abs().max() / b.abs().max())
        ran["exact_switch_returns_the_same_bits"] = bool(torch.equal(a, variants["silu_runtime_switch"]()))
        if args.split3:
            # not bitwise: the compiler may contract an inlined activation's last product into the hi / mid split
            c, d = variants["split3_silu_compile_time"](), variants["split3_silu_runtime_switch"]()
            ran["split3_switch_vs_compile_time_max_rel"] = float((c - d).abs().max() / d.abs().max())
            del c, d
        del a, b
        res = _alternate(variants, args.repeats, args.inner)

    def verdict(x, y):
        spread = max(res[x]["max_ms"] - res[x]["min_ms"], res[y]["max_ms"] - res[y]["min_ms"])
        diff = res[y]["median_ms"] - res[x]["median_ms"]
        return dict(compile_time_minus_switch_ms=round(-diff, 4), larger_spread_ms=round(spread, 4),
                    differs_by_more_than_3_spreads=abs(diff) > 3 * spread)

    doc = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, inner=args.inner,
               method="device events, variants alternated inside each repeat, median (min, max) per call",
               shape=f"edge update 3x{L} -> {2 * L} -> {L}, M = {M}, N = {args.nodes}", **ran,
               silu_fused_vs_library_max_rel=err, **res,
               verdict=verdict("silu_compile_time", "silu_runtime_switch"))
    if args.split3:
        doc["verdict_split3"] = verdict("split3_silu_compile_time", "split3_silu_runtime_switch")
    txt = json.dumps(doc, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
