#!/usr/bin/env python3
"""Fused fp32 MLP at widths between the template grid's (latent 96 / 192): the edge update at M = 2M edges, N = 120k
nodes, and the EC-IN 14-cell forward at latent 96, against

  (a) the library path of the same shape (``fused.set_enabled(False)``: gathered copies, the [M, 3L] concat, separate
      GEMM / LayerNorm / activation kernels) -- what these shapes ran on before they had a kernel, and
  (b) the native grid neighbour at the same M on the exact fp32 kernel (latent 128 for 96, 256 for 192), which issues
      the same MFMAs and moves more bytes; the neighbour's shipped default (split-bf16 GEMMs) is listed for information.

Public API only (``mlp.concat_mlp``, the model mirrors), so the same file runs on a commit without the padded kernels,
where the "fused" variant of a non-grid width is the library path too (``padded_calls`` says which one ran).

``--split3``: the opt-in split-bf16 route at these widths (``fused.options(split3_padded=True)``,
hgnn_mlp_forward_f32_split3_padded) against the route with the option off in the same session (the exact padded kernel)
and the native neighbour's split-bf16 default (latent 256: also its 64-row kernel, which is what the padded entry
launches, next to the 128-row tile); the same three rows.

``--square``: hidden = latent (``hidden_ratio: 1``) on the square route (hgnn_mlp_forward_f32_square): the edge update
3L -> L -> L and the node update 2L -> L -> L -> L at latent 128 and 256, M = 2M rows, against what these shapes ran on
before they had a kernel -- the library path (``fused.set_enabled(False)``).  ``beats_library_by_3x_spread``: the medians
differ by more than three times the larger (max - min) spread of the two variants.

Method: device events around ``--inner`` back-to-back calls, every variant warmed up first, the variants ALTERNATED
inside each of ``--repeats`` (>= 7) rounds; per variant the median per-call time and the spread (min, max) over the
rounds.  One JSON document on stdout (``--out FILE`` also writes it).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hierarchicalgnn_amd import _lib, fused, make_mlp, mlp, synth  # noqa: E402


def _time(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def _alternate(variants, repeats, inner, warmup=2):
    """variants: {name: callable}.  -> {name: dict(median_ms, min_ms, max_ms)}"""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ts[k].append(_time(fn, inner))
    out = {}
    for k, v in ts.items():
        v = sorted(v)
        out[k] = dict(median_ms=round(v[len(v) // 2], 4), min_ms=round(v[0], 4), max_ms=round(v[-1], 4))
    return out


def _library(fn):
    def run():
        fused.set_enabled(False)
        try:
            return fn()
        finally:
            fused.set_enabled(True)
    return run


def edge_update(L, neighbour, graph, N, repeats, inner):
    M = int(graph.shape[1])

    def make(width):
        torch.manual_seed(width)
        net = make_mlp(3 * width, 2 * width, width, 2, layer_norm=True, output_activation="Tanh",
                       hidden_activation="GELU").cuda()
        nodes = torch.randn(N, width, device="cuda")
        edges = torch.randn(M, width, device="cuda")
        segs = [(nodes, graph[0]), (nodes, graph[1]), (edges, None)]
        return lambda: mlp.concat_mlp(net, segs, skip=edges)

    own, nb = make(L), make(neighbour)

    def nb_exact():
        with fused.options(fp32_split3=False):
            return nb()

    with torch.no_grad():
        p0 = fused.stats.get("padded_calls", 0)
        a = own()
        padded = fused.stats.get("padded_calls", 0) > p0
        b = _library(own)()
        err = float((a - b).abs().max() / b.abs().max())
        del a, b
        res = _alternate({f"latent{L}_fused": own, f"latent{L}_library": _library(own),
                          f"latent{neighbour}_exact_fp32": nb_exact, f"latent{neighbour}_default": nb}, repeats, inner)
    return dict(shape=f"edge update 3x{L} -> {2 * L} -> {L}, M = {M}, N = {N}", padded_kernel_ran=padded,
                fused_vs_library_max_rel=err, **res)


def ec_in(L, x, ei, repeats):
    from hierarchicalgnn_amd.models import EC_InteractionGNN
    torch.manual_seed(0)
    hp = dict(spatial_channels=3, latent=L, hidden=2 * L, n_interaction_graph_iters=14, nb_node_layer=3, nb_edge_layer=2,
              output_layers=3, hidden_output_activation="GELU", hidden_activation="GELU", layernorm=True,
              share_weight=False)
    model = EC_InteractionGNN(hp).cuda().eval()
    run = lambda: model(x, ei)   # noqa: E731
    with torch.no_grad():
        p0 = fused.stats.get("padded_calls", 0)
        a = run()
        padded = fused.stats.get("padded_calls", 0) - p0
        b = _library(run)()
        err = float((a - b).abs().max() / b.abs().max())
        res = _alternate({"fused": run, "library": _library(run)}, repeats, 1)
    return dict(shape=f"EC-IN forward, 14 cells, latent {L}, E = {int(ei.shape[1])}", padded_calls_per_forward=padded,
                fused_vs_library_max_rel=err, **res)


def _split3_padded(fn):
    def run():
        with fused.options(split3_padded=True):
            return fn()
    return run


def _rows64(fn):
    """the neighbour's split-bf16 default on its 64-row kernel (the padded entry never launches the 128-row tile)"""
    def run():
        lib = _lib.load()
        _lib.check(lib.hgnn_set_option(b"mlp_split3_rows128", 0))
        try:
            return fn()
        finally:
            _lib.check(lib.hgnn_set_option(b"mlp_split3_rows128", 1))
    return run


def edge_update_split3(L, neighbour, graph, N, repeats, inner):
    M = int(graph.shape[1])

    def make(width):
        torch.manual_seed(width)
        net = make_mlp(3 * width, 2 * width, width, 2, layer_norm=True, output_activation="Tanh",
                       hidden_activation="GELU").cuda()
        nodes = torch.randn(N, width, device="cuda")
        edges = torch.randn(M, width, device="cuda")
        segs = [(nodes, graph[0]), (nodes, graph[1]), (edges, None)]
        return lambda: mlp.concat_mlp(net, segs, skip=edges)

    own, nb = make(L), make(neighbour)
    on = _split3_padded(own)
    with torch.no_grad():
        n0, p0 = fused.stats.get("split3_padded_calls", 0), fused.stats.get("padded_calls", 0)
        a = on()
        ran = fused.stats.get("split3_padded_calls", 0) == n0 + 1 and fused.stats.get("padded_calls", 0) == p0
        b = own()
        ran = ran and fused.stats.get("padded_calls", 0) == p0 + 1
        err = float((a - b).abs().max() / b.abs().max())
        del a, b
        variants = {f"latent{L}_exact_padded": own, f"latent{L}_split3_padded": on, f"latent{neighbour}_default": nb}
        if neighbour == 256:
            variants[f"latent{neighbour}_default_rows64"] = _rows64(nb)
        res = _alternate(variants, repeats, inner)
    return dict(shape=f"edge update 3x{L} -> {2 * L} -> {L}, M = {M}, N = {N}", split3_padded_kernel_ran=ran,
                split3_vs_exact_max_rel=err, **res)


def ec_in_split3(L, x, ei, repeats):
    from hierarchicalgnn_amd.models import EC_InteractionGNN
    torch.manual_seed(0)
    hp = dict(spatial_channels=3, latent=L, hidden=2 * L, n_interaction_graph_iters=14, nb_node_layer=3, nb_edge_layer=2,
              output_layers=3, hidden_output_activation="GELU", hidden_activation="GELU", layernorm=True,
              share_weight=False)
    model = EC_InteractionGNN(hp).cuda().eval()
    run = lambda: model(x, ei)   # noqa: E731
    on = _split3_padded(run)
    with torch.no_grad():
        n0 = fused.stats.get("split3_padded_calls", 0)
        a = on()
        calls = fused.stats.get("split3_padded_calls", 0) - n0
        b = run()
        diff = float((a - b).abs().max())
        res = _alternate({"exact_padded": run, "split3_padded": on}, repeats, 1)
    return dict(shape=f"EC-IN forward, 14 cells, latent {L}, E = {int(ei.shape[1])}", split3_padded_calls_per_forward=calls,
                split3_vs_exact_max_abs_score=diff, **res)


def square_update(L, kind, graph, N, repeats, inner):
    """hidden = latent: ``kind`` "edge" (3L -> L -> L on gathered node rows + edge rows, Tanh output) or "node"
    (2L -> L -> L -> L on M direct rows, GELU output), skip connection on the last segment"""
    M = int(graph.shape[1])
    torch.manual_seed(L)
    rows = torch.randn(M, L, device="cuda")
    if kind == "edge":
        net = make_mlp(3 * L, L, L, 2, layer_norm=True, output_activation="Tanh", hidden_activation="GELU").cuda()
        nodes = torch.randn(N, L, device="cuda")
        segs = [(nodes, graph[0]), (nodes, graph[1]), (rows, None)]
        shape = f"edge update 3x{L} -> {L} -> {L}, M = {M}, N = {N}"
    else:
        net = make_mlp(2 * L, L, L, 3, layer_norm=True, output_activation="GELU", hidden_activation="GELU").cuda()
        segs = [(rows, None), (torch.randn(M, L, device="cuda"), None)]
        shape = f"node update 2x{L} -> {L} -> {L} -> {L}, M = {M}"
    own = lambda: mlp.concat_mlp(net, segs, skip=rows)   # noqa: E731
    with torch.no_grad():
        n0 = fused.stats.get("square_calls", 0)
        a = own()
        ran = fused.stats.get("square_calls", 0) == n0 + 1
        b = _library(own)()
        err = float((a - b).abs().max() / b.abs().max())
        del a, b
        res = _alternate({"square": own, "library": _library(own)}, repeats, inner)
    sq, lib = res["square"], res["library"]
    spread = max(sq["max_ms"] - sq["min_ms"], lib["max_ms"] - lib["min_ms"])
    return dict(shape=shape, square_kernel_ran=ran, square_vs_library_max_rel=err,
                speedup=round(lib["median_ms"] / sq["median_ms"], 3),
                beats_library_by_3x_spread=bool(lib["median_ms"] - sq["median_ms"] > 3 * spread), **res)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=120_000)
    ap.add_argument("--edges", type=int, default=1_000_000, help="undirected edges (the update runs on twice as many)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--split3", action="store_true",
                    help="measure the opt-in split-bf16 route at these widths against the exact padded one "
                         "(default --out: profiles/mlp_widths_split3_bench.json)")
    ap.add_argument("--square", action="store_true",
                    help="measure hidden = latent on the square route against the library path "
                         "(default --out: profiles/mlp_square.json)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp_widths: needs a GPU (there is no CPU path to time)")
    if args.repeats < 7:
        raise SystemExit("bench_mlp_widths: at least 7 repeats")
    x, ei = synth.trackml_event(args.nodes, args.edges, seed=1)
    x, ei = x.cuda(), ei.cuda()
    graph = synth.directed(ei).cuda()
    head = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, inner=args.inner,
                method="device events, variants alternated inside each repeat, median (min, max) per call")
    if args.square:
        if args.out is None:
            args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                    "mlp_square.json")
        doc = dict(**head, updates=[square_update(L, kind, graph, args.nodes, args.repeats, args.inner)
                                    for L in (128, 256) for kind in ("edge", "node")])
    elif args.split3:
        if args.out is None:
            args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                    "mlp_widths_split3_bench.json")
        doc = dict(**head,
                   edge_update=[edge_update_split3(96, 128, graph, args.nodes, args.repeats, args.inner),
                                edge_update_split3(192, 256, graph, args.nodes, args.repeats, args.inner)],
                   ec_in=ec_in_split3(96, x, ei, args.repeats))
    else:
        doc = dict(**head,
                   edge_update=[edge_update(96, 128, graph, args.nodes, args.repeats, args.inner),
                                edge_update(192, 256, graph, args.nodes, args.repeats, args.inner)],
                   ec_in=ec_in(96, x, ei, args.repeats))
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
