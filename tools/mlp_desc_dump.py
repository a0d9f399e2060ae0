#!/usr/bin/env python3
"""Dump what the Python side of the fused MLP hands to the kernels, for a fixed seeded list of calls (needs the GPU).

    python tools/mlp_desc_dump.py --tree TREE --out PREFIX

Imports hierarchicalgnn_amd from TREE (a checkout with its library built) and writes PREFIX.bin, the raw bytes of every
array in order, and PREFIX.txt, one line per item: scalars as text, arrays as dtype, shape, byte count and SHA-256.
Two trees hand the kernels the same thing exactly when both files are byte-equal (``cmp``): run it once per tree.

Per call: the ``_Route`` fields; every scalar field of the descriptor ``_descriptor`` returns and the bytes of every
tensor one of its pointers refers to (found in the keep-alive list by address); the result of ``mlp.concat_mlp``; under
autograd every gradient; at the end ``fused.stats``.  Shapes are the smallest that reach each branch: M = 200 rows (no
multiple of 64), a 40-row table gathered twice (4 N <= M switches the pre-projection on) and one direct segment.
"""
import argparse
import hashlib
import json
import os
import sys

M, N = 200, 40
POINTERS = (("seg_table", 3), ("seg_index", 3), ("W", 3), ("b", 3), ("ln_w", 3), ("ln_b", 3), ("skip", 0),
            ("pre_table", 2), ("pre_index", 2), ("save_pre", 3))
SCALARS = (("n_seg", 0), ("seg_width", 3), ("n_layers", 0), ("width", 4), ("act", 3), ("ln_eps", 0), ("M", 0),
           ("w0_cols", 0), ("w_last_rows", 0), ("n_pre", 0))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tree", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import torch.nn as nn
    from hierarchicalgnn_amd import fused, mlp
    from hierarchicalgnn_amd.utils import make_mlp
    assert os.path.abspath(fused.__file__).startswith(os.path.abspath(args.tree) + os.sep), fused.__file__
    dev = torch.device("cuda:0")
    txt, raw = open(args.out + ".txt", "w"), open(args.out + ".bin", "wb")
    count = [0, 0]

    def put(label, value):
        if isinstance(value, torch.Tensor):
            data = value.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes() if value.numel() else b""
            raw.write(data)
            count[0] += 1
            count[1] += len(data)
            value = f"{value.dtype} {tuple(value.shape)} {len(data)} {hashlib.sha256(data).hexdigest()}"
        txt.write(f"{label}: {value}\n")

    def rows(gen, n, w, dt):
        return torch.randn(n, w, generator=gen).to(dev).to(dt)

    def call(name, net, widths, dt=torch.float32, skip=False, train=False, bf16_tail=False, **opts):
        """segments of ``widths``: the first two (if there are three) gather one 40-row table, the last is direct"""
        gen = torch.Generator().manual_seed(1234)
        net = net.to(dev)
        table = rows(gen, N, widths[0], dt)
        segments = []
        for w in widths[:-1]:
            assert w == widths[0]
            segments.append((table, torch.randint(0, N, (M,), generator=gen).to(dev)))
        segments.append((rows(gen, M, widths[-1], dt), None))
        n_out = [m for m in net if isinstance(m, nn.Linear)][-1].out_features
        sk = rows(gen, M, n_out, torch.bfloat16 if bf16_tail else dt) if skip else None
        leaves = [table, segments[-1][0]] + ([sk] if skip else [])
        for t in leaves:
            t.requires_grad_(train)
        with fused.options(**opts), torch.set_grad_enabled(train):
            r = fused._route(net, segments, sk, train=train)
            put(f"{name}/route", None if r is None else (r.entry, r.split_proj, r.chain, r.head, r.train))
            if r is not None:
                layers = r.layers[:1] if r.chain else (r.layers[:2] if r.head and not r.train else r.layers)
                with torch.no_grad():
                    desc = fused._descriptor(None, segments, None if (r.chain or r.head) else sk, r.entry, r.split_proj,
                                             layers=layers)
                put(f"{name}/descriptor", None if desc is None else "built")
                if desc is not None:
                    d, keep = desc[0], desc[1]
                    for f, k in SCALARS:
                        put(f"{name}/d.{f}", getattr(d, f) if k == 0 else list(getattr(d, f)))
                    by_address = {}
                    for t in keep:
                        if t is not None:
                            by_address.setdefault(t.data_ptr(), t)
                    for f, k in POINTERS:
                        for i, p in enumerate([getattr(d, f)] if k == 0 else list(getattr(d, f))):
                            put(f"{name}/d.{f}[{i}]", "NULL" if not p else by_address[p])
            try:
                y = mlp.concat_mlp(net, segments, sk, bf16_tail=bf16_tail)
            except RuntimeError as e:
                put(f"{name}/raised", str(e))
                return
            put(f"{name}/result", y)
            if train:
                params = list(net.parameters())
                grads = torch.autograd.grad(y, leaves + params, rows(gen, M, n_out, y.dtype), allow_unused=True)
                for i, g in enumerate(grads):
                    put(f"{name}/grad[{i}]", "None" if g is None else g)

    def net(k, h, o, n, out_act="Tanh"):
        torch.manual_seed(7)
        return make_mlp(k, h, o, n, "GELU", out_act, layer_norm=True)

    bf = torch.bfloat16
    with fused.options(fp32_split3=False):
        for n in (2, 3):
            for skip in (False, True):
                call(f"f32/cell_L32_n{n}_skip{int(skip)}", net(96, 64, 32, n), (32, 32, 32), skip=skip)
        call("f32/head_H64", net(128, 64, 1, 3, None), (64, 64))
        call("f32/small_k3", net(3, 128, 64, 3), (3,))
        call("f32/partial_o24", net(32, 64, 24, 3), (16, 16))
        call("f32/single_512", net(128, 512, 512, 1, "GELU"), (128,), skip=True)
        call("f32/single_1024", net(128, 1024, 1024, 1, "GELU"), (128,))
        call("f32/single_504", net(512, 504, 504, 1, "GELU"), (512,))
        call("f32_padded/cell_h48", net(48, 48, 24, 3), (16, 16, 16))
        call("f32_padded/cell_h96", net(144, 96, 48, 2), (48, 48, 48), skip=True)
        call("f32_padded/head", net(96, 96, 1, 3, None), (48, 48))
        call("f32_padded/small_k6", net(6, 96, 48, 3), (6,))
        call("train/f32_cell_L32", net(96, 64, 32, 3), (32, 32, 32), skip=True, train=True)
        call("train/f32_head_H64", net(128, 64, 1, 3, None), (64, 64), train=True)
        call("train/f32_padded_h48", net(48, 48, 24, 3), (16, 16, 16), train=True)
    with fused.options(fp32_split3=True):
        call("f32_split3/cell_L128", net(384, 256, 128, 2), (128, 128, 128), skip=True)
        call("f32_split3/head_H256", net(256, 256, 1, 3, None), (128, 128))
    call("bf16/cell_L32", net(96, 64, 32, 3), (32, 32, 32), dt=bf, skip=True)
    call("bf16_split/cell_L128_pre1", net(384, 256, 128, 2), (128, 128, 128), dt=bf, skip=True, preproject_bf16=True)
    call("bf16_split/cell_L128_pre0", net(384, 256, 128, 2), (128, 128, 128), dt=bf, skip=True, preproject_bf16=False)
    call("bf16_split/single_256", net(128, 256, 256, 1, "GELU"), (128,), dt=bf)
    call("train/bf16_cell_L128", net(384, 256, 128, 2), (128, 128, 128), dt=bf, skip=True, train=True)
    # the hybrid chains of concat_mlp (bf16_tail): no-grad at a first layer 512 wide; under autograd the fp32 training
    # route takes that width first, so the hybrid is reached at 1024 (latent 512)
    call("hybrid/encoder_512", net(3, 512, 256, 3), (3,), bf16_tail=True)
    call("hybrid/encoder_1024_train", net(3, 1024, 512, 3), (3,), bf16_tail=True, train=True)
    call("refused/strict", net(60, 40, 20, 2), (20, 20, 20), strict=True)
    call("library/fallback", net(60, 40, 20, 2), (20, 20, 20))
    put("stats", json.dumps(fused.stats, sort_keys=True))
    put("arrays", f"{count[0]} arrays, {count[1]} bytes")
    print(f"{args.out}: {count[0]} arrays, {count[1]} bytes")


if __name__ == "__main__":
    main()
