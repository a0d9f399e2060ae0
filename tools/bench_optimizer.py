#!/usr/bin/env python3
"""The fused optimiser step (hierarchicalgnn_amd.FusedAdamW, csrc/optim.hip) against the torch compositions it
replaces, on the parameter sets of the reference's shipped models with random gradients.

    python tools/bench_optimizer.py [--sets ec128,bc256,ec512,bc512] [--reps 30] [--warmup 3] [--out FILE]

  parameter sets   EC-IN and BC-HGNN-GMM built on the meta device from tests/golden/ref_configs.json, at their shipped
                   latents (128, 256) and at latent 512; only the shapes are used
  (a) torch        clip_grad_norm_(0.5) + torch.optim.AdamW(amsgrad=True) with defaults + zero_grad(set_to_none=False):
                   the reference's composition on the same device
  (b) torch_fused  the same with AdamW(fused=True), if this torch build accepts it
  (c) fused        FusedAdamW(max_grad_norm=0.5, zero_grads=True)

  *_ms             median over --reps of the device time of ONE step between two events on the stream (host work that
                   leaves the device idle in between is part of it); the three alternate, each on its own copy of the
                   parameters; the gradients are refilled before every step, outside the timed span
  ratio_a, ratio_b torch_ms / fused_ms, torch_fused_ms / fused_ms;  goal_met: fused_ms < torch_ms
  *_bytes_per_s    the ALGORITHMIC bytes of the fused step over the time: 44 B per parameter (the sum of squares reads
                   g; the update reads p, g, m, v, vmax and writes p, m, v, vmax and the zeroed g).  A whole-step rate,
                   not a kernel's share of peak; for (a) and (b) it is the same bytes over their time
  fused_launches   kernel launches of one fused step (hierarchicalgnn_amd.optim.stats); the torch variants' launches
                   are not counted here: see the kernel trace in profiles/ if one was taken
  max_rel_diff     largest |fused - torch| / max|torch| over the parameter tensors after the run: the three did the
                   same work
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import hierarchicalgnn_amd as H
from hierarchicalgnn_amd.models import BC_MessagePassing, EC_InteractionGNN

SETS = {"ec128": ("EC-IN", 128), "bc256": ("BC-HGNN-GMM", 256), "ec512": ("EC-IN", 512), "bc512": ("BC-HGNN-GMM", 512)}
BYTES_PER_PARAM = 44
MAX_NORM = 0.5
LR = 1e-3


def shapes_of(name, latent):
    with open(os.path.join(ROOT, "tests", "golden", "ref_configs.json")) as fh:
        raw = dict(json.load(fh)[name]["raw"], latent=latent)
    cls = EC_InteractionGNN if name == "EC-IN" else BC_MessagePassing
    with torch.device("meta"):
        model = cls(raw)
    return [tuple(p.shape) for p in model.parameters()]


class Variant:
    def __init__(self, kind, shapes, dev, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        self.kind = kind
        self.params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g) * 0.05) for s in shapes]
        self.fill = [torch.randn(s, device=dev, generator=g) * 1e-2 for s in shapes]
        for p in self.params:
            p.grad = torch.zeros_like(p)
        self.grads = [p.grad for p in self.params]
        if kind == "fused":
            self.opt = H.FusedAdamW(self.params, lr=LR, max_grad_norm=MAX_NORM, zero_grads=True)
        else:
            self.opt = torch.optim.AdamW(self.params, lr=LR, betas=(0.9, 0.999), eps=1e-8, amsgrad=True,
                                         fused=True if kind == "torch_fused" else None)
        self.times = []

    def refill(self):
        torch._foreach_copy_(self.grads, self.fill)

    def step(self):
        if self.kind == "fused":
            self.opt.step()
            self.opt.zero_grad()
        else:
            torch.nn.utils.clip_grad_norm_(self.params, MAX_NORM)
            self.opt.step()
            self.opt.zero_grad(set_to_none=False)

    def timed_step(self):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.refill()
        start.record()
        self.step()
        end.record()
        return start, end


def bench_set(tag, dev, reps, warmup):
    name, latent = SETS[tag]
    shapes = shapes_of(name, latent)
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    variants = [Variant("torch", shapes, dev, 1)]
    try:
        variants.append(Variant("torch_fused", shapes, dev, 1))
    except (RuntimeError, TypeError, ValueError) as err:          # this build has no fused AdamW for these tensors
        print(f"{tag}: torch fused=True not available: {err}", flush=True)
    variants.append(Variant("fused", shapes, dev, 1))
    for _ in range(warmup):
        for v in variants:
            v.refill()
            v.step()
    torch.cuda.synchronize()
    launches0 = H.optim.stats["launches"]
    events = {v.kind: [] for v in variants}
    for _ in range(reps):                                        # alternate, so that drift hits all alike
        for v in variants:
            events[v.kind].append(v.timed_step())
        torch.cuda.synchronize()
    med = lambda t: sorted(t)[len(t) // 2]                       # noqa: E731
    row = dict(set=tag, model=name, latent=latent, tensors=len(shapes), parameters=n, reps=reps,
               algorithmic_bytes=BYTES_PER_PARAM * n, fused_launches=(H.optim.stats["launches"] - launches0) // reps)
    for kind, evs in events.items():
        t = [s.elapsed_time(e) for s, e in evs]
        row[kind + "_ms"], row[kind + "_min_ms"], row[kind + "_max_ms"] = med(t), min(t), max(t)
        row[kind + "_bytes_per_s"] = BYTES_PER_PARAM * n / (med(t) * 1e-3)
    row["ratio_a"] = row["torch_ms"] / row["fused_ms"]
    row["ratio_b"] = row["torch_fused_ms"] / row["fused_ms"] if "torch_fused_ms" in row else None
    row["goal_met"] = bool(row["fused_ms"] < row["torch_ms"])
    by = {v.kind: v for v in variants}
    row["max_rel_diff"] = max(float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())
                              for a, b in zip(by["fused"].params, by["torch"].params) if a.numel())
    by["fused"].opt.check()
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="ec128,bc256,ec512,bc512")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tags = a.sets.split(",")
    for t in tags:
        if t not in SETS:
            raise SystemExit(f"unknown set {t!r}; choose from {', '.join(SETS)}")
    if not torch.cuda.is_available():
        raise SystemExit("bench_optimizer needs an MI355X: there is no CPU path and no fallback")
    dev = torch.device("cuda:0")
    rows = [bench_set(t, dev, a.reps, a.warmup) for t in tags]
    result = dict(tool="tools/bench_optimizer.py", device=torch.cuda.get_device_name(0), torch=torch.__version__,
                  command="python tools/bench_optimizer.py --reps %d" % a.reps, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
