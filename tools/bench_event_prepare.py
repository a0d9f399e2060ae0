#!/usr/bin/env python3
"""Three routes from a loaded event to a prepared event on the device, in one process:

  device   dataset.prepare_event_device on device tensors (csrc/eventprep.hip): one host read
  host     dataset.prepare_event on CPU tensors, then the copy of its result to the device
  torch    the same masking written with torch operators on device tensors (``prepare_event_torch`` below: this
           tool's own copy of the composition, with the allocations moved to the device; one host read per boolean
           index, ``edge_index.unique()`` sorts 2E ids)

    python tools/bench_event_prepare.py [--hits 120000] [--edges 1000000] [--rounds 9] [--warmup 2] [--out FILE]

The event: ``synth.trackml_event`` (x, edge_index) with ``synth.tracking_event``'s truth (pid, pt, primary); the
module-wise true edges join the consecutive hits of every particle (about 100k for the default size), the signal true
edges are a seeded 60 % of them.  hparams: remove_isolated on, noise off, n_hits 3, edge_dropping_ratio 0 and 0.2 (each
route draws its own mask where it works: the CPU for ``host``, the device for the other two).

Every round runs the three routes one after another, so that drift hits all alike.  Per route: median and min .. max
of the wall time of one call, device synchronise included (host reads stall the host, which only the wall time shows);
host_syncs: the host reads of one call as torch.cuda.set_sync_debug_mode("warn") counts them; device_reads: what
dataset.stats["host_reads"] counted.  faster_than_*: the project's rule -- the difference of the medians must exceed
3 x the larger min .. max spread.  With ratio 0 the three results are compared for equality before anything is timed."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
from hierarchicalgnn_amd import dataset as D
from hierarchicalgnn_amd import synth


def make_event(n_hits, n_edges, seed=1234):
    x, edge_index = synth.trackml_event(n_hits, n_edges, seed=seed)
    truth = synth.tracking_event(n_hits, seed=seed)
    g = torch.Generator().manual_seed(seed + 29)
    pid = truth["pid"]
    order = torch.argsort(pid, stable=True)
    p = pid[order]
    same = (p[1:] == p[:-1]) & (p[1:] != 0)
    true_edges = torch.stack([order[:-1][same], order[1:][same]])
    true_edges = true_edges[:, torch.randperm(true_edges.shape[1], generator=g)].contiguous()
    signal = true_edges[:, torch.rand(true_edges.shape[1], generator=g) < 0.6].contiguous()
    y_pid = pid[edge_index[0]] == pid[edge_index[1]]
    return {"x": x, "cell_data": torch.randn(n_hits, 4, generator=g), "pid": pid, "hid": torch.arange(n_hits),
            "pt": truth["pt"], "edge_index": edge_index, "modulewise_true_edges": true_edges,
            "signal_true_edges": signal, "y": y_pid & (torch.rand(n_edges, generator=g) < 0.9), "y_pid": y_pid,
            "primary": truth["primary"]}


def prepare_event_torch(event, hparams):
    """dataset.prepare_event with its allocations on the event's device; otherwise line for line"""
    ev = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in event.items()}
    pid, pt = ev["pid"], ev["pt"]
    dev = pid.device
    mask = (pid == pid) if hparams["noise"] else (pid != 0)
    if hparams["hard_ptcut"] > 0:
        mask = mask & (pt > hparams["hard_ptcut"])
    if hparams["remove_isolated"]:
        node_mask = torch.zeros(pid.shape, dtype=torch.bool, device=dev)
        node_mask[ev["edge_index"].unique()] = True
        mask = mask & node_mask
    pt[pid == 0] = 0
    inverse_mask = torch.zeros(len(pid), dtype=torch.long, device=dev)
    inverse_mask[mask] = torch.arange(int(mask.sum()), device=dev)
    ev["inverse_mask"] = torch.arange(len(mask), device=dev)[mask]
    _, inverse, counts = pid.unique(return_inverse=True, return_counts=True)
    ev["nhits"] = counts[inverse]
    if hparams["primary"]:
        ev["signal_mask"] = (ev["nhits"] >= hparams["n_hits"]) & (ev["primary"] == 1)
    else:
        ev["signal_mask"] = ev["nhits"] >= hparams["n_hits"]
    if hparams.get("edge_dropping_ratio", 0) != 0:
        keep = torch.rand(ev["edge_index"].shape[1], device=dev) >= hparams["edge_dropping_ratio"]
        ev["edge_index"] = ev["edge_index"][:, keep]
        ev["y"], ev["y_pid"] = ev["y"][keep], ev["y_pid"][keep]
    graph_mask = mask[ev["edge_index"]].all(0)
    for k in ("y", "y_pid"):
        ev[k] = ev[k][graph_mask]
    for k in D.EDGE_LISTS:
        e = ev[k]
        ev[k] = inverse_mask[e[:, mask[e].all(0)]]
    for k in D.NODE_FIELDS:
        ev[k] = ev[k][mask]
    if hparams["primary"]:
        ev["primary"] = ev["primary"][mask]
    return ev


def _wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _syncs(fn):
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    return sum("synchroniz" in str(w.message).lower() for w in rec)


def _summary(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def _faster(a, b):
    """route a against route b by the project's rule"""
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    return bool(b["median"] - a["median"] > 3 * spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=120_000)
    ap.add_argument("--edges", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "event_prepare_bench.json"))
    a = ap.parse_args()
    if a.rounds < 9:
        raise SystemExit("bench_event_prepare: at least 9 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_event_prepare needs an MI355X: the device route has no CPU path and no fallback")
    dev = torch.device("cuda:0")
    ev = make_event(a.hits, a.edges)
    dev_ev = {k: v.to(dev) for k, v in ev.items()}
    shape = dict(hits=a.hits, edges=a.edges, modulewise_true_edges=int(ev["modulewise_true_edges"].shape[1]),
                 signal_true_edges=int(ev["signal_true_edges"].shape[1]))
    rows = []
    for ratio in (0.0, 0.2):
        hp = {"noise": False, "hard_ptcut": 0, "remove_isolated": True, "primary": False, "n_hits": 3,
              "edge_dropping_ratio": ratio}
        routes = {"device": lambda: D.prepare_event_device(dev_ev, hp),
                  "host": lambda: {k: v.to(dev) for k, v in D.prepare_event(ev, hp).items()},
                  "torch": lambda: prepare_event_torch(dev_ev, hp)}
        if ratio == 0:
            ref = routes["host"]()
            for r in ("device", "torch"):
                got = routes[r]()
                assert set(got) == set(ref) and all(got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k])
                                                    for k in ref), r
        for _ in range(a.warmup):
            for fn in routes.values():
                fn()
        times = {r: [] for r in routes}
        reads = {}
        for _ in range(a.rounds):
            for r, fn in routes.items():
                before = D.stats["host_reads"]
                times[r].append(_wall_ms(fn))
                reads[r] = D.stats["host_reads"] - before
        row = dict(case="ratio_%g" % ratio, rounds=a.rounds, **shape)
        for r in routes:
            row[r + "_wall_ms"] = _summary(times[r])
            row[r + "_host_syncs"] = _syncs(routes[r])
        row["device_reads"] = reads["device"]
        assert row["device_reads"] == 1, "prepare_event_device must read the host exactly once"
        for other in ("host", "torch"):
            row["device_faster_than_" + other] = _faster(row["device_wall_ms"], row[other + "_wall_ms"])
        print(json.dumps(row), flush=True)
        rows.append(row)
    result = dict(tool="tools/bench_event_prepare.py", device=torch.cuda.get_device_name(0),
                  command="python tools/bench_event_prepare.py --hits %d --edges %d --rounds %d --warmup %d"
                  % (a.hits, a.edges, a.rounds, a.warmup), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
