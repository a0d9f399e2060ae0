"""On-disk events and the per-event masking of ``TrackMLDataset.__getitem__`` (reference
Modules/utils.py:28-113).  Host-side index bookkeeping, no kernels.

The reference stores each event as a torch-pickled PyG ``Data`` object.  Unpickling that needs
``torch_geometric`` and executes code from the file, so this package reads a plain, pickle-free
container instead: one ``.npz`` per event holding the same named arrays (``x, cell_data, pid, hid,
pt, edge_index, modulewise_true_edges, signal_true_edges, y, y_pid[, primary]``).  ``save_event`` writes it;
converting an existing TrackML directory is a one-off ``save_event(path, data.to_dict())`` in an
environment that has PyG.

``prepare_event`` applies exactly the reference's filtering: noise / hard pT cut / isolated-hit
removal masks, pT of noise hits set to 0, ``nhits`` per particle, ``signal_mask``, optional random
edge dropping, re-indexing of every edge list through the inverse mask, ``inverse_mask`` kept for
un-masking at evaluation time.  It is the CPU path.

``prepare_event_device`` is the same function for an event that lives on the HIP device (csrc/eventprep.hip, kernels
``k_ep_*``): same keys, dtypes, shapes and values, every tensor on the inputs' device, ONE host read per event (the
info vector: N', the three edge counts and the status word), counted in ``stats["host_reads"]``.
``particle_hit_counts`` is its ``nhits`` operator on its own, with no host read.
"""
from __future__ import annotations

import math
from ctypes import c_void_p
from typing import Dict, Optional, Sequence

import numpy as np
import torch
from torch.utils.data import Dataset

from . import _lib

EDGE_LISTS = ("modulewise_true_edges", "signal_true_edges", "edge_index")
NODE_FIELDS = ("x", "cell_data", "pid", "hid", "pt", "signal_mask")

stats = {"host_reads": 0}   # host reads of prepare_event_device: one per call
_EVENT_DTYPES = {"x": torch.float32, "cell_data": torch.float32, "pid": torch.int64, "hid": torch.int64,
                 "pt": torch.float32, "edge_index": torch.int64, "modulewise_true_edges": torch.int64,
                 "signal_true_edges": torch.int64, "y": torch.bool, "y_pid": torch.bool}
_EDGE_SLOTS = (("edge_index", _lib.EP_E_EDGE_INDEX), ("modulewise_true_edges", _lib.EP_E_MODULEWISE),
               ("signal_true_edges", _lib.EP_E_SIGNAL))
_MAX = 2 ** 31 - 1


def save_event(path: str, event: Dict[str, torch.Tensor]) -> None:
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
                                  for k, v in event.items() if k != "dir"})


def load_event(path: str) -> Dict[str, torch.Tensor]:
    with np.load(path, allow_pickle=False) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def prepare_event(event: Dict[str, torch.Tensor], hparams, generator: torch.Generator = None) -> Dict[str, torch.Tensor]:
    """utils.py:57-108 on a dict of CPU tensors; returns a new dict (inputs are not modified)"""
    ev = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in event.items()}
    pid, pt = ev["pid"], ev["pt"]
    if hparams["noise"]:
        mask = pid == pid                                  # only NaN particle ids are dropped
    else:
        mask = pid != 0
    if hparams["hard_ptcut"] > 0:
        mask = mask & (pt > hparams["hard_ptcut"])
    if hparams["remove_isolated"]:
        node_mask = torch.zeros(pid.shape, dtype=torch.bool)
        node_mask[ev["edge_index"].unique()] = True
        mask = mask & node_mask
    pt[pid == 0] = 0
    inverse_mask = torch.zeros(len(pid), dtype=torch.long)
    inverse_mask[mask] = torch.arange(int(mask.sum()))
    ev["inverse_mask"] = torch.arange(len(mask))[mask]
    _, inverse, counts = pid.unique(return_inverse=True, return_counts=True)
    ev["nhits"] = counts[inverse]
    if hparams["primary"]:
        ev["signal_mask"] = (ev["nhits"] >= hparams["n_hits"]) & (ev["primary"] == 1)
    else:
        ev["signal_mask"] = ev["nhits"] >= hparams["n_hits"]
    if hparams.get("edge_dropping_ratio", 0) != 0:
        keep = torch.rand(ev["edge_index"].shape[1], generator=generator) >= hparams["edge_dropping_ratio"]
        ev["edge_index"] = ev["edge_index"][:, keep]
        ev["y"], ev["y_pid"] = ev["y"][keep], ev["y_pid"][keep]
    graph_mask = mask[ev["edge_index"]].all(0)
    for k in ("y", "y_pid"):
        ev[k] = ev[k][graph_mask]
    for k in EDGE_LISTS:
        e = ev[k]
        ev[k] = inverse_mask[e[:, mask[e].all(0)]]
    for k in NODE_FIELDS:
        ev[k] = ev[k][mask]
    if hparams["primary"]:
        ev["primary"] = ev["primary"][mask]
    return ev


def _check_event(event, hparams, edge_keep) -> None:
    """the argument ValueErrors of prepare_event_device: nothing here touches the library or a device"""
    who = "prepare_event_device"
    for k, dt in _EVENT_DTYPES.items():
        if k not in event or not torch.is_tensor(event[k]):
            raise ValueError(f"{who}: event[{k!r}] must be a tensor")
        if event[k].dtype != dt:
            raise ValueError(f"{who}: event[{k!r}] must be {dt}, got {event[k].dtype}")
    n = event["pid"].numel()
    if event["pid"].dim() != 1 or n > _MAX:
        raise ValueError(f"{who}: pid must be int64 [N], N < 2^31, got {tuple(event['pid'].shape)}")
    for k in ("hid", "pt"):
        if event[k].shape != event["pid"].shape:
            raise ValueError(f"{who}: {k} {tuple(event[k].shape)} does not match pid [{n}]")
    for k in ("x", "cell_data"):
        if event[k].dim() != 2 or event[k].shape[0] != n:
            raise ValueError(f"{who}: {k} must be [N = {n}, C], got {tuple(event[k].shape)}")
    for k, _ in _EDGE_SLOTS:
        if event[k].dim() != 2 or event[k].shape[0] != 2 or event[k].shape[1] > _MAX:
            raise ValueError(f"{who}: {k} must be int64 [2, E], E < 2^31, got {tuple(event[k].shape)}")
    e = event["edge_index"].shape[1]
    for k in ("y", "y_pid"):
        if event[k].shape != (e,):
            raise ValueError(f"{who}: {k} {tuple(event[k].shape)} does not match edge_index [2, {e}]")
    if hparams["primary"]:
        p = event.get("primary")
        if not torch.is_tensor(p):
            raise ValueError(f"{who}: hparams['primary'] needs event['primary']")
        if p.dtype != torch.int64 or p.shape != event["pid"].shape:
            raise ValueError(f"{who}: primary must be int64 [N = {n}], got {p.dtype} {tuple(p.shape)}")
    if edge_keep is not None and (not torch.is_tensor(edge_keep) or edge_keep.dtype != torch.bool
                                  or edge_keep.shape != (e,)):
        raise ValueError(f"{who}: edge_keep must be a bool [E = {e}] tensor")


def _gather_rows(lib, src: torch.Tensor, index: torch.Tensor, stream) -> torch.Tensor:
    """``src[index]`` along dim 0 by hgnn_event_gather_rows (rows of 1, 4 or 8-byte elements)"""
    src = src.contiguous()
    out = torch.empty((index.numel(),) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    cols = int(math.prod(src.shape[1:]))
    _lib.check(lib.hgnn_event_gather_rows(_lib.ptr(src), int(src.shape[0]), cols, src.element_size(), _lib.ptr(index),
                                          int(index.numel()), _lib.ptr(out), stream), "hgnn_event_gather_rows")
    return out


def prepare_event_device(event: Dict[str, torch.Tensor], hparams, generator: Optional[torch.Generator] = None,
                         edge_keep: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """``prepare_event`` for a dict of HIP device tensors: the same keys, dtypes, shapes and values, every tensor on
    the inputs' device, the inputs not written.  One host read: the info vector (N', the three edge counts, status).

    Edge dropping (``hparams["edge_dropping_ratio"] != 0``): ``edge_keep`` (bool [E], any device) wins; otherwise
    ``torch.rand(E, generator=generator) >= ratio`` is drawn on the generator's device, so a CPU generator reproduces
    ``prepare_event`` with the same seed bit for bit; with ``generator=None`` the draw is on the events' device.

    Kept quirks of the reference: ``nhits`` stays length N; ``primary`` is masked only with ``hparams["primary"]``;
    the pT cut uses the un-zeroed ``pt``; ``remove_isolated`` looks at ``edge_index`` before dropping.
    Differences: an edge id outside [0, N) in any of the three lists (dropped by ``edge_keep`` or not) is a
    ValueError from the single read -- the kernels skip it, no address is formed from it; ``n_hits`` is compared as
    an integer (its ceiling).
    RuntimeError for CPU tensors (``prepare_event`` is the CPU path); ValueError, before any launch, for a wrong dtype
    (pid, hid, edge lists int64; pt, x, cell_data float32; y, y_pid bool; primary int64), mismatched lengths or a
    missing ``primary`` with ``hparams["primary"]``."""
    _check_event(event, hparams, edge_keep)
    tensors = [event[k] for k in _EVENT_DTYPES] + ([event["primary"]] if hparams["primary"] else [])
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError("prepare_event_device needs HIP device tensors: hierarchicalgnn_amd has no CPU path "
                           "(prepare_event is the host-side function)")
    dev = event["pid"].device
    if any(t.device != dev for t in tensors):
        raise ValueError("prepare_event_device: the event's tensors must be on one device")
    use_primary = bool(hparams["primary"])
    pid, pt = event["pid"].contiguous(), event["pt"].contiguous()
    primary = event["primary"].contiguous() if use_primary else None
    edges = {k: event[k].contiguous() for k, _ in _EDGE_SLOTS}
    y, y_pid = event["y"].contiguous(), event["y_pid"].contiguous()
    n, e = int(pid.numel()), int(edges["edge_index"].shape[1])
    ratio = hparams.get("edge_dropping_ratio", 0)
    keep = None
    if ratio != 0:
        if edge_keep is not None:
            keep = edge_keep.to(dev).contiguous()
        elif generator is not None:
            keep = (torch.rand(e, generator=generator, device=generator.device) >= ratio).to(dev)
        else:
            keep = torch.rand(e, device=dev) >= ratio
    flags = (_lib.EP_NOISE if hparams["noise"] else 0) | (_lib.EP_REMOVE_ISOLATED if hparams["remove_isolated"] else 0) \
        | (_lib.EP_USE_PRIMARY if use_primary else 0)
    lib = _lib.load()
    new_id = torch.empty(n, dtype=torch.int32, device=dev)
    pt_out = torch.empty(n, dtype=torch.float32, device=dev)
    nhits = torch.empty(n, dtype=torch.int64, device=dev)
    signal = torch.empty(n, dtype=torch.bool, device=dev)
    info = torch.empty(_lib.EP_INFO, dtype=torch.int64, device=dev)
    info_at = lambda slot: c_void_p(info.data_ptr() + 8 * slot)     # noqa: E731
    with torch.cuda.device(dev):
        stream = _lib.current_stream(dev)
        ws, nb = _lib.workspace("hgnn_event_nodes_workspace_bytes", dev, n, e)
        _lib.check(lib.hgnn_event_nodes(
            _lib.ptr(pid), _lib.ptr(pt), _lib.ptr(primary), _lib.ptr(edges["edge_index"]), n, e,
            float(hparams["hard_ptcut"]), int(math.ceil(hparams["n_hits"])), flags, _lib.ptr(new_id), _lib.ptr(pt_out),
            _lib.ptr(nhits), _lib.ptr(signal), _lib.ptr(info), _lib.ptr(ws), nb, stream), "hgnn_event_nodes")
        scratch = {}
        for k, slot in _EDGE_SLOTS:
            ek = int(edges[k].shape[1])
            scratch[k] = _lib.workspace("hgnn_event_edges_workspace_bytes", dev, ek)
            _lib.check(lib.hgnn_event_edges_count(
                _lib.ptr(edges[k]), ek, _lib.ptr(keep if k == "edge_index" else None), _lib.ptr(new_id), n,
                info_at(slot), info_at(_lib.EP_STATUS), _lib.ptr(scratch[k][0]), scratch[k][1], stream),
                "hgnn_event_edges_count")
        stats["host_reads"] += 1
        got = info.tolist()                                       # the one read of the event
        if got[_lib.EP_STATUS] & _lib.EP_ST_BAD_ID:
            raise ValueError(f"prepare_event_device: an edge list holds a hit id outside [0, N = {n})")
        n_kept = got[_lib.EP_N_NODES]
        inverse_mask = torch.empty(n_kept, dtype=torch.int64, device=dev)
        _lib.check(lib.hgnn_event_inverse_mask(_lib.ptr(new_id), n, _lib.ptr(inverse_mask), n_kept, stream),
                   "hgnn_event_inverse_mask")
        out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in event.items()
               if k not in _EVENT_DTYPES and not (k == "primary" and use_primary)}
        for k, slot in _EDGE_SLOTS:
            ek, cnt, labelled = int(edges[k].shape[1]), got[slot], k == "edge_index"
            out[k] = torch.empty((2, cnt), dtype=torch.int64, device=dev)
            if labelled:
                out["y"] = torch.empty(cnt, dtype=torch.bool, device=dev)
                out["y_pid"] = torch.empty(cnt, dtype=torch.bool, device=dev)
            _lib.check(lib.hgnn_event_edges_fill(
                _lib.ptr(edges[k]), ek, _lib.ptr(keep if labelled else None), _lib.ptr(new_id), n,
                _lib.ptr(y if labelled else None), _lib.ptr(y_pid if labelled else None), _lib.ptr(out[k]), cnt,
                _lib.ptr(out["y"] if labelled else None), _lib.ptr(out["y_pid"] if labelled else None),
                _lib.ptr(scratch[k][0]), scratch[k][1], stream), "hgnn_event_edges_fill")
        fields = {"x": event["x"], "cell_data": event["cell_data"], "pid": pid, "hid": event["hid"], "pt": pt_out,
                  "signal_mask": signal}
        if use_primary:
            fields["primary"] = primary
        for k, v in fields.items():
            out[k] = _gather_rows(lib, v, inverse_mask, stream)
    out["inverse_mask"], out["nhits"] = inverse_mask, nhits
    return out


def particle_hit_counts(pid: torch.Tensor) -> torch.Tensor:
    """``counts[inverse]`` of ``pid.unique(return_inverse=True, return_counts=True)``: for every hit the number of hits
    that share its particle id (0 counts as one particle), int64 [N], by one radix sort on the device
    (hgnn_event_hit_counts) with no host read."""
    if not torch.is_tensor(pid) or pid.dtype != torch.int64 or pid.dim() != 1 or pid.numel() > _MAX:
        raise ValueError("particle_hit_counts: pid must be an int64 [N] tensor, N < 2^31")
    if not pid.is_cuda:
        raise RuntimeError("particle_hit_counts needs a HIP device tensor: hierarchicalgnn_amd has no CPU path")
    dev, n = pid.device, int(pid.numel())
    pid = pid.contiguous()
    nhits = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return nhits
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws, nb = _lib.workspace("hgnn_event_hit_counts_workspace_bytes", dev, n)
        _lib.check(lib.hgnn_event_hit_counts(_lib.ptr(pid), None, n, 0, _lib.ptr(nhits), None, _lib.ptr(ws), nb,
                                             _lib.current_stream(dev)), "hgnn_event_hit_counts")
    return nhits


class TrackMLDataset(Dataset):
    """same constructor and indexing contract as the reference class, over ``.npz`` events.

    ``device="cpu"`` (the default) prepares the event on the host with ``prepare_event``.  With a HIP ``device``
    ``__getitem__`` loads the ``.npz``, moves it to the device once and calls ``prepare_event_device``: the item's
    tensors are on the device.  A device dataset goes with ``DataLoader(num_workers=0)``: forked workers must not
    touch the GPU."""

    def __init__(self, dirs: Sequence[str], hparams, stage: str = "train", device: str = "cpu"):
        super().__init__()
        self.dirs, self.num = list(dirs), len(dirs)
        self.device, self.stage, self.hparams = device, stage, hparams

    def __getitem__(self, key):
        if torch.device(self.device).type == "cpu":
            ev = prepare_event(load_event(self.dirs[key]), self.hparams)
        else:
            ev = prepare_event_device({k: v.to(self.device) for k, v in load_event(self.dirs[key]).items()},
                                      self.hparams)
        ev["dir"] = self.dirs[key]
        return ev

    def __len__(self):
        return self.num
