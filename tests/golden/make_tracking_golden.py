#!/usr/bin/env python3
"""Generate tests/golden/tracking_eval.npz by IMPORTING the reference's own Modules/tracking_utils.py.

Run in the build container only (it needs the reference checkout, which never travels to the GPU box):

    python tests/golden/make_tracking_golden.py

The reference's eval_metrics is built on cupy / cupy.sparse, which do not exist here.  Stand-ins, in the style of
make_golden.py's stubs:
  * cupy: numpy arrays; ``cupy.sparse.coo_matrix(...).tocsr()`` is a scipy CSR matrix behind a thin wrapper whose
    indexing, ``.sum``, ``.max(...).todense()`` and comparisons return plain ndarrays (cupy has no matrix type; with
    np.matrix the reference's ``[0]`` at :57 would pick the wrong axis).  ``linspace`` is numpy's.
  * torch_scatter: scatter_min = Tensor.scatter_reduce("amin", include_self=False), scatter_sum =
    Tensor.scatter_add.  The reference never imports scatter_sum (its primary=True branch is dead code), so for the
    primary=True cases it is injected into the module.
  * matplotlib / sklearn / mpl_toolkits: imported by the module for plotting only; empty modules.
The event is a dict with attribute access (``"primary" in event`` works, as for a PyG Data).

Every case stores its inputs and the reference's four outputs (or that it raised / returned default_response).  The
file is written with fixed zip timestamps, so re-running reproduces it bit for bit.
"""
import io
import os
import sys
import tempfile
import types
import zipfile

sys.dont_write_bytecode = True
sys.pycache_prefix = tempfile.mkdtemp(prefix="golden_pyc_")

import numpy as np
import scipy.sparse as sp
import torch

REF = os.environ.get("HGNN_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tracking_eval.npz")


# --------------------------------------------------------------------------
# stand-ins
# --------------------------------------------------------------------------
class _Sparse:
    """a scipy CSR matrix that hands back ndarrays wherever cupy would"""

    def __init__(self, m):
        self.m = m.tocsr()

    @property
    def shape(self):
        return self.m.shape

    def tocsr(self):
        return self

    def sum(self, axis=None):
        return np.asarray(self.m.sum(axis))

    def multiply(self, other):
        return _Sparse(sp.csr_matrix(self.m.multiply(np.asarray(other))))

    def max(self, axis=None):
        r = self.m.max(axis=axis)
        return types.SimpleNamespace(todense=lambda: np.asarray(r.todense()))

    def _dense(self):
        return self.m.toarray()

    def __ge__(self, other):
        return self._dense() >= np.asarray(other)

    def __gt__(self, other):
        return self._dense() > np.asarray(other)

    def __eq__(self, other):
        return self._dense() == np.asarray(other)

    def __getitem__(self, idx):
        r = self.m[idx]
        return _Sparse(r) if sp.issparse(r) else np.asarray(r)


def _scatter_min(src, index, dim=0, dim_size=None):
    assert dim == 0
    n = int(dim_size) if dim_size is not None else int(index.max()) + 1
    out = torch.zeros(n, dtype=src.dtype).scatter_reduce(0, index, src, "amin", include_self=False)
    return out, None


def _scatter_sum(src, index, dim=0, dim_size=None):
    assert dim == 0
    n = int(dim_size) if dim_size is not None else int(index.max()) + 1
    return torch.zeros(n, dtype=src.dtype).scatter_add(0, index, src)


def _install_stubs():
    ts = types.ModuleType("torch_scatter")
    ts.scatter_min = _scatter_min
    ts.scatter_add = ts.scatter_sum = _scatter_sum

    def _unused(*a, **k):
        raise NotImplementedError

    ts.scatter_mean = ts.scatter_max = _unused
    sys.modules["torch_scatter"] = ts

    cp = types.ModuleType("cupy")
    cp.asarray = lambda t: np.asarray(t.detach().cpu() if torch.is_tensor(t) else t)
    cp.array = np.array
    cp.ones = np.ones
    cp.where = np.where
    cp.linspace = np.linspace
    cps = types.ModuleType("cupy.sparse")
    cps.coo_matrix = lambda arg, shape: _Sparse(sp.coo_matrix(arg, shape=shape))
    cp.sparse = cps
    sys.modules["cupy"] = cp
    sys.modules["cupy.sparse"] = cps

    for name in ("matplotlib", "matplotlib.pyplot", "sklearn", "sklearn.manifold", "mpl_toolkits"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["matplotlib"].cm = None
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["sklearn.manifold"].TSNE = None
    sys.modules["mpl_toolkits"].mplot3d = None


def _import_reference():
    _install_stubs()
    sys.path.insert(0, os.path.join(REF, "Modules"))
    import tracking_utils
    tracking_utils.scatter_sum = _scatter_sum   # named at :37, never imported by the reference
    return tracking_utils


class Event(dict):
    __getattr__ = dict.__getitem__


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
def random_event(rng, n_particles=150, noise=0.1, big_pids=False):
    sizes = 1 + rng.poisson(9, n_particles)
    if big_pids:
        pids = rng.choice(np.arange(-(1 << 40), 1 << 40, 7919, dtype=np.int64), n_particles, replace=False)
        pids[pids == 0] = 1
    else:
        pids = rng.choice(np.arange(1, 1 << 20, dtype=np.int64), n_particles, replace=False)
    pid = np.repeat(pids, sizes)
    pt_p = (0.3 + rng.exponential(1.0, n_particles)).astype(np.float32)
    pt = (np.repeat(pt_p, sizes) * (1 + 0.05 * rng.random(pid.size))).astype(np.float32)
    prim_p = rng.random(n_particles) < 0.8
    primary = (np.repeat(prim_p, sizes) & (rng.random(pid.size) < 0.5)).astype(np.int64)
    n_noise = int(noise * pid.size)
    pid = np.concatenate([pid, np.zeros(n_noise, np.int64)])
    pt = np.concatenate([pt, np.zeros(n_noise, np.float32)])
    primary = np.concatenate([primary, np.zeros(n_noise, np.int64)])
    perm = rng.permutation(pid.size)
    return pid[perm], pt[perm], primary[perm]


def random_candidates(rng, pid, dup=0.02, labels_signed=False):
    """candidates from the truth: most particles found with some hits lost and a few foreign hits, some split in
    two, some junk candidates of random hits; a few duplicated pairs"""
    hits, cands = [], []
    label = 0
    for p in np.unique(pid):
        if p == 0:
            continue
        h = np.nonzero(pid == p)[0]
        if rng.random() < 0.1:
            continue
        parts = [h] if rng.random() < 0.85 or h.size < 4 else np.array_split(rng.permutation(h), 2)
        for part in parts:
            part = part[rng.random(part.size) < 0.85]
            extra = rng.integers(0, pid.size, rng.poisson(1.0))
            mem = np.concatenate([part, extra])
            hits.append(mem)
            cands.append(np.full(mem.size, label))
            label += 1
    for _ in range(len(cands) // 10):
        mem = rng.integers(0, pid.size, rng.integers(2, 12))
        hits.append(mem)
        cands.append(np.full(mem.size, label))
        label += 1
    hit, cand = np.concatenate(hits).astype(np.int64), np.concatenate(cands).astype(np.int64)
    n_dup = int(dup * hit.size)
    d = rng.integers(0, hit.size, n_dup)
    hit, cand = np.concatenate([hit, hit[d]]), np.concatenate([cand, cand[d]])
    # arbitrary label values, as connected-component roots are
    span = 1 << 40
    vals = rng.choice(np.arange(-span if labels_signed else 0, span, 104729, dtype=np.int64), label, replace=False)
    perm = rng.permutation(hit.size)
    return hit[perm], vals[cand][perm]


def cases():
    rng = np.random.default_rng(20261016)
    out = []

    def add(name, hit, cand, pid, pt, primary, pt_cut=1.0, nhits_cut=5, majority_cut=0.5, use_primary=False):
        out.append(dict(name=name, hit=np.asarray(hit, np.int64), cand=np.asarray(cand, np.int64),
                        pid=np.asarray(pid, np.int64), pt=np.asarray(pt, np.float32),
                        primary=np.asarray(primary, np.int64),
                        params=np.array([pt_cut, nhits_cut, majority_cut, 1.0 if use_primary else 0.0])))

    # random events with noise, both majority cuts, primary off and on
    for k in range(4):
        pid, pt, prim = random_event(rng)
        hit, cand = random_candidates(rng, pid)
        add(f"random{k}_m050", hit, cand, pid, pt, prim)
        add(f"random{k}_m075", hit, cand, pid, pt, prim, majority_cut=0.75)
        add(f"random{k}_m050_primary", hit, cand, pid, pt, prim, use_primary=True)
        add(f"random{k}_m075_primary_pt05_n3", hit, cand, pid, pt, prim, pt_cut=0.5, nhits_cut=3, majority_cut=0.75,
            use_primary=True)

    # negative and 40-bit pids, signed candidate labels
    pid, pt, prim = random_event(rng, big_pids=True)
    hit, cand = random_candidates(rng, pid, labels_signed=True)
    add("pids_40bit_signed", hit, cand, pid, pt, prim)
    add("pids_40bit_signed_primary", hit, cand, pid, pt, prim, use_primary=True)

    # heavy duplicate pairs: coo_matrix sums them
    pid, pt, prim = random_event(rng, n_particles=60)
    hit, cand = random_candidates(rng, pid, dup=0.5)
    add("duplicates", hit, cand, pid, pt, prim)

    # C = 6000 > 4505: the 6-hit particle's 3 + 3 hits land in two candidates with the same hash -> two matches
    C = 6000
    h = np.linspace(1, 1 + 1e-12, C)
    c0 = int(np.nonzero(h[1:] == h[:-1])[0][0])
    pid = np.concatenate([np.full(6, 77), np.zeros(30, np.int64)])
    pt = np.concatenate([np.full(6, 2.0), np.zeros(30)]).astype(np.float32)
    hits, cands = [], []
    for c in range(C):
        if c in (c0, c0 + 1):
            hits.append(np.arange(3) + 3 * (c - c0))
        else:
            hits.append(6 + (np.arange(3) + 3 * c) % 30)
        cands.append(np.full(3, c))
    add("hash_tie_C6000", np.concatenate(hits), np.concatenate(cands), pid, pt, np.ones(pid.size))

    # float32 size filter: 25 * 0.56 = 14.000000000000002 -> float32 14.0, so a 14-pair candidate survives
    pid = np.concatenate([np.full(25, 5), np.full(20, 9), np.zeros(10, np.int64)])
    pt = np.concatenate([np.full(25, 3.0), np.full(20, 2.0), np.zeros(10)]).astype(np.float32)
    hit = np.concatenate([np.arange(14), 25 + np.arange(13), 25 + np.arange(20), 45 + np.arange(10)])
    cand = np.concatenate([np.full(14, 100), np.full(13, 200), np.full(20, 300), np.full(10, 400)])
    add("size_filter_fp32_boundary", hit, cand, pid, pt, np.ones(pid.size), nhits_cut=25, majority_cut=0.56)
    add("size_filter_fp32_boundary_n13", hit, cand, pid, pt, np.ones(pid.size), nhits_cut=13, majority_cut=0.56)

    # float32 pt cut: particles 1, 2, 5 (min pt == float32(0.1)) are not > 0.1 in float32 (they are in float64)
    pid = np.repeat(np.arange(1, 7), 6)
    pt = np.repeat(np.array([0.1, 0.1, 0.2, 0.05, 0.1, 0.3], np.float32), 6)
    hit = np.arange(pid.size)
    cand = np.repeat(np.arange(6) * 3 + 1, 6)
    hit, cand = np.delete(hit, np.arange(14, 18)), np.delete(cand, np.arange(14, 18))   # particle 3 unmatched
    add("pt_cut_fp32_boundary", hit, cand, pid, pt, np.ones(pid.size), pt_cut=0.1)

    # no match: every candidate mixes hits of many particles
    pid, pt, prim = random_event(rng, n_particles=40)
    hit = rng.permutation(pid.size)
    cand = np.arange(pid.size) % 7
    add("no_match_mixed", hit, cand, pid, pt, prim)
    # every match is noise: dropped by the filter
    pid = np.concatenate([np.zeros(12, np.int64), np.full(4, 3)])
    pt = np.zeros(16, np.float32)
    add("no_match_after_filter", np.arange(12), np.zeros(12), pid, pt, np.zeros(16))
    # zero truth particles: track_eff = 0 / 0 = nan
    pid, pt, prim = random_event(rng, n_particles=50)
    hit, cand = random_candidates(rng, pid)
    add("zero_truth_nan", hit, cand, pid, pt, prim, pt_cut=1e9)
    # every candidate below the size filter (the reference raises; defined here as default_response)
    add("all_filtered", hit[:40], np.arange(40), pid, pt, prim)
    add("empty", np.zeros(0), np.zeros(0), pid, pt, prim)

    # NaN pt (a generator of their own: the cases above keep their bytes).  scatter_min (amin) propagates NaN, so a
    # particle with a NaN pt is not reconstructable.  The reference's loader keeps noise hits, whose pt can be NaN:
    # pid 0 with all-NaN pt and more than nhits_cut hits must not count in track_eff's denominator
    rng = np.random.default_rng(20261020)
    pid, pt, prim = random_event(rng, n_particles=40)
    hit, cand = random_candidates(rng, pid)
    assert (pid == 0).sum() >= 5
    pt = pt.copy()
    pt[pid == 0] = np.nan
    add("pt_nan_noise", hit, cand, pid, pt, prim)
    # one real particle with a single NaN hit, otherwise above the cut and matched with 6 of its 8 hits: were it
    # taken for reconstructable, hit_eff would be (6/8 + 1) / 2 instead of 1
    pid = np.concatenate([np.full(8, 11), np.full(6, 12), np.full(7, 13), np.zeros(4, np.int64)])
    pt = np.concatenate([np.full(8, 2.0), np.full(6, 3.0), np.full(7, 0.5), np.zeros(4)]).astype(np.float32)
    pt[5] = np.nan
    hit = np.concatenate([np.arange(6), np.arange(8, 21)])
    cand = np.concatenate([np.full(6, 40), np.full(6, 50), np.full(7, 60)])
    add("pt_nan_mixed", hit, cand, pid, pt, np.ones(pid.size))
    return out


def main():
    tu = _import_reference()
    arrays = {}
    names = []
    for cs in cases():
        pt_cut, nhits_cut, majority_cut, use_primary = cs["params"]
        ev = Event(pid=torch.from_numpy(cs["pid"]), pt=torch.from_numpy(cs["pt"]))
        if use_primary:
            ev["primary"] = torch.from_numpy(cs["primary"])
        bg = torch.from_numpy(np.stack([cs["hit"], cs["cand"]]))
        status = 0   # 0: metrics, 1: default_response, 2: raised
        expected = np.zeros(4)
        try:
            r = tu.eval_metrics(bg, ev, pt_cut=float(pt_cut), nhits_cut=int(nhits_cut),
                                majority_cut=float(majority_cut), primary=bool(use_primary))
            if r is tu.default_response:
                status = 1
            else:
                expected = np.array([r[k] for k in ("track_eff", "track_pur", "hit_eff", "hit_pur")], np.float64)
        except Exception:
            status = 2
        n = cs["name"]
        names.append(n)
        for k in ("hit", "cand", "pid", "pt", "primary", "params"):
            arrays[f"{n}/{k}"] = cs[k]
        arrays[f"{n}/expected"] = expected
        arrays[f"{n}/status"] = np.array(status, np.int64)
        print(f"{n:40s} status={status} {expected}")
    arrays["cases"] = np.array(names)
    with zipfile.ZipFile(OUT, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    with np.errstate(divide="ignore", invalid="ignore"):
        main()
