"""GPU: event preparation on the device (csrc/eventprep.hip, dataset.prepare_event_device) against the reference's own
``TrackMLDataset.__getitem__`` (tests/golden/dataset_masking.npz) and against ``prepare_event`` on the CPU, which
tests/test_dataset.py pins to that fixture.  Nothing here rounds, so every comparison is exact equality of every key,
dtype and shape.

Shapes: N in {1, 63, 64, 65, 257, 20011} and E in {0, 1, 255, 256, 257, 70001} walk round the workgroup size (256) and
the wavefront (64); the last pair is past rocprim's single-workgroup scan and sort (a few thousand items), so the
look-back scan and the multi-pass radix sort run.  The kernels' grids are capped at 2048 x 256 = 524288 threads and
loop beyond that; every shape above stays inside one trip, so ``test_second_grid_trip`` adds N = 140001 (x 4 columns
in the gather) and E = 600001, where every kernel makes a second one.  ``test_raw_entries_stay_in_bounds`` calls the
C entries on poisoned buffers with guard zones."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from conftest import load_golden
from hierarchicalgnn_amd import dataset as D
from hierarchicalgnn_amd.dataset import (TrackMLDataset, particle_hit_counts, prepare_event, prepare_event_device,
                                         save_event)

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (N, E, E_modulewise, E_signal, pid kind)
SHAPES = [(1, 0, 0, 3, "mixed"), (63, 1, 2, 0, "mixed"), (64, 255, 100, 17, "mixed"), (65, 256, 64, 300, "mixed"),
          (257, 257, 513, 129, "one"), (257, 257, 513, 129, "mixed"), (20011, 70001, 9001, 4999, "mixed")]
FLAGS = list(itertools.product((False, True), repeat=3))          # noise, remove_isolated, primary
PTCUTS = (0, 0.1, 1.0)


def make_event(n, e, e_mod, e_sig, kind="mixed", seed=0):
    """a seeded CPU event; ``mixed`` pids: zeros (noise), negative ids, ids above 2^32, about six hits per particle"""
    g = torch.Generator().manual_seed(1000 + seed + 7 * n + e)
    if kind == "one":
        pid = torch.full((n,), 7, dtype=torch.int64)
    else:
        n_part = max(1, n // 6)
        pool = torch.randint(-(1 << 40), 1 << 40, (n_part,), generator=g)
        pool[::3] += 1 << 33                                          # above 2^32 whatever the draw
        pool[1::3] = -pool[1::3].abs() - 1                            # negative
        pid = pool[torch.randint(0, n_part, (n,), generator=g)]
        pid[torch.rand(n, generator=g) < 0.15] = 0
    pt = (torch.rand(n, generator=g) * 2).float()
    pt[torch.rand(n, generator=g) < 0.1] = np.float32(0.1).item()     # exactly on the 0.1 cut
    ri = lambda m: torch.randint(0, max(n, 1), (2, m), generator=g)   # noqa: E731
    return {"x": torch.randn(n, 3, generator=g), "cell_data": torch.randn(n, 4, generator=g), "pid": pid,
            "hid": torch.randperm(n, generator=g), "pt": pt, "edge_index": ri(e), "modulewise_true_edges": ri(e_mod),
            "signal_true_edges": ri(e_sig), "y": torch.rand(e, generator=g) < 0.3,
            "y_pid": torch.rand(e, generator=g) < 0.4, "primary": torch.randint(0, 2, (n,), generator=g)}


def hp(noise=False, remove_isolated=False, primary=False, hard_ptcut=0, n_hits=3, ratio=0.0):
    return {"noise": noise, "remove_isolated": remove_isolated, "primary": primary, "hard_ptcut": hard_ptcut,
            "n_hits": n_hits, "edge_dropping_ratio": ratio}


def to_dev(ev):
    return {k: v.to(DEV) for k, v in ev.items()}


def assert_same(got, ref, what=""):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k, r in ref.items():
        r = torch.from_numpy(r) if isinstance(r, np.ndarray) else r
        g = got[k]
        assert g.is_cuda and g.dtype == r.dtype and g.shape == r.shape, (what, k, g.dtype, tuple(g.shape),
                                                                         r.dtype, tuple(r.shape))
        assert torch.equal(g.cpu(), r), (what, k)


def _golden_case(z, ci):
    pre = f"case{ci}."
    ev = {k[len(pre + "in."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre + "in.")}
    hparams = {k[len(pre + "hp."):]: z[k].item() for k in z.files if k.startswith(pre + "hp.")}
    out = {k[len(pre + "out."):]: z[k] for k in z.files if k.startswith(pre + "out.")}
    return ev, hparams, out


# 1 ---------------------------------------------------------------- the reference's own output
def test_golden_fixture():
    z = load_golden("dataset_masking.npz")
    assert int(z["n_cases"]) == 3
    for ci in range(int(z["n_cases"])):
        ev, hparams, ref = _golden_case(z, ci)
        dev_ev = to_dev(ev)
        reads = D.stats["host_reads"]
        got = prepare_event_device(dev_ev, hparams)
        assert D.stats["host_reads"] == reads + 1
        assert_same(got, ref, f"case{ci}")
        assert all(torch.equal(dev_ev[k].cpu(), ev[k]) for k in ev), "inputs were written"


# 2 ---------------------------------------------------------------- prepare_event on the CPU
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"N{s[0]}-E{s[1]}-{s[4]}")
def test_matches_prepare_event(shape):
    ev = make_event(*shape)
    dev_ev = to_dev(ev)
    for (noise, isolated, primary), cut in itertools.product(FLAGS, PTCUTS):
        hparams = hp(noise, isolated, primary, cut)
        assert_same(prepare_event_device(dev_ev, hparams), prepare_event(ev, hparams), str((shape, hparams)))
    assert all(torch.equal(dev_ev[k].cpu(), ev[k]) for k in ev), "inputs were written"


def test_second_grid_trip():
    ev = make_event(140001, 600001, 9001, 4999)
    dev_ev = to_dev(ev)
    for hparams in (hp(remove_isolated=True, primary=True, hard_ptcut=0.1), hp(noise=True)):
        assert_same(prepare_event_device(dev_ev, hparams), prepare_event(ev, hparams), str(hparams))


# 3 ---------------------------------------------------------------- the float32 comparison
def test_ptcut_is_compared_in_float32():
    ev = make_event(65, 256, 64, 30)
    ev["pid"] = torch.arange(1, 66)
    ev["pt"] = torch.full((65,), 0.5)
    ev["pt"][3] = np.float32(0.1).item()        # float32(0.1) > 0.1 in double, not in float32
    ev["pt"][9] = float("nan")
    ev["pt"][11] = np.nextafter(np.float32(0.1), np.float32(1)).item()
    got = prepare_event_device(to_dev(ev), hp(hard_ptcut=0.1))
    kept = got["inverse_mask"].cpu().tolist()
    assert 3 not in kept and 9 not in kept and 11 in kept and len(kept) == 63
    assert_same(got, prepare_event(ev, hp(hard_ptcut=0.1)))
    got = prepare_event_device(to_dev(ev), hp())
    assert got["inverse_mask"].cpu().tolist() == list(range(65))       # NaN pt kept without a cut
    assert_same({k: v for k, v in got.items() if k != "pt"},
                {k: v for k, v in prepare_event(ev, hp()).items() if k != "pt"})
    assert torch.equal(got["pt"].cpu().view(torch.int32), prepare_event(ev, hp())["pt"].view(torch.int32))  # NaN bits


# 4 ---------------------------------------------------------------- edge dropping
@pytest.mark.parametrize("isolated", [False, True])
def test_edge_dropping(isolated):
    ev = make_event(257, 4097, 513, 129)
    dev_ev = to_dev(ev)
    hparams = hp(remove_isolated=isolated, ratio=0.3)
    seeded = lambda: torch.Generator().manual_seed(5)                  # noqa: E731
    ref = prepare_event(ev, hparams, generator=seeded())
    assert ref["edge_index"].shape[1] < prepare_event(ev, hp(remove_isolated=isolated))["edge_index"].shape[1]
    assert_same(prepare_event_device(dev_ev, hparams, generator=seeded()), ref, "seeded CPU generator")
    # an explicit mask wins over the generator; the CPU result with that mask is the seeded one
    keep = torch.rand(4097, generator=seeded()) >= 0.3
    for k in (keep, keep.to(DEV)):
        assert_same(prepare_event_device(dev_ev, hparams, generator=torch.Generator().manual_seed(99), edge_keep=k),
                    ref, "explicit edge_keep")
    all_true = prepare_event_device(dev_ev, hparams, edge_keep=torch.ones(4097, dtype=torch.bool))
    assert_same(all_true, prepare_event(ev, hp(remove_isolated=isolated)), "all-true mask")
    none = prepare_event_device(dev_ev, hparams, edge_keep=torch.zeros(4097, dtype=torch.bool))
    assert_same(none, prepare_event(ev, hp(remove_isolated=isolated, ratio=2.0)), "all-false mask")
    assert none["edge_index"].shape == (2, 0) and none["y"].shape == (0,)
    # generator=None: drawn on the device; a valid filtering of the undropped result, in input order
    got = prepare_event_device(dev_ev, hparams)
    full = all_true["edge_index"].cpu()
    key = lambda t: (t[0] * 257 + t[1]).tolist()                       # noqa: E731
    it = iter(key(full))
    assert 0 < got["edge_index"].shape[1] < full.shape[1] and all(k in it for k in key(got["edge_index"].cpu()))


# 5 ---------------------------------------------------------------- degenerate events
def test_degenerate_events():
    ev = make_event(257, 257, 513, 129)
    ev["pid"] = torch.zeros(257, dtype=torch.int64)
    got = prepare_event_device(to_dev(ev), hp())                       # every hit is noise
    assert_same(got, prepare_event(ev, hp()))
    assert got["inverse_mask"].shape == (0,) and got["x"].shape == (0, 3) and got["nhits"].shape == (257,)
    assert all(got[k].shape == (2, 0) for k in D.EDGE_LISTS)
    got = prepare_event_device(to_dev(ev), hp(noise=True))             # no hit masked
    assert_same(got, prepare_event(ev, hp(noise=True)))
    assert got["inverse_mask"].cpu().tolist() == list(range(257)) and got["edge_index"].shape == (2, 257)
    ev = make_event(65, 0, 64, 30)
    got = prepare_event_device(to_dev(ev), hp(noise=True, remove_isolated=True))   # E = 0: every hit is isolated
    assert_same(got, prepare_event(ev, hp(noise=True, remove_isolated=True)))
    assert got["inverse_mask"].shape == (0,) and got["modulewise_true_edges"].shape == (2, 0)


# 6 ---------------------------------------------------------------- nhits on its own
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"N{s[0]}-{s[4]}")
def test_particle_hit_counts(shape):
    pid = make_event(*shape)["pid"]
    _, inverse, counts = pid.unique(return_inverse=True, return_counts=True)
    reads = D.stats["host_reads"]
    got = particle_hit_counts(pid.to(DEV))
    assert D.stats["host_reads"] == reads
    assert got.is_cuda and got.dtype == torch.int64 and torch.equal(got.cpu(), counts[inverse])
    assert particle_hit_counts(torch.empty(0, dtype=torch.int64, device=DEV)).shape == (0,)


# 7 ---------------------------------------------------------------- ids outside [0, N): an error, never an address
@pytest.mark.parametrize("which", D.EDGE_LISTS)
@pytest.mark.parametrize("bad", ["N", -1])
@pytest.mark.parametrize("isolated", [False, True])
def test_bad_ids_raise(which, bad, isolated):
    ev = make_event(65, 256, 64, 30)
    ev[which] = ev[which].clone()
    ev[which][1, ev[which].shape[1] // 2] = 65 if bad == "N" else -1
    with pytest.raises(ValueError, match="outside"):
        prepare_event_device(to_dev(ev), hp(noise=True, remove_isolated=isolated))
    ev = make_event(65, 256, 64, 30)                                   # and the next call is well
    assert_same(prepare_event_device(to_dev(ev), hp()), prepare_event(ev, hp()))


# 8 ---------------------------------------------------------------- determinism and hygiene
def test_determinism_and_hygiene():
    ev = make_event(20011, 70001, 9001, 4999)
    dev_ev = to_dev(ev)
    hparams = hp(remove_isolated=True, primary=True, hard_ptcut=0.1)
    a, b = prepare_event_device(dev_ev, hparams), prepare_event_device(dev_ev, hparams)
    assert_same(a, {k: v.cpu() for k, v in b.items()})
    ins = {v.untyped_storage().data_ptr() for v in dev_ev.values()}
    outs = [v.untyped_storage().data_ptr() for v in a.values() if v.numel()]
    assert len(set(outs)) == len(outs) and not ins & set(outs)
    assert all(v.is_contiguous() and v.device == dev_ev["pid"].device for v in a.values())


# 9 ---------------------------------------------------------------- the dataset
def test_device_dataset(tmp_path):
    ev = make_event(257, 257, 513, 129)
    path = str(tmp_path / "event0.npz")
    save_event(path, ev)
    hparams = hp(remove_isolated=True, primary=True)
    cpu_item = TrackMLDataset([path], hparams, stage="train")[0]
    item = TrackMLDataset([path], hparams, stage="train", device=DEV)[0]
    assert item.pop("dir") == cpu_item.pop("dir") == path
    assert_same(item, cpu_item)


# ------------------------------------------------------------------ the C entries on poisoned buffers
GUARD, POISON = 64, 0x5A


def _guarded(n, dtype):
    """(buffer of poison bytes, its middle n elements as ``dtype``) with GUARD elements on either side"""
    size = torch.empty(0, dtype=dtype).element_size()
    buf = torch.full(((n + 2 * GUARD) * size,), POISON, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD * size:(GUARD + n) * size].view(dtype)


def _guards_intact(buf, n, dtype):
    size = torch.empty(0, dtype=dtype).element_size()
    return bool((buf[:GUARD * size] == POISON).all()) and bool((buf[(GUARD + n) * size:] == POISON).all())


def test_raw_entries_stay_in_bounds():
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    n, e = 257, 300
    ev = make_event(n, e, 64, 30)
    ev["edge_index"][0, 5], ev["edge_index"][1, 7] = n, -1               # two ids the kernels must skip
    d = to_dev(ev)
    stream = _lib.current_stream(torch.device(DEV))
    vp = lambda t: ctypes.c_void_p(t.data_ptr())                          # noqa: E731
    nb = ctypes.c_size_t(0)
    _lib.check(lib.hgnn_event_nodes_workspace_bytes(n, e, ctypes.byref(nb)))
    ws = torch.full((nb.value + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    outs = {"new_id": (n, torch.int32), "pt": (n, torch.float32), "nhits": (n, torch.int64), "signal": (n, torch.bool),
            "info": (_lib.EP_INFO, torch.int64)}
    bufs = {k: _guarded(*v) for k, v in outs.items()}
    flags = _lib.EP_REMOVE_ISOLATED | _lib.EP_USE_PRIMARY
    _lib.check(lib.hgnn_event_nodes(vp(d["pid"]), vp(d["pt"]), vp(d["primary"]), vp(d["edge_index"]), n, e, 0.1, 3,
                                    flags, *(vp(bufs[k][1]) for k in ("new_id", "pt", "nhits", "signal", "info")),
                                    vp(ws), nb.value, stream), "hgnn_event_nodes")
    torch.cuda.synchronize()
    assert all(_guards_intact(bufs[k][0], *outs[k]) for k in outs) and bool((ws[nb.value:] == POISON).all())
    new_id, info = bufs["new_id"][1], bufs["info"][1]
    n_kept = int(info[_lib.EP_N_NODES])
    assert int(info[_lib.EP_STATUS]) == _lib.EP_ST_BAD_ID and n_kept == int((new_id >= 0).sum())
    _, inverse, counts = ev["pid"].unique(return_inverse=True, return_counts=True)
    assert torch.equal(bufs["nhits"][1].cpu(), counts[inverse])
    touched = torch.zeros(n, dtype=torch.bool)
    touched[ev["edge_index"][(ev["edge_index"] >= 0) & (ev["edge_index"] < n)]] = True
    keep = (ev["pid"] != 0) & (ev["pt"] > 0.1) & touched
    assert torch.equal(new_id.cpu() >= 0, keep) and torch.equal(new_id.cpu()[keep].long(), torch.arange(n_kept))
    assert torch.equal(bufs["signal"][1].cpu(), (counts[inverse] >= 3) & (ev["primary"] == 1))
    # the edge stage of edge_index: the two bad edges are dropped, the status bit is set again, nothing else written
    _lib.check(lib.hgnn_event_edges_workspace_bytes(e, ctypes.byref(nb)))
    ws = torch.full((nb.value + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    cbuf, cnt = _guarded(2, torch.int64)
    cnt.zero_()
    _lib.check(lib.hgnn_event_edges_count(vp(d["edge_index"]), e, None, vp(new_id), n, vp(cnt), vp(cnt[1:]), vp(ws),
                                          nb.value, stream), "hgnn_event_edges_count")
    torch.cuda.synchronize()
    count, status = cnt.tolist()
    good = torch.ones(e, dtype=torch.bool)
    good[5] = good[7] = False
    kept = new_id.cpu()[ev["edge_index"].clamp(0, n - 1)].ge(0).all(0) & good
    assert status == _lib.EP_ST_BAD_ID and count == int(kept.sum()) and _guards_intact(cbuf, 2, torch.int64)
    obuf, out = _guarded(2 * count, torch.int64)
    ybuf, y_out = _guarded(count, torch.bool)
    _lib.check(lib.hgnn_event_edges_fill(vp(d["edge_index"]), e, None, vp(new_id), n, vp(d["y"]), None, vp(out), count,
                                         vp(y_out), None, vp(ws), nb.value, stream), "hgnn_event_edges_fill")
    torch.cuda.synchronize()
    assert _guards_intact(obuf, 2 * count, torch.int64) and _guards_intact(ybuf, count, torch.bool)
    assert bool((ws[nb.value:] == POISON).all())
    assert torch.equal(out.view(2, count).cpu(), new_id.cpu()[ev["edge_index"][:, kept]].long())
    assert torch.equal(y_out.cpu(), ev["y"][kept])
    # the gather: a row whose index is outside [0, n_rows) is zero-filled
    index = torch.tensor([3, n, 0, -1, n - 1], device=DEV)
    for src in (d["x"], d["pid"], d["y"][:n].contiguous()):
        cols = src[0].numel()
        gbuf, g = _guarded(5 * cols, src.dtype)
        _lib.check(lib.hgnn_event_gather_rows(vp(src), n, cols, src.element_size(), vp(index), 5, vp(g), stream))
        torch.cuda.synchronize()
        want = src[index.clamp(0, n - 1)].clone()
        want[1], want[3] = 0, 0
        assert _guards_intact(gbuf, 5 * cols, src.dtype) and torch.equal(g.view(want.shape), want)
