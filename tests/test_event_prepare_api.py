"""The host side of device event preparation (dataset.prepare_event_device, particle_hit_counts, TrackMLDataset's
``device``): argument checks, the no-CPU-path error, the unchanged CPU dataset.  No GPU."""
import pytest
import torch

import hierarchicalgnn_amd as H
from conftest import load_golden
from hierarchicalgnn_amd import _lib
from hierarchicalgnn_amd import dataset as D


def _event(n=12, e=20):
    g = torch.Generator().manual_seed(3)
    ri = lambda m: torch.randint(0, n, (2, m), generator=g)           # noqa: E731
    return {"x": torch.randn(n, 3, generator=g), "cell_data": torch.randn(n, 4, generator=g),
            "pid": torch.randint(0, 4, (n,), generator=g), "hid": torch.arange(n), "pt": torch.rand(n, generator=g),
            "edge_index": ri(e), "modulewise_true_edges": ri(7), "signal_true_edges": ri(5),
            "y": torch.rand(e, generator=g) < 0.5, "y_pid": torch.rand(e, generator=g) < 0.5,
            "primary": torch.randint(0, 2, (n,), generator=g)}


HP = {"noise": False, "remove_isolated": True, "primary": True, "hard_ptcut": 0.5, "n_hits": 3,
      "edge_dropping_ratio": 0.0}


def test_new_names_are_exported():
    for name in ("prepare_event_device", "particle_hit_counts", "TrackMLDataset"):
        assert getattr(H, name) is getattr(D, name)
    assert D.stats["host_reads"] >= 0


def test_cpu_tensors_have_no_path():
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.prepare_event_device(_event(), HP)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.particle_hit_counts(torch.arange(5))


@pytest.fixture
def no_library(monkeypatch):
    """any request to the library is a failure"""
    def refuse(*a, **k):
        raise AssertionError("the library was asked before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "workspace", refuse)


@pytest.mark.parametrize("key,value", [
    ("pid", torch.zeros(12, dtype=torch.int32)), ("hid", torch.zeros(12, dtype=torch.int32)),
    ("pt", torch.zeros(12, dtype=torch.float64)), ("x", torch.zeros(12, 3, dtype=torch.float64)),
    ("cell_data", torch.zeros(12, 4, dtype=torch.float16)), ("edge_index", torch.zeros(2, 20, dtype=torch.int32)),
    ("modulewise_true_edges", torch.zeros(2, 7, dtype=torch.int32)),
    ("signal_true_edges", torch.zeros(2, 5, dtype=torch.float32)), ("y", torch.zeros(20, dtype=torch.uint8)),
    ("y_pid", torch.zeros(20, dtype=torch.float32)), ("primary", torch.zeros(12, dtype=torch.bool)),
    # lengths and shapes
    ("pt", torch.zeros(11)), ("hid", torch.zeros(13, dtype=torch.int64)), ("x", torch.zeros(11, 3)),
    ("cell_data", torch.zeros(12)), ("y", torch.zeros(19, dtype=torch.bool)),
    ("y_pid", torch.zeros(21, dtype=torch.bool)), ("edge_index", torch.zeros(20, 2, dtype=torch.int64)),
    ("signal_true_edges", torch.zeros(5, dtype=torch.int64)), ("primary", torch.zeros(11, dtype=torch.int64)),
    ("pid", torch.zeros(12, 1, dtype=torch.int64)), ("primary", None), ("pid", None),
])
def test_argument_errors_come_before_the_library(no_library, key, value):
    ev = _event()
    if value is None:
        del ev[key]
    else:
        ev[key] = value
    with pytest.raises(ValueError, match=key):
        H.prepare_event_device(ev, HP)


def test_edge_keep_and_pid_argument_errors(no_library):
    for keep in (torch.ones(19, dtype=torch.bool), torch.ones(20, dtype=torch.uint8), [True] * 20):
        with pytest.raises(ValueError, match="edge_keep"):
            H.prepare_event_device(_event(), dict(HP, edge_dropping_ratio=0.5), edge_keep=keep)
    for pid in (torch.zeros(4, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64), [1, 2]):
        with pytest.raises(ValueError, match="pid"):
            H.particle_hit_counts(pid)


def test_primary_is_optional_without_the_hparam(no_library):
    ev = _event()
    del ev["primary"]
    with pytest.raises(RuntimeError, match="no CPU path"):            # past the checks, stopped at the device check
        H.prepare_event_device(ev, dict(HP, primary=False))


def test_default_dataset_is_the_cpu_path(tmp_path):
    z = load_golden("dataset_masking.npz")
    for ci in range(int(z["n_cases"])):
        pre = f"case{ci}."
        ev = {k[len(pre + "in."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre + "in.")}
        hparams = {k[len(pre + "hp."):]: z[k].item() for k in z.files if k.startswith(pre + "hp.")}
        path = str(tmp_path / f"event{ci}.npz")
        D.save_event(path, ev)
        want = D.prepare_event(D.load_event(path), hparams)
        for ds in (H.TrackMLDataset([path], hparams, "train"), H.TrackMLDataset([path], hparams, "train", "cpu"),
                   H.TrackMLDataset([path], hparams, "train", torch.device("cpu"))):
            item = ds[0]
            assert item.pop("dir") == path and list(item) == list(want)
            for k, v in want.items():
                assert item[k].device.type == "cpu" and item[k].dtype == v.dtype and torch.equal(item[k], v), (ci, k)


def test_c_entries_check_their_sizes_on_the_host():
    import ctypes
    lib = _lib.load()
    nb = ctypes.c_size_t(7)
    bad = 1                                                           # HGNN_ERR_INVALID_ARG
    assert lib.hgnn_event_nodes_workspace_bytes(1 << 31, 0, ctypes.byref(nb)) == bad
    assert b"2^31" in lib.hgnn_last_error()
    assert lib.hgnn_event_nodes_workspace_bytes(4, 1 << 31, ctypes.byref(nb)) == bad
    assert lib.hgnn_event_edges_workspace_bytes(-1, ctypes.byref(nb)) == bad
    assert lib.hgnn_event_hit_counts_workspace_bytes(1 << 31, ctypes.byref(nb)) == bad
    assert lib.hgnn_event_edges_workspace_bytes(4, None) == bad
    assert lib.hgnn_event_gather_rows(None, 4, 1, 3, None, 4, None, None) == bad
    assert b"elem_bytes" in lib.hgnn_last_error()
    assert lib.hgnn_event_nodes(None, None, None, None, 4, 0, 0.0, 3, 8, None, None, None, None, None, None, 0,
                                None) == bad and b"flag" in lib.hgnn_last_error()
    # empty inputs need no scratch and no device
    for fn, args in ((lib.hgnn_event_nodes_workspace_bytes, (0, 0)), (lib.hgnn_event_edges_workspace_bytes, (0,)),
                     (lib.hgnn_event_hit_counts_workspace_bytes, (0,))):
        assert fn(*args, ctypes.byref(nb)) == _lib.HGNN_OK and nb.value <= 4096
    assert lib.hgnn_event_gather_rows(None, 0, 3, 4, None, 0, None, None) == _lib.HGNN_OK
    assert lib.hgnn_event_inverse_mask(None, 0, None, 0, None) == _lib.HGNN_OK
