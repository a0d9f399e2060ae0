"""CPU: the public surface of the row-local pair construction (no GPU needed): exports, the C ABI additions, the
argument errors -- raised before anything touches a device -- and the loud refusal of CPU tensors."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import conftest

HP = dict(train_r=1.0, knn=4, true_edges="modulewise_true_edges")


def _batch(n=6, t=3):
    return {"modulewise_true_edges": torch.zeros((2, t), dtype=torch.int64), "signal_mask": torch.ones(n, dtype=torch.bool),
            "pid": torch.zeros(n, dtype=torch.int64)}


def _idx(n=6, k=4):
    return torch.full((n, k), -1, dtype=torch.int64)


def test_exports_and_signatures():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import embedding
    assert H.training_pairs is embedding.training_pairs
    assert inspect.signature(embedding.training_samples).parameters["fused"].default is False
    for fn in (embedding.embedding_in_training_loss, embedding.embedding_hgnn_training_loss):
        assert inspect.signature(fn).parameters["fused_samples"].default is False


def test_header_constants_and_entry_points():
    from hierarchicalgnn_amd import _lib
    txt = open(os.path.join(conftest.ROOT, "include", "hgnn_hip.h")).read()
    assert int(re.search(r"#define\s+HGNN_ABI_VERSION\s+(\d+)", txt).group(1)) == _lib.ABI_VERSION == 26
    tp = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+HGNN_TP_(\w+)\s+(\d+)", txt)}
    assert set(tp) == {"MAX_K", "MODE_MODULEWISE", "MODE_PID", "ST_BAD_IDX", "ST_BAD_MTE", "P", "N_ROW", "N_TRUTH",
                       "STATUS", "INFO"}
    assert all(getattr(_lib, "TP_" + k) == v for k, v in tp.items()) and tp["MAX_K"] == 128
    for name in ("hgnn_training_pairs_workspace_bytes", "hgnn_training_pairs_count", "hgnn_training_pairs_fill"):
        assert name in _lib.declared_symbols() and name + "(" in txt
    assert "hgnn_training_pairs_fill with HGNN_TP_*" in txt.split("#define HGNN_ABI_VERSION")[0]   # un-bumped list


def test_argument_checks_of_the_library_are_host_side():
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    q = lib.hgnn_training_pairs_workspace_bytes
    assert q(100, 0, 10, 0, ctypes.byref(nb)) != 0 and b"K = 0" in lib.hgnn_last_error()
    assert q(100, 129, 10, 0, ctypes.byref(nb)) != 0 and b"[1, 128]" in lib.hgnn_last_error()
    assert q(-1, 4, 10, 0, ctypes.byref(nb)) != 0
    assert q(100, 4, -1, 0, ctypes.byref(nb)) != 0
    assert q(100, 4, 10, 2, ctypes.byref(nb)) != 0 and b"mode" in lib.hgnn_last_error()
    assert q(1 << 25, 128, 0, 0, ctypes.byref(nb)) != 0 and b"int32" in lib.hgnn_last_error()
    assert q(100, 4, 10, 0, None) != 0
    info = (ctypes.c_int64 * 4)()
    assert lib.hgnn_training_pairs_count(None, 10, 129, None, 0, None, None, 0, info, None, 0, None) != 0
    assert lib.hgnn_training_pairs_count(None, 10, 4, None, 0, None, None, 0, None, None, 0, None) != 0
    assert lib.hgnn_training_pairs_fill(None, 10, 4, None, 0, None, None, 0, None, None, 41, None, 0, None) != 0
    assert b"cap" in lib.hgnn_last_error()


@pytest.mark.parametrize("what,make", [
    ("idx int32", lambda: (_idx().int(), _batch())),
    ("idx 1-d", lambda: (_idx().reshape(-1), _batch())),
    ("idx not a tensor", lambda: (_idx().tolist(), _batch())),
    ("K = 0", lambda: (_idx(6, 0), _batch())),
    ("K = 129", lambda: (_idx(6, 129), _batch())),
    ("mte int32", lambda: (_idx(), dict(_batch(), modulewise_true_edges=torch.zeros((2, 3), dtype=torch.int32)))),
    ("mte [3, T]", lambda: (_idx(), dict(_batch(), modulewise_true_edges=torch.zeros((3, 3), dtype=torch.int64)))),
    ("mte 1-d", lambda: (_idx(), dict(_batch(), modulewise_true_edges=torch.zeros(6, dtype=torch.int64)))),
    ("signal_mask uint8", lambda: (_idx(), dict(_batch(), signal_mask=torch.ones(6, dtype=torch.uint8)))),
    ("signal_mask length", lambda: (_idx(), dict(_batch(), signal_mask=torch.ones(5, dtype=torch.bool)))),
    ("pid int32", lambda: (_idx(), dict(_batch(), pid=torch.zeros(6, dtype=torch.int32)))),
    ("pid length", lambda: (_idx(), dict(_batch(), pid=torch.zeros(7, dtype=torch.int64)))),
    ("pid [N, 1]", lambda: (_idx(), dict(_batch(), pid=torch.zeros((6, 1), dtype=torch.int64)))),
    ("devices", lambda: (_idx(), dict(_batch(), pid=torch.zeros(6, dtype=torch.int64, device="meta")))),
])
def test_argument_errors_are_raised_before_any_launch(what, make):
    import hierarchicalgnn_amd as H
    idx, batch = make()
    with pytest.raises(ValueError, match="training_pairs"):
        H.training_pairs(idx, batch, HP)


def test_unknown_mode_is_a_value_error():
    import hierarchicalgnn_amd as H
    with pytest.raises(ValueError, match="true_edges"):
        H.training_pairs(_idx(), _batch(), dict(HP, true_edges="truth"))


def test_cpu_tensors_are_refused_loudly():
    import hierarchicalgnn_amd as H
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.training_pairs(_idx(), _batch(), HP)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.training_pairs(_idx(0, 4), _batch(0, 0), HP)


def test_fused_training_samples_on_cpu_tensors():
    """fails before the feature with a TypeError: training_samples has no ``fused``"""
    import hierarchicalgnn_amd as H
    emb = torch.nn.functional.normalize(torch.randn(6, 8), dim=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.training_samples(emb, _batch(), HP, fused=True)
    with pytest.raises(ValueError, match="prediction_graph"):
        H.training_samples(emb, _batch(), HP, prediction_graph=torch.zeros((2, 1), dtype=torch.int64), fused=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.embedding_in_training_loss(emb, dict(_batch(), pt=torch.ones(6)), HP, fused_samples=True)
