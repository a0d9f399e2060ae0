"""GPU: exact conformance of hgnn_track_eval (csrc/trackeval.hip) at its launch edges, against the float64 restatement
(tests/tracking_ref.py) on the cases of tests/tracking_exact_cases.py (proved by tests/test_tracking_exact_ref.py).

Every case is run without and with ``primary`` and all 12 entries of result[HGNN_TE_*] are compared on bits (every
NaN counts as the same NaN: its sign and payload are not part of the contract).  On a no_match case the restatement
defines neither n_mask / n_truth nor the four raw ratios; there ``eval_metrics`` must return ``default_response``.

  * buffers: through ctypes with a workspace of exactly the reported size between guard zones, filled with 0xFF
    twice and with 0x00 twice (``ccol`` is written for kept candidates only, ``prow_*`` rely on a memset): the same
    bits four times, the restatement's.
  * a side stream; ``bipartite_graph`` as an int32 tensor and as a non-contiguous view (the wrapper converts both).

Measured wall time on an MI355X: 1.3 s for the file (104 tests); the slowest test takes 0.22 s (the first call).

Wrong kernel run once on an MI355X against this file (a library variant built outside the tree): k_te_particles
selecting ``v < m ? v : m`` (a NaN pt never selected, the behaviour before the fix) failed the four edge_nan_* cases
here and the two pt_nan_* fixture cases of tests/test_gpu_tracking.py."""
import ctypes

import numpy as np
import pytest
import torch

import tracking_exact_cases as X
import tracking_ref as T
from test_gpu_scalar_ops_exact import Workspace, assert_bits, on_side_stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = (False, True)
QNAN = np.float64(np.nan)


def _H():
    import hierarchicalgnn_amd
    return hierarchicalgnn_amd


def _event(c):
    return {k: torch.from_numpy(c[k]).to(DEV) for k in ("pid", "pt", "primary")}


def _graph(c):
    return torch.from_numpy(np.stack([c["hit"], c["cand"]])).to(DEV)


def _canon(v):
    v = np.array(v, np.float64)
    v[np.isnan(v)] = QNAN
    return v


def _check(c, use_primary, got, what=""):
    want, idx, ref = X.expected(c, use_primary)
    what = f"{c['name']} primary={use_primary}{what}"
    got = np.asarray(got, np.float64)
    assert got.shape == (len(X.RESULT),)
    for i in idx:
        assert_bits(_canon(got[i:i + 1]), _canon(want[i:i + 1]), f"{what}: {X.RESULT[i]}")
    return ref


def _params(c):
    return dict(pt_cut=c["pt_cut"], nhits_cut=c["nhits_cut"], majority_cut=c["majority_cut"])


def _run(c, use_primary, bg=None):
    from hierarchicalgnn_amd import tracking
    r = tracking.track_eval(_graph(c) if bg is None else bg, _event(c), primary=use_primary, **_params(c))
    return r.cpu().numpy()


@pytest.mark.parametrize("name", X.NAMES)
def test_case_matches_the_restatement(name):
    c = X.CASES[name]
    for use_primary in MODES:
        ref = _check(c, use_primary, _run(c, use_primary))
        got = _H().eval_metrics(_graph(c), _event(c), primary=use_primary, **_params(c))
        if ref["no_match"]:
            assert got == {k: 0 for k in T.KEYS} and all(type(v) is int for v in got.values()), (name, got)
        else:
            assert all(type(v) is float for v in got.values())
            assert_bits(_canon([got[k] for k in T.KEYS]), _canon([ref[k] for k in T.KEYS]), f"{name}: eval_metrics")


def _ctypes_call(c, use_primary, fill):
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    B, N = int(c["hit"].size), int(c["pid"].size)
    nb = ctypes.c_size_t(0)
    _lib.check(lib.hgnn_track_eval_workspace_bytes(B, N, ctypes.byref(nb)), "hgnn_track_eval_workspace_bytes")
    ws = Workspace(nb.value, fill)
    t = {k: torch.from_numpy(c[k]).to(DEV) for k in ("hit", "cand", "pid", "pt", "primary")}
    result = torch.full((_lib.TE_RESULT,), -7.0, dtype=torch.float64, device=DEV)
    _lib.check(lib.hgnn_track_eval(_lib.ptr(t["hit"]), _lib.ptr(t["cand"]), B, _lib.ptr(t["pid"]), _lib.ptr(t["pt"]),
                                   _lib.ptr(t["primary"]) if use_primary else None, N, float(c["pt_cut"]),
                                   float(c["nhits_cut"]), float(c["majority_cut"]), _lib.ptr(result), ws.ptr(),
                                   nb.value, _lib.current_stream(result.device)), "hgnn_track_eval")
    torch.cuda.synchronize()
    ws.done(f"{c['name']} fill {fill:#x}")
    return result.cpu().numpy()


@pytest.mark.parametrize("name", ["fill_b257_n255", "fill_b3_n512", "spread_65_big", "hits_129_prim", "parts_257",
                                  "edge_size_eq", "edge_all_filtered", "edge_no_pairs"])
def test_poisoned_exact_size_workspace(name):
    c = X.CASES[name]
    for use_primary in MODES:
        runs = [_ctypes_call(c, use_primary, fill) for fill in (0xFF, 0xFF, 0x00, 0x00)]
        _, idx, _ = X.expected(c, use_primary)
        for r, fill in zip(runs, ("0xff", "0xff again", "0x00", "0x00 again")):
            _check(c, use_primary, r, f" (workspace filled with {fill})")
            assert_bits(_canon(r[idx]), _canon(runs[0][idx]), f"{name}: run with {fill} against the first")


def test_side_stream():
    c = X.CASES["parts_8193"]
    for use_primary in MODES:
        _check(c, use_primary, on_side_stream(lambda: _run(c, use_primary)), " (side stream)")


def test_int32_and_non_contiguous_graph_operands():
    c = X.CASES["edge_split_even"]
    assert np.abs(c["cand"]).max() > 2 ** 31                       # int32 cannot hold these labels:
    c = dict(c, cand=np.unique(c["cand"], return_inverse=True)[1] * 7 - 9)   # the same candidates, small labels
    bg = _graph(c)
    assert int(bg.abs().max()) < 2 ** 31 and int(bg.min()) < 0
    wide = torch.full((2, 2 * bg.shape[1] + 1), -1, dtype=torch.int64, device=DEV)
    wide[:, 1::2] = bg
    view = wide[:, 1::2]
    assert not view.is_contiguous() and not view[0].is_contiguous()
    for use_primary in MODES:
        _check(c, use_primary, _run(c, use_primary, bg.to(torch.int32)), " (int32 graph)")
        _check(c, use_primary, _run(c, use_primary, view), " (strided graph)")
        _check(c, use_primary, _run(c, use_primary, bg.t().contiguous().t()), " (transposed storage)")
