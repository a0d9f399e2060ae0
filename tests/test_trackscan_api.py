"""CPU: the public surface of the score-cut scan (no GPU needed): the exports, the header / binding agreement, the
argument checks (they run before anything touches a device) and the loud refusal of CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

import conftest

HEADER = os.path.join(conftest.ROOT, "include", "hgnn_hip.h")
GRAPH = torch.tensor([[0, 1, 2], [1, 2, 0]])
SCORES = torch.tensor([0.9, 0.5, 0.1])
MASK = torch.arange(3)


def _event(n=3):
    return {"pid": torch.tensor([1] * n), "pt": torch.ones(n)}


def _both():
    import hierarchicalgnn_amd as H
    return (("edge_score_scan", H.edge_score_scan), ("bipartite_score_scan", H.bipartite_score_scan))


def test_exports():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import assignment, edge_classifier, tracking
    assert H.edge_score_scan is tracking.edge_score_scan
    assert H.bipartite_score_scan is tracking.bipartite_score_scan
    assert H.ec_score_scan is edge_classifier.ec_score_scan
    assert H.bc_score_scan is assignment.bc_score_scan


def test_header_binding_and_library_agree():
    from hierarchicalgnn_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("hgnn_track_scan", "hgnn_track_scan_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _lib.declared_symbols()
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+HGNN_TS_(\w+)\s+(\d+)", txt)}
    assert found == {"EDGE": _lib.TS_EDGE, "PAIR": _lib.TS_PAIR, "MAX_CUTS": _lib.TS_MAX_CUTS,
                     "N_PASS": _lib.TS_N_PASS, "N_TRUE_PASS": _lib.TS_N_TRUE_PASS, "N_TRUE": _lib.TS_N_TRUE,
                     "ROW": _lib.TS_ROW}
    assert re.search(r"#define\s+HGNN_TS_RESERVED_LABEL\s+INT64_MAX", txt) and _lib.TS_RESERVED_LABEL == 2 ** 63 - 1
    # a row is hgnn_track_eval's result vector followed by the three counts
    assert (_lib.TS_N_PASS, _lib.TS_N_TRUE_PASS, _lib.TS_N_TRUE, _lib.TS_ROW) == tuple(
        _lib.TE_RESULT + k for k in range(4))
    # the binding passes as many arguments as the header declares
    for name in ("hgnn_track_scan", "hgnn_track_scan_workspace_bytes"):
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib._SIGNATURES[name][1]), name


def test_host_side_checks_of_the_c_entry():
    """the argument checks return before the library asks for a device (the size itself needs one: rocPRIM's
    temporary-storage query; tests/test_gpu_trackscan.py checks it)"""
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    size = lib.hgnn_track_scan_workspace_bytes
    assert size(2, 10, 10, 10, 4, ctypes.byref(nb)) == 1 and b"mode" in lib.hgnn_last_error()
    assert size(_lib.TS_EDGE, 10, 10, 10, 0, ctypes.byref(nb)) == 1 and b"n_cuts" in lib.hgnn_last_error()
    assert size(_lib.TS_PAIR, 10, 10, 10, 65, ctypes.byref(nb)) == 1 and b"n_cuts" in lib.hgnn_last_error()
    assert size(_lib.TS_PAIR, -1, 10, 10, 4, ctypes.byref(nb)) == 1 and b"negative" in lib.hgnn_last_error()
    assert size(_lib.TS_EDGE, 10, 1 << 31, 10, 4, ctypes.byref(nb)) == 1 and b"2^31" in lib.hgnn_last_error()
    assert size(_lib.TS_EDGE, 10, 10, 10, 4, None) == 1 and b"NULL bytes" in lib.hgnn_last_error()
    args = [_lib.TS_EDGE, None, None, 0, None, None, 65, None, 0, None, None, None, None, None, 0, 1.0, 5.0, 0.5, None,
            None, 0, None]
    assert lib.hgnn_track_scan(*args) == 1 and b"n_cuts" in lib.hgnn_last_error()
    args[6] = 4
    assert lib.hgnn_track_scan(*args) == 1 and b"NULL result" in lib.hgnn_last_error()


def test_cpu_tensors_are_refused_loudly():
    import hierarchicalgnn_amd as H
    for name, fn in _both():
        with pytest.raises(RuntimeError, match=name + " needs HIP device"):
            fn(GRAPH, SCORES, [0.5], MASK, _event(), primary=False)
    hp = {"true_edges": "pid_true_edges", "ptcut": 1.0, "n_hits": 3, "majority_cut": 0.5}
    batch = {"edge_index": GRAPH, "inverse_mask": MASK, "y": torch.ones(3), "y_pid": torch.ones(3)}
    with pytest.raises(RuntimeError, match="HIP device"):
        H.ec_score_scan(SCORES, batch, _event(), hp, [0.5])
    with pytest.raises(RuntimeError, match="HIP device"):
        H.bc_score_scan(GRAPH, SCORES, batch, _event(), hp, [0.5])
    with pytest.raises(ValueError, match="ec_score_scan: true_edges"):
        H.ec_score_scan(SCORES, batch, _event(), dict(hp, true_edges="all"), [0.5])


@pytest.mark.parametrize("cuts, what", [
    ([], "1..64 cuts"), ([0.5] * 65, "1..64 cuts"), ([0.5, float("nan")], "a cut is NaN"),
    (torch.tensor([float("nan")]), "a cut is NaN"),
])
def test_bad_cuts_raise(cuts, what):
    for name, fn in _both():
        with pytest.raises(ValueError, match=name + ": .*" + what):
            fn(GRAPH, SCORES, cuts, MASK, _event(), primary=False)


def test_length_mismatches_and_other_argument_errors():
    for name, fn in _both():
        with pytest.raises(ValueError, match=name + ": one score per item"):
            fn(GRAPH, SCORES[:2], [0.5], MASK, _event(), primary=False)
        with pytest.raises(ValueError, match=name + r": a \[2, n\] graph"):
            fn(GRAPH.t(), SCORES, [0.5], MASK, _event(), primary=False)
        with pytest.raises(ValueError, match=name + ": truth must be bool or uint8 with one entry per item"):
            fn(GRAPH, SCORES, [0.5], MASK, _event(), primary=False, truth=torch.ones(2, dtype=torch.bool))
        with pytest.raises(ValueError, match=name + ": truth must be bool or uint8"):
            fn(GRAPH, SCORES, [0.5], MASK, _event(), primary=False, truth=torch.ones(3))
        with pytest.raises(ValueError, match=name + ": keep must be bool or uint8 with one entry per item"):
            fn(GRAPH, SCORES, [0.5], MASK, _event(), primary=False, truth=torch.ones(3, dtype=torch.bool),
               keep=torch.ones(4, dtype=torch.uint8))
        with pytest.raises(ValueError, match=name + ": keep needs truth"):
            fn(GRAPH, SCORES, [0.5], MASK, _event(), primary=False, keep=torch.ones(3, dtype=torch.bool))
    import hierarchicalgnn_amd as H
    with pytest.raises(ValueError, match="edge_score_scan: inverse_mask is needed"):
        H.edge_score_scan(GRAPH, SCORES, [0.5], None, _event(), primary=False)
