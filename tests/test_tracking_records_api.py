"""CPU: the public surface of track_records (no GPU needed): the exports, the header / binding / shim names, the
argument checks (they run before anything touches a device) and the loud refusal of CPU tensors."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import conftest

HEADER = os.path.join(conftest.ROOT, "include", "hgnn_hip.h")


def _event(n=3):
    return {"pid": torch.tensor([1] * n), "pt": torch.ones(n), "eta": torch.zeros(n)}


GRAPH = torch.tensor([[0, 1, 2], [0, 0, 0]])


def test_exports():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import tracking
    assert H.track_records is tracking.track_records
    assert [k for k, _ in tracking.PARTICLE_FIELDS] == ["pid", "nhits", "pt", "primary", "reconstructable", "n_match",
                                                        "n_kept", "n_mask", "cand_index", "shared"]
    assert [k for k, _ in tracking.CANDIDATE_FIELDS] == ["label", "size", "n_kept", "n_mask", "particle", "shared"]
    assert len(tracking.BIN_COLUMNS) == 6


def test_header_binding_and_library_expose_the_entry():
    from hierarchicalgnn_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("hgnn_track_records", "hgnn_track_records_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _lib.declared_symbols()
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+HGNN_TR_(\w+)\s+(\d+)", txt)}
    assert found == {"MAX_VARS": _lib.TR_MAX_VARS, "MAX_BINS": _lib.TR_MAX_BINS, "COLUMNS": _lib.TR_COLUMNS}
    # the struct mirrors list the header's members in the header's order
    for struct, mirror in (("hgnn_tr_particles", _lib.HgnnTrParticles), ("hgnn_tr_candidates", _lib.HgnnTrCandidates)):
        body = re.search(r"struct\s+" + struct + r"\s*\{(.*?)\}", txt, flags=re.S).group(1)
        assert re.findall(r"\*\s*(\w+)\s*;", body) == [k for k, _ in mirror._fields_]
        assert ctypes.sizeof(mirror) == 8 * len(mirror._fields_)


def test_host_side_checks_of_the_c_entry():
    """the argument checks return before the library asks for a device (the size itself needs one: rocPRIM's
    temporary-storage query; tests/test_gpu_tracking_records.py checks it)"""
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    assert lib.hgnn_track_records_workspace_bytes(600, 120, 5, ctypes.byref(nb)) == 1      # HGNN_ERR_INVALID_ARG
    assert b"n_vars" in lib.hgnn_last_error()
    assert lib.hgnn_track_records_workspace_bytes(-1, 120, 0, ctypes.byref(nb)) == 1
    assert b"negative" in lib.hgnn_last_error()
    assert lib.hgnn_track_records_workspace_bytes(600, 120, 0, None) == 1
    args = [None, None, 0, None, None, None, 0, None, 0, None, None, 1.0, 5.0, 0.5, None, None, None, None, None, 0,
            None]
    assert lib.hgnn_track_records(*args) == 1 and b"NULL result" in lib.hgnn_last_error()
    args[8] = 5
    assert lib.hgnn_track_records(*args) == 1 and b"n_vars" in lib.hgnn_last_error()


def test_shim_offers_track_records_beside_eval_metrics():
    code = ("from tracking_utils import eval_metrics, track_records, default_response; "
            "import hierarchicalgnn_amd.tracking as t; assert track_records is t.track_records; print('ok')")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(conftest.ROOT, "tracking_utils_shim"),
                                                        conftest.ROOT]))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_cpu_tensors_are_refused_loudly():
    import hierarchicalgnn_amd as H
    with pytest.raises(RuntimeError, match="HIP device"):
        H.track_records(GRAPH, _event(), primary=False)
    with pytest.raises(RuntimeError, match="HIP device"):
        H.track_records(GRAPH, _event(), bins={"eta": ("eta", [0.0, 1.0])}, primary=False)


@pytest.mark.parametrize("edges, what", [
    ([1.0], "2..65 edges"), (list(range(66)), "2..65 edges"), ([0.0, 0.0], "strictly ascending"),
    ([1.0, 0.5], "strictly ascending"), ([0.0, float("inf")], "finite"), ([float("nan"), 1.0], "finite"),
    ([0.0, 1e39], "finite"),                                  # overflows when rounded to float32
    ([1.0, 1.0 + 2.0 ** -30], "strictly ascending"),          # equal once rounded to float32
])
def test_bad_edges_raise(edges, what):
    import hierarchicalgnn_amd as H
    with pytest.raises(ValueError, match="track_records: .*" + what):
        H.track_records(GRAPH, _event(), bins={"eta": ("eta", edges)}, primary=False)


def test_other_argument_errors():
    import hierarchicalgnn_amd as H
    ev = _event()
    five = {f"v{i}": ("eta", [0.0, 1.0]) for i in range(5)}
    with pytest.raises(ValueError, match="track_records: at most 4 binning variables"):
        H.track_records(GRAPH, ev, bins=five, primary=False)
    with pytest.raises(ValueError, match="track_records: .*one entry per hit"):
        H.track_records(GRAPH, ev, bins={"x": (torch.zeros(4), [0.0, 1.0])}, primary=False)
    with pytest.raises(ValueError, match=r"track_records: bins\['x'\] must be \(values, edges\)"):
        H.track_records(GRAPH, ev, bins={"x": torch.zeros(3)}, primary=False)
    with pytest.raises(ValueError, match="tensor or an event field name"):
        H.track_records(GRAPH, ev, bins={"x": ([0.0, 0.0, 0.0], [0.0, 1.0])}, primary=False)
