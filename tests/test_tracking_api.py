"""CPU: the public surface of the tracking metrics (no GPU needed): exports, the C ABI result layout, the
tracking_utils drop-in, and the loud refusal of CPU tensors."""
import os
import re
import subprocess
import sys

import pytest
import torch

import conftest


def test_exports_and_default_response():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import tracking
    assert H.eval_metrics is tracking.eval_metrics
    assert callable(H.edge_track_candidates) and callable(H.bipartite_track_candidates)
    assert tracking.default_response == {"track_eff": 0, "track_pur": 0, "hit_eff": 0, "hit_pur": 0}


def test_result_indices_match_the_header():
    from hierarchicalgnn_amd import _lib
    txt = open(os.path.join(conftest.ROOT, "include", "hgnn_hip.h")).read()
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+HGNN_TE_(\w+)\s+(\d+)", txt)}
    assert found and all(getattr(_lib, "TE_" + k) == v for k, v in found.items())
    assert _lib.TE_RESULT == found["RESULT"] == 12


def test_cpu_tensors_are_refused_loudly():
    import hierarchicalgnn_amd as H
    ev = {"pid": torch.tensor([1, 1, 1]), "pt": torch.ones(3)}
    with pytest.raises(RuntimeError, match="HIP device"):
        H.eval_metrics(torch.tensor([[0, 1, 2], [0, 0, 0]]), ev, primary=False)


def test_shim_is_importable_the_way_the_bases_import_it():
    code = ("from tracking_utils import eval_metrics, default_response; "
            "import hierarchicalgnn_amd.tracking as t; assert eval_metrics is t.eval_metrics; print('ok')")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(conftest.ROOT, "tracking_utils_shim"),
                                                        conftest.ROOT]))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
