"""CPU: the public surface of the embedding stage (no GPU needed): exports, the C ABI additions, the loud refusal
of CPU tensors, the frnn drop-in and the Embedding-IN mirror's parameters against the reference config."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import conftest

REF_IN_YAML = {  # GNNEmbedding/Configs/IN.yaml, model keys
    "model": "Embedding-IN", "spatial_channels": 3, "latent": 128, "hidden": "ratio", "hidden_ratio": 2,
    "emb_dim": 8, "n_interaction_graph_iters": 12, "nb_node_layer": 3, "nb_edge_layer": 2, "output_layers": 3,
    "hidden_output_activation": "GELU", "hidden_activation": "GELU", "layernorm": True, "share_weight": False,
    "train_r": 1.0, "knn": 100, "true_edges": "modulewise_true_edges"}


def test_exports():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import embedding, models
    for name in ("frnn_graph", "graph_intersection", "training_samples", "training_weights", "hinge_distance"):
        assert getattr(H, name) is getattr(embedding, name)
    assert callable(models.Embedding_InteractionGNN)


def test_header_constants_and_entry_points():
    from hierarchicalgnn_amd import _lib
    txt = open(os.path.join(conftest.ROOT, "include", "hgnn_hip.h")).read()
    assert int(re.search(r"#define\s+HGNN_ABI_VERSION\s+(\d+)", txt).group(1)) == _lib.ABI_VERSION == 26
    dts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+HGNN_DT_(\w+)\s+(\d+)", txt)}
    assert all(getattr(_lib, "DT_" + k) == v for k, v in dts.items()) and dts["F64"] == 4
    for name in ("hgnn_graph_intersection", "hgnn_graph_intersection_workspace_bytes"):
        assert name in _lib.declared_symbols() and name + "(" in txt


def test_workspace_queries_are_host_side():
    from hierarchicalgnn_amd import _lib
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    # (the intersection's size query asks rocPRIM, which needs a device: only its argument check runs here)
    assert lib.hgnn_graph_intersection_workspace_bytes(-1, 0, 0, ctypes.byref(nb)) != 0
    # kNN: K up to 128 (the split workspace for few queries), K = 129 refused
    _lib.check(lib.hgnn_knn_workspace_bytes(100, 5000, 100, ctypes.byref(nb)))
    assert nb.value > 0
    _lib.check(lib.hgnn_knn_workspace_bytes(120_000, 120_000, 100, ctypes.byref(nb)))
    assert nb.value == 0
    assert lib.hgnn_knn_workspace_bytes(100, 5000, 129, ctypes.byref(nb)) != 0
    assert lib.hgnn_knn_radius_f32(None, 10, None, 10, 8, 129, ctypes.c_float(1.0), None, None, None) != 0
    assert b"[1, 128]" in lib.hgnn_last_error()


def test_cpu_tensors_are_refused_loudly():
    import hierarchicalgnn_amd as H
    g = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(RuntimeError, match="HIP device"):
        H.graph_intersection(g, g)
    with pytest.raises(RuntimeError, match="HIP device"):
        H.frnn_graph(torch.randn(10, 8), 1.0, 50)


def test_frnn_shim_is_importable_the_way_utils_imports_it():
    code = ("import frnn\nfrom frnn import frnn_grid_points\nimport torch\n"
            "import hierarchicalgnn_amd.ops\n"
            "try:\n    frnn.frnn_grid_points(torch.zeros(2, 5, 8), torch.zeros(2, 5, 8), K=3, r=1.0)\n"
            "except NotImplementedError as e:\n    assert 'batch size 1' in str(e)\n"
            "else:\n    raise SystemExit('batch size 2 accepted')\n"
            "print('ok')")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(conftest.ROOT, "frnn_shim"), conftest.ROOT]))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def _n_params(m):
    return sum(p.numel() for p in m.parameters())


def test_embedding_in_mirror_matches_the_reference_layout():
    """a raw IN.yaml builds (hidden: ratio); the state_dict keys are the reference's ignn_block.* names"""
    from hierarchicalgnn_amd import models
    m = models.Embedding_InteractionGNN(dict(REF_IN_YAML))
    keys = list(m.state_dict())
    assert all(k.startswith("ignn_block.") for k in keys)
    for must in ("ignn_block.node_encoder.0.weight", "ignn_block.edge_encoder.0.weight",
                 "ignn_block.ignn_cells.11.node_network.0.weight", "ignn_block.output_layer.6.weight"):
        assert must in keys, must
    assert m.ignn_block.output_layer[-1].out_features == 8
    assert "ignn_block.ignn_cells.12.node_network.0.weight" not in keys
    m2 = models.Embedding_InteractionGNN(dict(REF_IN_YAML))
    m2.load_state_dict(m.state_dict(), strict=True)
    assert _n_params(m) == _n_params(m2) > 0
