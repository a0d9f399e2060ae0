"""CPU: the C ABI, binding and package surface of the fused pair hinge loss, and the layout of the
Embedding-HGNN-GMM and gMRT mirrors against the reference models built from their shipped configs
(tests/golden/embedding_hgnn.npz, tests/golden/make_embedding_hgnn_golden.py)."""
import json
import os
import re

import numpy as np
import pytest
import torch

import conftest
from golden import seeded
from hierarchicalgnn_amd import _lib

GOLDEN = os.path.join(conftest.GOLDEN, "embedding_hgnn.npz")
GOLDEN_GMRT = os.path.join(conftest.GOLDEN, "embedding_hgnn_gmrt.npz")


def _load():
    z = {}
    for path in (GOLDEN, GOLDEN_GMRT):
        with np.load(path, allow_pickle=False) as f:
            z.update({k: f[k] for k in f.files})
    return z


Z = _load()
ENTRY_POINTS = ("hgnn_pair_hinge_workspace_bytes", "hgnn_pair_hinge_forward", "hgnn_pair_hinge_backward")


def test_header_declares_the_entry_points_under_abi_26():
    txt = open(os.path.join(conftest.ROOT, "include", "hgnn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    assert int(re.search(r"#define\s+HGNN_ABI_VERSION\s+(\d+)", txt).group(1)) == 26 == _lib.ABI_VERSION
    assert int(re.search(r"#define\s+HGNN_PH_MAX_DIM\s+(\d+)", txt).group(1)) == _lib.PH_MAX_DIM == 16
    for name in ("KT", "KF", "ST", "SF", "LOSS", "STATE", "HPARAMS", "MARGIN", "SCALE", "LOG_WEIGHT_RATIO"):
        assert int(re.search(rf"#define\s+HGNN_PH_{name}\s+(\d+)", txt).group(1)) == getattr(_lib, "PH_" + name)


def test_binding_and_library_have_them():
    assert set(ENTRY_POINTS) <= set(_lib.declared_symbols())
    lib = _lib.load()
    assert lib.hgnn_abi_version() == 26
    import ctypes
    nb = ctypes.c_size_t(0)
    assert lib.hgnn_pair_hinge_workspace_bytes(12_000_000, 120_000, 8, 0, ctypes.byref(nb)) == 0
    fwd = nb.value
    assert 0 < fwd < 1 << 20                                     # per-workgroup partials only: nothing of size P
    assert lib.hgnn_pair_hinge_workspace_bytes(12_000_000, 120_000, 8, 1, ctypes.byref(nb)) == 0
    assert fwd + 4 * 12_000_000 <= nb.value < fwd + 4 * 12_000_000 + 4096     # one float per pair
    assert lib.hgnn_pair_hinge_workspace_bytes(10, 10, 17, 0, ctypes.byref(nb)) != 0
    assert b"D <= 16" in lib.hgnn_last_error()


def test_package_exports():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import models, utils
    for name in ("pair_hinge_loss", "pair_hinge_check", "embedding_hgnn_training_loss", "embedding_in_training_loss"):
        assert callable(getattr(H, name)), name
    assert callable(utils.match_dims) and models.Embedding_HierarchicalGNN_GMM and models.gMRT
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.pair_hinge_loss(torch.zeros(4, 8), torch.zeros(2, 3, dtype=torch.long), torch.zeros(3, dtype=torch.bool),
                          {"pt": torch.zeros(4)}, {})


def test_match_dims_layout():
    from hierarchicalgnn_amd.utils import match_dims
    m = match_dims(3, 32, layer_norm=True, output_activation="GELU")
    assert [type(x).__name__ for x in m] == ["Linear", "LayerNorm", "GELU"]
    m = match_dims(32, 8, layer_norm=True, output_activation=None)
    assert [type(x).__name__ for x in m] == ["Linear", "LayerNorm"]
    assert [type(x).__name__ for x in match_dims(6, 32)] == ["Linear", "GELU"]


def _mirror(tag):
    from hierarchicalgnn_amd import models
    return {"emb": models.Embedding_HierarchicalGNN_GMM, "gmrt": models.gMRT}[tag]


@pytest.mark.parametrize("tag,model_name", [("emb", "Embedding-HGNN-GMM"), ("gmrt", "BC-HGNN-GMM")])
def test_mirror_builds_from_the_raw_shipped_yaml(tag, model_name):
    raw = json.loads(str(Z[f"cfg/{tag}/yaml"]))
    assert raw["model"] == model_name and raw["hidden"] == "ratio"
    if tag == "gmrt":
        assert "data_dir" in raw and "super_dir" in raw         # accepted and ignored
    m = _mirror(tag)(raw)
    assert list(m.state_dict()) == json.loads(str(Z[f"cfg/{tag}/keys"]))
    assert sum(p.numel() for p in m.parameters()) == int(Z[f"cfg/{tag}/n_params"])


@pytest.mark.parametrize("tag", ["emb", "gmrt"])
def test_small_mirror_has_the_reference_state_dict_layout(tag):
    hp = json.loads(str(Z[f"{tag}/hp"]))
    m = _mirror(tag)(hp)
    shapes = json.loads(str(Z[f"{tag}/sd_shapes"]))
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == shapes
    seeded.fill_parameters(m, int(Z[f"{tag}/seed"]))
    seeded.check_parameters(m, Z[f"{tag}/param_checksums"])
    # a state dict with the reference's keys loads strictly
    sd = {k: torch.zeros(s) for k, s in shapes.items()}
    m.load_state_dict(sd, strict=True)


def test_block_switches_leave_the_bc_block_unchanged():
    from hierarchicalgnn_amd import models
    hp = json.loads(str(Z["emb/hp"]))
    bc = models.HierarchicalGNNBlock(hp)
    assert bc.l1_pool and not bc.emb_head and not hasattr(bc, "output_layer")
    emb = models.Embedding_HierarchicalGNN_GMM(hp).hgnn_block
    assert not emb.l1_pool and emb.emb_head and type(emb) is models.HierarchicalGNNBlock
    assert type(models.gMRT(hp).hgnn_block) is models.HierarchicalGNNBlock and not hasattr(models.gMRT(hp), "ignn_block")


def test_fixture_is_small_and_the_cut_is_clear():
    assert os.path.getsize(GOLDEN) < 1 << 20 and os.path.getsize(GOLDEN_GMRT) < 1 << 20
    for tag in ("emb", "gmrt"):
        assert float(Z[f"{tag}/cut_gap"]) > 1e-4
