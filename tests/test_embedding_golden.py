"""CPU: the restatement of the embedding stage's pair construction (tests/embedding_ref.py) against the
reference's own outputs pinned in tests/golden/embedding_samples.npz (tests/golden/make_embedding_golden.py), and
the Embedding-IN mirror's layout against the reference model built from its shipped IN.yaml."""
import json
import os

import numpy as np
import pytest

import embedding_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "embedding_samples.npz")
Z = np.load(GOLDEN, allow_pickle=False)
GI_CASES = [str(c) for c in Z["gi/cases"]]
MODES = ("modulewise_true_edges", "pid_true_edges")


@pytest.mark.parametrize("name", GI_CASES)
def test_intersection_restatement_matches_reference(name):
    pred, truth = Z[f"gi/{name}/pred"], Z[f"gi/{name}/truth"]
    g, y = R.graph_intersection(pred, truth)
    if int(Z[f"gi/{name}/status"]) != 0:
        # the reference raises on .max() of an empty truth graph; here: every y false
        assert truth.shape[1] == 0 and not y.any() and g.shape[1] == np.unique(R._keys(pred)).size
        return
    assert np.array_equal(g, Z[f"gi/{name}/graph"]) and np.array_equal(y, Z[f"gi/{name}/y"])
    for dt in ("float32", "float64"):
        _, _, w = R.graph_intersection(pred, truth, Z[f"gi/{name}/w_{dt}"])
        ref = Z[f"gi/{name}/new_w_{dt}"]
        assert w.dtype == ref.dtype and np.array_equal(w, ref), dt


@pytest.mark.parametrize("mode", MODES)
def test_training_samples_restatement_matches_reference(mode):
    g, y = R.training_samples(Z["ev/pred"], Z["ev/modulewise_true_edges"], Z["ev/signal_mask"], Z["ev/pid"], mode)
    assert np.array_equal(g, Z[f"ts/{mode}/graph"]) and np.array_equal(y, Z[f"ts/{mode}/y"])


def test_fixture_covers_the_contract():
    small = Z["gi/small/pred"], Z["gi/small/truth"]
    assert "empty_truth" in GI_CASES and int(Z["gi/empty_truth/status"]) == 1
    k = R._keys(small[0])
    assert np.unique(k).size < k.size and np.unique(R._keys(small[1])).size < small[1].shape[1]   # duplicates
    assert (small[0][0] == small[0][1]).any()                                                      # self loops
    assert not np.isin(R._keys(small[1]), k).all()                                                 # truth-only pairs
    assert (Z["ev/pid"] == 0).any() and (~Z["ev/signal_mask"]).any() and np.isnan(Z["ev/pt"]).any()
    # embedding_base.py:131 parses as ((signal & ...) | y) == 0: the pid mode keeps no true pair
    assert Z["ts/modulewise_true_edges/y"].any() and not Z["ts/pid_true_edges/y"].any()
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_mirror_matches_reference_in_yaml():
    import torch
    from hierarchicalgnn_amd import models
    raw = json.loads(str(Z["model/in_yaml"]))
    assert raw["model"] == "Embedding-IN" and raw["knn"] == 100 and raw["hidden"] == "ratio"
    m = models.Embedding_InteractionGNN(raw)      # the raw YAML dict: process_hparams resolves hidden: ratio
    assert sorted(m.state_dict()) == sorted(str(k) for k in Z["model/in_yaml_keys"])
    assert sum(p.numel() for p in m.parameters()) == int(Z["model/in_yaml_n_params"])
    sd = {k[len("model/sd/"):]: torch.from_numpy(Z[k]) for k in Z.files if k.startswith("model/sd/")}
    small = models.Embedding_InteractionGNN(dict(raw, latent=32, n_interaction_graph_iters=2))
    small.load_state_dict(sd, strict=True)
