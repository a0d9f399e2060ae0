"""GPU: the embedding stage's pair construction (hierarchicalgnn_amd.embedding; csrc/intersect.hip and the large-K
kNN) against the numpy restatement (tests/embedding_ref.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest
import embedding_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

HP = dict(train_r=1.0, knn=100, weight_leak=1.0, weight_min=0.5, pt_interval=0.5, ptcut=1.0, log_weight_ratio=0.0)


def _random_graph(rng, n_nodes, n_pairs, dup=0.3):
    g = rng.integers(0, n_nodes, (2, n_pairs))
    d = rng.integers(0, n_pairs, int(dup * n_pairs))
    g = np.concatenate([g, g[:, d]], 1)
    return g[:, rng.permutation(g.shape[1])]


def _check_intersection(pred, truth, w=None):
    import hierarchicalgnn_amd as H
    p, t = torch.from_numpy(pred).to(DEV), torch.from_numpy(truth).to(DEV)
    if w is None:
        g, y = H.graph_intersection(p, t)
        rg, ry = R.graph_intersection(pred, truth)
    else:
        g, y, nw = H.graph_intersection(p, t, using_weights=True, weights_bidir=torch.from_numpy(w).to(DEV))
        rg, ry, rw = R.graph_intersection(pred, truth, w)
        assert nw.dtype == torch.from_numpy(w).dtype
        assert np.array_equal(nw.cpu().numpy(), rw)
    assert g.dtype == torch.int64 and y.dtype == torch.bool and g.device == p.device
    assert np.array_equal(g.cpu().numpy(), rg) and np.array_equal(y.cpu().numpy(), ry)
    return g, y


def test_intersection_small_cases():
    # duplicates in both, self loops, pairs only in truth, c1 > c2 and c1 < c2
    pred = np.array([[0, 0, 1, 2, 2, 2, 3, 5, 5], [1, 1, 0, 2, 2, 3, 3, 4, 4]])
    truth = np.array([[0, 2, 2, 2, 3, 7, 5], [1, 2, 3, 3, 3, 7, 9]])
    w = np.array([0.5, 1.25, 2.0, 3.0, 0.75, 9.0, 4.0], np.float32)
    g, y = _check_intersection(pred, truth)
    assert g.cpu().tolist() == [[0, 1, 2, 2, 3, 5], [1, 0, 2, 3, 3, 4]]
    assert y.cpu().tolist() == [True, False, True, True, True, False]
    _check_intersection(pred, truth, w)
    _check_intersection(pred, truth, w.astype(np.float64))


@pytest.mark.parametrize("n_pred,n_truth,n_nodes", [(1000, 300, 50), (200_000, 30_000, 120_000),
                                                     (2_000_000, 300_000, 120_000)])
def test_intersection_random_vs_restatement(n_pred, n_truth, n_nodes):
    rng = np.random.default_rng(n_pred)
    pred = _random_graph(rng, n_nodes, n_pred)
    truth = np.concatenate([pred[:, rng.integers(0, pred.shape[1], n_truth // 2)],
                            _random_graph(rng, n_nodes, n_truth // 2, dup=0.2)], 1)
    _check_intersection(pred, truth)
    w = rng.random(truth.shape[1]).astype(np.float32)
    _check_intersection(pred, truth, w)
    _check_intersection(pred, truth, w.astype(np.float64) * 3.1)


def test_intersection_int32_empty_and_bad_ids():
    import hierarchicalgnn_amd as H
    pred = torch.tensor([[3, 1, 3], [4, 2, 4]], dtype=torch.int32, device=DEV)
    truth = torch.tensor([[1], [2]], dtype=torch.int32, device=DEV)
    g, y = H.graph_intersection(pred, truth)
    assert g.cpu().tolist() == [[1, 3], [2, 4]] and y.cpu().tolist() == [True, False]
    empty = torch.zeros((2, 0), dtype=torch.int64, device=DEV)
    g, y = H.graph_intersection(pred, empty)                      # empty truth: all false
    assert g.cpu().tolist() == [[1, 3], [2, 4]] and y.cpu().tolist() == [False, False]
    g, y, w = H.graph_intersection(empty, truth, True, torch.ones(1, device=DEV))   # empty pred: empty graph
    assert g.shape == (2, 0) and y.shape == (0,) and w.shape == (0,)
    with pytest.raises(ValueError, match="negative"):
        H.graph_intersection(torch.tensor([[0, -1], [1, 1]], device=DEV), truth)
    with pytest.raises(ValueError, match="negative"):
        H.graph_intersection(pred, torch.tensor([[1 << 31], [0]], device=DEV))


def test_intersection_is_repeatable():
    import hierarchicalgnn_amd as H
    rng = np.random.default_rng(7)
    pred = torch.from_numpy(_random_graph(rng, 5000, 300_000)).to(DEV)
    truth = torch.from_numpy(_random_graph(rng, 5000, 100_000, dup=0.5)).to(DEV)
    w = torch.rand(truth.shape[1], device=DEV)
    a = H.graph_intersection(pred, truth, True, w)
    b = H.graph_intersection(pred, truth, True, w)
    assert all(torch.equal(x, z) for x, z in zip(a, b))


def test_frnn_graph_layout():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import synth
    from hierarchicalgnn_amd.ops import knn_radius
    emb = synth.embedding_event(5000)["embeddings"].to(DEV)
    g = H.frnn_graph(emb, 1.0, 100)
    idx = knn_radius(emb, emb, 100, 1.0).cpu()
    pos = idx >= 0
    ind = torch.arange(idx.shape[0]).unsqueeze(1).expand(idx.shape)
    assert g.dtype == torch.int64 and torch.equal(g.cpu(), torch.stack([ind[pos], idx[pos]]))
    assert bool((g[0, 1:] >= g[0, :-1]).all())
    assert bool((g[0] == g[1]).sum() == emb.shape[0])             # self pairs included


@pytest.mark.parametrize("mode", ["modulewise_true_edges", "pid_true_edges"])
def test_training_samples_vs_restatement(mode):
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import synth
    ev = synth.embedding_event(20_000, seed=5)
    batch = {k: v.to(DEV) for k, v in ev.items()}
    emb = batch["embeddings"]
    hp = dict(HP, true_edges=mode)
    g, y = H.training_samples(emb, batch, hp)
    pred = H.frnn_graph(emb, 1.0, 100).cpu().numpy()
    rg, ry = R.training_samples(pred, ev["modulewise_true_edges"].numpy(), ev["signal_mask"].numpy(),
                                ev["pid"].numpy(), mode)
    assert np.array_equal(g.cpu().numpy(), rg) and np.array_equal(y.cpu().numpy(), ry)
    if mode == "modulewise_true_edges":
        assert bool(y.any()) and bool((~y).any())
    else:
        # embedding_base.py:131 keeps ((all | y) == 0): only non-signal fakes survive, y is all false there
        assert g.shape[1] > 0 and not bool(y.any())
    # weights, distances and the loss against the same torch expressions on the CPU
    pt = batch["pt"].clone()
    w = H.training_weights(batch, g, y, hp)
    assert torch.equal(batch["pt"], pt)                            # batch.pt is not written
    hinge, dist = H.hinge_distance(emb, g, y)
    loss = torch.nn.functional.hinge_embedding_loss(dist, hinge, margin=1.0, reduction="none").square()
    loss = torch.dot(loss, w)
    cpu = {k: v for k, v in ev.items()}
    w_c = H.training_weights(cpu, g.cpu(), y.cpu(), hp)
    h_c, d_c = H.hinge_distance(ev["embeddings"], g.cpu(), y.cpu())
    l_c = torch.dot(torch.nn.functional.hinge_embedding_loss(d_c, h_c, margin=1.0, reduction="none").square(), w_c)
    assert torch.equal(hinge.cpu(), h_c)
    assert conftest.rel_err(w.cpu(), w_c) <= 1e-6 and conftest.rel_err(dist.cpu(), d_c) <= 1e-6
    assert abs(float(loss) - float(l_c)) <= 1e-6 * max(abs(float(l_c)), 1.0)


@pytest.mark.both_fp32_gemms(must_run=False)
def test_embedding_in_forward_and_step(fp32_gemm):
    """Embedding_InteractionGNN: unit embeddings, and one training step's loss on the pair construction"""
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import models, synth
    hp = dict(spatial_channels=3, latent=32, hidden="ratio", hidden_ratio=2, emb_dim=8, n_interaction_graph_iters=2,
              nb_node_layer=3, nb_edge_layer=2, output_layers=3, hidden_output_activation="GELU",
              hidden_activation="GELU", layernorm=True, share_weight=False, true_edges="modulewise_true_edges",
              **HP)
    torch.manual_seed(0)
    model = models.Embedding_InteractionGNN(hp).to(DEV)
    x, ei = synth.trackml_event(3000, 12_000, seed=3)
    ev = synth.embedding_event(3000, seed=3)
    batch = {k: v.to(DEV) for k, v in ev.items()}
    emb = model(x.to(DEV), ei.to(DEV))
    assert emb.shape == (3000, 8)
    assert float((emb.norm(dim=1) - 1).abs().max()) < 1e-5
    g, y = H.training_samples(emb, batch, hp)
    w = H.training_weights(batch, g, y, hp)
    hinge, dist = H.hinge_distance(emb, g, y)
    loss = torch.dot(torch.nn.functional.hinge_embedding_loss(dist, hinge, margin=1.0, reduction="none").square(), w)
    loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(gr).all() for gr in grads)


def test_frnn_shim_runs_on_the_gpu():
    code = ("import torch, frnn; from hierarchicalgnn_amd.ops import knn_radius; "
            "p = torch.nn.functional.normalize(torch.randn(1, 500, 8, device='cuda'), dim=2); "
            "d, i, a, b = frnn.frnn_grid_points(p, p, None, None, K=100, r=1.0); "
            "i2, d2 = knn_radius(p[0], p[0], 100, 1.0, return_dist2=True); "
            "assert a is None and b is None and i.shape == (1, 500, 100); "
            "assert torch.equal(i[0], i2) and torch.equal(d[0], d2); print('ok')")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(conftest.ROOT, "frnn_shim"), conftest.ROOT]))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# ---------------------------------------------------------------------------------------------------------------
# against the reference's own outputs (tests/golden/embedding_samples.npz)
# ---------------------------------------------------------------------------------------------------------------
from test_embedding_golden import GI_CASES, MODES, Z  # noqa: E402


def _batch():
    return {k: torch.from_numpy(Z[f"ev/{k}"]).to(DEV) for k in ("pid", "pt", "signal_mask", "modulewise_true_edges")}


@pytest.mark.parametrize("name", GI_CASES)
def test_intersection_matches_reference_fixture(name):
    import hierarchicalgnn_amd as H
    pred, truth = (torch.from_numpy(Z[f"gi/{name}/{k}"]).to(DEV) for k in ("pred", "truth"))
    g, y = H.graph_intersection(pred, truth)
    if int(Z[f"gi/{name}/status"]) != 0:                          # empty truth (the reference raises)
        assert not bool(y.any()) and g.shape[1] == torch.unique(pred[0] * (1 << 31) + pred[1]).numel()
        return
    assert np.array_equal(g.cpu().numpy(), Z[f"gi/{name}/graph"]) and np.array_equal(y.cpu().numpy(), Z[f"gi/{name}/y"])
    for dt in ("float32", "float64"):
        w = torch.from_numpy(Z[f"gi/{name}/w_{dt}"]).to(DEV)
        g2, y2, nw = H.graph_intersection(pred, truth, using_weights=True, weights_bidir=w)
        assert torch.equal(g2, g) and torch.equal(y2, y)
        assert np.array_equal(nw.cpu().numpy(), Z[f"gi/{name}/new_w_{dt}"]), dt


@pytest.mark.parametrize("mode", MODES)
def test_training_samples_match_reference_fixture(mode):
    import hierarchicalgnn_amd as H
    batch = _batch()
    emb = torch.from_numpy(Z["ev/embeddings"]).to(DEV)
    hp = dict(HP, true_edges=mode)
    g, y = H.training_samples(emb, batch, hp, prediction_graph=torch.from_numpy(Z["ev/pred"]).to(DEV))
    assert np.array_equal(g.cpu().numpy(), Z[f"ts/{mode}/graph"]) and np.array_equal(y.cpu().numpy(), Z[f"ts/{mode}/y"])
    pt = batch["pt"].clone()
    w = H.training_weights(batch, g, y, hp)
    assert torch.equal(batch["pt"].isnan(), pt.isnan()) and torch.equal(batch["pt"].nan_to_num(), pt.nan_to_num())
    hinge, dist = H.hinge_distance(emb, g, y)
    loss = torch.dot(torch.nn.functional.hinge_embedding_loss(dist, hinge, margin=1.0, reduction="none").square(), w)
    assert np.array_equal(hinge.cpu().numpy(), Z[f"ts/{mode}/hinge"])
    for got, key in ((w, "weights"), (dist, "dist"), (loss, "loss")):
        ref = Z[f"ts/{mode}/{key}"]
        assert conftest.rel_err(got.detach().cpu().numpy(), ref) <= 1e-6, key


@pytest.mark.both_fp32_gemms(must_run=False)
def test_embedding_in_matches_reference_fixture(fp32_gemm):
    """Embedding_InteractionGNN (latent 32, 2 iterations) with the reference's weights: forward, and one training
    step's loss and parameter gradients on the reference's pair construction, within the 1e-4 bar"""
    import json
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import models
    raw = json.loads(str(Z["model/in_yaml"]))
    r = float(Z["model/train_r"])
    hp = dict(raw, latent=32, n_interaction_graph_iters=2, **dict(HP, train_r=r), true_edges="modulewise_true_edges")
    model = models.Embedding_InteractionGNN(hp)
    sd = {k[len("model/sd/"):]: torch.from_numpy(Z[k]) for k in Z.files if k.startswith("model/sd/")}
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    x = torch.from_numpy(Z["model/x"]).to(DEV)
    emb = model(x, torch.from_numpy(Z["model/graph"]).to(DEV))
    conftest.assert_parity(emb, Z["model/embeddings"], what="embeddings")
    batch = _batch()
    g, y = H.training_samples(emb, batch, hp, prediction_graph=torch.from_numpy(Z["model/pred"]).to(DEV))
    w = H.training_weights(batch, g, y, hp)
    hinge, dist = H.hinge_distance(emb, g, y)
    loss = torch.dot(torch.nn.functional.hinge_embedding_loss(dist, hinge, margin=r, reduction="none").square(), w)
    loss.backward()
    conftest.assert_parity(loss.detach().reshape(1), Z["model/loss"].reshape(1), what="loss")
    grads = {k[len("model/grad/"):]: Z[k] for k in Z.files if k.startswith("model/grad/")}
    for k, p in model.named_parameters():
        if k in grads:
            conftest.assert_parity(p.grad, grads[k], what=k)
        else:
            assert p.grad is None or not bool(p.grad.any()), k
