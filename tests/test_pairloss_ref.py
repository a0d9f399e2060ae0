"""CPU: the float64 restatement of the pair hinge loss (tests/pairloss_ref.py) against the reference's own weights,
distances and losses pinned in tests/golden/embedding_samples.npz, and its gradient against float64 autograd."""
import numpy as np
import pytest
import torch

import conftest
import pairloss_ref as PR
from test_embedding_golden import MODES, Z

HP = dict(train_r=1.0, knn=100, weight_leak=1.0, weight_min=0.5, pt_interval=0.5, ptcut=1.0, log_weight_ratio=0.0)


@pytest.mark.parametrize("mode", MODES)
def test_restatement_matches_reference_fixture(mode):
    g, y = Z[f"ts/{mode}/graph"], Z[f"ts/{mode}/y"]
    loss, _, w, d = PR.pair_hinge(Z["ev/embeddings"], g, y, Z["ev/pt"], HP)
    assert conftest.rel_err(w, Z[f"ts/{mode}/weights"]) <= 1e-6
    assert conftest.rel_err(d, Z[f"ts/{mode}/dist"]) <= 1e-6
    assert conftest.rel_err(np.array([loss]), Z[f"ts/{mode}/loss"].reshape(1)) <= 1e-6


def _torch_loss(e, graph, y, pt, hp, margin, scale):
    """the same formula with float64 torch tensors, differentiable in e"""
    w = torch.from_numpy(PR.weights(pt, graph, y, hp))
    a, b = torch.from_numpy(graph[0]), torch.from_numpy(graph[1])
    d = ((e[a] - e[b]).square().sum(-1) + 1e-12).sqrt()
    hinge = torch.where(torch.from_numpy(y), 1, -1)
    per_pair = torch.nn.functional.hinge_embedding_loss(scale * d, hinge, margin=margin, reduction="none").square()
    return torch.dot(per_pair, w)


@pytest.mark.parametrize("scale,margin,lwr", [(1.0, 1.0, 0.0), (1.0 / 0.7, 1.0, 0.0), (1.0, 0.6, 0.8)])
def test_restatement_gradient_equals_float64_autograd(scale, margin, lwr):
    rng = np.random.default_rng(3)
    n, p, dim = 300, 4000, 8
    emb = rng.normal(size=(n, dim))
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    graph = rng.integers(0, n, (2, p))
    graph[:, :50] = graph[:, 50:100]                 # duplicate pairs
    graph[1, 100:130] = graph[0, 100:130]            # self pairs
    y = rng.random(p) < 0.3
    pt = rng.exponential(1.0, n).astype(np.float32)
    pt[::17] = np.nan
    hp = dict(HP, log_weight_ratio=lwr)
    loss, grad, _, _ = PR.pair_hinge(emb, graph, y, pt, hp, margin=margin, scale=scale)
    e = torch.from_numpy(emb).requires_grad_(True)
    l_t = _torch_loss(e, graph, y, pt, hp, margin, scale)
    l_t.backward()
    assert abs(loss - float(l_t.detach())) <= 1e-12 * abs(float(l_t.detach()))
    assert conftest.rel_err(grad, e.grad.numpy()) <= 1e-12


def test_empty_inputs_and_empty_class():
    emb = np.eye(4, 3)
    pt = np.ones(4, np.float32)
    loss, grad, _, _ = PR.pair_hinge(emb, np.zeros((2, 0), np.int64), np.zeros(0, bool), pt, HP)
    assert loss == 0.0 and not grad.any()
    loss, grad, w, _ = PR.pair_hinge(emb, np.array([[0, 1], [2, 3]]), np.zeros(2, bool), pt, HP)
    assert np.isfinite(loss) and np.isfinite(grad).all() and abs(w.sum() - 0.5) < 1e-15
