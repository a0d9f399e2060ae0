"""CPU: the float64 restatement of the pT-weighted BCE (tests/wbce_ref.py) against the reference's own
EdgeClassifierBase.training_step pinned in tests/golden/ec_loss.npz, and against float64 autograd of the formula."""
import numpy as np
import pytest
import torch

import conftest
import wbce_ref as WR

Z = conftest.load_golden("ec_loss.npz")
MODES = [str(m) for m in Z["modes"]]
LWRS = [float(v) for v in Z["log_weight_ratios"]]


def fixture_hparams(mode, lwr):
    hp = {str(k): float(v) for k, v in zip(Z["hparam_keys"], Z["hparams"])}
    return dict(hp, true_edges=mode, log_weight_ratio=lwr)


def fixture_case(mode):
    """(y, keep) of a true_edges mode, as training_step (:116-123) selects them"""
    y, y_pid = Z["ev/y"], Z["ev/y_pid"]
    if mode == "modulewise_true_edges":
        return y, (y_pid == 0) | (y == 1)
    return y_pid, np.ones(y.shape, bool)


@pytest.mark.parametrize("lwr", LWRS)
@pytest.mark.parametrize("mode", MODES)
def test_restatement_matches_reference_fixture(mode, lwr):
    y, keep = fixture_case(mode)
    key = f"{mode}/lwr{lwr:g}"
    loss, grad, w, _ = WR.weighted_bce(Z["ev/scores"], Z["ev/edge_index"], y, Z["ev/pt"], fixture_hparams(mode, lwr),
                                       keep=keep)
    assert not keep.all() or mode == "pid_true_edges"          # the modulewise mode drops edges
    assert conftest.rel_err(w[keep], Z[f"{key}/weights"]) <= 1e-6
    assert conftest.rel_err(np.array([loss]), Z[f"{key}/loss"].reshape(1)) <= 1e-6
    assert not w[~keep].any() and not grad[~keep].any()
    conftest.assert_parity(grad, Z[f"{key}/grad"], what="dloss/dscores")


def _torch_loss(s, graph, y, pt_a, pt_b, hp, combine, keep):
    """the reference formula with float64 torch tensors, differentiable in s: the weights as the restatement's own
    class-normalised raw weights, torch's binary_cross_entropy, the dot product"""
    raw = torch.from_numpy(WR.raw_weights(pt_a, pt_b, graph, hp, combine))
    yt, kt = torch.from_numpy(y), torch.from_numpy(keep)
    w = torch.zeros_like(raw)
    for cls, sign in ((yt & kt, 1.0), (~yt & kt, -1.0)):
        k = torch.sigmoid(torch.tensor(sign * hp["log_weight_ratio"], dtype=torch.float64))
        w[cls] = raw[cls] / raw[cls].sum() * k
    return torch.dot(torch.nn.functional.binary_cross_entropy(s, yt.double(), reduction="none"), w)


@pytest.mark.parametrize("combine,lwr,with_keep", [("sum", 0.0, False), ("sum", 0.8, True), ("max", -0.5, True)])
def test_restatement_equals_float64_autograd(combine, lwr, with_keep):
    rng = np.random.default_rng(5)
    na, nb, p = 300, 170, 4000
    graph = np.stack([rng.integers(0, na, p), rng.integers(0, nb, p)])
    y = rng.random(p) < 0.3
    keep = rng.random(p) < 0.8 if with_keep else np.ones(p, bool)
    pt_a = rng.exponential(1.0, na).astype(np.float32)
    pt_b = rng.exponential(1.0, nb).astype(np.float32)
    pt_a[::17] = np.nan
    # scores that float32 holds exactly together with 1 - s: the float32 and the float64 1 - s are then one number
    scores = (rng.integers(1, 4096, p) / 4096.0).astype(np.float32)
    hp = dict(weight_leak=0.1, ptcut=1.0, pt_interval=0.5, weight_min=0.1, log_weight_ratio=lwr)
    loss, grad, _, _ = WR.weighted_bce(scores, graph, y, pt_a, hp, pt_b=pt_b, combine=combine, keep=keep)
    s = torch.from_numpy(scores.astype(np.float64)).requires_grad_(True)
    l_t = _torch_loss(s, graph, y, pt_a, pt_b, hp, combine, keep)
    l_t.backward()
    assert abs(loss - float(l_t.detach())) <= 1e-12 * abs(float(l_t.detach()))
    assert conftest.rel_err(grad, s.grad.numpy()) <= 1e-12


def test_clamps_empty_inputs_and_empty_class():
    hp = dict(weight_leak=0.1, ptcut=1.0, pt_interval=0.5, weight_min=0.1, log_weight_ratio=0.0)
    pt = np.ones(4, np.float32)
    loss, grad, w, sums = WR.weighted_bce(np.zeros(0, np.float32), np.zeros((2, 0), np.int64), np.zeros(0, bool), pt,
                                          hp)
    assert loss == 0.0 and grad.size == 0 and sums == (0.0, 0.0)
    g = np.array([[0, 1, 2, 3], [1, 2, 3, 0]])
    s = np.array([0.0, 1.0, 0.5, 0.25], np.float32)
    loss, grad, w, _ = WR.weighted_bce(s, g, np.zeros(4, bool), pt, hp)            # no true pair
    assert np.isfinite(loss) and np.isfinite(grad).all() and abs(w.sum() - 0.5) < 1e-15
    assert abs(loss - 0.125 * (100.0 - np.log(0.5) - np.log(0.75))) < 1e-12         # log(1 - 1) clamps at -100
    loss, grad, _, _ = WR.weighted_bce(s, g, np.ones(4, bool), pt, hp)
    assert grad[0] == 0.125 * -1.0 / 1e-12                                          # the gradient's clamp
