"""The model mirrors with the make_mlp arguments a config sweep changes first -- ``hidden_activation: SiLU``,
``hidden_output_activation: ELU``, ``layernorm: False`` -- stay on the project's kernels: under
``fused.options(strict=True)`` the no-grad forward does not raise (it raised before these activation codes existed),
no MLP is counted in ``library_calls``, and scores and gradients agree with the same model on the ATen path
(``fused.options(enabled=False)`` / ``set_enabled(False)``) within the project's 1e-4 bar, normwise and element-wise.
Shipped hparams (tests/golden/ref_configs.json) at latent 32, a synthetic event of about 2k hits."""
import json
import os

import pytest
import torch

import conftest
from conftest import elem_err, rel_err

pytestmark = pytest.mark.gpu
BAR = 1e-4
ACTS = dict(hidden_activation="SiLU", hidden_output_activation="ELU")


def _raw(name, **over):
    with open(os.path.join(conftest.GOLDEN, "ref_configs.json")) as f:
        return dict(json.load(f)[name]["raw"], **over)


def _close(tag, a, b):
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    r, e = rel_err(a, b), elem_err(a, b)
    print(f"RATIO {tag} rel {r:.3g} elem {e:.3g}")
    assert r <= BAR and e <= BAR, (tag, r, e)


@pytest.fixture
def plain_default():
    """process default on: the backward and the recompute of a checkpoint run on autograd's thread"""
    from hierarchicalgnn_amd import fused
    old = fused._plain_layers
    fused.set_plain_layers(True)
    yield fused
    fused.set_plain_layers(old)


def _ec(**over):
    from hierarchicalgnn_amd import synth
    from hierarchicalgnn_amd.models import EC_InteractionGNN
    torch.manual_seed(0)
    model = EC_InteractionGNN(_raw("EC-IN", latent=32, fp32_gemm="exact", **over)).cuda().eval()
    x, ei = synth.trackml_event(2000, 12000, seed=5)
    return model, x.cuda(), ei.cuda()


def _strict_forward(fused, forward, **opts):
    lib0 = fused.stats["library_calls"]
    with torch.no_grad(), fused.options(strict=True, **opts):
        on = forward()
    assert fused.stats["library_calls"] == lib0
    with torch.no_grad(), fused.options(enabled=False, train_enabled=False):
        off = forward()
    assert fused.stats["library_calls"] > lib0
    assert bool(torch.isfinite(on).all())
    return on, off


def test_ec_in_silu_elu_forward_stays_on_the_kernels():
    from hierarchicalgnn_amd import fused
    model, x, ei = _ec(**ACTS)
    on, off = _strict_forward(fused, lambda: model(x, ei))
    _close("EC-IN SiLU/ELU scores", on, off)


def test_ec_in_plain_forward_needs_the_option(plain_default):
    fused = plain_default
    model, x, ei = _ec(layernorm=False, **ACTS)
    p0 = fused.stats["plain_calls"]
    on, off = _strict_forward(fused, lambda: model(x, ei))
    assert fused.stats["plain_calls"] > p0
    _close("EC-IN plain scores", on, off)
    with pytest.raises(RuntimeError, match="strict"), torch.no_grad(), fused.options(strict=True, plain_layers=False):
        model(x, ei)


def _bc_forward(hidden=False, **over):
    from hierarchicalgnn_amd import synth
    from hierarchicalgnn_amd.models import BC_MessagePassing
    torch.manual_seed(0)
    model = BC_MessagePassing(_raw("BC-HGNN-GMM", latent=32, emb_dim=8, fp32_gemm="exact", **over)).cuda().eval()
    x, ei = synth.trackml_event(2000, 12000, seed=5)
    x, ei = x.cuda(), ei.cuda()
    bg, bw = synth.bipartite_assignment(2000, 40, 5, seed=2)
    sg, sw = synth.super_graph(40, 10, seed=2)
    means = torch.nn.functional.normalize(torch.randn(40, 8)).cuda()

    def forward():
        directed, emb, nodes, edges, _ = model.embed(x, ei)
        n_out, sn_out, _, _ = model.hgnn_block(nodes, edges, directed, means, bg.cuda(), bw.cuda(), sg.cuda(), sw.cuda())
        # ``hidden``: the node rows the score head reads (the scores of an untrained model can saturate)
        return n_out if hidden else model.score(n_out, sn_out, bg.cuda())
    return forward


def test_bc_silu_elu_forward_stays_on_the_kernels():
    from hierarchicalgnn_amd import fused
    on, off = _strict_forward(fused, _bc_forward(**ACTS))
    _close("BC SiLU/ELU scores", on, off)
    _close("BC SiLU/ELU node rows", *_strict_forward(fused, _bc_forward(hidden=True, **ACTS)))


def test_bc_plain_forward(plain_default):
    fused = plain_default
    p0 = fused.stats["plain_calls"]
    on, off = _strict_forward(fused, _bc_forward(layernorm=False, **ACTS))
    assert fused.stats["plain_calls"] > p0
    _close("BC plain scores", on, off)
    _close("BC plain node rows", *_strict_forward(fused, _bc_forward(hidden=True, layernorm=False, **ACTS)))


def _train_step(model, x, ei):
    model.zero_grad(set_to_none=True)
    scores = model(x, ei)
    w = torch.randn(scores.shape, generator=torch.Generator().manual_seed(1)).cuda()
    (scores * w).sum().backward()
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("layernorm", [True, False], ids=["layernorm", "plain"])
def test_ec_in_training_step_gradients(layernorm, plain_default):
    fused = plain_default
    model, x, ei = _ec(layernorm=layernorm, **ACTS)
    model.train()
    lib0, t0 = fused.stats["library_calls"], fused.stats["fused_train_calls"]
    g_on = _train_step(model, x, ei)
    assert fused.stats["library_calls"] == lib0 and fused.stats["fused_train_calls"] > t0
    old = (fused._enabled, fused._train_enabled)
    fused.set_enabled(False)
    try:
        g_off = _train_step(model, x, ei)
    finally:
        fused.set_enabled(*old)
    assert g_on.keys() == g_off.keys() and len(g_on) > 10
    worst, worst_e, bad = 0.0, 0.0, []
    for n in g_on:
        a, b = g_on[n].double().cpu().numpy(), g_off[n].double().cpu().numpy()
        r, e = rel_err(a, b), elem_err(a, b)
        worst, worst_e = max(worst, r), max(worst_e, e)
        if not (r <= BAR and e <= BAR):
            bad.append((n, r, e))
    print(f"RATIO EC-IN train layernorm={layernorm} worst parameter gradient rel {worst:.3g} elem {worst_e:.3g}")
    assert not bad, bad
