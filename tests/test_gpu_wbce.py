"""GPU: the fused pT-weighted BCE (hierarchicalgnn_amd.weighted_bce_loss; csrc/wbce.hip), the edge classifier's
training step and the fused tail of the assignment loss against the float64 restatement (tests/wbce_ref.py), the
reference fixtures (tests/golden/ec_loss.npz, assignment_loss.npz) and the torch composition.

Bars.  Loss: 1e-6 relative.  Every term of the loss has one sign, and each carries a handful of float32 roundings
(the two ptw, their sum or max, 1 - s) plus one logf, about 5 * 2^-24 = 3e-7 in all; the float64 sum adds nothing to
that, so the whole stays below about 5e-7.  Gradient: conftest.assert_parity, the project's 1e-4 normwise and
element-wise bar.  Where scores of exactly 0 or 1 are planted, the 1e-12 clamp makes their gradient 1e9 times the
others', which then weigh nothing in either norm: those cases are also held to the bar over the other pairs alone."""
import numpy as np
import pytest
import torch

import conftest
import wbce_ref as WR
from test_wbce_ref import LWRS, MODES, Z, fixture_case, fixture_hparams

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

HP = dict(weight_leak=1.0, weight_min=0.5, pt_interval=0.5, ptcut=1.0, log_weight_ratio=0.7)


def _fused(scores, graph, y, pt_a, hp, pt_b=None, combine="sum", keep=None, **kw):
    """(loss tensor, grad tensor) of one fused call on a fresh leaf"""
    import hierarchicalgnn_amd as H
    s = torch.as_tensor(scores, dtype=torch.float32).to(DEV).requires_grad_(True)
    loss = H.weighted_bce_loss(s, torch.as_tensor(graph).to(DEV), torch.as_tensor(y).to(DEV),
                               torch.as_tensor(pt_a).to(DEV), hp,
                               pt_b=None if pt_b is None else torch.as_tensor(pt_b).to(DEV), combine=combine,
                               keep=None if keep is None else torch.as_tensor(keep).to(DEV), **kw)
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    return loss.detach(), s.grad


def _check(scores, graph, y, pt_a, hp, pt_b=None, combine="sum", keep=None, ordinary=None):
    loss, grad = _fused(scores, graph, y, pt_a, hp, pt_b, combine, keep)
    r_loss, r_grad, _, _ = WR.weighted_bce(scores, graph, y, pt_a, hp, pt_b=pt_b, combine=combine, keep=keep)
    err = abs(float(loss) - r_loss) / max(abs(r_loss), 1e-30)
    g = grad.cpu().numpy()
    print(f"weighted bce: P={len(y)} {combine} keep={keep is not None} loss {float(loss):.9g} ref {r_loss:.9g} "
          f"rel_err {err:.3g} grad normwise {conftest.rel_err(g, r_grad):.3g} "
          f"element-wise {conftest.elem_err(g, r_grad):.3g}")
    assert err <= 1e-6
    conftest.assert_parity(grad, r_grad, what="grad_scores")
    if ordinary is not None:
        conftest.assert_parity(g[ordinary], r_grad[ordinary], what="grad_scores away from the clamp")
    if keep is not None:
        assert not g[~np.asarray(keep, bool)].any()
    return loss, grad


def _random_case(seed, n, p, idt, nb=None):
    """(scores, graph, y, pt_a, pt_b, keep, ordinary): duplicate and self pairs, NaN pt every 13th hit, scores
    sigmoid(4 * normal) with exact 0.0 and 1.0 planted in both classes; ordinary = the pairs that are not planted"""
    rng = np.random.default_rng(seed)
    nb = n if nb is None else nb
    graph = np.stack([rng.integers(0, n, p), rng.integers(0, nb, p)])
    q = p // 20
    graph[:, :q] = graph[:, q:2 * q]                                       # duplicate pairs
    graph[1, 2 * q:3 * q] = np.minimum(graph[0, 2 * q:3 * q], nb - 1)      # self pairs
    y = rng.random(p) < 0.3
    keep = rng.random(p) < 0.85
    pt_a = rng.exponential(1.0, n).astype(np.float32)
    pt_a[::13] = np.nan
    pt_b = rng.exponential(1.0, nb).astype(np.float32)
    scores = (1.0 / (1.0 + np.exp(-4.0 * rng.standard_normal(p)))).astype(np.float32)
    ordinary = np.ones(p, bool)
    for cls in (np.flatnonzero(y & keep), np.flatnonzero(~y & keep)):
        scores[cls[:3]], scores[cls[3:6]] = 0.0, 1.0
        ordinary[cls[:6]] = False
    ordinary &= (scores > 0) & (scores < 1)
    return scores, graph.astype(idt), y, pt_a, pt_b, keep, ordinary


@pytest.mark.parametrize("idt", [np.int64, np.int32])
@pytest.mark.parametrize("p", [200_000, 200_003])
def test_random_cases_vs_restatement(p, idt):
    scores, graph, y, pt_a, _, keep, ordinary = _random_case(p % 1000, 5000, p, idt)
    _check(scores, graph, y, pt_a, HP, ordinary=ordinary)
    _check(scores, graph, y, pt_a, HP, keep=keep, ordinary=ordinary)
    scores, graph, y, pt_a, pt_b, keep, ordinary = _random_case(p % 1000 + 1, 5000, p, idt, nb=3001)
    _check(scores, graph, y, pt_a, HP, pt_b=pt_b, combine="max", ordinary=ordinary)
    _check(scores, graph, y, pt_a, HP, pt_b=pt_b, combine="max", keep=keep, ordinary=ordinary)


def test_grid_stride_path():
    """2048 workgroups x 256 threads x 4 int32 pairs = 2 097 152 pairs fill one grid: P beyond that loops"""
    p = 2048 * 256 * 4 + 12_345
    scores, graph, y, pt_a, _, keep, ordinary = _random_case(11, 5000, p, np.int32)
    _check(scores, graph, y, pt_a, HP, keep=keep, ordinary=ordinary)


@pytest.mark.parametrize("lwr", LWRS)
@pytest.mark.parametrize("mode", MODES)
def test_ec_training_loss_matches_the_reference_fixture(mode, lwr):
    import hierarchicalgnn_amd as H
    hp = fixture_hparams(mode, lwr)
    key = f"{mode}/lwr{lwr:g}"
    batch = {k: torch.from_numpy(Z[f"ev/{k}"]).to(DEV) for k in ("edge_index", "y", "y_pid", "pt")}
    pt0 = batch["pt"].clone()
    s = torch.from_numpy(Z["ev/scores"]).to(DEV).requires_grad_(True)
    loss = H.ec_training_loss(s, batch, hp)
    loss.backward()
    print(f"{key}: loss {float(loss.detach()):.9g} fixture {float(Z[f'{key}/loss']):.9g}")
    conftest.assert_parity(loss.reshape(1), Z[f"{key}/loss"].reshape(1), what="loss")
    conftest.assert_parity(s.grad, Z[f"{key}/grad"], what="dloss/dscores")
    assert torch.equal(batch["pt"].isnan(), pt0.isnan()) and torch.equal(batch["pt"].nan_to_num(), pt0.nan_to_num())
    # the keep mask against the compacted edge list, as training_step (:118-120) forms it
    _, keep = fixture_case(mode)
    k = torch.from_numpy(keep).to(DEV)
    cut = {"edge_index": batch["edge_index"][:, k], "y": batch["y"][k], "y_pid": batch["y_pid"][k],
           "pt": batch["pt"]}
    s_cut = s.detach()[k].requires_grad_(True)
    loss_cut = H.ec_training_loss(s_cut, cut, hp)
    loss_cut.backward()
    assert abs(float(loss) - float(loss_cut)) <= 1e-6 * abs(float(loss_cut))
    assert conftest.rel_err(s.grad[k].cpu().numpy(), s_cut.grad.cpu().numpy()) <= 1e-6
    assert not bool(s.grad[~k].any())
    H.weighted_bce_check()


def test_empty_pair_list_empty_classes_and_empty_keep():
    scores, graph, y, pt_a, _, _, _ = _random_case(1, 100, 1000, np.int64)
    loss, grad = _fused(np.zeros(0, np.float32), np.zeros((2, 0), np.int64), np.zeros(0, bool), pt_a, HP)
    assert float(loss) == 0.0 and grad.shape == (0,)
    for cls in (np.zeros(1000, bool), np.ones(1000, bool)):
        loss, grad = _check(scores, graph, cls, pt_a, HP)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    loss, grad = _check(scores, graph, y, pt_a, HP, keep=np.zeros(1000, bool))
    assert float(loss) == 0.0 and not bool(grad.any())


@pytest.mark.parametrize("what,bad", [("pair id", -1), ("pair id", 100), ("pair id", 1 << 40), ("score", 1.5),
                                      ("score", float("nan")), ("score", -1e-3)])
def test_bad_ids_and_scores_are_skipped_and_reported_not_faulted(what, bad):
    import hierarchicalgnn_amd as H
    rng = np.random.default_rng(4)
    p, n = 10_000, 100
    graph = rng.integers(0, n, (2, p))
    scores = rng.uniform(0.05, 0.95, p).astype(np.float32)
    y = rng.random(p) < 0.4
    pt = rng.exponential(1.0, n).astype(np.float32)
    if what == "pair id":
        graph[1, 777] = bad
    else:
        scores[777] = bad
    keep = np.ones(p, bool)
    keep[777] = False
    H.weighted_bce_check()
    args = (torch.from_numpy(graph).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(pt).to(DEV), HP)
    s = torch.from_numpy(scores).to(DEV).requires_grad_(True)
    with pytest.raises(ValueError, match=what):
        H.weighted_bce_loss(s, *args, check=True)
    loss = H.weighted_bce_loss(s, *args)                                   # lazily: the next check reports it
    loss.backward()
    with pytest.raises(ValueError, match=what):
        H.weighted_bce_check()
    H.weighted_bce_check()                                                 # cleared
    # the pair is skipped: the same loss and gradient as with the pair dropped (and its inputs made harmless)
    graph[1, 777], scores[777] = 0, 0.5
    r_loss, r_grad, _, _ = WR.weighted_bce(scores, graph, y, pt, HP, keep=keep)
    assert abs(float(loss) - r_loss) <= 1e-6 * abs(r_loss)
    conftest.assert_parity(s.grad, r_grad, what="grad_scores")
    assert float(s.grad[777]) == 0.0
    H.weighted_bce_loss(torch.from_numpy(scores).to(DEV), torch.from_numpy(graph).to(DEV), *args[1:],
                        check=True)                                        # a clean call does not raise


def _forward64(scores, graph, y, pt):
    """the forward entry point's outputs: (float32 loss, float64 state)"""
    from hierarchicalgnn_amd import edge_classifier as EC, _lib
    loss = torch.empty(1, device=DEV)
    state = torch.empty(_lib.WB_STATE, dtype=torch.float64, device=DEV)
    status = torch.empty(1, dtype=torch.int32, device=DEV)
    ws, nb = _lib.workspace("hgnn_weighted_bce_workspace_bytes", scores.device, scores.numel(), 0)
    y8 = y.view(torch.uint8)
    _lib.check(_lib.load().hgnn_weighted_bce_forward(
        _lib.ptr(scores), _lib.ptr(graph), _lib.DT_I64, _lib.ptr(y8), None, _lib.ptr(pt), pt.numel(), _lib.ptr(pt),
        pt.numel(), scores.numel(), _lib.WB_COMBINE_SUM, EC._wb_scalars(HP), _lib.ptr(loss), _lib.ptr(state),
        _lib.ptr(status), _lib.ptr(ws), nb, _lib.current_stream(scores.device)), "hgnn_weighted_bce_forward")
    assert int(status) == 0
    return loss, state


def test_bitwise_reproducible_no_host_read_and_the_float64_state():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import _lib
    scores, graph, y, pt_a, _, keep, _ = _random_case(2, 20_000, 1_000_000, np.int64)
    l1, g1 = _fused(scores, graph, y, pt_a, HP, keep=keep)
    l2, g2 = _fused(scores, graph, y, pt_a, HP, keep=keep)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    s = torch.from_numpy(scores).to(DEV).requires_grad_(True)
    g, yy, pt = torch.from_numpy(graph).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(pt_a).to(DEV)
    torch.cuda.synchronize()
    reads = (H.embedding.stats["host_reads"], H.assignment.stats["host_reads"], H.edge_classifier.stats["host_reads"])
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = H.weighted_bce_loss(s, g, yy, pt, HP)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert reads == (H.embedding.stats["host_reads"], H.assignment.stats["host_reads"],
                     H.edge_classifier.stats["host_reads"])
    H.weighted_bce_check()
    assert H.edge_classifier.stats["host_reads"] == reads[2] + 1           # the explicit check is the one read
    loss32, state = _forward64(s.detach(), g, yy, pt)
    r_loss, _, _, (s_t, s_f) = WR.weighted_bce(scores, graph, y, pt_a, HP)
    assert float(loss32) == float(state[_lib.WB_LOSS].float()) == float(loss)
    assert abs(float(state[_lib.WB_LOSS]) - r_loss) <= 1e-6 * r_loss
    assert abs(float(state[_lib.WB_ST]) - s_t) <= 1e-6 * s_t and abs(float(state[_lib.WB_SF]) - s_f) <= 1e-6 * s_f


# ---- the assignment path ------------------------------------------------------------------------------------------
G = conftest.load_golden("assignment_loss.npz")
G_HP = {str(k): float(v) for k, v in zip(G["hparam_keys"], G["hparams"])}


@pytest.mark.parametrize("name", [str(c) for c in G["cases"]])
def test_bipartite_loss_fused_equals_unfused_on_the_fixture(name):
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import assignment
    c = {k: G[f"{name}/{k}"] for k in ("pid", "pt", "bipartite_graph", "scores", "asgmt_loss")}
    batch = {"pid": torch.from_numpy(c["pid"]).to(DEV), "pt": torch.from_numpy(c["pt"]).to(DEV)}
    pt_before = batch["pt"].clone()
    graph = torch.from_numpy(c["bipartite_graph"]).to(DEV)
    out = {}
    for fused in (False, True):
        s = torch.from_numpy(c["scores"]).to(DEV).requires_grad_(True)
        plain = H.bipartite_loss(s.detach(), graph, batch, G_HP, fused=fused)
        reads = assignment.stats["host_reads"]
        loss, d = H.bipartite_loss(s, graph, batch, G_HP, return_details=True, fused=fused)
        loss.backward()
        assert abs(float(plain) - float(loss)) <= (0.0 if fused else 1e-6 * abs(float(loss)))
        out[fused] = (loss.detach(), d, s.grad, reads)
    H.weighted_bce_check()
    (l0, d0, g0, r0), (l1, d1, g1, r1) = out[False], out[True]
    print(f"{name}: unfused {float(l0):.9g} ({r0} reads) fused {float(l1):.9g} ({r1} reads) "
          f"fixture {float(c['asgmt_loss']):.9g}")
    assert r1 == r0 - 4
    assert torch.equal(d0["truth"], d1["truth"]) and d1["truth"].dtype == torch.bool
    assert torch.equal(d0["row_match"], d1["row_match"]) and torch.equal(d0["col_match"], d1["col_match"])
    assert conftest.rel_err(d1["weights"].cpu().numpy(), d0["weights"].cpu().numpy()) <= 1e-6
    assert abs(float(l1) - float(l0)) <= 1e-6 * abs(float(l0))
    conftest.assert_parity(l1.reshape(1), np.array([float(c["asgmt_loss"])]), what="asgmt_loss")
    conftest.assert_parity(g1, g0, what="d asgmt_loss / d scores")
    assert torch.equal(batch["pt"], pt_before), "batch.pt was written"


# ---- end to end ---------------------------------------------------------------------------------------------------
def test_ec_in_training_step_equals_the_torch_composition():
    """EC_InteractionGNN at latent 32: forward, ec_training_loss, backward, against the same step with the loss as
    the torch composition (training_weights + binary_cross_entropy + dot) on the compacted edge list"""
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import synth
    from hierarchicalgnn_amd.models import EC_InteractionGNN
    hp = dict(spatial_channels=3, latent=32, hidden=64, n_interaction_graph_iters=2, nb_node_layer=3,
              nb_edge_layer=2, output_layers=3, hidden_output_activation="GELU", hidden_activation="GELU",
              layernorm=True, share_weight=False, weight_leak=0.1, weight_min=0.1, pt_interval=0.5, ptcut=1.0,
              log_weight_ratio=0.3, true_edges="modulewise_true_edges")
    torch.manual_seed(0)
    n, e = 2000, 12_000
    x, ei = synth.trackml_event(n, e, seed=5)
    x, ei = x.to(DEV), ei.to(DEV)
    g = torch.Generator().manual_seed(5)
    y_pid = torch.rand(e, generator=g) < 0.4
    y = y_pid & (torch.rand(e, generator=g) < 0.7)
    pt = torch.empty(n).exponential_(1.0, generator=g)
    pt[::13] = float("nan")
    batch = {"edge_index": ei, "y": y.to(DEV), "y_pid": y_pid.to(DEV), "pt": pt.to(DEV)}
    model = EC_InteractionGNN(hp).to(DEV).train()

    def step(loss_fn):
        model.zero_grad(set_to_none=True)
        loss = loss_fn(model(x, ei))
        loss.backward()
        return loss.detach(), {k: p.grad.clone() for k, p in model.named_parameters()}

    def torch_loss(scores):
        k = (batch["y_pid"] == 0) | (batch["y"] == 1)
        yy = batch["y"][k]
        w = H.training_weights(batch, ei[:, k], yy, hp)
        return torch.dot(torch.nn.functional.binary_cross_entropy(scores[k], yy.float(), reduction="none"), w)

    l_f, g_f = step(lambda scores: H.ec_training_loss(scores, batch, hp))
    l_t, g_t = step(torch_loss)
    H.weighted_bce_check()
    print(f"EC-IN step: fused loss {float(l_f):.9g} torch {float(l_t):.9g}")
    conftest.assert_parity(l_f.reshape(1), l_t.reshape(1), what="loss")
    assert len(g_f) == len(g_t) > 0
    for k in g_t:
        conftest.assert_parity(g_f[k], g_t[k], what=k)
