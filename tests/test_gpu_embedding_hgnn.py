"""GPU: the Embedding-HGNN-GMM and gMRT mirrors against the reference's own outputs (tests/golden/embedding_hgnn.npz,
made by tests/golden/make_embedding_hgnn_golden.py), with the recorded hierarchy injected and with the GPU hierarchy
decision, and one full training step of the embedding stage on the fused pair hinge loss."""
import json
import os

import numpy as np
import pytest
import torch

import conftest
from golden import seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
def _load():
    z = {}
    for name in ("embedding_hgnn.npz", "embedding_hgnn_gmrt.npz"):
        with np.load(os.path.join(conftest.GOLDEN, name), allow_pickle=False) as f:
            z.update({k: f[k] for k in f.files})
    return z


Z = _load()


def _model(tag, fp32_gemm):
    from hierarchicalgnn_amd import models
    hp = dict(json.loads(str(Z[f"{tag}/hp"])), fp32_gemm=fp32_gemm)
    m = {"emb": models.Embedding_HierarchicalGNN_GMM, "gmrt": models.gMRT}[tag](hp)
    seeded.fill_parameters(m, int(Z[f"{tag}/seed"]))
    seeded.check_parameters(m, Z[f"{tag}/param_checksums"])
    sd = m.state_dict()
    for k in Z:
        if k.startswith(f"{tag}/buffer/"):
            sd[k[len(f"{tag}/buffer/"):]] = torch.from_numpy(Z[k])
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval(), hp


def _t(key, dtype=None):
    t = torch.from_numpy(Z[key])
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _hierarchy(tag):
    return _t(f"{tag}/clusters"), _t(f"{tag}/bipartite_graph", torch.int64), _t(f"{tag}/super_graph", torch.int64)


def _batch():
    b = {k: _t(f"emb/ev/{k}") for k in ("pid", "pt", "signal_mask", "modulewise_true_edges")}
    b["edge_index"] = _t("emb/graph")
    return b


def _check_grads(tag, model, tol=1e-4):
    """EVERY parameter gradient against the reference's, to the parity bar"""
    without = set(json.loads(str(Z[f"{tag}/params_without_grad"])))
    stored = {k[len(f"{tag}/grad/"):] for k in Z if k.startswith(f"{tag}/grad/")}
    params = dict(model.named_parameters())
    assert stored | without == set(params) and not stored & without
    for n, p in params.items():
        if n in without:
            assert p.grad is None or not bool(p.grad.any()), n
            continue
        ref = Z[f"{tag}/grad/{n}"]
        if float(np.abs(ref).sum()) < 1e-6:
            # analytically ZERO (the bias of the BatchNorm in front of a mean-normalised exp weight: exp(bias)
            # cancels in w / mean(w)): rounding residue in the reference's evaluation (|g| ~ 1e-9) and in any
            # other; held to the absolute floor tests/test_gpu_configs.py states for it, not to a ratio of residues
            assert float(p.grad.abs().sum()) <= 1e-6, (n, p.grad, ref)
        else:
            conftest.assert_parity(p.grad, ref, tol=tol, what=n)


def _same_partition(a, b):
    """identical partition of the hits up to a renumbering of the clusters (-1 = unclustered stays -1)"""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = np.unique(np.stack([a, b]), axis=1)
    return pairs.shape[1] == np.unique(a).size == np.unique(b).size


@pytest.mark.both_fp32_gemms(must_run=False)
def test_embedding_hgnn_matches_reference_with_injected_hierarchy(fp32_gemm):
    import hierarchicalgnn_amd as H
    model, hp = _model("emb", fp32_gemm)
    x = _t("emb/x")
    emb, inter, clusters = model(x, _t("emb/graph"), hierarchy=_hierarchy("emb"))
    conftest.assert_parity(inter, Z["emb/intermediate"], what="intermediate embeddings")
    conftest.assert_parity(emb, Z["emb/embeddings"], what="embeddings")
    assert np.array_equal(clusters.cpu().numpy(), Z["emb/clusters"])
    loss, emb_loss, inter_loss = H.embedding_hgnn_training_loss(
        emb, inter, _batch(), hp, float(Z["emb/loss_schedule"]), prediction_graph=_t("emb/pred", torch.int64))
    for got, key in ((loss, "loss"), (emb_loss, "emb_loss"), (inter_loss, "intermediate_loss")):
        conftest.assert_parity(got.detach().reshape(1), Z[f"emb/{key}"].reshape(1), what=key)
    loss.backward()
    _check_grads("emb", model)


@pytest.mark.both_fp32_gemms(must_run=False)
def test_gmrt_matches_reference_with_injected_hierarchy(fp32_gemm):
    model, hp = _model("gmrt", fp32_gemm)
    bg, scores, emb = model(_t("gmrt/x"), _t("gmrt/graph"), hierarchy=_hierarchy("gmrt"))
    assert np.array_equal(bg.cpu().numpy(), Z["gmrt/bipartite_graph"])
    conftest.assert_parity(emb, Z["gmrt/embeddings"], what="embeddings")
    conftest.assert_parity(scores, Z["gmrt/bipartite_scores"], what="bipartite_scores")
    r = _t("gmrt/r_scores")
    loss = (scores * r).sum() + float(Z["gmrt/c_emb"]) * (emb * emb.roll(1, 0)).sum()
    conftest.assert_parity(loss.detach().reshape(1), Z["gmrt/loss"].reshape(1), what="loss")
    loss.backward()
    _check_grads("gmrt", model)


@pytest.mark.both_fp32_gemms(must_run=False)
@pytest.mark.parametrize("tag", ["emb", "gmrt"])
def test_gpu_hierarchy_decision_end_to_end(tag, fp32_gemm):
    """the GPU hierarchy decision instead of the injected one: the forward runs, and the clusters are the recorded
    partition (the generator asserts that no edge likelihood lies within 1e-4 of the cut on this event)"""
    model, hp = _model(tag, fp32_gemm)
    with torch.no_grad():
        out = model(_t(f"{tag}/x"), _t(f"{tag}/graph"))
    if tag == "emb":
        emb, inter, clusters = out
        assert emb.shape == inter.shape == (Z["emb/x"].shape[0], 8) and bool(torch.isfinite(emb).all())
        assert _same_partition(clusters.cpu().numpy(), Z["emb/clusters"])
    else:
        bg, scores, emb = out
        assert bg.shape[0] == 2 and scores.shape == (bg.shape[1],) and bool(torch.isfinite(scores).all())
        with torch.no_grad():
            clusters = model.hgnn_block.clustering(emb, model.embed(_t("gmrt/x"), _t("gmrt/graph"))[0])
        assert _same_partition(clusters.cpu().numpy(), Z["gmrt/clusters"])


@pytest.mark.both_fp32_gemms(must_run=False)
def test_full_training_step_is_finite_and_reproducible(fp32_gemm):
    import hierarchicalgnn_amd as H
    model, hp = _model("emb", fp32_gemm)
    model.train()
    batch = _batch()
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        model.hgnn_block.score_cut.copy_(_t("emb/buffer/hgnn_block.score_cut"))
        emb, inter, _ = model(_t("emb/x"), batch["edge_index"], hierarchy=_hierarchy("emb"))
        loss, emb_loss, inter_loss = H.embedding_hgnn_training_loss(emb, inter, batch, hp, 0.3,
                                                                    prediction_graph=_t("emb/pred", torch.int64))
        loss.backward()
        grads = [p.grad.detach().clone() for p in model.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
        runs.append([loss.detach().clone(), emb_loss.detach().clone(), inter_loss.detach().clone()] + grads)
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs))
    # with the kNN pair construction of the step itself (frnn_graph + graph_intersection)
    emb, inter, _ = model(_t("emb/x"), batch["edge_index"])
    loss, _, _ = H.embedding_hgnn_training_loss(emb, inter, batch, hp, 0.3)
    loss.backward()
    assert bool(torch.isfinite(loss))


def test_track_candidates_and_metrics_run_on_the_output():
    import hierarchicalgnn_amd as H
    model, hp = _model("emb", "exact")
    with torch.no_grad():
        emb, _, _ = model(_t("emb/x"), _t("emb/graph"))
    batch = _batch()
    cand = H.embedding_track_candidates(emb, min_cluster_size=3)
    assert cand.shape[0] == 2 and cand.shape[1] > 0
    event = dict(batch, pt=batch["pt"].nan_to_num())
    metrics = H.eval_metrics(cand, event, pt_cut=1.0, nhits_cut=5, majority_cut=0.5, primary=False)
    assert metrics is not None
