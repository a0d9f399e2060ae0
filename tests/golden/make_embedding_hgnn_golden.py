#!/usr/bin/env python3
"""Generate tests/golden/embedding_hgnn.npz (emb/*, cfg/*) and embedding_hgnn_gmrt.npz (gmrt/*) by IMPORTING the reference's Embedding-HGNN-GMM and gMRT models.

    python tests/golden/make_embedding_hgnn_golden.py

Same method and stand-ins as make_golden.py (torch_scatter as zeros().scatter_add, containers for Lightning / PyG,
brute-force kNN for frnn, scipy connected components for cugraph; sklearn's GaussianMixture and scipy's fsolve are the
real ones), plus empty cuml / wandb / tracking_utils modules that the embedding base imports and never calls here.
The reference's own classes run on CPU fp32, eval() mode (no running statistic moves), one thread; the file holds
arrays and parsed settings only and regenerates bit for bit (fixed zip timestamps).

Weights are seeded.fill_parameters (checksums stored, as for the bc_hgnn_train fixtures); graphs are stored as int32.

  emb/*   Embedding_HierarchicalGNN_GMM, latent 32, 2 + 2 iterations, on a synth_tracks event: weights, x, graph,
          the captured hierarchy (clusters, bipartite and super graph), both embeddings, the reference training_step's
          two loss terms and combined loss at loss_schedule = 0.3 on a recorded prediction graph, parameter gradients
  gmrt/*  gMRT, latent 32, 2 iterations: weights, forward outputs with the captured hierarchy, the gradients of
          make_golden.py's surrogate loss
  cfg/*   the two shipped HGNN_GMM.yaml files: parsed settings, parameter counts and state-dict key lists
"""
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch
import yaml

import make_golden as MG
import seeded

REF = MG.REF
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "embedding_hgnn.npz")
OUT_GMRT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "embedding_hgnn_gmrt.npz")
HP_SMALL = dict(latent=32, hidden=64, n_interaction_graph_iters=2, n_hierarchical_graph_iters=2)
HP_LOSS = dict(train_r=1.0, knn=100, weight_leak=1.0, weight_min=0.5, pt_interval=0.5, ptcut=1.0,
               log_weight_ratio=0.0, true_edges="modulewise_true_edges", loss_schedule=0.3)
CUT_MARGIN = 1e-4


class Batch(dict):
    __getattr__ = dict.__getitem__


def _import_reference():
    MG._install_stubs()
    pl = sys.modules["pytorch_lightning"]
    pl.LightningModule.device = property(lambda self: torch.device("cpu"))
    for name in ("wandb", "cuml", "cuml.cluster", "tracking_utils"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["cuml.cluster"].HDBSCAN = lambda **k: None
    sys.modules["tracking_utils"].eval_metrics = None
    sys.path.insert(0, os.path.join(REF, "Modules"))
    from GNNEmbedding import embedding_base
    from GNNEmbedding.Models.HGNN_GMM import Embedding_HierarchicalGNN_GMM
    from gMRT.Models.HGNN_GMM import gMRT
    return embedding_base, Embedding_HierarchicalGNN_GMM, gMRT


def _config(rel):
    with open(os.path.join(REF, "Modules", rel)) as f:
        raw = yaml.safe_load(f)
    hp = dict(raw)
    hp["hidden"] = hp["hidden_ratio"] * hp["latent"]
    hp.setdefault("cluster_granularity", 0)
    return raw, hp


def _capture(hb):
    """record the hierarchy decision of one reference forward: cluster labels, bipartite and super graph"""
    cap = {}
    real = hb.clustering

    def clustering(xx, emb, gr):
        cl = real(xx, emb, gr)
        with torch.no_grad():
            lik = torch.atanh(torch.clamp(torch.einsum("ij,ij->i", emb[gr[0]], emb[gr[1]]), -1 + 1e-7, 1 - 1e-7))
        cap["clusters"], cap["likelihood"] = cl.detach().clone(), lik
        return cl

    hb.clustering = clustering
    hb.bipartite_graph_construction.register_forward_hook(
        lambda m, i, o: cap.__setitem__("bg", o[0].detach().clone()))
    hb.super_graph_construction.register_forward_hook(lambda m, i, o: cap.__setitem__("sg", o[0].detach().clone()))
    return cap


def _assert_cut_is_clear(cap, hb):
    gap = float((cap["likelihood"] - hb.score_cut).abs().min())
    assert gap > CUT_MARGIN, f"an edge likelihood lies within {CUT_MARGIN} of the cut ({gap}): pick another event"
    assert int(cap["clusters"].max()) > 2       # the cut graph was used, not the fall-back to the uncut graph
    return gap


def _event(gen, n_tracks=70, hits=9):
    x, graph = MG.synth_tracks(n_tracks, hits, gen)
    n = x.shape[0]
    pid = torch.arange(n_tracks).repeat_interleave(hits) + 1
    pid[torch.randperm(n, generator=gen)[:n // 12]] = 0                      # noise hits
    pt_track = 0.2 + torch.empty(n_tracks + 1).exponential_(1.0, generator=gen)
    pt = pt_track[pid].float()
    pt[pid == 0] = 0
    pt[torch.randperm(n, generator=gen)[:4]] = float("nan")
    signal_mask = torch.rand(n, generator=gen) >= 0.1
    i = torch.arange(n - 1)
    same = (pid[i] == pid[i + 1]) & (pid[i] != 0)
    return x, graph, Batch(x=x, edge_index=graph, pid=pid, pt=pt, signal_mask=signal_mask,
                           modulewise_true_edges=torch.stack([i[same], i[same] + 1]))


def _store_model(model, seed, tag, arrays):
    """The weights are seeded.fill_parameters(model, seed), as for the bc_hgnn_train fixtures: stored are their
    checksums, the buffers, the shapes of the whole state dict and the gradient of EVERY parameter that has one.
    Returns the names of the parameters without a gradient."""
    named = list(model.named_parameters())
    params = {n for n, _ in named}
    arrays[f"{tag}/seed"] = np.array(seed, np.int64)
    arrays[f"{tag}/param_checksums"] = seeded.checksums(named)
    arrays[f"{tag}/sd_shapes"] = np.array(json.dumps({k: list(v.shape) for k, v in model.state_dict().items()}))
    for k, v in model.state_dict().items():
        if k not in params:
            arrays[f"{tag}/buffer/{k}"] = v.numpy().copy()
    no_grad = [n for n, p in named if p.grad is None]
    for n, p in named:
        if p.grad is not None:
            arrays[f"{tag}/grad/{n}"] = p.grad.numpy()
    arrays[f"{tag}/params_without_grad"] = np.array(json.dumps(no_grad))
    return no_grad


def gen_embedding(eb, Model, arrays):
    raw, hp_full = _config("GNNEmbedding/Configs/HGNN_GMM.yaml")
    full = Model(hp_full)
    arrays["cfg/emb/yaml"] = np.array(json.dumps(raw, sort_keys=True))
    arrays["cfg/emb/n_params"] = np.array(sum(p.numel() for p in full.parameters()), np.int64)
    arrays["cfg/emb/keys"] = np.array(json.dumps(list(full.state_dict())))
    del full
    gen = torch.Generator().manual_seed(9301)
    torch.manual_seed(9301)
    np.random.seed(9301)
    hp = dict(hp_full, **HP_SMALL, **HP_LOSS)
    model = Model(hp)
    seeded.fill_parameters(model, 9301)
    model.eval()
    hb = model.hgnn_block
    hb.super_graph_construction.knn_radius.fill_(2.0)
    hb.bipartite_graph_construction.knn_radius.fill_(2.0)
    cap = _capture(hb)
    x, graph, batch = _event(gen)
    pred = {}

    def frnn_graph(embeddings, r, k):
        """the recorded prediction graph: every hit's 12 nearest hits (itself included), query ascending"""
        with torch.no_grad():
            order = torch.argsort(torch.cdist(embeddings, embeddings), dim=1, stable=True)[:, :12]
            ind = torch.arange(order.shape[0]).unsqueeze(1).expand(order.shape)
            pred["graph"] = torch.stack([ind.reshape(-1), order.reshape(-1)])
        return pred["graph"]

    eb.FRNN_graph = frnn_graph
    logged = {}
    model.log_dict = lambda d, *a, **k: logged.update(d)
    embeddings, intermediate, clusters = model(x.clone(), graph)
    gap = _assert_cut_is_clear(cap, hb)
    assert torch.equal(clusters, cap["clusters"])
    loss = model.training_step(batch, 0)          # runs the forward again: same weights, same event, eval mode
    assert torch.equal(cap["clusters"], clusters)
    loss.backward()
    arrays.update({"emb/x": x.detach().numpy(), "emb/graph": graph.numpy(), "emb/clusters": clusters.numpy(),
                   "emb/bipartite_graph": cap["bg"].numpy().astype(np.int32),
                   "emb/super_graph": cap["sg"].numpy().astype(np.int32),
                   "emb/score_cut": hb.score_cut.numpy().copy(), "emb/cut_gap": np.array(gap),
                   "emb/embeddings": embeddings.detach().numpy(), "emb/intermediate": intermediate.detach().numpy(),
                   "emb/pred": pred["graph"].numpy().astype(np.int32), "emb/loss": loss.detach().numpy(),
                   "emb/emb_loss": logged["embedding_loss"].detach().numpy(),
                   "emb/intermediate_loss": logged["intermediate_loss"].detach().numpy(),
                   "emb/loss_schedule": np.array(HP_LOSS["loss_schedule"]),
                   "emb/hp": np.array(json.dumps({k: v for k, v in hp.items()}, sort_keys=True))})
    for k in ("pid", "pt", "signal_mask", "modulewise_true_edges"):
        arrays[f"emb/ev/{k}"] = batch[k].numpy()
    no_grad = _store_model(model, 9301, "emb", arrays)
    print(f"emb: {x.shape[0]} hits, {int(clusters.max()) + 1} clusters, cut gap {gap:.3g}, loss {float(loss):.6g} "
          f"(emb {float(logged['embedding_loss']):.6g}, intermediate {float(logged['intermediate_loss']):.6g}), "
          f"params without grad: {len(no_grad)}")


def gen_gmrt(Model, arrays, c_emb=0.1):
    raw, hp_full = _config("gMRT/Configs/HGNN_GMM.yaml")
    full = Model(hp_full)
    arrays["cfg/gmrt/yaml"] = np.array(json.dumps(raw, sort_keys=True))
    arrays["cfg/gmrt/n_params"] = np.array(sum(p.numel() for p in full.parameters()), np.int64)
    arrays["cfg/gmrt/keys"] = np.array(json.dumps(list(full.state_dict())))
    del full
    seed = 9302
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)
    hp = dict(hp_full, **HP_SMALL)
    model = Model(hp)
    seeded.fill_parameters(model, seed)
    model.eval()
    hb = model.hgnn_block
    hb.super_graph_construction.knn_radius.fill_(2.0)
    hb.bipartite_graph_construction.knn_radius.fill_(2.0)
    cap = _capture(hb)
    x, graph = MG.synth_tracks(70, 9, gen)
    bg, scores, emb = model(x.clone(), graph)
    gap = _assert_cut_is_clear(cap, hb)
    assert torch.equal(bg, cap["bg"])
    r = seeded.randn(seed, "r_scores", scores.shape[0])
    loss = (scores * r).sum() + c_emb * (emb * emb.roll(1, 0)).sum()
    loss.backward()
    arrays.update({"gmrt/x": x.detach().numpy(), "gmrt/graph": graph.numpy(), "gmrt/clusters": cap["clusters"].numpy(),
                   "gmrt/bipartite_graph": cap["bg"].numpy().astype(np.int32),
                   "gmrt/super_graph": cap["sg"].numpy().astype(np.int32),
                   "gmrt/score_cut": hb.score_cut.numpy().copy(), "gmrt/cut_gap": np.array(gap),
                   "gmrt/bipartite_scores": scores.detach().numpy(), "gmrt/embeddings": emb.detach().numpy(),
                   "gmrt/r_scores": r.numpy(), "gmrt/c_emb": np.array(c_emb), "gmrt/loss": loss.detach().numpy(),
                   "gmrt/hp": np.array(json.dumps({k: v for k, v in hp.items()}, sort_keys=True))})
    _store_model(model, seed, "gmrt", arrays)
    print(f"gmrt: {int(cap['clusters'].max()) + 1} clusters, {bg.shape[1]} bipartite edges, cut gap {gap:.3g}, "
          f"loss {float(loss):.6g}")


def _write(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


def main():
    eb, Emb, GMRT = _import_reference()
    arrays = {}
    gen_embedding(eb, Emb, arrays)
    gen_gmrt(GMRT, arrays)
    # two files, each below the size limit of a committed file: every gradient of both models is 1.1 MB of floats
    _write(OUT, {k: v for k, v in arrays.items() if not k.startswith("gmrt/")})
    _write(OUT_GMRT, {k: v for k, v in arrays.items() if k.startswith("gmrt/")})


if __name__ == "__main__":
    main()
