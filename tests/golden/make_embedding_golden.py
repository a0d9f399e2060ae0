#!/usr/bin/env python3
"""Generate tests/golden/embedding_samples.npz by IMPORTING the reference's own Modules/utils.py,
GNNEmbedding/embedding_base.py and GNNEmbedding/Models/IN.py.

Run in the build container only (it needs the reference checkout, which never travels to the GPU box):

    python tests/golden/make_embedding_golden.py

graph_intersection is the reference's, on real scipy.  get_training_samples, get_training_weight and
get_hinge_distance are the reference's methods, called on a stand-in ``self`` (hparams, device = cpu) with the
module's FRNN_graph replaced by a function that returns a recorded prediction graph.  Embedding_InteractionGNN is
the reference's class at latent 32 with 2 iterations (CPU), for its forward, one training step's loss and parameter
gradients, and the parameter count of the shipped IN.yaml.
Stand-ins for modules that are absent here and not used by these code paths: frnn, torch_geometric.data,
pytorch_lightning (LightningModule = nn.Module with save_hyperparameters), cupy, cudf, cugraph, wandb, cuml,
sklearn.*, tracking_utils; torch_scatter.scatter_add = Tensor.index_add (the cells' aggregation).
The file is written with fixed zip timestamps, so re-running reproduces it bit for bit.
"""
import importlib.machinery
import io
import json
import os
import sys
import tempfile
import types
import zipfile

sys.dont_write_bytecode = True
sys.pycache_prefix = tempfile.mkdtemp(prefix="golden_pyc_")

import numpy as np
import torch
import yaml

torch.set_num_threads(1)   # the CPU model step in a fixed summation order: the file regenerates bit for bit

REF = os.environ.get("HGNN_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "embedding_samples.npz")
HP_MODEL = dict(spatial_channels=3, latent=32, hidden="ratio", hidden_ratio=2, emb_dim=8,
                n_interaction_graph_iters=2, nb_node_layer=3, nb_edge_layer=2, output_layers=3,
                hidden_output_activation="GELU", hidden_activation="GELU", layernorm=True, share_weight=False)
HP_LOSS = dict(train_r=1.0, knn=100, weight_leak=1.0, weight_min=0.5, pt_interval=0.5, ptcut=1.0,
               log_weight_ratio=0.0)


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)   # torch._dynamo looks modules up by spec
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _scatter_add(src, index, dim=0, dim_size=None):
    assert dim == 0
    out = torch.zeros((dim_size,) + tuple(src.shape[1:]), dtype=src.dtype)
    return out.index_add(0, index, src)


class _LightningModule(torch.nn.Module):
    def save_hyperparameters(self, hp):
        self.hparams = hp

    @property
    def device(self):
        return torch.device("cpu")


def _install_stubs():
    def unused(*a, **k):
        raise NotImplementedError

    _module("frnn", frnn_grid_points=unused)
    _module("torch_geometric")
    _module("torch_geometric.data", Data=dict, DataLoader=unused)
    _module("pytorch_lightning", LightningModule=_LightningModule)
    _module("torch_scatter", scatter_add=_scatter_add, scatter_mean=unused, scatter_min=unused)
    for name in ("cupy", "cudf", "cugraph", "cugraph.structure", "wandb", "sklearn", "sklearn.metrics",
                 "sklearn.mixture"):
        _module(name)
    _module("cugraph.structure.symmetrize", symmetrize=unused)
    sys.modules["sklearn.metrics"].roc_auc_score = unused
    sys.modules["sklearn.mixture"].GaussianMixture = unused
    _module("cuml")
    _module("cuml.cluster", HDBSCAN=lambda **k: None)
    _module("tracking_utils", eval_metrics=unused)


def _import_reference():
    _install_stubs()
    sys.path.insert(0, os.path.join(REF, "Modules"))
    import utils
    from GNNEmbedding import embedding_base
    from GNNEmbedding.Models import IN
    return utils, embedding_base, IN


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
def intersection_cases(rng):
    out = {}
    # duplicates in both, self loops, pairs only in truth, c1 > c2 (2 pred copies vs 1) and c1 < c2 (1 vs 2)
    pred = np.array([[0, 0, 1, 2, 2, 2, 3, 5, 5, 6], [1, 1, 0, 2, 2, 3, 3, 4, 4, 0]])
    truth = np.array([[0, 2, 2, 2, 3, 7, 5, 6, 6], [1, 2, 3, 3, 3, 7, 9, 0, 0]])
    out["small"] = (pred, truth)
    n = 400
    pred = rng.integers(0, n, (2, 6000))
    pred = np.concatenate([pred, pred[:, rng.integers(0, 6000, 2000)], np.stack([np.arange(50)] * 2)], 1)
    truth = np.concatenate([pred[:, rng.integers(0, pred.shape[1], 800)], rng.integers(0, n, (2, 700))], 1)
    truth = np.concatenate([truth, truth[:, rng.integers(0, truth.shape[1], 300)]], 1)   # duplicate truth pairs
    out["random"] = (pred[:, rng.permutation(pred.shape[1])], truth[:, rng.permutation(truth.shape[1])])
    out["empty_truth"] = (pred[:, :100], np.zeros((2, 0), np.int64))
    return out


def event(rng, n=600, hpp=8):
    n_noise = n // 10
    part = rng.integers(0, (n - n_noise) // hpp, n - n_noise)
    pid = np.concatenate([part + 1, np.zeros(n_noise, np.int64)])
    pt_p = 0.2 + rng.exponential(1.0, part.max() + 1)
    pt = np.concatenate([pt_p[part], np.zeros(n_noise)]).astype(np.float32)
    pt[rng.integers(0, n, 5)] = np.nan                                  # pt_weighting's NaN -> 0
    perm = rng.permutation(n)
    pid, pt = pid[perm], pt[perm]
    signal_mask = rng.random(n) >= 0.1
    order = np.argsort(pid * n + np.arange(n), kind="stable")
    ps = pid[order]
    same = (ps[1:] == ps[:-1]) & (ps[1:] != 0)
    mte = np.stack([order[:-1][same], order[1:][same]])
    # the recorded prediction graph: per query (ascending) up to 12 neighbours, self first; same-particle and
    # foreign pairs, noise included
    rows, cols = [], []
    for q in range(n):
        mates = np.nonzero((pid == pid[q]) & (pid != 0))[0]
        nb = np.concatenate([[q], rng.choice(mates, min(4, mates.size)), rng.integers(0, n, rng.integers(2, 8))])
        rows.append(np.full(nb.size, q))
        cols.append(nb)
    pred = np.stack([np.concatenate(rows), np.concatenate(cols)]).astype(np.int64)
    return dict(pid=pid.astype(np.int64), pt=pt, signal_mask=signal_mask, modulewise_true_edges=mte.astype(np.int64),
                pred=pred)


class Batch(dict):
    __getattr__ = dict.__getitem__


def main():
    utils, eb, IN = _import_reference()
    rng = np.random.default_rng(20261016)
    arrays = {}

    names = []
    for name, (pred, truth) in intersection_cases(rng).items():
        names.append(name)
        arrays[f"gi/{name}/pred"] = pred.astype(np.int64)
        arrays[f"gi/{name}/truth"] = truth.astype(np.int64)
        try:
            g, y = utils.graph_intersection(torch.from_numpy(pred), torch.from_numpy(truth))
            arrays[f"gi/{name}/graph"], arrays[f"gi/{name}/y"] = g.numpy(), y.numpy()
            status = 0
        except RuntimeError:       # the reference takes .max() of the truth graph: empty truth raises
            status = 1
        arrays[f"gi/{name}/status"] = np.array(status, np.int64)
        if status == 0:
            for dt in (np.float32, np.float64):
                w = (rng.random(truth.shape[1]) * 4).astype(dt)
                g, y, nw = utils.graph_intersection(torch.from_numpy(pred), torch.from_numpy(truth), True,
                                                    torch.from_numpy(w))
                key = np.dtype(dt).name
                arrays[f"gi/{name}/w_{key}"] = w
                arrays[f"gi/{name}/new_w_{key}"] = nw.numpy()
        print(f"graph_intersection {name:12s} status={status}")
    arrays["gi/cases"] = np.array(names)

    ev = event(rng)
    for k, v in ev.items():
        arrays[f"ev/{k}"] = v
    emb = torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((ev["pid"].size, 8)).astype(np.float32)))
    arrays["ev/embeddings"] = emb.numpy()
    batch = Batch({k: torch.from_numpy(v) for k, v in ev.items() if k != "pred"})
    eb.FRNN_graph = lambda embeddings, r, k: torch.from_numpy(ev["pred"])
    for mode in ("modulewise_true_edges", "pid_true_edges"):
        me = types.SimpleNamespace(hparams=dict(HP_LOSS, true_edges=mode), device=torch.device("cpu"))
        me.pt_weighting = types.MethodType(eb.EmbeddingBase.pt_weighting, me)
        pt_before = batch.pt.clone()
        g, y = eb.EmbeddingBase.get_training_samples(me, emb, batch)
        w = eb.EmbeddingBase.get_training_weight(me, batch, g, y)
        hinge, dist = eb.EmbeddingBase.get_hinge_distance(me, batch, emb, g, y)
        loss = torch.nn.functional.hinge_embedding_loss(dist, hinge, margin=1.0, reduction="none").square()
        loss = torch.dot(loss, w)
        assert np.array_equal(pt_before.numpy(), batch.pt.numpy(), equal_nan=True)
        for k, v in (("graph", g), ("y", y), ("weights", w), ("hinge", hinge), ("dist", dist), ("loss", loss)):
            arrays[f"ts/{mode}/{k}"] = v.numpy()
        print(f"training_samples {mode}: {g.shape[1]} pairs, {int(y.sum())} true, loss {float(loss):.6g}")

    # the shipped IN.yaml: parsed config and parameter count of the reference model
    with open(os.path.join(REF, "Modules", "GNNEmbedding", "Configs", "IN.yaml")) as f:
        raw = yaml.safe_load(f)
    arrays["model/in_yaml"] = np.array(json.dumps(raw, sort_keys=True))
    hp = dict(raw)
    hp["hidden"] = hp["hidden_ratio"] * hp["latent"]
    full = IN.Embedding_InteractionGNN(hp)
    arrays["model/in_yaml_n_params"] = np.array(sum(p.numel() for p in full.parameters()), np.int64)
    arrays["model/in_yaml_keys"] = np.array(list(full.state_dict()))

    # latent-32 model: forward, one step's loss on the recorded samples and the parameter gradients
    torch.manual_seed(0)
    hp = dict(raw, **HP_MODEL)
    hp["hidden"] = hp["hidden_ratio"] * hp["latent"]
    model = IN.Embedding_InteractionGNN(hp)
    n = ev["pid"].size
    x = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
    graph = torch.from_numpy(rng.integers(0, n, (2, 3 * n)).astype(np.int64))
    arrays["model/x"], arrays["model/graph"] = x.numpy(), graph.numpy()
    embeddings = model(x.clone(), graph)
    # the model case's prediction graph is a real fixed-radius kNN (k = 100) of its embeddings.  A freshly
    # initialised model puts the embeddings close together, so r is chosen from the data: below every row's 100th
    # distance (no row is cut by k) and with no distance within 1e-5 of r^2 (r^2 = fl32(r)^2, the kernel's
    # arithmetic) -- the pair set is then unambiguous; the modulewise samples are sorted pairs, so the order inside a
    # row does not matter
    with torch.no_grad():
        e = embeddings.detach()
        d2 = torch.zeros(n, n)
        for d in range(e.shape[1]):
            t = e[:, d:d + 1] - e[:, d].unsqueeze(0)
            d2 = torch.addcmul(d2, t, t)
        ds = torch.sort(d2, dim=1).values
        r = float(np.float32(np.sqrt(float(ds[:, 99].min()) * 0.9)))
        while True:
            r2 = float(np.float32(r) * np.float32(r))
            if not bool(((d2 - r2).abs() < 1e-5).any()):
                break
            r = float(np.float32(r * 0.997))
        assert int((d2 < r2).sum(1).max()) < 100 and int((d2 < r2).sum(1).min()) >= 1
        order = torch.argsort(d2, dim=1, stable=True)[:, :100]
        ds = torch.gather(d2, 1, order)
        idx = torch.where(ds < r2, order, torch.full_like(order, -1))
        pos = idx >= 0
        ind = torch.arange(n).unsqueeze(1).expand(idx.shape)
        pred = torch.stack([ind[pos], idx[pos]])
    arrays["model/train_r"] = np.array(r, np.float64)
    arrays["model/pred"] = pred.numpy()
    eb.FRNN_graph = lambda embeddings, r, k: pred
    me = types.SimpleNamespace(hparams=dict(hp, **dict(HP_LOSS, train_r=r), true_edges="modulewise_true_edges"),
                               device=torch.device("cpu"))
    me.pt_weighting = types.MethodType(eb.EmbeddingBase.pt_weighting, me)
    g, y = eb.EmbeddingBase.get_training_samples(me, embeddings, batch)
    w = eb.EmbeddingBase.get_training_weight(me, batch, g, y)
    hinge, dist = eb.EmbeddingBase.get_hinge_distance(me, batch, embeddings, g, y)
    loss = torch.dot(torch.nn.functional.hinge_embedding_loss(dist, hinge, margin=r, reduction="none").square(), w)
    loss.backward()
    arrays["model/embeddings"] = embeddings.detach().numpy()
    arrays["model/loss"] = loss.detach().numpy()
    for k, v in model.state_dict().items():
        arrays[f"model/sd/{k}"] = v.numpy()
    for k, p in model.named_parameters():
        if p.grad is not None:      # the last cell's edge network does not reach the embeddings
            arrays[f"model/grad/{k}"] = p.grad.numpy()
    print(f"model: {len(list(model.parameters()))} tensors, loss {float(loss):.6g}, "
          f"IN.yaml params {int(arrays['model/in_yaml_n_params'])}")

    with zipfile.ZipFile(OUT, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
