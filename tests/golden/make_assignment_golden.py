#!/usr/bin/env python3
"""Generate tests/golden/assignment_loss.npz by RUNNING the reference's own
BipartiteClassificationBase.get_bipartite_loss and the embedding-loss lines of its training_step on the CPU.

Run in the build container only (it needs the reference checkout, which never travels to the GPU box):

    python tests/golden/make_assignment_golden.py

The reference module imports pytorch_lightning, torch_geometric and torch_scatter, none of which exist here, and its
own ``utils`` / ``tracking_utils`` (frnn, cupy).  Stand-ins, in the style of make_tracking_golden.py:
  * pytorch_lightning.LightningModule: a torch.nn.Module with ``save_hyperparameters`` (stores ``hparams``) and a
    ``device`` of "cpu".
  * torch_geometric.data: empty DataLoader / Data names (never called by the methods run here).
  * torch_scatter.scatter_min = Tensor.scatter_reduce("amin", include_self=False).
  * utils / tracking_utils: modules that only carry the imported names.
scipy's csr_matrix and min_weight_full_bipartite_matching are the real ones.

Cases: small events (50-300 particles) with scores on the 2^-12 grid (float32 and float64 sums are then exact and
equal): plain, with noise hits, more particles than clusters, fewer particles than clusters, and one where particles
that share their only cluster must fall back to the virtual column.  Every event is certified to have a UNIQUE optimal
matching by a margin above gap_bound (tests/assign_ref.py:certify_unique); seeds are advanced until it is, and the
margin found is stored.  Inputs, the matching after the noise / virtual filter, truth, the weights and both losses
are stored.  The file is written with fixed zip timestamps, so re-running reproduces it bit for bit.
"""
import io
import os
import sys
import tempfile
import types
import zipfile

sys.dont_write_bytecode = True
sys.pycache_prefix = tempfile.mkdtemp(prefix="golden_pyc_")

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import assign_ref as R   # noqa: E402

REF = os.environ.get("HGNN_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "assignment_loss.npz")
HP_KEYS = ("weight_leak", "ptcut", "pt_interval", "weight_min", "log_weight_ratio", "train_r")
SCALE_BITS = 30


def _install_stubs():
    pl = types.ModuleType("pytorch_lightning")

    class LightningModule(torch.nn.Module):
        device = "cpu"

        def save_hyperparameters(self, hparams):
            self.hparams = dict(hparams)

    pl.LightningModule = LightningModule
    sys.modules["pytorch_lightning"] = pl
    tg, tgd = types.ModuleType("torch_geometric"), types.ModuleType("torch_geometric.data")
    tgd.DataLoader = tgd.Data = None
    tg.data = tgd
    sys.modules["torch_geometric"], sys.modules["torch_geometric.data"] = tg, tgd
    ts = types.ModuleType("torch_scatter")

    def scatter_min(src, index, dim=0, dim_size=None):
        assert dim == 0
        out = torch.zeros(int(dim_size), dtype=src.dtype).scatter_reduce(0, index, src, "amin", include_self=False)
        return out, None

    ts.scatter_min = scatter_min
    sys.modules["torch_scatter"] = ts
    ut = types.ModuleType("utils")
    ut.TrackMLDataset = ut.load_dataset_paths = ut.FRNN_graph = ut.graph_intersection = None
    sys.modules["utils"] = ut
    tu = types.ModuleType("tracking_utils")
    tu.eval_metrics = None
    sys.modules["tracking_utils"] = tu


def _import_reference():
    _install_stubs()
    sys.path.insert(0, os.path.join(REF, "Modules", "BipartiteClassification"))
    import bipartite_classification_base as b
    return b


class Event(dict):
    __getattr__ = dict.__getitem__


def make_event(rng, n_particles, n_clusters, k=3, noise=0.0, shared_only_cluster=0):
    sizes = 2 + rng.poisson(5, n_particles)
    pids = rng.choice(np.arange(1, 1 << 20, dtype=np.int64), n_particles, replace=False)
    pid = np.repeat(pids, sizes)
    pt_p = (0.3 + rng.exponential(1.0, n_particles)).astype(np.float32)
    pt = (np.repeat(pt_p, sizes) * (1 + 0.05 * rng.random(pid.size))).astype(np.float32)
    home = np.repeat(rng.integers(0, n_clusters, n_particles), sizes)
    part = np.repeat(np.arange(n_particles), sizes)
    n_noise = int(noise * pid.size)
    pid = np.concatenate([pid, np.zeros(n_noise, np.int64)])
    pt = np.concatenate([pt, np.zeros(n_noise, np.float32)])
    home = np.concatenate([home, rng.integers(0, n_clusters, n_noise)])
    part = np.concatenate([part, np.full(n_noise, -1)])
    n = pid.size
    col = rng.integers(0, n_clusters, (n, k))
    col[:, 0] = home
    score = rng.integers(1, 2400, (n, k))
    score[:, 0] = rng.integers(2048, 4097, n)
    # the first `shared_only_cluster` pairs of particles share one cluster and have no other edge
    lonely = np.zeros(n, bool)
    for s in range(shared_only_cluster):
        a, b = 2 * s, 2 * s + 1
        col[(part == a) | (part == b), :] = col[part == a][0, 0]
        lonely |= (part == a) | (part == b)
    hit = np.repeat(np.arange(n), k)
    col, score = col.reshape(-1), score.reshape(-1)
    keep = ~(np.repeat(lonely, k) & (np.tile(np.arange(k), n) > 0))
    hit, col, score = hit[keep], col[keep], score[keep]
    col[-1] = n_clusters - 1   # the reference sizes the problem by bipartite_graph[1].max() + 1
    perm = rng.permutation(hit.size)
    hit, col, score = hit[perm], col[perm], (score[perm] / 4096.0).astype(np.float32)
    hperm = rng.permutation(n)
    inv = np.argsort(hperm)
    pid, pt, hit = pid[hperm], pt[hperm], inv[hit]
    e = 6 * n
    edge_index = np.stack([rng.integers(0, n, e), rng.integers(0, n, e)])
    same = rng.random(e) < 0.3   # a share of true edges
    order = np.argsort(pid, kind="stable")
    nxt = np.empty(n, np.int64)
    nxt[order] = np.roll(order, -1)
    edge_index[1, same] = nxt[edge_index[0, same]]
    emb = rng.standard_normal((n, 8)).astype(np.float32) * 0.4
    return dict(pid=pid, pt=pt, graph=np.stack([hit, col]).astype(np.int64), scores=score,
                edge_index=edge_index.astype(np.int64), embeddings=emb)


SPECS = [
    ("plain", dict(n_particles=120, n_clusters=110)),
    ("noise", dict(n_particles=150, n_clusters=140, noise=0.15)),
    ("more_particles_than_clusters", dict(n_particles=260, n_clusters=70)),
    ("fewer_particles_than_clusters", dict(n_particles=50, n_clusters=220)),
    ("virtual_fallback", dict(n_particles=90, n_clusters=100, noise=0.05, shared_only_cluster=4)),
]
HPARAMS = {"weight_leak": 0.1, "ptcut": 1.0, "pt_interval": 0.5, "weight_min": 0.1, "log_weight_ratio": 0.4,
           "train_r": 0.9}


def certified_event(name, spec, base_seed):
    for attempt in range(200):
        rng = np.random.default_rng(base_seed + 1000 * attempt)
        ev = make_event(rng, **spec)
        uniq, pidx = np.unique(ev["pid"], return_inverse=True)
        n_rows, n_cols = uniq.size, int(ev["graph"][1].max()) + 1
        pr, pc, pw = R.contract(pidx[ev["graph"][0]], ev["graph"][1], ev["scores"], n_rows, n_cols)
        gap = (n_rows + n_cols) * 2.0 ** -SCALE_BITS
        ok, margin = R.certify_unique(pr, pc, pw, n_rows, n_cols, gap)
        if ok:
            return ev, margin, gap, attempt
    raise RuntimeError(f"{name}: no certified event in 200 seeds")


def main():
    ref = _import_reference()
    model = ref.BipartiteClassificationBase(HPARAMS)
    arrays, names = {}, []
    for idx, (name, spec) in enumerate(SPECS):
        ev, margin, gap, attempt = certified_event(name, spec, 20261016 + idx)
        batch = Event(pid=torch.from_numpy(ev["pid"]), pt=torch.from_numpy(ev["pt"].copy()))
        graph, scores = torch.from_numpy(ev["graph"]), torch.from_numpy(ev["scores"])
        ei, emb = torch.from_numpy(ev["edge_index"]), torch.from_numpy(ev["embeddings"])

        # get_bipartite_loss, and its locals through a traced copy of the same statements' results
        asgmt_loss = model.get_bipartite_loss(scores, graph, batch)
        # the matching, truth and weights: re-run the method's own statements through its helpers
        original_pid, pid = torch.unique(batch.pid, return_inverse=True)
        captured = {}
        orig_w = model.get_asgmt_weight

        def spy(batch_, pt_, bg_, y_, rm_, cm_):
            w = orig_w(batch_, pt_, bg_, y_, rm_, cm_)
            captured.update(truth=y_.clone(), row_match=rm_.clone(), col_match=cm_.clone(), weights=w.clone())
            return w

        model.get_asgmt_weight = spy
        again = model.get_bipartite_loss(scores, graph, batch)
        model.get_asgmt_weight = orig_w
        assert again.item() == asgmt_loss.item()

        y_pid = batch.pid[ei[0]] == batch.pid[ei[1]]
        w_emb = model.get_emb_weight(batch, ei, y_pid)
        hinge, dist = model.get_hinge_distance(batch, emb, ei, y_pid)
        emb_loss = torch.nn.functional.hinge_embedding_loss(dist / model.hparams["train_r"], hinge, margin=1,
                                                            reduction="none").square()
        emb_loss = torch.dot(emb_loss, w_emb)

        n_cols = int(graph[1].max()) + 1
        n_virtual = int(original_pid.numel()) - int(captured["row_match"].numel()) - int((original_pid == 0).any())
        names.append(name)
        arrays[f"{name}/pid"], arrays[f"{name}/pt"] = ev["pid"], ev["pt"]
        arrays[f"{name}/bipartite_graph"], arrays[f"{name}/scores"] = ev["graph"], ev["scores"]
        arrays[f"{name}/edge_index"], arrays[f"{name}/embeddings"] = ev["edge_index"], ev["embeddings"]
        arrays[f"{name}/row_match"] = captured["row_match"].numpy()
        arrays[f"{name}/col_match"] = captured["col_match"].numpy()
        arrays[f"{name}/truth"] = captured["truth"].numpy()
        arrays[f"{name}/weights"] = captured["weights"].numpy()
        arrays[f"{name}/asgmt_loss"] = np.array(asgmt_loss.item(), np.float64)
        arrays[f"{name}/emb_loss"] = np.array(emb_loss.item(), np.float64)
        arrays[f"{name}/unique_margin"] = np.array(margin, np.float64)
        arrays[f"{name}/gap_bound"] = np.array(gap, np.float64)
        print(f"{name:32s} P={original_pid.numel():4d} C={n_cols:4d} B={graph.shape[1]:5d} matched="
              f"{captured['row_match'].numel():4d} unmatched_signal~{n_virtual:3d} margin={margin:.3e} gap={gap:.2e} "
              f"seed_attempt={attempt} asgmt={asgmt_loss.item():.6f} emb={emb_loss.item():.6f}")
    arrays["cases"] = np.array(names)
    arrays["hparams"] = np.array([HPARAMS[k] for k in HP_KEYS], np.float64)
    arrays["hparam_keys"] = np.array(HP_KEYS)
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
