#!/usr/bin/env python3
"""Generate tests/golden/ec_loss.npz by RUNNING the reference's own EdgeClassifierBase.training_step on the CPU.

Run in the build container only (it needs the reference checkout, which never travels to the GPU box):

    python tests/golden/make_ec_loss_golden.py

The reference module imports pytorch_lightning, torch_geometric, cupy, cugraph and cudf, none of which exist here, and
its own ``utils`` / ``tracking_utils``.  Stand-ins, in the style of make_assignment_golden.py:
  * pytorch_lightning.LightningModule: a torch.nn.Module with ``save_hyperparameters`` (stores ``hparams``), a
    ``device`` of "cpu" and a ``log`` that does nothing.
  * torch_geometric.data: empty DataLoader / Data names; cupy, cugraph, cudf: empty modules (training_step calls none).
  * utils / tracking_utils: modules that only carry the imported names.
The model is a subclass whose ``forward`` returns the stored scores as a leaf that requires grad, so ``training_step``
(:113-132) runs word for word: the neutral-edge cut, get_training_weight, binary_cross_entropy and the dot product.

One event: 300 hits, 4000 edges; pt with NaNs and zeros; y (modulewise truth) a subset of y_pid (PID truth), so the
modulewise mode has neutral edges to drop; scores sigmoid(3 * normal), strictly inside (0, 1) so that no element of
the gradient dwarfs the others (the clamps are the GPU test's random cases' business).
Cases: both ``true_edges`` modes x log_weight_ratio in {0, 0.6}.  Stored: the inputs and, per case, the loss,
dloss/dscores over ALL edges and get_training_weight's output (over the edges the mode keeps).  The file is written
with fixed zip timestamps, so re-running reproduces it bit for bit.
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
REF = os.environ.get("HGNN_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "ec_loss.npz")
HP_KEYS = ("weight_leak", "ptcut", "pt_interval", "weight_min")
HPARAMS = {"weight_leak": 0.1, "ptcut": 1.0, "pt_interval": 0.5, "weight_min": 0.1}
MODES = ("modulewise_true_edges", "pid_true_edges")
LWRS = (0.0, 0.6)


def _install_stubs():
    pl = types.ModuleType("pytorch_lightning")

    class LightningModule(torch.nn.Module):
        device = "cpu"

        def save_hyperparameters(self, hparams):
            self.hparams = dict(hparams)

        def log(self, *args, **kwargs):
            pass

    pl.LightningModule = LightningModule
    sys.modules["pytorch_lightning"] = pl
    tg, tgd = types.ModuleType("torch_geometric"), types.ModuleType("torch_geometric.data")
    tgd.DataLoader = tgd.Data = None
    tg.data = tgd
    sys.modules["torch_geometric"], sys.modules["torch_geometric.data"] = tg, tgd
    for name in ("cupy", "cugraph", "cudf"):
        sys.modules[name] = types.ModuleType(name)
    ut = types.ModuleType("utils")
    ut.TrackMLDataset = ut.load_dataset_paths = None
    sys.modules["utils"] = ut
    tu = types.ModuleType("tracking_utils")
    tu.eval_metrics = None
    sys.modules["tracking_utils"] = tu


def _import_reference():
    _install_stubs()
    sys.path.insert(0, os.path.join(REF, "Modules", "EdgeClassifier"))
    import edge_classifier_base as b
    return b


class Event(dict):
    __getattr__ = dict.__getitem__


def make_event(rng, n=300, e=4000):
    pid = rng.integers(0, 60, n)                       # 0 = noise
    edge_index = rng.integers(0, n, (2, e))
    edge_index[:, :100] = edge_index[:, 100:200]       # duplicate edges
    edge_index[1, 200:230] = edge_index[0, 200:230]    # self edges
    y_pid = (pid[edge_index[0]] == pid[edge_index[1]]) & (pid[edge_index[0]] != 0)
    flip = rng.random(e) < 0.25                        # a larger share of PID-true edges
    y_pid = y_pid | flip
    y = y_pid & (rng.random(e) < 0.7)                  # modulewise truth: a subset; the rest of y_pid is neutral
    pt = rng.exponential(1.0, n).astype(np.float32)
    pt[::13] = np.nan
    pt[5::17] = 0.0
    scores = (1.0 / (1.0 + np.exp(-3.0 * rng.standard_normal(e)))).astype(np.float32)
    return dict(edge_index=edge_index.astype(np.int64), y=y, y_pid=y_pid, pt=pt, scores=scores)


def main():
    ref = _import_reference()

    class Stored(ref.EdgeClassifierBase):
        def forward(self, x, edge_index):
            return self.leaf

    ev = make_event(np.random.default_rng(20261017))
    arrays = {f"ev/{k}": v for k, v in ev.items()}
    for mode in MODES:
        for lwr in LWRS:
            model = Stored(dict(HPARAMS, true_edges=mode, log_weight_ratio=lwr))
            model.leaf = torch.from_numpy(ev["scores"].copy()).requires_grad_(True)
            batch = Event(x=None, edge_index=torch.from_numpy(ev["edge_index"]), y=torch.from_numpy(ev["y"]),
                          y_pid=torch.from_numpy(ev["y_pid"]), pt=torch.from_numpy(ev["pt"].copy()))
            captured = {}
            orig = model.get_training_weight

            def spy(batch_, graph_, y_, orig=orig, captured=captured):
                w = orig(batch_, graph_, y_)
                captured["weights"] = w.clone()
                return w

            model.get_training_weight = spy
            loss = model.training_step(batch, 0)
            loss.backward()
            key = f"{mode}/lwr{lwr:g}"
            arrays[f"{key}/loss"] = np.array(loss.item(), np.float64)
            arrays[f"{key}/grad"] = model.leaf.grad.numpy().copy()
            arrays[f"{key}/weights"] = captured["weights"].detach().numpy().copy()
            print(f"{key:36s} kept={captured['weights'].numel():5d} loss={loss.item():.9g} "
                  f"|grad|max={np.abs(arrays[f'{key}/grad']).max():.4g}")
    arrays["modes"] = np.array(MODES)
    arrays["log_weight_ratios"] = np.array(LWRS, np.float64)
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
