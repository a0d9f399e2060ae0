"""GPU: training_pairs (hierarchicalgnn_amd.embedding; csrc/trainpairs.hip), the row-local pair construction from
the kNN matrix, bit for bit (torch.equal / array_equal on both outputs, pair order included) against its numpy
restatement (tests/training_pairs_ref.py), against the existing composition
``training_samples(..., prediction_graph=<the expansion of the same idx>)`` on the device, and against the
reference's recorded outputs (tests/golden/embedding_samples.npz)."""
import numpy as np
import pytest
import torch

import training_pairs_ref as TP
from test_embedding_golden import Z

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

HP = dict(train_r=1.0, knn=100, weight_leak=1.0, weight_min=0.5, pt_interval=0.5, ptcut=1.0, log_weight_ratio=0.0)


def _dev_batch(mte, sm, pid):
    return {"modulewise_true_edges": torch.from_numpy(np.ascontiguousarray(mte)).to(DEV),
            "signal_mask": torch.from_numpy(np.ascontiguousarray(sm)).to(DEV),
            "pid": torch.from_numpy(np.ascontiguousarray(pid)).to(DEV)}


def _check(idx, mte, sm, pid, modes=TP.MODES):
    """training_pairs == the restatement == the composition, both modes; returns {mode: (graph, y)}"""
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import embedding
    batch = _dev_batch(mte, sm, pid)
    d_idx = torch.from_numpy(idx).to(DEV)
    pred = torch.from_numpy(TP.pairs_from_idx(idx)).to(DEV)
    out = {}
    for mode in modes:
        hp = dict(HP, true_edges=mode)
        reads = embedding.stats["host_reads"]
        g, y = H.training_pairs(d_idx, batch, hp)
        assert embedding.stats["host_reads"] == reads + 1
        assert g.dtype == torch.int64 and y.dtype == torch.bool and g.device == d_idx.device
        assert g.is_contiguous() and y.is_contiguous() and g.shape == (2, y.shape[0])
        rg, ry = TP.training_pairs(idx, mte, sm, pid, mode)
        assert np.array_equal(g.cpu().numpy(), rg) and np.array_equal(y.cpu().numpy(), ry), mode
        cg, cy = H.training_samples(d_idx, batch, hp, prediction_graph=pred)
        assert torch.equal(g, cg) and torch.equal(y, cy), mode
        out[mode] = (g, y)
    return out


@pytest.mark.parametrize("scatter", [False, True], ids=["tail", "scattered"])
def test_golden_fixture(scatter):
    n = Z["ev/pid"].shape[0]
    idx = TP.idx_from_pairs(Z["ev/pred"], n, scatter=np.random.default_rng(3) if scatter else None)
    out = _check(idx, Z["ev/modulewise_true_edges"], Z["ev/signal_mask"], Z["ev/pid"])
    for mode in TP.MODES:
        g, y = out[mode]
        assert np.array_equal(g.cpu().numpy(), Z[f"ts/{mode}/graph"])
        assert np.array_equal(y.cpu().numpy(), Z[f"ts/{mode}/y"])


def _grid_case(n, k):
    rng = np.random.default_rng(1000 * n + k)
    idx, kinds = TP.grid_idx(rng, n, k)
    pid = np.where(rng.random(n) < 0.25, 0, rng.integers(1, max(n // 4, 2), n)).astype(np.int64)   # noise: pid 0
    sm = rng.random(n) < 0.7
    mte = TP.random_truth(rng, idx, min(2 * n, 400))
    return idx, kinds, mte, sm, pid


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 100, 127, 128])
def test_shape_grid(k, n):
    idx, kinds, mte, sm, pid = _grid_case(n, k)
    _check(idx, mte, sm, pid)


@pytest.mark.parametrize("k", [100, 128])
def test_shape_grid_covers_the_row_kinds(k):
    """what the K = 100 and K = 128 cases of the grid hold at N = 1000"""
    idx, kinds, mte, sm, pid = _grid_case(1000, k)
    rows = np.arange(1000)
    assert (idx[kinds == "empty"] == -1).all() and (kinds == "empty").sum() > 100
    full = idx[kinds == "full"]
    assert (full >= 0).all() and all(np.unique(r).size == k for r in full)
    assert all(np.unique(r).size == 1 and r[0] >= 0 for r in idx[kinds == "copies"])
    holes = idx[kinds == "holes"]
    assert (holes[:, 0] == -1).any() and (holes[:, -1] >= 0).any() and (holes[:, k // 2] == -1).any()
    selfy = np.isin(kinds, ("self", "all_self")) & (idx == rows[:, None]).any(1)
    assert (selfy & (pid == 0)).any() and (selfy & (pid != 0) & sm).any() and (selfy & ~sm).any()
    # the modulewise membership test has hits, and both classes come out
    eb = TP.e_bidir(mte, sm)
    keys = lambda g: (g[0] << 31) | g[1]                                       # noqa: E731
    assert np.isin(keys(TP.pairs_from_idx(idx)), keys(eb)).any()


def _small(seed=2, n=200, k=100, t=120):
    rng = np.random.default_rng(seed)
    idx, _ = TP.grid_idx(rng, n, k)
    pid = rng.integers(0, 20, n).astype(np.int64)
    sm = rng.random(n) < 0.7
    return rng, idx, TP.random_truth(rng, idx, t), sm, pid


@pytest.mark.parametrize("case", ["t0", "all_masked", "dup_columns", "self_loops", "both_directions", "one_pid",
                                  "pid_zero", "all_signal"])
def test_truth_edge_cases(case):
    rng, idx, mte, sm, pid = _small()
    n = idx.shape[0]
    if case == "t0":
        mte = np.zeros((2, 0), np.int64)
    elif case == "all_masked":
        sm = np.zeros(n, bool)
    elif case == "dup_columns":
        mte = np.concatenate([mte, mte[:, ::2], mte[:, :5]], 1)
    elif case == "self_loops":
        mte = np.concatenate([mte, np.stack([np.arange(0, n, 3)] * 2)], 1)
    elif case == "both_directions":
        mte = np.concatenate([mte, mte[::-1]], 1)
    elif case == "one_pid":
        pid = np.full(n, 5, np.int64)
    elif case == "pid_zero":
        pid = np.zeros(n, np.int64)
    elif case == "all_signal":
        sm = np.ones(n, bool)
    out = _check(idx, mte, sm, pid)
    y = out["modulewise_true_edges"][1]
    if case in ("t0", "all_masked"):
        assert not bool(y.any())
    else:
        assert int(y.sum()) == TP.e_bidir(mte, sm).shape[1] > 0
    if case == "one_pid":
        assert not bool((~y).any())                                            # no fake pair survives the pid test
    assert not bool(out["pid_true_edges"][1].any())


@pytest.mark.parametrize("mode", TP.MODES)
def test_knn_event_through_training_samples_fused(mode):
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import embedding, synth
    from hierarchicalgnn_amd.ops import knn_radius
    ev = synth.embedding_event(20_000, seed=5)
    batch = {k: v.to(DEV) for k, v in ev.items()}
    emb = batch["embeddings"]
    hp = dict(HP, true_edges=mode)
    reads = embedding.stats["host_reads"]
    g, y = H.training_samples(emb, batch, hp, fused=True)
    assert embedding.stats["host_reads"] == reads + 1
    g2, y2 = H.training_samples(emb, batch, hp)                                # today's route
    assert torch.equal(g, g2) and torch.equal(y, y2) and g.is_contiguous()
    idx = knn_radius(emb, emb, 100, 1.0)
    rg, ry = TP.training_pairs(idx.cpu().numpy(), ev["modulewise_true_edges"].numpy(), ev["signal_mask"].numpy(),
                               ev["pid"].numpy(), mode)
    assert np.array_equal(g.cpu().numpy(), rg) and np.array_equal(y.cpu().numpy(), ry)
    if mode == "modulewise_true_edges":
        assert bool(y.any()) and bool((~y).any())
    gs, ys = H.training_samples(emb, batch, dict(hp, knn_method="sorted"), fused=True)
    assert torch.equal(gs, g) and torch.equal(ys, y)
    with pytest.raises(ValueError, match="prediction_graph"):
        H.training_samples(emb, batch, hp, prediction_graph=g, fused=True)


def test_empty_inputs():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import embedding
    empty = _dev_batch(np.zeros((2, 0), np.int64), np.zeros(0, bool), np.zeros(0, np.int64))
    for mode in TP.MODES:
        reads = embedding.stats["host_reads"]
        g, y = H.training_pairs(torch.zeros((0, 100), dtype=torch.int64, device=DEV), empty, dict(HP, true_edges=mode))
        assert g.shape == (2, 0) and y.shape == (0,) and g.dtype == torch.int64 and y.dtype == torch.bool
        assert g.is_cuda and embedding.stats["host_reads"] == reads            # nothing launched, nothing read
        # rows without a valid slot and no truth: an empty result out of the kernels
        batch = _dev_batch(np.zeros((2, 0), np.int64), np.ones(5, bool), np.arange(5))
        g, y = H.training_pairs(torch.full((5, 3), -1, dtype=torch.int64, device=DEV), batch, dict(HP, true_edges=mode))
        assert g.shape == (2, 0) and y.shape == (0,)
    with pytest.raises(ValueError, match="modulewise_true_edges"):
        H.training_pairs(torch.zeros((0, 4), dtype=torch.int64, device=DEV),
                         dict(empty, modulewise_true_edges=torch.zeros((2, 1), dtype=torch.int64, device=DEV)),
                         dict(HP, true_edges="pid_true_edges"))


def test_one_host_read_contiguous_and_repeatable():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import embedding
    rng, idx, mte, sm, pid = _small(seed=9, n=3000, k=128, t=2000)
    batch, d_idx = _dev_batch(mte, sm, pid), torch.from_numpy(idx).to(DEV)
    # a non-contiguous view of the kNN matrix is accepted
    wide = torch.full((3000, 130), -7, dtype=torch.int64, device=DEV)
    wide[:, 1:129] = d_idx
    for mode in TP.MODES:
        hp = dict(HP, true_edges=mode)
        reads = embedding.stats["host_reads"]
        a = H.training_pairs(d_idx, batch, hp)
        assert embedding.stats["host_reads"] == reads + 1
        b = H.training_pairs(d_idx, batch, hp)
        c = H.training_pairs(wide[:, 1:129], batch, hp)
        assert embedding.stats["host_reads"] == reads + 3
        for g, y in (a, b, c):
            assert g.is_contiguous() and y.is_contiguous() and g.shape[1] == y.shape[0] > 0
            assert torch.equal(g, a[0]) and torch.equal(y, a[1])


@pytest.mark.parametrize("mode", TP.MODES)
@pytest.mark.parametrize("bad", ["idx_n", "idx_minus_2", "mte_n"])
def test_bad_ids_raise_and_are_skipped(bad, mode):
    """ValueError from the public call, no fault; and through the same two launches without the status check, the
    rest of the call equals the restatement with the bad slot treated as empty / the bad column dropped"""
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import _lib, embedding
    rng, idx, mte, sm, pid = _small(seed=4, n=130, k=65, t=60)
    n = idx.shape[0]
    if bad == "idx_n":
        idx[7, 64], idx[100, 3] = n, n + 12345
        bit, word = _lib.TP_ST_BAD_IDX, "knn_idx"
    elif bad == "idx_minus_2":
        idx[8, 0], idx[129, 64] = -2, -(1 << 40)
        bit, word = _lib.TP_ST_BAD_IDX, "knn_idx"
    else:
        mte[0, 5], mte[1, 17] = n, -1
        bit, word = _lib.TP_ST_BAD_MTE, "modulewise_true_edges"
    batch, d_idx = _dev_batch(mte, sm, pid), torch.from_numpy(idx).to(DEV)
    with pytest.raises(ValueError, match=word):
        H.training_pairs(d_idx, batch, dict(HP, true_edges=mode))
    g, y, info = embedding._tp_launch(d_idx, batch["modulewise_true_edges"], batch["signal_mask"].view(torch.uint8),
                                      batch["pid"], embedding._TP_MODES[mode], check=False)
    torch.cuda.synchronize()
    assert info[_lib.TP_STATUS] == bit
    rg, ry = TP.training_pairs(idx, mte, sm, pid, mode, skip_bad=True)
    assert np.array_equal(g.cpu().numpy(), rg) and np.array_equal(y.cpu().numpy(), ry)
    assert info[_lib.TP_P] == rg.shape[1] and info[_lib.TP_N_TRUTH] == int(ry.sum())
    assert info[_lib.TP_N_ROW] + info[_lib.TP_N_TRUTH] == info[_lib.TP_P]


@pytest.mark.parametrize("mode", TP.MODES)
def test_training_losses_fused_samples_are_bit_equal(mode):
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import synth
    ev = synth.embedding_event(2000, seed=8)
    batch = {k: v.to(DEV) for k, v in ev.items()}
    g = torch.Generator().manual_seed(1)
    ei = torch.randint(0, 2000, (2, 6000), generator=g)
    batch["edge_index"] = ei.to(DEV)
    hp = dict(HP, true_edges=mode)
    inter = torch.nn.functional.normalize(torch.randn(2000, 8, generator=g), dim=1).to(DEV)

    def run(fused, hgnn):
        emb = batch["embeddings"].clone().requires_grad_(True)
        if hgnn:
            loss, emb_loss, inter_loss = H.embedding_hgnn_training_loss(emb, inter, batch, hp, 0.25,
                                                                        fused_samples=fused)
        else:
            loss = H.embedding_in_training_loss(emb, batch, hp, fused_samples=fused)
        loss.backward()
        return loss.detach(), emb.grad

    a = H.training_samples(batch["embeddings"], batch, hp)
    b = H.training_samples(batch["embeddings"], batch, hp, fused=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].shape[1] > 0
    for hgnn in (False, True):
        l0, g0 = run(False, hgnn)
        l1, g1 = run(True, hgnn)
        assert torch.isfinite(l0) and torch.equal(l0, l1) and torch.equal(g0, g1)
        assert bool(g0.any())
    H.pair_hinge_check(DEV)
