"""GPU: the fused weighted pair hinge loss (hierarchicalgnn_amd.pair_hinge_loss; csrc/pairloss.hip) against the
float64 restatement (tests/pairloss_ref.py), the reference fixture and the existing torch composition."""
import numpy as np
import pytest
import torch

import conftest
import pairloss_ref as PR
from test_embedding_golden import MODES, Z

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

HP = dict(train_r=1.0, knn=100, weight_leak=1.0, weight_min=0.5, pt_interval=0.5, ptcut=1.0, log_weight_ratio=0.0)


def _fused(emb, graph, y, pt, hp, **kw):
    """(loss tensor, grad tensor) of one fused call on fresh leaves"""
    import hierarchicalgnn_amd as H
    e = torch.as_tensor(emb, dtype=torch.float32).to(DEV).requires_grad_(True)
    g = torch.as_tensor(graph).to(DEV)
    yy = torch.as_tensor(y).to(DEV)
    batch = {"pt": torch.as_tensor(pt, dtype=torch.float32).to(DEV)}
    loss = H.pair_hinge_loss(e, g, yy, batch, hp, **kw)
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    return loss.detach(), e.grad


def _check(emb, graph, y, pt, hp, margin=None, scale=1.0):
    emb32 = np.asarray(emb, np.float32)
    loss, grad = _fused(emb32, graph, y, pt, hp, margin=margin, scale=scale)
    r_loss, r_grad, _, _ = PR.pair_hinge(emb32, graph, y, pt, hp, margin=margin, scale=scale)
    err = abs(float(loss) - r_loss) / max(abs(r_loss), 1e-30)
    print(f"pair hinge: P={np.asarray(graph).shape[1]} loss {float(loss):.9g} ref {r_loss:.9g} rel_err {err:.3g} "
          f"grad normwise {conftest.rel_err(grad.cpu().numpy(), r_grad):.3g} "
          f"element-wise {conftest.elem_err(grad.cpu().numpy(), r_grad):.3g}")
    assert err <= 1e-6
    conftest.assert_parity(grad, r_grad, what="grad_E")
    return loss, grad


def _random_case(seed, n, p, dim, idt):
    rng = np.random.default_rng(seed)
    emb = rng.normal(size=(n, dim)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    graph = rng.integers(0, n, (2, p))
    q = p // 20
    graph[:, :q] = graph[:, q:2 * q]                   # duplicate pairs
    graph[1, 2 * q:3 * q] = graph[0, 2 * q:3 * q]      # self pairs
    y = rng.random(p) < 0.3
    pt = rng.exponential(1.0, n).astype(np.float32)
    pt[::13] = np.nan
    return emb, graph.astype(idt), y, pt


@pytest.mark.parametrize("mode", MODES)
def test_matches_restatement_and_reference_on_the_fixture(mode):
    g, y = Z[f"ts/{mode}/graph"], Z[f"ts/{mode}/y"]
    loss, _ = _check(Z["ev/embeddings"], g, y, Z["ev/pt"], HP)
    assert conftest.rel_err(loss.cpu().numpy().reshape(1), Z[f"ts/{mode}/loss"].reshape(1)) <= 1e-6


@pytest.mark.parametrize("idt", [np.int64, np.int32])
@pytest.mark.parametrize("dim", [1, 3, 8, 16])
def test_random_cases_vs_restatement(dim, idt):
    emb, graph, y, pt = _random_case(dim, 5000, 200_003 if dim == 3 else 200_000, dim, idt)
    hp = dict(HP, log_weight_ratio=0.7, train_r=0.8)
    _check(emb, graph, y, pt, hp)                                          # the embedding stage: scale 1, margin r
    _check(emb, graph, y, pt, hp, margin=1.0, scale=1.0 / hp["train_r"])   # bc_embedding_loss


def test_empty_pair_list_and_empty_class():
    emb, graph, y, pt = _random_case(1, 100, 1000, 8, np.int64)
    loss, grad = _fused(emb, np.zeros((2, 0), np.int64), np.zeros(0, bool), pt, HP)
    assert float(loss) == 0.0 and not bool(grad.any())
    for cls in (np.zeros(1000, bool), np.ones(1000, bool)):
        loss, grad = _check(emb, graph, cls, pt, HP)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())


def _loss64(e, graph, y, pt_t):
    """the forward entry point's float64 loss (state[HGNN_PH_LOSS]): what the float32 result is rounded from"""
    from hierarchicalgnn_amd import embedding as E, _lib
    g_t = torch.from_numpy(np.ascontiguousarray(graph)).to(DEV)
    y_t = torch.from_numpy(np.ascontiguousarray(y)).to(DEV).view(torch.uint8)
    loss = torch.empty(1, device=DEV)
    state = torch.empty(_lib.PH_STATE, dtype=torch.float64, device=DEV)
    status = torch.empty(1, dtype=torch.int32, device=DEV)
    ws, nb = _lib.workspace("hgnn_pair_hinge_workspace_bytes", e.device, g_t.shape[1], e.shape[0], e.shape[1], 0)
    _lib.check(_lib.load().hgnn_pair_hinge_forward(
        _lib.ptr(e), e.shape[0], e.shape[1], _lib.ptr(g_t), _lib.DT_I64, _lib.ptr(y_t), _lib.ptr(pt_t), g_t.shape[1],
        E._ph_scalars(HP, None, 1.0), _lib.ptr(loss), _lib.ptr(state), _lib.ptr(status), _lib.ptr(ws), nb,
        _lib.current_stream(e.device)), "hgnn_pair_hinge_forward")
    assert int(status) == 0 and float(loss) == float(state[_lib.PH_LOSS].float())
    return float(state[_lib.PH_LOSS])


def test_bitwise_reproducible_and_permutation_insensitive():
    emb, graph, y, pt = _random_case(2, 20_000, 1_000_000, 8, np.int64)
    l1, g1 = _fused(emb, graph, y, pt, HP)
    l2, g2 = _fused(emb, graph, y, pt, HP)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    perm = np.random.default_rng(0).permutation(graph.shape[1])
    e, pt_t = torch.from_numpy(emb).to(DEV), torch.from_numpy(pt).to(DEV)
    a = _loss64(e, graph, y, pt_t)
    b = _loss64(e, graph[:, perm], y[perm], pt_t)
    print(f"float64 loss, two pair orders: {a!r} {b!r} rel {abs(a - b) / abs(a):.3g}")
    assert abs(a - b) <= 1e-12 * abs(a)
    assert a == _loss64(e, graph, y, pt_t)


def test_no_host_read_and_sync_debug_mode():
    import hierarchicalgnn_amd as H
    emb, graph, y, pt = _random_case(3, 5000, 100_000, 8, np.int64)
    e = torch.from_numpy(emb).to(DEV).requires_grad_(True)
    g, yy = torch.from_numpy(graph).to(DEV), torch.from_numpy(y).to(DEV)
    batch = {"pt": torch.from_numpy(pt).to(DEV)}
    pt0 = batch["pt"].clone()
    H.pair_hinge_loss(e, g, yy, batch, HP).backward()              # warm-up: code objects, allocator
    torch.cuda.synchronize()
    reads = H.embedding.stats["host_reads"]
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = H.pair_hinge_loss(e, g, yy, batch, HP)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert H.embedding.stats["host_reads"] == reads
    assert bool(torch.isfinite(loss))
    assert torch.equal(batch["pt"].isnan(), pt0.isnan()) and torch.equal(batch["pt"].nan_to_num(), pt0.nan_to_num())
    H.pair_hinge_check()
    assert H.embedding.stats["host_reads"] == reads + 1            # the explicit check is the one read


@pytest.mark.parametrize("bad", [-1, 5000, 1 << 40])
def test_out_of_range_id_is_reported_not_faulted(bad):
    import hierarchicalgnn_amd as H
    emb, graph, y, pt = _random_case(4, 5000, 10_000, 8, np.int64)
    graph[1, 777] = bad
    e = torch.from_numpy(emb).to(DEV).requires_grad_(True)
    batch = {"pt": torch.from_numpy(pt).to(DEV)}
    g, yy = torch.from_numpy(graph).to(DEV), torch.from_numpy(y).to(DEV)
    with pytest.raises(ValueError, match="pair id"):
        H.pair_hinge_loss(e, g, yy, batch, HP, check=True)
    loss = H.pair_hinge_loss(e, g, yy, batch, HP)                  # lazily: the next check reports it
    loss.backward()
    assert bool(torch.isfinite(e.grad).all())
    with pytest.raises(ValueError, match="pair id"):
        H.pair_hinge_check()
    H.pair_hinge_check()                                           # cleared


def test_cpu_tensors_and_bad_shapes_are_refused():
    import hierarchicalgnn_amd as H
    emb, graph, y, pt = _random_case(5, 100, 500, 8, np.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.pair_hinge_loss(torch.from_numpy(emb), torch.from_numpy(graph), torch.from_numpy(y),
                          {"pt": torch.from_numpy(pt)}, HP)
    wide = torch.zeros(100, 17, device=DEV)
    with pytest.raises(ValueError, match="D <= 16"):
        H.pair_hinge_loss(wide, torch.from_numpy(graph).to(DEV), torch.from_numpy(y).to(DEV),
                          {"pt": torch.from_numpy(pt).to(DEV)}, HP)


@pytest.mark.parametrize("lwr", [0.0, -0.4])
def test_equals_the_existing_torch_composition(lwr):
    import hierarchicalgnn_amd as H
    emb, graph, y, pt = _random_case(6, 5000, 300_000, 8, np.int64)
    hp = dict(HP, log_weight_ratio=lwr, train_r=0.9)
    e = torch.from_numpy(emb).to(DEV)
    g, yy = torch.from_numpy(graph).to(DEV), torch.from_numpy(y).to(DEV)
    batch = {"pt": torch.from_numpy(pt).to(DEV)}
    w = H.training_weights(batch, g, yy, hp)
    hinge, dist = H.hinge_distance(e, g, yy)
    ref = torch.dot(torch.nn.functional.hinge_embedding_loss(dist, hinge, margin=hp["train_r"],
                                                             reduction="none").square(), w)
    got = H.pair_hinge_loss(e, g, yy, batch, hp)
    assert abs(float(got) - float(ref)) <= 1e-6 * abs(float(ref))


def test_bc_embedding_loss_fused_switch():
    import hierarchicalgnn_amd as H
    emb, graph, y, pt = _random_case(7, 5000, 200_000, 8, np.int64)
    rng = np.random.default_rng(7)
    e = torch.from_numpy(emb).to(DEV)
    g = torch.from_numpy(graph).to(DEV)
    batch = {"pt": torch.from_numpy(pt).to(DEV), "pid": torch.from_numpy(rng.integers(0, 40, 5000)).to(DEV)}
    hp = dict(HP, train_r=0.8)
    a = H.bc_embedding_loss(e, g, batch, hp)
    b = H.bc_embedding_loss(e, g, batch, hp, fused=True)
    assert abs(float(a) - float(b)) <= 1e-6 * abs(float(a))
