"""GPU: the fused optimiser step (hierarchicalgnn_amd.FusedAdamW; csrc/optim.hip, k_opt_*) against the float64
restatement (tests/optim_ref.py) and against clip_grad_norm_ + torch.optim.AdamW on the same device.

Bars (optim_ref.BAR_*; tests/test_optim_ref.py holds torch's own float32 arithmetic to HALF of each on these inputs):
p_T - p_0 at conftest.assert_parity's 1e-4, normwise and element-wise (torch float32: 2.8e-5 / 4.6e-5); exp_avg,
exp_avg_sq and max_exp_avg_sq at 1e-5 (torch: 1.9e-6); the total norm at 5e-6 relative (torch: 9.2e-7).
"""
import copy
import functools
import types

import numpy as np
import pytest
import torch

import conftest
import optim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATE_KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")


@functools.lru_cache(maxsize=None)
def _case(gscale):
    return R.Case(gscale)


@functools.lru_cache(maxsize=None)
def _ref(gscale, amsgrad, max_norm):
    return R.run(_case(gscale), amsgrad=amsgrad, max_norm=max_norm)


def _params(case):
    """the case's parameters on the device; the last one is ``base[1:258]``: contiguous, on a 4-byte-misaligned
    address"""
    out = []
    for i, a in enumerate(case.params):
        t = torch.tensor(a, device=DEV)
        if i == getattr(case, "misaligned", -1):
            base = torch.zeros(260, device=DEV)
            base[1:258] = t
            t = base[1:258]
            assert t.is_contiguous() and t.data_ptr() % 16 == 4
        out.append(torch.nn.Parameter(t))
    return out


def _set_grads(params, grads):
    for q, g in zip(params, grads):
        q.grad = None if g is None else torch.tensor(g, device=DEV)


def _fused_run(case, amsgrad=True, max_norm=R.MAX_NORM, steps=R.STEPS, lrs=R.LRS, sync=False, scalar=False, **kw):
    """(optimizer, params, result in optim_ref's layout) of ``steps`` FusedAdamW steps; the norms are read at the end"""
    import hierarchicalgnn_amd as H
    params = _params(case)
    opt = H.FusedAdamW(params, lr=lrs[0], amsgrad=amsgrad, max_grad_norm=max_norm, **kw)
    norms = []
    for t in range(steps):
        for pg in opt.param_groups:
            pg["lr"] = lrs[t]
        _set_grads(params, case.grads[t])
        opt.step(_scalar_path=scalar) if scalar else opt.step()
        if max_norm is not None:
            norms.append(opt.last_grad_norm.clone())
        if sync:
            torch.cuda.synchronize()
    return opt, params, R.torch_result(opt, params, [float(n) for n in norms])


def _assert_bars(got, ref, case, amsgrad, what):
    e = R.errors(got, ref, case, amsgrad)
    print(f"{what}: {e}")
    assert R.within_bars(e), (what, e)


def _assert_parity(got, ref, case, amsgrad, what):
    """every tensor of p_T - p_0 and of the state at conftest.assert_parity's default"""
    for i, p0 in enumerate(case.params):
        conftest.assert_parity(got["p"][i] - p0, ref["p"][i] - p0, what=f"{what}: p[{i}] - p0")
        for k in STATE_KEYS[:3 if amsgrad else 2]:
            conftest.assert_parity(got[k][i], ref[k][i], what=f"{what}: {k}[{i}]")


def _bitwise(a, b, amsgrad=True):
    return all(np.array_equal(x, y, equal_nan=True) for k in ("p",) + STATE_KEYS[:3 if amsgrad else 2]
               for x, y in zip(a[k], b[k])) and a["norms"] == b["norms"] and a["step"] == b["step"]


# ---- parity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [R.MAX_NORM, None])
@pytest.mark.parametrize("amsgrad", [True, False])
@pytest.mark.parametrize("gscale", R.GSCALES)
def test_five_steps_equal_the_restatement_and_torch(gscale, amsgrad, max_norm):
    """the test parameter set (sizes 1 .. 131072, a 2-D, an empty and a misaligned tensor, one gradient absent on step
    2, a changing lr) against the float64 restatement at the bars, and against the torch composition on the device"""
    case = _case(gscale)
    opt, params, got = _fused_run(case, amsgrad, max_norm)
    ref = _ref(gscale, amsgrad, max_norm)
    assert got["step"] == ref["step"] and got["step"][case.absent] == R.STEPS - 1
    assert set(opt.state[params[0]]) == {"step"} | set(STATE_KEYS[:3 if amsgrad else 2])
    _assert_bars(got, ref, case, amsgrad, f"gscale {gscale:g} amsgrad {amsgrad} max_norm {max_norm}")
    tor = R.torch_run(case, torch.float32, device=DEV, amsgrad=amsgrad, max_norm=max_norm,
                      make_params=lambda: _params(case))
    _assert_parity(got, tor, case, amsgrad, "against torch")
    assert (opt.last_grad_norm is None) == (max_norm is None)
    opt.check()


@pytest.mark.parametrize("amsgrad", [True, False])
def test_the_element_wise_path_gives_the_bits_of_the_16_byte_path(amsgrad):
    case = _case(1e-2)
    _, _, vec = _fused_run(case, amsgrad, steps=2)
    _, _, sca = _fused_run(case, amsgrad, steps=2, scalar=True)
    assert _bitwise(vec, sca, amsgrad)


def test_two_parameter_groups_in_one_call():
    """different lr and weight decay per group: one table, one launch sequence"""
    import hierarchicalgnn_amd as H
    case = _case(1e-2)
    half = len(case.params) // 2
    groups = lambda ps: [dict(params=ps[:half], lr=1e-3, weight_decay=0.0),             # noqa: E731
                         dict(params=ps[half:], lr=2e-3, weight_decay=0.1)]
    params, t_params = _params(case), _params(case)
    opt = H.FusedAdamW(groups(params), lr=1.0, max_grad_norm=R.MAX_NORM)
    tor = torch.optim.AdamW(groups(t_params), lr=1.0, amsgrad=True)
    n0 = H.optim.stats["launches"]
    for t in range(3):
        _set_grads(params, case.grads[t])
        _set_grads(t_params, case.grads[t])
        opt.step()
        torch.nn.utils.clip_grad_norm_(t_params, R.MAX_NORM)
        tor.step()
    assert H.optim.stats["launches"] == n0 + 3 * 3
    _assert_parity(R.torch_result(opt, params), R.torch_result(tor, t_params), case, True, "two groups")
    # and each half against the restatement run with its own group's settings
    a = R.run(case, lrs=[1e-3] * 3, weight_decay=0.0, steps=3)
    b = R.run(case, lrs=[2e-3] * 3, weight_decay=0.1, steps=3)
    ref = {k: a[k][:half] + b[k][half:] for k in ("p",) + STATE_KEYS}
    ref["norms"] = []
    got = R.torch_result(opt, params)
    _assert_bars(got, ref, case, True, "two groups against the restatement")


def test_more_chunks_than_workgroups():
    """one tensor of 2049 * 4096 + 777 = 8 393 481 elements, that is 2050 chunks of HGNN_OPT_CHUNK = 4096 elements, and a
    5-element tensor behind it: 2051 chunks for a grid capped at 2048 workgroups.  Workgroups 0, 1 and 2 take a second
    chunk: a whole one, the partial tail of the large tensor, and the small tensor.

    Two steps.  The state and the norm are held to the bars above.  The parameters here are normal * 0.1 and move by
    about sum(lr) = 8e-4, so p_T - p_0 is mostly the rounding of p and the 1e-4 bar on it does not apply; p_T itself
    is held to what float32 allows: per step the factor 1 - lr wd is itself rounded to float32 (2^-25 below 1), the
    product and the subtraction are rounded (2^-24 each), 2.5 * 2^-24 |p| = 1.5e-7 |p| in all, and the update, at most
    about lr in size, carries the relative error of m / denom, below 2e-6 by the state bar.  A chunk that was skipped, done twice or mapped to the wrong place is off by 8e-4, a thousand times more."""
    from hierarchicalgnn_amd import _lib
    n = 2049 * _lib.OPT_CHUNK + 777
    rng = np.random.default_rng(7)
    case = types.SimpleNamespace(
        params=[(rng.standard_normal(n) * 0.1).astype(np.float32), rng.standard_normal(5).astype(np.float32)],
        grads=[[(rng.standard_normal(n) * 1e-2).astype(np.float32), rng.standard_normal(5).astype(np.float32)]
               for _ in range(2)])
    _, _, got = _fused_run(case, steps=2)
    ref = R.run(case, steps=2)
    e = R.errors(got, ref, case)
    print(f"2051 chunks: {e}")
    assert e["state"] <= R.BAR_STATE and e["norm"] <= R.BAR_NORM
    for a, b in zip(got["p"], ref["p"]):
        excess = np.abs(a - b) - (2 * 1.5e-7 * np.abs(b) + 2e-6 * sum(R.LRS[:2]))
        print(f"2051 chunks: p_T off by at most {np.abs(a - b).max():.3g}, {excess.max():.3g} above the bound")
        assert excess.max() <= 0.0
    tor = R.torch_run(case, torch.float32, device=DEV, steps=2)
    for i in range(2):
        conftest.assert_parity(got["p"][i], tor["p"][i], what=f"p[{i}] against torch")
        for k in STATE_KEYS:
            conftest.assert_parity(got[k][i], tor[k][i], what=f"{k}[{i}] against torch")


# ---- ordering and reproducibility ---------------------------------------------------------------------------------
def test_back_to_back_steps_need_no_synchronisation():
    """three steps queued without a synchronisation between them, the gradients re-allocated in between
    (zero_grad(set_to_none=True)), equal bit for bit the same steps with a synchronize() after each: neither the
    staged table nor the device copy of one step is overwritten before its kernels have read it"""
    import hierarchicalgnn_amd as H
    case = _case(1e-2)
    dev_grads = [[None if g is None else torch.tensor(g, device=DEV) for g in step] for step in case.grads[:3]]

    def run(sync):
        params = _params(case)
        opt = H.FusedAdamW(params, lr=1e-3, max_grad_norm=R.MAX_NORM)
        norms = []
        torch.cuda.synchronize()
        for t in range(3):
            opt.zero_grad(set_to_none=True)
            for q, g in zip(params, dev_grads[t]):
                q.grad = None if g is None else g.clone()
            opt.step()
            norms.append(opt.last_grad_norm.clone())
            if sync:
                torch.cuda.synchronize()
        return R.torch_result(opt, params, [float(x) for x in norms])

    assert _bitwise(run(False), run(True))


def test_two_fresh_runs_give_the_same_bits():
    case = _case(1.0)
    _, _, a = _fused_run(case)
    _, _, b = _fused_run(case)
    assert _bitwise(a, b) and len(a["norms"]) == R.STEPS


# ---- the gradients afterwards -------------------------------------------------------------------------------------
def test_zero_grads_and_the_written_back_clip():
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import _lib
    case = _case(1.0)
    plain_opt, _, plain = _fused_run(case, steps=1)
    params = _params(case)
    opt = H.FusedAdamW(params, lr=R.LRS[0], max_grad_norm=R.MAX_NORM, zero_grads=True)
    _set_grads(params, case.grads[0])
    grads = [q.grad for q in params]
    ptrs = [g.data_ptr() for g in grads]
    opt.step()
    opt.zero_grad()                                   # a no-op: nothing is set to None
    assert all(q.grad is g and g.data_ptr() == a for q, g, a in zip(params, grads, ptrs))
    assert all(not g.any() for g in grads)
    assert _bitwise(R.torch_result(opt, params), dict(plain, norms=[]))
    # write_clipped_grads: g * coef, the product torch's in-place clip leaves, bit for bit
    params = _params(case)
    opt = H.FusedAdamW(params, lr=R.LRS[0], max_grad_norm=R.MAX_NORM, write_clipped_grads=True)
    _set_grads(params, case.grads[0])
    opt.step()
    coef = opt._opt_state[_lib.OPT_COEF].float()
    want = np.float32(R.MAX_NORM) / (np.float32(R.total_norm(case.grads[0])) + np.float32(1e-6))
    # two float32 roundings (the norm, the quotient) separate the kernel's coefficient from this one: 2 ulp = 2.4e-7
    assert abs(float(coef) - float(want)) <= 2.4e-7 * float(want) and float(coef) < 1.0
    for q, g in zip(params, case.grads[0]):
        assert torch.equal(q.grad, torch.tensor(g, device=DEV) * coef)
    assert _bitwise(R.torch_result(opt, params), dict(plain, norms=[]))
    # without either option the gradients are left as they were
    for q, g in zip(plain_opt.param_groups[0]["params"], case.grads[0]):
        assert torch.equal(q.grad, torch.tensor(g, device=DEV))


def test_non_finite_and_all_zero_gradients():
    import hierarchicalgnn_amd as H
    case = _case(1e-2)
    grads = [None if g is None else g.copy() for g in case.grads[0]]
    grads[5][17] = np.inf
    params, t_params = _params(case), _params(case)
    opt = H.FusedAdamW(params, lr=1e-3, max_grad_norm=R.MAX_NORM)
    tor = torch.optim.AdamW(t_params, lr=1e-3, amsgrad=True)
    _set_grads(params, grads)
    _set_grads(t_params, grads)
    opt.step()
    torch.nn.utils.clip_grad_norm_(t_params, R.MAX_NORM)
    tor.step()
    assert float(opt.last_grad_norm) == np.inf
    n_nan = 0
    for q, r in zip(params, t_params):
        assert torch.equal(torch.isnan(q), torch.isnan(r))
        n_nan += int(torch.isnan(q).sum())
        conftest.assert_parity(torch.nan_to_num(q), torch.nan_to_num(r), what="finite elements")
    assert n_nan == 1
    with pytest.raises(RuntimeError, match="inf or NaN"):
        opt.check()
    opt.check()                                        # cleared
    # all-zero gradients: the decay and nothing else
    params = _params(case)
    before = [q.detach().clone() for q in params]
    opt = H.FusedAdamW(params, lr=1e-3, weight_decay=0.1, max_grad_norm=R.MAX_NORM)
    for q in params:
        q.grad = torch.zeros_like(q)
    opt.step()
    for q, b in zip(params, before):
        assert torch.equal(q.detach(), b * np.float32(1.0 - 1e-3 * 0.1))
        assert not opt.state[q]["exp_avg"].any() and not opt.state[q]["max_exp_avg_sq"].any()
    assert float(opt.last_grad_norm) == 0.0
    opt.check()


def test_gradients_the_kernels_cannot_read_are_refused():
    import hierarchicalgnn_amd as H
    p = torch.nn.Parameter(torch.zeros(4, 6, device=DEV))
    opt = H.FusedAdamW([p], lr=1e-3)
    p.grad = torch.zeros(6, 4, device=DEV).t()
    with pytest.raises(RuntimeError, match="contiguous"):
        opt.step()
    p.grad = torch.zeros(4, 6, device=DEV).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()
    assert float(opt.state.get(p, {}).get("step", 0.0)) == 0.0          # a refused step counts nothing
    with pytest.raises(RuntimeError, match="add_param_group"):
        opt.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(3, device=DEV))]))


# ---- state dicts --------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_and_a_torch_state_dict():
    import hierarchicalgnn_amd as H
    case = _case(1e-2)
    # (a) save after two steps, load into a fresh optimiser over copies of the parameters, go on: the same bits
    opt, params, _ = _fused_run(case, steps=2)
    sd = copy.deepcopy(opt.state_dict())
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    params2 = [torch.nn.Parameter(q.detach().clone()) for q in params]
    opt2 = H.FusedAdamW(params2, lr=123.0, max_grad_norm=R.MAX_NORM)
    opt2.load_state_dict(sd)
    opt.load_state_dict(opt.state_dict())             # onto itself: the loaded tensors ARE the views
    for o, ps in ((opt, params), (opt2, params2)):
        for t in range(2, R.STEPS):
            for pg in o.param_groups:
                pg["lr"] = R.LRS[t]
            _set_grads(ps, case.grads[t])
            o.step()
    _, _, straight = _fused_run(case)
    for o, ps in ((opt, params), (opt2, params2)):
        assert _bitwise(R.torch_result(o, ps), dict(straight, norms=[]))
    q = params2[3]
    assert opt2.state[q]["exp_avg"].untyped_storage().data_ptr() == opt2._flat["exp_avg"].untyped_storage().data_ptr()
    # (b) a torch.optim.AdamW state dict after two steps: the third step matches torch's third step
    t_params = _params(case)
    tor = torch.optim.AdamW(t_params, lr=R.LRS[0], amsgrad=True)
    for t in range(3):
        if t == 2:
            params3 = [torch.nn.Parameter(q.detach().clone()) for q in t_params]
            opt3 = H.FusedAdamW(params3, lr=R.LRS[0], max_grad_norm=R.MAX_NORM)
            opt3.load_state_dict(copy.deepcopy(tor.state_dict()))
            _set_grads(params3, case.grads[t])
            opt3.step()
        _set_grads(t_params, case.grads[t])
        torch.nn.utils.clip_grad_norm_(t_params, R.MAX_NORM)
        tor.step()
    _assert_parity(R.torch_result(opt3, params3), R.torch_result(tor, t_params), case, True, "third step")
    assert R.torch_result(opt3, params3)["step"] == R.torch_result(tor, t_params)["step"]
    # (c) and the other way: torch.optim.AdamW accepts a FusedAdamW state dict
    torch.optim.AdamW(_params(case), lr=1e-3, amsgrad=True).load_state_dict(copy.deepcopy(opt3.state_dict()))


# ---- the weight-cache contract ------------------------------------------------------------------------------------
@pytest.mark.both_fp32_gemms
def test_the_fused_forward_sees_the_updated_weights():
    """a make_mlp network at latent 128 on 64 rows: after step() the fused no-grad forward (which keeps prepared copies
    of the weights keyed on their version counters) matches the library path, differs from its pre-step output, and
    every parameter's version counter rose"""
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import fused
    torch.manual_seed(3)
    L = 128
    net = H.make_mlp(L, 2 * L, L, 2, layer_norm=True, output_activation="Tanh", hidden_activation="GELU").to(DEV)
    x = torch.randn(64, L, device=DEV)

    def run():
        with torch.no_grad():
            return fused.fused_concat_mlp(net, [(x, None)], None).clone()

    def library():
        with torch.no_grad(), fused.options(enabled=False):
            return net(x)

    before = run()
    assert float((before - library()).abs().max()) < 1e-4
    opt = H.FusedAdamW(net.parameters(), lr=1e-2, max_grad_norm=0.5)
    for p in net.parameters():
        p.grad = torch.randn_like(p)
    versions = [p._version for p in net.parameters()]
    opt.step()
    assert all(p._version > v for p, v in zip(net.parameters(), versions))
    after = run()
    assert float((after - library()).abs().max()) < 1e-4
    assert float((after - before).abs().max()) > 1e-3


# ---- end to end ---------------------------------------------------------------------------------------------------
def test_ec_in_training_step_equals_the_torch_composition():
    """EC_InteractionGNN at latent 32 on 400 synthetic hits: forward, ec_training_loss, backward, optimizer_step
    (warm-up lr, clip at 0.5, AdamW, zero_grad), against the same step through clip_grad_norm_ + torch.optim.AdamW"""
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import synth
    from hierarchicalgnn_amd.models import EC_InteractionGNN
    hp = dict(spatial_channels=3, latent=32, hidden=64, n_interaction_graph_iters=2, nb_node_layer=3,
              nb_edge_layer=2, output_layers=3, hidden_output_activation="GELU", hidden_activation="GELU",
              layernorm=True, share_weight=False, weight_leak=0.1, weight_min=0.1, pt_interval=0.5, ptcut=1.0,
              log_weight_ratio=0.3, true_edges="pid_true_edges", lr=2e-3, warmup=4, patience=10, factor=0.3,
              model=1)
    torch.manual_seed(0)
    n, e = 400, 2400
    x, ei = synth.trackml_event(n, e, seed=5)
    x, ei = x.to(DEV), ei.to(DEV)
    g = torch.Generator().manual_seed(5)
    y_pid = torch.rand(e, generator=g) < 0.4
    pt = torch.empty(n).exponential_(1.0, generator=g)
    batch = {"edge_index": ei, "y": y_pid.to(DEV), "y_pid": y_pid.to(DEV), "pt": pt.to(DEV)}
    model = EC_InteractionGNN(hp).to(DEV).train()
    twin = copy.deepcopy(model)
    (opt,), (sched,) = H.configure_optimizers(model, hp)
    assert isinstance(opt, H.FusedAdamW) and opt.max_grad_norm == 0.5 and sched["scheduler"].step_size == 10
    tor = torch.optim.AdamW(twin.parameters(), lr=hp["lr"], betas=(0.9, 0.999), eps=1e-08, amsgrad=True)
    for step in range(2):
        H.ec_training_loss(model(x, ei), batch, hp).backward()
        H.optimizer_step(opt, step, hp)
        H.ec_training_loss(twin(x, ei), batch, hp).backward()
        for pg in tor.param_groups:
            pg["lr"] = hp["lr"] * (step + 1) / hp["warmup"]
        torch.nn.utils.clip_grad_norm_(twin.parameters(), 0.5)
        tor.step()
        tor.zero_grad()
    H.weighted_bce_check()
    opt.check()
    assert opt.param_groups[0]["lr"] == hp["lr"] * 2 / 4
    assert all(p.grad is None for p in model.parameters())
    named, t_named = dict(model.named_parameters()), dict(twin.named_parameters())
    assert len(named) == len(t_named) > 0
    for k in named:
        conftest.assert_parity(named[k], t_named[k], what=k)
