"""CPU proofs behind the activation codes 4..7 (tests/act_ref.py): the float64 definitions are torch.nn's, the float32
emulation of the device forms stays within the bounds stated in csrc/mlp_common.h on the whole input grid at every
modelled error of the two transcendental instructions, and the GPU cases of tests/test_gpu_mlp_activations.py /
tests/test_gpu_mlp_plain.py stay within HALF of the 1e-4 bar in that emulation."""
import itertools

import numpy as np
import pytest
import torch

import act_ref as A
import ln_ref as R

_MODULES = {A.ACT_SILU: torch.nn.SiLU, A.ACT_LEAKY_RELU: torch.nn.LeakyReLU, A.ACT_ELU: torch.nn.ELU,
            A.ACT_SIGMOID: torch.nn.Sigmoid}
_DELTAS = list(itertools.product((-1, 0, 1), repeat=2))


@pytest.mark.parametrize("act", A.NEW_CODES)
def test_definitions_are_torch_nn_at_its_defaults(act):
    y = torch.from_numpy(A.grid().astype(np.float64))
    y = y[y.abs() < 1e4].clone().requires_grad_(True)
    out = _MODULES[act]()(y)
    assert torch.equal(out.detach(), A.act64(y.detach(), act))
    out.sum().backward()
    d = A.act_grad64(y.detach(), act)
    # autograd's SiLU / Sigmoid derivative forms 1 - s, which cancels to |y| 2^-52 at |y| <= 104; act_grad64 does not
    assert float((y.grad - d).abs().max()) <= 104 * 2.0 ** -51
    assert A.ACT_CODE[_MODULES[act].__name__] == act


@pytest.mark.parametrize("kind", ["val", "grad", "val2"])
@pytest.mark.parametrize("act", A.NEW_CODES)
def test_emulated_device_forms_stay_within_the_stated_bounds(act, kind):
    x = A.grid()
    xd = torch.from_numpy(x.astype(np.float64))
    ref = (A.act_grad64 if kind == "grad" else A.act64)(xd, act).numpy()
    fn = {"val": A.emul_act, "grad": A.emul_act_grad, "val2": A.emul_act_val}[kind]
    worst = 0.0
    for dexp, drcp in _DELTAS:
        got = fn(x, act, dexp, drcp).astype(np.float64)
        assert np.isfinite(got).all(), (act, kind, dexp, drcp, x[~np.isfinite(got)][:4])
        ratio = np.abs(got - ref) / A.bound(kind, act, x.astype(np.float64), ref)
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (act, kind, dexp, drcp, float(x[ratio.argmax()]), float(ratio.max()))
    print(f"act {act} {kind}: worst error / stated bound = {worst:.3f}")


def test_elu_holds_its_relative_bound_in_the_cancelling_range():
    # exp(x) - 1 in float32 loses everything below |x| ~ 2^-24 and half the bits at 2^-12: the form must not
    x = A._f([-s * 2.0 ** e for e in range(-20, -5) for s in (1.0, 1.3, 1.7)])
    ref = torch.expm1(torch.from_numpy(x.astype(np.float64))).numpy()
    for dexp in (-1, 0, 1):
        got = A.emul_act(x, A.ACT_ELU, dexp).astype(np.float64)
        assert float((np.abs(got - ref) / np.abs(ref)).max()) <= 4 * A.U
    naive = (np.exp(x) - np.float32(1.0)).astype(np.float64)
    assert float((np.abs(naive - ref) / np.abs(ref)).max()) > 1e-3      # what the issue rules out


def test_silu_derivative_relative_to_its_scale():
    x = A.grid()
    x = x[np.abs(x) <= 30]
    ref = A.act_grad64(torch.from_numpy(x.astype(np.float64)), A.ACT_SILU).numpy()
    got = A.emul_act_grad(x, A.ACT_SILU, 1, -1).astype(np.float64)
    assert float((np.abs(got - ref) / np.maximum(np.abs(ref), 0.125)).max()) <= 64 * A.U


_ALL = [("f32", k, c, False, False) for k, c in A.F32_ACT_CONFIGS.items()] + \
       [("split3", k, c, False, True) for k, c in A.SPLIT3_ACT_CONFIGS.items()] + \
       [("plain", k, c, True, False) for k, c in A.PLAIN_CONFIGS.items()]


@pytest.mark.parametrize("kernel,key,cfg,plain,matrix", _ALL, ids=[f"{a}-{b}" for a, b, *_ in _ALL])
def test_gpu_cases_stay_within_half_the_bar_in_the_emulation(kernel, key, cfg, plain, matrix):
    case = A.case_for(cfg, "r0", plain=plain, matrix=matrix, M=64)
    ref = case["ref"].numpy()
    for order, (dexp, drcp) in (("fwd", (1, 1)), ("rev", (-1, -1))):
        got = A.emul_net(case, order, dexp, drcp)
        assert np.isfinite(got).all()
        assert R.rel_err(got, ref) <= 0.5 * R.F32_BAR, (key, order, R.rel_err(got, ref))
        assert R.elem_err(got, ref) <= 0.5 * R.F32_BAR, (key, order, R.elem_err(got, ref))


def test_case_machinery_matches_ln_ref_on_the_codes_it_knows():
    a = A.make_case("r0", [96, 64, 32], [R.ACT_GELU, R.ACT_TANH], M=16)
    b = R.make_case("r0", [96, 64, 32], M=16)
    assert torch.equal(a["ref"], b["ref"]) and all(torch.equal(x, y) for x, y in zip(a["zs"], b["zs"]))
