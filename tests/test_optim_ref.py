"""CPU: the float64 restatement of clip + AdamW (tests/optim_ref.py) against torch.optim.AdamW(amsgrad) +
clip_grad_norm_ run in float64, torch's own float32 error on the test parameter set against the bars of the GPU test,
and the mistakes those bars catch.

Torch's float32 composition against float64 on the test parameter set (CPU, the three gradient scales, amsgrad on and
off), measured by test_torch_float32_is_within_half_of_every_bar, which prints the figures:
    p_T - p_0           2.8e-5 normwise, 4.6e-5 element-wise     bar 1e-4 (conftest.assert_parity's default)
    m, v, vmax          <= 1.9e-6 (normwise and element-wise)    bar 1e-5
    total_norm          <= 9.2e-7 relative                       bar 5e-6
The differences p_T - p_0 are about 3e-3 of parameters of about 0.09, so one float32 rounding of p is already 1e-6 of
the difference; that is where the first line comes from.
"""
import numpy as np
import pytest
import torch

import optim_ref as R

CASES = {g: R.Case(g) for g in R.GSCALES}
REF = {(g, a): R.run(CASES[g], amsgrad=a) for g in R.GSCALES for a in (True, False)}


@pytest.mark.parametrize("amsgrad", [True, False])
@pytest.mark.parametrize("gscale", R.GSCALES)
def test_restatement_equals_torch_in_float64(gscale, amsgrad):
    """five steps, a changing lr, one parameter without a gradient on step 2 (it keeps its step count)"""
    case = CASES[gscale]
    got, ref = REF[gscale, amsgrad], R.torch_run(case, torch.float64, amsgrad=amsgrad)
    assert got["step"] == ref["step"] and got["step"][case.absent] == R.STEPS - 1
    e = R.errors(got, ref, case, amsgrad)
    print(f"gscale {gscale:g} amsgrad {amsgrad}: {e}")
    assert max(e.values()) <= 1e-11
    clipped = [n > R.MAX_NORM for n in got["norms"]]
    assert all(clipped) if gscale > 1e-4 else not any(clipped)


def test_restatement_without_clip_equals_torch_in_float64():
    case = CASES[1e-2]
    e = R.errors(R.run(case, max_norm=None), R.torch_run(case, torch.float64, max_norm=None), case)
    assert max(e.values()) <= 1e-11


def test_restatement_continues_from_a_state():
    case = CASES[1e-2]
    two = R.run(case, steps=2)
    e = R.errors(R.run(case, steps=R.STEPS - 2, state=two), REF[1e-2, True], case)
    assert max(e.values()) == 0.0


@pytest.mark.parametrize("amsgrad", [True, False])
@pytest.mark.parametrize("gscale", R.GSCALES)
def test_torch_float32_is_within_half_of_every_bar(gscale, amsgrad):
    """the bars of the GPU test leave torch's own float32 arithmetic a factor of two"""
    case = CASES[gscale]
    e = R.errors(R.torch_run(case, torch.float32, amsgrad=amsgrad), REF[gscale, amsgrad], case, amsgrad)
    print(f"torch float32 against float64, gscale {gscale:g} amsgrad {amsgrad}: {e}")
    assert R.within_bars(e, scale=0.5), e


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_the_bars_catch_a_planted_mistake(mutate):
    """each mistake misses the bars on at least one gradient scale (the unclamped coefficient can only show where the
    norm is below max_norm)"""
    errs = {g: R.errors(R.run(CASES[g], mutate=mutate), REF[g, True], CASES[g]) for g in R.GSCALES}
    print(mutate, errs)
    assert not all(R.within_bars(e) for e in errs.values()), errs
