"""CPU-only checks of the torch_scatter shim's surface and of hgnn_segment_reduce_ex's host-side argument checks."""
import importlib
import inspect
import sys

import pytest
import torch

import conftest
from hierarchicalgnn_amd import _lib

# every name the reference imports from torch_scatter, plus the generic entry
NAMES = ["scatter_add", "scatter_sum", "scatter_mean", "scatter_min", "scatter_max", "scatter"]


@pytest.fixture()
def shim():
    sys.path.insert(0, conftest.ROOT + "/torch_scatter_shim")
    try:
        yield importlib.import_module("torch_scatter")
    finally:
        sys.path.pop(0)
        sys.modules.pop("torch_scatter", None)


def test_shim_exports_the_reference_names(shim):
    for n in NAMES:
        assert callable(getattr(shim, n, None)), f"torch_scatter shim lacks {n}"
    for n in ("scatter_min", "scatter_max", "scatter"):
        sig = inspect.signature(getattr(shim, n))
        assert list(sig.parameters)[:5] == ["src", "index", "dim", "out", "dim_size"], n
        assert sig.parameters["dim"].default == -1, n
    assert inspect.signature(shim.scatter).parameters["reduce"].default == "sum"


def test_cpu_tensors_raise_runtime_error_not_not_implemented(shim):
    x, idx = torch.randn(6, 3), torch.tensor([0, 0, 1, 2, 2, 2])
    for call in (lambda: shim.scatter_min(x, idx, dim=0),
                 lambda: shim.scatter_max(x, idx, dim=0),
                 lambda: shim.scatter(x, idx, dim=0, reduce="max"),
                 lambda: shim.scatter_sum(idx, idx),
                 lambda: shim.scatter_mean(idx, idx)):
        with pytest.raises(RuntimeError) as ei:
            call()
        assert not isinstance(ei.value, NotImplementedError)
    with pytest.raises(RuntimeError, match="CPU fallback"):
        shim.scatter_min(x, idx, dim=0)
    with pytest.raises(RuntimeError, match="float64"):
        shim.scatter_max(x.double(), idx, dim=0)
    with pytest.raises(ValueError):
        shim.scatter(x, idx, dim=0, reduce="mul")


def test_segment_reduce_ex_rejects_bad_codes_on_the_host():
    lib = _lib.load()
    plan = _lib.HgnnPlan()
    rc = lib.hgnn_segment_reduce_ex(plan, 7, _lib.DT_F32, None, 4, None, None, None, None, None)
    assert rc != 0 and b"op" in lib.hgnn_last_error()
    rc = lib.hgnn_segment_reduce_ex(plan, _lib.RED_MIN, 9, None, 4, None, None, None, None, None)
    assert rc != 0 and b"dtype" in lib.hgnn_last_error()
    rc = lib.hgnn_segment_reduce_ex(plan, _lib.RED_SUM, _lib.DT_F32, None, 4, None, None, None, None, None)
    assert rc != 0 and b"hgnn_segment_reduce_f32" in lib.hgnn_last_error()
    rc = lib.hgnn_segment_reduce_ex(None, _lib.RED_MAX, _lib.DT_I64, None, 4, None, None, None, None, None)
    assert rc != 0 and b"plan" in lib.hgnn_last_error()
    rc = lib.hgnn_segment_arg_backward(None, 4, 1, 4, _lib.DT_I32, None, None, None)
    assert rc != 0 and b"dtype" in lib.hgnn_last_error()
