"""CPU: the boundary of the fused optimiser step: header, binding and exports agree, the host-side entry points check
their table before anything is launched, FusedAdamW refuses what it cannot do before it touches a device, and the
warm-up / StepLR mirrors follow the reference's arithmetic."""
import ctypes
import os
import re

import pytest
import torch

import conftest
from hierarchicalgnn_amd import _lib

HEADER = os.path.join(conftest.ROOT, "include", "hgnn_hip.h")
ENTRY_POINTS = ("hgnn_sizeof_opt_entry", "hgnn_optim_workspace_bytes", "hgnn_optim_grad_norm",
                "hgnn_optim_adamw_step")


def test_entry_points_and_constants_are_declared_exported_and_bound():
    txt = open(HEADER).read()
    lib = _lib.load()
    assert int(re.search(r"#define\s+HGNN_ABI_VERSION\s+(\d+)", txt).group(1)) == _lib.ABI_VERSION \
        == lib.hgnn_abi_version()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\(", txt) and name in _lib.declared_symbols() and hasattr(lib, name)
    for name in ("CHUNK", "AMSGRAD", "CLIP", "ZERO_GRADS", "WRITE_GRADS", "SCALAR", "ST_NONFINITE", "NORM", "COEF",
                 "SUMSQ", "STATE"):
        assert int(re.search(rf"#define\s+HGNN_OPT_{name}\s+(\d+)", txt).group(1)) == getattr(_lib, "OPT_" + name)
    assert lib.hgnn_sizeof_opt_entry() == ctypes.sizeof(_lib.HgnnOptEntry) == 72
    from hierarchicalgnn_amd import optim
    assert optim._ENTRY.itemsize == 72
    assert [optim._ENTRY.fields[n][1] for n, _ in _lib.HgnnOptEntry._fields_] == \
        [getattr(_lib.HgnnOptEntry, n).offset for n, _ in _lib.HgnnOptEntry._fields_]


def test_workspace_size_does_not_depend_on_the_chunk_count():
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    sizes = []
    for n in (0, 1, 1 << 20):
        assert lib.hgnn_optim_workspace_bytes(n, ctypes.byref(nb)) == 0
        sizes.append(nb.value)
    assert sizes[0] == sizes[1] == sizes[2] > 0
    assert lib.hgnn_optim_workspace_bytes(-1, ctypes.byref(nb)) != 0


def _table(entries):
    t = (_lib.HgnnOptEntry * len(entries))()
    for e, (numel, offset, first_chunk) in zip(t, entries):
        e.p = e.g = 64                   # non-NULL; nothing is dereferenced before the checks fail
        e.numel, e.offset, e.first_chunk = numel, offset, first_chunk
    return t


@pytest.mark.parametrize("entries,n_chunks,state_numel,word", [
    ([(5000, 0, 0), (10, 5000, 1)], 3, 5010, b"first_chunk"),          # 5000 elements are two chunks
    ([(5000, 0, 0), (10, 5000, 2)], 4, 5010, b"n_chunks"),
    ([(5000, 0, 0), (10, 5004, 2)], 3, 5010, b"outside the state buffers"),
    ([(-1, 0, 0)], 0, 16, b"outside the state buffers"),
    ([(8, -4, 0)], 1, 16, b"outside the state buffers"),
])
def test_a_table_that_would_leave_its_buffers_is_refused_on_the_host(entries, n_chunks, state_numel, word):
    """the checks run on the host copy of the table and fail before any launch: no device is needed"""
    lib = _lib.load()
    t = _table(entries)
    rc = lib.hgnn_optim_adamw_step(ctypes.cast(t, ctypes.c_void_p), ctypes.c_void_p(64), len(entries), n_chunks,
                                   ctypes.c_void_p(64), ctypes.c_void_p(64), ctypes.c_void_p(64), state_numel,
                                   _lib.OPT_AMSGRAD, None, None)
    assert rc != 0 and word in lib.hgnn_last_error(), lib.hgnn_last_error()


def test_bad_flags_and_null_pointers_are_refused_on_the_host():
    lib = _lib.load()
    t = _table([(8, 0, 0)])
    args = (ctypes.cast(t, ctypes.c_void_p), ctypes.c_void_p(64), 1, 1, ctypes.c_void_p(64), ctypes.c_void_p(64),
            ctypes.c_void_p(64), 8)
    assert lib.hgnn_optim_adamw_step(*args, 1 << 10, None, None) != 0
    assert lib.hgnn_optim_adamw_step(*args, _lib.OPT_ZERO_GRADS | _lib.OPT_WRITE_GRADS, None, None) != 0
    assert lib.hgnn_optim_adamw_step(*args, _lib.OPT_CLIP, None, None) != 0             # clip without a state
    assert lib.hgnn_optim_adamw_step(*args[:4], None, None, None, 8, 0, None, None) != 0
    assert lib.hgnn_optim_adamw_step(*args[:4], ctypes.c_void_p(68), ctypes.c_void_p(64), None, 8, 0, None,
                                     None) != 0 and b"16-byte" in lib.hgnn_last_error()
    assert lib.hgnn_optim_grad_norm(args[0], args[1], 1, 1, 0.5, 0, None, None, None, 0, None) != 0
    assert lib.hgnn_optim_grad_norm(args[0], args[1], 1, 1, 0.5, _lib.OPT_CLIP, ctypes.c_void_p(64),
                                    ctypes.c_void_p(64), ctypes.c_void_p(64), 1 << 20, None) != 0
    rc = lib.hgnn_optim_grad_norm(args[0], args[1], 1, 1, 0.5, 0, ctypes.c_void_p(64), ctypes.c_void_p(64),
                                  ctypes.c_void_p(64), 8, None)
    assert rc != 0 and b"workspace" in lib.hgnn_last_error()


def test_python_surface_is_exported():
    import inspect
    import hierarchicalgnn_amd as H
    from hierarchicalgnn_amd import optim
    for name in ("FusedAdamW", "configure_optimizers", "optimizer_step"):
        assert getattr(H, name) is getattr(optim, name)
    assert issubclass(H.FusedAdamW, torch.optim.Optimizer)
    sig = inspect.signature(H.FusedAdamW.__init__).parameters
    want = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, amsgrad=True, max_grad_norm=None, zero_grads=False)
    assert list(sig)[:9] == ["self", "params", "lr"] + list(want)
    for k, v in want.items():
        assert sig[k].default == v


def test_cpu_parameters_are_refused_loudly():
    import hierarchicalgnn_amd as H
    with pytest.raises(RuntimeError, match="HIP device"):
        H.FusedAdamW([torch.nn.Parameter(torch.zeros(8))], lr=1e-3)
    with pytest.raises(RuntimeError, match="HIP device"):
        H.configure_optimizers(torch.nn.Linear(4, 4), dict(lr=1e-3, patience=10, factor=0.3))


def test_what_the_kernels_cannot_do_is_refused_not_emulated():
    import hierarchicalgnn_amd as H
    p = lambda t: [torch.nn.Parameter(t)]   # noqa: E731
    for bad, word in ((torch.zeros(8, dtype=torch.float64), "float32"), (torch.zeros(8, dtype=torch.bfloat16), "float32"),
                      (torch.zeros(4, 6).t(), "contiguous")):
        with pytest.raises(RuntimeError, match=word):
            H.FusedAdamW(p(bad), lr=1e-3)
    for kw in ("maximize", "capturable", "differentiable"):
        with pytest.raises(RuntimeError, match=kw):
            H.FusedAdamW(p(torch.zeros(8)), lr=1e-3, **{kw: True})
    with pytest.raises(RuntimeError, match="Python number"):
        H.FusedAdamW(p(torch.zeros(8)), lr=torch.tensor(1e-3))
    for kw in (dict(lr=-1.0), dict(lr=1e-3, betas=(1.0, 0.999)), dict(lr=1e-3, eps=-1.0),
               dict(lr=1e-3, max_grad_norm=0.0), dict(lr=1e-3, zero_grads=True, write_clipped_grads=True)):
        with pytest.raises(ValueError):
            H.FusedAdamW(p(torch.zeros(8)), **kw)


def _reference_warmup_lr(global_step, hparams, current):
    """the rule of edge_classifier_base.py:221-232 restated: what pg["lr"] holds after it ran"""
    if (hparams["warmup"] is not None) and (global_step < hparams["warmup"]):
        lr_scale = min(1.0, float(global_step + 1) / hparams["warmup"])
        if hparams["model"] == "mlp" or hparams["model"] == 3:
            return lr_scale * hparams["mlp_lr"]
        return lr_scale * hparams["lr"]
    return current


class _Recorder(torch.optim.Optimizer):
    """an optimiser that only records: the mirrors are host arithmetic and run without a device"""

    def __init__(self, lr):
        super().__init__([torch.nn.Parameter(torch.zeros(2))], dict(lr=lr))
        self.calls = []

    def step(self, closure=None):
        self.calls.append(("step", self.param_groups[0]["lr"]))

    def zero_grad(self, set_to_none=True):
        self.calls.append(("zero_grad", set_to_none))


@pytest.mark.parametrize("model,warmup", [(1, 5), ("mlp", 5), (3, 4), (2, None), (2, 0)])
def test_warmup_and_step_lr_follow_the_reference(model, warmup):
    """steps 0 .. warmup + 2, two steps per epoch, StepLR(patience=2, factor=0.3) stepped per epoch as Lightning does"""
    from hierarchicalgnn_amd import optim
    hp = dict(lr=2e-3, mlp_lr=5e-4, warmup=warmup, model=model, patience=2, factor=0.3)
    opt = _Recorder(hp["lr"])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=hp["patience"], gamma=hp["factor"])
    ref_opt = _Recorder(hp["lr"])
    ref_sched = torch.optim.lr_scheduler.StepLR(ref_opt, step_size=hp["patience"], gamma=hp["factor"])
    for step in range((warmup or 0) + 3):
        want = _reference_warmup_lr(step, hp, ref_opt.param_groups[0]["lr"])
        ref_opt.param_groups[0]["lr"] = want
        opt.calls.clear()
        optim.optimizer_step(opt, step, hp)
        assert opt.calls == [("step", want), ("zero_grad", True)]
        assert opt.param_groups[0]["lr"] == want
        if step % 2 == 1:
            sched.step()
            ref_sched.step()
            assert opt.param_groups[0]["lr"] == ref_opt.param_groups[0]["lr"]
