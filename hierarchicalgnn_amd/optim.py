"""The update of the reference's training loops on the GPU: global-norm clip + AdamW (amsgrad) as one operator.

All four bases of the reference (Modules/*/..._base.py ``configure_optimizers`` / ``optimizer_step``) train with
``Trainer(gradient_clip_val=0.5)``, ``torch.optim.AdamW(lr, betas=(0.9, 0.999), eps=1e-8, amsgrad=True)`` with the
default decoupled ``weight_decay=0.01``, ``StepLR(patience, factor)`` per epoch and a linear warm-up that overwrites
``pg["lr"]``.  Here:

    FusedAdamW(params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, amsgrad=True, max_grad_norm=None,
               zero_grads=False)                     a torch.optim.Optimizer: csrc/optim.hip, k_opt_*.  A clipped step
                                                     is three launches (sum of squares, finish, update), an unclipped
                                                     one a single launch; every array is read and written once; no
                                                     host read; bitwise reproducible
    configure_optimizers(model, hparams)             ([FusedAdamW], [StepLR entry]) as the bases return them
    optimizer_step(optimizer, global_step, hparams)  the warm-up rule, then step(), then zero_grad()

The fused forwards keep prepared copies of the weights keyed on the parameters' version counters
(``fused._WeightCache``).  The kernels write through raw pointers, so ``step()`` itself bumps the counter of every
parameter it updated: the next forward sees the new weights.

There is no CPU path and no fallback: parameters must be contiguous float32 HIP device tensors.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

stats = {"host_reads": 0, "launches": 0}

_ALIGN = 4   # elements: every tensor's slice of the flat state buffers starts on a 16-byte boundary

_ENTRY = np.dtype([("p", "<u8"), ("g", "<u8"), ("offset", "<i8"), ("numel", "<i8"), ("first_chunk", "<i8"),
                   ("decay", "<f4"), ("step_size", "<f4"), ("inv_sqrt_bc2", "<f4"), ("one_minus_b1", "<f4"),
                   ("b2", "<f4"), ("one_minus_b2", "<f4"), ("eps", "<f4"), ("reserved", "<i4")])
assert _ENTRY.itemsize == ctypes.sizeof(_lib.HgnnOptEntry)


def _refuse(msg):
    raise RuntimeError("FusedAdamW: " + msg)


class FusedAdamW(torch.optim.Optimizer):
    """``clip_grad_norm_(params, max_grad_norm)`` + ``torch.optim.AdamW`` (+ ``zero_grad(set_to_none=False)`` with
    ``zero_grads=True``) in hand-written HIP kernels, float32 arithmetic in torch's order.

    * ``max_grad_norm=None``: no clip, one launch.  Otherwise the total norm is a float64 sum in a fixed order;
      ``last_grad_norm`` is that norm (before the clip) as a 0-d float64 device tensor, for logging.
    * ``write_clipped_grads=True`` (keyword only, not with ``zero_grads``) stores the clipped gradients back, as the
      in-place clip of ``clip_grad_norm_`` leaves them.
    * State: ``exp_avg``, ``exp_avg_sq`` and ``max_exp_avg_sq`` live in three flat float32 buffers; ``self.state[p]``
      holds views into them plus torch's ``step`` entry, so ``state_dict()`` has ``torch.optim.AdamW``'s layout and
      ``load_state_dict()`` accepts one of its state dicts (a Lightning checkpoint's ``optimizer_states[0]``).
    * lr, betas, eps and weight_decay are read from ``param_groups`` on the host at every step: torch's schedulers work
      unchanged.  Parameters whose ``grad`` is None are skipped and keep their step count.
    * ``step()`` makes NO host read.  The table of the step is staged in one of two pinned host buffers, used in
      turn; a buffer is written again only after the copy that last read it has finished (an event recorded behind
      that copy: two steps old, so the wait is a formality), which is what lets steps follow each other without any
      synchronisation.  ``check()`` is the one optional host read: RuntimeError if a gradient norm was inf or NaN.
    * Refused with RuntimeError: CPU parameters, parameters or gradients that are not contiguous float32, sparse
      gradients, ``maximize``, ``capturable``, ``differentiable``, parameters on several devices, ``add_param_group``
      after construction.
    """

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, amsgrad=True, max_grad_norm=None,
                 zero_grads=False, *, write_clipped_grads=False, maximize=False, capturable=False,
                 differentiable=False):
        if maximize or capturable or differentiable:
            _refuse("maximize, capturable and differentiable are not supported")
        if isinstance(lr, torch.Tensor):
            _refuse("lr must be a Python number (a tensor lr would need a host read per step)")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError(f"FusedAdamW: lr, eps and weight_decay must be >= 0, got {lr}, {eps}, {weight_decay}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdamW: betas must lie in [0, 1), got {betas}")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"FusedAdamW: max_grad_norm must be > 0 or None, got {max_grad_norm}")
        if zero_grads and write_clipped_grads:
            raise ValueError("FusedAdamW: zero_grads and write_clipped_grads exclude each other")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.zero_grads = bool(zero_grads)
        self.write_clipped_grads = bool(write_clipped_grads)
        self._built = False
        # the group keys of torch.optim.AdamW, so that state dicts move both ways
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad), maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._build()

    # ---- construction -------------------------------------------------------------------------------------------
    def add_param_group(self, param_group):
        if self._built:
            _refuse("add_param_group after construction is not supported (the flat state buffers are laid out once)")
        super().add_param_group(param_group)

    def _build(self):
        self._params = [p for g in self.param_groups for p in g["params"]]
        if not self._params:
            raise ValueError("FusedAdamW: no parameters")
        for p in self._params:
            self._check_tensor(p, "a parameter")
            if not p.is_cuda:
                _refuse("needs HIP device parameters: hierarchicalgnn_amd has no CPU path")
        self._device = self._params[0].device
        if any(p.device != self._device for p in self._params):
            _refuse("all parameters must be on one device")
        if len({g["amsgrad"] for g in self.param_groups}) != 1:
            _refuse("amsgrad must be the same in every parameter group")
        self.amsgrad = bool(self.param_groups[0]["amsgrad"])
        self._index = {id(p): i for i, p in enumerate(self._params)}
        numel = np.array([p.numel() for p in self._params], np.int64)
        padded = (numel + _ALIGN - 1) // _ALIGN * _ALIGN
        self._numel = numel
        self._offset = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
        self._state_numel = int(padded.sum())
        dev = self._device
        names = ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if self.amsgrad else ())
        self._flat = {k: torch.zeros(max(self._state_numel, _ALIGN), dtype=torch.float32, device=dev) for k in names}
        self._steps = torch.zeros(len(self._params), dtype=torch.float32)     # torch's `step` entries, on the host
        self._steps_np = self._steps.numpy()
        self._group_of = np.concatenate([np.full(len(g["params"]), gi, np.int64)
                                         for gi, g in enumerate(self.param_groups)])
        self._opt_state = torch.zeros(_lib.OPT_STATE, dtype=torch.float64, device=dev)
        self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        nb = ctypes.c_size_t(0)
        _lib.check(_lib.load().hgnn_optim_workspace_bytes(0, ctypes.byref(nb)), "hgnn_optim_workspace_bytes")
        self._ws = torch.empty(int(nb.value), dtype=torch.uint8, device=dev)
        self._ws_bytes = int(nb.value)
        self._staging = [None, None]          # [pinned uint8 tensor, event behind the copy that last read it]
        self._turn = 0
        self._p_ptr = np.array([p.data_ptr() for p in self._params], np.uint64)
        self._built = True

    @staticmethod
    def _check_tensor(t, what):
        if t.is_sparse or t.layout != torch.strided:
            _refuse(f"{what} is sparse; only dense tensors are supported")
        if t.dtype != torch.float32:
            _refuse(f"{what} is {t.dtype}; only float32 is supported")
        if not t.is_contiguous():
            _refuse(f"{what} is not contiguous")

    def _views(self, i):
        p = self._params[i]
        o, n = int(self._offset[i]), int(self._numel[i])
        return {k: buf[o:o + n].view(p.shape) for k, buf in self._flat.items()}

    def _init_state(self, i):
        st = self.state[self._params[i]]
        if "step" not in st:
            st["step"] = self._steps[i]
            st.update(self._views(i))

    # ---- the step -----------------------------------------------------------------------------------------------
    @property
    def last_grad_norm(self):
        """total gradient norm of the last clipped step, before the clip: 0-d float64 on the device, or None"""
        return self._opt_state[_lib.OPT_NORM] if self._have_norm else None

    _have_norm = False

    def _table(self):
        """(host table as a structured array, n_chunks, the parameters in it) for the parameters that have a gradient;
        their step counts are advanced"""
        idx, gptr, empty = [], [], []
        for i, p in enumerate(self._params):
            g = p.grad
            if g is None:
                continue
            if not g.is_cuda or g.device != self._device:
                _refuse("a gradient is not on the parameters' HIP device")
            self._check_tensor(g, "a gradient")
            if p.numel() == 0:
                empty.append(i)
                continue
            idx.append(i)
            gptr.append(g.data_ptr())
            if p.data_ptr() != int(self._p_ptr[i]):            # p.data was re-pointed (load_state_dict does not, .to() may)
                self._check_tensor(p, "a parameter")
                self._p_ptr[i] = p.data_ptr()
        for i in empty:                                        # nothing to update, but torch counts the step
            self._init_state(i)
            self._steps_np[i] += 1
        idx = np.asarray(idx, np.int64)
        t = np.zeros(len(idx), _ENTRY)
        if len(idx) == 0:
            return t, 0, []
        for i in idx:
            self._init_state(int(i))
        steps = self._steps_np[idx].astype(np.float64) + 1.0
        self._steps_np[idx] = steps
        gi = self._group_of[idx]
        col = lambda key: np.array([float(g[key]) for g in self.param_groups], np.float64)[gi]   # noqa: E731
        lr, wd, eps = col("lr"), col("weight_decay"), col("eps")
        b1 = np.array([float(g["betas"][0]) for g in self.param_groups], np.float64)[gi]
        b2 = np.array([float(g["betas"][1]) for g in self.param_groups], np.float64)[gi]
        for g in self.param_groups:
            if g.get("maximize") or g.get("capturable") or g.get("differentiable"):
                _refuse("maximize, capturable and differentiable are not supported")
            if g["amsgrad"] != self.amsgrad:
                _refuse("amsgrad cannot change after construction")
        numel = self._numel[idx]
        chunks = (numel + _lib.OPT_CHUNK - 1) // _lib.OPT_CHUNK
        t["p"] = self._p_ptr[idx]
        t["g"] = np.asarray(gptr, np.uint64)
        t["offset"] = self._offset[idx]
        t["numel"] = numel
        t["first_chunk"] = np.cumsum(chunks) - chunks
        t["decay"] = 1.0 - lr * wd
        t["step_size"] = lr / (1.0 - b1 ** steps)
        t["inv_sqrt_bc2"] = 1.0 / np.sqrt(1.0 - b2 ** steps)
        t["one_minus_b1"] = 1.0 - b1
        t["b2"] = b2
        t["one_minus_b2"] = 1.0 - b2
        t["eps"] = eps
        return t, int(chunks.sum()), [self._params[int(i)] for i in idx]

    def _upload(self, table):
        """the table in device memory, copied stream-ordered from one of the two pinned staging buffers"""
        nbytes = table.nbytes
        slot = self._staging[self._turn]
        if slot is None or slot[0].numel() < nbytes:
            if slot is not None:
                slot[1].synchronize()
            slot = [torch.empty(max(nbytes, 4096), dtype=torch.uint8).pin_memory(), None]
            self._staging[self._turn] = slot
        elif slot[1] is not None:
            slot[1].synchronize()                     # the copy of two steps ago: finished long since
        self._turn ^= 1
        host = slot[0][:nbytes]
        host.numpy()[:] = table.view(np.uint8).reshape(-1)
        dev = torch.empty(nbytes, dtype=torch.uint8, device=self._device)
        dev.copy_(host, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(self._device))
        return host, dev

    @torch.no_grad()
    def step(self, closure=None, *, _scalar_path=False):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        table, n_chunks, updated = self._table()
        if len(table) == 0:
            return loss
        lib = _lib.load()
        flags = (_lib.OPT_AMSGRAD if self.amsgrad else 0) | (_lib.OPT_SCALAR if _scalar_path else 0)
        if self.zero_grads:
            flags |= _lib.OPT_ZERO_GRADS
        elif self.write_clipped_grads:
            flags |= _lib.OPT_WRITE_GRADS
        with torch.cuda.device(self._device):
            host, dev = self._upload(table)
            stream = _lib.current_stream(self._device)
            hp, dp = ctypes.c_void_p(host.data_ptr()), ctypes.c_void_p(dev.data_ptr())
            if self.max_grad_norm is not None:
                flags |= _lib.OPT_CLIP
                _lib.check(lib.hgnn_optim_grad_norm(hp, dp, len(table), n_chunks, self.max_grad_norm,
                                                    flags & _lib.OPT_SCALAR, _lib.ptr(self._opt_state),
                                                    _lib.ptr(self._status), _lib.ptr(self._ws), self._ws_bytes,
                                                    stream), "hgnn_optim_grad_norm")
                self._have_norm = True
                stats["launches"] += 2
            vmax = self._flat.get("max_exp_avg_sq")
            _lib.check(lib.hgnn_optim_adamw_step(hp, dp, len(table), n_chunks, _lib.ptr(self._flat["exp_avg"]),
                                                 _lib.ptr(self._flat["exp_avg_sq"]), _lib.ptr(vmax),
                                                 self._state_numel, flags, _lib.ptr(self._opt_state), stream),
                       "hgnn_optim_adamw_step")
            stats["launches"] += 1
        # the kernels wrote through raw pointers: tell autograd, and with it fused._WeightCache, that p changed
        torch.autograd.graph.increment_version(updated)
        return loss

    def zero_grad(self, set_to_none=True):
        """a no-op with ``zero_grads=True``: the update kernel has already stored zeros"""
        if not self.zero_grads:
            super().zero_grad(set_to_none=set_to_none)

    def check(self):
        """the one optional host read: RuntimeError if the gradient norm of any step since the last check was inf or
        NaN (the update then spread NaN exactly as torch's does)"""
        stats["host_reads"] += 1
        word = int(self._status.item())
        self._status.zero_()
        if word & _lib.OPT_ST_NONFINITE:
            raise RuntimeError("FusedAdamW: the gradient norm of a step was inf or NaN")

    # ---- state dicts --------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        """accepts its own and ``torch.optim.AdamW``'s state dicts: the loaded tensors are copied into the flat
        buffers and ``self.state`` is re-pointed at the views"""
        groups = state_dict["param_groups"]
        for g in groups:
            if g.get("maximize") or g.get("capturable") or g.get("differentiable"):
                _refuse("a state dict with maximize, capturable or differentiable cannot be loaded")
            if bool(g.get("amsgrad", False)) != self.amsgrad:
                _refuse(f"the state dict has amsgrad={g.get('amsgrad')}, this optimiser amsgrad={self.amsgrad}")
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            g.update(foreach=None, fused=None)
        # a loaded tensor may BE one of the views (torch does not copy what already has the right dtype and device):
        # nothing is cleared before everything is copied
        for i, p in enumerate(self._params):
            if p not in self.state:
                for view in self._views(i).values():
                    view.zero_()
                self._steps_np[i] = 0.0
        for p, st in list(self.state.items()):
            i = self._index[id(p)]
            views = self._views(i)
            for k, view in views.items():
                if k not in st:
                    _refuse(f"the state dict has no {k} for a parameter")
                view.copy_(st[k].to(device=self._device, dtype=torch.float32))
                st[k] = view
            self._steps_np[i] = float(st.get("step", 0.0))
            st["step"] = self._steps[i]


def configure_optimizers(model, hparams):
    """``configure_optimizers`` of the reference's bases (edge_classifier_base.py:59-80): ([optimizer], [scheduler
    entry]), the optimizer a FusedAdamW that also does the Trainer's ``gradient_clip_val`` (default 0.5, as the
    reference's training scripts set it), the scheduler StepLR(patience, factor) per epoch"""
    params = model.parameters() if hasattr(model, "parameters") else model
    optimizer = [FusedAdamW(params, lr=hparams["lr"], betas=(0.9, 0.999), eps=1e-08, amsgrad=True,
                            max_grad_norm=hparams.get("gradient_clip_val", 0.5))]
    scheduler = [{"scheduler": torch.optim.lr_scheduler.StepLR(optimizer[0], step_size=hparams["patience"],
                                                               gamma=hparams["factor"]),
                  "interval": "epoch", "frequency": 1}]
    return optimizer, scheduler


def warmup_lr(global_step, hparams):
    """the lr the reference's ``optimizer_step`` writes at ``global_step``, or None past the warm-up"""
    warmup = hparams.get("warmup")
    if warmup is None or not global_step < warmup:
        return None
    lr_scale = min(1.0, float(global_step + 1) / warmup)
    key = "mlp_lr" if hparams.get("model") == "mlp" or hparams.get("model") == 3 else "lr"
    return lr_scale * hparams[key]


def optimizer_step(optimizer, global_step, hparams, closure=None):
    """``optimizer_step`` of the reference's bases (edge_classifier_base.py:207-235): the linear warm-up that overwrites
    every group's lr while ``global_step < warmup``, then ``step()``, then ``zero_grad()``"""
    lr = warmup_lr(global_step, hparams)
    if lr is not None:
        for pg in optimizer.param_groups:
            pg["lr"] = lr
    loss = optimizer.step(closure=closure)
    optimizer.zero_grad()
    return loss
