"""AdamW of the example trainer as one launch (ref xrays/train_xrays_example.py:322-323, 376 uses
``torch.optim.AdamW(lr=1e-4, weight_decay=0.01)``).  Same update rule and the same state layout as torch's (per parameter:
``step`` -- a float32 scalar on the device --, ``exp_avg``, ``exp_avg_sq``), so state dicts move between the two; the step
counters advance on the device, which makes ``step()`` capturable into a HIP graph without further flags.

Two entry points of the library sit behind ``FusedAdamW.step``:

* ``aecf_adamw_step``: float32 parameters with float32 gradients, a Python-number ``lr``, no clipping, no GradScaler -- the
  step of the float32 trainer, unchanged.
* ``aecf_adamw_mp_step``: everything else -- bf16 / f16 parameters (gradients in the parameter's dtype or float32) with
  float32 moments and, with ``master_weights=True``, float32 master weights in ``state[p]["master"]``; global-norm clipping
  (``max_grad_norm``); ``torch.amp.GradScaler`` on the device; a learning rate read from device memory.

Under capture the Python-number hyper-parameters are kernel ARGUMENTS: a captured step replays with the values it was captured
with.  A learning-rate schedule therefore passes ``lr`` as a one-element float32 tensor on the parameters' device (as torch's
fused AdamW allows): the kernel reads it at replay time, so ``lr.fill_(...)`` between replays is followed.  A replay moves no
version counter: ``xray.GraphedTrainStep`` tells the pools of its model after each one; after replays of a graph of your own,
call ``invalidate_cast_cache()`` on the pools before inference.

``FusedAdamW(ema_decay=...)`` keeps an exponential moving average of the weights, ``e <- e + (1 - decay) (w - e)``, in the
step's own launch (``aecf_adamw_mp_ema_step``; ``aecf_ema_update`` for the parameters that had no gradient): the momentum key
encoder of MoCo beside ``losses.KeyQueue``, and the averaged weights people evaluate and ship.  ``EmaModel`` is a copy of the
model whose parameters ARE those averages; ``FusedAdamW.ema_weights()`` puts them into the live model for a ``with`` block."""
from __future__ import annotations

import contextlib
import copy
import ctypes
from itertools import chain
from typing import Iterable

import torch

from . import _lib
from .layer import _stream

_DTYPES = {torch.bfloat16: _lib.AECF_BF16, torch.float32: _lib.AECF_F32, torch.float16: _lib.AECF_F16}
_F32_STATE = ("master", "exp_avg", "exp_avg_sq", "ema")


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _launch_grad_norm(grads, max_norm, grad_scale, workspace, out):
    lib = _lib.load()
    numel = (ctypes.c_int64 * len(grads))(*[g.numel() for g in grads])
    _lib.check(lib.aecf_grad_norm(
        len(grads), _ptr_array(grads), (ctypes.c_int32 * len(grads))(*[_DTYPES[g.dtype] for g in grads]), numel,
        float(max_norm), None if grad_scale is None else grad_scale.data_ptr(), workspace.data_ptr(),
        workspace.numel() * 4, out.data_ptr(), _stream()), "aecf_grad_norm")


def _dense_grads(params):
    grads = []
    for p in params:
        g = p.grad
        if g is None or g.numel() == 0:
            continue
        if g.device.type != "cuda" or g.is_sparse or g.dtype not in _DTYPES:
            raise RuntimeError("aecf_amd.optim: dense float32 / bfloat16 / float16 gradients on a ROCm device only")
        grads.append(g if g.is_contiguous() else g.contiguous())
    return grads


def grad_norm(params, *, grad_scale=None) -> torch.Tensor:
    """Global L2 norm of the gradients of ``params`` (``aecf_grad_norm``: two launches, fixed summation order) as a float32
    scalar ON THE DEVICE -- no host synchronisation.  ``grad_scale`` (a one-element float32 device tensor, e.g. a GradScaler's
    scale) divides the result.  What ``torch.nn.utils.clip_grad_norm_(params, inf)`` returns, without touching the gradients."""
    grads = _dense_grads([params] if torch.is_tensor(params) else list(params))
    if not grads:
        raise RuntimeError("aecf_amd.optim.grad_norm: no gradients")
    dev = grads[0].device
    if any(g.device != dev for g in grads):
        raise RuntimeError("aecf_amd.optim.grad_norm: gradients on one device only")
    lib = _lib.load()
    need = lib.aecf_grad_norm_workspace_bytes(len(grads), (ctypes.c_int64 * len(grads))(*[g.numel() for g in grads]))
    workspace = torch.empty(need // 4, dtype=torch.float32, device=dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    _launch_grad_norm(grads, 0.0, grad_scale, workspace, out)
    return out[0]


class FusedAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` (amsgrad / maximize off) in one launch per 24 tensors.

    ``lr``: a Python number, or a one-element float32 tensor on the parameters' device that the kernel reads.
    ``master_weights``: keep a float32 ``state[p]["master"]`` for every bf16 / f16 parameter (created from the parameter at
    its first step); the parameter is then the round-to-nearest-even of its master after every step.  At lr = 1e-4 the update
    of a bf16 weight near 1 is below half an ulp: without masters such a weight never moves.
    ``max_grad_norm``: clip by the global L2 norm of all gradients of this optimiser (they must live on one device), computed
    by one ``aecf_grad_norm`` before the update launches.  ``last_grad_norm`` is the (unscaled) norm and ``last_clip_coef`` the
    coefficient, as device tensors that are never read on the host.  Two differences from ``torch.nn.utils.clip_grad_norm_``: the gradients themselves are NOT rewritten
    (the coefficient ``min(1, max / (norm + 1e-6))`` is applied inside the update), and a non-finite norm does not let NaN
    through -- the step is skipped on the device (nothing is written, no step counter advances) and the device counter
    ``skipped_steps`` (None until the first clipped step) goes up by one.
    ``torch.amp.GradScaler``: ``scaler.step(opt)`` hands over its scale and its found-inf flag as device tensors; the kernel
    unscales and skips by them, with no ``.item()``.  With clipping on, the scaler's flag and the norm's are two pointer
    arguments of the same launch (OR-ed by the kernel).
    ``ema_decay``: None (no average: the calls and bits of an optimiser without the argument), a number in [0, 1], or a
    one-element float32 tensor on the parameters' device that the kernel reads at replay time (a schedule -- a warm-up, say --
    is written into that tensor; there is no built-in rule).  ``state[p]["ema"]`` is a float32 average of the weight as STORED
    (the master where there is one), created from it at the parameter's first step and moved by every step that is not
    skipped on the device -- for the parameters without a gradient in that step too -- and by none that is.  One decay for
    the whole optimiser; under data parallel every rank keeps the same averages (replicated, not sharded)."""

    _step_supports_amp_scaling = True

    def __init__(self, params: Iterable, lr=1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, *,
                 master_weights: bool = False, max_grad_norm=None, ema_decay=None):
        if torch.is_tensor(lr):
            if lr.numel() != 1 or lr.dtype != torch.float32:
                raise ValueError("FusedAdamW: a tensor lr is ONE float32 element (on the parameters' device)")
        elif lr < 0:
            raise ValueError("FusedAdamW: invalid hyper-parameter")
        if eps < 0 or not 0 < betas[0] < 1 or not 0 < betas[1] < 1 or weight_decay < 0:
            raise ValueError("FusedAdamW: invalid hyper-parameter")
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError("FusedAdamW: max_grad_norm must be positive (None: no clipping)")
        if torch.is_tensor(ema_decay):
            if ema_decay.numel() != 1 or ema_decay.dtype != torch.float32:
                raise ValueError("FusedAdamW: a tensor ema_decay is ONE float32 element (on the parameters' device)")
        elif ema_decay is not None:
            if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 <= float(ema_decay) <= 1.0:
                raise ValueError("FusedAdamW: ema_decay is None, a number in [0, 1] or a one-element float32 tensor")
            ema_decay = float(ema_decay)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.ema_decay = ema_decay
        self._ema_out = {}                # 16-bit parameter -> the tensor of its dtype an EmaModel reads (ema.to(dtype))
        self._ema_held = {}               # parameter -> the float32 average an EmaModel is bound to: never replaced, only written
        self._ema_models = []
        self.master_weights = bool(master_weights)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = self.last_clip_coef = None
        self.skipped_steps = None
        self._tickets = {}
        self._norm_out = None             # [norm, coef, non-finite flag] on the device
        self._norm_workspaces = []

    def _ticket(self, device, group_index, n):
        """Ticket words of one parameter group's launch, kept for the optimizer's lifetime: a buffer that has been handed to a
        launch is NEVER freed or replaced (a captured graph replays with its address), a group that grows gets a new, larger one
        next to it."""
        need = 65 * ((n + 23) // 24)                              # AECF_ADAMW_TICKET_WORDS per launch group
        held = self._tickets.setdefault((device, group_index), [])
        for t in held:
            if t.numel() >= need:
                return t
        t = torch.zeros(max(need, 65 * 8), dtype=torch.int32, device=device)
        held.append(t)
        return t

    def _clip(self, grads, grad_scale):
        """One aecf_grad_norm over every gradient of the step; its buffers are kept like the tickets."""
        dev = grads[0].device
        if any(g.device != dev for g in grads):
            raise RuntimeError("FusedAdamW: max_grad_norm needs all parameters on one device")
        if self._norm_out is None:
            self._norm_out = torch.zeros(3, dtype=torch.float32, device=dev)
            self.skipped_steps = torch.zeros((), dtype=torch.float32, device=dev)
            self.last_grad_norm, self.last_clip_coef = self._norm_out[0], self._norm_out[1]
        elif self._norm_out.device != dev:
            raise RuntimeError("FusedAdamW: the parameters moved to another device")
        need = _lib.load().aecf_grad_norm_workspace_bytes(len(grads), (ctypes.c_int64 * len(grads))(*[g.numel() for g in grads])) // 4
        workspace = next((w for w in self._norm_workspaces if w.numel() >= need), None)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.float32, device=dev)
            self._norm_workspaces.append(workspace)
        _launch_grad_norm(grads, self.max_grad_norm, grad_scale, workspace, self._norm_out)
        self.skipped_steps.add_(self._norm_out[2])                 # (bookkeeping on the device; the skip itself is the kernel's)

    def _ema_state(self, p, st):
        """``st["ema"]`` of parameter ``p``, created from the stored weight (the master, or the widened parameter) if missing."""
        ema = st.get("ema")
        held = self._ema_held.get(p)
        if ema is None:
            src = st.get("master") if p.dtype != torch.float32 else None
            src = p.detach() if src is None else src
            if held is None:
                ema = src.to(torch.float32, memory_format=torch.contiguous_format, copy=True)
            else:
                ema = held.copy_(src)
            st["ema"] = ema
            if p in self._ema_out:
                self._ema_out[p].copy_(ema)
        elif ema.device != p.device or ema.dtype != torch.float32 or not ema.is_contiguous():
            ema = st["ema"] = ema.to(device=p.device, dtype=torch.float32).contiguous()
        return ema

    def _bind_ema(self, p, q):
        """``q`` -- the parameter of an EmaModel's copy that pairs with ``p`` -- becomes the average's output: a float32 ``q``
        IS ``state[p]["ema"]`` from here on (same storage, same version counter), a 16-bit one is written beside it."""
        if p in self._ema_held:
            raise RuntimeError("FusedAdamW: one EmaModel per optimiser")
        if not q.is_contiguous() or q.shape != p.shape or q.dtype != p.dtype or q.device != p.device:
            raise RuntimeError("EmaModel: a copy's parameter must match its original (contiguous, same shape, dtype and device)")
        st = self.state[p]
        with torch.no_grad():
            ema = self._ema_state(p, st)
            q.copy_(ema)
            if p.dtype == torch.float32:
                ema = st["ema"] = q.detach()
            else:
                self._ema_out[p] = q
            self._ema_held[p] = ema

    @contextlib.contextmanager
    def ema_weights(self):
        """Evaluate the SAME module on the averaged weights: every parameter that has an average is overwritten from it (cast to
        the parameter's dtype) on entry and restored bit for bit on exit, both by ``copy_`` (version counters move, so the pools'
        inference caches follow).  Masters are not touched.  Not for use under capture."""
        if self.ema_decay is None:
            raise RuntimeError("FusedAdamW.ema_weights: the optimiser was built without ema_decay")
        saved = []
        with torch.no_grad():
            for group in self.param_groups:
                for p in group["params"]:
                    ema = self.state.get(p, {}).get("ema")
                    if ema is not None:
                        saved.append((p, p.detach().clone()))
                        p.copy_(ema)
        try:
            yield self
        finally:
            with torch.no_grad():
                for p, keep in saved:
                    p.copy_(keep)

    def load_state_dict(self, state_dict):
        """``Optimizer.load_state_dict`` casts floating-point state to the parameter's dtype, which would round the float32
        masters and moments of a bf16 / f16 parameter: the float32 tensors of the incoming state are put back afterwards, on
        the parameter's device.  (A state written by ``torch.optim.AdamW`` for bf16 parameters holds bf16 moments and no
        master: the next step widens the moments and creates the masters from the parameters.)"""
        super().load_state_dict(state_dict)
        saved_ids = list(chain.from_iterable(g["params"] for g in state_dict["param_groups"]))
        own = list(chain.from_iterable(g["params"] for g in self.param_groups))
        for pid, p in zip(saved_ids, own):
            src = state_dict["state"].get(pid)
            if not src or p.dtype == torch.float32:
                continue
            for key in _F32_STATE:
                value = src.get(key)
                if torch.is_tensor(value) and value.dtype == torch.float32:
                    self.state[p][key] = value.detach().to(device=p.device, copy=True)
        # an average an EmaModel is bound to keeps its tensor: the loaded values are written INTO it (a loaded state without
        # "ema" gets one from the weights at the next step, in the same tensor)
        for p, held in self._ema_held.items():
            st = self.state[p]
            value = st.get("ema")
            if torch.is_tensor(value) and value is not held:
                with torch.no_grad():
                    held.copy_(value)
                    if p in self._ema_out:
                        self._ema_out[p].copy_(held)
                st["ema"] = held

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        vp = ctypes.c_void_p
        # what torch.amp.GradScaler.step sets for the duration of this call (grad_scale is None when the gradients have been
        # unscaled already, found_inf is the scaler's flag either way)
        grad_scale = getattr(self, "grad_scale", None)
        found_inf = getattr(self, "found_inf", None)
        for t in (grad_scale, found_inf):
            if t is not None and (not torch.is_tensor(t) or t.numel() != 1 or t.dtype != torch.float32 or t.device.type != "cuda"):
                raise RuntimeError("FusedAdamW: grad_scale / found_inf must be one-element float32 device tensors")
        work = []
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize"):
                # (a state dict loaded from torch.optim.AdamW can carry these; the kernel implements neither)
                raise RuntimeError("FusedAdamW: amsgrad / maximize are not implemented by aecf_adamw_step")
            ps = [p for p in group["params"] if p.grad is not None and p.numel() > 0]    # (torch skips empty tensors too)
            if not ps:
                continue
            for p in ps:
                if p.device.type != "cuda" or p.dtype not in _DTYPES or p.grad.dtype not in _DTYPES or p.grad.is_sparse:
                    raise RuntimeError("FusedAdamW: float32 / bfloat16 / float16 parameters with dense gradients on a ROCm "
                                       "device only (no CPU fallback is provided)")
                if p.grad.dtype != torch.float32 and p.grad.dtype != p.dtype:
                    raise RuntimeError("FusedAdamW: a gradient is float32 or of its parameter's dtype")
                if not p.is_contiguous():
                    raise RuntimeError("FusedAdamW: parameters must be contiguous")
                st = self.state[p]
                if "step" not in st and "exp_avg" not in st:             # (an average alone may be there already)
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["exp_avg"] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                else:
                    # a state loaded from torch.optim.AdamW keeps `step` on the host (or as a Python number) unless that optimizer
                    # was capturable: the kernel reads and advances it on the device
                    step = st["step"]
                    if not torch.is_tensor(step) or step.device != p.device or step.dtype != torch.float32:
                        st["step"] = torch.as_tensor(float(step), dtype=torch.float32, device=p.device)
                    for key in ("exp_avg", "exp_avg_sq"):
                        if st[key].device != p.device or st[key].dtype != torch.float32 or not st[key].is_contiguous():
                            st[key] = st[key].to(device=p.device, dtype=torch.float32).contiguous()
                if p.dtype != torch.float32:
                    master = st.get("master")                       # (a loaded state may carry one without the flag: it is kept)
                    if master is None:
                        if self.master_weights:
                            st["master"] = p.detach().to(torch.float32, memory_format=torch.contiguous_format)
                    elif master.device != p.device or master.dtype != torch.float32 or not master.is_contiguous():
                        st["master"] = master.to(device=p.device, dtype=torch.float32).contiguous()
                if self.ema_decay is not None:
                    self._ema_state(p, st)
            grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in ps]
            work.append((gi, group, ps, grads))
        if not work:
            if self.ema_decay is not None:
                self._ema_rest(lib, found_inf, None)
            return loss
        clip = self.max_grad_norm is not None
        if clip:
            self._clip([g for _, _, _, grads in work for g in grads], grad_scale)
        ema_dev = None
        if torch.is_tensor(self.ema_decay):
            ema_dev = self.ema_decay
            if ema_dev.numel() != 1 or ema_dev.dtype != torch.float32 or ema_dev.device != work[0][2][0].device:
                raise RuntimeError("FusedAdamW: a tensor ema_decay is ONE float32 element on the parameters' device")
        for gi, group, ps, grads in work:
            dev = ps[0].device
            lr = group["lr"]
            b1, b2 = group["betas"]
            states = [self.state[p] for p in ps]
            numel = (ctypes.c_int64 * len(ps))(*[p.numel() for p in ps])
            ticket = self._ticket(dev, gi, len(ps)).data_ptr()
            plain = (not clip and grad_scale is None and found_inf is None and not torch.is_tensor(lr)
                     and all(p.dtype == torch.float32 and g.dtype == torch.float32 for p, g in zip(ps, grads)))
            if plain and self.ema_decay is None:
                _lib.check(lib.aecf_adamw_step(
                    len(ps), _ptr_array(ps), _ptr_array(grads), _ptr_array([st["exp_avg"] for st in states]),
                    _ptr_array([st["exp_avg_sq"] for st in states]), _ptr_array([st["step"] for st in states]),
                    numel, ticket, float(lr), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), _stream()),
                    "aecf_adamw_step")
            else:
                lr_dev = None
                if torch.is_tensor(lr):
                    if lr.numel() != 1 or lr.dtype != torch.float32 or lr.device != dev:
                        raise RuntimeError("FusedAdamW: a tensor lr is ONE float32 element on the parameters' device")
                    lr_dev = lr.data_ptr()
                for t in (grad_scale, found_inf):
                    if t is not None and t.device != dev:
                        raise RuntimeError("FusedAdamW: the GradScaler's tensors and the parameters must share a device")
                i32 = ctypes.c_int32 * len(ps)
                if ema_dev is not None and ema_dev.device != dev:
                    raise RuntimeError("FusedAdamW: a tensor ema_decay is ONE float32 element on the parameters' device")
                tail, entry, name = (), lib.aecf_adamw_mp_step, "aecf_adamw_mp_step"
                if self.ema_decay is not None:
                    tail = (_ptr_array([st["ema"] for st in states]), _ptr_array([self._ema_out.get(p) for p in ps]),
                            0.0 if ema_dev is not None else self.ema_decay, None if ema_dev is None else ema_dev.data_ptr())
                    entry, name = lib.aecf_adamw_mp_ema_step, "aecf_adamw_mp_ema_step"
                _lib.check(entry(
                    len(ps), _ptr_array(ps), _ptr_array(grads), _ptr_array([st.get("master") for st in states]),
                    _ptr_array([st["exp_avg"] for st in states]), _ptr_array([st["exp_avg_sq"] for st in states]),
                    _ptr_array([st["step"] for st in states]), numel, i32(*[_DTYPES[p.dtype] for p in ps]),
                    i32(*[_DTYPES[g.dtype] for g in grads]), ticket, 0.0 if lr_dev else float(lr), float(b1), float(b2),
                    float(group["eps"]), float(group["weight_decay"]), lr_dev,
                    None if grad_scale is None else grad_scale.data_ptr(),
                    self._norm_out[1:].data_ptr() if clip else None,
                    None if found_inf is None else found_inf.data_ptr(),
                    self._norm_out[2:].data_ptr() if clip else None, *tail, _stream()), name)
            # the launch wrote the parameters through raw pointers: move their version counters the way an in-place torch op
            # would, so that whatever keys on them (the pool's inference caches, autograd's saved-tensor checks) sees the update
            torch.autograd.graph.increment_version(ps)
            if self.ema_decay is not None:
                self._ema_written(ps)
        if self.ema_decay is not None:
            self._ema_rest(lib, found_inf, self._norm_out[2:] if clip else None)
        return loss

    def _ema_written(self, ps):
        """Version counters of the output tensors an EmaModel reads, as for the parameters."""
        outs = [self._ema_out[p] if p in self._ema_out else self._ema_held[p] for p in ps if p in self._ema_held]
        if outs:
            torch.autograd.graph.increment_version(outs)

    def _ema_rest(self, lib, found_inf, found_inf2):
        """The averages of the parameters WITHOUT a gradient in this step: one ``aecf_ema_update`` (per device) under the same
        skip flags, so that every average moves on every step that is not skipped, and on none that is."""
        rest = {}
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None and p.numel() > 0 and p.device.type == "cuda" and p.dtype in _DTYPES and p.is_contiguous():
                    rest.setdefault(p.device, []).append(p)
        for dev, ps in rest.items():
            ema_dev = self.ema_decay if torch.is_tensor(self.ema_decay) else None
            for t in (ema_dev, found_inf, found_inf2):
                if t is not None and t.device != dev:
                    raise RuntimeError("FusedAdamW: ema_decay and the skip flags must live on the parameters' device")
            emas = [self._ema_state(p, self.state[p]) for p in ps]
            # the weight as stored: the float32 master of a 16-bit parameter where there is one
            srcs = [self.state[p].get("master") if p.dtype != torch.float32 else None for p in ps]
            srcs = [p if s is None else s for p, s in zip(ps, srcs)]
            i32 = ctypes.c_int32 * len(ps)
            with torch.cuda.device(dev):
                _lib.check(lib.aecf_ema_update(
                    len(ps), _ptr_array(srcs), i32(*[_DTYPES[s.dtype] for s in srcs]), _ptr_array(emas),
                    _ptr_array([self._ema_out.get(p) for p in ps]), i32(*[_DTYPES[p.dtype] for p in ps]),
                    (ctypes.c_int64 * len(ps))(*[p.numel() for p in ps]), 0.0 if ema_dev is not None else self.ema_decay,
                    None if ema_dev is None else ema_dev.data_ptr(), None if found_inf is None else found_inf.data_ptr(),
                    None if found_inf2 is None else found_inf2.data_ptr(), _stream()), "aecf_ema_update")
            self._ema_written(ps)


class EmaModel:
    """A copy of ``model`` whose parameters are the moving averages ``optimizer`` (a ``FusedAdamW(ema_decay=...)``) keeps: the
    momentum key encoder of MoCo (``k = ema.module(x)`` under ``no_grad``), the model to validate and ship.

    ``module``: ``copy.deepcopy(model)`` with ``requires_grad_(False)``.  Parameters pair by name.  A float32 parameter of the
    copy IS that parameter's ``state["ema"]`` (no second buffer); a 16-bit one is written by the step as ``ema.to(dtype)``
    beside the float32 ``state["ema"]``.  Parameters the optimiser does not hold, and all buffers, are copied from the model
    by ``sync()`` (buffers are copied, not averaged).  Build it once the model is on its device and BEFORE a step is captured
    (the graph holds the addresses); after replays of a graph of your own call ``after_replay()``, as ``invalidate_cast_cache()``
    is called on the model's pools (``xray.GraphedTrainStep`` does both)."""

    def __init__(self, model: torch.nn.Module, optimizer: FusedAdamW):
        if getattr(optimizer, "ema_decay", None) is None:
            raise ValueError("EmaModel: the optimiser keeps no average (FusedAdamW(..., ema_decay=...))")
        params = dict(model.named_parameters())
        if len({p.device for p in params.values()}) > 1:
            raise ValueError("EmaModel: the parameters of the model live on several devices")
        self.model, self.optimizer = model, optimizer
        self.module = copy.deepcopy(model).requires_grad_(False)
        held = {id(p) for group in optimizer.param_groups for p in group["params"]}
        copies = dict(self.module.named_parameters())
        self._unheld = []
        for name, p in params.items():
            if id(p) in held and p.numel() > 0 and p.dtype in _DTYPES:
                optimizer._bind_ema(p, copies[name])
            else:
                self._unheld.append((p, copies[name]))
        self._pools = tuple(m for m in self.module.modules() if hasattr(m, "invalidate_cast_cache"))
        optimizer._ema_models.append(self)
        self.sync()

    @torch.no_grad()
    def sync(self):
        """Copy what the optimiser does not average: the parameters it does not hold, and all buffers."""
        for p, q in self._unheld:
            q.copy_(p)
        for src, dst in zip(self.model.buffers(), self.module.buffers()):
            dst.copy_(src)

    def after_replay(self):
        """A graph replay moves no version counter: the copy's pools forget what inference derived from the old averages."""
        for pool in self._pools:
            pool.invalidate_cast_cache()

    def __call__(self, *args, **kwargs):
        return self.module(*args, **kwargs)
