"""The loss side of the AECF objective: the entropy regulariser of the reference
(``CurriculumMasking.entropy_loss``, ref aecf/AECFLayer.py:285-314) plus the contrastive term that
BASELINE.json's north_star names.

The contrastive term does NOT exist in the reference; it is build-defined here as
the symmetric InfoNCE of two views' fused embeddings, L2-normalised, with cross-batch negatives all-gathered
over the data-parallel group:

    L = 0.5 / B_all * sum_i [ CE(za_i . zb_all / T, i) + CE(zb_i . za_all / T, i) ]

All arithmetic (normalisation, logits GEMM, softmax / loss rows, both gradient GEMMs) runs in libaecf_hip.so;
the exchange steps are ``dp.all_gather_rows`` (forward) and its reduce-scatter (backward).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Union

import torch

from . import _lib, dp
from .layer import _DTYPES, _capturing, _ptr, _require_device, _stream, CurriculumMasking


def _plus(total: torch.Tensor, term: torch.Tensor) -> torch.Tensor:
    """total + term for two loss scalars whose dtypes may differ (a float32 InfoNCE term, a bf16 entropy regulariser): the
    addend is brought to the sum's dtype first.  torch's mixed-dtype elementwise kernel (the run-time cast variant) takes ~41 us
    for ONE element on this ROCm build against ~7 us for a same-dtype add (tools/debug/scalar_add_time.py) -- 1.4 % of the
    configs[2] step for a scalar."""
    if term.dtype != total.dtype and term.dim() == 0 and total.dim() == 0:
        term = term.to(torch.promote_types(total.dtype, term.dtype))
        total = total.to(term.dtype)
    return total + term


MIN_TEMPERATURE = 0.025     # the tile forms' bound: 1/T is the constant shift of every exponential (nce_gemm_supported)


def _temperature_arg(temperature, z: torch.Tensor, min_temperature: float):
    """A Python number -> float (the host path, as before).  A tensor -> itself, checked: one float32 element on z's device,
    read by the kernels (``max(T, min_temperature)``) with no host read, its gradient formed by the library's kernels."""
    if not isinstance(temperature, torch.Tensor):
        return float(temperature)
    if temperature.dtype != torch.float32:
        raise TypeError(f"aecf_amd: a tensor temperature must be float32, got {temperature.dtype}")
    if temperature.numel() != 1:
        raise ValueError(f"aecf_amd: a tensor temperature must hold one element, got shape {tuple(temperature.shape)}")
    if temperature.device != z.device:
        raise ValueError(f"aecf_amd: the temperature lives on {temperature.device}, the embeddings on {z.device}")
    _check_min_temperature(min_temperature)
    return temperature


def _check_min_temperature(min_temperature) -> None:
    if not (isinstance(min_temperature, (int, float)) and float(min_temperature) > 0.0):
        raise ValueError(f"aecf_amd: min_temperature must be a positive float, got {min_temperature!r}")


def _check_two_views(name: str, za: torch.Tensor, zb: torch.Tensor) -> None:
    if za.shape != zb.shape or za.dim() != 2:
        raise ValueError(f"{name} expects two [b, d] tensors of equal shape, got {tuple(za.shape)} and {tuple(zb.shape)}")


def _device_scalar(value, z: torch.Tensor) -> torch.Tensor:
    """A checked temperature or bias as the kernels read it: a tensor as it is, a float filled into one float32 element on z's
    device."""
    return value if isinstance(value, torch.Tensor) else torch.full((1,), value, dtype=torch.float32, device=z.device)


def _temperature_scalar(temperature, z: torch.Tensor, min_temperature: float) -> torch.Tensor:
    return _device_scalar(_temperature_arg(temperature, z, min_temperature), z)


# The data-parallel policy of the contrastive drivers.  Every rank of ``group`` must issue the same collectives in the same
# order -- a rank that took another form, or raised where the others went on, would leave them waiting -- so the drivers
# exchange their row counts, gather rows, agree on a refusal and form their return value through these.  (``info_nce`` keeps
# the count exchange it had: it gathers first and sends a default-dtype count, and that sequence is part of its behaviour.)

def _row_ranges(b_local: int, device, group):
    """``(sizes, offset, b_all)``: every rank's row count in rank order, this rank's first row among the gathered rows and their
    total, from one all-gather of an int64 element.  One rank: ``(None, 0, b_local)``, no collective."""
    rank, world = dp.world_info(group)
    if world == 1:
        return None, 0, b_local
    n = torch.tensor([b_local], device=device, dtype=torch.int64)
    got = [torch.zeros_like(n) for _ in range(world)]
    torch.distributed.all_gather(got, n, group=group)
    sizes = [int(v.item()) for v in got]
    return sizes, sum(sizes[:rank]), sum(sizes)


def _all_rows(x: torch.Tensor, group, sizes) -> torch.Tensor:
    """The rows of every rank (``sizes`` of ``_row_ranges``); on one rank x itself, with no copy."""
    return x if sizes is None else dp.all_gather_rows(x, group, sizes=sizes)


def _agreed_refusal(refusal: Optional[str], device, group) -> Optional[str]:
    """This rank's refusal of a form (None: it would run it) -> the group's: a MIN all-reduce of one flag, after which a rank
    that would have run while another refused refuses too.  One rank: the refusal as it came."""
    if dp.world_info(group)[1] > 1:
        flag = torch.tensor([1 if refusal is None else 0], device=device)
        torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN, group=group)
        if refusal is None and not bool(int(flag.item())):
            refusal = "the same on every rank (another rank refused it)"
    return refusal


def _dp_value(share: torch.Tensor, group) -> torch.Tensor:
    """This rank's rows' share of a global objective -> what the driver returns."""
    world = dp.world_info(group)[1]
    if world == 1:
        return share
    # Data-parallel convention (dp.FlatGradBucket.all_reduce(average=True)): gradients are AVERAGED over ranks, so
    # the local term carries a factor `world`; the returned VALUE is the global loss on every rank.
    total = share.detach().clone()
    torch.distributed.all_reduce(total, group=group)
    scaled = share * world
    return scaled + (total - scaled.detach())


class _L2Norm(torch.autograd.Function):
    """aecf_l2norm_forward / _backward: rows -> unit norm."""

    @staticmethod
    def forward(ctx, z, eps):
        lib = _lib.load()
        n, d = z.shape
        zc = z.contiguous()
        zn = torch.empty_like(zc)
        inv = torch.empty(n, dtype=torch.float32, device=z.device)
        _lib.check(lib.aecf_l2norm_forward(n, d, _DTYPES[z.dtype], eps, _ptr(zc), _ptr(zn), _ptr(inv), _stream()),
                   "aecf_l2norm_forward")
        ctx.save_for_backward(zn, inv)
        return zn

    @staticmethod
    def backward(ctx, dzn):
        lib = _lib.load()
        zn, inv = ctx.saved_tensors
        n, d = zn.shape
        g = dzn.to(torch.float32).contiguous()
        dz = torch.empty_like(zn)
        _lib.check(lib.aecf_l2norm_backward(n, d, _DTYPES[zn.dtype], _ptr(zn), _ptr(inv), _ptr(g), _ptr(dz), _stream()),
                   "aecf_l2norm_backward")
        return dz, None


class _NceDirection(torch.autograd.Function):
    """aecf_nce_fwd_bwd: sum_i [logsumexp_j(q_i.k_j/T) - q_i.k_{off+i}/T] * coef for local unit-norm q against all k.
    Forward and both gradients come out of the same call (the gradients are linear in the upstream scalar).  A tensor
    temperature runs aecf_nce_fwd_bwd_dt, which also forms dL/dT."""

    @staticmethod
    def forward(ctx, q, k_all, row_offset, temperature, coef, low_memory=False, min_temperature=MIN_TEMPERATURE):
        lib = _lib.load()
        rows, d = q.shape
        cols = k_all.shape[0]
        dt = q.dtype
        qc, kc = q.contiguous(), k_all.to(dt).contiguous()
        dev = q.device
        loss_rows = torch.empty(rows, dtype=torch.float32, device=dev)
        dq = torch.empty(rows, d, dtype=torch.float32, device=dev)
        dk = torch.empty(cols, d, dtype=torch.float32, device=dev)
        # the workspace handed over selects the implementation (include/aecf_hip.h): rows x cols bf16 -> tile GEMMs,
        # O(rows d) -> the streaming form
        ws_bytes = lib.aecf_nce_stream_workspace_bytes(rows, cols, d, _DTYPES[dt]) if low_memory else 0
        if ws_bytes == 0:
            if low_memory:
                raise NotImplementedError(f"aecf_amd: no streaming InfoNCE for dtype {dt}, d = {d}")
            ws_bytes = lib.aecf_nce_workspace_bytes(rows, cols, d, _DTYPES[dt])
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        d_t = None
        if isinstance(temperature, torch.Tensor):
            d_t = torch.empty(1, dtype=torch.float32, device=dev) if ctx.needs_input_grad[3] else None
            _lib.check(lib.aecf_nce_fwd_bwd_dt(rows, cols, row_offset, d, _DTYPES[dt], _ptr(temperature), float(min_temperature),
                                               coef, _ptr(qc), _ptr(kc), _ptr(loss_rows), _ptr(dq), _ptr(dk), _ptr(d_t), _ptr(ws),
                                               ws_bytes, _stream()), "aecf_nce_fwd_bwd_dt")
            ctx.t_shape = temperature.shape
        else:
            _lib.check(lib.aecf_nce_fwd_bwd(rows, cols, row_offset, d, _DTYPES[dt], temperature, coef, _ptr(qc), _ptr(kc),
                                            _ptr(loss_rows), _ptr(dq), _ptr(dk), _ptr(ws), ws_bytes, _stream()),
                       "aecf_nce_fwd_bwd")
        ctx.save_for_backward(dq, dk, d_t)
        ctx.dtypes = (q.dtype, k_all.dtype)
        return loss_rows.sum() * coef

    @staticmethod
    def backward(ctx, dloss):
        dq, dk, d_t = ctx.saved_tensors
        g = dloss.to(torch.float32)
        g_t = (d_t * g).reshape(ctx.t_shape) if d_t is not None else None
        return (dq * g).to(ctx.dtypes[0]), (dk * g).to(ctx.dtypes[1]), None, g_t, None, None, None


class _NceSymmetric(torch.autograd.Function):
    """aecf_nce_sym_pass1 / _loss / _grads: BOTH directions of the symmetric InfoNCE from one block of logits (local rows of view a
    against the gathered rows of view b).  The column sums of the exponentials are the one thing ranks exchange (one
    all-reduce of `cols` floats between pass 1 and the loss); the gradient on the gathered keys is this rank's share (the
    caller's all-gather backward reduce-scatters it).  The forward runs the logits pass and the loss; the two gradient products
    run in the backward, scaled on the device by the gradient that arrives there and written in the inputs' dtype (no float32
    [cols, d] intermediate, no multiply / cast passes).  Optionally carries CurriculumMasking.entropy_loss (ref
    aecf/AECFLayer.py:285-314) in the loss launch.  Returns (this rank's rows' share of the loss, entropy loss).
    A tensor temperature runs the _dt calls: T is read on the device, and the backward returns dL/dT -- this rank's share
    (-(1/T) sum_i a_i.da_i over its rows, which sum to the global value over ranks) times ``t_grad_scale``."""

    @staticmethod
    def forward(ctx, a, b_all, entropy, row_offset, temperature, coef, group, last_seq_len, entropy_target,
                min_temperature=MIN_TEMPERATURE, t_grad_scale=1.0):
        lib = _lib.load()
        rows, d = a.shape
        cols = b_all.shape[0]
        dev = a.device
        ac, bc = a.detach().to(torch.bfloat16).contiguous(), b_all.detach().to(torch.bfloat16).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        ws_bytes = lib.aecf_nce_sym_workspace_bytes(rows, cols, d)
        if ws_bytes == 0:
            raise NotImplementedError(f"aecf_amd: symmetric InfoNCE needs d % 64 == 0, got d = {d}")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        col_sums = torch.empty(cols, **f32)
        dev_t = isinstance(temperature, torch.Tensor)
        if dev_t:
            tp, t_min = _ptr(temperature), float(min_temperature)
            _lib.check(lib.aecf_nce_sym_pass1_dt(rows, cols, d, tp, t_min, _ptr(ac), _ptr(bc), _ptr(ws), ws_bytes, _ptr(col_sums),
                                                 _stream()), "aecf_nce_sym_pass1_dt")
        else:
            _lib.check(lib.aecf_nce_sym_pass1(rows, cols, d, temperature, _ptr(ac), _ptr(bc), _ptr(ws), ws_bytes, _ptr(col_sums),
                                              _stream()), "aecf_nce_sym_pass1")
        if dp.world_info(group)[1] > 1:
            torch.distributed.all_reduce(col_sums, group=group)
        loss_rows = torch.empty(rows, **f32)
        if entropy is not None:
            ent = entropy.detach().to(torch.float32).contiguous().reshape(-1)
            ent_loss, dent = torch.zeros(1, **f32), torch.empty(ent.numel(), **f32)
            n_ent, p_ent, p_el, p_de = ent.numel(), _ptr(ent), _ptr(ent_loss), _ptr(dent)
        else:
            ent_loss, dent, n_ent, p_ent, p_el, p_de = torch.zeros(1, **f32), None, 0, None, None, None
        if dev_t:
            _lib.check(lib.aecf_nce_sym_loss_dt(rows, cols, row_offset, d, tp, t_min, _ptr(ac), _ptr(bc), _ptr(col_sums), _ptr(ws),
                                                ws_bytes, _ptr(loss_rows), n_ent, last_seq_len, entropy_target, p_ent, 1.0, p_el, p_de,
                                                _stream()), "aecf_nce_sym_loss_dt")
        else:
            _lib.check(lib.aecf_nce_sym_loss(rows, cols, row_offset, d, temperature, _ptr(ac), _ptr(bc), _ptr(col_sums), _ptr(ws),
                                             ws_bytes, _ptr(loss_rows), n_ent, last_seq_len, entropy_target, p_ent, 1.0, p_el, p_de,
                                             _stream()), "aecf_nce_sym_loss")
        # (a device temperature is kept as a tensor: the backward reads it where it lives)
        ctx.save_for_backward(ac, bc, ws, temperature.detach() if dev_t else None, *([dent] if dent is not None else []))
        ctx.meta = (a.dtype, b_all.dtype, None if entropy is None else (entropy.dtype, entropy.shape),
                    (rows, cols, int(row_offset), d, None if dev_t else float(temperature), float(coef), ws_bytes))
        ctx.dev_t = (temperature.shape, float(min_temperature), float(t_grad_scale)) if dev_t else None
        return loss_rows.sum() * coef, ent_loss.reshape(())

    @staticmethod
    def backward(ctx, d_nce, d_ent):
        lib = _lib.load()
        ac, bc, ws, t_dev = ctx.saved_tensors[:4]
        ad, bd, em, (rows, cols, row_offset, d, temperature, coef, ws_bytes) = ctx.meta
        if getattr(ctx, "_spent", False):
            raise RuntimeError("aecf_amd: the symmetric InfoNCE backward runs once per forward (it consumes the stored logits)")
        ctx._spent = True
        gdt = torch.bfloat16 if (ad == torch.bfloat16 and bd == torch.bfloat16) else torch.float32
        da = torch.empty(rows, d, dtype=gdt, device=ac.device)
        db = torch.empty(cols, d, dtype=gdt, device=ac.device)
        up = d_nce.detach().to(torch.float32).reshape(1).contiguous()
        g_t = None
        if ctx.dev_t is not None:
            t_shape, t_min, t_scale = ctx.dev_t
            d_t = torch.empty(1, dtype=torch.float32, device=ac.device) if ctx.needs_input_grad[4] else None
            _lib.check(lib.aecf_nce_sym_grads_dt(rows, cols, row_offset, d, _ptr(t_dev), t_min, coef, _ptr(ac), _ptr(bc), _ptr(ws),
                                                 ws_bytes, _ptr(up), _DTYPES[gdt], _ptr(da), _ptr(db), _ptr(d_t), _stream()),
                       "aecf_nce_sym_grads_dt")
            if d_t is not None:
                g_t = (d_t * t_scale if t_scale != 1.0 else d_t).reshape(t_shape)
        else:
            _lib.check(lib.aecf_nce_sym_grads(rows, cols, row_offset, d, temperature, coef, _ptr(ac), _ptr(bc), _ptr(ws), ws_bytes,
                                              _ptr(up), _DTYPES[gdt], _ptr(da), _ptr(db), _stream()), "aecf_nce_sym_grads")
        g_ent = None
        if em is not None:
            g_ent = (ctx.saved_tensors[4] * d_ent.to(torch.float32)).reshape(em[1]).to(em[0])
        return da.to(ad), db.to(bd), g_ent, None, g_t, None, None, None, None, None, None


def _sym_supported(z: torch.Tensor, temperature, cols: Optional[int] = None, min_temperature: float = MIN_TEMPERATURE) -> bool:
    """The tile-GEMM form applies (bf16, d % 64 == 0, 1/T a safe exponent shift) AND its workspace -- rows x cols bf16 -- fits
    comfortably in what the device has free; otherwise the callers take the streaming kernels (O(rows d) workspace).  A tensor
    temperature is never read here: its bound is min_temperature (the kernels use max(T, min_temperature))."""
    bound = min_temperature if isinstance(temperature, torch.Tensor) else temperature
    if not (z.dtype == torch.bfloat16 and z.shape[1] % 64 == 0 and bound >= MIN_TEMPERATURE):
        return False
    if cols is not None and z.is_cuda:
        need = _lib.load().aecf_nce_sym_workspace_bytes(z.shape[0], cols, z.shape[1])
        free, _ = torch.cuda.mem_get_info(z.device)
        if need > 0.6 * free:
            return False
    return True


def _stream_form(z: torch.Tensor, cols: int) -> bool:
    """True when the streaming InfoNCE kernels (no [rows, cols] logits in memory) exist for z's dtype and width."""
    if z.dtype not in _DTYPES or not z.is_cuda:
        return False
    return _lib.load().aecf_nce_stream_workspace_bytes(z.shape[0], cols, z.shape[1], _DTYPES[z.dtype]) > 0


class _LossDirection(torch.autograd.Function):
    """aecf_loss_fwd_bwd: ONE call for one InfoNCE direction (streaming form: no [rows, cols] logits) AND the entropy
    regulariser of the reference (CurriculumMasking.entropy_loss, ref aecf/AECFLayer.py:285-314) with their gradients
    -- BASELINE.json north_star's "second fused kernel".  Returns (contrastive share, entropy loss).  A tensor temperature
    runs aecf_loss_fwd_bwd_dt, which also forms dL/dT."""

    @staticmethod
    def forward(ctx, q, k_all, entropy, row_offset, temperature, coef, last_seq_len, entropy_target,
                min_temperature=MIN_TEMPERATURE):
        lib = _lib.load()
        rows, d = q.shape
        cols = k_all.shape[0]
        dev = q.device
        qc, kc = q.detach().to(torch.bfloat16).contiguous(), k_all.detach().to(torch.bfloat16).contiguous()
        ent = entropy.detach().to(torch.float32).contiguous().reshape(-1)
        f32 = dict(dtype=torch.float32, device=dev)
        loss_rows, dq, dk = torch.empty(rows, **f32), torch.empty(rows, d, **f32), torch.empty(cols, d, **f32)
        ent_loss, dent = torch.empty(1, **f32), torch.empty(ent.numel(), **f32)
        # this operator is the fallback of the symmetric tile-GEMM form (too little free memory for rows x cols bf16, or a
        # temperature its constant-shift softmax does not take): hand over the STREAMING workspace (O(rows d)) where that
        # kernel exists, so that the fallback never allocates more than the form it replaces
        ws_bytes = lib.aecf_nce_stream_workspace_bytes(rows, cols, d, _lib.AECF_BF16)
        if ws_bytes == 0:
            ws_bytes = lib.aecf_nce_workspace_bytes(rows, cols, d, _lib.AECF_BF16)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        d_t = None
        if isinstance(temperature, torch.Tensor):
            d_t = torch.empty(1, **f32) if ctx.needs_input_grad[4] else None
            _lib.check(lib.aecf_loss_fwd_bwd_dt(rows, cols, row_offset, d, _ptr(temperature), float(min_temperature), coef,
                                                _ptr(qc), _ptr(kc), _ptr(loss_rows), _ptr(dq), _ptr(dk), _ptr(d_t), ent.numel(),
                                                last_seq_len, entropy_target, _ptr(ent), 1.0, _ptr(ent_loss), _ptr(dent), _ptr(ws),
                                                ws_bytes, _stream()), "aecf_loss_fwd_bwd_dt")
            ctx.t_shape = temperature.shape
        else:
            _lib.check(lib.aecf_loss_fwd_bwd(rows, cols, row_offset, d, temperature, coef, _ptr(qc), _ptr(kc), _ptr(loss_rows),
                                             _ptr(dq), _ptr(dk), ent.numel(), last_seq_len, entropy_target, _ptr(ent), 1.0,
                                             _ptr(ent_loss), _ptr(dent), _ptr(ws), ws_bytes, _stream()), "aecf_loss_fwd_bwd")
        ctx.save_for_backward(dq, dk, dent, d_t)
        ctx.meta = (q.dtype, k_all.dtype, entropy.dtype, entropy.shape)
        return loss_rows.sum() * coef, ent_loss.reshape(())

    @staticmethod
    def backward(ctx, d_nce, d_ent):
        dq, dk, dent, d_t = ctx.saved_tensors
        qd, kd, ed, eshape = ctx.meta
        g = d_nce.to(torch.float32)
        g_t = (d_t * g).reshape(ctx.t_shape) if d_t is not None else None
        return ((dq * g).to(qd), (dk * g).to(kd), (dent * d_ent.to(torch.float32)).reshape(eshape).to(ed),
                None, g_t, None, None, None, None)


def contrastive_entropy_loss(za: torch.Tensor, zb: torch.Tensor, masking: CurriculumMasking, entropy: torch.Tensor,
                             temperature: Union[float, torch.Tensor] = 0.07, entropy_weight: float = 0.01,
                             contrastive_weight: float = 1.0, min_temperature: float = MIN_TEMPERATURE) -> torch.Tensor:
    """``contrastive_weight * info_nce(za, zb) + entropy_weight * masking.entropy_loss(entropy)`` (single rank, bf16
    embeddings) with the entropy regulariser riding in the launch of the first InfoNCE direction (aecf_loss_fwd_bwd).
    ``temperature`` / ``min_temperature``: as for ``info_nce``."""
    _require_device(za, "za")
    if za.shape != zb.shape or za.dim() != 2:
        raise ValueError(f"expected two [b, d] tensors of equal shape, got {tuple(za.shape)} and {tuple(zb.shape)}")
    t = _temperature_arg(temperature, za, min_temperature)
    na, nb = l2_normalize(za), l2_normalize(zb)
    coef = 0.5 / float(za.shape[0])
    seq_len = masking._last_seq_len if hasattr(masking, "_last_seq_len") else 2
    if _sym_supported(za, t, za.shape[0], min_temperature):
        l_nce, l_ent = _NceSymmetric.apply(na, nb, entropy, 0, t, coef, None, int(seq_len), float(masking.entropy_target),
                                           min_temperature, 1.0)
        return _plus(contrastive_weight * l_nce, entropy_weight * l_ent.to(za.dtype))
    l_ab, l_ent = _LossDirection.apply(na, nb, entropy, 0, t, coef, int(seq_len), float(masking.entropy_target), min_temperature)
    l_ba = _NceDirection.apply(nb, na, 0, t, coef, _stream_form(nb, na.shape[0]), min_temperature)
    return _plus(contrastive_weight * (l_ab + l_ba), entropy_weight * l_ent.to(za.dtype))


def gathered_contrastive_entropy_loss(za: torch.Tensor, nb_all: torch.Tensor, row_offset: int, masking: CurriculumMasking,
                                      entropy: torch.Tensor, temperature: Union[float, torch.Tensor] = 0.07,
                                      entropy_weight: float = 0.01, contrastive_weight: float = 1.0, group=None,
                                      min_temperature: float = MIN_TEMPERATURE) -> torch.Tensor:
    """The loss side of a data-parallel step in ONE operator: this rank's rows ``za`` [b_local, d] (bf16, not yet normalised)
    against the unit-norm rows of the other view from EVERY rank ``nb_all`` [b_all, d] (``dp.all_gather_rows(l2_normalize(zb))``:
    its backward reduce-scatters the share of the gradient this call returns), positives at ``row_offset + i``; both InfoNCE
    directions from the one block of logits (``aecf_nce_sym_pass1`` / ``_loss`` / ``_grads``; the column sums are all-reduced over ``group`` between
    the passes) plus ``entropy_weight * masking.entropy_loss(entropy)`` riding in the same call.  Returns this rank's share of
    ``contrastive_weight * L_nce`` (coef = 0.5 / b_all) plus the entropy term.

    A tensor ``temperature`` (as for ``info_nce``, ``min_temperature >= 0.025``) gets the gradient ``world * (this rank's share
    of dL/dT)``: the gradient average of the training loop (``dp.all_reduce_grads``) then leaves the one-rank gradient of the
    global objective on a replicated temperature -- the convention ``info_nce`` follows for every input."""
    _require_device(za, "za")
    t = _temperature_arg(temperature, za, min_temperature)
    if not _sym_supported(za, t, None, min_temperature):
        if isinstance(t, torch.Tensor):
            raise NotImplementedError("aecf_amd: the gathered contrastive loss needs bfloat16 rows with d % 64 == 0 and "
                                      "min_temperature >= 0.025 for a tensor temperature")
        raise NotImplementedError("aecf_amd: the gathered contrastive loss needs bfloat16 rows with d % 64 == 0 and temperature >= 0.025")
    na = l2_normalize(za)
    coef = 0.5 / float(nb_all.shape[0])
    seq_len = masking._last_seq_len if hasattr(masking, "_last_seq_len") else 2
    world = dp.world_info(group)[1] if isinstance(t, torch.Tensor) else 1
    l_nce, l_ent = _NceSymmetric.apply(na, nb_all, entropy, int(row_offset), t, coef, group, int(seq_len),
                                       float(masking.entropy_target), min_temperature, float(world))
    return _plus(contrastive_weight * l_nce, entropy_weight * l_ent.to(za.dtype))


def l2_normalize(z: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    _require_device(z, "z")
    return _L2Norm.apply(z, float(eps))


def info_nce(za: torch.Tensor, zb: torch.Tensor, temperature: Union[float, torch.Tensor] = 0.07, group=None,
             min_temperature: float = MIN_TEMPERATURE) -> torch.Tensor:
    """Symmetric InfoNCE between the local rows of two views with negatives from every rank of ``group``.
    ``za``, ``zb``: [b_local, d] on a ROCm device.  bfloat16 with d % 64 == 0 (temperature >= 0.025) runs the symmetric tile-GEMM
    form: both directions from ONE block of logits, exponentials kept as bf16 [b_local, b_all] (any row counts); float32:
    d % 64 == 0 and total rows over ranks % 64 == 0.

    ``temperature``: a Python float, or a learnable one -- a one-element float32 tensor on za's device, e.g.
    ``1 / logit_scale.exp()``.  A tensor is read by the kernels on the device (no host read: a captured step replays its current
    value) as ``max(T, min_temperature)``, and its gradient (zero where ``T < min_temperature``) comes from the same kernels.
    The form is chosen from the dtype, d, memory and ``min_temperature`` (below 0.025: the streaming form), never from T."""
    _require_device(za, "za")
    _require_device(zb, "zb")
    _check_two_views("info_nce", za, zb)
    if za.dtype not in _DTYPES:
        raise NotImplementedError(f"aecf_amd: dtype {za.dtype} is not supported (bfloat16 / float32 only)")
    t = _temperature_arg(temperature, za, min_temperature)
    rank, world = dp.world_info(group)
    na, nb = l2_normalize(za), l2_normalize(zb)
    nb_all = dp.all_gather_rows(nb, group) if world > 1 else nb
    b_all = nb_all.shape[0]
    # every rank must take the same form (they exchange different things)
    sym = _agreed_refusal(None if _sym_supported(za, t, b_all, min_temperature) else "no symmetric form", za.device, group) is None
    if world > 1:
        sizes = torch.tensor([za.shape[0]], device=za.device)
        all_sizes = [torch.zeros_like(sizes) for _ in range(world)]
        torch.distributed.all_gather(all_sizes, sizes, group=group)
        offset = int(sum(int(s.item()) for s in all_sizes[:rank]))
    else:
        offset = 0
    coef = 0.5 / float(b_all)
    if sym:
        # both directions from the one block of logits this rank owns (its rows of view a against every row of view b):
        # view a is never gathered, one all-reduce of b_all floats replaces the second direction's pass
        share, _ = _NceSymmetric.apply(na, nb_all, None, offset, t, coef, group, 2, 0.0, min_temperature, 1.0)
    else:
        na_all = dp.all_gather_rows(na, group) if world > 1 else na
        # (the symmetric form was refused -- memory, temperature or dtype: the streaming kernels where they exist, never
        #  a second rows x cols allocation per direction)
        low = _stream_form(na, b_all)
        l_ab = _NceDirection.apply(na, nb_all, offset, t, coef, low, min_temperature)
        l_ba = _NceDirection.apply(nb, na_all, offset, t, coef, low, min_temperature)
        share = l_ab + l_ba              # this rank's rows' share of the global objective
    return _dp_value(share, group)


MULTIVIEW_MAX_VIEWS = 8     # the pair table of the logits launch holds the 28 pairs of 8 views


def multiview_pairs(views: int, anchor: Optional[int] = None):
    """The pairs (m, n), m < n, of ``multiview_info_nce`` in the order the library walks them: every pair in lexicographic
    order, or -- with an anchor view k -- (min(k, n), max(k, n)) for every n != k, n rising."""
    if anchor is None:
        return [(m, n) for m in range(views) for n in range(m + 1, views)]
    return [(min(anchor, n), max(anchor, n)) for n in range(views) if n != anchor]


def _spend(ctx, what: str) -> None:
    """The backward of a tile form overwrites the logits its forward stored: it runs once, a second call is refused."""
    if getattr(ctx, "_spent", False):
        raise RuntimeError(f"aecf_amd: the {what} backward runs once per forward (it consumes the stored logits)")
    ctx._spent = True


def _multiview_buffers(workspace_bytes, x: torch.Tensor, x_all: torch.Tensor, anchor: int):
    """What the two multi-view forwards hand their launches: ``(xc, xa, ws, ws_bytes, col_sums, loss_rows)`` -- the rows as the
    kernels read them, the workspace the library's query asks for, the [P, cols] column sums and the [P, rows] loss rows."""
    rows, views, d = x.shape
    cols = x_all.shape[0]
    pairs = len(multiview_pairs(views, None if anchor < 0 else anchor))
    f32 = dict(dtype=torch.float32, device=x.device)
    ws_bytes = workspace_bytes(rows, cols, d, views, anchor)
    if ws_bytes == 0:
        raise NotImplementedError(f"aecf_amd: multi-view InfoNCE needs d % 64 == 0, 64 <= d <= 4096, 2 to 8 views and fewer than "
                                  f"2^31 gathered rows; got d = {d}, {views} views, {cols} rows")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    return (x.detach().contiguous(), x_all.detach().contiguous(), ws, ws_bytes, torch.empty(pairs, cols, **f32),
            torch.empty(pairs, rows, **f32))


def _multiview_grad_buffers(ctx, xc: torch.Tensor, xa: torch.Tensor, d_loss: torch.Tensor, wants_dt: bool):
    """What the two multi-view backwards hand their one call, which runs once per forward: ``(dx, dx_all, up, d_t)``."""
    _spend(ctx, "multi-view InfoNCE")
    dx, dx_all = torch.empty_like(xc, dtype=torch.bfloat16), torch.empty_like(xa, dtype=torch.bfloat16)
    up = d_loss.detach().to(torch.float32).reshape(1).contiguous()
    return dx, dx_all, up, torch.empty(1, dtype=torch.float32, device=xc.device) if wants_dt else None


class _NceMultiView(torch.autograd.Function):
    """aecf_nce_multi_pass1 / _loss / _grads: the symmetric InfoNCE of every pair of views of x [rows, M, d] (unit-norm bf16 rows,
    read in place), modelled on ``_NceSymmetric``.  One logits launch for all P pair blocks; the [P, cols] column sums are the
    one thing ranks exchange (one all-reduce); the backward runs the weights pass and ONE gradient product per role, whose K loop
    walks every partner block of a view: a gradient element is one float32 sum over all its partners, rounded once.  The
    gradient on the gathered rows is this rank's share.  The temperature is a one-element float32 device tensor; the backward
    returns this rank's share of dL/dT."""

    @staticmethod
    def forward(ctx, x, x_all, row_offset, temperature, coef, group, min_temperature, anchor):
        lib = _lib.load()
        rows, views, d = x.shape
        cols = x_all.shape[0]
        xc, xa, ws, ws_bytes, col_sums, loss_rows = _multiview_buffers(lib.aecf_nce_multi_workspace_bytes, x, x_all, anchor)
        t = temperature.detach()
        tp, t_min = _ptr(t), float(min_temperature)
        _lib.check(lib.aecf_nce_multi_pass1(rows, cols, d, views, anchor, tp, t_min, _ptr(xc), _ptr(xa), _ptr(ws), ws_bytes,
                                            _ptr(col_sums), _stream()), "aecf_nce_multi_pass1")
        if dp.world_info(group)[1] > 1:
            torch.distributed.all_reduce(col_sums, group=group)
        _lib.check(lib.aecf_nce_multi_loss(rows, cols, int(row_offset), d, views, anchor, tp, t_min, _ptr(xc), _ptr(xa), _ptr(col_sums),
                                           _ptr(ws), ws_bytes, _ptr(loss_rows), _stream()), "aecf_nce_multi_loss")
        ctx.save_for_backward(xc, xa, ws, t)
        ctx.meta = (temperature.shape, (rows, cols, int(row_offset), d, views, anchor, float(coef), t_min, ws_bytes))
        return loss_rows.sum() * coef

    @staticmethod
    def backward(ctx, d_loss):
        lib = _lib.load()
        xc, xa, ws, t = ctx.saved_tensors
        t_shape, (rows, cols, row_offset, d, views, anchor, coef, t_min, ws_bytes) = ctx.meta
        dx, dx_all, up, d_t = _multiview_grad_buffers(ctx, xc, xa, d_loss, ctx.needs_input_grad[3])
        _lib.check(lib.aecf_nce_multi_grads(rows, cols, row_offset, d, views, anchor, _ptr(t), t_min, coef, _ptr(xc), _ptr(xa), _ptr(ws),
                                            ws_bytes, _ptr(up), _DTYPES[torch.bfloat16], _ptr(dx), _ptr(dx_all), _ptr(d_t), _stream()),
                   "aecf_nce_multi_grads")
        g_t = d_t.reshape(t_shape) if d_t is not None else None
        return dx, dx_all, None, g_t, None, None, None, None


class _L2NormMaskedSlots(torch.autograd.Function):
    """aecf_l2norm_masked_forward / _backward over the slots of x [rows * views, d]: a present slot is ``_L2Norm``'s, an absent one
    (``mask`` [rows * views] uint8, non-zero) comes out as zeros whatever it holds and gets a zero gradient.  Also returns the
    presence byte of every row (bit v: view v present), packed in the same launch."""

    @staticmethod
    def forward(ctx, z, mask, views, eps):
        lib = _lib.load()
        n, d = z.shape
        zc = z.contiguous()
        zn = torch.empty_like(zc)
        inv = torch.empty(n, dtype=torch.float32, device=z.device)
        pres = torch.empty(n // views, dtype=torch.uint8, device=z.device)
        _lib.check(lib.aecf_l2norm_masked_forward(n, d, views, _DTYPES[z.dtype], eps, _ptr(zc), _ptr(mask), _ptr(zn), _ptr(inv), _ptr(pres),
                                                  _stream()), "aecf_l2norm_masked_forward")
        ctx.save_for_backward(zn, inv, mask)
        ctx.mark_non_differentiable(pres)
        return zn, pres

    @staticmethod
    def backward(ctx, dzn, _):
        lib = _lib.load()
        zn, inv, mask = ctx.saved_tensors
        n, d = zn.shape
        g = dzn.to(torch.float32).contiguous()
        dz = torch.empty_like(zn)
        _lib.check(lib.aecf_l2norm_masked_backward(n, d, _DTYPES[zn.dtype], _ptr(zn), _ptr(inv), _ptr(g), _ptr(mask), _ptr(dz), _stream()),
                   "aecf_l2norm_masked_backward")
        return dz, None, None, None


class _NceMultiViewMasked(torch.autograd.Function):
    """aecf_nce_multi_masked_pair_coef / _pass1 / _loss / _grads: ``_NceMultiView`` where a row may lack views.  ``pres`` [rows] /
    ``pres_all`` [cols] are the presence bytes (bit v: view v present); pair p runs over the rows holding both its views and
    weighs 0.5 / n_p / P', formed on the device from the gathered bytes -- nothing is read on the host.  The gradient products,
    the dT sum and the slab sum are ``_NceMultiView``'s kernels."""

    @staticmethod
    def forward(ctx, x, x_all, pres, pres_all, row_offset, temperature, group, min_temperature, anchor):
        lib = _lib.load()
        rows, views, d = x.shape
        cols = x_all.shape[0]
        xc, xa, ws, ws_bytes, col_sums, loss_rows = _multiview_buffers(lib.aecf_nce_multi_masked_workspace_bytes, x, x_all, anchor)
        pair_coef = torch.empty(col_sums.shape[0], dtype=torch.float32, device=x.device)
        t = temperature.detach()
        tp, t_min = _ptr(t), float(min_temperature)
        _lib.check(lib.aecf_nce_multi_masked_pair_coef(cols, views, anchor, _ptr(pres_all), _ptr(pair_coef), _stream()),
                   "aecf_nce_multi_masked_pair_coef")
        _lib.check(lib.aecf_nce_multi_masked_pass1(rows, cols, d, views, anchor, tp, t_min, _ptr(xc), _ptr(xa), _ptr(pres), _ptr(pres_all),
                                                   _ptr(ws), ws_bytes, _ptr(col_sums), _stream()), "aecf_nce_multi_masked_pass1")
        if dp.world_info(group)[1] > 1:
            torch.distributed.all_reduce(col_sums, group=group)
        _lib.check(lib.aecf_nce_multi_masked_loss(rows, cols, int(row_offset), d, views, anchor, tp, t_min, _ptr(xc), _ptr(xa), _ptr(pres),
                                                  _ptr(pres_all), _ptr(col_sums), _ptr(ws), ws_bytes, _ptr(loss_rows), _stream()),
                   "aecf_nce_multi_masked_loss")
        ctx.save_for_backward(xc, xa, ws, t, pair_coef, pres)
        ctx.meta = (temperature.shape, (rows, cols, int(row_offset), d, views, anchor, t_min, ws_bytes))
        return (loss_rows.sum(dim=1) * pair_coef).sum()

    @staticmethod
    def backward(ctx, d_loss):
        lib = _lib.load()
        xc, xa, ws, t, pair_coef, pres = ctx.saved_tensors
        t_shape, (rows, cols, row_offset, d, views, anchor, t_min, ws_bytes) = ctx.meta
        dx, dx_all, up, d_t = _multiview_grad_buffers(ctx, xc, xa, d_loss, ctx.needs_input_grad[5])
        _lib.check(lib.aecf_nce_multi_masked_grads(rows, cols, row_offset, d, views, anchor, _ptr(t), t_min, _ptr(pair_coef), _ptr(xc),
                                                   _ptr(xa), _ptr(pres), _ptr(ws), ws_bytes, _ptr(up), _DTYPES[torch.bfloat16], _ptr(dx),
                                                   _ptr(dx_all), _ptr(d_t), _stream()), "aecf_nce_multi_masked_grads")
        g_t = d_t.reshape(t_shape) if d_t is not None else None
        return dx, dx_all, None, None, None, g_t, None, None, None


class _NceMultiViewPairwise(torch.autograd.Function):
    """aecf_nce_multi_pp_pair_coef / _pass1 / _loss / _grads: ``_NceMultiView`` (``pres`` None) or ``_NceMultiViewMasked`` with a
    temperature and a weight per pair.  ``temperatures`` [P] float32 on the device, read there as ``max(T_p, min_temperature)``;
    ``weights`` [P] float32 on the device or None (uniform), normalised there over the pairs that have a row.  Where the
    temperatures want a gradient the logits launch also leaves the per-pair sums of E (s - 1), and the backward forms this rank's
    share of every dL/dT_p from them -- the gradient products are the one-temperature form's, in their plain form."""

    @staticmethod
    def forward(ctx, x, x_all, pres, pres_all, row_offset, temperatures, weights, group, min_temperature, anchor):
        lib = _lib.load()
        rows, views, d = x.shape
        cols = x_all.shape[0]
        xc, xa, ws, ws_bytes, col_sums, loss_rows = _multiview_buffers(lib.aecf_nce_multi_pp_workspace_bytes, x, x_all, anchor)
        pair_coef = torch.empty(col_sums.shape[0], dtype=torch.float32, device=x.device)
        t = temperatures.detach().contiguous()
        tp, t_min, with_dt = _ptr(t), float(min_temperature), int(bool(ctx.needs_input_grad[5]))
        pl, pa = (_ptr(pres), _ptr(pres_all)) if pres is not None else (None, None)
        _lib.check(lib.aecf_nce_multi_pp_pair_coef(cols, views, anchor, pa, _ptr(weights), _ptr(pair_coef), _stream()),
                   "aecf_nce_multi_pp_pair_coef")
        _lib.check(lib.aecf_nce_multi_pp_pass1(rows, cols, d, views, anchor, tp, t_min, _ptr(xc), _ptr(xa), pl, pa, with_dt, _ptr(ws),
                                               ws_bytes, _ptr(col_sums), _stream()), "aecf_nce_multi_pp_pass1")
        if dp.world_info(group)[1] > 1:
            torch.distributed.all_reduce(col_sums, group=group)
        _lib.check(lib.aecf_nce_multi_pp_loss(rows, cols, int(row_offset), d, views, anchor, tp, t_min, _ptr(xc), _ptr(xa), pl, pa,
                                              _ptr(col_sums), _ptr(ws), ws_bytes, _ptr(loss_rows), _stream()), "aecf_nce_multi_pp_loss")
        ctx.save_for_backward(xc, xa, ws, t, pair_coef, pres)
        ctx.meta = (temperatures.shape, (rows, cols, int(row_offset), d, views, anchor, t_min, ws_bytes))
        return (loss_rows.sum(dim=1) * pair_coef).sum()

    @staticmethod
    def backward(ctx, d_loss):
        lib = _lib.load()
        xc, xa, ws, t, pair_coef, pres = ctx.saved_tensors
        t_shape, (rows, cols, row_offset, d, views, anchor, t_min, ws_bytes) = ctx.meta
        dx, dx_all, up, _ = _multiview_grad_buffers(ctx, xc, xa, d_loss, False)
        d_t = torch.empty(t.shape, dtype=torch.float32, device=xc.device) if ctx.needs_input_grad[5] else None
        _lib.check(lib.aecf_nce_multi_pp_grads(rows, cols, row_offset, d, views, anchor, _ptr(t), t_min, _ptr(pair_coef), _ptr(xc), _ptr(xa),
                                               _ptr(pres), _ptr(ws), ws_bytes, _ptr(up), _DTYPES[torch.bfloat16], _ptr(dx), _ptr(dx_all),
                                               _ptr(d_t), _stream()), "aecf_nce_multi_pp_grads")
        g_t = d_t.reshape(t_shape) if d_t is not None else None
        return dx, dx_all, None, None, None, g_t, None, None, None, None


def _pair_order(views: int, anchor: Optional[int]) -> str:
    pairs = multiview_pairs(views, anchor)
    return f"P = {len(pairs)} entries in the order of multiview_pairs({views}, {anchor}): {pairs}"


def _pair_temperatures(temperature, x: torch.Tensor, views: int, anchor: Optional[int]):
    """``temperature`` of ``multiview_info_nce`` by its FORM: a number or a one-element tensor -> ``(False, that)`` (one
    temperature: ``_temperature_scalar`` serves it); a sequence of P numbers or a float32 tensor of P elements on x's device ->
    ``(True, [P] float32 device tensor)``, the tensor itself so that its gradient reaches it."""
    pairs = len(multiview_pairs(views, anchor))
    if isinstance(temperature, torch.Tensor):
        if temperature.numel() == 1:
            return False, temperature
        if temperature.numel() != pairs:
            raise ValueError(f"multiview_info_nce: a tensor temperature holds 1 element or one per pair, got shape "
                             f"{tuple(temperature.shape)}; {_pair_order(views, anchor)}")
        if temperature.dtype != torch.float32:
            raise TypeError(f"aecf_amd: a tensor temperature must be float32, got {temperature.dtype}")
        if temperature.device != x.device:
            raise ValueError(f"aecf_amd: the temperature lives on {temperature.device}, the embeddings on {x.device}")
        return True, temperature.reshape(pairs)
    if isinstance(temperature, (list, tuple)):
        if len(temperature) != pairs:
            raise ValueError(f"multiview_info_nce: a sequence of temperatures holds one per pair, got {len(temperature)}; "
                             f"{_pair_order(views, anchor)}")
        return True, torch.tensor([float(v) for v in temperature], dtype=torch.float32, device=x.device)
    return False, temperature


def _pair_weights(pair_weights, x: torch.Tensor, views: int, anchor: Optional[int]) -> Optional[torch.Tensor]:
    """``pair_weights`` of ``multiview_info_nce`` as the kernels read them: None, or [P] float32 on x's device.  Host weights are
    checked here (non-negative, finite); a device tensor is not read on the host -- it is normalised by the pair-coefficient
    launch."""
    if pair_weights is None:
        return None
    pairs = len(multiview_pairs(views, anchor))
    if isinstance(pair_weights, torch.Tensor):
        if pair_weights.numel() != pairs:
            raise ValueError(f"multiview_info_nce: pair_weights holds one weight per pair, got shape {tuple(pair_weights.shape)}; "
                             f"{_pair_order(views, anchor)}")
        if pair_weights.dtype != torch.float32:
            raise TypeError(f"multiview_info_nce: a tensor of pair_weights must be float32, got {pair_weights.dtype}")
        if pair_weights.device != x.device:
            raise ValueError(f"multiview_info_nce: the pair_weights live on {pair_weights.device}, the embeddings on {x.device}")
        if pair_weights.requires_grad:
            raise ValueError("multiview_info_nce: pair_weights are not differentiable; pass a tensor that does not require grad")
        return pair_weights.reshape(pairs).contiguous()
    if not isinstance(pair_weights, (list, tuple)) or len(pair_weights) != pairs:
        raise ValueError(f"multiview_info_nce: pair_weights holds one weight per pair, got {pair_weights!r}; {_pair_order(views, anchor)}")
    host = [float(v) for v in pair_weights]
    if any(not (v >= 0.0) or v == float("inf") for v in host):
        raise ValueError(f"multiview_info_nce: pair_weights must be non-negative and finite, got {host}")
    return torch.tensor(host, dtype=torch.float32, device=x.device)


def _multiview_refusal(x: torch.Tensor, cols: int, min_temperature: float, anchor: int, per_pair: bool = False) -> Optional[str]:
    """None where multi-view InfoNCE runs; else the limit that stands against it.  The memory test (P blocks of b_local x b_all
    bfloat16 and the float32 slabs within 0.6 of the free device memory) is skipped while a graph is being captured."""
    rows, views, d = x.shape
    if x.dtype != torch.bfloat16:
        return f"bfloat16 rows (got {x.dtype})"
    if d % 64 != 0 or not 64 <= d <= 4096:
        return f"d % 64 == 0 with 64 <= d <= 4096 (got d = {d})"
    if not float(min_temperature) >= MIN_TEMPERATURE:
        return f"min_temperature >= {MIN_TEMPERATURE} (got {min_temperature}): 1 / T is the constant shift of every exponential"
    lib = _lib.load()
    need = (lib.aecf_nce_multi_pp_workspace_bytes if per_pair else lib.aecf_nce_multi_workspace_bytes)(rows, cols, d, views, anchor)
    if need == 0:
        return f"fewer than 2^31 gathered rows (got {cols})"
    if not _capturing() and need > 0.6 * torch.cuda.mem_get_info(x.device)[0]:
        return f"a workspace (one b_local x b_all bfloat16 block per pair, {need} bytes here) within 0.6 of the free device memory"
    return None


def multiview_info_nce(x, temperature: Union[float, torch.Tensor] = 0.07, group=None, min_temperature: float = MIN_TEMPERATURE,
                       anchor: Optional[int] = None, pair_weights=None, key_padding_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Symmetric InfoNCE over the pairs of M views, negatives from every rank of ``group``:

        L = (1 / P) * sum over the pairs (m, n) of info_nce(x[:, m], x[:, n], temperature, group, min_temperature)

    ``x``: [b_local, M, d] bfloat16 on a ROCm device, 2 <= M <= 8 -- the layout the fusion pool takes; the views are read where
    they lie.  A sequence of M [b_local, d] tensors is accepted too: it is stacked once, which costs a copy of every view.
    ``anchor=None``: every pair m < n, P = M (M - 1) / 2.  ``anchor=k``: the pairs that hold view k (the ImageBind arrangement),
    P = M - 1.  In pair (m, n), m < n, view m supplies this rank's rows and view n the gathered keys.

    One normalisation launch over all b_local M rows, one all-gather of the normalised block, ONE logits launch for all P pair
    blocks, one all-reduce of [P, b_all] column sums; in the backward one gradient product per role whose K loop runs through
    every partner block of a view, so a gradient element is one float32 sum over all its partners, rounded once (a loop of
    ``info_nce`` rounds every pair's gradient to bfloat16 and adds them afterwards).  ``temperature`` as in ``info_nce``: a
    float (placed in a device scalar) or a learnable one-element float32 device tensor, read as ``max(T, min_temperature)``
    with no host read, its gradient formed by the kernels.  The return and gradient conventions under data parallel are
    ``info_nce``'s.  The backward runs once per forward.

    A temperature and a weight PER PAIR.  ``temperature`` may also be a sequence of P floats or a float32 device tensor of P
    elements, and ``pair_weights`` a sequence of P non-negative floats or a float32 [P] device tensor that does not require grad
    (None: uniform); P and the order of the entries are those of ``multiview_pairs(M, anchor)``.  Pair p runs at
    ``T_p = max(temperature[p], min_temperature)``, read on the device (no host read, capturable), and

        L = sum_p w_p info_nce_p / sum_p w_p

    A [P] temperature that requires grad receives a [P] gradient: the logits launch then also sums E (s - 1) per row and per
    column of every pair from its float32 accumulators, and one small launch forms every dL/dT_p from those sums in a fixed order
    (an entry below ``min_temperature`` gets 0, as the scalar does).  A zero weight gives its pair exact-zero gradients, dT_p
    included; where all weights are zero the loss is 0 with zero gradients.  Device weights are normalised on the device.  The
    form of the arguments selects the path, never their values: a number or a one-element tensor with ``pair_weights=None`` is the
    code path, the launches and the bits described above; with ``pair_weights`` given it is spread over the pairs.  A tensor with
    another element count, or negative or non-finite host weights, raise ValueError.

    Needs bfloat16, d % 64 == 0 (64 to 4096), ``min_temperature >= 0.025`` and a workspace (P blocks of b_local x b_all
    bfloat16 plus float32 slabs) within 0.6 of the free device memory (not tested while capturing); otherwise raises
    NotImplementedError naming the limit -- a loop of ``info_nce`` over the pairs serves such inputs.  No fallback.

    ``key_padding_mask`` (None: every row holds every view -- the code path, launches and bits above): [b_local, M], bool or uint8,
    on x's device, True / non-zero where view m of row i is ABSENT -- the fusion pool's convention, so one tensor serves both
    calls.  A row may keep all views, some, one or none.  Pair (m, n) then runs over V = the rows, of every rank, that hold both
    views: only they are anchors, only they are keys, in both directions,

        L = (1 / P') * sum over the pairs with a row of info_nce(x[V, m], x[V, n], ...),   P' = the number of such pairs

    (with ``pair_weights``: sum over those pairs of w_p info_nce_p / the sum of their w_p -- a pair without a row drops out of the
    normalisation, its dT_p is 0)

    (0 with zero gradients where no pair has a row; a pair with one row adds 0).  What an absent slot holds -- zeros, stale data,
    inf, NaN -- does not matter: it is excluded by the mask and by index, never by value; its gradient is an exact zero.  The
    mask is read on the device (no host read; a captured step replays the mask's current contents); the row counts of the
    pairs and their weights 0.5 / n / P' are formed there.  Data parallel adds one all-gather of b_local presence bytes beside
    the all-gather of the rows; every rank derives the counts from the gathered bytes.  A masked pair costs a full pair: absent
    rows are zeroed, not skipped."""
    if isinstance(x, (list, tuple)):
        views = list(x)
        if not all(isinstance(v, torch.Tensor) and v.dim() == 2 for v in views) or any(v.shape != views[0].shape for v in views):
            raise ValueError("multiview_info_nce expects [b, M, d] or a sequence of [b, d] views of equal shape, got "
                             f"{[tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__ for v in views]}")
        if not 2 <= len(views) <= MULTIVIEW_MAX_VIEWS:
            raise ValueError(f"multiview_info_nce serves 2 to {MULTIVIEW_MAX_VIEWS} views, got {len(views)}")
        for k, v in enumerate(views):
            _require_device(v, f"view {k}")
        x = torch.stack(views, dim=1)
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError("multiview_info_nce expects [b, M, d] or a sequence of [b, d] views of equal shape, got "
                         f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    b_local, views, d = x.shape
    if not 2 <= views <= MULTIVIEW_MAX_VIEWS:
        raise ValueError(f"multiview_info_nce serves 2 to {MULTIVIEW_MAX_VIEWS} views, got {views}")
    if anchor is not None and not (isinstance(anchor, int) and not isinstance(anchor, bool) and 0 <= anchor < views):
        raise ValueError(f"multiview_info_nce: anchor must be None or a view index in 0..{views - 1}, got {anchor!r}")
    _check_min_temperature(min_temperature)
    if key_padding_mask is not None:
        if not isinstance(key_padding_mask, torch.Tensor) or key_padding_mask.dim() != 2 or \
                tuple(key_padding_mask.shape) != (b_local, views):
            raise ValueError(f"multiview_info_nce: key_padding_mask must be a [b, M] = [{b_local}, {views}] tensor, got "
                             f"{tuple(key_padding_mask.shape) if isinstance(key_padding_mask, torch.Tensor) else type(key_padding_mask).__name__}")
        if key_padding_mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"multiview_info_nce: key_padding_mask must be bool or uint8, got {key_padding_mask.dtype}")
        if key_padding_mask.device != x.device:
            raise ValueError(f"multiview_info_nce: the key_padding_mask lives on {key_padding_mask.device}, the embeddings on {x.device}")
    per_pair, temperature = _pair_temperatures(temperature, x, views, anchor)
    weights = _pair_weights(pair_weights, x, views, anchor)
    per_pair = per_pair or weights is not None
    _require_device(x, "x")
    k = -1 if anchor is None else int(anchor)
    world = dp.world_info(group)[1]
    sizes, offset, b_all = _row_ranges(b_local, x.device, group)
    # every rank must refuse together (they exchange between the passes)
    refusal = _agreed_refusal(_multiview_refusal(x, b_all, min_temperature, k, per_pair), x.device, group)
    if refusal is not None:
        raise NotImplementedError("aecf_amd: multi-view InfoNCE needs " + refusal + "; a loop of info_nce over the pairs serves "
                                  "such inputs")
    if per_pair:
        if not (isinstance(temperature, torch.Tensor) and temperature.numel() > 1):     # one temperature, spread over the pairs
            temperature = _temperature_scalar(temperature, x, min_temperature).reshape(1).expand(len(multiview_pairs(views, anchor)))
        t = temperature
    else:
        t = _temperature_scalar(temperature, x, min_temperature)
    if key_padding_mask is not None:
        absent = key_padding_mask.detach().contiguous().view(torch.uint8).reshape(b_local * views)      # a view: read at replay
        nx, pres = _L2NormMaskedSlots.apply(x.reshape(b_local * views, d), absent, views, 1e-12)
        nx = nx.reshape(b_local, views, d)
        if world > 1:
            nx_all = dp.all_gather_rows(nx.reshape(b_local, views * d), group, sizes=sizes).reshape(b_all, views, d)
            with torch.no_grad():                   # the one exchange the mask adds: b_local bytes per rank
                pres_all = dp.all_gather_rows(pres.reshape(b_local, 1), group, sizes=sizes).reshape(b_all).contiguous()
        else:
            nx_all, pres_all = nx, pres
        if per_pair:
            share = _NceMultiViewPairwise.apply(nx, nx_all, pres, pres_all, offset, t, weights, group, float(min_temperature), k)
        else:
            share = _NceMultiViewMasked.apply(nx, nx_all, pres, pres_all, offset, t, group, float(min_temperature), k)
    else:
        nx = l2_normalize(x.reshape(b_local * views, d)).reshape(b_local, views, d)
        nx_all = dp.all_gather_rows(nx.reshape(b_local, views * d), group, sizes=sizes).reshape(b_all, views, d) if world > 1 else nx
        if per_pair:
            share = _NceMultiViewPairwise.apply(nx, nx_all, None, None, offset, t, weights, group, float(min_temperature), k)
        else:
            pairs = len(multiview_pairs(views, anchor))
            share = _NceMultiView.apply(nx, nx_all, offset, t, 0.5 / float(b_all) / float(pairs), group, float(min_temperature), k)
    return _dp_value(share, group)


def _sig_scalar_arg(value, z: torch.Tensor, what: str):
    """``temperature`` / ``bias`` of ``sigmoid_contrastive``: a Python number -> float; a tensor -> itself, checked like
    ``_temperature_arg`` (one float32 element on z's device: the kernels read it there)."""
    if not isinstance(value, torch.Tensor):
        return float(value)
    if value.dtype != torch.float32:
        raise TypeError(f"aecf_amd: a tensor {what} must be float32, got {value.dtype}")
    if value.numel() != 1:
        raise ValueError(f"aecf_amd: a tensor {what} must hold one element, got shape {tuple(value.shape)}")
    if value.device != z.device:
        raise ValueError(f"aecf_amd: the {what} lives on {value.device}, the embeddings on {z.device}")
    return value


def _sig_args(temperature, bias, z: torch.Tensor, min_temperature):
    _check_min_temperature(min_temperature)
    return _sig_scalar_arg(temperature, z, "temperature"), _sig_scalar_arg(bias, z, "bias")


class _SigmoidContrastive(torch.autograd.Function):
    """aecf_sig_pass1 / aecf_sig_grads: the pairwise sigmoid loss of local unit-norm rows ``a`` against the gathered rows
    ``b_all`` (positives at ``row_offset + i``), temperature and bias one-element float32 device tensors.  The forward runs the
    logits GEMM, whose epilogue leaves g = sigmoid(l) - [positive] in the workspace together with the loss rows and dbias; the
    backward runs the two gradient products over it, scaled on the device by the gradient that arrives.  Every logit is its own
    term: NO collective runs between the two passes (the only exchanges are the caller's all-gather and its reduce-scatter).
    Returns this rank's rows' share of the loss; gradients: da, this rank's share of db_all, dT, dbias."""

    @staticmethod
    def forward(ctx, a, b_all, temperature, bias, row_offset, coef, min_temperature):
        lib = _lib.load()
        rows, d = a.shape
        cols = b_all.shape[0]
        dev = a.device
        ac, bc = a.detach().to(torch.bfloat16).contiguous(), b_all.detach().to(torch.bfloat16).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        ws_bytes = lib.aecf_sig_workspace_bytes(rows, cols, d)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        loss_rows, d_bias = torch.empty(rows, **f32), torch.empty(1, **f32)
        t = temperature.detach()
        _lib.check(lib.aecf_sig_pass1(rows, cols, row_offset, d, _ptr(t), float(min_temperature), _ptr(bias.detach()), _ptr(ac),
                                      _ptr(bc), _ptr(ws), ws_bytes, _ptr(loss_rows), _ptr(d_bias), _stream()), "aecf_sig_pass1")
        ctx.save_for_backward(ac, bc, ws, t, d_bias)
        ctx.meta = (a.dtype, b_all.dtype, temperature.shape, bias.shape,
                    (rows, cols, int(row_offset), d, float(coef), float(min_temperature), ws_bytes))
        return loss_rows.sum() * coef

    @staticmethod
    def backward(ctx, d_loss):
        lib = _lib.load()
        ac, bc, ws, t, d_bias = ctx.saved_tensors
        ad, bd, t_shape, b_shape, (rows, cols, row_offset, d, coef, t_min, ws_bytes) = ctx.meta
        gdt = torch.bfloat16 if (ad == torch.bfloat16 and bd == torch.bfloat16) else torch.float32
        da = torch.empty(rows, d, dtype=gdt, device=ac.device)
        db = torch.empty(cols, d, dtype=gdt, device=ac.device)
        up = d_loss.detach().to(torch.float32).reshape(1).contiguous()
        d_t = torch.empty(1, dtype=torch.float32, device=ac.device) if ctx.needs_input_grad[2] else None
        _lib.check(lib.aecf_sig_grads(rows, cols, row_offset, d, _ptr(t), t_min, coef, _ptr(ac), _ptr(bc), _ptr(ws), ws_bytes,
                                      _ptr(up), _DTYPES[gdt], _ptr(da), _ptr(db), _ptr(d_t), _stream()), "aecf_sig_grads")
        g_t = d_t.reshape(t_shape) if d_t is not None else None
        g_b = (d_bias * coef * up).reshape(b_shape) if ctx.needs_input_grad[3] else None
        return da.to(ad), db.to(bd), g_t, g_b, None, None, None


SIG_STREAM_WIDTHS = (128, 256, 384, 512, 768, 1024)     # the widths aecf_sig_stream_workspace_bytes answers for


class _SigmoidStream(torch.autograd.Function):
    """aecf_sig_stream_fwd_bwd: the same share of the loss as ``_SigmoidContrastive`` without the b_local x b_all block, modelled
    on ``_NceDirection``: the forward makes the one call with gradients at upstream 1 and saves them (float32), the backward
    multiplies them by the gradient that arrives, on the device.  Where no input requires a gradient or grad mode is off the
    forward takes the call's loss-only mode (``grads`` False, decided by the caller: grad mode is off inside a forward; the same
    loss bits).  No collective anywhere."""

    @staticmethod
    def forward(ctx, a, b_all, temperature, bias, row_offset, coef, min_temperature, grads):
        lib = _lib.load()
        rows, d = a.shape
        cols = b_all.shape[0]
        dev = a.device
        ac, bc = a.detach().to(torch.bfloat16).contiguous(), b_all.detach().to(torch.bfloat16).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        ws_bytes = lib.aecf_sig_stream_workspace_bytes(rows, cols, d)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        loss_rows = torch.empty(rows, **f32)
        da = db = d_bias = d_t = None
        if grads:
            da, db = torch.empty(rows, d, **f32), torch.empty(cols, d, **f32)
            d_bias = torch.empty(1, **f32) if ctx.needs_input_grad[3] else None
            d_t = torch.empty(1, **f32) if ctx.needs_input_grad[2] else None
        _lib.check(lib.aecf_sig_stream_fwd_bwd(rows, cols, row_offset, d, _ptr(temperature.detach()), float(min_temperature),
                                               _ptr(bias.detach()), float(coef), _ptr(ac), _ptr(bc), _ptr(loss_rows), _ptr(d_bias),
                                               _ptr(d_t), _ptr(da), _ptr(db), _ptr(ws), ws_bytes, _stream()),
                   "aecf_sig_stream_fwd_bwd")
        ctx.save_for_backward(da, db, d_t, d_bias)
        ctx.meta = (a.dtype, b_all.dtype, temperature.shape, bias.shape, float(coef))
        return loss_rows.sum() * coef

    @staticmethod
    def backward(ctx, d_loss):
        da, db, d_t, d_bias = ctx.saved_tensors
        ad, bd, t_shape, b_shape, coef = ctx.meta
        g = d_loss.detach().to(torch.float32)
        g_t = (d_t * g).reshape(t_shape) if d_t is not None else None
        g_b = (d_bias * coef * g).reshape(b_shape) if d_bias is not None else None
        return (da * g).to(ad), (db * g).to(bd), g_t, g_b, None, None, None, None


def sigmoid_contrastive(za: torch.Tensor, zb: torch.Tensor, temperature: Union[float, torch.Tensor] = 0.1,
                        bias: Union[float, torch.Tensor] = -10.0, group=None, min_temperature: float = 1e-3,
                        low_memory: Optional[bool] = None) -> torch.Tensor:
    """Pairwise sigmoid (SigLIP) loss between the local rows of two views, negatives from every rank of ``group``:

        L = 1 / B_all * sum_ij softplus(-y_ij (na_i . nb_j / max(T, min_temperature) + bias)),  y_ij = +1 on the positives, else -1

    ``za``, ``zb``: [b_local, d] bfloat16 on a ROCm device, d % 64 == 0, any row count (the same on every rank).  Every logit is
    its own binary term, so nothing is normalised over rows, columns or ranks: the forward issues ONE all-gather (the rows of
    view b) and one scalar all-reduce (the returned value), and no collective runs between the logits pass and the gradient
    products.  ``temperature`` and ``bias``: a Python float, or a learnable one -- a one-element float32 tensor on za's device
    (e.g. ``1 / logit_scale.exp()``).  Both are read by the kernels on the device (a float is filled into a one-element tensor;
    no host read anywhere, so a captured step replays the values the tensors hold then) and both get their gradient from the
    same kernels (dT is zero where ``T < min_temperature``; any positive ``min_temperature`` is legal).

    ``low_memory``: which of the two implementations runs.  ``False``: the tile-GEMM form, which keeps g = sigmoid(l) -
    [positive] as a b_local x b_all bfloat16 block between forward and backward (d % 64 == 0, and the block within 0.6 of the
    free device memory).  ``True``: the streaming form (d in 128, 256, 384, 512, 768, 1024), which never holds that block -- its
    workspace is O(b_local d) -- at 8/6 or more of the matrix work.  ``None`` (the default): the tile form wherever it runs, else
    the streaming form.  Ranks may take different forms: nothing is exchanged between the passes of either.

    Data-parallel convention: ``info_nce``'s -- the returned value is the global loss on every rank, the local term carries
    ``world`` so that an averaging gradient reduce leaves the one-rank gradient on the replicated parameters, T and bias
    included."""
    _require_device(za, "za")
    _require_device(zb, "zb")
    _check_two_views("sigmoid_contrastive", za, zb)
    t, b = _sig_args(temperature, bias, za, min_temperature)
    rank, world = dp.world_info(group)
    rows, d = za.shape
    cols = rows * world
    bf16 = za.dtype == torch.bfloat16 and zb.dtype == torch.bfloat16
    stream_need = _lib.load().aecf_sig_stream_workspace_bytes(rows, cols, d) if bf16 and low_memory is not False else 0
    if low_memory:
        if stream_need == 0:
            raise NotImplementedError("aecf_amd: the streaming sigmoid contrastive loss needs bfloat16 rows with d in "
                                      f"{SIG_STREAM_WIDTHS}; got {za.dtype}, d = {d}")
        form = _SigmoidStream
    else:
        need = _lib.load().aecf_sig_workspace_bytes(rows, cols, d) if bf16 else 0
        form = _SigmoidContrastive
        if need == 0 or (not _capturing() and need > 0.6 * torch.cuda.mem_get_info(za.device)[0]):
            if low_memory is False:
                raise NotImplementedError("aecf_amd: the sigmoid contrastive loss needs bfloat16 rows with d % 64 == 0 and a "
                                          f"workspace (b_local x b_all bfloat16, {need} bytes here) within 0.6 of the free device "
                                          f"memory; got {za.dtype}, d = {d}")
            if stream_need == 0:
                raise NotImplementedError("aecf_amd: the sigmoid contrastive loss needs bfloat16 rows and either d % 64 == 0 with a "
                                          f"workspace (b_local x b_all bfloat16, {need} bytes here) within 0.6 of the free device "
                                          f"memory (the tile form) or d in {SIG_STREAM_WIDTHS} (the streaming form); got "
                                          f"{za.dtype}, d = {d}")
            form = _SigmoidStream
    t, b = _device_scalar(t, za), _device_scalar(b, za)
    na, nb = l2_normalize(za), l2_normalize(zb)
    nb_all = dp.all_gather_rows(nb, group, sizes=[rows] * world) if world > 1 else nb
    if form is _SigmoidStream:
        grads = torch.is_grad_enabled() and any(x.requires_grad for x in (na, nb_all, t, b))
        share = form.apply(na, nb_all, t, b, rank * rows, 1.0 / float(cols), float(min_temperature), grads)
    else:
        share = form.apply(na, nb_all, t, b, rank * rows, 1.0 / float(cols), float(min_temperature))
    return _dp_value(share, group)


SUPCON_WIDTHS = (128, 256, 384, 512, 768, 1024)         # the widths aecf_supcon_workspace_bytes answers for


def _labels_arg(labels, z: torch.Tensor) -> torch.Tensor:
    """``labels`` of ``supervised_contrastive``, checked against the embeddings ``z`` [b_local, d]: one int64 or int32 class per
    local row, on z's device (a negative class = unlabeled).  Returns them as they are: the caller widens int32 on the device."""
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"aecf_amd: labels must be a tensor of int64 or int32 classes, got {type(labels).__name__}")
    if labels.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"aecf_amd: labels must be int64 or int32, got {labels.dtype}")
    if labels.dim() != 1 or labels.shape[0] != z.shape[0]:
        raise ValueError(f"aecf_amd: labels must hold one class per local row, shape ({z.shape[0]},); got {tuple(labels.shape)}")
    if labels.device != z.device:
        raise ValueError(f"aecf_amd: the labels live on {labels.device}, the embeddings on {z.device}")
    return labels


class _StreamForm(NamedTuple):
    """One streaming direction as data.  The operator takes ``apply(q, k_all, *riders, *options, *offsets, temperature, coef,
    min_temperature, grads)`` and the library's call ``(rows, cols, *offsets, d, T, min T, coef, q, k_all, *riders, *options,
    loss rows, dq, dk, dT, workspace, its bytes, stream)``."""
    call: str                   # the entry point that forms the loss and both gradients
    workspace_bytes: str        # its workspace query: 0 where the width is not served
    riders: tuple               # the int64 tensors beside q and k_all
    options: tuple              # the integers handed on after them
    offsets: tuple              # where local row i finds its partner (and itself) among the keys
    needs: str                  # "<the loss> needs", as the refusal opens


class _StreamDirection(torch.autograd.Function):
    """One direction of a label-aware contrastive loss on the streaming kernels, the call named by ``form`` (a subclass sets
    it).  Modelled on ``_NceDirection``: the forward makes the one call with the gradients at upstream 1 and saves them
    (float32), the backward multiplies them by the gradient that arrives, on the device.  ``grads`` False (decided by the caller:
    grad mode is off inside a forward) takes the call's loss-only mode: the same loss bits, no gradient buffers.  The temperature
    is a one-element float32 device tensor."""
    form: _StreamForm

    @classmethod                # (not torch's usual staticmethod: the class ``apply`` was called on carries the form)
    def forward(cls, ctx, q, k_all, *args):
        form = cls.form
        n_riders = len(form.riders)
        n_options = n_riders + len(form.options)
        n_plain = n_options + len(form.offsets)             # (the temperature follows q, k_all and these)
        riders, options, offsets = args[:n_riders], args[n_riders:n_options], args[n_options:n_plain]
        temperature, coef, min_temperature, grads = args[n_plain:]
        lib = _lib.load()
        rows, d = q.shape
        cols = k_all.shape[0]
        dev = q.device
        bf16 = q.dtype == torch.bfloat16 and k_all.dtype == torch.bfloat16
        ws_bytes = getattr(lib, form.workspace_bytes)(rows, cols, d) if bf16 else 0
        if ws_bytes == 0:
            raise NotImplementedError(f"aecf_amd: {form.needs} bfloat16 rows with d in {SUPCON_WIDTHS}; got {q.dtype}, d = {d}")
        qc, kc = q.detach().contiguous(), k_all.detach().contiguous()
        riders = [r.contiguous() for r in riders]
        f32 = dict(dtype=torch.float32, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        loss_rows = torch.empty(rows, **f32)
        dq = dk = d_t = None
        if grads:
            dq, dk = torch.empty(rows, d, **f32), torch.empty(cols, d, **f32)
            d_t = torch.empty(1, **f32) if ctx.needs_input_grad[2 + n_plain] else None
        _lib.check(getattr(lib, form.call)(rows, cols, *map(int, offsets), d, _ptr(temperature.detach()), float(min_temperature),
                                           float(coef), _ptr(qc), _ptr(kc), *map(_ptr, riders), *map(int, options), _ptr(loss_rows),
                                           _ptr(dq), _ptr(dk), _ptr(d_t), _ptr(ws), ws_bytes, _stream()), form.call)
        ctx.save_for_backward(dq, dk, d_t)
        ctx.meta = (q.dtype, k_all.dtype, temperature.shape, n_plain)
        return loss_rows.sum() * coef

    @staticmethod
    def backward(ctx, d_loss):
        dq, dk, d_t = ctx.saved_tensors
        qd, kd, t_shape, n_plain = ctx.meta
        g = d_loss.detach().to(torch.float32)
        g_t = (d_t * g).reshape(t_shape) if d_t is not None else None
        return ((dq * g).to(qd), (dk * g).to(kd), *[None] * n_plain, g_t, None, None, None)


class _SupConDirection(_StreamDirection):
    """aecf_supcon_fwd_bwd: sum_i [logsumexp_j(q_i.k_j/T) - mean over the positives of q_i.k_j/T] * coef for local unit-norm q
    against all k, the positives of row i being its partner ``row_offset + i`` and every key that carries its (non-negative)
    label.  Forward, backward, ``grads`` and the temperature: ``_StreamDirection``'s."""
    form = _StreamForm("aecf_supcon_fwd_bwd", "aecf_supcon_workspace_bytes", riders=("q_labels", "k_labels"), options=(),
                       offsets=("row_offset",), needs="the supervised contrastive loss needs")


class _SupConPoolDirection(_StreamDirection):
    """aecf_supcon_pool_fwd_bwd: ``_SupConDirection`` over a pool of keys that holds the anchors themselves.  ``k_all`` is the one
    key buffer of both views; local row i has its partner at ``row_offset + i`` and itself at ``self_offset + i``, and that key is
    left out of the log-sum-exp, of the positives and of both gradients.  The gradient on ``k_all`` is the whole pool's, so
    autograd splits it over the two views."""
    form = _StreamForm("aecf_supcon_pool_fwd_bwd", "aecf_supcon_workspace_bytes", riders=("q_labels", "k_labels"), options=(),
                       offsets=("row_offset", "self_offset"), needs="the pooled contrastive losses need")


class _TileForm(NamedTuple):
    """One two-view tile form as data.  The operator takes ``apply(*operands, *riders, *options, row_offset, temperature, coef,
    group, min_temperature)``; the library's three calls take the operands, riders and options in that order:
    ``<prefix>_pass1(rows, cols, offset, d, T, min T, *operands, *riders, *options, workspace, its bytes, column statistics, stream)``,
    ``<prefix>_loss(rows, cols, offset, d, T, min T, first operand, last operand, column statistics, workspace, its bytes, loss
    rows, stream)`` and ``<prefix>_grads(rows, cols, offset, d, T, min T, coef, *operands, *riders, *options, workspace, its bytes,
    upstream, gradient dtype, one gradient per operand, dT, stream)``."""
    prefix: str                 # the symbols are <prefix>_workspace_bytes / _pass1 / _loss / _grads
    operands: tuple             # unit-norm rows: (a, b_all) -- one block of logits -- or (a, b, a_all, b_all) -- three
    riders: tuple               # the int64 tensors that say which keys are positives
    options: tuple              # the integers handed on after them
    stats: tuple                # the column statistics ranks all-reduce are [*stats, cols] float32
    needs: str                  # "<the loss> needs <its limits>", as the forward refuses a shape the library does not serve
    backward: str               # the backward, as the refusal of its second run names it


class _TileSymmetric(torch.autograd.Function):
    """Every anchor of this rank's two-view contrastive loss from the block (or blocks) of logits this rank owns, the calls
    named by ``form`` (a subclass sets it).  Modelled on ``_NceSymmetric`` without the entropy rider: the column statistics are
    the one thing ranks exchange, one all-reduce between pass 1 and the loss; the gradients on gathered rows are this rank's
    shares.  The forward runs the logits pass and the loss; the backward runs the weights passes and the gradient products once,
    scaled on the device by the gradient that arrives and written in the inputs' dtype (bfloat16 where every operand was, else
    float32).  The temperature is a one-element float32 device tensor; the backward returns this rank's share of dL/dT."""
    form: _TileForm

    @classmethod                # (not torch's usual staticmethod: the class ``apply`` was called on carries the form)
    def forward(cls, ctx, *args):
        form = cls.form
        n_operands = len(form.operands)
        n_riders = n_operands + len(form.riders)
        n_options = n_riders + len(form.options)
        operands, riders, options = args[:n_operands], args[n_operands:n_riders], args[n_riders:n_options]
        row_offset, temperature, coef, group, min_temperature = args[n_options:]
        lib = _lib.load()
        rows, d = operands[0].shape
        cols = operands[-1].shape[0]
        dev = operands[0].device
        dtypes = [x.dtype for x in operands]
        operands = [x.detach().to(torch.bfloat16).contiguous() for x in operands]
        riders = [r.contiguous() for r in riders]
        f32 = dict(dtype=torch.float32, device=dev)
        ws_bytes = getattr(lib, form.prefix + "_workspace_bytes")(rows, cols, d)
        if ws_bytes == 0:
            raise NotImplementedError(f"aecf_amd: {form.needs}; got d = {d}, {cols} rows")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        col_stats = torch.empty(*form.stats, cols, **f32)
        t = temperature.detach()
        dims, t_min, options = (rows, cols, int(row_offset), d), float(min_temperature), tuple(map(int, options))
        _lib.check(getattr(lib, form.prefix + "_pass1")(*dims, _ptr(t), t_min, *map(_ptr, operands), *map(_ptr, riders), *options,
                                                        _ptr(ws), ws_bytes, _ptr(col_stats), _stream()), form.prefix + "_pass1")
        if dp.world_info(group)[1] > 1:
            torch.distributed.all_reduce(col_stats, group=group)
        loss_rows = torch.empty(rows, **f32)
        _lib.check(getattr(lib, form.prefix + "_loss")(*dims, _ptr(t), t_min, _ptr(operands[0]), _ptr(operands[-1]), _ptr(col_stats),
                                                       _ptr(ws), ws_bytes, _ptr(loss_rows), _stream()), form.prefix + "_loss")
        ctx.save_for_backward(t, ws, *operands, *riders)
        ctx.meta = (dtypes, temperature.shape, dims, t_min, float(coef), options, ws_bytes)
        return loss_rows.sum() * coef

    @classmethod
    def backward(cls, ctx, d_loss):
        form = cls.form
        lib = _lib.load()
        t, ws, *rows_and_riders = ctx.saved_tensors
        n_operands = len(form.operands)
        t_index = n_operands + len(form.riders) + len(form.options) + 1     # (row_offset stands between them and the temperature)
        dtypes, t_shape, dims, t_min, coef, options, ws_bytes = ctx.meta
        _spend(ctx, form.backward)
        gdt = torch.bfloat16 if dtypes.count(torch.bfloat16) == n_operands else torch.float32
        grads = [torch.empty_like(x, dtype=gdt) for x in rows_and_riders[:n_operands]]
        up = d_loss.detach().to(torch.float32).reshape(1).contiguous()
        d_t = torch.empty(1, dtype=torch.float32, device=ws.device) if ctx.needs_input_grad[t_index] else None
        _lib.check(getattr(lib, form.prefix + "_grads")(*dims, _ptr(t), t_min, coef, *map(_ptr, rows_and_riders), *options, _ptr(ws),
                                                        ws_bytes, _ptr(up), _DTYPES[gdt], *map(_ptr, grads), _ptr(d_t), _stream()),
                   form.prefix + "_grads")
        g_t = d_t.reshape(t_shape) if d_t is not None else None
        return (*[g.to(x) for g, x in zip(grads, dtypes)], *[None] * (t_index - n_operands), g_t, None, None, None)


class _SupConSymmetric(_TileSymmetric):
    """aecf_supcon_sym_pass1 / _loss / _grads: BOTH directions of the symmetric supervised contrastive loss from one block of
    logits (local rows of view a against the gathered rows of view b), the labels shared by the two views.  The column statistics
    [3, cols] are the sums of the exponentials and the counts and raw-score sums of the label matches."""
    form = _TileForm("aecf_supcon_sym", operands=("a", "b_all"), riders=("row_labels", "col_labels"), options=(), stats=(3,),
                     needs="the tile form of the supervised contrastive loss needs d % 64 == 0, 64 <= d <= 4096 and at most "
                           "2^24 gathered rows",
                     backward="symmetric supervised contrastive")


class _TileLimits(NamedTuple):
    """What differs between the tile forms' refusals: ``_tile_refusal``."""
    workspace_bytes: str        # the library's workspace query: 0 for more gathered rows than the form serves
    row_limit: str              # ... which is then said with this, {cols} filled in
    workspace: str              # what the workspace holds


_SUPCON_LIMITS = _TileLimits("aecf_supcon_sym_workspace_bytes", "at most 2^24 gathered rows (got {cols})",
                             "b_local x b_all bfloat16")
_NTXENT_LIMITS = _TileLimits("aecf_ntxent_sym_workspace_bytes", "fewer than 2^31 gathered rows (got {cols})",
                             "three b_local x b_all bfloat16 blocks")
_POOL_LIMITS = _TileLimits("aecf_supcon_pool_sym_workspace_bytes",
                           "at most 2^23 gathered rows (got {cols}): the counts of two blocks add in float32",
                           "three b_local x b_all bfloat16 blocks")


def _tile_refusal(limits: _TileLimits, z: torch.Tensor, zb: torch.Tensor, cols: int, min_temperature: float) -> Optional[str]:
    """None where a two-view tile form runs; else what stands against it.  The memory test (the workspace -- the block or blocks
    of b_local x b_all bfloat16 exponentials and their float32 staging -- within 0.6 of the free device memory) is skipped while
    a graph is being captured."""
    rows, d = z.shape
    if z.dtype != torch.bfloat16 or zb.dtype != torch.bfloat16:
        return f"bfloat16 rows (got {z.dtype} and {zb.dtype})"
    if d % 64 != 0 or not 64 <= d <= 4096:
        return f"d % 64 == 0 with 64 <= d <= 4096 (got d = {d})"
    if not float(min_temperature) >= MIN_TEMPERATURE:
        return f"min_temperature >= {MIN_TEMPERATURE} (got {min_temperature}): 1 / T is the constant shift of every exponential"
    need = getattr(_lib.load(), limits.workspace_bytes)(rows, cols, d)
    if need == 0:
        return limits.row_limit.format(cols=cols)
    if not _capturing() and need > 0.6 * torch.cuda.mem_get_info(z.device)[0]:
        return f"a workspace ({limits.workspace}, {need} bytes here) within 0.6 of the free device memory"
    return None


def supervised_contrastive(za: torch.Tensor, zb: torch.Tensor, labels: torch.Tensor, temperature: Union[float, torch.Tensor] = 0.07,
                           group=None, min_temperature: float = MIN_TEMPERATURE, low_memory: Optional[bool] = True,
                           intra_view: bool = False) -> torch.Tensor:
    """Symmetric supervised contrastive loss (Khosla et al. 2020, "L_out") between the local rows of two views, keys from every
    rank of ``group``: the positives of row i of one view are row i of the other view and every row of the other view that
    carries the same label,

        L = 0.5 / B_all * sum over both directions and rows i of [ logsumexp_j x_ij - mean_{j in positives(i)} x_ij ],
        x_ij = na_i . nb_j / max(T, min_temperature)

    ``za``, ``zb``: [b_local, d] bfloat16 on a ROCm device, d in 128, 256, 384, 512, 768, 1024 (anything else is refused: there is
    no torch fallback).  ``labels``: [b_local] int64 or int32 (widened on the device) on the same device, one class per local
    row, shared by both views; a negative class marks an unlabeled row, whose only positive is its partner (two unlabeled rows
    never match).  With all labels negative or all distinct this is ``info_nce``.  Labels carry no gradient.

    ``low_memory``: which of the two implementations runs.  ``True`` (the default): both directions run the streaming kernels
    (aecf_supcon_fwd_bwd): neither the b_local x b_all logits nor a match mask ever exists; the workspace is O(b_local d).
    ``False``: the tile-GEMM form (aecf_supcon_sym_pass1 / _loss / _grads), both directions from ONE block of logits kept as
    b_local x b_all bfloat16 exponentials between forward and backward -- 6 rows cols d matrix flops against the streaming
    form's 16, the labels a sparse correction to InfoNCE's weights.  It needs bfloat16 rows, d % 64 == 0 (64 to 4096),
    ``min_temperature >= 0.025`` and that block within 0.6 of the free device memory (not tested while capturing), and raises
    NotImplementedError naming the limit otherwise; its backward runs once per forward.  ``None``: the tile form wherever it
    runs, the streaming form otherwise.  Under data parallel the ranks agree on one form (they exchange different things).
    ``temperature``: a Python float (filled into a one-element device tensor) or a
    learnable one-element float32 tensor on za's device, read by the kernels as ``max(T, min_temperature)`` with no host read --
    on one rank the call captures into a graph and replays the current temperature and labels -- and given its gradient by the
    same kernels (zero where ``T < min_temperature``; any positive ``min_temperature`` is legal).  Under ``torch.no_grad()``, or
    when no input requires a gradient, only the loss passes run and no gradient buffer is allocated.

    Data parallel: the streaming form all-gathers both views, the labels and the row counts; the tile form gathers view b, the
    labels and the row counts only and all-reduces the [3, b_all] column statistics between its passes.  The convention is
    ``info_nce``'s -- the returned value is the global loss on every rank and the local term carries ``world`` for an averaging
    gradient reduce.

    ``intra_view``: ``False`` (the default) is the cross-view loss above.  ``True`` is the loss as published, over ONE pool of
    the 2 B_all rows of both views: every row is an anchor against the other 2 B_all - 1 rows, itself left out,

        L = 1 / (2 B_all) * sum over the 2 B_all anchors of [ logsumexp_{k != self} x - mean_{k in positives} x ],

    the positives being the partner and every row of EITHER view with the same non-negative label, the anchor excepted.  It
    differs from the reference code of Khosla et al. (``SupConLoss``) only by that code's ``T / base_T`` factor.  Both
    directions run the streaming kernels (aecf_supcon_pool_fwd_bwd) against one key buffer, the gathered rows of view b then
    those of view a; it needs bfloat16 rows, d in 128 .. 1024 as above and 2 B_all < 2^31; ``low_memory`` True or None take
    it, ``False`` raises NotImplementedError: the tile form of the pooled loss is a function of its own,
    ``pooled_supervised_contrastive(..., low_memory=False)``.  With every label negative it is ``nt_xent``."""
    if intra_view and low_memory is False:
        raise NotImplementedError("aecf_amd: the tile form of the supervised contrastive loss has no intra-view keys (it forms "
                                  "the a x b block only); intra_view=True runs the streaming form, low_memory=True or None")
    _require_device(za, "za")
    _require_device(zb, "zb")
    _check_two_views("supervised_contrastive", za, zb)
    labels = _labels_arg(labels, za)
    if low_memory not in (True, False, None):
        raise ValueError(f"aecf_amd: low_memory must be True, False or None, got {low_memory!r}")
    streams = za.dtype == torch.bfloat16 and zb.dtype == torch.bfloat16 and za.shape[1] in SUPCON_WIDTHS
    if intra_view:
        low_memory = True
    if low_memory is True and not streams:
        raise NotImplementedError(f"aecf_amd: the supervised contrastive loss needs bfloat16 rows with d in {SUPCON_WIDTHS}; got "
                                  f"{za.dtype} and {zb.dtype}, d = {za.shape[1]}")
    _check_min_temperature(min_temperature)
    sizes, offset, b_all = _row_ranges(za.shape[0], za.device, group)
    tile = False
    if low_memory is not True:
        # every rank must take the same form (they exchange different things)
        refusal = _agreed_refusal(_tile_refusal(_SUPCON_LIMITS, za, zb, b_all, min_temperature), za.device, group)
        tile = refusal is None
        if not tile and (low_memory is False or not streams):
            raise NotImplementedError("aecf_amd: the tile form of the supervised contrastive loss needs " + refusal
                                      + ("" if low_memory is False else f"; the streaming form needs bfloat16 rows with d in "
                                         f"{SUPCON_WIDTHS}, got {za.dtype} and {zb.dtype}, d = {za.shape[1]}"))
    t = _temperature_scalar(temperature, za, min_temperature)
    lab = labels.detach().to(torch.int64)
    na, nb = l2_normalize(za), l2_normalize(zb)
    nb_all = _all_rows(nb, group, sizes)
    lab_all = _all_rows(lab, group, sizes)
    coef = 0.5 / float(b_all)
    if intra_view:
        if 2 * b_all >= 2 ** 31:
            raise NotImplementedError(f"aecf_amd: the pooled supervised contrastive loss needs 2 b_all < 2^31 keys, got b_all = {b_all}")
        na_all = _all_rows(na, group, sizes)
        pool, lab_pool = torch.cat([nb_all, na_all]), torch.cat([lab_all, lab_all])
        grads = torch.is_grad_enabled() and any(x.requires_grad for x in (na, nb, t))
        l_a = _SupConPoolDirection.apply(na, pool, lab, lab_pool, offset, b_all + offset, t, coef, float(min_temperature), grads)
        l_b = _SupConPoolDirection.apply(nb, pool, lab, lab_pool, b_all + offset, offset, t, coef, float(min_temperature), grads)
        share = l_a + l_b                # this rank's anchors' share of the global objective
    elif tile:
        # both directions from the one block of logits this rank owns: view a is never gathered
        share = _SupConSymmetric.apply(na, nb_all, lab, lab_all, offset, t, coef, group, float(min_temperature))
    else:
        na_all = _all_rows(na, group, sizes)
        grads = torch.is_grad_enabled() and any(x.requires_grad for x in (na, nb, t))
        l_ab = _SupConDirection.apply(na, nb_all, lab, lab_all, offset, t, coef, float(min_temperature), grads)
        l_ba = _SupConDirection.apply(nb, na_all, lab, lab_all, offset, t, coef, float(min_temperature), grads)
        share = l_ab + l_ba              # this rank's rows' share of the global objective
    return _dp_value(share, group)


class _NtXentSymmetric(_TileSymmetric):
    """aecf_ntxent_sym_pass1 / _loss / _grads: the 2 b_local anchors of this rank's NT-Xent from three blocks of logits (a_loc x
    b_all, a_loc x a_all, b_loc x b_all; the anchor itself left out of the last two by index).  The [cols] column sums are those
    of the a x b block plus the b x b row sums on this rank's own range; the backward runs the three weights passes and the six
    gradient products."""
    form = _TileForm("aecf_ntxent_sym", operands=("a", "b", "a_all", "b_all"), riders=(), options=(), stats=(),
                     needs="the tile form of NT-Xent needs d % 64 == 0, 64 <= d <= 4096 and fewer than 2^31 gathered rows",
                     backward="tile-form NT-Xent")


def _ntxent_tile(za: torch.Tensor, zb: torch.Tensor, temperature, group, min_temperature: float, required: bool):
    """The tile form of ``nt_xent``, or None where it does not run and ``required`` is False (the caller then streams)."""
    _check_two_views("nt_xent", za, zb)
    _check_min_temperature(min_temperature)
    sizes, offset, b_all = _row_ranges(za.shape[0], za.device, group)
    # every rank must take the same form (they exchange different things)
    refusal = _agreed_refusal(_tile_refusal(_NTXENT_LIMITS, za, zb, b_all, min_temperature), za.device, group)
    if refusal is not None:
        if required:
            raise NotImplementedError("aecf_amd: the tile form of NT-Xent needs " + refusal)
        return None
    t = _temperature_scalar(temperature, za, min_temperature)
    na, nb = l2_normalize(za), l2_normalize(zb)
    na_all = _all_rows(na, group, sizes)
    nb_all = _all_rows(nb, group, sizes)
    share = _NtXentSymmetric.apply(na, nb, na_all, nb_all, offset, t, 0.5 / float(b_all), group, float(min_temperature))
    return _dp_value(share, group)


def nt_xent(za: torch.Tensor, zb: torch.Tensor, temperature: Union[float, torch.Tensor] = 0.07, group=None,
            min_temperature: float = MIN_TEMPERATURE, low_memory: Optional[bool] = True) -> torch.Tensor:
    """NT-Xent (SimCLR, Chen et al. 2020) between the local rows of two views, keys from every rank of ``group``: the 2 B_all
    rows of both views are one pool, and every row is an anchor whose positive is its partner and whose negatives are the other
    2 B_all - 2 rows of BOTH views,

        L = 1 / (2 B_all) * sum over the 2 B_all anchors of [ logsumexp_{k != self} x_k - x_partner ],   x = n . n_k / max(T, min_temperature)

    ``low_memory``: which of the two implementations runs.  ``True`` (the default) is
    ``supervised_contrastive(za, zb, labels = all -1, ..., intra_view=True)``: the same streaming kernels
    (aecf_supcon_pool_fwd_bwd), the same requirements (bfloat16 on a ROCm device, d in 128, 256, 384, 512, 768, 1024, no torch
    fallback), and the same temperature, ``torch.no_grad()`` and data-parallel behaviour.  ``False``: the tile-GEMM form
    (aecf_ntxent_sym_pass1 / _loss / _grads): three blocks of logits of this rank (a_loc x b_all, a_loc x a_all, b_loc x b_all,
    the anchor itself left out by index) kept as bfloat16 exponentials between forward and backward -- 18 rows cols d matrix
    flops against the streaming form's 64.  It needs bfloat16 rows, d % 64 == 0 (64 to 4096), ``min_temperature >= 0.025`` and
    its workspace (those three blocks plus float32 staging) within 0.6 of the free device memory (not tested while capturing),
    and raises NotImplementedError naming the limit otherwise; its backward runs once per forward.  With one row in all (no
    negative anywhere) the streaming form returns exactly 0, the tile form log(E) + 1/T - s/T, which is 0 only to rounding.
    ``None``: the tile form wherever it runs, the streaming form otherwise (at 8192 x 65536 x 768 the tile form's whole range of
    times lies below the streaming form's, 8.2 ms against 53.7 ms: profiles/ntxent_tile_time.txt).  Under data parallel the tile form gathers both views, the ranks agree on one form (a MIN
    all-reduce, as in ``supervised_contrastive``) and all-reduce the [b_all] column sums between the passes; the returned value
    follows ``info_nce``'s convention."""
    if low_memory not in (True, False, None):
        raise ValueError(f"aecf_amd: low_memory must be True, False or None, got {low_memory!r}")
    _require_device(za, "za")
    if low_memory is not True:
        _require_device(zb, "zb")
        out = _ntxent_tile(za, zb, temperature, group, min_temperature, required=low_memory is False)
        if out is not None:
            return out
    labels = torch.full((za.shape[0],), -1, dtype=torch.int64, device=za.device)
    return supervised_contrastive(za, zb, labels, temperature, group, min_temperature, True, True)


class KeyQueue:
    """Past keys of the two views as further negatives of ``queued_info_nce`` (MoCo's queue, cross-batch memory): two ring
    buffers ``keys_a``, ``keys_b`` [capacity, d] bfloat16 (zeros until written) and ``state``, a device int64 pair (cursor,
    valid).  The state is read and written by kernels alone (aecf_key_queue_push): a push captures into a graph and nothing of it
    is ever read on the host.  ``version`` counts the pushes on the host: the loss's backward reads the buffers again and
    refuses to run across a push.  ``labels=True`` adds ``self.labels``, ONE ring of int64 classes [capacity] beside the two key
    rings (slot s of all three belongs to the same past row; -1 = unlabeled until written), which
    ``queued_supervised_contrastive`` reads: a stored key of the anchor's class is a positive."""

    def __init__(self, capacity: int, d: int, device, labels: bool = False):
        capacity, d = int(capacity), int(d)
        if not 1 <= capacity < 2 ** 31:
            raise ValueError(f"aecf_amd: a key queue holds 1 to 2^31 - 1 rows, got capacity = {capacity}")
        if d <= 0 or d % 8 != 0:
            raise ValueError(f"aecf_amd: a key queue needs d % 8 == 0 (16-byte row copies), got d = {d}")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"aecf_amd: a key queue must be on a ROCm device (got {device}); this package has no CPU path")
        self.capacity, self.d = capacity, d
        self.keys_a = torch.zeros(capacity, d, dtype=torch.bfloat16, device=device)
        self.keys_b = torch.zeros(capacity, d, dtype=torch.bfloat16, device=device)
        self.state = torch.zeros(2, dtype=torch.int64, device=device)
        self.valid = self.state[1:]         # what the loss reads as its count of valid slots
        self.labels = torch.full((capacity,), -1, dtype=torch.int64, device=device) if labels else None
        self.version = 0

    @torch.no_grad()
    def push(self, za: torch.Tensor, zb: torch.Tensor, group=None, normalize: bool = True,
             labels: Optional[torch.Tensor] = None) -> None:
        """Append this step's rows of both views, the oldest slots overwritten first (more rows than the capacity: the last
        ``capacity`` of them stay).  ``za``, ``zb``: [b_local, d] bfloat16 on the queue's device; ``normalize`` runs
        ``l2_normalize`` on them first (pass False for rows that are unit-norm already).  No autograd.  Under data parallel the
        rows of every rank of ``group`` go in, in all-gather order, so that every rank holds the same queue.  ``labels``: on a
        queue made with ``labels=True``, the [b_local] int64 or int32 classes of the rows (gathered with them); None there writes
        -1 into the slots the push fills, so that no label of an overwritten key stays attached to a new one.  A queue made
        without a label ring takes no labels (ValueError)."""
        if labels is not None and self.labels is None:
            raise ValueError("aecf_amd: this key queue has no label ring (KeyQueue(..., labels=True) makes one); push takes no "
                             "labels")
        _require_device(za, "za")
        _require_device(zb, "zb")
        _check_two_views("KeyQueue.push", za, zb)
        if za.dtype != torch.bfloat16 or zb.dtype != torch.bfloat16 or za.shape[1] != self.d or za.device != self.state.device:
            raise ValueError(f"aecf_amd: the key queue holds bfloat16 rows of d = {self.d} on {self.state.device}; got {za.dtype} "
                             f"and {zb.dtype}, d = {za.shape[1]} on {za.device}")
        na, nb = (l2_normalize(za.detach()), l2_normalize(zb.detach())) if normalize else (za.detach(), zb.detach())
        sizes, _, _ = _row_ranges(za.shape[0], za.device, group)
        na, nb = _all_rows(na, group, sizes).contiguous(), _all_rows(nb, group, sizes).contiguous()
        if self.labels is not None:
            lab = None
            if labels is not None:
                lab = _all_rows(_labels_arg(labels, za).detach().to(torch.int64), group, sizes).contiguous()
            _lib.check(_lib.load().aecf_key_queue_push_labeled(self.capacity, self.d, na.shape[0], _ptr(na), _ptr(nb), _ptr(lab),
                                                               _ptr(self.keys_a), _ptr(self.keys_b), _ptr(self.labels),
                                                               _ptr(self.state), _stream()), "aecf_key_queue_push_labeled")
            self.version += 1
            return
        _lib.check(_lib.load().aecf_key_queue_push(self.capacity, self.d, na.shape[0], _ptr(na), _ptr(nb), _ptr(self.keys_a),
                                                   _ptr(self.keys_b), _ptr(self.state), _stream()), "aecf_key_queue_push")
        self.version += 1


class _QueuedNce(torch.autograd.Function):
    """aecf_nce_queue_pass1 / _loss / _grads: both directions of this rank's symmetric InfoNCE from the a_loc x b_all block of
    logits plus two blocks against the stored keys of a ``KeyQueue`` (a_loc x keys_b, b_loc x keys_a; the slots at or above the
    queue's device count left out by index).  Modelled on ``_TileSymmetric``: the [cols] column sums (those of the a x b block plus
    the b x keys_a row sums on this rank's own range) are the one thing ranks exchange; the backward runs the three weights passes
    and the four gradient products once.  The queues take no gradient, but the products read them again: the backward refuses to
    run where the queue was pushed to since the forward."""

    @staticmethod
    def forward(ctx, a, b, b_all, queue, row_offset, temperature, coef, group, min_temperature):
        lib = _lib.load()
        rows, d = a.shape
        cols = b_all.shape[0]
        dev = a.device
        operands = [x.detach().to(torch.bfloat16).contiguous() for x in (a, b, b_all)]
        f32 = dict(dtype=torch.float32, device=dev)
        ws_bytes = lib.aecf_nce_queue_workspace_bytes(rows, cols, queue.capacity, d)
        if ws_bytes == 0:
            raise NotImplementedError("aecf_amd: InfoNCE with a key queue needs d % 64 == 0, 64 <= d <= 4096 and fewer than 2^31 "
                                      f"gathered rows; got d = {d}, {cols} rows")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        col_sums = torch.empty(cols, **f32)
        t = temperature.detach()
        dims, t_min = (rows, cols, int(row_offset), d), float(min_temperature)
        stored = (_ptr(queue.keys_a), _ptr(queue.keys_b), queue.capacity, _ptr(queue.valid))
        _lib.check(lib.aecf_nce_queue_pass1(*dims, _ptr(t), t_min, _ptr(operands[0]), _ptr(operands[1]), *stored, _ptr(operands[2]),
                                            _ptr(ws), ws_bytes, _ptr(col_sums), _stream()), "aecf_nce_queue_pass1")
        if dp.world_info(group)[1] > 1:
            torch.distributed.all_reduce(col_sums, group=group)
        loss_rows = torch.empty(rows, **f32)
        _lib.check(lib.aecf_nce_queue_loss(*dims, _ptr(t), t_min, _ptr(operands[0]), _ptr(operands[2]), queue.capacity,
                                           _ptr(col_sums), _ptr(ws), ws_bytes, _ptr(loss_rows), _stream()), "aecf_nce_queue_loss")
        ctx.save_for_backward(t, ws, *operands)
        ctx.queue, ctx.queue_version = queue, queue.version
        ctx.meta = ([x.dtype for x in (a, b, b_all)], temperature.shape, dims, t_min, float(coef), ws_bytes)
        return loss_rows.sum() * coef

    @staticmethod
    def backward(ctx, d_loss):
        lib = _lib.load()
        t, ws, *operands = ctx.saved_tensors
        dtypes, t_shape, dims, t_min, coef, ws_bytes = ctx.meta
        queue = ctx.queue
        if queue.version != ctx.queue_version:
            raise RuntimeError("aecf_amd: the key queue was pushed to between the forward and the backward of queued_info_nce "
                               "(the gradient products read the stored keys again): the order is loss, backward, push")
        _spend(ctx, "queued InfoNCE")
        gdt = torch.bfloat16 if dtypes.count(torch.bfloat16) == 3 else torch.float32
        grads = [torch.empty_like(x, dtype=gdt) for x in operands]
        up = d_loss.detach().to(torch.float32).reshape(1).contiguous()
        d_t = torch.empty(1, dtype=torch.float32, device=ws.device) if ctx.needs_input_grad[5] else None
        stored = (_ptr(queue.keys_a), _ptr(queue.keys_b), queue.capacity, _ptr(queue.valid))
        _lib.check(lib.aecf_nce_queue_grads(*dims, _ptr(t), t_min, coef, _ptr(operands[0]), _ptr(operands[1]), *stored,
                                            _ptr(operands[2]), _ptr(ws), ws_bytes, _ptr(up), _DTYPES[gdt], *map(_ptr, grads),
                                            _ptr(d_t), _stream()), "aecf_nce_queue_grads")
        g_t = d_t.reshape(t_shape) if d_t is not None else None
        return (*[g.to(x) for g, x in zip(grads, dtypes)], None, None, g_t, None, None, None)


def _queue_refusal(z: torch.Tensor, zb: torch.Tensor, cols: int, queue: KeyQueue, min_temperature: float) -> Optional[str]:
    """``_tile_refusal`` for the queue form: its workspace query takes the queue's capacity, and the queue must fit the rows."""
    rows, d = z.shape
    if z.dtype != torch.bfloat16 or zb.dtype != torch.bfloat16:
        return f"bfloat16 rows (got {z.dtype} and {zb.dtype})"
    if d % 64 != 0 or not 64 <= d <= 4096:
        return f"d % 64 == 0 with 64 <= d <= 4096 (got d = {d})"
    if queue.d != d or queue.state.device != z.device:
        return f"a key queue of the rows' width and device (the queue holds d = {queue.d} on {queue.state.device}, got d = {d} on {z.device})"
    if not float(min_temperature) >= MIN_TEMPERATURE:
        return f"min_temperature >= {MIN_TEMPERATURE} (got {min_temperature}): 1 / T is the constant shift of every exponential"
    need = _lib.load().aecf_nce_queue_workspace_bytes(rows, cols, queue.capacity, d)
    if need == 0:
        return f"fewer than 2^31 gathered rows (got {cols})"
    if not _capturing() and need > 0.6 * torch.cuda.mem_get_info(z.device)[0]:
        return (f"a workspace (b_local x b_all and two b_local x capacity bfloat16 blocks, {need} bytes here) within 0.6 of the "
                "free device memory")
    return None


def queued_info_nce(za: torch.Tensor, zb: torch.Tensor, queue: KeyQueue, temperature: Union[float, torch.Tensor] = 0.07,
                    group=None, min_temperature: float = MIN_TEMPERATURE) -> torch.Tensor:
    """Symmetric InfoNCE between the local rows of two views with the keys of every rank of ``group`` AND the stored keys of
    ``queue`` as negatives: an anchor of view a sees the gathered rows of view b and the valid slots of ``queue.keys_b``, an
    anchor of view b the gathered rows of view a and the valid slots of ``queue.keys_a``,

        L = 0.5 / B_all * sum over both directions and rows i of [ log(sum_batch e^x + sum_queue e^x) - x_ii ],
        x = n . n_k / max(T, min_temperature)

    With an empty queue the three calls give the bits of the symmetric tile form (aecf_nce_sym_*_dt).  ``za``, ``zb``: [b_local, d] bfloat16 on a ROCm device,
    d % 64 == 0 (64 to 4096), ``min_temperature >= 0.025``, and the workspace (the b_local x b_all block and two b_local x capacity
    blocks of bfloat16 exponentials plus float32 staging) within 0.6 of the free device memory (not tested while capturing);
    anything else raises NotImplementedError naming the limit -- there is no streaming form and no torch fallback.
    ``temperature``: a Python float (filled into a one-element device tensor) or a learnable one-element float32 tensor on za's
    device, read by the kernels as ``max(T, min_temperature)`` with no host read and given its gradient by the same kernels;
    there is ONE temperature for batch and queue keys.  The queue's count of valid slots is read on the device too, so a captured
    step replays against whatever the queue holds then.  The stored keys take no gradient.  Under ``torch.no_grad()`` only the
    logits pass and the loss run; the backward runs once per forward.

    The function does NOT push.  Its backward reads the stored keys again, so it raises RuntimeError if ``queue.push`` ran
    between the forward and the backward.  The order of a step is: loss, backward, push --

        loss = queued_info_nce(za, zb, queue, t); loss.backward(); queue.push(za, zb)

    The cost follows the queue's capacity, not its count of valid slots: the logits pass skips the tiles above the count, the
    gradient products run over every slot with an exact-zero weight.  Under data parallel the queue is replicated on every rank
    (``push`` gathers), the ranks agree on a refusal and all-reduce the [b_all] column sums between the passes; the returned
    value follows ``info_nce``'s convention."""
    _require_device(za, "za")
    _require_device(zb, "zb")
    _check_two_views("queued_info_nce", za, zb)
    if not isinstance(queue, KeyQueue):
        raise TypeError(f"aecf_amd: queue must be a KeyQueue, got {type(queue).__name__}")
    _check_min_temperature(min_temperature)
    sizes, offset, b_all = _row_ranges(za.shape[0], za.device, group)
    # every rank must raise or run together (the ranks that run all-reduce between their passes)
    refusal = _agreed_refusal(_queue_refusal(za, zb, b_all, queue, min_temperature), za.device, group)
    if refusal is not None:
        raise NotImplementedError("aecf_amd: InfoNCE with a key queue needs " + refusal)
    t = _temperature_scalar(temperature, za, min_temperature)
    na, nb = l2_normalize(za), l2_normalize(zb)
    nb_all = _all_rows(nb, group, sizes)
    share = _QueuedNce.apply(na, nb, nb_all, queue, offset, t, 0.5 / float(b_all), group, float(min_temperature))
    return _dp_value(share, group)


class _QueuedSupCon(torch.autograd.Function):
    """aecf_supcon_queue_pass1 / _loss / _grads: ``_QueuedNce`` with label positives -- the a_loc x b_all block with the label
    statistics of ``_SupConSymmetric`` and the two blocks against the stored keys searched against the queue's label ring (a
    slot at or above the device count left out by index, of the sums and of the matches).  The [3, cols] column statistics are the
    one thing ranks exchange.  The queue takes no gradient, but the backward reads keys, labels and count again: it refuses to run
    where the queue was pushed to since the forward."""

    @staticmethod
    def forward(ctx, a, b, b_all, lab, lab_all, queue, row_offset, temperature, coef, group, min_temperature):
        lib = _lib.load()
        rows, d = a.shape
        cols = b_all.shape[0]
        dev = a.device
        operands = [x.detach().to(torch.bfloat16).contiguous() for x in (a, b, b_all)]
        labels = [lab.contiguous(), lab_all.contiguous()]
        f32 = dict(dtype=torch.float32, device=dev)
        ws_bytes = lib.aecf_supcon_queue_workspace_bytes(rows, cols, queue.capacity, d)
        if ws_bytes == 0:
            raise NotImplementedError("aecf_amd: the supervised contrastive loss with a key queue needs d % 64 == 0, 64 <= d <= 4096 "
                                      f"and gathered rows + capacity <= 2^24; got d = {d}, {cols} rows, capacity {queue.capacity}")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        col_stats = torch.empty(3, cols, **f32)
        t = temperature.detach()
        dims, t_min = (rows, cols, int(row_offset), d), float(min_temperature)
        stored = (_ptr(queue.keys_a), _ptr(queue.keys_b), queue.capacity, _ptr(queue.valid))
        riders = (_ptr(labels[0]), _ptr(labels[1]), _ptr(queue.labels))
        _lib.check(lib.aecf_supcon_queue_pass1(*dims, _ptr(t), t_min, _ptr(operands[0]), _ptr(operands[1]), *stored, _ptr(operands[2]),
                                               *riders, _ptr(ws), ws_bytes, _ptr(col_stats), _stream()), "aecf_supcon_queue_pass1")
        if dp.world_info(group)[1] > 1:
            torch.distributed.all_reduce(col_stats, group=group)
        loss_rows = torch.empty(rows, **f32)
        _lib.check(lib.aecf_supcon_queue_loss(*dims, _ptr(t), t_min, _ptr(operands[0]), _ptr(operands[2]), queue.capacity,
                                              _ptr(col_stats), _ptr(ws), ws_bytes, _ptr(loss_rows), _stream()),
                   "aecf_supcon_queue_loss")
        ctx.save_for_backward(t, ws, *operands, *labels)
        ctx.queue, ctx.queue_version = queue, queue.version
        ctx.meta = ([x.dtype for x in (a, b, b_all)], temperature.shape, dims, t_min, float(coef), ws_bytes)
        return loss_rows.sum() * coef

    @staticmethod
    def backward(ctx, d_loss):
        lib = _lib.load()
        t, ws, *rest = ctx.saved_tensors
        operands, labels = rest[:3], rest[3:]
        dtypes, t_shape, dims, t_min, coef, ws_bytes = ctx.meta
        queue = ctx.queue
        if queue.version != ctx.queue_version:
            raise RuntimeError("aecf_amd: the key queue was pushed to between the forward and the backward of "
                               "queued_supervised_contrastive (the gradient products read the stored keys and labels again): the "
                               "order is loss, backward, push")
        _spend(ctx, "queued supervised contrastive")
        gdt = torch.bfloat16 if dtypes.count(torch.bfloat16) == 3 else torch.float32
        grads = [torch.empty_like(x, dtype=gdt) for x in operands]
        up = d_loss.detach().to(torch.float32).reshape(1).contiguous()
        d_t = torch.empty(1, dtype=torch.float32, device=ws.device) if ctx.needs_input_grad[7] else None
        stored = (_ptr(queue.keys_a), _ptr(queue.keys_b), queue.capacity, _ptr(queue.valid))
        riders = (_ptr(labels[0]), _ptr(labels[1]), _ptr(queue.labels))
        _lib.check(lib.aecf_supcon_queue_grads(*dims, _ptr(t), t_min, coef, _ptr(operands[0]), _ptr(operands[1]), *stored,
                                               _ptr(operands[2]), *riders, _ptr(ws), ws_bytes, _ptr(up), _DTYPES[gdt],
                                               *map(_ptr, grads), _ptr(d_t), _stream()), "aecf_supcon_queue_grads")
        g_t = d_t.reshape(t_shape) if d_t is not None else None
        return (*[g.to(x) for g, x in zip(grads, dtypes)], None, None, None, None, g_t, None, None, None)


def queued_supervised_contrastive(za: torch.Tensor, zb: torch.Tensor, labels: torch.Tensor, queue: KeyQueue,
                                  temperature: Union[float, torch.Tensor] = 0.07, group=None,
                                  min_temperature: float = MIN_TEMPERATURE) -> torch.Tensor:
    """Symmetric supervised contrastive loss (L_out) between the local rows of two views with the stored keys of ``queue`` as
    further keys AND, where their stored label is the anchor's, further positives (cross-batch memory with labels; MoCo-style
    SupCon).  For an anchor of view a with label y >= 0 the positives are its partner (by index), the gathered rows of view b
    with label y and the valid slots of ``queue.keys_b`` whose entry of ``queue.labels`` is y; an anchor of view b mirrors it on
    view a and ``queue.keys_a``,

        L = 0.5 / B_all * sum over both directions and rows i of [ log(sum_batch e^x + sum_queue e^x) - mean_{p in P(i)} x_ip ],
        x = n . n_k / max(T, min_temperature)

    Same-class keys stay in the denominator.  A negative label is unlabeled: its only positive is the partner, and a stored -1
    matches nothing.  With an empty queue this is ``supervised_contrastive(..., low_memory=False)`` to the bit, with every label
    negative ``queued_info_nce``.  ``queue`` must have been made with ``labels=True`` (ValueError otherwise) and be fed by
    ``queue.push(za, zb, labels=labels)``.  ``labels``: [b_local] int64 or int32 on za's device, shared by the two views.

    Shapes, temperature, ``torch.no_grad()`` and the order of a step (loss, backward, push: the backward reads keys, labels and
    count again and raises RuntimeError across a push; it runs once per forward) are those of ``queued_info_nce``; on top of its
    limits, gathered rows + capacity must not exceed 2^24 (an anchor's count of positives travels as an exact float32 integer).
    Anything else raises NotImplementedError naming the limit.  There is one label per row and one temperature, the cost follows
    the capacity, there is no streaming form, and the queue is replicated on every rank.  Under data parallel the ranks agree on
    a refusal and all-reduce the [3, b_all] column statistics between the passes."""
    _require_device(za, "za")
    _require_device(zb, "zb")
    _check_two_views("queued_supervised_contrastive", za, zb)
    if not isinstance(queue, KeyQueue):
        raise TypeError(f"aecf_amd: queue must be a KeyQueue, got {type(queue).__name__}")
    if queue.labels is None:
        raise ValueError("aecf_amd: queued_supervised_contrastive needs a key queue with a label ring: KeyQueue(..., labels=True)")
    labels = _labels_arg(labels, za)
    _check_min_temperature(min_temperature)
    sizes, offset, b_all = _row_ranges(za.shape[0], za.device, group)
    refusal = None
    if b_all + queue.capacity > 2 ** 24:
        refusal = (f"gathered rows + queue capacity <= 2^24 (got {b_all} + {queue.capacity}): an anchor's count of positives has to "
                   "stay an exact float32 integer")
    refusal = refusal or _queue_refusal(za, zb, b_all, queue, min_temperature)
    # every rank must raise or run together (the ranks that run all-reduce between their passes)
    refusal = _agreed_refusal(refusal, za.device, group)
    if refusal is not None:
        raise NotImplementedError("aecf_amd: the supervised contrastive loss with a key queue needs " + refusal)
    t = _temperature_scalar(temperature, za, min_temperature)
    lab = labels.detach().to(torch.int64)
    na, nb = l2_normalize(za), l2_normalize(zb)
    nb_all = _all_rows(nb, group, sizes)
    lab_all = _all_rows(lab, group, sizes)
    share = _QueuedSupCon.apply(na, nb, nb_all, lab, lab_all, queue, offset, t, 0.5 / float(b_all), group, float(min_temperature))
    return _dp_value(share, group)


class _SupConPoolSymmetric(_TileSymmetric):
    """aecf_supcon_pool_sym_pass1 / _loss / _grads: the 2 b_local anchors of this rank's pooled supervised contrastive loss from
    the three blocks of logits of ``_NtXentSymmetric``, the labels shared by the two views.  The [3, cols] column statistics are
    those of the a x b block plus the b x b row statistics on this rank's own range."""
    form = _TileForm("aecf_supcon_pool_sym", operands=("a", "b", "a_all", "b_all"), riders=("row_labels", "col_labels"), options=(),
                     stats=(3,),
                     needs="the tile form of the pooled supervised contrastive loss needs d % 64 == 0, 64 <= d <= 4096 and at "
                           "most 2^23 gathered rows",
                     backward="tile-form pooled supervised contrastive")


def _supcon_pool_tile(za: torch.Tensor, zb: torch.Tensor, labels: torch.Tensor, temperature, group, min_temperature: float,
                      required: bool):
    """The tile form of ``pooled_supervised_contrastive``, or None where it does not run and ``required`` is False (the caller
    then streams)."""
    _check_two_views("pooled_supervised_contrastive", za, zb)
    labels = _labels_arg(labels, za)
    _check_min_temperature(min_temperature)
    sizes, offset, b_all = _row_ranges(za.shape[0], za.device, group)
    # every rank must take the same form (they exchange different things)
    refusal = _agreed_refusal(_tile_refusal(_POOL_LIMITS, za, zb, b_all, min_temperature), za.device, group)
    if refusal is not None:
        if required:
            raise NotImplementedError("aecf_amd: the tile form of the pooled supervised contrastive loss needs " + refusal)
        return None
    t = _temperature_scalar(temperature, za, min_temperature)
    lab = labels.detach().to(torch.int64)
    na, nb = l2_normalize(za), l2_normalize(zb)
    na_all = _all_rows(na, group, sizes)
    nb_all = _all_rows(nb, group, sizes)
    lab_all = _all_rows(lab, group, sizes)
    share = _SupConPoolSymmetric.apply(na, nb, na_all, nb_all, lab, lab_all, offset, t, 0.5 / float(b_all), group,
                                       float(min_temperature))
    return _dp_value(share, group)


def pooled_supervised_contrastive(za: torch.Tensor, zb: torch.Tensor, labels: torch.Tensor,
                                  temperature: Union[float, torch.Tensor] = 0.07, group=None,
                                  min_temperature: float = MIN_TEMPERATURE, low_memory: Optional[bool] = True) -> torch.Tensor:
    """The supervised contrastive loss as published (Khosla et al. 2020) between the local rows of two views, keys from every rank
    of ``group``: the 2 B_all rows of both views are one pool, every row is an anchor against the other 2 B_all - 1 rows, and its
    positives are its partner and every row of EITHER view with the same non-negative label,

        L = 1 / (2 B_all) * sum over the 2 B_all anchors of [ logsumexp_{k != self} x_k - mean_{k in positives} x_k ],
        x = n . n_k / max(T, min_temperature)

    ``labels``: as for ``supervised_contrastive``.  ``low_memory``: which of the two implementations runs.  ``True`` (the
    default) is ``supervised_contrastive(za, zb, labels, ..., intra_view=True)``: the same streaming kernels
    (aecf_supcon_pool_fwd_bwd), bits, messages and requirements.  ``False``: the tile-GEMM form (aecf_supcon_pool_sym_pass1 /
    _loss / _grads): the three blocks of logits of ``nt_xent``'s tile form (a_loc x b_all, a_loc x a_all, b_loc x b_all, the
    anchor itself left out by index) kept as bfloat16 exponentials between forward and backward, the label positives a sparse
    correction to NT-Xent's weights whose statistics are combined over the three blocks -- 18 rows cols d matrix flops against
    the streaming form's 64.  It needs bfloat16 rows, d % 64 == 0 (64 to 4096), ``min_temperature >= 0.025``, at most 2^23
    gathered rows and its workspace (those three blocks plus float32 staging) within 0.6 of the free device memory (not tested
    while capturing), and raises NotImplementedError naming the limit otherwise; its backward runs once per forward.  With every
    label negative it has the bits of ``nt_xent(low_memory=False)``.  ``None``: the tile form wherever it runs, the streaming
    form otherwise (at 8192 x 65536 x 768 the tile form's whole range of times lies below the streaming form's, 11.0 ms against
    53.8 ms: profiles/supcon_pool_tile_time.txt).  Under data parallel the tile form gathers both views and the labels,
    the ranks agree on one form (a MIN all-reduce) and all-reduce the [3, b_all] column statistics between the passes; the
    returned value follows ``info_nce``'s convention.  ``temperature``: as for ``supervised_contrastive`` (a float or a learnable
    one-element device tensor, no host read: on one rank the call captures into a graph)."""
    if low_memory not in (True, False, None):
        raise ValueError(f"aecf_amd: low_memory must be True, False or None, got {low_memory!r}")
    if low_memory is not True:
        _require_device(za, "za")
        _require_device(zb, "zb")
        out = _supcon_pool_tile(za, zb, labels, temperature, group, min_temperature, required=low_memory is False)
        if out is not None:
            return out
    return supervised_contrastive(za, zb, labels, temperature, group, min_temperature, True, True)


SET_CLASSES = 64                                        # one uint64 per row: the most classes a label set can name
SET_WEIGHTINGS = {"overlap": _lib.AECF_SETS_OVERLAP, "jaccard": _lib.AECF_SETS_JACCARD}
_SET_KINDS = {torch.bool: _lib.AECF_SETS_U8, torch.uint8: _lib.AECF_SETS_U8, torch.bfloat16: _lib.AECF_BF16,
              torch.float16: _lib.AECF_F16, torch.float32: _lib.AECF_F32}


def _multi_hot_arg(multi_hot) -> torch.Tensor:
    """a multi-hot tensor [b, C] of ``pack_label_sets``, checked: bool, uint8, bfloat16, float16 or float32, 1 <= C <= 64"""
    if not isinstance(multi_hot, torch.Tensor):
        raise TypeError(f"aecf_amd: label sets must be a tensor, got {type(multi_hot).__name__}")
    if multi_hot.dtype not in _SET_KINDS:
        raise TypeError(f"aecf_amd: multi-hot label sets must be bool, uint8, bfloat16, float16 or float32, got {multi_hot.dtype}")
    if multi_hot.dim() != 2 or multi_hot.shape[0] < 1 or multi_hot.shape[1] < 1:
        raise ValueError(f"aecf_amd: multi-hot label sets must have shape [b, C] with b, C >= 1, got {tuple(multi_hot.shape)}")
    if multi_hot.shape[1] > SET_CLASSES:
        raise NotImplementedError(f"aecf_amd: label sets hold at most {SET_CLASSES} classes (one 64-bit mask per row), got "
                                  f"C = {multi_hot.shape[1]}")
    return multi_hot


def _label_sets_arg(label_sets, z: torch.Tensor) -> torch.Tensor:
    """``label_sets`` of ``multilabel_contrastive``, checked against the embeddings ``z`` [b_local, d]: ready int64 masks
    [b_local] (bit c = class c) or a multi-hot tensor [b_local, C <= 64], on z's device.  Returns them as they are: the caller
    packs a multi-hot tensor on the device."""
    if not isinstance(label_sets, torch.Tensor):
        raise TypeError(f"aecf_amd: label sets must be a tensor, got {type(label_sets).__name__}")
    if label_sets.dim() == 1:
        if label_sets.dtype != torch.int64:
            raise TypeError(f"aecf_amd: ready label sets (one mask per row) must be int64, got {label_sets.dtype}")
    else:
        _multi_hot_arg(label_sets)
    if label_sets.shape[0] != z.shape[0]:
        raise ValueError(f"aecf_amd: label sets must hold one set per local row ({z.shape[0]} rows), got shape {tuple(label_sets.shape)}")
    if label_sets.device != z.device:
        raise ValueError(f"aecf_amd: the label sets live on {label_sets.device}, the embeddings on {z.device}")
    return label_sets


def pack_label_sets(multi_hot: torch.Tensor) -> torch.Tensor:
    """Multi-hot rows ``[b, C]`` (bool, uint8, bfloat16, float16 or float32 on a ROCm device, C <= 64; nonzero = member) ->
    ``[b]`` int64 masks, bit c = class c (aecf_label_sets_pack: one wave per row, one ballot).  Class 63 is the sign bit of the
    int64: a row that holds it reads as a negative number, which is expected -- the kernels take the word as unsigned."""
    _multi_hot_arg(multi_hot)
    _require_device(multi_hot, "multi_hot")
    rows, classes = multi_hot.shape
    src = multi_hot.detach().contiguous()
    sets = torch.empty(rows, dtype=torch.int64, device=multi_hot.device)
    _lib.check(_lib.load().aecf_label_sets_pack(rows, classes, _SET_KINDS[multi_hot.dtype], _ptr(src), _ptr(sets), _stream()),
               "aecf_label_sets_pack")
    return sets


class _SupConMlDirection(_StreamDirection):
    """aecf_supcon_ml_fwd_bwd: sum_i [logsumexp_j(q_i.k_j/T) - the w-weighted mean of q_i.k_j/T] * coef for local unit-norm q
    against all k, w(i, j) = 1 for the partner ``row_offset + i`` and the overlap or Jaccard weight of the two rows' class sets
    (int64 masks) otherwise: ``_SupConDirection`` with sets for labels."""
    form = _StreamForm("aecf_supcon_ml_fwd_bwd", "aecf_supcon_ml_workspace_bytes", riders=("q_sets", "k_sets"),
                       options=("weighting",), offsets=("row_offset",), needs="the multi-label contrastive loss needs")


class _SupConMlSymmetric(_TileSymmetric):
    """aecf_supcon_ml_sym_pass1 / _loss / _grads: BOTH directions of the symmetric multi-label contrastive loss from one block of
    logits (local rows of view a against the gathered rows of view b), the class sets (int64 masks) shared by the two views:
    ``_SupConSymmetric`` with sets and a weighting for the labels.  The column statistics [3, cols] are the sums of the
    exponentials, of the set weights and of weight times raw score."""
    form = _TileForm("aecf_supcon_ml_sym", operands=("a", "b_all"), riders=("row_sets", "col_sets"), options=("weighting",),
                     stats=(3,),
                     needs="the tile form of the multi-label contrastive loss needs d % 64 == 0, 64 <= d <= 4096 and at most "
                           "2^24 gathered rows",
                     backward="symmetric multi-label contrastive")


def multilabel_contrastive(za: torch.Tensor, zb: torch.Tensor, label_sets: torch.Tensor, weighting: str = "overlap",
                           temperature: Union[float, torch.Tensor] = 0.07, group=None,
                           min_temperature: float = MIN_TEMPERATURE, low_memory: Optional[bool] = True) -> torch.Tensor:
    """Symmetric multi-label supervised contrastive loss between the local rows of two views, keys from every rank of ``group``:
    every row carries a SET of classes, and a row of the other view counts as a positive of row i with a weight

        w(i, j) = 1 for the partner (row i of the other view, by index, whatever the sets say), else
                  [A_i and B_j share a class]          weighting="overlap"
                  |A_i & B_j| / |A_i | B_j|            weighting="jaccard"

        L = 0.5 / B_all * sum over both directions and rows i of [ logsumexp_j x_ij - sum_j w(i, j) x_ij / sum_j w(i, j) ],
        x_ij = na_i . nb_j / max(T, min_temperature)

    ``za``, ``zb``: [b_local, d] bfloat16 on a ROCm device, d in 128, 256, 384, 512, 768, 1024 (anything else is refused: there is
    no torch fallback).  ``label_sets``, shared by both views, on the same device: a multi-hot tensor [b_local, C] of bool, uint8,
    bfloat16, float16 or float32 with C <= 64 (nonzero = member; packed on the device by ``pack_label_sets``), or ready int64
    masks [b_local] (bit c = class c; class 63 is the sign bit).  An empty set marks an unlabeled row: its only positive is its
    partner and it is nobody's positive by label.  With one-hot sets both weightings are ``supervised_contrastive``; with all
    sets empty or pairwise disjoint they are ``info_nce``.  Sets carry no gradient.

    ``low_memory``: which of the two implementations runs.  ``True`` (the default): both directions run the streaming kernels
    (aecf_supcon_ml_fwd_bwd): neither the b_local x b_all logits nor a weight matrix ever exists; the workspace is O(b_local d).
    ``False``: the tile-GEMM form (aecf_supcon_ml_sym_pass1 / _loss / _grads), both directions from ONE block of logits kept as
    b_local x b_all bfloat16 exponentials between forward and backward, the set weights formed in a dense epilogue of the logits
    GEMM and again in the weights pass.  It needs bfloat16 rows, d % 64 == 0 (64 to 4096, so it serves widths the streaming form
    does not), ``min_temperature >= 0.025`` and that block within 0.6 of the free device memory (not tested while capturing), and
    raises NotImplementedError naming the limit otherwise; its backward runs once per forward.  ``None``: the tile form wherever
    it runs, the streaming form otherwise.  Under data parallel the ranks agree on one form (they exchange different things).
    ``temperature``: a Python float or a learnable one-element float32 tensor on
    za's device, read as ``max(T, min_temperature)`` with no host read -- on one rank the call captures into a graph and replays
    the current temperature and sets -- and given its gradient by the same kernels.  Under ``torch.no_grad()``, or when no input
    requires a gradient, only the loss passes of the streaming form run and no gradient buffer is allocated.

    Data parallel: the streaming form all-gathers both views, the packed sets and the row counts; the tile form gathers view b, the
    packed sets and the row counts only and all-reduces the [3, b_all] column statistics between its passes.  The convention is
    ``info_nce``'s -- the returned value is the global loss on every rank and the local term carries ``world`` for an averaging
    gradient reduce."""
    if weighting not in SET_WEIGHTINGS:
        raise ValueError(f"aecf_amd: weighting must be 'overlap' or 'jaccard', got {weighting!r}")
    _require_device(za, "za")
    _require_device(zb, "zb")
    _check_two_views("multilabel_contrastive", za, zb)
    label_sets = _label_sets_arg(label_sets, za)
    if low_memory not in (True, False, None):
        raise ValueError(f"aecf_amd: low_memory must be True, False or None, got {low_memory!r}")
    streams = za.dtype == torch.bfloat16 and zb.dtype == torch.bfloat16 and za.shape[1] in SUPCON_WIDTHS
    if low_memory is True and not streams:
        raise NotImplementedError(f"aecf_amd: the multi-label contrastive loss needs bfloat16 rows with d in {SUPCON_WIDTHS}; got "
                                  f"{za.dtype} and {zb.dtype}, d = {za.shape[1]}")
    _check_min_temperature(min_temperature)
    sizes, offset, b_all = _row_ranges(za.shape[0], za.device, group)
    tile = False
    if low_memory is not True:
        # every rank must take the same form (they exchange different things); the single-label limits: the two tile forms
        # share their served shapes and their workspace
        refusal = _agreed_refusal(_tile_refusal(_SUPCON_LIMITS, za, zb, b_all, min_temperature), za.device, group)
        tile = refusal is None
        if not tile and (low_memory is False or not streams):
            raise NotImplementedError("aecf_amd: the tile form of the multi-label contrastive loss needs " + refusal
                                      + ("" if low_memory is False else f"; the streaming form needs bfloat16 rows with d in "
                                         f"{SUPCON_WIDTHS}, got {za.dtype} and {zb.dtype}, d = {za.shape[1]}"))
    t = _temperature_scalar(temperature, za, min_temperature)
    sets = label_sets.detach() if label_sets.dim() == 1 else pack_label_sets(label_sets)
    na, nb = l2_normalize(za), l2_normalize(zb)
    nb_all = _all_rows(nb, group, sizes)
    sets_all = _all_rows(sets, group, sizes)
    coef = 0.5 / float(b_all)
    w = SET_WEIGHTINGS[weighting]
    if tile:
        # both directions from the one block of logits this rank owns: view a is never gathered
        share = _SupConMlSymmetric.apply(na, nb_all, sets, sets_all, w, offset, t, coef, group, float(min_temperature))
    else:
        na_all = _all_rows(na, group, sizes)
        grads = torch.is_grad_enabled() and any(x.requires_grad for x in (na, nb, t))
        l_ab = _SupConMlDirection.apply(na, nb_all, sets, sets_all, w, offset, t, coef, float(min_temperature), grads)
        l_ba = _SupConMlDirection.apply(nb, na_all, sets, sets_all, w, offset, t, coef, float(min_temperature), grads)
        share = l_ab + l_ba              # this rank's rows' share of the global objective
    return _dp_value(share, group)


class _SupConMlPoolSymmetric(_TileSymmetric):
    """aecf_supcon_ml_pool_sym_pass1 / _loss / _grads: the 2 b_local anchors of this rank's pooled multi-label contrastive loss
    from the three blocks of logits of ``_NtXentSymmetric``, the class sets (int64 masks) shared by the two views:
    ``_SupConPoolSymmetric`` with sets and a weighting for the labels."""
    form = _TileForm("aecf_supcon_ml_pool_sym", operands=("a", "b", "a_all", "b_all"), riders=("row_sets", "col_sets"),
                     options=("weighting",), stats=(3,),
                     needs="the pooled multi-label contrastive loss needs d % 64 == 0, 64 <= d <= 4096 and at most 2^23 gathered "
                           "rows",
                     backward="pooled multi-label contrastive")


def pooled_multilabel_contrastive(za: torch.Tensor, zb: torch.Tensor, label_sets: torch.Tensor, weighting: str = "overlap",
                                  temperature: Union[float, torch.Tensor] = 0.07, group=None,
                                  min_temperature: float = MIN_TEMPERATURE) -> torch.Tensor:
    """The supervised contrastive loss as published (Khosla et al. 2020) with a SET of classes per row, between the local rows of
    two views, keys from every rank of ``group``: the 2 B_all rows of both views are one pool, every row is an anchor against the
    other 2 B_all - 1 rows (itself left out by index), and a key of EITHER view counts as its positive with a weight

        w = 1 for the partner (the same row of the other view, by index, whatever the sets say), else
            [A and B share a class]          weighting="overlap"
            |A & B| / |A | B|                weighting="jaccard"

        L = 0.5 / B_all * sum over the 2 B_all anchors of [ logsumexp_{k != self} x_k - sum_k w_k x_k / sum_k w_k ],
        x = n . n_k / max(T, min_temperature)

    ``label_sets``: as for ``multilabel_contrastive`` (a multi-hot tensor [b_local, C <= 64] or ready int64 masks [b_local], shared
    by both views); an empty set marks an unlabeled row: its only positive is its partner and it is nobody's positive by label.
    With all sets empty or pairwise disjoint it has the bits of ``nt_xent(low_memory=False)``; with one-hot sets both weightings
    are ``pooled_supervised_contrastive``.  Sets carry no gradient.

    There is one implementation, the tile-GEMM form (aecf_supcon_ml_pool_sym_pass1 / _loss / _grads): the three blocks of logits
    of ``nt_xent``'s tile form (a_loc x b_all, a_loc x a_all, b_loc x b_all) kept as bfloat16 exponentials between forward and
    backward, the set weights formed in a dense epilogue of each logits GEMM and again in the weights passes, their statistics
    combined over the three blocks.  It needs bfloat16 rows, d % 64 == 0 (64 to 4096), ``min_temperature >= 0.025``, at most 2^23
    gathered rows and its workspace (those three blocks plus float32 staging) within 0.6 of the free device memory (not tested
    while capturing), and raises NotImplementedError naming the limit otherwise: there is no streaming form and no torch fallback.
    Its backward runs once per forward.  ``temperature``: a float or a learnable one-element float32 device tensor, no host read:
    on one rank the call captures into a graph and replays the current temperature and sets.

    Data parallel: both views, the packed sets and the row counts are gathered, the ranks agree on refusal (a MIN all-reduce) and
    all-reduce the [3, b_all] column statistics between the passes; the returned value follows ``info_nce``'s convention -- the
    global loss on every rank, the local term carrying ``world`` for an averaging gradient reduce."""
    if weighting not in SET_WEIGHTINGS:
        raise ValueError(f"aecf_amd: weighting must be 'overlap' or 'jaccard', got {weighting!r}")
    _require_device(za, "za")
    _require_device(zb, "zb")
    _check_two_views("pooled_multilabel_contrastive", za, zb)
    label_sets = _label_sets_arg(label_sets, za)
    _check_min_temperature(min_temperature)
    sizes, offset, b_all = _row_ranges(za.shape[0], za.device, group)
    # every rank must agree (a rank that refused would leave the others waiting); the single-label limits: the two pooled tile
    # forms share their served shapes and their workspace
    refusal = _agreed_refusal(_tile_refusal(_POOL_LIMITS, za, zb, b_all, min_temperature), za.device, group)
    if refusal is not None:
        raise NotImplementedError("aecf_amd: the pooled multi-label contrastive loss (a tile form only) needs " + refusal)
    t = _temperature_scalar(temperature, za, min_temperature)
    sets = label_sets.detach() if label_sets.dim() == 1 else pack_label_sets(label_sets)
    na, nb = l2_normalize(za), l2_normalize(zb)
    na_all = _all_rows(na, group, sizes)
    nb_all = _all_rows(nb, group, sizes)
    sets_all = _all_rows(sets, group, sizes)
    share = _SupConMlPoolSymmetric.apply(na, nb, na_all, nb_all, sets, sets_all, SET_WEIGHTINGS[weighting], offset, t,
                                         0.5 / float(b_all), group, float(min_temperature))
    return _dp_value(share, group)


class RetrievalRanks(NamedTuple):
    """What ``retrieval_ranks`` returns: for each of this rank's rows, how many OTHER rows of the other view score higher than
    (``greater``) or exactly as high as (``equal``) its partner; int32 [b_local] each."""
    a2b_greater: torch.Tensor
    a2b_equal: torch.Tensor
    b2a_greater: torch.Tensor
    b2a_equal: torch.Tensor


_TIES = {"optimistic": 0.0, "average": 0.5, "pessimistic": 1.0}


def retrieval_ranks(za: torch.Tensor, zb: torch.Tensor, group=None, normalize: bool = True) -> RetrievalRanks:
    """Retrieval ranks of the contrastive views, both directions from ONE logits pass that stores nothing of size
    b_local x b_all (aecf_retrieval_positive / aecf_retrieval_ranks).  ``za``, ``zb``: [b_local, d] bfloat16 on a ROCm device,
    d % 64 == 0, 64 <= d <= 4096, the same row count on every rank; row i of one view is the partner of row i of the other.

    With s_ij = a_i . b_j (float32 accumulation) over the rows of view b from every rank of ``group``, the call returns, for
    this rank's rows, ``a2b_greater[i] = #{j != i : s_ij > s_ii}`` and ``a2b_equal`` (the same with ==), and for its rows of
    view b against the rows of view a from every rank ``b2a_greater`` / ``b2a_equal``.  A positive's rank under a tie rule f is
    ``greater + f * equal``.  A comparison with a NaN is false on both sides.

    ``normalize=True`` brings the rows to unit norm with the library's kernel first; ``False`` takes them as given.  Nothing
    is rounded to bfloat16 on the way in -- a ranking is the one output where that would change answers -- so other dtypes are
    refused.  Runs without a graph (inputs detached, outputs carry none) and without a host read: it captures on one rank.
    Data parallel: one all-gather of the rows of view b, one of the b_local positive logits, one all-reduce of the b_all int32
    column counts."""
    _require_device(za, "za")
    _require_device(zb, "zb")
    if za.shape != zb.shape or za.dim() != 2:
        raise ValueError(f"retrieval_ranks expects two [b, d] tensors of equal shape, got {tuple(za.shape)} and {tuple(zb.shape)}")
    if za.dtype != torch.bfloat16 or zb.dtype != torch.bfloat16:
        raise NotImplementedError(f"aecf_amd: retrieval_ranks takes bfloat16 rows only (nothing is rounded on the way in); got "
                                  f"{za.dtype} and {zb.dtype}")
    rows, d = za.shape
    if d % 64 != 0 or not 64 <= d <= 4096:
        raise NotImplementedError(f"aecf_amd: retrieval_ranks needs d % 64 == 0 and 64 <= d <= 4096, got d = {d}")
    lib = _lib.load()
    rank, world = dp.world_info(group)
    cols, offset = rows * world, rank * rows
    ws_bytes = lib.aecf_retrieval_workspace_bytes(rows, cols, d)
    if ws_bytes == 0:
        raise NotImplementedError(f"aecf_amd: retrieval_ranks does not serve {rows} x {cols} x {d}")
    with torch.no_grad():
        a, b = za.detach(), zb.detach()
        if normalize:
            a, b = l2_normalize(a), l2_normalize(b)
        a, b = a.contiguous(), b.contiguous()
        b_all = dp.all_gather_rows(b, group, sizes=[rows] * world).contiguous() if world > 1 else b
        dev = za.device
        pos = torch.empty(rows, dtype=torch.float32, device=dev)
        _lib.check(lib.aecf_retrieval_positive(rows, cols, offset, d, _ptr(a), _ptr(b_all), _ptr(pos), _stream()),
                   "aecf_retrieval_positive")
        pos_all = dp.all_gather_rows(pos, group, sizes=[rows] * world).contiguous() if world > 1 else pos
        i32 = dict(dtype=torch.int32, device=dev)
        row_g, row_e = torch.empty(rows, **i32), torch.empty(rows, **i32)
        col = torch.empty(2, cols, **i32)                    # greater | equal: one all-reduce
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.aecf_retrieval_ranks(rows, cols, offset, d, _ptr(a), _ptr(b_all), _ptr(pos), _ptr(pos_all), _ptr(row_g),
                                            _ptr(row_e), _ptr(col[0]), _ptr(col[1]), _ptr(ws), ws_bytes, _stream()),
                   "aecf_retrieval_ranks")
        if world > 1:
            torch.distributed.all_reduce(col, group=group)
        return RetrievalRanks(row_g, row_e, col[0, offset:offset + rows], col[1, offset:offset + rows])


def retrieval_metrics(za: torch.Tensor, zb: torch.Tensor, ks: Sequence[int] = (1, 5, 10), group=None, ties: str = "average",
                      normalize: bool = True) -> dict:
    """Recall@k, mean reciprocal rank and mean rank of both retrieval directions, global over ``group``, from
    ``retrieval_ranks``.  The 0-based rank of a positive is ``greater + f * equal`` with f = 0 (``ties="optimistic"``), 0.5
    (``"average"``) or 1 (``"pessimistic"``).  Returns 0-dim float32 device tensors: ``a2b_R@k`` / ``b2a_R@k`` for every k in
    ``ks`` (the share of rows with rank < k), ``a2b_mrr`` / ``b2a_mrr`` (mean of 1 / (rank + 1)) and ``a2b_mean_rank`` /
    ``b2a_mean_rank``.  The means over this rank's rows are torch reductions; the ranks exchange one all-reduce of one small
    vector.  No host read."""
    if ties not in _TIES:
        raise ValueError(f"aecf_amd: ties must be one of {sorted(_TIES)}, got {ties!r}")
    ks = tuple(ks)
    if not ks or any(isinstance(k, bool) or not isinstance(k, int) or k <= 0 for k in ks):
        raise ValueError(f"aecf_amd: ks must be positive integers, got {ks!r}")
    r = retrieval_ranks(za, zb, group, normalize)
    f = _TIES[ties]
    world = dp.world_info(group)[1]
    with torch.no_grad():
        sums = []
        for g, e in ((r.a2b_greater, r.a2b_equal), (r.b2a_greater, r.b2a_equal)):
            # float64 sums: every term is exact there, so the value does not depend on how the rows are dealt over ranks
            rank = g.to(torch.float64) + f * e.to(torch.float64)
            sums += [(rank < k).to(torch.float64).sum() for k in ks] + [(1.0 / (rank + 1.0)).sum(), rank.sum()]
        vec = torch.stack(sums)
        if world > 1:
            torch.distributed.all_reduce(vec, group=group)
        vec = (vec / float(za.shape[0] * world)).to(torch.float32)
    names = [f"R@{k}" for k in ks] + ["mrr", "mean_rank"]
    return {f"{side}_{n}": vec[i * len(names) + j] for i, side in enumerate(("a2b", "b2a")) for j, n in enumerate(names)}


class RetrievalTopK(NamedTuple):
    """What ``retrieval_topk`` returns: for each of this rank's queries the scores (``values``, float32 [b_local, k], best
    first) and the positions (``indices``, int64 [b_local, k]) of its k best keys; a position indexes the keys of every rank in
    all-gather order (rank r's key j is ``r * b_k + j``)."""
    values: torch.Tensor
    indices: torch.Tensor


def retrieval_topk(queries: torch.Tensor, keys: torch.Tensor, k: int, group=None, normalize: bool = True,
                   exclude_partner: bool = False) -> RetrievalTopK:
    """The k best keys of every query, from ONE logits pass that stores nothing of size b_local x b_all (aecf_retrieval_topk):
    hard negatives between steps, kNN evaluation, a look at what a query retrieves, the input of a re-ranking stage.
    ``queries``: [b_q, d], ``keys``: [b_k, d], bfloat16 on a ROCm device, d % 64 == 0, 64 <= d <= 4096, 1 <= k <= 16, the same
    row counts on every rank.  b_q and b_k may differ unless ``exclude_partner`` is set.

    With s_ij = q_i . key_j (float32 accumulation) over the keys of every rank of ``group``, row i of the result lists the k
    first keys of row i of s in a fixed total order: the higher score first; among equal scores the lower index first; NaN
    scores, all equal to each other, after -inf.  The order is total, so the answer does not depend on how the keys are dealt
    over ranks.  ``exclude_partner=True`` (shapes must be equal) leaves out the query's own partner, global key
    ``rank * b_local + i`` for local row i -- what hard-negative mining wants.  k may not exceed the keys that remain.

    One direction per call: for the best queries of every key swap the arguments.  ``normalize=True`` brings the rows to unit
    norm with the library's kernel first; ``False`` takes them as given.  Nothing is rounded to bfloat16 on the way in -- a
    ranking is the one output where that would change answers -- so other dtypes are refused.  Runs without a graph (inputs
    detached, outputs carry none) and without a host read: it captures on one rank.  Data parallel: one all-gather of the keys
    and nothing else; each rank answers for its own queries."""
    _require_device(queries, "queries")
    _require_device(keys, "keys")
    if queries.dim() != 2 or keys.dim() != 2 or queries.shape[1] != keys.shape[1]:
        raise ValueError(f"retrieval_topk expects queries [b_q, d] and keys [b_k, d], got {tuple(queries.shape)} and {tuple(keys.shape)}")
    if exclude_partner and queries.shape != keys.shape:
        raise ValueError(f"retrieval_topk with exclude_partner expects two [b, d] tensors of equal shape, got {tuple(queries.shape)} "
                         f"and {tuple(keys.shape)}")
    if isinstance(k, bool) or not isinstance(k, int) or k <= 0:
        raise ValueError(f"aecf_amd: retrieval_topk needs a positive integer k, got {k!r}")
    if queries.dtype != torch.bfloat16 or keys.dtype != torch.bfloat16:
        raise NotImplementedError(f"aecf_amd: retrieval_topk takes bfloat16 rows only (nothing is rounded on the way in); got "
                                  f"{queries.dtype} and {keys.dtype}")
    rows, d = queries.shape
    if d % 64 != 0 or not 64 <= d <= 4096:
        raise NotImplementedError(f"aecf_amd: retrieval_topk needs d % 64 == 0 and 64 <= d <= 4096, got d = {d}")
    if k > 16:
        raise NotImplementedError(f"aecf_amd: retrieval_topk serves k <= 16, got k = {k}")
    rank, world = dp.world_info(group)
    b_k = keys.shape[0]
    cols, offset = b_k * world, rank * rows
    left = cols - (1 if exclude_partner else 0)
    if rows == 0 or k > left:
        raise ValueError(f"aecf_amd: retrieval_topk needs at least one query and k <= the {left} keys to choose from, got "
                         f"{rows} queries and k = {k}")
    lib = _lib.load()
    ws_bytes = lib.aecf_retrieval_topk_workspace_bytes(rows, cols, d, k)
    if ws_bytes == 0:
        raise NotImplementedError(f"aecf_amd: retrieval_topk does not serve {rows} x {cols} x {d}, k = {k}")
    with torch.no_grad():
        a, b = queries.detach(), keys.detach()
        if normalize:
            a, b = l2_normalize(a), l2_normalize(b)
        a, b = a.contiguous(), b.contiguous()
        b_all = dp.all_gather_rows(b, group, sizes=[b_k] * world).contiguous() if world > 1 else b
        dev = queries.device
        values = torch.empty(rows, k, dtype=torch.float32, device=dev)
        indices = torch.empty(rows, k, dtype=torch.int32, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.aecf_retrieval_topk(rows, cols, offset, d, k, 1 if exclude_partner else 0, _ptr(a), _ptr(b_all), _ptr(values),
                                           _ptr(indices), _ptr(ws), ws_bytes, _stream()), "aecf_retrieval_topk")
        return RetrievalTopK(values, indices.to(torch.int64))


def fusion_objective(task_loss: torch.Tensor, masking: Optional[CurriculumMasking], entropy: Optional[torch.Tensor],
                     za: Optional[torch.Tensor] = None, zb: Optional[torch.Tensor] = None, entropy_weight: float = 0.01,
                     contrastive_weight: float = 1.0, temperature: Union[float, torch.Tensor] = 0.07, group=None,
                     min_temperature: float = MIN_TEMPERATURE, contrastive: str = "info_nce",
                     bias: Union[None, float, torch.Tensor] = None, low_memory: Optional[bool] = None,
                     labels: Optional[torch.Tensor] = None, label_weighting: str = "overlap",
                     intra_view: bool = False, queue: Optional["KeyQueue"] = None) -> torch.Tensor:
    """task + entropy_weight * entropy_loss(entropy) [ref README.md:205-208] + contrastive_weight * info_nce(za, zb)
    (``temperature`` / ``min_temperature``: as for ``info_nce``).  ``contrastive="sigmoid"`` takes ``sigmoid_contrastive(za, zb,
    temperature, bias)`` as the contrastive term instead (``bias``: None = its default of -10; ``low_memory``: its choice of
    implementation, ignored for ``info_nce``); ``contrastive="supervised"`` takes ``supervised_contrastive(za, zb, labels,
    temperature)`` -- handed ``low_memory`` when it is not None (False: the tile-GEMM form), its own default (the streaming form)
    otherwise -- and ``contrastive="multilabel"`` takes ``multilabel_contrastive(za, zb, labels, label_weighting,
    temperature)``, handed ``low_memory`` in the same way, with ``labels`` the label sets (multi-hot rows or int64 masks); these two, ``supervised_pool`` and ``multilabel_pool`` are the only forms that take
    ``labels``, and ``label_weighting`` ("overlap" or "jaccard") is read by the multi-label forms alone.  ``contrastive="nt_xent"``
    takes ``nt_xent(za, zb, temperature)``, the pool of both views without labels, handed ``low_memory`` when it is not None
    (False: its tile-GEMM form) and its own default (the streaming form) otherwise; ``intra_view`` is handed to the supervised
    form (True: the same pool with label positives from either view) and read by no other.
    ``contrastive="supervised_pool"`` takes ``pooled_supervised_contrastive(za, zb, labels, temperature)``, that pooled loss
    under a name of its own, handed ``low_memory`` when it is not None (False: its tile-GEMM form) and its own default (the
    streaming form) otherwise; it takes ``labels`` and ignores ``intra_view``.
    ``contrastive="multilabel_pool"`` takes ``pooled_multilabel_contrastive(za, zb, labels, label_weighting, temperature)``, the
    same pool with label sets: it takes ``labels`` (the sets) and ``label_weighting`` and ignores ``intra_view``; ``low_memory``
    None or False select its one implementation, the tile-GEMM form, and True raises NotImplementedError (there is no streaming
    form).
    ``contrastive="queued"`` takes ``queued_info_nce(za, zb, queue, temperature)`` and ``contrastive="supervised_queued"`` takes
    ``queued_supervised_contrastive(za, zb, labels, queue, temperature)`` (it takes ``labels``; the queue must hold a label ring):
    the two forms that take ``queue``, a ``KeyQueue`` the caller pushes to after the backward.  They have one implementation
    (``low_memory`` is not read); ``queue`` given to any other form raises ValueError."""
    with_labels = ("supervised", "multilabel", "supervised_pool", "multilabel_pool", "supervised_queued")
    with_queue = ("queued", "supervised_queued")
    if contrastive not in ("info_nce", "sigmoid", "supervised", "multilabel", "nt_xent", "supervised_pool", "multilabel_pool",
                           "queued", "supervised_queued"):
        raise ValueError(f"aecf_amd: contrastive must be 'info_nce', 'sigmoid', 'supervised', 'multilabel', 'nt_xent', "
                         f"'supervised_pool', 'multilabel_pool', 'queued' or 'supervised_queued', got {contrastive!r}")
    if contrastive in with_labels and labels is None:
        raise ValueError(f"aecf_amd: contrastive={contrastive!r} needs labels")
    if contrastive not in with_labels and labels is not None:
        raise ValueError(f"aecf_amd: labels are taken by contrastive='supervised', 'multilabel', 'supervised_pool', "
                         f"'multilabel_pool' and 'supervised_queued' only, got contrastive={contrastive!r}")
    if contrastive in with_queue and queue is None:
        raise ValueError(f"aecf_amd: contrastive={contrastive!r} needs queue, a KeyQueue")
    if contrastive not in with_queue and queue is not None:
        raise ValueError(f"aecf_amd: queue is taken by contrastive='queued' and 'supervised_queued' only, got "
                         f"contrastive={contrastive!r}")
    if label_weighting not in SET_WEIGHTINGS:
        raise ValueError(f"aecf_amd: label_weighting must be 'overlap' or 'jaccard', got {label_weighting!r}")
    total = task_loss
    if masking is not None and entropy is not None:
        total = _plus(total, entropy_weight * masking.entropy_loss(entropy))
    if za is not None and zb is not None:
        if contrastive == "multilabel":
            if low_memory is None:
                term = multilabel_contrastive(za, zb, labels, label_weighting, temperature, group, min_temperature)
            else:
                term = multilabel_contrastive(za, zb, labels, label_weighting, temperature, group, min_temperature, low_memory)
        elif contrastive == "supervised":
            if low_memory is None:
                term = supervised_contrastive(za, zb, labels, temperature, group, min_temperature, intra_view=intra_view)
            else:
                term = supervised_contrastive(za, zb, labels, temperature, group, min_temperature, low_memory, intra_view)
        elif contrastive == "sigmoid":
            term = sigmoid_contrastive(za, zb, temperature, -10.0 if bias is None else bias, group, min_temperature, low_memory)
        elif contrastive == "nt_xent":
            if low_memory is None:
                term = nt_xent(za, zb, temperature, group, min_temperature)
            else:
                term = nt_xent(za, zb, temperature, group, min_temperature, low_memory)
        elif contrastive == "supervised_pool":
            if low_memory is None:
                term = pooled_supervised_contrastive(za, zb, labels, temperature, group, min_temperature)
            else:
                term = pooled_supervised_contrastive(za, zb, labels, temperature, group, min_temperature, low_memory)
        elif contrastive == "multilabel_pool":
            if low_memory is True:
                raise NotImplementedError("aecf_amd: contrastive='multilabel_pool' has no streaming form (low_memory=True); "
                                          "low_memory=None or False take its tile-GEMM form")
            term = pooled_multilabel_contrastive(za, zb, labels, label_weighting, temperature, group, min_temperature)
        elif contrastive == "queued":
            term = queued_info_nce(za, zb, queue, temperature, group, min_temperature)
        elif contrastive == "supervised_queued":
            term = queued_supervised_contrastive(za, zb, labels, queue, temperature, group, min_temperature)
        else:
            term = info_nce(za, zb, temperature, group, min_temperature)
        total = _plus(total, contrastive_weight * term)
    return total


# ---------------------------------------------------------------------------------------------------------------------------
# Multi-label classification loss: binary cross-entropy, focal and asymmetric loss as one elementwise formula
# (aecf_mlloss_forward / _backward, include/aecf_hip.h "multi-label classification loss"); replaces the torch criterion of the
# reference's example, nn.BCEWithLogitsLoss (ref xrays/train_xrays_example.py:327, 366, 374).
# ---------------------------------------------------------------------------------------------------------------------------

_MLLOSS_LABEL_KINDS = {torch.float32: _lib.AECF_F32, torch.bfloat16: _lib.AECF_BF16, torch.float16: _lib.AECF_F16,
                       torch.bool: _lib.AECF_MLLOSS_U8, torch.uint8: _lib.AECF_MLLOSS_U8, torch.int8: _lib.AECF_MLLOSS_I8}
_MLLOSS_LOGIT_KINDS = {torch.float32: _lib.AECF_F32, torch.bfloat16: _lib.AECF_BF16, torch.float16: _lib.AECF_F16}
_MLLOSS_REDUCTIONS = {"mean": _lib.AECF_MLLOSS_MEAN, "sum": _lib.AECF_MLLOSS_SUM}
MLLOSS_MAX_CLASSES = 4096
MLLOSS_MAX_ELEMENTS = 1 << 30


class _MultilabelLoss(torch.autograd.Function):
    """aecf_mlloss_forward (two launches: the pass over (logits, targets) and the fixed-order finalize) and aecf_mlloss_backward
    (one launch that recomputes the element and reads its scale, upstream * factor / N, on the device).  Returns the reduced
    loss (0-dim float32) and the float64 [2, C] stats (loss sums | valid counts per class), global over ``group`` after ONE
    all-reduce of the stats.  Nothing of size n x C is kept between the passes; nothing is read on the host."""

    @staticmethod
    def forward(ctx, logits, targets, pos_scale, neg_scale, gamma_pos, gamma_neg, margin, eps, reduction, group):
        lib = _lib.load()
        rows, C = logits.shape
        dev = logits.device
        x, y = logits.detach(), targets.detach()         # (the steps of a host-bound call are counted: no op that does nothing)
        if not x.is_contiguous():
            x = x.contiguous()
        if not y.is_contiguous():
            y = y.contiguous()
        if y.dtype == torch.bool:
            y = y.view(torch.uint8)
        kinds = (_MLLOSS_LOGIT_KINDS[x.dtype], _MLLOSS_LABEL_KINDS[targets.dtype])
        opts = (float(gamma_pos), float(gamma_neg), float(margin), float(eps), _MLLOSS_REDUCTIONS[reduction])
        world = dp.world_info(group)[1]
        stats = torch.empty(2, C, dtype=torch.float64, device=dev)
        totals = torch.empty(6, dtype=torch.float32, device=dev)     # the 24-byte record: float64 sum, float64 N, float32 loss, 0
        if rows == 0:                       # an empty shard: nothing to launch, its stats are zeros
            stats.zero_()
            totals.zero_()
        else:
            ws_bytes = lib.aecf_mlloss_workspace_bytes(rows, C)
            if ws_bytes == 0:
                raise NotImplementedError(f"aecf_amd: multilabel_loss serves C <= {MLLOSS_MAX_CLASSES} and n * C <= 2**30 per rank, "
                                          f"got {rows} x {C}")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.aecf_mlloss_forward(rows, C, *kinds, _ptr(x), _ptr(y), _ptr(pos_scale), _ptr(neg_scale), *opts,
                                               _ptr(stats), _ptr(totals), _ptr(ws), ws_bytes, _stream()), "aecf_mlloss_forward")
        if world > 1:
            torch.distributed.all_reduce(stats, group=group)
            total, count = stats[0].sum(), stats[1].sum()
            if reduction == "mean":
                value = torch.where(count > 0, total / torch.where(count > 0, count, torch.ones_like(count)), torch.zeros_like(total))
            else:
                value = total
            totals = torch.stack((total, count, torch.zeros_like(total)))
            loss = value.to(torch.float32)
        else:
            loss = totals[4]
        ctx.save_for_backward(x, y, pos_scale, neg_scale, totals)
        ctx.meta = (rows, C, kinds, opts, float(world))
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss, _d_stats):
        lib = _lib.load()
        x, y, pos_scale, neg_scale, totals = ctx.saved_tensors
        rows, C, kinds, opts, factor = ctx.meta
        dx = torch.empty_like(x)
        if rows > 0:
            up = d_loss if d_loss.dtype == torch.float32 else d_loss.to(torch.float32)       # one element, read on the device
            _lib.check(lib.aecf_mlloss_backward(rows, C, *kinds, _ptr(x), _ptr(y), _ptr(pos_scale), _ptr(neg_scale), *opts,
                                                _ptr(totals), _ptr(up), factor, _ptr(dx), _stream()), "aecf_mlloss_backward")
        return dx, None, None, None, None, None, None, None, None, None


def _class_vector(value, name: str, C: int, device) -> Optional[torch.Tensor]:
    """``pos_weight`` / ``class_weight`` as a float32 [C] tensor on the device.  A sequence is checked on the host (finite, not
    negative); a tensor is taken as it is -- checking it would be a host read."""
    if value is None:
        return None
    if isinstance(value, torch.Tensor):
        if value.dim() != 1 or value.shape[0] != C:
            raise ValueError(f"aecf_amd: {name} must hold one value per class, [{C}], got shape {tuple(value.shape)}")
        if not value.dtype.is_floating_point:
            raise TypeError(f"aecf_amd: a tensor {name} must be floating point, got {value.dtype}")
        return value.detach().to(device=device, dtype=torch.float32)
    if isinstance(value, (str, bytes)) or not hasattr(value, "__len__"):
        raise TypeError(f"aecf_amd: {name} must be a [C] tensor or a sequence of numbers, got {type(value).__name__}")
    vals = [float(v) for v in value]
    if len(vals) != C:
        raise ValueError(f"aecf_amd: {name} must hold one value per class, {C}, got {len(vals)}")
    if any(not (v >= 0.0 and v != float("inf")) for v in vals):
        raise ValueError(f"aecf_amd: {name} must be finite and not negative")
    return torch.tensor(vals, dtype=torch.float32, device=device)


def _compute_scales(pos_weight, class_weight, alpha, C: int, device):
    """a = w p (alpha or 1), b = w ((1 - alpha) or 1) as float32 [C] device tensors, None where the vector is all ones"""
    p = _class_vector(pos_weight, "pos_weight", C, device)
    w = _class_vector(class_weight, "class_weight", C, device)
    a, b = w, w
    if p is not None:
        a = p if a is None else a * p
    if alpha is not None:
        a = torch.full((C,), alpha, dtype=torch.float32, device=device) if a is None else a * alpha
        b = torch.full((C,), 1.0 - alpha, dtype=torch.float32, device=device) if b is None else b * (1.0 - alpha)
    return (None if a is None else a.contiguous()), (None if b is None else b.contiguous())


def _weight_key(value):
    """what names a weight argument in a fold's key: a tensor by identity and version, a sequence by its values"""
    if value is None or isinstance(value, torch.Tensor):
        return (id(value), getattr(value, "_version", None))
    try:
        return tuple(float(v) for v in value)
    except TypeError:
        return (id(value), None)


_mlloss_scales: list = []           # the functional form's last fold: (key, the objects the key names, pos_scale, neg_scale)


def _fold_scales(pos_weight, class_weight, alpha, C: int, device):
    """The scale vectors of the FUNCTIONAL form.  The last fold is kept and reused while the same weights come again (tensors by
    identity and version, sequences by value); another call's weights replace it.  A captured graph holds the vectors' addresses,
    not the vectors: a caller that captures the functional form with ``alpha`` or with both weights keeps the fold alive by not
    calling it with other weights -- or uses ``MultilabelLoss``, which owns its vectors."""
    if pos_weight is None and class_weight is None and alpha is None:
        return None, None
    key = (_weight_key(pos_weight), _weight_key(class_weight), alpha, C, str(device))
    if _mlloss_scales and _mlloss_scales[0][0] == key:
        return _mlloss_scales[0][2], _mlloss_scales[0][3]
    a, b = _compute_scales(pos_weight, class_weight, alpha, C, device)
    _mlloss_scales[:] = [(key, (pos_weight, class_weight), a, b)]
    return a, b


def _unit_interval(value, name: str, closed_top: bool = False) -> float:
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise TypeError(f"aecf_amd: {name} must be a Python number, got {type(value).__name__}")
    v = float(value)
    if not (0.0 <= v <= 1.0 if closed_top else 0.0 <= v < 1.0):
        raise ValueError(f"aecf_amd: {name} must lie in [0, 1{']' if closed_top else ')'}, got {value!r}")
    return v


def _gamma(value, name: str) -> float:
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise TypeError(f"aecf_amd: {name} must be a Python number, got {type(value).__name__}")
    v = float(value)
    if not (0.0 <= v < float("inf")):
        raise ValueError(f"aecf_amd: {name} must be finite and >= 0, got {value!r}")
    return v


def multilabel_loss(logits: torch.Tensor, targets: torch.Tensor, *, pos_weight=None, class_weight=None, alpha: Optional[float] = None,
                    gamma_pos: float = 0.0, gamma_neg: float = 0.0, margin: float = 0.0, label_smoothing: float = 0.0,
                    reduction: str = "mean", group=None, return_per_class: bool = False, _fold=_fold_scales):
    """The multi-label classification loss of ``logits`` [n, C] (float32, bfloat16 or float16 on a ROCm device, read as stored)
    against ``targets`` [n, C], in float32 on the library's kernels.  With s = sigmoid(x), t' = t (1 - label_smoothing) +
    label_smoothing / 2, q = max(s - margin, 0), a = class_weight * pos_weight * (alpha or 1) and b = class_weight * ((1 - alpha)
    or 1) per class:

        l = - a t' (1 - s)^gamma_pos log s  -  b (1 - t') q^gamma_neg log(1 - q)            (p^0 = 1 for every p)

    ``gamma_pos = gamma_neg = margin = 0`` is ``F.binary_cross_entropy_with_logits(x, t, weight=class_weight,
    pos_weight=pos_weight)`` (soft targets included); ``gamma_pos = gamma_neg = gamma`` with ``alpha`` is the focal loss (Lin et
    al. 2017); hard targets with ``(gamma_pos, gamma_neg, margin) = (0, 4, 0.05)`` are the asymmetric loss (Ridnik et al. 2021)
    without its 1e-8 clamps.  Where s - margin <= 0 in float32 the second term and its gradient are exact zeros.

    UNKNOWN targets are left out of the loss and of its normalisation: a floating-point target that is NaN or < 0, a negative
    int8 target (bool and uint8 have no unknown value; an integer target that is not zero counts as 1).  Their gradient is an
    exact zero and their logit reaches no output.  ``reduction="mean"`` divides by the number N of valid elements over all
    ranks (N = 0: loss 0, zero gradients); ``"sum"`` does not divide; there is no ``"none"``.

    Returns a 0-dim float32 device tensor; with ``return_per_class`` also a detached float32 [C]: the mean loss over the valid
    elements of each class, 0 where a class has none.  Once differentiable.  Data parallel (``group``): ONE all-reduce of the
    float64 [2, C] stats; the value is the global loss on every rank and the gradient carries ``world / N`` for the averaging
    collectives of ``dp`` (the convention of the contrastive drivers).  Shards may be uneven or empty.  ``pos_weight`` /
    ``class_weight``: [C] tensors or sequences, folded into the two scale vectors with torch ops on [C] tensors (the last fold
    is reused while the same weights come again; ``MultilabelLoss`` owns its folds, which is what a captured step needs).  There is no torch fallback: unserved shapes raise NotImplementedError."""
    _require_device(logits, "logits")
    _require_device(targets, "targets")
    if logits.dim() != 2 or targets.shape != logits.shape:
        raise ValueError(f"multilabel_loss expects logits and targets of one shape [n, C], got {tuple(logits.shape)} and "
                         f"{tuple(targets.shape)}")
    if logits.dtype not in _MLLOSS_LOGIT_KINDS:
        raise TypeError(f"aecf_amd: multilabel_loss takes float32, bfloat16 or float16 logits, got {logits.dtype}")
    if targets.dtype not in _MLLOSS_LABEL_KINDS:
        raise TypeError(f"aecf_amd: multilabel_loss takes float32, bfloat16, float16, bool, uint8 or int8 targets, got {targets.dtype}")
    if targets.device != logits.device:
        raise ValueError(f"aecf_amd: the targets live on {targets.device}, the logits on {logits.device}")
    if reduction not in _MLLOSS_REDUCTIONS:
        raise ValueError(f"aecf_amd: multilabel_loss reduces by 'mean' or 'sum' (there is no 'none'), got {reduction!r}")
    gamma_pos, gamma_neg = _gamma(gamma_pos, "gamma_pos"), _gamma(gamma_neg, "gamma_neg")
    margin = _unit_interval(margin, "margin")
    eps = _unit_interval(label_smoothing, "label_smoothing")
    if alpha is not None:
        alpha = _unit_interval(alpha, "alpha", closed_top=True)
    rows, C = logits.shape
    if C < 1:
        raise ValueError("aecf_amd: multilabel_loss needs at least one class")
    if C > MLLOSS_MAX_CLASSES or rows * C > MLLOSS_MAX_ELEMENTS:
        raise NotImplementedError(f"aecf_amd: multilabel_loss serves C <= {MLLOSS_MAX_CLASSES} and n * C <= 2**30 per rank, got "
                                  f"{rows} x {C}")
    a, b = _fold(pos_weight, class_weight, alpha, C, logits.device)
    loss, stats = _MultilabelLoss.apply(logits, targets, a, b, gamma_pos, gamma_neg, margin, eps, reduction, group)
    if not return_per_class:
        return loss
    count = stats[1]
    per_class = torch.where(count > 0, stats[0] / torch.where(count > 0, count, torch.ones_like(count)), torch.zeros_like(count))
    return loss, per_class.to(torch.float32)


class MultilabelLoss(torch.nn.Module):
    """``multilabel_loss`` with its options fixed, called as ``criterion(logits, labels)``: a drop-in for the criterion of
    ``xray.train_step`` and ``xray.GraphedTrainStep``.  ``pos_weight`` / ``class_weight`` are kept as float32 buffers (they move
    with the module).  The module OWNS its folded scale vectors: one fold per device and state of the buffers (identity and
    version), kept for the module's life, so the addresses a captured graph holds stay valid whatever other losses are called
    in between.  (A graph captured before the buffers were edited or moved keeps reading the fold of its capture.)"""

    def __init__(self, pos_weight=None, class_weight=None, alpha: Optional[float] = None, gamma_pos: float = 0.0,
                 gamma_neg: float = 0.0, margin: float = 0.0, label_smoothing: float = 0.0, reduction: str = "mean", group=None):
        super().__init__()
        if reduction not in _MLLOSS_REDUCTIONS:
            raise ValueError(f"aecf_amd: multilabel_loss reduces by 'mean' or 'sum' (there is no 'none'), got {reduction!r}")
        self.gamma_pos, self.gamma_neg = _gamma(gamma_pos, "gamma_pos"), _gamma(gamma_neg, "gamma_neg")
        self.margin = _unit_interval(margin, "margin")
        self.label_smoothing = _unit_interval(label_smoothing, "label_smoothing")
        self.alpha = None if alpha is None else _unit_interval(alpha, "alpha", closed_top=True)
        self.reduction, self.group = reduction, group
        for name, value in (("pos_weight", pos_weight), ("class_weight", class_weight)):
            if value is not None and not isinstance(value, torch.Tensor):
                value = _class_vector(value, name, len(value), "cpu")
            self.register_buffer(name, None if value is None else value.detach().to(torch.float32).clone())
        self._folds = {}                    # (buffers' identity and version, C, device) -> (pos_scale, neg_scale), never dropped

    def _fold(self, pos_weight, class_weight, alpha, C: int, device):
        if pos_weight is None and class_weight is None and alpha is None:
            return None, None
        key = (_weight_key(pos_weight), _weight_key(class_weight), alpha, C, str(device))
        if key not in self._folds:
            # (the entry holds the tensors its key names by id(): an id is not reused while its object lives)
            self._folds[key] = _compute_scales(pos_weight, class_weight, alpha, C, device) + (pos_weight, class_weight)
        return self._folds[key][:2]

    def forward(self, logits: torch.Tensor, targets: torch.Tensor, return_per_class: bool = False):
        return multilabel_loss(logits, targets, pos_weight=self.pos_weight, class_weight=self.class_weight, alpha=self.alpha,
                               gamma_pos=self.gamma_pos, gamma_neg=self.gamma_neg, margin=self.margin,
                               label_smoothing=self.label_smoothing, reduction=self.reduction, group=self.group,
                               return_per_class=return_per_class, _fold=self._fold)

    def extra_repr(self) -> str:
        return (f"gamma_pos={self.gamma_pos}, gamma_neg={self.gamma_neg}, margin={self.margin}, alpha={self.alpha}, "
                f"label_smoothing={self.label_smoothing}, reduction={self.reduction!r}")


def class_balance_weights(labels: torch.Tensor, group=None, max_weight: Optional[float] = None) -> torch.Tensor:
    """``pos_weight[c] = n_neg[c] / n_pos[c]`` over the valid labels [n, C] of every rank of ``group`` (``multilabel_loss``'s
    rule for unknown targets; a valid target counts as positive iff it is not zero), 1 where a class has no positive, clamped to
    ``max_weight`` if given.  A float32 [C] device tensor; torch reductions over the label matrix, run once before training --
    nothing is read on the host on one rank, the ranks join their float64 [2, C] counts in one all-reduce."""
    _require_device(labels, "labels")
    if labels.dim() != 2:
        raise ValueError(f"class_balance_weights expects labels [n, C], got {tuple(labels.shape)}")
    if labels.dtype not in _MLLOSS_LABEL_KINDS:
        raise TypeError(f"aecf_amd: class_balance_weights takes float32, bfloat16, float16, bool, uint8 or int8 labels, got {labels.dtype}")
    if max_weight is not None and not (isinstance(max_weight, (int, float)) and not isinstance(max_weight, bool) and max_weight > 0):
        raise ValueError(f"aecf_amd: max_weight must be a positive number, got {max_weight!r}")
    with torch.no_grad():
        y = labels.detach()
        valid = torch.ones_like(y, dtype=torch.bool) if y.dtype in (torch.bool, torch.uint8) else y >= 0
        pos = valid & (y != 0)
        counts = torch.stack((pos.sum(0), valid.sum(0))).to(torch.float64)
        if dp.world_info(group)[1] > 1:
            torch.distributed.all_reduce(counts, group=group)
        n_pos, n_neg = counts[0], counts[1] - counts[0]
        w = torch.where(n_pos > 0, n_neg / torch.where(n_pos > 0, n_pos, torch.ones_like(n_pos)), torch.ones_like(n_pos))
        if max_weight is not None:
            w = w.clamp(max=float(max_weight))
        return w.to(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# Fused classifier head: that loss of hidden @ W.T + b and all three gradients without the [n, C] logits
# (aecf_mlhead_forward / _backward, include/aecf_hip.h "fused classifier head"); replaces classifier[3] of the reference
# example's model together with its criterion.
# ---------------------------------------------------------------------------------------------------------------------------

MLHEAD_WIDTHS = (128, 256, 384, 512, 768, 1024)
MLHEAD_MAX_CLASSES = 65536
_MLHEAD_ALTERNATIVE = "use F.linear(hidden, weight, bias) with multilabel_loss"


class _LinearMultilabelLoss(torch.autograd.Function):
    """aecf_mlhead_forward (the CLS role over the rows, the combine of its splits, the totals) and aecf_mlhead_backward (the ROW
    role for d hidden where it is wanted, the scaling of dW / dbias).  ``want_params``: the forward also forms the unscaled
    float32 dW and dbias, which are all it saves beside the inputs and the 24-byte totals; the split slabs are transient.
    Returns the reduced loss and the float64 [2, C] stats, global over ``group`` after ONE all-reduce of the stats."""

    @staticmethod
    def forward(ctx, hidden, weight, bias, targets, pos_scale, neg_scale, gamma_pos, gamma_neg, margin, eps, reduction, group,
                want_params):
        lib = _lib.load()
        rows, K = hidden.shape
        C = weight.shape[0]
        dev = hidden.device
        h, w, y = hidden.detach(), weight.detach(), targets.detach()
        if not h.is_contiguous():
            h = h.contiguous()
        if not w.is_contiguous():
            w = w.contiguous()
        if not y.is_contiguous():
            y = y.contiguous()
        if y.dtype == torch.bool:
            y = y.view(torch.uint8)
        b = None
        if bias is not None:
            b = bias.detach()
            if b.dtype != torch.float32:
                b = b.to(torch.float32)                 # [C]: the kernels add the bias in float32
            if not b.is_contiguous():
                b = b.contiguous()
        kinds = (_lib.AECF_BF16, _MLLOSS_LABEL_KINDS[targets.dtype])
        opts = (float(gamma_pos), float(gamma_neg), float(margin), float(eps), _MLLOSS_REDUCTIONS[reduction])
        world = dp.world_info(group)[1]
        stats = torch.empty(2, C, dtype=torch.float64, device=dev)
        totals = torch.empty(6, dtype=torch.float32, device=dev)     # the 24-byte record: float64 sum, float64 N, float32 loss, 0
        dw_u = torch.empty(C, K, dtype=torch.float32, device=dev) if want_params else None
        db_u = torch.empty(C, dtype=torch.float32, device=dev) if want_params else None
        if rows == 0:                       # an empty shard: nothing to launch, its stats and gradient sums are zeros
            stats.zero_()
            totals.zero_()
            if want_params:
                dw_u.zero_()
                db_u.zero_()
        else:
            ws_bytes = lib.aecf_mlhead_workspace_bytes(rows, C, K)
            if ws_bytes == 0:
                raise NotImplementedError(f"aecf_amd: linear_multilabel_loss does not serve {rows} x {C} x {K}; {_MLHEAD_ALTERNATIVE}")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.aecf_mlhead_forward(rows, C, K, *kinds, _ptr(h), _ptr(w), _ptr(b), _ptr(y), _ptr(pos_scale),
                                               _ptr(neg_scale), *opts, 1 if want_params else 0, _ptr(stats), _ptr(totals),
                                               _ptr(dw_u), _ptr(db_u), _ptr(ws), ws_bytes, _stream()), "aecf_mlhead_forward")
        if world > 1:
            torch.distributed.all_reduce(stats, group=group)
            total, count = stats[0].sum(), stats[1].sum()
            if reduction == "mean":
                value = torch.where(count > 0, total / torch.where(count > 0, count, torch.ones_like(count)), torch.zeros_like(total))
            else:
                value = total
            totals = torch.stack((total, count, torch.zeros_like(total)))
            loss = value.to(torch.float32)
        else:
            loss = totals[4]
        ctx.save_for_backward(h, w, b, y, pos_scale, neg_scale, totals, dw_u, db_u)
        ctx.meta = (rows, C, K, kinds, opts, float(world), weight.dtype, None if bias is None else bias.dtype)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss, _d_stats):
        lib = _lib.load()
        h, w, b, y, pos_scale, neg_scale, totals, dw_u, db_u = ctx.saved_tensors
        rows, C, K, kinds, opts, factor, w_dtype, b_dtype = ctx.meta
        want_h, want_w, want_b = ctx.needs_input_grad[:3]
        if (want_w or want_b) and dw_u is None:
            raise RuntimeError("aecf_amd: linear_multilabel_loss was run without the parameter gradients (grad mode was off)")
        dev = h.device
        dh = torch.empty_like(h) if want_h else None
        dw = torch.empty(C, K, dtype=torch.float32, device=dev) if want_w else None
        db = torch.empty(C, dtype=torch.float32, device=dev) if want_b else None
        if rows > 0 or want_w or want_b:
            up = d_loss if d_loss.dtype == torch.float32 else d_loss.to(torch.float32)       # one element, read on the device
            run_h = want_h and rows > 0
            ws, ws_bytes = None, 0
            if run_h:
                ws_bytes = lib.aecf_mlhead_workspace_bytes(rows, C, K)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.aecf_mlhead_backward(max(rows, 1), C, K, *kinds, _ptr(h), _ptr(w), _ptr(b), _ptr(y), _ptr(pos_scale),
                                                _ptr(neg_scale), *opts, _ptr(totals), _ptr(up), factor, _ptr(dw_u), _ptr(db_u),
                                                _lib.AECF_BF16, _ptr(dh) if run_h else None, _ptr(dw), _ptr(db), _ptr(ws),
                                                ws_bytes, _stream()), "aecf_mlhead_backward")
        if dw is not None and dw.dtype != w_dtype:
            dw = dw.to(w_dtype)
        if db is not None and db.dtype != b_dtype:
            db = db.to(b_dtype)
        return dh, dw, db, None, None, None, None, None, None, None, None, None, None


def linear_multilabel_loss(hidden: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], targets: torch.Tensor, *,
                           pos_weight=None, class_weight=None, alpha: Optional[float] = None, gamma_pos: float = 0.0,
                           gamma_neg: float = 0.0, margin: float = 0.0, label_smoothing: float = 0.0, reduction: str = "mean",
                           group=None, return_per_class: bool = False, _fold=_fold_scales):
    """``multilabel_loss(F.linear(hidden, weight, bias), targets, ...)`` and its gradients with respect to ``hidden`` [n, K],
    ``weight`` [C, K] (``nn.Linear``'s layout) and ``bias`` [C] or None, with nothing of size n x C ever allocated: the logits
    z = hidden @ weight.T + bias live in registers, one streaming pass over the rows in the forward (which also forms dW and
    dbias when grad mode is on and ``weight`` or ``bias`` requires grad) and one over the classes in the backward (only when
    ``hidden`` requires grad -- a linear probe on frozen features is ONE pass per step).

    Options, the folding of the weights, the rule for UNKNOWN targets, the reductions and the return values are those of
    ``multilabel_loss``.  Arithmetic: z is the float32 accumulation of the bf16 products plus the bias in one float32 add, never
    rounded to bfloat16 (``F.linear`` in bfloat16 would round it); the element is ``multilabel_loss``'s; dl/dz enters the two
    gradient products rounded once to bfloat16, dbias sums it unrounded; ``weight.grad`` and ``bias.grad`` are float32 sums cast
    once to the parameter's dtype.  No atomics: the same bits on every run.  Nothing is read on the host on one rank, so forward
    + backward capture into a graph.  Data parallel (``group``): ``multilabel_loss``'s contract -- ONE all-reduce of the float64
    [2, C] stats, the value is the global loss on every rank, all three gradients carry ``world / N`` for the averaging
    collectives of ``dp``; shards may be uneven, empty or fully unknown.

    Non-finite features are the caller's problem, as in any GEMM: a NaN row of ``hidden`` reaches ``weight.grad`` even when all
    its targets are unknown, because the product forms 0 x NaN.

    Served: bfloat16 ``hidden`` and ``weight`` on a ROCm device, K in {128, 256, 384, 512, 768, 1024}, C <= 65536, n < 2**31;
    everything else raises NotImplementedError naming the limit -- there ``F.linear`` + ``multilabel_loss`` is the way."""
    _require_device(hidden, "hidden")
    _require_device(weight, "weight")
    _require_device(targets, "targets")
    if hidden.dim() != 2 or weight.dim() != 2 or hidden.shape[1] != weight.shape[1]:
        raise ValueError(f"linear_multilabel_loss expects hidden [n, K] and weight [C, K], got {tuple(hidden.shape)} and "
                         f"{tuple(weight.shape)}")
    rows, K = hidden.shape
    C = weight.shape[0]
    if targets.dim() != 2 or tuple(targets.shape) != (rows, C):
        raise ValueError(f"linear_multilabel_loss expects targets [n, C] = [{rows}, {C}], got {tuple(targets.shape)}")
    if bias is not None:
        _require_device(bias, "bias")
        if bias.dim() != 1 or bias.shape[0] != C or not bias.dtype.is_floating_point:
            raise ValueError(f"linear_multilabel_loss expects a floating-point bias [C] = [{C}], got {tuple(bias.shape)} {bias.dtype}")
    for name, t in (("weight", weight), ("targets", targets), ("bias", bias)):
        if t is not None and t.device != hidden.device:
            raise ValueError(f"aecf_amd: the {name} lives on {t.device}, the hidden features on {hidden.device}")
    if hidden.dtype != torch.bfloat16 or weight.dtype != torch.bfloat16:
        raise NotImplementedError(f"aecf_amd: linear_multilabel_loss serves bfloat16 hidden and weight only, got {hidden.dtype} and "
                                  f"{weight.dtype}; {_MLHEAD_ALTERNATIVE}")
    if targets.dtype not in _MLLOSS_LABEL_KINDS:
        raise TypeError(f"aecf_amd: linear_multilabel_loss takes float32, bfloat16, float16, bool, uint8 or int8 targets, got {targets.dtype}")
    if reduction not in _MLLOSS_REDUCTIONS:
        raise ValueError(f"aecf_amd: linear_multilabel_loss reduces by 'mean' or 'sum' (there is no 'none'), got {reduction!r}")
    gamma_pos, gamma_neg = _gamma(gamma_pos, "gamma_pos"), _gamma(gamma_neg, "gamma_neg")
    margin = _unit_interval(margin, "margin")
    eps = _unit_interval(label_smoothing, "label_smoothing")
    if alpha is not None:
        alpha = _unit_interval(alpha, "alpha", closed_top=True)
    if C < 1:
        raise ValueError("aecf_amd: linear_multilabel_loss needs at least one class")
    if K not in MLHEAD_WIDTHS:
        raise NotImplementedError(f"aecf_amd: linear_multilabel_loss serves K in {MLHEAD_WIDTHS}, got K = {K}; {_MLHEAD_ALTERNATIVE}")
    if C > MLHEAD_MAX_CLASSES or rows >= 1 << 31:
        raise NotImplementedError(f"aecf_amd: linear_multilabel_loss serves C <= {MLHEAD_MAX_CLASSES} and n < 2**31, got {rows} x {C}; "
                                  f"{_MLHEAD_ALTERNATIVE}")
    a, b = _fold(pos_weight, class_weight, alpha, C, hidden.device)
    want_params = torch.is_grad_enabled() and (weight.requires_grad or (bias is not None and bias.requires_grad))
    loss, stats = _LinearMultilabelLoss.apply(hidden, weight, bias, targets, a, b, gamma_pos, gamma_neg, margin, eps, reduction, group,
                                              want_params)
    if not return_per_class:
        return loss
    count = stats[1]
    per_class = torch.where(count > 0, stats[0] / torch.where(count > 0, count, torch.ones_like(count)), torch.zeros_like(count))
    return loss, per_class.to(torch.float32)


class MultilabelHead(torch.nn.Module):
    """A linear classifier head with its multi-label loss fused in: ``weight`` [num_classes, in_features] and ``bias`` are
    initialised as ``nn.Linear`` initialises them and carry its state_dict keys, so the head and an ``nn.Linear`` load each
    other's state.  ``forward(hidden)`` returns the logits (``F.linear``, for evaluation); ``loss(hidden, targets)`` is
    ``linear_multilabel_loss`` with the options given here -- no logits exist.  ``from_linear(linear, **options)`` SHARES the
    layer's parameter objects.  ``pos_weight`` / ``class_weight`` are float32 buffers outside the state_dict, and the module
    owns its folded scale vectors as ``MultilabelLoss`` does, so the addresses a captured graph holds stay valid."""

    def __init__(self, in_features: int, num_classes: int, bias: bool = True, *, pos_weight=None, class_weight=None,
                 alpha: Optional[float] = None, gamma_pos: float = 0.0, gamma_neg: float = 0.0, margin: float = 0.0,
                 label_smoothing: float = 0.0, reduction: str = "mean", group=None, device=None, dtype=None, _linear=None):
        super().__init__()
        if reduction not in _MLLOSS_REDUCTIONS:
            raise ValueError(f"aecf_amd: linear_multilabel_loss reduces by 'mean' or 'sum' (there is no 'none'), got {reduction!r}")
        self.gamma_pos, self.gamma_neg = _gamma(gamma_pos, "gamma_pos"), _gamma(gamma_neg, "gamma_neg")
        self.margin = _unit_interval(margin, "margin")
        self.label_smoothing = _unit_interval(label_smoothing, "label_smoothing")
        self.alpha = None if alpha is None else _unit_interval(alpha, "alpha", closed_top=True)
        self.reduction, self.group = reduction, group
        linear = _linear if _linear is not None else torch.nn.Linear(in_features, num_classes, bias=bias, device=device, dtype=dtype)
        self.in_features, self.num_classes = linear.in_features, linear.out_features
        self.weight = linear.weight
        self.bias = linear.bias
        for name, value in (("pos_weight", pos_weight), ("class_weight", class_weight)):
            if value is not None and not isinstance(value, torch.Tensor):
                value = _class_vector(value, name, len(value), "cpu")
            self.register_buffer(name, None if value is None else value.detach().to(torch.float32).clone(), persistent=False)
        self._folds = {}                    # (buffers' identity and version, C, device) -> (pos_scale, neg_scale), never dropped

    _fold = MultilabelLoss._fold

    @classmethod
    def from_linear(cls, linear: torch.nn.Linear, **options) -> "MultilabelHead":
        if not isinstance(linear, torch.nn.Linear):
            raise TypeError(f"aecf_amd: MultilabelHead.from_linear takes an nn.Linear, got {type(linear).__name__}")
        return cls(linear.in_features, linear.out_features, linear.bias is not None, _linear=linear, **options)

    def forward(self, hidden: torch.Tensor) -> torch.Tensor:
        return torch.nn.functional.linear(hidden, self.weight, self.bias)

    def loss(self, hidden: torch.Tensor, targets: torch.Tensor, return_per_class: bool = False):
        return linear_multilabel_loss(hidden, self.weight, self.bias, targets, pos_weight=self.pos_weight,
                                      class_weight=self.class_weight, alpha=self.alpha, gamma_pos=self.gamma_pos,
                                      gamma_neg=self.gamma_neg, margin=self.margin, label_smoothing=self.label_smoothing,
                                      reduction=self.reduction, group=self.group, return_per_class=return_per_class, _fold=self._fold)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, num_classes={self.num_classes}, bias={self.bias is not None}, "
                f"gamma_pos={self.gamma_pos}, gamma_neg={self.gamma_neg}, margin={self.margin}, alpha={self.alpha}, "
                f"label_smoothing={self.label_smoothing}, reduction={self.reduction!r}")
