"""Multi-label evaluation on the device: tie-exact average precision, AUROC and F1 per class, and the macro scores the
reference's example ranks models by (``calculate_metrics``, ref xrays/train_xrays_example.py:260-295), over the rows of every
rank of a process group.

Nothing is sorted.  For every valid (non-NaN) positive i of a class the library counts, over the class's valid entries j,
``ge_all = #{s_j >= s_i}``, ``gt_all = #{s_j > s_i}`` and the same two over the positives only (aecf_mlmetrics_prepare /
_counts / _finalize, include/aecf_hip.h "multi-label evaluation").  Then

    AP    = (1 / npos) sum_i ge_pos_i / ge_all_i                       sklearn's step-wise average precision: every sample at
                                                                       one score shares that threshold's precision
    AUROC = sum_i (lt_neg_i + eq_neg_i / 2) / (npos nneg)              the Mann-Whitney statistic with half credit for ties
    F1    = 2 TP / (2 TP + FP + FN) at logit > t                       0 where the class has no positive or no true positive

The counts are integers, so a result does not depend on tiles, blocks or how the rows are dealt over ranks beyond the rounding
of the float64 sums that close it.

Differences from the reference, on purpose: logits are ranked as given, not their float32 sigmoids (which merge distinct large
logits); "predicted positive" is ``logit > float32(log(threshold / (1 - threshold)))`` -- at 0.5 that is ``logit > 0``, which
differs from ``sigmoid_f32(x) > 0.5`` only for 0 < x below about 2**-22; labels may be bool, uint8 or floating point (positive
iff non-zero); a NaN logit is an invalid entry of its class -- in no count, reported in ``n_invalid`` -- where sklearn raises.
"""
from __future__ import annotations

import math

import torch

from . import _lib, dp
from .layer import _POOL_DTYPES, _ptr, _require_device, _stream
from .losses import _all_rows, _row_ranges

__all__ = ["multilabel_metrics"]


def _labels_u8(labels: torch.Tensor) -> torch.Tensor:
    if labels.dtype == torch.uint8:
        return labels.contiguous()
    if labels.dtype == torch.bool or labels.dtype.is_floating_point:
        return (labels != 0).to(torch.uint8).contiguous()
    raise TypeError(f"aecf_amd: multilabel_metrics takes bool, uint8 or floating-point labels, got {labels.dtype}")


def multilabel_metrics(logits: torch.Tensor, labels: torch.Tensor, threshold: float = 0.5, group=None) -> dict:
    """Per-class and macro evaluation of ``logits`` [n, C] (float32, bfloat16 or float16, on a ROCm device) against ``labels``
    [n, C] (bool, uint8 or floating point; positive iff non-zero), global over the rows of every rank of ``group``.

    Returns a dict of device tensors, the same on every rank:

    ``ap``, ``auroc``, ``f1``   float64 [C].  ``ap`` and ``f1`` are 0 for a class without a positive; ``auroc`` is NaN for a
                                class without a positive or without a negative.
    ``n_pos``, ``n_invalid``    int64 [C]: the valid positives and the NaN logits of every class.
    ``map``                     mean of ``ap`` over the classes with a positive, 0 if there is none (the reference's rule).
    ``macro_auroc``             mean of ``auroc`` over the classes with a positive and a negative (NaN if there is none).
    ``macro_f1``                mean of the per-class F1 values that are > 0, else 0 (the reference's rule).

    One rank: no host read, so the call captures into a graph.  Data parallel: the ranks exchange their row counts (the one host
    read), all-gather logits and labels -- shards may be uneven or empty -- count their own rows against all, and all-reduce
    the float64 [5, C] shares once; the closing arithmetic is float64 torch on the device."""
    _require_device(logits, "logits")
    _require_device(labels, "labels")
    if logits.dim() != 2 or labels.shape != logits.shape:
        raise ValueError(f"multilabel_metrics expects logits and labels of one shape [n, C], got {tuple(logits.shape)} and "
                         f"{tuple(labels.shape)}")
    if logits.dtype not in _POOL_DTYPES:
        raise TypeError(f"aecf_amd: multilabel_metrics takes float32, bfloat16 or float16 logits (nothing is rounded on the way "
                        f"in), got {logits.dtype}")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 < threshold < 1.0:
        raise ValueError(f"aecf_amd: multilabel_metrics needs a threshold inside (0, 1), got {threshold!r}")
    logit_threshold = math.log(threshold / (1.0 - threshold))          # rounded to float32 on the way into the library
    rows, C = logits.shape
    if C < 1:
        raise ValueError("aecf_amd: multilabel_metrics needs at least one class")
    lib = _lib.load()
    dev = logits.device
    with torch.no_grad():
        y = _labels_u8(labels.detach())
        x = logits.detach().contiguous()
        sizes, offset, n_all = _row_ranges(rows, dev, group)
        if n_all < 1:
            raise ValueError("aecf_amd: multilabel_metrics needs at least one row")
        ws_bytes = lib.aecf_mlmetrics_workspace_bytes(n_all, C)
        if ws_bytes == 0:
            raise NotImplementedError(f"aecf_amd: multilabel_metrics serves C <= 4096, n <= 2**24 and n * C <= 2**28 over all "
                                      f"ranks, got {n_all} x {C}")
        x_all = _all_rows(x, group, sizes).contiguous()
        y_all = _all_rows(y, group, sizes).contiguous()
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        class_counts = torch.empty(3, C, dtype=torch.int32, device=dev)
        counts = torch.empty(4, C, rows, dtype=torch.int32, device=dev)
        shares = torch.empty(5, C, dtype=torch.float64, device=dev)
        st = _stream()
        _lib.check(lib.aecf_mlmetrics_prepare(n_all, C, _POOL_DTYPES[x_all.dtype], _ptr(x_all), _ptr(y_all), _ptr(class_counts),
                                              _ptr(ws), ws_bytes, st), "aecf_mlmetrics_prepare")
        _lib.check(lib.aecf_mlmetrics_counts(n_all, C, offset, rows, _ptr(class_counts), _ptr(counts) if rows else None, _ptr(ws),
                                             ws_bytes, st), "aecf_mlmetrics_counts")
        _lib.check(lib.aecf_mlmetrics_finalize(n_all, C, offset, rows, logit_threshold, _ptr(class_counts),
                                               _ptr(counts) if rows else None, _ptr(shares), _ptr(ws), ws_bytes, st),
                   "aecf_mlmetrics_finalize")
        if sizes is not None:
            torch.distributed.all_reduce(shares, group=group)
        return _close(shares, class_counts)


def _close(shares: torch.Tensor, class_counts: torch.Tensor) -> dict:
    """The per-class and macro values from the summed shares [5, C] and npos | nvalid | ninvalid [3, C]: float64, selects in
    place of divisions by zero, no host read."""
    f64 = torch.float64
    n_pos, n_valid, n_invalid = (class_counts[k].to(torch.int64) for k in range(3))
    npos = n_pos.to(f64)
    nneg = (n_valid - n_pos).to(f64)
    zero, one = torch.zeros((), dtype=f64, device=shares.device), torch.ones((), dtype=f64, device=shares.device)
    has_pos = n_pos > 0
    both = has_pos & (n_valid > n_pos)
    ap = torch.where(has_pos, shares[0] / torch.where(has_pos, npos, one), zero)
    auroc = torch.where(both, shares[1] / torch.where(both, npos * nneg, one), torch.full((), float("nan"), dtype=f64, device=shares.device))
    tp, fp, fn = shares[2], shares[3], shares[4]
    den = 2.0 * tp + fp + fn
    scored = has_pos & (tp > 0)
    f1 = torch.where(scored, 2.0 * tp / torch.where(scored, den, one), zero)

    def mean_over(values, keep, empty):
        k = keep.sum()
        m = torch.where(keep, values, zero).sum() / torch.where(k > 0, k, torch.ones_like(k)).to(f64)
        return torch.where(k > 0, m, torch.full((), empty, dtype=f64, device=shares.device))

    return dict(ap=ap, auroc=auroc, f1=f1, n_pos=n_pos, n_invalid=n_invalid,
                map=mean_over(ap, has_pos, 0.0), macro_auroc=mean_over(auroc, both, float("nan")),
                macro_f1=mean_over(f1, f1 > 0, 0.0))
