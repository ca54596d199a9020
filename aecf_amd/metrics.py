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
from typing import Optional

import torch

from . import _lib, dp
from .layer import _POOL_DTYPES, _ptr, _require_device, _stream
from .losses import _all_rows, _row_ranges

__all__ = ["multilabel_metrics"]         # (pinned by tests/test_metrics_cpu.py; multilabel_calibration and fit_calibration, below,
#                                          are public all the same)


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


# ---------------------------------------------------------------------------------------------------------------------------
# Calibration: reliability bins (ECE / MCE), Brier score and NLL under a per-class scale and bias, and the fit of that scaling
# (aecf_mlcal_stats / _fit_sums / _fit_update, include/aecf_hip.h "multi-label calibration").  The reference names calibration
# as the property its fusion layer keeps when modalities are missing; this is what measures it.
# ---------------------------------------------------------------------------------------------------------------------------

_CAL_MODES = {"temperature": _lib.AECF_MLCAL_TEMPERATURE, "class_temperature": _lib.AECF_MLCAL_CLASS_TEMPERATURE,
              "platt": _lib.AECF_MLCAL_PLATT}
_CAL_FIT_ROWS = 9           # L | g1 | g0 | h11 | h01 | h00 | n_used | used positives | n_skipped
_CAL_STATE_ROWS = 12        # accepted scale | bias | L | lambda | g1 | g0 | h11 | h01 | h00 | phase | first L | accepted steps


def calibration_edges(n_bins: int):
    """The ``n_bins - 1`` inner edges of equal-width probability bins in logit space, ``float32(log(j / (n_bins - j)))`` with
    the logarithm in float64, as the ctypes array the library takes (None for one bin)."""
    import ctypes
    if n_bins == 1:
        return None
    return (ctypes.c_float * (n_bins - 1))(*[math.log(j / (n_bins - j)) for j in range(1, n_bins)])


def _check_pair(logits: torch.Tensor, labels: torch.Tensor, what: str) -> None:
    from .losses import _MLLOSS_LABEL_KINDS
    _require_device(logits, "logits")
    _require_device(labels, "labels")
    if logits.dim() != 2 or labels.shape != logits.shape:
        raise ValueError(f"{what} expects logits and labels of one shape [n, C], got {tuple(logits.shape)} and "
                         f"{tuple(labels.shape)}")
    if logits.dtype not in _POOL_DTYPES:
        raise TypeError(f"aecf_amd: {what} takes float32, bfloat16 or float16 logits (nothing is rounded on the way in), got "
                        f"{logits.dtype}")
    if labels.dtype not in _MLLOSS_LABEL_KINDS:
        raise TypeError(f"aecf_amd: {what} takes float32, bfloat16, float16, bool, uint8 or int8 labels, got {labels.dtype}")
    if labels.device != logits.device:
        raise ValueError(f"aecf_amd: the labels live on {labels.device}, the logits on {logits.device}")
    if logits.shape[1] < 1:
        raise ValueError(f"aecf_amd: {what} needs at least one class")


def _cal_inputs(logits: torch.Tensor, labels: torch.Tensor):
    from .losses import _MLLOSS_LABEL_KINDS
    x, y = logits.detach(), labels.detach()
    if not x.is_contiguous():
        x = x.contiguous()
    if not y.is_contiguous():
        y = y.contiguous()
    kinds = (_POOL_DTYPES[x.dtype], _MLLOSS_LABEL_KINDS[labels.dtype])
    if y.dtype == torch.bool:
        y = y.view(torch.uint8)
    return x, y, kinds


def _class_param(value, name: str, C: int, device) -> Optional[torch.Tensor]:
    """``scale`` / ``bias`` as a float32 [C] device tensor: None stays None, a number fills, a tensor is taken as it is"""
    if value is None:
        return None
    if isinstance(value, torch.Tensor):
        if value.dim() != 1 or value.shape[0] != C:
            raise ValueError(f"aecf_amd: {name} must hold one value per class, [{C}], got shape {tuple(value.shape)}")
        if not value.dtype.is_floating_point:
            raise TypeError(f"aecf_amd: a tensor {name} must be floating point, got {value.dtype}")
        return value.detach().to(device=device, dtype=torch.float32).contiguous()
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise TypeError(f"aecf_amd: {name} must be None, a Python number or a [C] tensor, got {type(value).__name__}")
    return torch.full((C,), float(value), dtype=torch.float32, device=device)


def multilabel_calibration(logits: torch.Tensor, labels: torch.Tensor, n_bins: int = 15, scale=None, bias=None, group=None) -> dict:
    """Calibration of ``sigmoid(logits * scale + bias)`` [n, C] (float32, bfloat16 or float16 logits on a ROCm device, read as
    stored) against ``labels`` [n, C] (``multilabel_loss``'s kinds and rule for unknown targets: a floating-point NaN or value
    < 0, a negative int8), global over the rows of every rank of ``group``.  ``scale`` / ``bias``: None, a number, or a float32
    [C] device tensor (what ``fit_calibration`` returns).  The bins are ``n_bins`` (1 .. 32) equal-width probability bins, taken
    in logit space: an element falls into bin ``#{j : z > float32(log(j / (n_bins - j)))}``, an element on an edge into the lower
    bin -- sklearn's ``calibration_curve(strategy="uniform")`` without the rounding of a float32 sigmoid.  A NaN logit on a known
    target is an invalid entry: counted in ``n_invalid``, in nothing else.

    Returns a dict of device tensors, the same on every rank:

    ``ece``, ``mce``, ``brier``, ``nll``            0-dim float64, POOLED: every valid (row, class) element as one binary problem;
                                                    ece = sum_k |conf_k - pos_k| / N, mce = max over the non-empty bins of
                                                    |conf_k - pos_k| / count_k.  NaN without a valid element.
    ``ece_per_class`` .. ``nll_per_class``          float64 [C], the same per class; NaN for a class without a valid entry.
    ``macro_ece``, ``macro_brier``, ``macro_nll``   means over the classes with a valid entry (NaN if there is none).
    ``bin_count``, ``bin_pos``, ``bin_conf``        [C, n_bins]: the reliability diagram (int64, int64, float64 sums of p).
    ``n_valid``, ``n_pos``, ``n_invalid``           int64 [C].

    One pass of the library over this rank's OWN rows (nothing is gathered), ONE all-reduce of the float64 [3 n_bins + 5, C]
    block, float64 torch to close.  Shards may be uneven, empty or fully unknown.  One rank reads nothing on the host: the call
    captures into a graph.  Unserved shapes raise NotImplementedError."""
    _check_pair(logits, labels, "multilabel_calibration")
    if isinstance(n_bins, bool) or not isinstance(n_bins, int) or not 1 <= n_bins <= _lib.AECF_MLCAL_MAX_BINS:
        raise ValueError(f"aecf_amd: multilabel_calibration needs n_bins in 1 .. {_lib.AECF_MLCAL_MAX_BINS}, got {n_bins!r}")
    rows, C = logits.shape
    dev = logits.device
    lib = _lib.load()
    with torch.no_grad():
        sc, bi = _class_param(scale, "scale", C, dev), _class_param(bias, "bias", C, dev)
        x, y, kinds = _cal_inputs(logits, labels)
        stats = torch.empty(3 * n_bins + 5, C, dtype=torch.float64, device=dev)
        if rows == 0:                       # an empty shard: nothing to launch, its block is zeros
            stats.zero_()
        else:
            ws_bytes = lib.aecf_mlcal_workspace_bytes(rows, C, n_bins)
            if ws_bytes == 0:
                raise NotImplementedError(f"aecf_amd: multilabel_calibration serves C <= 4096 and n * C <= 2**30 per rank, got "
                                          f"{rows} x {C}")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.aecf_mlcal_stats(rows, C, *kinds, _ptr(x), _ptr(y), _ptr(sc), _ptr(bi), n_bins, calibration_edges(n_bins),
                                            _ptr(stats), _ptr(ws), ws_bytes, _stream()), "aecf_mlcal_stats")
        if dp.world_info(group)[1] > 1:
            torch.distributed.all_reduce(stats, group=group)
        return _close_calibration(stats, n_bins)


def _close_calibration(stats: torch.Tensor, B: int) -> dict:
    """The closing values from the summed block [3 B + 5, C]: float64, selects in place of divisions by zero, no host read"""
    f64 = torch.float64
    dev = stats.device
    cnt, pos, conf = stats[0:B], stats[B:2 * B], stats[2 * B:3 * B]
    brier, nll, n_invalid, n_valid, n_pos = (stats[3 * B + k] for k in range(5))
    zero, one = torch.zeros((), dtype=f64, device=dev), torch.ones((), dtype=f64, device=dev)
    nan = torch.full((), float("nan"), dtype=f64, device=dev)

    def close(cnt, pos, conf, brier, nll, n):
        has = n > 0
        n1 = torch.where(has, n, one)
        gap = (conf - pos).abs()
        filled = cnt > 0
        worst = torch.where(filled, gap / torch.where(filled, cnt, one), zero).max(0).values
        return (torch.where(has, gap.sum(0) / n1, nan), torch.where(has, worst, nan), torch.where(has, brier / n1, nan),
                torch.where(has, nll / n1, nan))

    ece_c, mce_c, brier_c, nll_c = close(cnt, pos, conf, brier, nll, n_valid)
    ece, mce, brier_p, nll_p = close(cnt.sum(1), pos.sum(1), conf.sum(1), brier.sum(), nll.sum(), n_valid.sum())
    has = n_valid > 0
    k = has.sum()

    def macro(values):
        m = torch.where(has, values, zero).sum() / torch.where(k > 0, k, torch.ones_like(k)).to(f64)
        return torch.where(k > 0, m, nan)

    i64 = torch.int64
    return dict(ece=ece, mce=mce, brier=brier_p, nll=nll_p, ece_per_class=ece_c, mce_per_class=mce_c, brier_per_class=brier_c,
                nll_per_class=nll_c, macro_ece=macro(ece_c), macro_brier=macro(brier_c), macro_nll=macro(nll_c),
                bin_count=cnt.t().to(i64), bin_pos=pos.t().to(i64), bin_conf=conf.t().contiguous(),
                n_valid=n_valid.to(i64), n_pos=n_pos.to(i64), n_invalid=n_invalid.to(i64))


def fit_calibration(logits: torch.Tensor, labels: torch.Tensor, mode: str = "temperature", max_iter: int = 32, group=None) -> dict:
    """Fit the scaling ``z = x * scale + bias`` that minimises the NLL of ``sigmoid(z)`` against ``labels`` over the rows of
    every rank of ``group`` (temperature scaling, Guo et al. 2017).  ``mode``: ``"temperature"`` -- ONE scale for all classes
    (T = 1 / scale); ``"class_temperature"`` -- a scale per class; ``"platt"`` -- a scale and a bias per class.  The fit uses
    the valid elements with a finite logit.  It is a damped Newton iteration on the device (include/aecf_hip.h, "optimiser
    rule"): exactly ``max_iter`` rounds of (sums pass, all-reduce of the float64 [9, C] sums when there is a group, one update
    launch), no host read and no data-dependent stop, so the loop captures on one rank and every rank holds the same bits.

    Returns device tensors: ``scale``, ``bias`` float32 [C] -- the last ACCEPTED parameters, what ``multilabel_calibration``
    takes; ``temperature`` float64 [C] = 1 / scale; per problem ([1] for ``"temperature"``, else [C]) ``fitted`` (False: no used
    element, no positive or no negative -- scale 1, bias 0), ``converged`` (an accepted step at most 2**-20 max(1, |theta|)),
    ``nll_before`` and ``nll_after`` (float64 SUMS over the used elements: at scale 1, bias 0, and the smallest of the accepted
    trials -- a trial is accepted while its sum is not above that by more than 2**-14 of it, the float32 noise of two sums, so
    the returned parameters' own sum may exceed ``nll_after`` by that much); ``n_used`` and ``n_skipped`` int64 [C]
    (``n_skipped``: +-inf logits on known targets)."""
    _check_pair(logits, labels, "fit_calibration")
    if mode not in _CAL_MODES:
        raise ValueError(f"aecf_amd: fit_calibration fits 'temperature', 'class_temperature' or 'platt', got {mode!r}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 1:
        raise ValueError(f"aecf_amd: fit_calibration needs max_iter >= 1, got {max_iter!r}")
    rows, C = logits.shape
    dev = logits.device
    lib = _lib.load()
    with torch.no_grad():
        x, y, kinds = _cal_inputs(logits, labels)
        ws_bytes = 0
        if rows > 0:
            ws_bytes = lib.aecf_mlcal_workspace_bytes(rows, C, 1)
            if ws_bytes == 0:
                raise NotImplementedError(f"aecf_amd: fit_calibration serves C <= 4096 and n * C <= 2**30 per rank, got {rows} x {C}")
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        sums = torch.zeros(_CAL_FIT_ROWS, C, dtype=torch.float64, device=dev)
        state = torch.zeros(_CAL_STATE_ROWS, C, dtype=torch.float64, device=dev)
        scale_eval, scale = (torch.ones(C, dtype=torch.float32, device=dev) for _ in range(2))
        bias_eval, bias = (torch.zeros(C, dtype=torch.float32, device=dev) for _ in range(2))
        world = dp.world_info(group)[1]
        st = _stream()
        for _ in range(max_iter):
            if rows > 0:
                _lib.check(lib.aecf_mlcal_fit_sums(rows, C, *kinds, _ptr(x), _ptr(y), _ptr(scale_eval), _ptr(bias_eval), _ptr(sums),
                                                   _ptr(ws), ws_bytes, st), "aecf_mlcal_fit_sums")
            if world > 1:
                if rows == 0:
                    sums.zero_()
                torch.distributed.all_reduce(sums, group=group)
            _lib.check(lib.aecf_mlcal_fit_update(C, _CAL_MODES[mode], _ptr(sums), _ptr(state), _ptr(scale_eval), _ptr(bias_eval),
                                                 _ptr(scale), _ptr(bias), st), "aecf_mlcal_fit_update")
        P = 1 if mode == "temperature" else C
        phase = state[9, :P]
        return dict(scale=scale, bias=bias, temperature=1.0 / scale.to(torch.float64), fitted=phase != 3.0, converged=phase == 2.0,
                    nll_before=state[10, :P].clone(), nll_after=state[2, :P].clone(), n_used=sums[6].to(torch.int64),
                    n_skipped=sums[8].to(torch.int64))


# ---------------------------------------------------------------------------------------------------------------------------
# Bootstrap confidence intervals of AP, AUROC and F1 (aecf_mlboot_order / _draw / _walk, include/aecf_hip.h "multi-label
# bootstrap").  The reference's experiment is a comparison -- baseline against AECF, full against a missing modality -- on a
# validation set where several classes hold a handful of positives; this is what says whether a difference means anything.
# ---------------------------------------------------------------------------------------------------------------------------

_BOOT_SCORES = ("ap", "auroc", "f1", "map", "macro_auroc", "macro_f1")
_BOOT_CALL_REPLICATES = 4096        # aecf_mlboot_*: replicates of one call at most
_BOOT_CHUNK_ELEMS = 1 << 26         # rows x replicates of one draw + walk: 256 MiB of int32 scratch, 64 MiB of weights


def _boot_chunk(n_all: int) -> int:
    """replicates of one draw + walk: a multiple of 64, at least 64, at most one call's, about _BOOT_CHUNK_ELEMS / n_all"""
    return max(64, min(_BOOT_CALL_REPLICATES, _BOOT_CHUNK_ELEMS // n_all // 64 * 64))


def _boot_thresholds(threshold, C: int, device) -> torch.Tensor:
    """``threshold`` as float32 [C] logit thresholds: a probability inside (0, 1) for all classes, or a [C] tensor of logit
    thresholds taken as it is"""
    if isinstance(threshold, torch.Tensor):
        if threshold.dim() != 1 or threshold.shape[0] != C or not threshold.dtype.is_floating_point:
            raise ValueError(f"aecf_amd: a tensor threshold holds one floating-point logit threshold per class, [{C}], got "
                             f"{threshold.dtype} {tuple(threshold.shape)}")
        return threshold.detach().to(device=device, dtype=torch.float32).contiguous()
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 < threshold < 1.0:
        raise ValueError(f"aecf_amd: bootstrap_metrics needs a threshold inside (0, 1) or a [C] tensor of logit thresholds, got "
                         f"{threshold!r}")
    return torch.full((C,), math.log(threshold / (1.0 - threshold)), dtype=torch.float32, device=device)


def _boot_stats(logits, labels, n_boot, threshold, seed, weights, group, want_weights):
    """The checks, the gather and the three library passes: (stats int64 [R, 7, C] of the R = n_boot + 1 replicates, replicate 0
    all ones; n_saturated int32 [1]; the uint8 weights [R, n_all] or None).  Each rank walks a contiguous slice of the
    replicates and ONE all-reduce of the zero-filled int64 block joins the slices: an integer sum with zeros moves no bit."""
    _require_device(logits, "logits")
    _require_device(labels, "labels")
    if logits.dim() != 2 or labels.shape != logits.shape:
        raise ValueError(f"bootstrap_metrics expects logits and labels of one shape [n, C], got {tuple(logits.shape)} and "
                         f"{tuple(labels.shape)}")
    if logits.dtype not in _POOL_DTYPES:
        raise TypeError(f"aecf_amd: bootstrap_metrics takes float32, bfloat16 or float16 logits (nothing is rounded on the way in), "
                        f"got {logits.dtype}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f"aecf_amd: bootstrap_metrics needs a seed in [0, 2**64), got {seed!r}")
    rows, C = logits.shape
    if C < 1:
        raise ValueError("aecf_amd: bootstrap_metrics needs at least one class")
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.dim() != 2 or weights.shape[0] < 1:
            raise ValueError("aecf_amd: weights are a [R, n] tensor of row multiplicities over the rows of every rank")
        if weights.dtype not in (torch.uint8, torch.int16, torch.int32, torch.int64):
            raise TypeError(f"aecf_amd: weights are uint8 (or int16 / int32 / int64, clipped to 0 .. 255 and counted in n_saturated), "
                            f"got {weights.dtype}")
        _require_device(weights, "weights")
        n_boot = weights.shape[0]
    if isinstance(n_boot, bool) or not isinstance(n_boot, int) or not 1 <= n_boot < (1 << 31) - 1:
        raise ValueError(f"aecf_amd: bootstrap_metrics needs n_boot >= 1, got {n_boot!r}")
    lib = _lib.load()
    dev = logits.device
    y = _labels_u8(labels.detach())
    x = logits.detach().contiguous()
    thr = _boot_thresholds(threshold, C, dev)
    sizes, _, n_all = _row_ranges(rows, dev, group)
    if n_all < 1:
        raise ValueError("aecf_amd: bootstrap_metrics needs at least one row")
    if weights is not None and weights.shape[1] != n_all:
        raise ValueError(f"aecf_amd: weights hold one multiplicity per row of every rank, [R, {n_all}], got {tuple(weights.shape)}")
    ws_bytes = lib.aecf_mlboot_workspace_bytes(n_all, C)
    if ws_bytes == 0:
        raise NotImplementedError(f"aecf_amd: bootstrap_metrics serves C <= 4096, n <= 2**24 and n * C <= 2**28 over all ranks, got "
                                  f"{n_all} x {C}")
    x_all = _all_rows(x, group, sizes).contiguous()
    y_all = _all_rows(y, group, sizes).contiguous()
    R = n_boot + 1
    rank, world = dp.world_info(group)
    lo, hi = dp.shard_bounds(R, rank, world)
    Np = (n_all + 63) // 64 * 64
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    class_counts = torch.empty(3, C, dtype=torch.int32, device=dev)
    order = torch.empty(C, Np, dtype=torch.int32, device=dev)
    n_sat = torch.zeros(1, dtype=torch.int32, device=dev)
    stats = torch.zeros(R, 7, C, dtype=torch.int64, device=dev) if world > 1 else torch.empty(R, 7, C, dtype=torch.int64, device=dev)
    kept = torch.empty(R, n_all, dtype=torch.uint8, device=dev) if want_weights else None
    st = _stream()
    _lib.check(lib.aecf_mlboot_order(n_all, C, _POOL_DTYPES[x_all.dtype], _ptr(x_all), _ptr(y_all), _ptr(thr), _ptr(class_counts),
                                     _ptr(order), _ptr(ws), ws_bytes, st), "aecf_mlboot_order")
    chunk = _boot_chunk(n_all)
    for r0 in range(lo, hi, chunk):
        reps = min(chunk, hi - r0)
        Rp = (reps + 63) // 64 * 64
        w = torch.empty(n_all, Rp, dtype=torch.uint8, device=dev)
        if weights is None:
            dws_bytes = lib.aecf_mlboot_draw_workspace_bytes(n_all, reps)
            dws = torch.empty(dws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.aecf_mlboot_draw(n_all, reps, r0, seed, None, _ptr(w), _ptr(n_sat), _ptr(dws), dws_bytes, st),
                       "aecf_mlboot_draw")
        else:                                   # replicate 0 stays the point estimate: ones, then the caller's rows
            counts = torch.zeros(n_all, Rp, dtype=torch.int32, device=dev)
            a = max(r0, 1)
            if r0 == 0:
                counts[:, 0] = 1
            counts[:, a - r0:reps] = weights[a - 1:r0 + reps - 1].t()
            _lib.check(lib.aecf_mlboot_draw(n_all, reps, r0, seed, _ptr(counts), _ptr(w), _ptr(n_sat), None, 0, st),
                       "aecf_mlboot_draw")
        _lib.check(lib.aecf_mlboot_walk(n_all, C, reps, _ptr(class_counts), _ptr(order), _ptr(w), _ptr(stats[r0:r0 + reps]), st),
                   "aecf_mlboot_walk")
        if kept is not None:
            kept[r0:r0 + reps] = w[:, :reps].t()
    if world > 1:
        torch.distributed.all_reduce(stats, group=group)
        torch.distributed.all_reduce(n_sat, group=group)
        if kept is not None:
            kept[:lo].zero_()
            kept[hi:].zero_()
            torch.distributed.all_reduce(kept, group=group)
    return stats, n_sat, kept


def _close_replicates(stats: torch.Tensor) -> dict:
    """``_close``'s rules for every replicate at once, from stats int64 [R, 7, C] = Wpos | Wvalid | U2 | TP | FP | FN | S bits:
    ap / auroc / f1 float64 [R, C] and map / macro_auroc / macro_f1 [R].  AP 0 without positive weight; AUROC NaN without positive
    or without negative weight; F1 0 without a true positive; mAP over the classes with positive weight IN THAT REPLICATE;
    macro AUROC over the defined ones; macro F1 over F1 > 0.  float64, selects in place of divisions by zero, no host read.
    (The integers convert exactly below 2**53: U2 and 2 Wpos Wneg pass it only beyond about 6e7 weighted pairs.)"""
    f64 = torch.float64
    dev = stats.device
    wpos, wvalid, u2, tp, fp, fn = (stats[:, k].to(f64) for k in range(6))
    s = stats[:, 6].contiguous().view(f64)
    wneg = wvalid - wpos
    zero, one = torch.zeros((), dtype=f64, device=dev), torch.ones((), dtype=f64, device=dev)
    nan = torch.full((), float("nan"), dtype=f64, device=dev)
    has_pos = wpos > 0
    both = has_pos & (wneg > 0)
    ap = torch.where(has_pos, s / torch.where(has_pos, wpos, one), zero)
    auroc = torch.where(both, u2 / torch.where(both, 2.0 * wpos * wneg, one), nan)
    scored = has_pos & (tp > 0)
    f1 = torch.where(scored, 2.0 * tp / torch.where(scored, 2.0 * tp + fp + fn, one), zero)

    def mean_over(values, keep, empty):
        k = keep.sum(1)
        m = torch.where(keep, values, zero).sum(1) / torch.where(k > 0, k, torch.ones_like(k)).to(f64)
        return torch.where(k > 0, m, torch.full((), empty, dtype=f64, device=dev))

    return dict(ap=ap, auroc=auroc, f1=f1, map=mean_over(ap, has_pos, 0.0), macro_auroc=mean_over(auroc, both, float("nan")),
                macro_f1=mean_over(f1, f1 > 0, 0.0))


def _boot_summary(values: torch.Tensor, confidence: float) -> dict:
    """point | ci | se | n_defined of replicate values [R, ...] (replicate 0: the point estimate).  Percentile interval over the
    replicates 1 .. R - 1 that are not NaN, ``torch.nanquantile(..., interpolation="linear")`` in float64; the standard error is
    their standard deviation (n - 1 in the divisor; NaN below two defined replicates)."""
    reps = values[1:]
    alpha = (1.0 - confidence) / 2.0
    ci = torch.stack([torch.nanquantile(reps, q, dim=0, interpolation="linear") for q in (alpha, 1.0 - alpha)])
    defined = ~torch.isnan(reps)
    n = defined.sum(0)
    nf = n.to(torch.float64)
    filled = torch.where(defined, reps, torch.zeros((), dtype=reps.dtype, device=reps.device))
    mean = filled.sum(0) / torch.clamp(nf, min=1.0)
    dev2 = torch.where(defined, (reps - mean) ** 2, torch.zeros((), dtype=reps.dtype, device=reps.device)).sum(0)
    se = torch.where(n > 1, (dev2 / torch.clamp(nf - 1.0, min=1.0)).sqrt(), torch.full((), float("nan"), dtype=reps.dtype, device=reps.device))
    return dict(point=values[0], ci=ci, se=se, n_defined=n)


def _check_confidence(confidence) -> None:
    if isinstance(confidence, bool) or not isinstance(confidence, (int, float)) or not 0.0 < confidence < 1.0:
        raise ValueError(f"aecf_amd: a confidence level lies inside (0, 1), got {confidence!r}")


def bootstrap_metrics(logits: torch.Tensor, labels: torch.Tensor, n_boot: int = 1000, confidence: float = 0.95, threshold=0.5,
                      seed: int = 0, weights: Optional[torch.Tensor] = None, group=None, return_replicates: bool = False,
                      return_weights: bool = False) -> dict:
    """``multilabel_metrics`` with percentile-bootstrap confidence intervals: ``n_boot`` resamples of the ROWS (a row carries all
    its classes, so the macro scores see the joint resample) of ``logits`` / ``labels`` [n, C] (``multilabel_metrics``' dtypes
    and label kinds), global over the rows of every rank of ``group``.  ``threshold``: a probability inside (0, 1), or a float
    [C] tensor of LOGIT thresholds, one per class.  Replicate r >= 1 is the classical multinomial bootstrap -- n draws with
    replacement, from Philox keyed by ``seed`` -- and depends on (seed, r, n) only; ``weights``, uint8 [R, n] row multiplicities
    (or a wider integer type, clipped to 0 .. 255 and counted in ``n_saturated``), replace the draw, and ``n_boot`` is then R.

    The classes are ranked once, by counting, and that one order is walked once for all replicates with one lane per replicate
    (include/aecf_hip.h, "multi-label bootstrap").  Up to the final quotients the arithmetic is integer: a replicate's scores are
    those of ``multilabel_metrics`` on the rows physically repeated by their multiplicities (AP to the rounding of its float64
    sum), whatever the tiles, blocks or ranks.

    Returns a dict of device tensors, the same on every rank.  For each of ``ap``, ``auroc``, ``f1`` (float64 [C]) and ``map``,
    ``macro_auroc``, ``macro_f1`` (0-dim): the point value under its name (replicate 0, all weights one: ``multilabel_metrics``'
    value), ``<name>_ci`` [2, ...] the lower and upper percentile limits at ``confidence`` over the replicates that are not NaN,
    ``<name>_se`` their standard deviation; ``n_defined``: a dict name -> int64 count of those replicates (an AUROC is NaN in a
    replicate that drew no positive or no negative of the class; per replicate mAP runs over the classes with a drawn
    positive, macro F1 over F1 > 0, ``_close``'s rules); ``n_saturated`` int64 0-dim.  ``return_replicates``: ``replicates``, a
    dict name -> float64 [n_boot + 1, C] / [n_boot + 1] with replicate 0 first; ``return_weights``: ``weights`` uint8
    [n_boot + 1, n], row 0 all ones.

    One rank reads nothing on the host: the call captures into a graph and a replay follows logits and labels changed in place.
    Data parallel: the rows are gathered as ``multilabel_metrics`` gathers them, every rank walks a contiguous slice of the
    replicates, and one all-reduce joins the int64 [n_boot + 1, 7, C] block -- the bits of the one-rank call.  More than about
    2**26 / n replicates are processed in chunks inside the call."""
    _check_confidence(confidence)
    with torch.no_grad():
        stats, n_sat, kept = _boot_stats(logits, labels, n_boot, threshold, seed, weights, group, return_weights)
        reps = _close_replicates(stats)
        out = dict(n_defined={}, n_saturated=n_sat[0].to(torch.int64))
        for name in _BOOT_SCORES:
            s = _boot_summary(reps[name], confidence)
            out[name], out[name + "_ci"], out[name + "_se"] = s["point"], s["ci"], s["se"]
            out["n_defined"][name] = s["n_defined"]
        if return_replicates:
            out["replicates"] = reps
        if return_weights:
            out["weights"] = kept
        return out


def bootstrap_compare(logits_a: torch.Tensor, logits_b: torch.Tensor, labels: torch.Tensor, n_boot: int = 1000,
                      confidence: float = 0.95, threshold=0.5, seed: int = 0, weights: Optional[torch.Tensor] = None, group=None,
                      return_replicates: bool = False) -> dict:
    """The PAIRED bootstrap of two models on the same rows: both are walked under the SAME resamples (the same ``seed``, or the
    same ``weights``), and every score's difference a - b is formed per replicate -- the reference's baseline-against-AECF and
    full-against-missing-modality question.  For each of ``ap``, ``auroc``, ``f1``, ``map``, ``macro_auroc``, ``macro_f1``:
    ``<name>`` the point difference, ``<name>_ci`` [2, ...] its percentile interval, ``<name>_se``, and ``<name>_p_le0`` /
    ``<name>_p_ge0``: the fractions of the defined replicates (neither side NaN) with a difference <= 0 and >= 0 (NaN without a
    defined replicate); ``n_defined`` as in ``bootstrap_metrics``; ``a`` and ``b``: the two ``bootstrap_metrics`` results."""
    _check_confidence(confidence)
    with torch.no_grad():
        kw = dict(n_boot=n_boot, confidence=confidence, threshold=threshold, seed=seed, weights=weights, group=group,
                  return_replicates=True)
        a = bootstrap_metrics(logits_a, labels, **kw)
        b = bootstrap_metrics(logits_b, labels, **kw)
        out = dict(n_defined={}, a=a, b=b)
        diffs = {}
        for name in _BOOT_SCORES:
            d = a["replicates"][name] - b["replicates"][name]            # NaN where either side is
            diffs[name] = d
            s = _boot_summary(d, confidence)
            out[name], out[name + "_ci"], out[name + "_se"] = s["point"], s["ci"], s["se"]
            out["n_defined"][name] = s["n_defined"]
            n = s["n_defined"].to(torch.float64)
            nan = torch.full((), float("nan"), dtype=torch.float64, device=d.device)
            for key, hit in (("_p_le0", d[1:] <= 0), ("_p_ge0", d[1:] >= 0)):
                out[name + key] = torch.where(n > 0, hit.sum(0).to(torch.float64) / torch.clamp(n, min=1.0), nan)
        if return_replicates:
            out["replicates"] = diffs
        else:
            del a["replicates"], b["replicates"]
        return out
