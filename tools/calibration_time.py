"""Timing of the calibration statistics and the scaling fit (aecf_amd.metrics.multilabel_calibration / fit_calibration) against
their torch eager equivalents on the same tensors:

    statistics   logits.float(), sigmoid, bucketize on the logit-space edges, three scatter_add into [C * B], the Brier sum and
                 binary_cross_entropy_with_logits per class, the same closing arithmetic
    fit          the shared temperature by 32 Newton steps in torch float64 (sums of (s - y) x and s (1 - s) x^2 per step),
                 nothing read on the host

A sample is the host-clock time of REPS calls that ends in a device synchronise; the routes are sampled in turn in ONE process
and the median, minimum and maximum over SAMPLES samples are printed, with the peak device memory of one call of each above what
the inputs hold.  The statistics pass alone (aecf_mlcal_stats through the C ABI, no closing arithmetic) is timed too and set
against its byte model: every logit and every label read once.

    python tools/calibration_time.py [--sizes 2048x15:float32:float32,...] [--out profiles/calibration_time.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aecf_amd import _lib, metrics  # noqa: E402
from aecf_amd.layer import _POOL_DTYPES, _ptr, _stream  # noqa: E402
from aecf_amd.losses import _MLLOSS_LABEL_KINDS  # noqa: E402


def torch_statistics(logits, labels, B, edges):
    x = logits.float()
    y = labels.float()
    n, C = x.shape
    p = torch.sigmoid(x)
    idx = (torch.bucketize(x, edges) + B * torch.arange(C, device=x.device)).flatten()
    cnt = torch.zeros(C * B, dtype=torch.float64, device=x.device).scatter_add_(0, idx, torch.ones_like(idx, dtype=torch.float64))
    pos = torch.zeros_like(cnt).scatter_add_(0, idx, y.flatten().double())
    conf = torch.zeros_like(cnt).scatter_add_(0, idx, p.flatten().double())
    brier = ((p - y) ** 2).sum(0, dtype=torch.float64)
    nll = F.binary_cross_entropy_with_logits(x, y, reduction="none").sum(0, dtype=torch.float64)
    gap = (conf - pos).abs().view(C, B)
    return dict(ece=(conf - pos).view(C, B).sum(0).abs().sum() / (n * C), ece_per_class=gap.sum(1) / n, brier=brier.sum() / (n * C), nll=nll.sum() / (n * C),
                bin_count=cnt.view(C, B))


def torch_fit(logits, labels, iters=32):
    x = logits.double()
    y = labels.double()
    s = torch.ones((), dtype=torch.float64, device=x.device)
    for _ in range(iters):
        p = torch.sigmoid(x * s)
        g = ((p - y) * x).sum()
        h = (p * (1 - p) * x * x).sum()
        s = (s - g / h).clamp(1.0 / 64, 64.0)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048x15:float32:float32,40960x80:bfloat16:float32,65536x4096:bfloat16:uint8",
                    help="comma-separated N x C : logits dtype : labels dtype")
    ap.add_argument("--bins", type=int, default=15)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("calibration_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B = args.bins
    lines = [f"sample = REPS calls ending in a synchronise, median [min .. max] of {args.samples} samples, the routes in turn; peak = "
             f"device memory of one call above the inputs; {B} bins; fit = shared temperature, 32 iterations"]
    edges_c = metrics.calibration_edges(B)
    edges_t = torch.tensor(list(edges_c), dtype=torch.float32, device=dev)

    def sample(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps              # ms per call

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2**20

    for size in args.sizes.split(","):
        shape, dtype, ldtype = size.split(":")
        n, c = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(7)
        labels = (torch.rand(n, c, generator=g, device=dev) < 0.2)
        logits = (2.0 * torch.randn(n, c, generator=g, device=dev) + 2.0 * labels - 1.5).to(getattr(torch, dtype))
        labels = labels.to(getattr(torch, ldtype))
        out = {}
        ws_bytes = lib.aecf_mlcal_workspace_bytes(n, c, B)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        block = torch.empty(3 * B + 5, c, dtype=torch.float64, device=dev)
        kinds = (_POOL_DTYPES[logits.dtype], _MLLOSS_LABEL_KINDS[labels.dtype])

        def pass_only():
            _lib.check(lib.aecf_mlcal_stats(n, c, *kinds, _ptr(logits), _ptr(labels), None, None, B, edges_c, _ptr(block), _ptr(ws),
                                            ws_bytes, _stream()), "aecf_mlcal_stats")

        def new_stats():
            out["new"] = metrics.multilabel_calibration(logits, labels, n_bins=B)

        def old_stats():
            out["old"] = torch_statistics(logits, labels, B, edges_t)

        def new_fit():
            out["new_fit"] = metrics.fit_calibration(logits, labels, mode="temperature")

        def old_fit():
            out["old_fit"] = torch_fit(logits, labels)

        big = n * c > 1 << 26
        runs = [("aecf_mlcal_stats alone (pass + finalize)", pass_only, args.reps),
                ("multilabel_calibration (pass + closing)", new_stats, args.reps),
                ("torch eager statistics", old_stats, args.reps),
                ("fit_calibration, temperature, 32 iterations", new_fit, 1 if big else args.reps),
                ("torch float64 Newton, 32 iterations", old_fit, 1 if big else args.reps)]
        for _, fn, reps in runs:                                    # warm-up: code objects, allocator pools
            for _ in range(2):
                sample(fn, reps)
        times = [[] for _ in runs]
        for _ in range(args.samples):
            for i, (_, fn, reps) in enumerate(runs):
                times[i].append(sample(fn, reps))
        peaks = [peak(fn) for _, fn, _ in runs]
        same = bool((out["new"]["bin_count"] == out["old"]["bin_count"].long()).all())
        lines.append(f"{n} x {c} {dtype} logits, {ldtype} labels; ece {float(out['new']['ece']):.6f} library, {float(out['old']['ece']):.6f} "
                     f"torch; bin counts equal: {same}; scale {float(out['new_fit']['scale'][0]):.6f} library, {float(out['old_fit']):.6f} torch")
        meds = []
        for (label, _, _), ts, pk in zip(runs, times, peaks):
            meds.append(statistics.median(ts))
            lines.append(f"  {label:<46} {meds[-1]:10.3f} ms [{min(ts):10.3f} .. {max(ts):10.3f}]  peak {pk:9.1f} MiB")
        nbytes = n * c * (logits.element_size() + labels.element_size())
        lines.append(f"  statistics pass: {nbytes / 2**20:.1f} MiB read once -> {nbytes / (meds[0] * 1e-3) / 1e9:.1f} GB/s;  "
                     f"multilabel_calibration / torch = {meds[1] / meds[2]:.3f};  fit_calibration / torch = {meds[3] / meds[4]:.3f}")
        for ln in lines[-(len(runs) + 2):]:
            print(ln, flush=True)
        del logits, labels, ws, block, out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
