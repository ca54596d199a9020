"""Timing of the multi-label evaluation (aecf_amd.metrics.multilabel_metrics: per-class tie-exact AP, AUROC, F1 and their macro
values, nothing read on the host) against the route the trainer had before it: train_xray.mean_average_precision on the
same tensors -- a torch argsort / gather / cumsum that gives mAP only, breaks ties by position and ends in a host read.

A sample is the host-clock time of REPS calls that ends in a device synchronise (the torch route synchronises by itself in every
call); the two routes are sampled in turn in ONE process and the median, minimum and maximum over SAMPLES samples are printed,
with the peak device memory of one call of each above what the inputs hold.

    python tools/metrics_time.py [--sizes 2048x15,25600x15,40960x80,65536x80] [--out profiles/metrics_time.txt]

Kernel split (a run of its own; tracing slows the host, so its times are not the ones above):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/metrics_time.py --samples 1 --reps 3 --sizes 65536x80
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aecf_amd import metrics, train_xray  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048x15,25600x15,40960x80,65536x80,40960x80@0.05",
                    help="comma-separated N x C, optionally @density of the positives (default 0.2)")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    lines = [f"sample = {args.reps} calls ending in a synchronise, median [min .. max] of {args.samples} samples, the two routes in "
             f"turn; peak = device memory of one call above the inputs"]

    def sample(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.reps        # ms per call

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2**20

    for size in args.sizes.split(","):
        shape, _, density = size.partition("@")
        n, c = (int(v) for v in shape.split("x"))
        density = float(density or 0.2)
        for dtype in args.dtypes.split(","):
            g = torch.Generator().manual_seed(7)
            labels = (torch.rand(n, c, generator=g) < density).float()
            logits = (torch.randn(n, c, generator=g) + 1.5 * labels - 1.0).to(getattr(torch, dtype)).to(dev)
            labels = labels.to(dev)
            out = {}

            def new():
                out["new"] = metrics.multilabel_metrics(logits, labels)

            def old():                                              # what train_xray.evaluate hands over: float32 logits
                out["old"] = train_xray.mean_average_precision(logits.float(), labels)

            runs = [("multilabel_metrics (AP, AUROC, F1 per class + macro)", new), ("mean_average_precision (mAP, torch sort)", old)]
            for _, fn in runs:                                      # warm-up: code objects, allocator pools
                for _ in range(2):
                    sample(fn)
            times = [[] for _ in runs]
            for _ in range(args.samples):
                for i, (_, fn) in enumerate(runs):
                    times[i].append(sample(fn))
            peaks = [peak(fn) for _, fn in runs]
            ties = 1.0 - sum(len(torch.unique(logits[:, k])) for k in range(min(c, 4))) / (min(c, 4) * n)
            lines.append(f"{n} x {c} {dtype}, density {density}, {ties:.0%} of the scores of a class repeat another; "
                         f"mAP {float(out['new']['map']):.6f} tie-exact, {out['old']:.6f} by position")
            meds = []
            for (label, _), ts, pk in zip(runs, times, peaks):
                meds.append(statistics.median(ts))
                lines.append(f"  {label:<54} {meds[-1]:9.3f} ms [{min(ts):9.3f} .. {max(ts):9.3f}]  peak {pk:8.1f} MiB")
            lines.append(f"  multilabel_metrics / mean_average_precision = {meds[0] / meds[1]:.3f}")
            for ln in lines[-4:]:
                print(ln, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
