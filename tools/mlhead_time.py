"""Timing and peak memory of the fused classifier head (aecf_amd.losses.linear_multilabel_loss: forward + backward, hidden,
weight and bias all requiring gradients) against the two ways of doing the same with logits, neither of which is the code under
test:

  (a) F.linear + losses.multilabel_loss of this same build       the [n, C] logits and their gradient exist in bfloat16
  (b) torch eager: F.linear, .float(), binary_cross_entropy_with_logits (or, for the asymmetric form, an eager transcription)

A sample is the host-clock time of REPS forward + backward calls that ends in a device synchronise, after warm-up; the three
routes are sampled in turn in ONE process and the median, minimum and maximum over SAMPLES samples are printed, with the peak
device memory of one call above what the inputs hold (torch.cuda.max_memory_allocated).  The frozen-features line is the fused
call and route (a) with hidden.requires_grad == False (a linear probe: no dh).  Labels are uint8.

    python tools/mlhead_time.py [--out profiles/mlhead_time.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aecf_amd import losses  # noqa: E402

SHAPES = ((65536, 4096, 512), (65536, 4096, 1024), (65536, 80, 256), (64, 15, 256))
FORMS = {"BCE": (0.0, 0.0, 0.0), "asymmetric (0, 4, 0.05)": (0.0, 4.0, 0.05)}


def torch_form(x, t, gp, gn, m):
    xf = x.float()
    tf = t.float()
    if gp == 0 and gn == 0 and m == 0:
        return F.binary_cross_entropy_with_logits(xf, tf)
    p = torch.sigmoid(xf)
    q = (p - m).clamp(min=0)
    pos = tf * torch.pow(1 - p, gp) * -F.logsigmoid(xf)
    neg = (1 - tf) * torch.pow(q, gn) * -torch.log1p(-q)
    return (pos + neg).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlhead_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    lines = [f"sample = {args.reps} forward + backward calls ending in a synchronise, median [min .. max] of {args.samples} samples, "
             f"the routes in turn; peak = device memory of one call above the inputs; bfloat16 features and weights, uint8 labels"]

    def sample(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps             # ms per call

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2**20

    def measure(title, runs, reps):
        for _, fn in runs:                                          # warm-up: code objects, allocator pools, GEMM algorithms
            for _ in range(3):
                sample(fn, reps)
        times = [[] for _ in runs]
        for _ in range(args.samples):
            for i, (_, fn) in enumerate(runs):
                times[i].append(sample(fn, reps))
        peaks = [peak(fn) for _, fn in runs]
        first = len(lines)
        lines.append(title)
        meds = [statistics.median(ts) for ts in times]
        for (name, _), ts, md, pk in zip(runs, times, meds, peaks):
            lines.append(f"  {name:<44} {md:9.3f} ms [{min(ts):9.3f} .. {max(ts):9.3f}]  peak {pk:9.1f} MiB")
        for i in range(1, len(runs)):
            whole = "the fused range lies below it" if max(times[0]) < min(times[i]) else (
                "the fused range lies ABOVE it" if min(times[0]) > max(times[i]) else "the ranges overlap")
            lines.append(f"  fused / {runs[i][0].split(':')[0]} = {meds[0] / meds[i]:.3f} ({whole})")
        for ln in lines[first:]:
            print(ln, flush=True)

    busy = torch.randn(4096, 4096, device=dev)                      # bring the clocks up before the first sample
    for _ in range(50):
        busy = torch.tanh(busy @ busy * 1e-4)
    torch.cuda.synchronize()
    del busy
    for n, c, k in SHAPES:
        g = torch.Generator().manual_seed(7)
        labels = (torch.rand(n, c, generator=g) < 0.1).to(torch.uint8).to(dev)
        hidden = torch.randn(n, k, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
        weight = (torch.randn(c, k, generator=g) * (2.0 / k ** 0.5)).to(torch.bfloat16).to(dev).requires_grad_(True)
        bias = (torch.randn(c, generator=g) - 2.0).to(torch.bfloat16).to(dev).requires_grad_(True)
        reps = args.reps if n * c >= 1 << 20 else 20 * args.reps
        for label, (gp, gn, m) in FORMS.items():
            opts = dict(gamma_pos=gp, gamma_neg=gn, margin=m)

            def clear():
                hidden.grad = weight.grad = bias.grad = None

            def fused():
                clear()
                losses.linear_multilabel_loss(hidden, weight, bias, labels, **opts).backward()

            def unfused():
                clear()
                losses.multilabel_loss(F.linear(hidden, weight, bias), labels, **opts).backward()

            def eager():
                clear()
                torch_form(F.linear(hidden, weight, bias), labels, gp, gn, m).backward()

            with torch.no_grad():
                vals = (float(losses.linear_multilabel_loss(hidden, weight, bias, labels, **opts)),
                        float(losses.multilabel_loss(F.linear(hidden, weight, bias), labels, **opts)),
                        float(torch_form(F.linear(hidden, weight, bias), labels, gp, gn, m)))
            measure(f"{n} x {c} x {k}, {label}: loss {vals[0]:.6f} fused, {vals[1]:.6f} (a), {vals[2]:.6f} (b)",
                    [("linear_multilabel_loss (fused)", fused), ("(a): F.linear + multilabel_loss", unfused),
                     ("(b): torch eager linear + float + loss", eager)], reps)
            if (n, c, k) == SHAPES[0]:
                hidden.requires_grad_(False)
                measure(f"{n} x {c} x {k}, {label}, frozen features (no dh)",
                        [("linear_multilabel_loss (fused)", fused), ("(a): F.linear + multilabel_loss", unfused)], reps)
                hidden.requires_grad_(True)
        del hidden, weight, bias, labels
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
