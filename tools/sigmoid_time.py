"""Timing of the two contrastive objectives on one rank's block of the configs[2] problem: 8192 local rows against 65536 gathered
keys, d = 768, bf16 -- the symmetric InfoNCE (aecf_nce_sym_*_dt) and the pairwise sigmoid loss (aecf_sig_*), each forward +
backward from unnormalised local rows to their gradient and the gathered keys' gradient, with a learnable temperature (and bias).

A sample is the device-event time of REPS forward + backward passes; the two objectives are sampled in turn (alternating, so
that drift hits both alike) in ONE process and the median, minimum and maximum over SAMPLES samples are printed.  InfoNCE is
the yardstick: it is measured in the same run.

    python tools/sigmoid_time.py [--rows 8192] [--cols 65536] [--d 768] [--out profiles/sigmoid_c3_time.txt]

Kernel split (a run of its own; tracing slows the host, so its times are not the ones above):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/sigmoid_time.py --samples 1 --reps 3
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aecf_amd import losses  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--cols", type=int, default=65536)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--offset", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sigmoid_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    zb = torch.randn(args.cols, args.d, generator=g)
    za = (0.8 * zb[args.offset:args.offset + args.rows] + 0.6 * torch.randn(args.rows, args.d, generator=g)).to(torch.bfloat16).to(dev)
    nb_all = losses.l2_normalize(zb.to(torch.bfloat16).to(dev)).detach().requires_grad_(True)
    za.requires_grad_(True)
    T = torch.tensor(0.1, device=dev, requires_grad=True)
    bias = torch.tensor(-10.0, device=dev, requires_grad=True)

    def info_nce():
        share, _ = losses._NceSymmetric.apply(losses.l2_normalize(za), nb_all, None, args.offset, T, 0.5 / args.cols, None, 2, 0.0,
                                              losses.MIN_TEMPERATURE, 1.0)
        share.backward()

    def sigmoid():
        share = losses._SigmoidContrastive.apply(losses.l2_normalize(za), nb_all, T, bias, args.offset, 1.0 / args.cols, 1e-3)
        share.backward()

    runs = [("info_nce symmetric (aecf_nce_sym_*_dt)", info_nce), ("sigmoid_contrastive (aecf_sig_*)", sigmoid)]

    def sample(fn):
        za.grad = nb_all.grad = T.grad = bias.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps                  # ms per forward + backward

    for _, fn in runs:                                          # warm-up: code objects, allocator
        for _ in range(2):
            sample(fn)
    times = [[] for _ in runs]
    for _ in range(args.samples):
        for i, (_, fn) in enumerate(runs):
            times[i].append(sample(fn))
    lines = [f"{args.rows} x {args.cols} x {args.d} bf16, row_offset {args.offset}, one rank, forward + backward, learnable T: "
             f"sample = {args.reps} passes, median [min .. max] of {args.samples} samples, objectives in turn"]
    meds = []
    for (label, _), ts in zip(runs, times):
        meds.append(statistics.median(ts))
        lines.append(f"{label:<42} {meds[-1]:7.3f} ms [{min(ts):7.3f} .. {max(ts):7.3f}]")
    lines.append(f"sigmoid / info_nce = {meds[1] / meds[0]:.3f}")
    for ln in lines:
        print(ln, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
