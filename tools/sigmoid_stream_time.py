"""Timing of the two implementations of the pairwise sigmoid loss on one GPU at the size of BASELINE configs[2]: one rank's
share of losses.sigmoid_contrastive, 8192 local rows against 65536 gathered rows, d = 768, learnable temperature and bias,
forward + backward (normalise of the local rows, the loss, every gradient), for low_memory=False (tile GEMMs, g kept as a
rows x cols bf16 block) and low_memory=True (the streaming form) in the same process.

The gathered rows of the other view are made here instead of by an all-gather; everything after the gather is the code
sigmoid_contrastive runs (its autograd functions on the normalised rows).  A sample is the device-event time of STEPS steps;
the two forms are sampled in turn (alternating, so that drift hits both alike) and the median, minimum and maximum over
SAMPLES samples are printed.

    python tools/sigmoid_stream_time.py [--rows 8192] [--cols 65536] [--d 768]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aecf_amd import _lib, losses  # noqa: E402

STEPS, SAMPLES, WARMUP = 5, 9, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--cols", type=int, default=65536)
    ap.add_argument("--d", type=int, default=768)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sigmoid_stream_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    rows, cols, d = args.rows, args.cols, args.d
    off = (cols // rows // 2) * rows                  # a rank in the middle
    g = torch.Generator().manual_seed(5)
    za = torch.randn(rows, d, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    nb_all = losses.l2_normalize(torch.randn(cols, d, generator=g).to(torch.bfloat16).to(dev)).detach().requires_grad_(True)
    ls = torch.tensor(2.3, device=dev, requires_grad=True)
    bias = torch.tensor([-10.0], device=dev, requires_grad=True)
    params = [za, nb_all, ls, bias]

    def step(low_memory):
        for p in params:
            p.grad = None
        t = (1 / ls.exp()).reshape(1)
        na = losses.l2_normalize(za)
        if low_memory:
            loss = losses._SigmoidStream.apply(na, nb_all, t, bias, off, 1.0 / cols, 1e-3, True)
        else:
            loss = losses._SigmoidContrastive.apply(na, nb_all, t, bias, off, 1.0 / cols, 1e-3)
        loss.backward()
        return loss

    def sample(low_memory):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            step(low_memory)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS                # ms per step

    lib = _lib.load()
    forms = [("low_memory=False (tile GEMMs)", False, lib.aecf_sig_workspace_bytes(rows, cols, d)),
             ("low_memory=True  (streaming)", True, lib.aecf_sig_stream_workspace_bytes(rows, cols, d))]
    values = []
    for _, low, _ in forms:
        for _ in range(WARMUP):
            loss = step(low)
        values.append(float(loss.detach()))
    times = [[] for _ in forms]
    for _ in range(SAMPLES):
        for i, (_, low, _) in enumerate(forms):
            times[i].append(sample(low))
    print(f"sigmoid loss forward + backward, {rows} x {cols} x {d}, bf16, learnable T and bias; sample = {STEPS} steps, "
          f"median [min .. max] of {SAMPLES} samples, forms in turn")
    for (label, _, ws), ts, v in zip(forms, times, values):
        print(f"{label:<32} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]  workspace {ws / 2**20:8.1f} MiB  "
              f"loss {v:.6f}", flush=True)


if __name__ == "__main__":
    main()
