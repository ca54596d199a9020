"""Timing of multi-view InfoNCE with a learnable temperature PER PAIR (losses.multiview_info_nce(x, temperature=[P])) on one GPU,
against the same call with ONE learnable temperature and against what a user would otherwise write: the loop of losses.info_nce
over the pairs, each pair at its own temperature on contiguous copies of its two views.  Same process, same inputs x [B, M, d]
bf16, one rank, forward + backward:

    small    B = 2048, M = 4, d = 512, all pairs          (P = 6)
    large    B = 8192, M = 3, d = 768, all pairs          (P = 3)
    anchor   B = 4096, M = 8, d = 512, anchor = 0         (P = 7)

The temperatures are exp(-log_scale) of a learnable [P] (or one-element) log scale, as a training step would form them.  A sample
is the device-event time of STEPS steps; the three forms are sampled in turn (alternating, so that drift hits all alike) and the
median, minimum and maximum over SAMPLES samples are printed, then the launches and the device time per kernel of one step of the
two multi-view forms from torch.profiler: the per-pair form's logits launch is the instance with the second sweep.

    python tools/multiview_pairwise_time.py [--shape small|large|anchor]      (default: all three)
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aecf_amd import losses  # noqa: E402

STEPS, SAMPLES, WARMUP = 5, 9, 3
SHAPES = {"small": (2048, 4, 512, None), "large": (8192, 3, 768, None), "anchor": (4096, 8, 512, 0)}


def run(name, dev):
    b, M, d, anchor = SHAPES[name]
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(b, 1, d, generator=g) + torch.randn(b, M, d, generator=g)).to(torch.bfloat16).to(dev).requires_grad_(True)
    pairs = losses.multiview_pairs(M, anchor)
    P = len(pairs)
    ls1 = torch.tensor(2.3, device=dev, requires_grad=True)
    lsp = torch.linspace(1.2, 3.2, P).to(dev).requires_grad_(True)         # T from 0.30 down to 0.04

    def step(form):
        x.grad = ls1.grad = lsp.grad = None
        if form == "scalar":
            loss = losses.multiview_info_nce(x, temperature=(1 / ls1.exp()).reshape(1), anchor=anchor)
        elif form == "pairs":
            loss = losses.multiview_info_nce(x, temperature=1 / lsp.exp(), anchor=anchor)
        else:
            t = 1 / lsp.exp()
            loss = sum(losses.info_nce(x[:, m].contiguous(), x[:, n].contiguous(), temperature=t[p].reshape(1))
                       for p, (m, n) in enumerate(pairs)) / P
        loss.backward()
        return loss

    def sample(form):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            step(form)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS                # ms per step

    forms = [("multi-view, one learnable T", "scalar"), ("multi-view, a learnable T per pair", "pairs"),
             ("loop of info_nce, a T per pair", "loop")]
    values = []
    for _, form in forms:
        for _ in range(WARMUP):
            loss = step(form)
        values.append(float(loss.detach()))
    times = [[] for _ in forms]
    for _ in range(SAMPLES):
        for i, (_, form) in enumerate(forms):
            times[i].append(sample(form))
    print(f"== {name}: B = {b}, M = {M}, d = {d}, {'all pairs' if anchor is None else f'anchor = {anchor}'} (P = {P}), bf16, "
          f"forward + backward; sample = {STEPS} steps, median [min .. max] of {SAMPLES} samples, forms in turn")
    for (label, _), ts, v in zip(forms, times, values):
        print(f"{label:<36} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]  loss {v:.6f}", flush=True)
    med = [statistics.median(ts) for ts in times]
    print(f"per pair / one T, medians: {med[1] / med[0]:.3f}   (ranges overlap: {min(times[1]) <= max(times[0])})")
    print(f"loop / per pair, medians: {med[2] / med[1]:.3f}   (the per-pair form's whole range below the loop's: "
          f"{max(times[1]) < min(times[2])})", flush=True)
    try:
        from torch.profiler import ProfilerActivity, profile
        for label, form in forms[:2]:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                step(form)
                torch.cuda.synchronize()
            dev_us = lambda e: getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0))
            rows = [e for e in prof.key_averages() if dev_us(e) > 0]
            rows.sort(key=dev_us, reverse=True)
            print(f"kernels of one step, {label}: {sum(e.count for e in rows)} launches, {sum(dev_us(e) for e in rows) / 1e3:.3f} ms on the device")
            for e in rows[:8]:
                print(f"    {e.count:4d} x {dev_us(e) / e.count / 1e3:8.3f} ms = {dev_us(e) / 1e3:8.3f} ms  {e.key[:110]}")
    except Exception as e:  # the profiler is an extra: the times above do not depend on it
        print(f"kernel breakdown not available here: {type(e).__name__}: {e}")
    print(flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=list(SHAPES), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multiview_pairwise_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    for name in ([args.shape] if args.shape else list(SHAPES)):
        run(name, dev)


if __name__ == "__main__":
    main()
