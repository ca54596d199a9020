"""Timing, launch counts and peak memory of multi-view InfoNCE (losses.multiview_info_nce) on one GPU against what it replaces: the
loop of losses.info_nce over the pairs, each pair on contiguous copies of its two views (the copies, the per-pair normalisation,
the seven launches per pair and the per-pair bf16 gradients that autograd then adds are the loop's cost and are timed with it).
Same process, same inputs x [B, M, d] bf16, learnable temperature, one rank, forward + backward:

    small    B = 2048, M = 4, d = 512, all pairs          (P = 6; a pair's logits GEMM is 64 tiles on 256 CUs)
    large    B = 8192, M = 3, d = 768, all pairs          (P = 3; every GEMM fills the device on its own)
    anchor   B = 4096, M = 8, d = 512, anchor = 0         (P = 7; view 0's gradient is one product over 7 partner blocks)

A sample is the device-event time of STEPS steps; the two forms are sampled in turn (alternating, so that drift hits both alike)
and the median, minimum and maximum over SAMPLES samples are printed; then torch.cuda.max_memory_allocated of one forward +
backward of each above what is allocated before the call; then, from torch.profiler on one step of each, the number of kernel
launches and the device time per kernel.

    python tools/multiview_time.py [--shape small|large|anchor]      (default: all three)
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
    ls = torch.tensor(2.3, device=dev, requires_grad=True)
    pairs = losses.multiview_pairs(M, anchor)

    def step(form):
        x.grad = ls.grad = None
        t = (1 / ls.exp()).reshape(1)
        if form == "multi":
            loss = losses.multiview_info_nce(x, temperature=t, anchor=anchor)
        else:
            loss = sum(losses.info_nce(x[:, m].contiguous(), x[:, n].contiguous(), temperature=t) for m, n in pairs) / len(pairs)
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

    def peak(form):
        x.grad = ls.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step(form)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    forms = [("multiview_info_nce", "multi"), ("loop of info_nce over the pairs", "loop")]
    values = []
    for _, form in forms:
        for _ in range(WARMUP):
            loss = step(form)
        values.append(float(loss.detach()))
    times = [[] for _ in forms]
    for _ in range(SAMPLES):
        for i, (_, form) in enumerate(forms):
            times[i].append(sample(form))
    print(f"== {name}: B = {b}, M = {M}, d = {d}, {'all pairs' if anchor is None else f'anchor = {anchor}'} (P = {len(pairs)}), bf16, "
          f"learnable T, forward + backward; sample = {STEPS} steps, median [min .. max] of {SAMPLES} samples, forms in turn")
    for (label, _), ts, v in zip(forms, times, values):
        print(f"{label:<34} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]  loss {v:.6f}", flush=True)
    med = [statistics.median(ts) for ts in times]
    print(f"loop / multi-view, medians: {med[1] / med[0]:.3f}   (the multi-view median not above the loop's range: "
          f"{med[0] <= max(times[1])}; its whole range below the loop's: {max(times[0]) < min(times[1])})", flush=True)
    print("peak device memory of one forward + backward above what is allocated before it (torch.cuda.max_memory_allocated):")
    for label, form in forms:
        print(f"{label:<34} {peak(form) / 2**20:10.1f} MiB", flush=True)
    try:
        from torch.profiler import ProfilerActivity, profile
        for label, form in forms:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                step(form)
                torch.cuda.synchronize()
            rows = [e for e in prof.key_averages() if getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0)) > 0]
            dev_us = lambda e: getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0))
            rows.sort(key=dev_us, reverse=True)
            print(f"kernels of one step, {label}: {sum(e.count for e in rows)} launches, {sum(dev_us(e) for e in rows) / 1e3:.3f} ms on the device")
            for e in rows[:14]:
                print(f"    {e.count:4d} x {dev_us(e) / e.count / 1e3:8.3f} ms = {dev_us(e) / 1e3:8.3f} ms  {e.key[:110]}")
            rest = rows[14:]
            if rest:
                print(f"    {sum(e.count for e in rest):4d} further launches, {sum(dev_us(e) for e in rest) / 1e3:8.3f} ms")
    except Exception as e:  # the profiler is an extra: the times above do not depend on it
        print(f"kernel breakdown not available here: {type(e).__name__}: {e}")
    print(flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=list(SHAPES), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multiview_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    for name in ([args.shape] if args.shape else list(SHAPES)):
        run(name, dev)


if __name__ == "__main__":
    main()
