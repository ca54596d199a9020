"""Timing and launch counts of multi-view InfoNCE with missing views (losses.multiview_info_nce(..., key_padding_mask=...)) on one
GPU.  Same process, same inputs x [B, M, d] bf16, learnable temperature, one rank, forward + backward, at the three shapes of
tools/multiview_time.py:

    small    B = 2048, M = 4, d = 512, all pairs          (P = 6)
    large    B = 8192, M = 3, d = 768, all pairs          (P = 3)
    anchor   B = 4096, M = 8, d = 512, anchor = 0         (P = 7)

Four forms, sampled in turn:
    unmasked                 multiview_info_nce(x): the path a call without a mask takes, which this mask leaves as it was
    masked, all present      key_padding_mask of zeros: the price of the mask where it is not needed (every tile takes the
                             unmasked tile's code after one vote; the masked normalisation, finalize and weights kernels, the
                             pair-coefficient launch and the per-pair final sum are the difference)
    masked, presence 0.7     a random mask, 0.7 per (row, view): every tile takes the select branch
    loop, presence 0.7       what a caller without the mask does: info_nce over index_select-ed subsets, pair by pair -- one
                             torch.nonzero (a host read of the pair's row count) and two gathered copies per pair, P launch chains;
                             it cannot be captured in a graph

A sample is the device-event time of STEPS steps (the loop's host reads fall inside it); the median, minimum and maximum over
SAMPLES samples are printed, then the ratios, then from torch.profiler on one step of each form the number of kernel launches and
the device time per kernel.

    python tools/multiview_masked_time.py [--shape small|large|anchor]      (default: all three)
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
PRESENCE = 0.7


def run(name, dev):
    b, M, d, anchor = SHAPES[name]
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(b, 1, d, generator=g) + torch.randn(b, M, d, generator=g)).to(torch.bfloat16).to(dev).requires_grad_(True)
    ls = torch.tensor(2.3, device=dev, requires_grad=True)
    pairs = losses.multiview_pairs(M, anchor)
    full = torch.zeros(b, M, dtype=torch.bool, device=dev)
    some = (torch.rand(b, M, generator=g) > PRESENCE).to(dev)
    host_reads = [0]

    def step(form):
        x.grad = ls.grad = None
        t = (1 / ls.exp()).reshape(1)
        if form == "plain":
            loss = losses.multiview_info_nce(x, temperature=t, anchor=anchor)
        elif form == "full":
            loss = losses.multiview_info_nce(x, temperature=t, anchor=anchor, key_padding_mask=full)
        elif form == "some":
            loss = losses.multiview_info_nce(x, temperature=t, anchor=anchor, key_padding_mask=some)
        else:
            terms = []
            for m, n in pairs:
                idx = torch.nonzero(~some[:, m] & ~some[:, n]).flatten()        # the host learns the pair's row count here
                host_reads[0] += 1
                if idx.numel():
                    terms.append(losses.info_nce(x[:, m].index_select(0, idx), x[:, n].index_select(0, idx), temperature=t))
            loss = sum(terms) / len(terms)
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

    forms = [("unmasked", "plain"), ("masked, all present", "full"), (f"masked, presence {PRESENCE}", "some"),
             (f"loop of info_nce, presence {PRESENCE}", "loop")]
    values = []
    for _, form in forms:
        for _ in range(WARMUP):
            loss = step(form)
        values.append(float(loss.detach()))
    times = [[] for _ in forms]
    for _ in range(SAMPLES):
        for i, (_, form) in enumerate(forms):
            times[i].append(sample(form))
    host_reads[0] = 0
    step("loop")
    print(f"== {name}: B = {b}, M = {M}, d = {d}, {'all pairs' if anchor is None else f'anchor = {anchor}'} (P = {len(pairs)}), bf16, "
          f"learnable T, forward + backward; sample = {STEPS} steps, median [min .. max] of {SAMPLES} samples, forms in turn")
    for (label, _), ts, v in zip(forms, times, values):
        print(f"{label:<34} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]  loss {v:.6f}", flush=True)
    med = [statistics.median(ts) for ts in times]
    print(f"masked, all present / unmasked, medians: {med[1] / med[0]:.3f}   (the two ranges overlap: "
          f"{min(times[1]) <= max(times[0]) and min(times[0]) <= max(times[1])})")
    print(f"masked, presence {PRESENCE} / unmasked, medians: {med[2] / med[0]:.3f}")
    print(f"loop / masked at presence {PRESENCE}, medians: {med[3] / med[2]:.3f}   (the masked form's whole range below the loop's: "
          f"{max(times[2]) < min(times[3])}); the loop reads the host {host_reads[0]} times per step and cannot be captured", flush=True)
    try:
        from torch.profiler import ProfilerActivity, profile
        for label, form in forms:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                step(form)
                torch.cuda.synchronize()
            dev_us = lambda e: getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0))
            rows = [e for e in prof.key_averages() if dev_us(e) > 0]
            rows.sort(key=dev_us, reverse=True)
            print(f"kernels of one step, {label}: {sum(e.count for e in rows)} launches, {sum(dev_us(e) for e in rows) / 1e3:.3f} ms on the device")
            top = 12 if form != "loop" else 8
            for e in rows[:top]:
                print(f"    {e.count:4d} x {dev_us(e) / e.count / 1e3:8.3f} ms = {dev_us(e) / 1e3:8.3f} ms  {e.key[:110]}")
            rest = rows[top:]
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
        raise SystemExit("multiview_masked_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    for name in ([args.shape] if args.shape else list(SHAPES)):
        run(name, dev)


if __name__ == "__main__":
    main()
