"""Timing of the optimiser entry points on one GPU: aecf_adamw_step (the baseline, measured twice so that its own run-to-run
spread is on the page), aecf_adamw_mp_step in float32, bf16 + master and bf16 without master, and aecf_grad_norm.

Every variant is captured into a graph of STEPS launches (no Python between them); a sample is the device-event time of
REPLAYS replays, the variants are sampled in turn (alternating, so that drift hits all alike) and the median, minimum and
maximum over SAMPLES samples are printed, with the achieved bytes/s from the traffic table of DESIGN section 4.

    python tools/optim_time.py [--sizes 1048576,16777216] [--tensors 16]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aecf_amd import optim  # noqa: E402

STEPS, REPLAYS, SAMPLES = 20, 25, 9
# (label, parameter dtype, tensor lr, masters, bytes per element)
ADAMW = [("aecf_adamw_step f32 (baseline)", torch.float32, False, False, 28),
         ("aecf_adamw_step f32 (baseline again)", torch.float32, False, False, 28),
         ("aecf_adamw_mp_step f32", torch.float32, True, False, 28),
         ("aecf_adamw_mp_step bf16 + master", torch.bfloat16, True, True, 28),
         ("aecf_adamw_mp_step bf16 no master", torch.bfloat16, True, False, 22)]
NORM = [("aecf_grad_norm f32", torch.float32, 4), ("aecf_grad_norm bf16", torch.bfloat16, 2)]


def capture(fn):
    for _ in range(3):
        fn()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(STEPS):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def sample(graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPLAYS):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (REPLAYS * STEPS)          # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1048576,16777216")
    ap.add_argument("--tensors", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    print(f"graph of {STEPS} launches, sample = {REPLAYS} replays, median [min .. max] of {SAMPLES} samples, variants in turn")
    for n in (int(s) for s in args.sizes.split(",")):
        runs, keep = [], []
        for label, dtype, tensor_lr, masters, bytes_per in ADAMW:
            ps = [torch.randn(n // args.tensors, device=dev).to(dtype).requires_grad_() for _ in range(args.tensors)]
            for p in ps:
                p.grad = torch.randn_like(p)
            lr = torch.tensor(1e-4, device=dev) if tensor_lr else 1e-4
            opt = optim.FusedAdamW(ps, lr=lr, weight_decay=0.01, master_weights=masters)
            runs.append((label, bytes_per, capture(opt.step)))
            keep.append((ps, opt))
        for label, dtype, bytes_per in NORM:
            ps = [torch.randn(n // args.tensors, device=dev).to(dtype).requires_grad_() for _ in range(args.tensors)]
            for p in ps:
                p.grad = torch.randn_like(p)
            runs.append((label, bytes_per, capture(lambda ps=ps: optim.grad_norm(ps))))
            keep.append(ps)
        times = [[] for _ in runs]
        for _ in range(SAMPLES):
            for i, (_, _, graph) in enumerate(runs):
                times[i].append(sample(graph))
        for (label, bytes_per, _), ts in zip(runs, times):
            med = statistics.median(ts)
            print(f"n={n:>9} tensors={args.tensors:>2}  {label:<38} {med:8.2f} us [{min(ts):8.2f} .. {max(ts):8.2f}]  "
                  f"{bytes_per} B/elem  {bytes_per * n / med / 1e6:6.3f} TB/s", flush=True)


if __name__ == "__main__":
    main()
