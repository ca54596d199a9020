"""Timing of top-k retrieval on one rank's block of the configs[2] problem: 8192 queries against 65536 gathered keys, d = 768,
bf16, k = 10 -- aecf_retrieval_topk -- against (b) the retrieval counting pass on the same block (aecf_retrieval_positive +
aecf_retrieval_ranks, both directions: the same MFMA work with a counting epilogue) and (c) what a user does without the call:
torch.topk over the float32 block a @ b.T (the float32 copies of the operands are made outside the timed region).

A sample is the device-event time of REPS calls; the three are sampled in turn (alternating, so that drift hits all alike) in
ONE process and the median, minimum and maximum over SAMPLES samples are printed, then the peak device memory above the inputs
of one losses.retrieval_topk call and of one torch.topk over the block.

    python tools/topk_time.py [--rows 8192] [--cols 65536] [--d 768] [--k 10] [--out profiles/topk_time.txt]

Kernel split (a run of its own; tracing slows the host, so its times are not the ones above):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/topk_time.py --samples 1 --reps 3
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aecf_amd import _lib, losses  # noqa: E402
from aecf_amd.layer import _ptr, _stream  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--cols", type=int, default=65536)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--offset", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    rows, cols, d, k, off = args.rows, args.cols, args.d, args.k, args.offset
    g = torch.Generator().manual_seed(3)
    zb = torch.randn(cols, d, generator=g)
    za_full = (0.15 * zb + torch.randn(cols, d, generator=g)).to(torch.bfloat16).to(dev)
    nb = losses.l2_normalize(zb.to(torch.bfloat16).to(dev)).detach()
    na_full = losses.l2_normalize(za_full).detach()
    a = na_full[off:off + rows].contiguous()
    lib = _lib.load()
    pos_col = torch.empty(cols, dtype=torch.float32, device=dev)
    _lib.check(lib.aecf_retrieval_positive(cols, cols, 0, d, _ptr(na_full), _ptr(nb), _ptr(pos_col), _stream()), "aecf_retrieval_positive")
    del na_full, za_full

    values = torch.empty(rows, k, dtype=torch.float32, device=dev)
    indices = torch.empty(rows, k, dtype=torch.int32, device=dev)
    t_bytes = lib.aecf_retrieval_topk_workspace_bytes(rows, cols, d, k)
    t_ws = torch.empty(t_bytes, dtype=torch.uint8, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    pos = torch.empty(rows, dtype=torch.float32, device=dev)
    outs = [torch.empty(rows, **i32), torch.empty(rows, **i32), torch.empty(cols, **i32), torch.empty(cols, **i32)]
    r_bytes = lib.aecf_retrieval_workspace_bytes(rows, cols, d)
    r_ws = torch.empty(r_bytes, dtype=torch.uint8, device=dev)
    a32, b32 = a.float(), nb.float()

    def topk():
        _lib.check(lib.aecf_retrieval_topk(rows, cols, 0, d, k, 0, _ptr(a), _ptr(nb), _ptr(values), _ptr(indices), _ptr(t_ws), t_bytes,
                                           _stream()), "aecf_retrieval_topk")

    def ranks():
        _lib.check(lib.aecf_retrieval_positive(rows, cols, off, d, _ptr(a), _ptr(nb), _ptr(pos), _stream()), "aecf_retrieval_positive")
        _lib.check(lib.aecf_retrieval_ranks(rows, cols, off, d, _ptr(a), _ptr(nb), _ptr(pos), _ptr(pos_col), *[_ptr(t) for t in outs],
                                            _ptr(r_ws), r_bytes, _stream()), "aecf_retrieval_ranks")

    def torch_topk():
        return torch.topk(a32 @ b32.T, k, dim=1)

    runs = [(f"top-k, k = {k} (aecf_retrieval_topk)", topk),
            ("retrieval ranks (aecf_retrieval_positive + _ranks)", ranks),
            ("torch.topk over the float32 a @ b.T block", torch_topk)]

    def sample(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps                  # ms per call

    for _, fn in runs:                                          # warm-up: code objects, the allocator's blocks
        for _ in range(2):
            sample(fn)
    times = [[] for _ in runs]
    for _ in range(args.samples):
        for i, (_, fn) in enumerate(runs):
            times[i].append(sample(fn))

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated(dev) - base) / 2**20

    del t_ws
    peak_a = peak(lambda: losses.retrieval_topk(a, nb, k, normalize=False))
    peak_c = peak(torch_topk)

    lines = [f"{rows} x {cols} x {d} bf16, k = {k}, one rank, one direction: sample = {args.reps} calls, median [min .. max] of "
             f"{args.samples} samples, the three in turn; workspace {t_bytes / 2**20:.1f} MiB"]
    meds = []
    for (label, _), ts in zip(runs, times):
        meds.append(statistics.median(ts))
        lines.append(f"{label:<58} {meds[-1]:7.3f} ms [{min(ts):7.3f} .. {max(ts):7.3f}]")
    lines.append(f"top-k / retrieval ranks = {meds[0] / meds[1]:.3f}, torch.topk / top-k = {meds[2] / meds[0]:.2f}")
    lines.append(f"peak device memory above the inputs: losses.retrieval_topk {peak_a:.1f} MiB, torch.topk over the block {peak_c:.1f} MiB")
    for ln in lines:
        print(ln, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
