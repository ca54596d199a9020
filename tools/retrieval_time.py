"""Timing of the retrieval counting pass on one rank's block of the configs[2] problem: 8192 local rows against 65536 gathered
rows, d = 768, bf16, row_offset 8192, both directions -- aecf_retrieval_positive + aecf_retrieval_ranks -- against the logits
pass of the symmetric InfoNCE (aecf_nce_sym_pass1), which forms the same block and also stores it.

A sample is the device-event time of REPS calls; the two are sampled in turn (alternating, so that drift hits both alike) in ONE
process and the median, minimum and maximum over SAMPLES samples are printed.  The InfoNCE pass is the yardstick: it is
measured in the same run.  ``--nce-lib`` takes it from another build of the library (e.g. the parent commit's), loaded beside
this one.

    python tools/retrieval_time.py [--rows 8192] [--cols 65536] [--d 768] [--out profiles/retrieval_time.txt]

Kernel split (a run of its own; tracing slows the host, so its times are not the ones above):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/retrieval_time.py --samples 1 --reps 3
"""
import argparse
import ctypes
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
    ap.add_argument("--offset", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--nce-lib", default=None, help="libaecf_hip.so of another build to take aecf_nce_sym_pass1 from")
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    rows, cols, d, off = args.rows, args.cols, args.d, args.offset
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

    nce = lib
    if args.nce_lib:
        nce = ctypes.CDLL(os.path.abspath(args.nce_lib))
        for name, restype, argtypes in _lib._SYMBOLS:
            if name in ("aecf_nce_sym_workspace_bytes", "aecf_nce_sym_pass1"):
                getattr(nce, name).restype, getattr(nce, name).argtypes = restype, argtypes

    i32 = dict(dtype=torch.int32, device=dev)
    pos = torch.empty(rows, dtype=torch.float32, device=dev)
    outs = [torch.empty(rows, **i32), torch.empty(rows, **i32), torch.empty(cols, **i32), torch.empty(cols, **i32)]
    r_bytes = lib.aecf_retrieval_workspace_bytes(rows, cols, d)
    r_ws = torch.empty(r_bytes, dtype=torch.uint8, device=dev)
    n_bytes = nce.aecf_nce_sym_workspace_bytes(rows, cols, d)
    n_ws = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    col_sums = torch.empty(cols, dtype=torch.float32, device=dev)

    def retrieval():
        _lib.check(lib.aecf_retrieval_positive(rows, cols, off, d, _ptr(a), _ptr(nb), _ptr(pos), _stream()), "aecf_retrieval_positive")
        _lib.check(lib.aecf_retrieval_ranks(rows, cols, off, d, _ptr(a), _ptr(nb), _ptr(pos), _ptr(pos_col), *[_ptr(t) for t in outs],
                                            _ptr(r_ws), r_bytes, _stream()), "aecf_retrieval_ranks")

    def nce_pass1():
        _lib.check(nce.aecf_nce_sym_pass1(rows, cols, d, 0.07, _ptr(a), _ptr(nb), _ptr(n_ws), n_bytes, _ptr(col_sums), _stream()),
                   "aecf_nce_sym_pass1")

    runs = [("retrieval ranks (aecf_retrieval_positive + _ranks)", retrieval),
            ("InfoNCE logits pass (aecf_nce_sym_pass1" + (", --nce-lib build)" if args.nce_lib else ")"), nce_pass1)]

    def sample(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps                  # ms per call

    for _, fn in runs:                                          # warm-up: code objects
        for _ in range(2):
            sample(fn)
    times = [[] for _ in runs]
    for _ in range(args.samples):
        for i, (_, fn) in enumerate(runs):
            times[i].append(sample(fn))
    lines = [f"{rows} x {cols} x {d} bf16, row_offset {off}, one rank, both retrieval directions: sample = {args.reps} calls, "
             f"median [min .. max] of {args.samples} samples, the two in turn; workspace {r_bytes / 2**20:.1f} MiB against "
             f"{n_bytes / 2**20:.1f} MiB"]
    meds = []
    for (label, _), ts in zip(runs, times):
        meds.append(statistics.median(ts))
        lines.append(f"{label:<58} {meds[-1]:7.3f} ms [{min(ts):7.3f} .. {max(ts):7.3f}]")
    lines.append(f"retrieval / InfoNCE logits pass = {meds[0] / meds[1]:.3f}")
    for ln in lines:
        print(ln, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
