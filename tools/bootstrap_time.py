"""Timing of the bootstrap intervals (aecf_amd.metrics.bootstrap_metrics: one order per class by counting, the multiplicities of
all replicates, one walk with a lane per replicate) against what a user of this build did before it: a loop that draws a
resample of the rows, ``index_select``s them and calls ``multilabel_metrics`` once per replicate, then takes the quantiles of
the collected macro values.  The same number of replicates on both sides.

A sample is the host-clock time of one call that ends in a device synchronise; the two routes are sampled in turn in ONE
process and the median, minimum and maximum over SAMPLES samples are printed, with the peak device memory of one call of each
above what the inputs hold.  The three library passes (aecf_mlboot_order, _draw, _walk through the C ABI, no closing arithmetic)
are timed the same way, each on its own.

    python tools/bootstrap_time.py [--sizes 2048x15:1000,25600x15:1000,65536x80:100] [--out profiles/bootstrap_time.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aecf_amd import _lib, metrics  # noqa: E402
from aecf_amd.layer import _POOL_DTYPES, _ptr, _stream  # noqa: E402


def loop_route(logits, labels, n_boot, seed):
    """today's route: R gathers and R evaluations, the percentile limits of the macro values at the end"""
    g = torch.Generator(device=logits.device).manual_seed(seed)
    n = logits.shape[0]
    rows = []
    for _ in range(n_boot):
        idx = torch.randint(n, (n,), device=logits.device, generator=g)
        m = metrics.multilabel_metrics(logits.index_select(0, idx), labels.index_select(0, idx))
        rows.append(torch.stack([m["map"], m["macro_auroc"], m["macro_f1"]]))
    q = torch.tensor([0.025, 0.975], dtype=torch.float64, device=logits.device)
    return torch.nanquantile(torch.stack(rows), q, dim=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048x15:1000,25600x15:1000,65536x80:100", help="comma-separated N x C : replicates")
    ap.add_argument("--dtype", default="float32")
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bootstrap_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = [f"sample = 1 call ending in a synchronise, median [min .. max] of {args.samples} samples, the routes in turn; peak = "
             f"device memory of one call above the inputs"]

    def sample(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2**20

    for size in args.sizes.split(","):
        shape, _, reps = size.partition(":")
        n, c = (int(v) for v in shape.split("x"))
        n_boot = int(reps or 1000)
        g = torch.Generator().manual_seed(7)
        labels = (torch.rand(n, c, generator=g) < 0.2).float()
        logits = (torch.randn(n, c, generator=g) + 1.5 * labels - 1.0).to(getattr(torch, args.dtype)).to(dev)
        labels = labels.to(dev)
        y8 = (labels != 0).to(torch.uint8)
        out = {}

        def new():
            out["new"] = metrics.bootstrap_metrics(logits, labels, n_boot=n_boot, seed=7)

        def old():
            out["old"] = loop_route(logits, labels, n_boot, 7)

        # the three passes on their own, on one chunk of replicates (the call above runs ceil((n_boot + 1) / chunk) of them)
        chunk = min(metrics._boot_chunk(n), n_boot + 1)
        Np, Rp = (n + 63) // 64 * 64, (chunk + 63) // 64 * 64
        wsb, dwsb = lib.aecf_mlboot_workspace_bytes(n, c), lib.aecf_mlboot_draw_workspace_bytes(n, chunk)
        ws, dws = (torch.empty(b, dtype=torch.uint8, device=dev) for b in (wsb, dwsb))
        thr = torch.zeros(c, device=dev)
        cc = torch.empty(3, c, dtype=torch.int32, device=dev)
        order = torch.empty(c, Np, dtype=torch.int32, device=dev)
        w = torch.empty(n, Rp, dtype=torch.uint8, device=dev)
        sat = torch.zeros(1, dtype=torch.int32, device=dev)
        stats = torch.empty(chunk, 7, c, dtype=torch.int64, device=dev)

        def p_order():
            _lib.check(lib.aecf_mlboot_order(n, c, _POOL_DTYPES[logits.dtype], _ptr(logits), _ptr(y8), _ptr(thr), _ptr(cc), _ptr(order),
                                             _ptr(ws), wsb, _stream()), "aecf_mlboot_order")

        def p_draw():
            _lib.check(lib.aecf_mlboot_draw(n, chunk, 0, 7, None, _ptr(w), _ptr(sat), _ptr(dws), dwsb, _stream()), "aecf_mlboot_draw")

        def p_walk():
            _lib.check(lib.aecf_mlboot_walk(n, c, chunk, _ptr(cc), _ptr(order), _ptr(w), _ptr(stats), _stream()), "aecf_mlboot_walk")

        runs = [("bootstrap_metrics (order + draw + walk + closing)", new), ("loop of index_select + multilabel_metrics", old),
                ("  aecf_mlboot_order alone (prepare + order)", p_order), (f"  aecf_mlboot_draw alone, {chunk} replicates", p_draw),
                (f"  aecf_mlboot_walk alone, {chunk} replicates", p_walk)]
        for _, fn in runs:                                          # warm-up: code objects, allocator pools
            sample(fn)
        times = [[] for _ in runs]
        for _ in range(args.samples):
            for i, (_, fn) in enumerate(runs):
                times[i].append(sample(fn))
        peaks = [peak(fn) for _, fn in runs[:2]] + [None] * 3
        ci, loop_ci = out["new"]["map_ci"], out["old"][:, 0]
        lines.append(f"{n} x {c} {args.dtype}, {n_boot} replicates; mAP {float(out['new']['map']):.6f}, 95 % interval "
                     f"[{float(ci[0]):.6f}, {float(ci[1]):.6f}] (the loop's own draws: [{float(loop_ci[0]):.6f}, {float(loop_ci[1]):.6f}])")
        meds = []
        for (label, _), ts, pk in zip(runs, times, peaks):
            meds.append(statistics.median(ts))
            mem = f"  peak {pk:8.1f} MiB" if pk is not None else ""
            lines.append(f"  {label:<54} {meds[-1]:10.3f} ms [{min(ts):10.3f} .. {max(ts):10.3f}]{mem}")
        lines.append(f"  bootstrap_metrics / loop = {meds[0] / meds[1]:.4f}; whole range below the loop's: {max(times[0]) < min(times[1])}")
        for ln in lines[-7:]:
            print(ln, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
