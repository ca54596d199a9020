"""Timing of the multi-label classification loss (aecf_amd.losses.multilabel_loss: forward + backward on the library's kernels)
against torch's eager equivalent, which is never the code under test:

  BCE with pos_weight   what the trainer calls without --loss: logits.float(), binary_cross_entropy_with_logits with pos_weight,
                        backward
  asymmetric (0, 4, 0.05)   an eager torch transcription of the definition (sigmoid, logsigmoid, clamp, pow, log1p), backward

A sample is the host-clock time of REPS forward + backward calls that ends in a device synchronise, after warm-up; the fused and
the torch route are sampled in turn in ONE process and the median, minimum and maximum over SAMPLES samples are printed, with
the device kernels one call launches (torch.profiler, where it reports device events), the peak device memory of one call above
what the inputs hold and, for the large shapes, the achieved bytes per second against the byte model -- forward: logit + label
per element; backward: logit + label + one gradient store -- and its share of the 8.0 TB/s HBM3E peak of an MI355X.

    python tools/mlloss_time.py [--out profiles/mlloss_time.txt] [--skip-trainer]

The last block times the example trainer's eager step at batch 64 (xray.train_step, FusedAdamW) with torch's criterion and with
MultilabelLoss (--loss bce), two copies of one model stepped in turn.
"""
import argparse
import copy
import os
import re
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aecf_amd import losses  # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = ((64, 15, "float32"), (65536, 80, "bfloat16"), (65536, 4096, "bfloat16"))
FORMS = {"BCE with pos_weight": (0.0, 0.0, 0.0), "asymmetric (0, 4, 0.05)": (0.0, 4.0, 0.05)}


def torch_form(x, t, pos_weight, gp, gn, m):
    xf = x.float()
    if gp == 0 and gn == 0 and m == 0:
        return F.binary_cross_entropy_with_logits(xf, t, pos_weight=pos_weight)
    p = torch.sigmoid(xf)
    q = (p - m).clamp(min=0)
    pos = t * torch.pow(1 - p, gp) * -F.logsigmoid(xf)
    neg = (1 - t) * torch.pow(q, gn) * -torch.log1p(-q)
    return (pos + neg).mean()


def kernels_of(fn):
    """names of the device kernels of one call, or None where the profiler reports no device events"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "Memcpy" not in e.name
                 and "Memset" not in e.name]
        return names or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--skip-trainer", action="store_true")
    ap.add_argument("--out", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlloss_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    lines = [f"sample = {args.reps} forward + backward calls ending in a synchronise, median [min .. max] of {args.samples} samples, "
             f"the two routes in turn; peak = device memory of one call above the inputs; labels float32"]

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

    busy = torch.randn(4096, 4096, device=dev)                      # bring the clocks up before the first sample
    for _ in range(50):
        busy = torch.tanh(busy @ busy * 1e-4)
    torch.cuda.synchronize()
    del busy
    for n, c, dtype in SHAPES:
        g = torch.Generator().manual_seed(7)
        labels = (torch.rand(n, c, generator=g) < 0.1).float().to(dev)
        logits = (2.0 * torch.randn(n, c, generator=g) - 1.0).to(getattr(torch, dtype)).to(dev).requires_grad_(True)
        pos_weight = (1.0 + 8.0 * torch.rand(c, generator=g)).to(dev)
        esize = logits.element_size()
        model_bytes = n * c * ((esize + 4) + (esize + 4 + esize))
        for label, (gp, gn, m) in FORMS.items():
            pw = pos_weight if gp == 0 and gn == 0 else None
            crit = losses.MultilabelLoss(pos_weight=pw, gamma_pos=gp, gamma_neg=gn, margin=m)

            def fused():
                logits.grad = None
                crit(logits, labels).backward()

            def eager():
                logits.grad = None
                torch_form(logits, labels, pw, gp, gn, m).backward()

            runs = [("multilabel_loss (fused)", fused), ("torch eager", eager)]
            for _, fn in runs:                                      # warm-up: code objects, allocator pools
                for _ in range(4):
                    sample(fn, args.reps)
            with torch.no_grad():
                a, b = float(crit(logits, labels)), float(torch_form(logits, labels, pw, gp, gn, m))
            times = [[] for _ in runs]
            for _ in range(args.samples):
                for i, (_, fn) in enumerate(runs):
                    times[i].append(sample(fn, args.reps))
            peaks = [peak(fn) for _, fn in runs]
            counts = [kernels_of(fn) for _, fn in runs]
            lines.append(f"{n} x {c} {dtype}, {label}: loss {a:.6f} fused, {b:.6f} torch")
            meds = []
            for (name, _), ts, pk, k in zip(runs, times, peaks, counts):
                meds.append(statistics.median(ts))
                rate = ""
                if n * c >= 1 << 20:
                    bps = model_bytes / (meds[-1] * 1e-3)
                    rate = f"  {bps / 1e12:6.3f} TB/s of the byte model, {bps / HBM_PEAK:6.1%} of the HBM peak"
                lines.append(f"  {name:<26} {meds[-1]:9.3f} ms [{min(ts):9.3f} .. {max(ts):9.3f}]  kernels "
                             f"{'not measured' if k is None else len(k)}  peak {pk:8.1f} MiB{rate}")
            if counts[0] is not None:
                short = [(re.findall(r"(mll_\w+|\w+_kernel\w*)", nm) or [nm[:40]])[0] for nm in counts[0]]
                lines.append(f"  the fused call's kernels: {', '.join(short)}")
            whole = "the fused range lies below torch's" if max(times[0]) < min(times[1]) else "the ranges OVERLAP or torch is faster"
            lines.append(f"  fused / torch = {meds[0] / meds[1]:.3f} ({whole})")
            for ln in lines[-5:]:
                print(ln, flush=True)
        del logits, labels

    if not args.skip_trainer:
        from aecf_amd.optim import FusedAdamW
        from aecf_amd.xray import AECFModel, train_step
        torch.manual_seed(3)
        base = AECFModel(512, 512, 15).to(dev).train()
        g = torch.Generator().manual_seed(9)
        image, text = torch.randn(64, 512, generator=g).to(dev), torch.randn(64, 512, generator=g).to(dev)
        labels = (torch.rand(64, 15, generator=g) < 0.2).float().to(dev)
        bce = torch.nn.BCEWithLogitsLoss()
        routes = []
        for name, crit in (("torch BCEWithLogitsLoss on logits.float()", lambda lg, y: bce(lg.float(), y)),
                           ("MultilabelLoss (--loss bce)", losses.MultilabelLoss())):
            model = copy.deepcopy(base)
            opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.01)
            routes.append((name, lambda model=model, opt=opt, crit=crit: train_step(model, opt, crit, image, text, labels)))
        for _, fn in routes:
            sample(fn, 20)
        times = [[] for _ in routes]
        for _ in range(args.samples):
            for i, (_, fn) in enumerate(routes):
                times[i].append(sample(fn, 20))
        lines.append("train_xray's eager step (xray.train_step, AECFModel 512 / 512 / 15, FusedAdamW) at batch 64, float32, 20 steps a sample")
        for (name, _), ts in zip(routes, times):
            lines.append(f"  {name:<44} {statistics.median(ts):9.3f} ms [{min(ts):9.3f} .. {max(ts):9.3f}]")
        for ln in lines[-3:]:
            print(ln, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
