"""Timing of the weights' moving average on one GPU, float32 and bf16 + master, 16 tensors:

  (a) aecf_adamw_mp_ema_step                     -- FusedAdamW(ema_decay=...), the average in the step's own launch;
  (b) aecf_adamw_mp_step + torch._foreach_lerp_  -- the average written in torch next to the step (on the float32 weights, the
                                                    masters for bf16), plus the cast to bf16 where (a) writes ema_out;
  (c) aecf_adamw_mp_step of this build against the same entry point of another build of the library (--parent-lib: the parent
      commit's libaecf_hip.so), through the C ABI: timed on the SAME tensors (the same addresses: where 28 B/element of streams
      land in memory moves a time by several percent), and whether five steps on equal copies end bit-equal;
  (d) bytes per element and achieved TB/s of (a).

As tools/optim_time.py: every variant is captured into a graph of STEPS launches (no Python between them); a sample is the
device-event time of REPLAYS replays, the variants are sampled in turn and the median, minimum and maximum over SAMPLES
samples are printed.

    python tools/ema_time.py [--sizes 1048576,16777216] [--tensors 16] [--parent-lib PATH]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aecf_amd import _lib, optim  # noqa: E402
from tools.optim_time import REPLAYS, SAMPLES, STEPS, capture, sample  # noqa: E402

BETA = 0.999
# (label, parameter dtype, masters, bytes per element of (a): the step's 28 + the average read and written + a bf16 ema_out)
CONFIGS = [("f32", torch.float32, False, 36), ("bf16 + master", torch.bfloat16, True, 38)]


class Bag(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t) for t in tensors])


def make(n, tensors, dtype, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    ps = [torch.randn(n // tensors, device=dev, generator=g).to(dtype) for _ in range(tensors)]
    grads = [torch.randn(n // tensors, device=dev, generator=g).to(dtype) for _ in range(tensors)]
    return ps, grads


def fused(n, tensors, dtype, masters, dev):
    ps, grads = make(n, tensors, dtype, dev, 1)
    bag = Bag(ps)
    for p, g in zip(bag.ps, grads):
        p.grad = g
    opt = optim.FusedAdamW(bag.ps, lr=torch.tensor(1e-4, device=dev), weight_decay=0.01, master_weights=masters, ema_decay=BETA)
    ema = optim.EmaModel(bag, opt)
    return opt.step, (bag, opt, ema)


def step_then_lerp(n, tensors, dtype, masters, dev):
    ps, grads = make(n, tensors, dtype, dev, 1)
    ps = [p.requires_grad_() for p in ps]
    for p, g in zip(ps, grads):
        p.grad = g
    opt = optim.FusedAdamW(ps, lr=torch.tensor(1e-4, device=dev), weight_decay=0.01, master_weights=masters)
    opt.step()                                                                  # (creates the masters)
    weights = [opt.state[p].get("master", p).detach() for p in ps]
    emas = [w.clone() for w in weights]
    outs = [torch.empty_like(p) for p in ps] if dtype != torch.float32 else None

    def run():
        opt.step()
        torch._foreach_lerp_(emas, weights, 1.0 - BETA)
        if outs is not None:
            torch._foreach_copy_(outs, emas)

    return run, (ps, opt, emas, outs)


class AbiStep:
    """aecf_adamw_mp_step of one build of the library, called through ctypes on tensors of its own."""

    def __init__(self, lib, n, tensors, dtype, masters, dev, share=None):
        self.lib = lib
        if share is None:
            ps, grads = make(n, tensors, dtype, dev, 1)
            self.p, self.g = ps, grads
            self.master = [p.float() for p in ps] if masters else None
            self.m = [torch.zeros(p.shape, device=dev) for p in ps]
            self.v = [torch.zeros(p.shape, device=dev) for p in ps]
            self.step = [torch.zeros((), device=dev) for _ in ps]
            self.ticket = torch.zeros(65 * ((tensors + 23) // 24), dtype=torch.int32, device=dev)
        else:
            self.p, self.g, self.master, self.m, self.v = share.p, share.g, share.master, share.m, share.v
            self.step, self.ticket = share.step, share.ticket
        ps, grads = self.p, self.g
        arr = lambda ts: (ctypes.c_void_p * tensors)(*[t.data_ptr() for t in ts])
        code = optim._DTYPES[dtype]
        self.args = (tensors, arr(ps), arr(grads), arr(self.master) if masters else None, arr(self.m), arr(self.v), arr(self.step),
                     (ctypes.c_int64 * tensors)(*[p.numel() for p in ps]), (ctypes.c_int32 * tensors)(*[code] * tensors),
                     (ctypes.c_int32 * tensors)(*[code] * tensors), self.ticket.data_ptr(), 1e-4, 0.9, 0.999, 1e-8, 0.01, None,
                     None, None, None, None)

    def __call__(self):
        _lib.check(self.lib.aecf_adamw_mp_step(*self.args, torch.cuda.current_stream().cuda_stream), "aecf_adamw_mp_step")

    def tensors(self):
        return self.p + (self.master or []) + self.m + self.v + self.step


def other_build(path):
    lib = ctypes.CDLL(path)
    ours = _lib.load().aecf_adamw_mp_step
    lib.aecf_adamw_mp_step.restype, lib.aecf_adamw_mp_step.argtypes = ours.restype, ours.argtypes
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1048576,16777216")
    ap.add_argument("--tensors", type=int, default=16)
    ap.add_argument("--parent-lib", default=None, help="libaecf_hip.so built from the parent commit, for (c)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    parent = other_build(args.parent_lib) if args.parent_lib else None
    print(f"graph of {STEPS} launches, sample = {REPLAYS} replays, median [min .. max] of {SAMPLES} samples, variants in turn")
    for n in (int(s) for s in args.sizes.split(",")):
        for name, dtype, masters, bytes_per in CONFIGS:
            runs, keep = [], []
            for label, build in (("(a) aecf_adamw_mp_ema_step", fused), ("(b) aecf_adamw_mp_step + _foreach_lerp_", step_then_lerp)):
                fn, held = build(n, args.tensors, dtype, masters, dev)
                runs.append((label, capture(fn)))
                keep.append(held)
            abis = [("(c) aecf_adamw_mp_step, this build", AbiStep(_lib.load(), n, args.tensors, dtype, masters, dev))]
            if parent is not None:
                abis.append(("(c) aecf_adamw_mp_step, parent build",
                             AbiStep(parent, n, args.tensors, dtype, masters, dev, share=abis[0][1])))
            for label, abi in abis:
                runs.append((label, capture(abi)))
            times = [[] for _ in runs]
            for _ in range(SAMPLES):
                for i, (_, graph) in enumerate(runs):
                    times[i].append(sample(graph))
            for (label, _), ts in zip(runs, times):
                med = statistics.median(ts)
                tail = f"  {bytes_per} B/elem  {bytes_per * n / med / 1e6:6.3f} TB/s" if label.startswith("(a)") else ""
                print(f"n={n:>9} tensors={args.tensors:>2} {name:<14} {label:<40} {med:8.2f} us [{min(ts):8.2f} .. {max(ts):8.2f}]{tail}",
                      flush=True)
            a, b = times[0], times[1]
            print(f"n={n:>9} {name:<14} (a) / (b) median {statistics.median(a) / statistics.median(b):.3f}; (a)'s range "
                  f"{'lies below' if max(a) < min(b) else 'does NOT lie below'} (b)'s", flush=True)
            if parent is not None:
                pair = [AbiStep(lib, n, args.tensors, dtype, masters, dev) for lib in (_lib.load(), parent)]
                for _ in range(5):
                    for abi in pair:
                        abi()
                same = all(torch.equal(x, y) for x, y in zip(pair[0].tensors(), pair[1].tensors()))
                c0, c1 = times[2], times[3]
                overlap = max(min(c0), min(c1)) <= min(max(c0), max(c1))
                print(f"n={n:>9} {name:<14} (c) outputs {'bit-equal' if same else 'DIFFER'}; ranges "
                      f"{'overlap' if overlap else 'do NOT overlap'}", flush=True)


if __name__ == "__main__":
    main()
