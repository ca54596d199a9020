"""Step time of the float32-master pool with the hi/lo weight-gradient products on and off, next to the bf16-parameter step, at the
per-rank shard shapes of BASELINE configs[2] (bench.py --config c3: [8192, 2, 768], 8 heads) and configs[4] (--config c5:
[16384, 4, 1024], 8 heads).  One process, one build, the modes interleaved over several rounds (median of each round's timed
steps); the same step as bench.py (forward + entropy loss + backward).
usage: hilo_time.py [--configs c3,c5] [--rounds 3] [--steps 40] [--modes bf16,f32_hilo,f32_default]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402


def timed(fn, n):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record()
    for i in range(n):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(n))
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c5")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--modes", default="bf16,f32_hilo,f32_default")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    modes = args.modes.split(",")
    for name in args.configs.split(","):
        cfg = bench.CONFIGS[name]
        runs = {}
        for mode in modes:
            pool, query, x, dy = bench.make_inputs(cfg, dev, f32_params=mode != "bf16")
            if mode == "f32_default":
                pool.options.hilo_grads = False
            params = [query] + list(pool.parameters())
            runs[mode] = (lambda pool=pool, query=query, x=x, dy=dy, params=params:
                          bench.step(pool, query, x, dy, params, False))
        times = {m: [] for m in modes}
        for _ in range(args.rounds):
            for m in modes:
                times[m].append(timed(runs[m], args.steps))
        B, M, E, H = cfg[:4]
        line = " ".join(f"{m}={' '.join(f'{t:.4f}' for t in times[m])}" for m in modes)
        print(f"{name} [B={B} M={M} d={E} H={H}] ms per step, {args.rounds} rounds: {line}")
        if "f32_hilo" in times and "f32_default" in times:
            on, off = min(times["f32_hilo"]), min(times["f32_default"])
            print(f"{name}: hi/lo on / off (best of rounds) = {on:.4f} / {off:.4f} ms = {100.0 * (on / off - 1.0):+.1f} %")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
