"""float16 next to the other element types at the headline shape [B=65536, M=3, d=512, 8 heads], one process, one box:
the bench.py step (forward + entropy_loss + backward) and the forward alone (no gradient recording, train-mode masking), for
bf16, float16, float32 master parameters under float16 activations, and float32.  Median of n events-timed repetitions.
usage: f16_time.py [B] [n] [mode]   (mode: one of bf16, f16, f16m, f32 -- e.g. to profile one of them alone)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import torch  # noqa: E402

import bench  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
N = int(sys.argv[2]) if len(sys.argv) > 2 else 40
dev = torch.device("cuda:0")
MODES = [("bf16", "bf16", torch.bfloat16, False), ("f16", "f16", torch.float16, False),
         ("f16m", "f32 masters, f16 activations", torch.float16, True), ("f32", "f32", torch.float32, False)]
if len(sys.argv) > 3:
    MODES = [m for m in MODES if m[0] == sys.argv[3]]


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


rows = []
for _, name, dt, masters in MODES:
    pool, query, x, dy = bench.make_inputs((B, 3, 512, 8, dt, 0.15), dev, f32_params=masters)
    params = [query] + list(pool.parameters())
    t_step = timed(lambda: bench.step(pool, query, x, dy, params, False), N)

    def fwd():
        with torch.no_grad():
            pool(query.expand(B, -1, -1), x, return_info=True)

    t_fwd = timed(fwd, N)
    rows.append((name, t_step, t_fwd))
    del pool, query, x, dy, params
    torch.cuda.empty_cache()

print(f"B={B} M=3 d=512 H=8, {torch.cuda.get_device_name(0)}, median of {N}")
for name, t_step, t_fwd in rows:
    print(f"  {name:30s} fwd+bwd step {t_step:.3f} ms ({B / t_step / 1e3:6.1f} M samples/s)   forward only {t_fwd:.3f} ms")
