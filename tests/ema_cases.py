"""The moving average of FusedAdamW(ema_decay=...) restated in float64, its single-step bound, and numpy emulations of the
kernel's arithmetic and of the forms it must NOT use (shared by tests/test_optim_ema_cpu.py and tests/test_optim_ema_gpu.py).

The restatement takes what the kernel sees: the stored float32 weight w', the float32 average e before the step, and
om = float32(1) - float32(beta) (one float32 subtraction, exact for beta >= 0.5).  The kernel computes
    e' = fma(om, fl(w' - e), e)
-- one rounding of the difference, one of the fused sum -- so against the exact E = e + om (w' - e):
    |e' - E| <= 2^-24 om |w' - e|  +  2^-24 |E| (1 + 2^-24)   (+ one float32 subnormal step)
BOUND below is that with 1 % of slack: 2^-24 (om |w' - e| + |E|) 1.01 + 2^-126.  The other two forms one could write leave it:
e + fl(om fl(w' - e)) reaches 1.15 of it and fl(beta e) + fl(om w') 1.96 at the worst element of the sweep in the CPU test (the
kernel's form: 0.99)."""
import numpy as np

SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 4097)         # below / at / above a lane's 8 and a block's 2048; two blocks and a tail
BETAS = (0.9, 0.9999)

f32 = np.float32


def one_minus(beta):
    """om as the kernel forms it: beta clamped to [0, 1], then ONE float32 subtraction."""
    b = f32(beta)
    b = f32(0.0) if b < 0 else b
    b = f32(1.0) if b > 1 else b
    return f32(1.0) - b


def exact(w, e, beta):
    """E in float64 from the float32 inputs the kernel read."""
    w, e = np.asarray(w, np.float32).astype(np.float64), np.asarray(e, np.float32).astype(np.float64)
    return e + float(one_minus(beta)) * (w - e)


def bound(w, e, beta):
    w, e = np.asarray(w, np.float32).astype(np.float64), np.asarray(e, np.float32).astype(np.float64)
    om = float(one_minus(beta))
    return 2.0 ** -24 * (om * np.abs(w - e) + np.abs(exact(w, e, beta))) * 1.01 + 2.0 ** -126


def excess(got, w, e, beta):
    """max over the elements of |got - E| / BOUND: inside the bound when <= 1."""
    got = np.asarray(got, np.float32).astype(np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - exact(w, e, beta)) / bound(w, e, beta)).max())


# ---- emulations in numpy (float32 operations; the fused sum through float64, where the product of two float32 is exact) ----
def fused(w, e, beta):
    """The kernel's form."""
    w, e = np.asarray(w, np.float32), np.asarray(e, np.float32)
    d = (w - e).astype(np.float32)
    return (float(one_minus(beta)) * d.astype(np.float64) + e.astype(np.float64)).astype(np.float32)


def unfused(w, e, beta):
    """e + fl(om fl(w' - e)): two roundings after the difference."""
    w, e = np.asarray(w, np.float32), np.asarray(e, np.float32)
    return (e + (one_minus(beta) * (w - e).astype(np.float32)).astype(np.float32)).astype(np.float32)


def beta_form(w, e, beta):
    """fl(fl(beta e) + fl(om w'))."""
    w, e = np.asarray(w, np.float32), np.asarray(e, np.float32)
    b = np.clip(f32(beta), f32(0), f32(1))
    return ((b * e).astype(np.float32) + (one_minus(beta) * w).astype(np.float32)).astype(np.float32)


def bf16_round(x):
    """float32 -> bf16 (round to nearest even) -> float32, as `x.to(torch.bfloat16).float()`."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)
