"""Timing and peak memory of the symmetric InfoNCE with a key queue (losses._QueuedNce: aecf_nce_queue_pass1 / _loss / _grads) on
one GPU, one rank's share, learnable temperature, forward + backward (normalise of the local rows of both views, the loss, every
gradient), at four sizes rows x cols x d with a FULL queue of q_cap keys per view (the cost follows the capacity, not the count):

    8192 x 65536 x 768, q_cap 65536        8192 x 65536 x 768, q_cap 8192        64 x 64 x 256, q_cap 4096        64 x 64 x 256, q_cap 65536

against, on the same inputs in the same process:

  * symmetric InfoNCE on the tile form without a queue (losses._NceSymmetric): one logits block and two products of the seven;
  * NT-Xent on the tile form (losses._NtXentSymmetric) over rows x cols: three logits blocks and six products -- at q_cap = cols
    the queue form does 14 rows cols d MFMA flops against its 18 and should not lie above it;
  * today's alternative to the queue form: two losses._NceDirection calls, each against torch.cat of the gathered rows and the
    stored keys (the concatenation included): two full logits blocks, gradient products on the stored keys too.

The gathered rows are made here instead of by an all-gather; everything after the gather is the code the drivers run (their
autograd functions on the normalised rows).  A sample is the device-event time of STEPS steps; the forms are sampled in turn
(alternating, so that drift hits all alike) and the median, minimum and maximum over SAMPLES samples are printed, then
torch.cuda.max_memory_allocated of one forward + backward of each above what is allocated before the call.

``--parent-lib``: another build of the library (the parent commit's), loaded beside this one: the three calls of info_nce's tile
form (aecf_nce_sym_pass1_dt / _loss_dt / _grads_dt) are then timed through the C ABI from both builds in turn at the first size --
no kernel they run may have moved.

    python tools/queue_nce_time.py [--parent-lib path/to/libaecf_hip.so]
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

STEPS, SAMPLES, WARMUP = 5, 9, 3
MIN_T = 0.025
SIZES = ((8192, 65536, 768, 65536), (8192, 65536, 768, 8192), (64, 64, 256, 4096), (64, 64, 256, 65536))


def measure(rows, cols, d, q_cap, dev):
    off = (cols // rows // 2) * rows                  # a rank in the middle
    g = torch.Generator().manual_seed(5)
    bf = torch.bfloat16
    unit = lambda n: losses.l2_normalize(torch.randn(n, d, generator=g).to(bf).to(dev)).detach()
    za = torch.randn(rows, d, generator=g).to(bf).to(dev).requires_grad_(True)
    zb = torch.randn(rows, d, generator=g).to(bf).to(dev).requires_grad_(True)
    na_all, nb_all = unit(cols).requires_grad_(True), unit(cols).requires_grad_(True)
    queue = losses.KeyQueue(q_cap, d, dev)
    queue.push(unit(q_cap), unit(q_cap), normalize=False)          # full: every slot a key
    ls = torch.tensor(2.3, device=dev, requires_grad=True)
    params = [za, zb, na_all, nb_all, ls]
    coef = 0.5 / cols

    def step(form):
        for p in params:
            p.grad = None
        t = (1 / ls.exp()).reshape(1)
        na = losses.l2_normalize(za)
        if form == "queue":
            loss = losses._QueuedNce.apply(na, losses.l2_normalize(zb), nb_all, queue, off, t, coef, None, MIN_T)
        elif form == "nce":
            loss, _ = losses._NceSymmetric.apply(na, nb_all, None, off, t, coef, None, 2, 0.0, MIN_T, 1.0)
        elif form == "ntxent":
            loss = losses._NtXentSymmetric.apply(na, losses.l2_normalize(zb), na_all, nb_all, off, t, coef, None, MIN_T)
        else:
            nb = losses.l2_normalize(zb)
            loss = losses._NceDirection.apply(na, torch.cat([nb_all, queue.keys_b]), off, t, coef, False, MIN_T) \
                + losses._NceDirection.apply(nb, torch.cat([na_all, queue.keys_a]), off, t, coef, False, MIN_T)
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

    def peak(form):
        for p in params:
            p.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step(form)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    lib = _lib.load()
    forms = [("InfoNCE with a key queue, tile form", "queue", lib.aecf_nce_queue_workspace_bytes(rows, cols, q_cap, d)),
             ("InfoNCE, tile form, no queue", "nce", lib.aecf_nce_sym_workspace_bytes(rows, cols, d)),
             ("NT-Xent, tile form (rows x cols)", "ntxent", lib.aecf_ntxent_sym_workspace_bytes(rows, cols, d)),
             ("two directions on torch.cat-ed keys", "cat", lib.aecf_nce_workspace_bytes(rows, cols + q_cap, d, _lib.AECF_BF16))]
    values = []
    for _, form, _ in forms:
        for _ in range(WARMUP):
            loss = step(form)
        values.append(float(loss.detach()))
    times = [[] for _ in forms]
    for _ in range(SAMPLES):
        for i, (_, form, _) in enumerate(forms):
            times[i].append(sample(form))
    print(f"\none rank, forward + backward, {rows} x {cols} x {d}, q_cap = {q_cap} (full), bf16, learnable T; sample = {STEPS} steps, "
          f"median [min .. max] of {SAMPLES} samples, forms in turn")
    for (label, _, ws), ts, v in zip(forms, times, values):
        print(f"{label:<38} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]  workspace {ws / 2**20:8.1f} MiB  "
              f"loss {v:.6f}", flush=True)
    med = [statistics.median(ts) for ts in times]
    print(f"queue / no queue, medians: {med[0] / med[1]:.3f}   queue / NT-Xent, medians: {med[0] / med[2]:.3f}   "
          f"torch.cat-ed directions / queue, medians: {med[3] / med[0]:.3f}", flush=True)
    if q_cap == cols:
        print(f"q_cap = cols: the queue form's median lies {'above' if med[0] > med[2] else 'not above'} NT-Xent's "
              f"(ranges [{min(times[0]):.3f} .. {max(times[0]):.3f}] and [{min(times[2]):.3f} .. {max(times[2]):.3f}])", flush=True)
    print("peak device memory of one forward + backward above what is allocated before it (torch.cuda.max_memory_allocated):")
    for label, form, _ in forms:
        print(f"{label:<38} {peak(form) / 2**20:10.1f} MiB", flush=True)


def parent_check(path, rows, cols, d, dev):
    """the three calls of info_nce's tile form from this build and from the build at ``path``, in turn"""
    here = _lib.load()
    other = ctypes.CDLL(os.path.abspath(path))
    names = ("aecf_nce_sym_workspace_bytes", "aecf_nce_sym_pass1_dt", "aecf_nce_sym_loss_dt", "aecf_nce_sym_grads_dt")
    for name, restype, argtypes in _lib._SYMBOLS:
        if name in names:
            getattr(other, name).restype, getattr(other, name).argtypes = restype, argtypes
    g = torch.Generator().manual_seed(6)
    bf = torch.bfloat16
    f32 = dict(dtype=torch.float32, device=dev)
    na = losses.l2_normalize(torch.randn(rows, d, generator=g).to(bf).to(dev)).detach()
    nb_all = losses.l2_normalize(torch.randn(cols, d, generator=g).to(bf).to(dev)).detach()
    off, coef = (cols // rows // 2) * rows, 0.5 / cols
    t, up = torch.tensor([0.1], **f32), torch.ones(1, **f32)
    wsb = here.aecf_nce_sym_workspace_bytes(rows, cols, d)
    assert wsb == other.aecf_nce_sym_workspace_bytes(rows, cols, d)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    col_sums, loss_rows, d_t = torch.empty(cols, **f32), torch.empty(rows, **f32), torch.empty(1, **f32)
    da, db = torch.empty(rows, d, dtype=bf, device=dev), torch.empty(cols, d, dtype=bf, device=dev)
    s = _stream()

    def run(lib):
        st = lib.aecf_nce_sym_pass1_dt(rows, cols, d, _ptr(t), MIN_T, _ptr(na), _ptr(nb_all), _ptr(ws), wsb, _ptr(col_sums), s)
        st |= lib.aecf_nce_sym_loss_dt(rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(nb_all), _ptr(col_sums), _ptr(ws), wsb,
                                       _ptr(loss_rows), 0, 2, 0.0, None, 1.0, None, None, s)
        st |= lib.aecf_nce_sym_grads_dt(rows, cols, off, d, _ptr(t), MIN_T, coef, _ptr(na), _ptr(nb_all), _ptr(ws), wsb, _ptr(up),
                                        _lib.AECF_BF16, _ptr(da), _ptr(db), _ptr(d_t), s)
        if st != 0:
            raise SystemExit(f"queue_nce_time: an aecf_nce_sym_*_dt call answered {st}")

    def sample(lib):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            run(lib)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS

    outs = []
    for lib in (here, other):
        for _ in range(WARMUP):
            run(lib)
        torch.cuda.synchronize()
        outs.append((loss_rows.clone(), da.clone(), db.clone(), d_t.clone()))
    same = all(torch.equal(x, y) for x, y in zip(*outs))
    times = [[], []]
    for _ in range(SAMPLES):
        for i, lib in enumerate((here, other)):
            times[i].append(sample(lib))
    print(f"\ninfo_nce's tile form through the C ABI (aecf_nce_sym_pass1_dt + _loss_dt + _grads_dt), {rows} x {cols} x {d}, this build "
          f"and the parent commit's in turn; sample = {STEPS} steps, median [min .. max] of {SAMPLES} samples")
    for label, ts in zip(("this build", "parent commit"), times):
        print(f"{label:<38} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]", flush=True)
    print(f"ranges overlap: {max(times[0]) >= min(times[1]) and max(times[1]) >= min(times[0])}   outputs bit-equal: {same}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libaecf_hip.so of the parent commit's build, for the A/B of info_nce's calls")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("queue_nce_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    for rows, cols, d, q_cap in SIZES:
        measure(rows, cols, d, q_cap, dev)
        torch.cuda.empty_cache()
    if args.parent_lib:
        parent_check(args.parent_lib, *SIZES[0][:3], dev)


if __name__ == "__main__":
    main()
