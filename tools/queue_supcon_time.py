"""Timing and peak memory of the supervised contrastive loss with a key queue (losses._QueuedSupCon: aecf_supcon_queue_pass1 / _loss /
_grads) on one GPU, one rank's share, learnable temperature, forward + backward (normalise of the local rows of both views, the
loss, every gradient), at the four sizes of tools/queue_nce_time.py, rows x cols x d with a FULL labelled queue of q_cap keys per
view (the cost follows the capacity, not the count):

    8192 x 65536 x 768, q_cap 65536        8192 x 65536 x 768, q_cap 8192        64 x 64 x 256, q_cap 4096        64 x 64 x 256, q_cap 65536

Labels: cols // 7 classes dealt at random over the gathered rows (about 6 label positives per row in the batch) and over the
stored keys.  Against, on the same inputs in the same process:

  * the symmetric InfoNCE with a key queue (losses._QueuedNce) at the same size: the same three blocks and four products, no labels;
  * the supervised contrastive loss on the tile form without a queue (losses._SupConSymmetric: supervised_contrastive with
    low_memory=False): one logits block and two products of the seven;
  * today's alternative to the queue form: two losses._SupConDirection calls (the streaming kernels), each against torch.cat of the
    gathered rows and the stored keys, and of their labels (the concatenations included).

The gathered rows are made here instead of by an all-gather; everything after the gather is the code the drivers run (their
autograd functions on the normalised rows).  A sample is the device-event time of STEPS steps; the forms are sampled in turn
(alternating, so that drift hits all alike) and the median, minimum and maximum over SAMPLES samples are printed, then
torch.cuda.max_memory_allocated of one forward + backward of each above what is allocated before the call.

``--parent-lib``: another build of the library (the parent commit's), loaded beside this one: the three calls of queued_info_nce
(aecf_nce_queue_*) and of supervised_contrastive's tile form (aecf_supcon_sym_*) are then run through the C ABI from both builds
in turn at the first size -- the outputs must be bit-equal, and no kernel they run may have moved.

    python tools/queue_supcon_time.py [--parent-lib path/to/libaecf_hip.so]
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
    classes = max(cols // 7, 1)
    lab_all = torch.randint(0, classes, (cols,), generator=g).to(dev)
    lab = lab_all[off:off + rows].contiguous()
    q_lab = torch.randint(0, classes, (q_cap,), generator=g).to(dev)
    queue = losses.KeyQueue(q_cap, d, dev, labels=True)
    queue.push(unit(q_cap), unit(q_cap), normalize=False, labels=q_lab)          # full: every slot a labelled key
    ls = torch.tensor(2.3, device=dev, requires_grad=True)
    params = [za, zb, na_all, nb_all, ls]
    coef = 0.5 / cols

    def step(form):
        for p in params:
            p.grad = None
        t = (1 / ls.exp()).reshape(1)
        na = losses.l2_normalize(za)
        if form == "supq":
            loss = losses._QueuedSupCon.apply(na, losses.l2_normalize(zb), nb_all, lab, lab_all, queue, off, t, coef, None, MIN_T)
        elif form == "nceq":
            loss = losses._QueuedNce.apply(na, losses.l2_normalize(zb), nb_all, queue, off, t, coef, None, MIN_T)
        elif form == "sup":
            loss = losses._SupConSymmetric.apply(na, nb_all, lab, lab_all, off, t, coef, None, MIN_T)
        else:
            nb = losses.l2_normalize(zb)
            k_lab = torch.cat([lab_all, queue.labels])
            loss = losses._SupConDirection.apply(na, torch.cat([nb_all, queue.keys_b]), lab, k_lab, off, t, coef, MIN_T, True) \
                + losses._SupConDirection.apply(nb, torch.cat([na_all, queue.keys_a]), lab, k_lab, off, t, coef, MIN_T, True)
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
    forms = [("supervised loss with a key queue, tile form", "supq", lib.aecf_supcon_queue_workspace_bytes(rows, cols, q_cap, d)),
             ("InfoNCE with a key queue, tile form", "nceq", lib.aecf_nce_queue_workspace_bytes(rows, cols, q_cap, d)),
             ("supervised loss, tile form, no queue", "sup", lib.aecf_supcon_sym_workspace_bytes(rows, cols, d)),
             ("two directions on torch.cat-ed keys", "cat", lib.aecf_supcon_workspace_bytes(rows, cols + q_cap, d))]
    values = []
    for _, form, _ in forms:
        for _ in range(WARMUP):
            loss = step(form)
        values.append(float(loss.detach()))
    times = [[] for _ in forms]
    for _ in range(SAMPLES):
        for i, (_, form, _) in enumerate(forms):
            times[i].append(sample(form))
    print(f"\none rank, forward + backward, {rows} x {cols} x {d}, q_cap = {q_cap} (full), {classes} classes, bf16, learnable T; "
          f"sample = {STEPS} steps, median [min .. max] of {SAMPLES} samples, forms in turn")
    for (label, _, ws), ts, v in zip(forms, times, values):
        print(f"{label:<44} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]  workspace {ws / 2**20:8.1f} MiB  "
              f"loss {v:.6f}", flush=True)
    med = [statistics.median(ts) for ts in times]
    print(f"supervised queue / InfoNCE queue, medians: {med[0] / med[1]:.3f}   supervised queue / no queue, medians: "
          f"{med[0] / med[2]:.3f}   torch.cat-ed directions / supervised queue, medians: {med[3] / med[0]:.3f}", flush=True)
    print("peak device memory of one forward + backward above what is allocated before it (torch.cuda.max_memory_allocated):")
    for label, form, _ in forms:
        print(f"{label:<44} {peak(form) / 2**20:10.1f} MiB", flush=True)


def parent_check(path, rows, cols, d, q_cap, dev):
    """the three calls of queued_info_nce and of supervised_contrastive's tile form from this build and from the build at
    ``path``, in turn: bit-equal outputs, and the times side by side"""
    here = _lib.load()
    other = ctypes.CDLL(os.path.abspath(path))
    names = ("aecf_nce_queue_workspace_bytes", "aecf_nce_queue_pass1", "aecf_nce_queue_loss", "aecf_nce_queue_grads",
             "aecf_supcon_sym_workspace_bytes", "aecf_supcon_sym_pass1", "aecf_supcon_sym_loss", "aecf_supcon_sym_grads")
    for name, restype, argtypes in _lib._SYMBOLS:
        if name in names:
            getattr(other, name).restype, getattr(other, name).argtypes = restype, argtypes
    g = torch.Generator().manual_seed(6)
    bf = torch.bfloat16
    f32 = dict(dtype=torch.float32, device=dev)
    unit = lambda n: losses.l2_normalize(torch.randn(n, d, generator=g).to(bf).to(dev)).detach()
    off, coef = (cols // rows // 2) * rows, 0.5 / cols
    na, nb_all, qa, qb = unit(rows), unit(cols), unit(q_cap), unit(q_cap)
    nb = nb_all[off:off + rows].contiguous()
    lab_all = torch.randint(0, max(cols // 7, 1), (cols,), generator=g).to(dev)
    lab = lab_all[off:off + rows].contiguous()
    qv = torch.tensor([q_cap], dtype=torch.int64, device=dev)
    t, up = torch.tensor([0.1], **f32), torch.ones(1, **f32)
    loss_rows, d_t = torch.empty(rows, **f32), torch.empty(1, **f32)
    da, db_loc, db = torch.empty(rows, d, dtype=bf, device=dev), torch.empty(rows, d, dtype=bf, device=dev), torch.empty(cols, d, dtype=bf, device=dev)
    col_sums, col_stats = torch.empty(cols, **f32), torch.empty(3, cols, **f32)
    s = _stream()
    wsq, wss = here.aecf_nce_queue_workspace_bytes(rows, cols, q_cap, d), here.aecf_supcon_sym_workspace_bytes(rows, cols, d)
    assert wsq == other.aecf_nce_queue_workspace_bytes(rows, cols, q_cap, d) and wss == other.aecf_supcon_sym_workspace_bytes(rows, cols, d)
    ws = torch.empty(max(wsq, wss), dtype=torch.uint8, device=dev)

    def run_queue(lib):
        st = lib.aecf_nce_queue_pass1(rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(nb), _ptr(qa), _ptr(qb), q_cap, _ptr(qv),
                                      _ptr(nb_all), _ptr(ws), wsq, _ptr(col_sums), s)
        st |= lib.aecf_nce_queue_loss(rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(nb_all), q_cap, _ptr(col_sums), _ptr(ws), wsq,
                                      _ptr(loss_rows), s)
        st |= lib.aecf_nce_queue_grads(rows, cols, off, d, _ptr(t), MIN_T, coef, _ptr(na), _ptr(nb), _ptr(qa), _ptr(qb), q_cap, _ptr(qv),
                                       _ptr(nb_all), _ptr(ws), wsq, _ptr(up), _lib.AECF_BF16, _ptr(da), _ptr(db_loc), _ptr(db), _ptr(d_t), s)
        if st != 0:
            raise SystemExit(f"queue_supcon_time: an aecf_nce_queue_* call answered {st}")
        return loss_rows, col_sums, da, db_loc, db, d_t

    def run_sup(lib):
        st = lib.aecf_supcon_sym_pass1(rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(nb_all), _ptr(lab), _ptr(lab_all), _ptr(ws),
                                       wss, _ptr(col_stats), s)
        st |= lib.aecf_supcon_sym_loss(rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(nb_all), _ptr(col_stats), _ptr(ws), wss,
                                       _ptr(loss_rows), s)
        st |= lib.aecf_supcon_sym_grads(rows, cols, off, d, _ptr(t), MIN_T, coef, _ptr(na), _ptr(nb_all), _ptr(lab), _ptr(lab_all),
                                        _ptr(ws), wss, _ptr(up), _lib.AECF_BF16, _ptr(da), _ptr(db), _ptr(d_t), s)
        if st != 0:
            raise SystemExit(f"queue_supcon_time: an aecf_supcon_sym_* call answered {st}")
        return loss_rows, col_stats, da, db, d_t

    def sample(run, lib):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            run(lib)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS

    for what, run in (("queued_info_nce's calls (aecf_nce_queue_pass1 + _loss + _grads)", run_queue),
                      ("supervised_contrastive's tile form (aecf_supcon_sym_pass1 + _loss + _grads)", run_sup)):
        outs = []
        for lib in (here, other):
            for _ in range(WARMUP):
                out = run(lib)
            torch.cuda.synchronize()
            outs.append([x.clone() for x in out])
        same = all(torch.equal(x, y) for x, y in zip(*outs))
        times = [[], []]
        for _ in range(SAMPLES):
            for i, lib in enumerate((here, other)):
                times[i].append(sample(run, lib))
        print(f"\n{what} through the C ABI, {rows} x {cols} x {d}" + (f", q_cap = {q_cap}" if run is run_queue else "")
              + f", this build and the parent commit's in turn; sample = {STEPS} steps, median [min .. max] of {SAMPLES} samples")
        for label, ts in zip(("this build", "parent commit"), times):
            print(f"{label:<44} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]", flush=True)
        print(f"ranges overlap: {max(times[0]) >= min(times[1]) and max(times[1]) >= min(times[0])}   outputs bit-equal: {same}",
              flush=True)
        if not same:
            raise SystemExit("queue_supcon_time: the outputs of the two builds differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libaecf_hip.so of the parent commit's build, for the A/B of the existing calls")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("queue_supcon_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    for rows, cols, d, q_cap in SIZES:
        measure(rows, cols, d, q_cap, dev)
        torch.cuda.empty_cache()
    if args.parent_lib:
        parent_check(args.parent_lib, *SIZES[0], dev)


if __name__ == "__main__":
    main()
