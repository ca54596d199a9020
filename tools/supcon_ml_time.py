"""Timing and peak memory of the streaming multi-label supervised contrastive loss on one GPU at the size of BASELINE configs[2]:
one rank's share of one direction of losses.multilabel_contrastive, 8192 local rows against 65536 gathered rows, d = 768,
learnable temperature, forward + backward (normalise of the local rows, the loss, every gradient), under both weightings, against
the single-label streaming kernels (losses._SupConDirection, aecf_supcon_fwd_bwd) on the same embeddings in the same process.

The gathered rows of the other view and their sets are made here instead of by an all-gather; everything after the gather is the
code multilabel_contrastive runs (its autograd function on the normalised rows).  Sets: multi-hot rows over 15 classes, each class
present with probability 0.2 (about 3 classes per row, some rows empty), packed by aecf_label_sets_pack.  The single-label run
takes the label plan of tools/supcon_time.py (cols / 8 classes, one row in five unlabeled).  A sample is the device-event time of
STEPS steps; the three forms are sampled in turn (alternating, so that drift hits all alike) and the median, minimum and maximum
over SAMPLES samples are printed, with the ratios of the medians to the single-label one.  Then the same for the C ABI calls
alone, split by what they run -- the loss-only call (statistics role + row merge) and the full call minus it (the dq and dk
roles, the dq merge, dT) -- which says which roles carry a difference.  Then torch.cuda.max_memory_allocated of one forward +
backward of each, above what is allocated before the call, beside a torch float32 evaluation of the Jaccard form (rows x cols
logits and weight matrix) where that fits on the card.

    python tools/supcon_ml_time.py [--rows 8192] [--cols 65536] [--d 768]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aecf_amd import _lib, losses  # noqa: E402
from aecf_amd.layer import _ptr, _stream  # noqa: E402

STEPS, SAMPLES, WARMUP = 5, 9, 3
MIN_T = 1e-3
CLASSES, DENSITY = 15, 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--cols", type=int, default=65536)
    ap.add_argument("--d", type=int, default=768)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("supcon_ml_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    rows, cols, d = args.rows, args.cols, args.d
    off = (cols // rows // 2) * rows                  # a rank in the middle
    g = torch.Generator().manual_seed(5)
    za = torch.randn(rows, d, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    nb_all = losses.l2_normalize(torch.randn(cols, d, generator=g).to(torch.bfloat16).to(dev)).detach().requires_grad_(True)
    lk = torch.randint(0, max(cols // 8, 1), (cols,), generator=g)
    lk[torch.rand(cols, generator=g) < 0.2] = -1
    lk = lk.to(dev)
    lq = lk[off:off + rows].clone()
    hot = (torch.rand(cols, CLASSES, generator=g) < DENSITY).to(dev)
    sk = losses.pack_label_sets(hot)
    sq = sk[off:off + rows].clone()
    ls = torch.tensor(2.3, device=dev, requires_grad=True)
    params = [za, nb_all, ls]
    coef = 1.0 / cols
    weighting = {"overlap": _lib.AECF_SETS_OVERLAP, "jaccard": _lib.AECF_SETS_JACCARD}

    def step(form):
        for p in params:
            p.grad = None
        t = (1 / ls.exp()).reshape(1)
        na = losses.l2_normalize(za)
        if form == "single":
            loss = losses._SupConDirection.apply(na, nb_all, lq, lk, off, t, coef, MIN_T, True)
        elif form in weighting:
            loss = losses._SupConMlDirection.apply(na, nb_all, sq, sk, weighting[form], off, t, coef, MIN_T, True)
        else:                                         # torch, float32: the rows x cols logits and the Jaccard weight matrix
            x = (na.float() @ nb_all.float().T) / t.clamp_min(MIN_T)
            i = torch.arange(rows, device=dev)
            hq, hk = hot[off:off + rows].float(), hot.float()
            inter = hq @ hk.T
            union = hq.sum(1)[:, None] + hk.sum(1)[None, :] - inter
            w = inter / union.clamp_min(1.0)
            w[i, off + i] = 1.0
            loss = (torch.logsumexp(x, dim=1) - (x * w).sum(dim=1) / w.sum(dim=1)).sum() * coef
        loss.backward()
        return loss

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            fn()
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
        loss = step(form)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, float(loss.detach())

    def show(label, ts, tail=""):
        print(f"{label:<44} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]{tail}", flush=True)

    lib = _lib.load()
    forms = [("single label (aecf_supcon_fwd_bwd)", "single", lib.aecf_supcon_workspace_bytes(rows, cols, d)),
             ("multi-label, overlap", "overlap", lib.aecf_supcon_ml_workspace_bytes(rows, cols, d)),
             ("multi-label, jaccard", "jaccard", lib.aecf_supcon_ml_workspace_bytes(rows, cols, d))]
    values = []
    for _, form, _ in forms:
        for _ in range(WARMUP):
            loss = step(form)
        values.append(float(loss.detach()))
    times = [[] for _ in forms]
    for _ in range(SAMPLES):
        for i, (_, form, _) in enumerate(forms):
            times[i].append(timed(lambda: step(form)))
    hq = hot[off:off + min(rows, 1024)].float()
    shared = ((hq @ hot.float().T) > 0).float().sum(dim=1).mean().item()
    print(f"library: {os.path.relpath(_lib.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))}")
    print(f"one direction, forward + backward, {rows} x {cols} x {d}, bf16, learnable T; sample = {STEPS} steps, "
          f"median [min .. max] of {SAMPLES} samples, forms in turn; sets: {CLASSES} classes at density {DENSITY}, "
          f"{hot.float().sum(dim=1).mean().item():.2f} classes per row, {shared:.0f} keys per row share a class with it")
    for (label, _, ws), ts, v in zip(forms, times, values):
        show(label, ts, f"  workspace {ws / 2**20:8.1f} MiB  loss {v:.6f}")
    base = statistics.median(times[0])
    for (label, _, _), ts in zip(forms[1:], times[1:]):
        print(f"{label} / single label, medians: {statistics.median(ts) / base:.3f}", flush=True)

    # the C ABI calls alone, on buffers of their own: loss-only (statistics role + row merge) and full
    with torch.no_grad():
        q = losses.l2_normalize(za.detach())
        k = nb_all.detach()
    f32 = dict(dtype=torch.float32, device=dev)
    t = torch.tensor([0.1], **f32)
    loss_rows, dq, dk, d_t = torch.empty(rows, **f32), torch.empty(rows, d, **f32), torch.empty(cols, d, **f32), torch.empty(1, **f32)
    wsb = lib.aecf_supcon_ml_workspace_bytes(rows, cols, d)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def abi(form, grads):
        gq, gk, gt = (_ptr(dq), _ptr(dk), _ptr(d_t)) if grads else (None, None, None)
        if form == "single":
            st = lib.aecf_supcon_fwd_bwd(rows, cols, off, d, _ptr(t), MIN_T, coef, _ptr(q), _ptr(k), _ptr(lq), _ptr(lk), _ptr(loss_rows),
                                         gq, gk, gt, _ptr(ws), wsb, _stream())
        else:
            st = lib.aecf_supcon_ml_fwd_bwd(rows, cols, off, d, _ptr(t), MIN_T, coef, _ptr(q), _ptr(k), _ptr(sq), _ptr(sk), weighting[form],
                                            _ptr(loss_rows), gq, gk, gt, _ptr(ws), wsb, _stream())
        _lib.check(st, "supcon_ml_time")

    part = {(form, grads): [] for _, form, _ in forms for grads in (False, True)}
    for key in part:
        abi(*key)
    for _ in range(SAMPLES):
        for key in part:
            part[key].append(timed(lambda: abi(*key)))
    print("the C ABI calls alone (no normalise, no autograd): loss-only = statistics role + row merge; gradients = full call - loss-only")
    for label, form, _ in forms:
        lo, full = part[(form, False)], part[(form, True)]
        print(f"{label:<44} loss-only {statistics.median(lo):7.3f} ms [{min(lo):7.3f} .. {max(lo):7.3f}]   full {statistics.median(full):7.3f} ms "
              f"[{min(full):7.3f} .. {max(full):7.3f}]   gradients {statistics.median(full) - statistics.median(lo):7.3f} ms", flush=True)
    del ws, dq, dk

    print("peak device memory of one forward + backward above what is allocated before it (torch.cuda.max_memory_allocated):")
    for label, form, _ in forms:
        p, _ = peak(form)
        print(f"{label:<44} {p / 2**20:10.1f} MiB", flush=True)
    try:
        p, v = peak("torch")
        print(f"{'torch float32 (logits + Jaccard weights)':<44} {p / 2**20:10.1f} MiB  loss {v:.6f}", flush=True)
    except torch.cuda.OutOfMemoryError:
        print(f"{'torch float32 (logits + Jaccard weights)':<44} does not fit on this card: no figure", flush=True)


if __name__ == "__main__":
    main()
