"""Timing and peak memory of the streaming supervised contrastive loss on one GPU at the size of BASELINE configs[2]: one rank's
share of one direction of losses.supervised_contrastive, 8192 local rows against 65536 gathered rows, d = 768, learnable
temperature, forward + backward (normalise of the local rows, the loss, every gradient), against streaming InfoNCE
(losses._NceDirection(..., low_memory=True)) on the same inputs in the same process.

The gathered rows of the other view and their labels are made here instead of by an all-gather; everything after the gather is
the code supervised_contrastive runs (its autograd function on the normalised rows).  Labels: classes drawn uniformly from
cols / 8 classes (about 8 keys per class), one row in five unlabeled.  A sample is the device-event time of STEPS steps; the two
losses are sampled in turn (alternating, so that drift hits both alike) and the median, minimum and maximum over SAMPLES samples
are printed.  Then torch.cuda.max_memory_allocated of one forward + backward of each, above what is allocated before the call,
beside a torch float32 evaluation of the same loss (rows x cols logits and match mask) where that fits on the card.

    python tools/supcon_time.py [--rows 8192] [--cols 65536] [--d 768]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aecf_amd import _lib, losses  # noqa: E402

STEPS, SAMPLES, WARMUP = 5, 9, 3
MIN_T = 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--cols", type=int, default=65536)
    ap.add_argument("--d", type=int, default=768)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("supcon_time: no GPU (a time from anything else says nothing)")
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
    ls = torch.tensor(2.3, device=dev, requires_grad=True)
    params = [za, nb_all, ls]
    coef = 1.0 / cols

    def step(form):
        for p in params:
            p.grad = None
        t = (1 / ls.exp()).reshape(1)
        na = losses.l2_normalize(za)
        if form == "supcon":
            loss = losses._SupConDirection.apply(na, nb_all, lq, lk, off, t, coef, MIN_T, True)
        elif form == "info_nce":
            loss = losses._NceDirection.apply(na, nb_all, off, t, coef, True, MIN_T)
        else:                                         # torch, float32: the rows x cols logits and the match mask
            x = (na.float() @ nb_all.float().T) / t.clamp_min(MIN_T)
            i = torch.arange(rows, device=dev)
            match = (lq[:, None] >= 0) & (lq[:, None] == lk[None, :])
            match[i, off + i] = True
            loss = (torch.logsumexp(x, dim=1) - (x * match).sum(dim=1) / match.sum(dim=1)).sum() * coef
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
        loss = step(form)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, float(loss.detach())

    lib = _lib.load()
    forms = [("supervised contrastive (streaming)", "supcon", lib.aecf_supcon_workspace_bytes(rows, cols, d)),
             ("InfoNCE low_memory=True (streaming)", "info_nce", lib.aecf_nce_stream_workspace_bytes(rows, cols, d, _lib.AECF_BF16))]
    values = []
    for _, form, _ in forms:
        for _ in range(WARMUP):
            loss = step(form)
        values.append(float(loss.detach()))
    times = [[] for _ in forms]
    for _ in range(SAMPLES):
        for i, (_, form, _) in enumerate(forms):
            times[i].append(sample(form))
    n_pos = ((lq[:, None] >= 0) & (lq[:, None] == lk[None, :])).sum(dim=1).float().mean().item() if rows * cols <= 2 ** 30 else None
    print(f"one direction, forward + backward, {rows} x {cols} x {d}, bf16, learnable T; sample = {STEPS} steps, "
          f"median [min .. max] of {SAMPLES} samples, losses in turn"
          + (f"; {n_pos:.2f} positives by label per row on average" if n_pos is not None else ""))
    for (label, _, ws), ts, v in zip(forms, times, values):
        print(f"{label:<38} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]  workspace {ws / 2**20:8.1f} MiB  "
              f"loss {v:.6f}", flush=True)
    print(f"supervised contrastive / InfoNCE, medians: {statistics.median(times[0]) / statistics.median(times[1]):.3f}", flush=True)
    print("peak device memory of one forward + backward above what is allocated before it (torch.cuda.max_memory_allocated):")
    for label, form in (("supervised contrastive (streaming)", "supcon"), ("InfoNCE low_memory=True (streaming)", "info_nce")):
        p, _ = peak(form)
        print(f"{label:<38} {p / 2**20:10.1f} MiB", flush=True)
    try:
        p, v = peak("torch")
        print(f"{'torch float32 (logits + match mask)':<38} {p / 2**20:10.1f} MiB  loss {v:.6f}", flush=True)
    except torch.cuda.OutOfMemoryError:
        print(f"{'torch float32 (logits + match mask)':<38} does not fit on this card: no figure", flush=True)


if __name__ == "__main__":
    main()
