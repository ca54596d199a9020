"""Timing and peak memory of the pooled contrastive losses (NT-Xent, the supervised contrastive loss over both views) on one GPU at
the size of BASELINE configs[2]: one rank's share of the symmetric loss, 8192 local rows of each view against 65536 gathered
rows of each view, d = 768, learnable temperature, forward + backward (normalise of the local rows, both directions, every
gradient), against the cross-view streaming form (losses._SupConDirection twice, what supervised_contrastive(low_memory=True)
runs) on the same embeddings in the same process.

The gathered rows of both views and their labels are made here instead of by an all-gather -- the local normalised rows sit
inside them at the rank's offset, as after a gather, so the pooled forms find every anchor in the pool --; everything after the
gather is the code supervised_contrastive / nt_xent run: the concatenation of the two views into one key buffer and the two
calls of the autograd function.  Each pooled direction streams 2 x 65536 keys where a cross-view direction streams 65536.
Labels: classes drawn uniformly from cols / 8 classes, one row in five unlabeled, shared by the views (about 6 positives by
label per row in the other view, twice that in the pool).  A sample is the device-event time of STEPS steps; the forms are
sampled in turn (alternating, so that drift hits all alike) and the median, minimum and maximum over SAMPLES samples are
printed.  Then torch.cuda.max_memory_allocated of one forward + backward of each, above what is allocated before the call,
beside a torch float32 evaluation of the pooled supervised loss (two rows x 2 cols blocks of logits and match masks) where that
fits on the card.  Last, the C calls alone on the same rows, so that the ratio can be taken apart: aecf_supcon_fwd_bwd against
cols keys, the same call against the pool's 2 cols keys (what doubling the keys costs), and aecf_supcon_pool_fwd_bwd against the
pool (what the exclusion costs beside it); the rest of the ratio is the autograd graph around the calls.

    python tools/supcon_pool_time.py [--rows 8192] [--cols 65536] [--d 768]
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
        raise SystemExit("supcon_pool_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    rows, cols, d = args.rows, args.cols, args.d
    off = (cols // rows // 2) * rows                  # a rank in the middle
    g = torch.Generator().manual_seed(5)
    unit = lambda n: losses.l2_normalize(torch.randn(n, d, generator=g).to(torch.bfloat16).to(dev)).detach()
    za = torch.randn(rows, d, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    zb = torch.randn(rows, d, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    # the other ranks' rows of each view, before and after this rank's (leaves: their gradient is the gather's backward input)
    others = [unit(n).requires_grad_(True) for n in (off, cols - off - rows, off, cols - off - rows)]
    lab_all = torch.randint(0, max(cols // 8, 1), (cols,), generator=g)
    lab_all[torch.rand(cols, generator=g) < 0.2] = -1
    lab_all = lab_all.to(dev)
    lab = lab_all[off:off + rows].clone()
    none_all, none = torch.full_like(lab_all, -1), torch.full_like(lab, -1)
    lab_pool, none_pool = torch.cat([lab_all, lab_all]), torch.cat([none_all, none_all])
    ls = torch.tensor(2.3, device=dev, requires_grad=True)
    params = [za, zb, ls] + others
    coef = 0.5 / cols

    def step(form):
        for p in params:
            p.grad = None
        t = (1 / ls.exp()).reshape(1)
        na, nb = losses.l2_normalize(za), losses.l2_normalize(zb)
        na_all, nb_all = torch.cat([others[0], na, others[1]]), torch.cat([others[2], nb, others[3]])
        if form == "cross":
            loss = (losses._SupConDirection.apply(na, nb_all, lab, lab_all, off, t, coef, MIN_T, True)
                    + losses._SupConDirection.apply(nb, na_all, lab, lab_all, off, t, coef, MIN_T, True))
        elif form in ("pool", "nt_xent"):
            lq, lk = (lab, lab_pool) if form == "pool" else (none, none_pool)
            pool = torch.cat([nb_all, na_all])
            loss = (losses._SupConPoolDirection.apply(na, pool, lq, lk, off, cols + off, t, coef, MIN_T, True)
                    + losses._SupConPoolDirection.apply(nb, pool, lq, lk, cols + off, off, t, coef, MIN_T, True))
        else:                                         # torch, float32: the rows x 2 cols logits and the match masks
            pool = torch.cat([nb_all, na_all]).float()
            i = torch.arange(rows, device=dev)
            loss = 0.0
            for q, partner, own in ((na, off, cols + off), (nb, cols + off, off)):
                x = (q.float() @ pool.T) / t.clamp_min(MIN_T)
                match = (lab[:, None] >= 0) & (lab[:, None] == lab_pool[None, :])
                match[i, partner + i] = True
                match[i, own + i] = False
                x = x.index_put((i, own + i), torch.tensor(float("-inf"), device=dev))
                loss = loss + (torch.logsumexp(x, dim=1) - torch.where(match, x, 0.0).sum(dim=1) / match.sum(dim=1)).sum() * coef
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
    forms = [("cross-view supervised (streaming)", "cross", 2 * lib.aecf_supcon_workspace_bytes(rows, cols, d)),
             ("NT-Xent (pool of both views)", "nt_xent", 2 * lib.aecf_supcon_workspace_bytes(rows, 2 * cols, d)),
             ("supervised, intra_view=True (pool)", "pool", 2 * lib.aecf_supcon_workspace_bytes(rows, 2 * cols, d))]
    values = []
    for _, form, _ in forms:
        for _ in range(WARMUP):
            loss = step(form)
        values.append(float(loss.detach()))
    times = [[] for _ in forms]
    for _ in range(SAMPLES):
        for i, (_, form, _) in enumerate(forms):
            times[i].append(sample(form))
    n_pos = ((lab[:, None] >= 0) & (lab[:, None] == lab_all[None, :])).sum(dim=1).float().mean().item() if rows * cols <= 2 ** 30 else None
    print(f"the symmetric loss (both directions), forward + backward, {rows} local x {cols} gathered rows per view x {d}, bf16, "
          f"learnable T; sample = {STEPS} steps, median [min .. max] of {SAMPLES} samples, forms in turn"
          + (f"; {n_pos:.2f} rows of a view carry a row's label on average" if n_pos is not None else ""))
    for (label, _, ws), ts, v in zip(forms, times, values):
        print(f"{label:<38} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]  workspace {ws / 2**20:8.1f} MiB  "
              f"loss {v:.6f}", flush=True)
    base = statistics.median(times[0])
    for (label, _, _), ts in zip(forms[1:], times[1:]):
        print(f"{label} / cross-view, medians: {statistics.median(ts) / base:.3f}", flush=True)
    print("peak device memory of one forward + backward above what is allocated before it (torch.cuda.max_memory_allocated):")
    for label, form, _ in forms:
        p, _ = peak(form)
        print(f"{label:<38} {p / 2**20:10.1f} MiB", flush=True)
    try:
        p, v = peak("torch")
        print(f"{'torch float32 (pool logits + masks)':<38} {p / 2**20:10.1f} MiB  loss {v:.6f}", flush=True)
    except torch.cuda.OutOfMemoryError:
        print(f"{'torch float32 (pool logits + masks)':<38} does not fit on this card: no figure", flush=True)

    # ---- the calls alone
    from aecf_amd.layer import _ptr, _stream
    with torch.no_grad():
        q = losses.l2_normalize(za.detach())
        pool = torch.cat([torch.cat([others[2], losses.l2_normalize(zb.detach()), others[3]]), torch.cat([others[0], q, others[1]])]).contiguous()
    f32 = dict(dtype=torch.float32, device=dev)
    loss_rows, dq, dk, d_t = torch.empty(rows, **f32), torch.empty(rows, d, **f32), torch.empty(2 * cols, d, **f32), torch.empty(1, **f32)
    ws_bytes = lib.aecf_supcon_workspace_bytes(rows, 2 * cols, d)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    t = torch.tensor([1 / 2.3 ** 2], **f32)

    def call(form):
        if form == "plain":
            st = lib.aecf_supcon_fwd_bwd(rows, cols, off, d, _ptr(t), MIN_T, coef, _ptr(q), _ptr(pool), _ptr(lab), _ptr(lab_pool),
                                         _ptr(loss_rows), _ptr(dq), _ptr(dk), _ptr(d_t), _ptr(ws), ws_bytes, _stream())
        elif form == "plain2":
            st = lib.aecf_supcon_fwd_bwd(rows, 2 * cols, off, d, _ptr(t), MIN_T, coef, _ptr(q), _ptr(pool), _ptr(lab), _ptr(lab_pool),
                                         _ptr(loss_rows), _ptr(dq), _ptr(dk), _ptr(d_t), _ptr(ws), ws_bytes, _stream())
        else:
            st = lib.aecf_supcon_pool_fwd_bwd(rows, 2 * cols, off, cols + off, d, _ptr(t), MIN_T, coef, _ptr(q), _ptr(pool), _ptr(lab),
                                              _ptr(lab_pool), _ptr(loss_rows), _ptr(dq), _ptr(dk), _ptr(d_t), _ptr(ws), ws_bytes, _stream())
        _lib.check(st, "supcon_pool_time")

    def sample_call(form):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            call(form)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / STEPS

    calls = [(f"aecf_supcon_fwd_bwd, {cols} keys", "plain"), (f"aecf_supcon_fwd_bwd, {2 * cols} keys", "plain2"),
             (f"aecf_supcon_pool_fwd_bwd, {2 * cols} keys", "pool")]
    for _, form in calls:
        for _ in range(WARMUP):
            call(form)
    ctimes = [[] for _ in calls]
    for _ in range(SAMPLES):
        for i, (_, form) in enumerate(calls):
            ctimes[i].append(sample_call(form))
    print(f"one direction, the C call alone (statistics, dq, dk, dT), {rows} rows, same samples and order:")
    for (label, _), ts in zip(calls, ctimes):
        print(f"{label:<42} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]", flush=True)
    m = [statistics.median(ts) for ts in ctimes]
    print(f"twice the keys: {m[1] / m[0]:.3f}; the exclusion beside it: {m[2] / m[1]:.3f}; pooled call / cross-view call: {m[2] / m[0]:.3f}",
          flush=True)


if __name__ == "__main__":
    main()
