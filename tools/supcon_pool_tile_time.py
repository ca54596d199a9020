"""Timing and peak memory of the tile-GEMM form of the pooled supervised contrastive loss on one GPU at the size of BASELINE
configs[2]: one rank's share, 8192 local rows against 65536 gathered rows per view, d = 768, learnable temperature, forward +
backward (normalise of the local rows of both views, the loss, every gradient), against the three things it stands between, on
the same inputs in the same process:

  * the streaming pooled loss, the form it replaces -- two losses._SupConPoolDirection over the pool [b_all | a_all] with the
    labels, as pooled_supervised_contrastive(low_memory=True) runs them (the concatenation of the pool included);
  * NT-Xent on the tile form (losses._NtXentSymmetric) -- the same three logits blocks and six products without the label work;
  * the cross-view supervised loss on the tile form (losses._SupConSymmetric) -- one block with the label work: a third of the
    MFMA flops.

The gathered rows of both views and the labels are made here instead of by an all-gather (they do not contain the local rows, so
the forms do the same work but do not evaluate the same number; partner and anchor are found by index all the same).  Labels:
classes drawn uniformly from cols / 8 classes, one row in five unlabeled, shared by both views: about 6 rows per view carry a
row's label.  A sample is the device-event time of STEPS steps; the forms are sampled in turn (alternating, so that drift hits
all alike) and the median, minimum and maximum over SAMPLES samples are printed, then torch.cuda.max_memory_allocated of one
forward + backward of each above what is allocated before the call, then a per-call breakdown through the C ABI (device events
around each call, median of 9) beside NT-Xent's and the cross-view form's calls.

    python tools/supcon_pool_tile_time.py [--rows 8192] [--cols 65536] [--d 768]

Per-kernel times come from a kernel trace of a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/supcon_pool_tile_time.py --trace-form tile
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
MIN_T = 0.025


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--cols", type=int, default=65536)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--trace-form", choices=["tile", "stream", "ntxent", "cross"], default=None,
                    help="run 8 steps of this one form and exit: the run to put under a kernel trace (per-kernel times)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("supcon_pool_tile_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    rows, cols, d = args.rows, args.cols, args.d
    off = (cols // rows // 2) * rows                  # a rank in the middle
    g = torch.Generator().manual_seed(5)
    bf = torch.bfloat16
    za = torch.randn(rows, d, generator=g).to(bf).to(dev).requires_grad_(True)
    zb = torch.randn(rows, d, generator=g).to(bf).to(dev).requires_grad_(True)
    na_all = losses.l2_normalize(torch.randn(cols, d, generator=g).to(bf).to(dev)).detach().requires_grad_(True)
    nb_all = losses.l2_normalize(torch.randn(cols, d, generator=g).to(bf).to(dev)).detach().requires_grad_(True)
    lk = torch.randint(0, max(cols // 8, 1), (cols,), generator=g)
    lk[torch.rand(cols, generator=g) < 0.2] = -1
    lk = lk.to(dev)
    lq = lk[off:off + rows].clone()
    lab_pool = torch.cat([lk, lk])
    ls = torch.tensor(2.3, device=dev, requires_grad=True)
    params = [za, zb, na_all, nb_all, ls]
    coef = 0.5 / cols

    def step(form):
        for p in params:
            p.grad = None
        t = (1 / ls.exp()).reshape(1)
        na = losses.l2_normalize(za)
        if form == "tile":
            nb = losses.l2_normalize(zb)
            loss = losses._SupConPoolSymmetric.apply(na, nb, na_all, nb_all, lq, lk, off, t, coef, None, MIN_T)
        elif form == "stream":
            nb = losses.l2_normalize(zb)
            pool = torch.cat([nb_all, na_all])
            loss = losses._SupConPoolDirection.apply(na, pool, lq, lab_pool, off, cols + off, t, coef, MIN_T, True) \
                + losses._SupConPoolDirection.apply(nb, pool, lq, lab_pool, cols + off, off, t, coef, MIN_T, True)
        elif form == "ntxent":
            nb = losses.l2_normalize(zb)
            loss = losses._NtXentSymmetric.apply(na, nb, na_all, nb_all, off, t, coef, None, MIN_T)
        else:
            loss = losses._SupConSymmetric.apply(na, nb_all, lq, lk, off, t, coef, None, MIN_T)
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

    if args.trace_form:
        for _ in range(8):
            step(args.trace_form)
        torch.cuda.synchronize()
        print(f"supcon_pool_tile_time: 8 steps of {args.trace_form} done")
        return

    lib = _lib.load()
    forms = [("pooled supervised, tile form (three blocks)", "tile", lib.aecf_supcon_pool_sym_workspace_bytes(rows, cols, d)),
             ("pooled supervised, streaming (two directions)", "stream", 2 * lib.aecf_supcon_workspace_bytes(rows, 2 * cols, d)),
             ("NT-Xent, tile form (no labels)", "ntxent", lib.aecf_ntxent_sym_workspace_bytes(rows, cols, d)),
             ("cross-view supervised, tile form (one block)", "cross", lib.aecf_supcon_sym_workspace_bytes(rows, cols, d))]
    values = []
    for _, form, _ in forms:
        for _ in range(WARMUP):
            loss = step(form)
        values.append(float(loss.detach()))
    times = [[] for _ in forms]
    for _ in range(SAMPLES):
        for i, (_, form, _) in enumerate(forms):
            times[i].append(sample(form))
    print(f"contrastive loss of one rank, forward + backward, {rows} x {cols} x {d}, bf16, learnable T; sample = {STEPS} steps, "
          f"median [min .. max] of {SAMPLES} samples, forms in turn")
    for (label, _, ws), ts, v in zip(forms, times, values):
        print(f"{label:<46} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]  workspace {ws / 2**20:8.1f} MiB  "
              f"loss {v:.6f}", flush=True)
    med = [statistics.median(ts) for ts in times]
    print(f"streaming / tile, medians: {med[1] / med[0]:.3f}   (the tile form's whole range below the streaming form's: "
          f"{max(times[0]) < min(times[1])})", flush=True)
    print(f"pooled tile / NT-Xent tile, medians: {med[0] / med[2]:.3f}   (the label search on three blocks and the label-aware "
          f"weights passes)", flush=True)
    print(f"pooled tile / cross-view tile, medians: {med[0] / med[3]:.3f}   (3 by MFMA flops)", flush=True)
    print("peak device memory of one forward + backward above what is allocated before it (torch.cuda.max_memory_allocated):")
    for label, form, _ in forms:
        print(f"{label:<46} {peak(form) / 2**20:10.1f} MiB", flush=True)

    # ---- per-call breakdown through the C ABI
    with torch.no_grad():
        na, nb = losses.l2_normalize(za).detach(), losses.l2_normalize(zb).detach()
    aa, ba = na_all.detach(), nb_all.detach()
    t = torch.tensor([0.1], dtype=torch.float32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    wsb = lib.aecf_supcon_pool_sym_workspace_bytes(rows, cols, d)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)       # the three forms run one after the other: one workspace serves
    assert wsb >= lib.aecf_ntxent_sym_workspace_bytes(rows, cols, d) and wsb >= lib.aecf_supcon_sym_workspace_bytes(rows, cols, d)
    col_stats, col_sums, loss_rows = torch.empty(3, cols, **f32), torch.empty(cols, **f32), torch.empty(rows, **f32)
    d_a, d_b = torch.empty(rows, d, dtype=bf, device=dev), torch.empty(rows, d, dtype=bf, device=dev)
    d_aa, d_ba = torch.empty(cols, d, dtype=bf, device=dev), torch.empty(cols, d, dtype=bf, device=dev)
    d_t, up = torch.empty(1, **f32), torch.ones(1, **f32)
    s = _stream()
    calls = {
        "aecf_supcon_pool_sym_pass1 (EPI_SUP + 2 EPI_SUP_SELF + sums)": lambda: lib.aecf_supcon_pool_sym_pass1(
            rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(nb), _ptr(aa), _ptr(ba), _ptr(lq), _ptr(lk), _ptr(ws), wsb, _ptr(col_stats), s),
        "aecf_supcon_pool_sym_loss": lambda: lib.aecf_supcon_pool_sym_loss(
            rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(ba), _ptr(col_stats), _ptr(ws), wsb, _ptr(loss_rows), s),
        "aecf_supcon_pool_sym_grads (3 label weights passes + 6 products)": lambda: lib.aecf_supcon_pool_sym_grads(
            rows, cols, off, d, _ptr(t), MIN_T, coef, _ptr(na), _ptr(nb), _ptr(aa), _ptr(ba), _ptr(lq), _ptr(lk), _ptr(ws), wsb, _ptr(up),
            _lib.AECF_BF16, _ptr(d_a), _ptr(d_b), _ptr(d_aa), _ptr(d_ba), _ptr(d_t), s),
        "aecf_ntxent_sym_pass1 (EPI_EXP_DT + 2 EPI_EXP_SELF + sums)": lambda: lib.aecf_ntxent_sym_pass1(
            rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(nb), _ptr(aa), _ptr(ba), _ptr(ws), wsb, _ptr(col_sums), s),
        "aecf_ntxent_sym_loss": lambda: lib.aecf_ntxent_sym_loss(
            rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(ba), _ptr(col_sums), _ptr(ws), wsb, _ptr(loss_rows), s),
        "aecf_ntxent_sym_grads (3 weights passes + 6 products)": lambda: lib.aecf_ntxent_sym_grads(
            rows, cols, off, d, _ptr(t), MIN_T, coef, _ptr(na), _ptr(nb), _ptr(aa), _ptr(ba), _ptr(ws), wsb, _ptr(up), _lib.AECF_BF16,
            _ptr(d_a), _ptr(d_b), _ptr(d_aa), _ptr(d_ba), _ptr(d_t), s),
        "aecf_supcon_sym_pass1 (EPI_SUP + sums)": lambda: lib.aecf_supcon_sym_pass1(
            rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(ba), _ptr(lq), _ptr(lk), _ptr(ws), wsb, _ptr(col_stats), s),
        "aecf_supcon_sym_loss": lambda: lib.aecf_supcon_sym_loss(
            rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(ba), _ptr(col_stats), _ptr(ws), wsb, _ptr(loss_rows), s),
        "aecf_supcon_sym_grads (label weights pass + da + db)": lambda: lib.aecf_supcon_sym_grads(
            rows, cols, off, d, _ptr(t), MIN_T, coef, _ptr(na), _ptr(ba), _ptr(lq), _ptr(lk), _ptr(ws), wsb, _ptr(up), _lib.AECF_BF16,
            _ptr(d_a), _ptr(d_ba), _ptr(d_t), s),
    }
    spent = {k: [] for k in calls}
    for _ in range(2 + 9):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            status = call()
            e1.record()
            torch.cuda.synchronize()
            if status != 0:
                raise SystemExit(f"supcon_pool_tile_time: {name} answered {status}")
            spent[name].append(e0.elapsed_time(e1))
    print("per call through the C ABI, device events around one call, median [min .. max] of 9 after 2 warm-up rounds "
          "(the gradients calls hold the weights passes and the gradient products):")
    for name, ts in spent.items():
        ts = ts[2:]
        print(f"{name:<66} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]", flush=True)


if __name__ == "__main__":
    main()
