"""Timing and peak memory of the pooled multi-label contrastive loss (tile-GEMM form, both weightings) on one GPU at the size of
BASELINE configs[2]: one rank's share, 8192 local rows against 65536 gathered rows per view, d = 768, learnable temperature,
forward + backward (normalise of the local rows of both views, the loss, every gradient), against the three forms it stands
between, on the same inputs in the same process:

  (a) the pooled supervised loss on the tile form (losses._SupConPoolSymmetric) -- the same three blocks and six products with
      one label per row: a sparse label search where this form runs a dense set sweep;
  (b) the cross-view multi-label loss on the tile form (losses._SupConMlSymmetric, both weightings) -- one block with the dense
      set sweep, rows and columns: a third of the MFMA flops;
  (c) NT-Xent on the tile form (losses._NtXentSymmetric) -- the same three blocks and six products without any label work.

The gathered rows of both views, the sets and the labels are made here instead of by an all-gather (they do not contain the local
rows, so the forms do the same work but do not evaluate the same number; partner and anchor are found by index all the same).
Sets: 15 classes, every class a member with probability 0.2, shared by both views (a row in 28 is empty; about four pairs in ten
carry a weight: dense).  Labels for (a): classes drawn uniformly from cols / 8 classes, one row in five unlabeled.  A sample is the
device-event time of STEPS steps; the forms are sampled in turn (alternating, so that drift hits all alike) and the median, minimum
and maximum over SAMPLES samples are printed, then torch.cuda.max_memory_allocated of one forward + backward of each above what is
allocated before the call, then a per-call breakdown through the C ABI (device events around each call, median of 9).

    python tools/supcon_ml_pool_tile_time.py [--rows 8192] [--cols 65536] [--d 768]

Per-kernel times come from a kernel trace of a run of its own (all forms, 4 steps each; the instantiations of the logits kernel are
told apart by their template arguments):
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/supcon_ml_pool_tile_time.py --trace
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
CLASSES, DENSITY = 15, 0.2
OV, JAC = _lib.AECF_SETS_OVERLAP, _lib.AECF_SETS_JACCARD


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--cols", type=int, default=65536)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--trace", action="store_true",
                    help="run 4 steps of every form and exit: the run to put under a kernel trace (per-kernel times)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("supcon_ml_pool_tile_time: no GPU (a time from anything else says nothing)")
    dev = torch.device("cuda:0")
    rows, cols, d = args.rows, args.cols, args.d
    off = (cols // rows // 2) * rows                  # a rank in the middle
    g = torch.Generator().manual_seed(5)
    bf = torch.bfloat16
    za = torch.randn(rows, d, generator=g).to(bf).to(dev).requires_grad_(True)
    zb = torch.randn(rows, d, generator=g).to(bf).to(dev).requires_grad_(True)
    na_all = losses.l2_normalize(torch.randn(cols, d, generator=g).to(bf).to(dev)).detach().requires_grad_(True)
    nb_all = losses.l2_normalize(torch.randn(cols, d, generator=g).to(bf).to(dev)).detach().requires_grad_(True)
    sk = losses.pack_label_sets((torch.rand(cols, CLASSES, generator=g) < DENSITY).to(dev))
    sq = sk[off:off + rows].clone()
    lk = torch.randint(0, max(cols // 8, 1), (cols,), generator=g)
    lk[torch.rand(cols, generator=g) < 0.2] = -1
    lk = lk.to(dev)
    lq = lk[off:off + rows].clone()
    ls = torch.tensor(2.3, device=dev, requires_grad=True)
    params = [za, zb, na_all, nb_all, ls]
    coef = 0.5 / cols

    def step(form):
        for p in params:
            p.grad = None
        t = (1 / ls.exp()).reshape(1)
        na = losses.l2_normalize(za)
        if form in ("pool_ov", "pool_jac"):
            nb = losses.l2_normalize(zb)
            loss = losses._SupConMlPoolSymmetric.apply(na, nb, na_all, nb_all, sq, sk, OV if form == "pool_ov" else JAC, off, t, coef,
                                                       None, MIN_T)
        elif form == "pool_label":
            nb = losses.l2_normalize(zb)
            loss = losses._SupConPoolSymmetric.apply(na, nb, na_all, nb_all, lq, lk, off, t, coef, None, MIN_T)
        elif form == "ntxent":
            nb = losses.l2_normalize(zb)
            loss = losses._NtXentSymmetric.apply(na, nb, na_all, nb_all, off, t, coef, None, MIN_T)
        else:
            loss = losses._SupConMlSymmetric.apply(na, nb_all, sq, sk, OV if form == "cross_ov" else JAC, off, t, coef, None, MIN_T)
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
    pool_ws = lib.aecf_supcon_ml_pool_sym_workspace_bytes(rows, cols, d)
    cross_ws = lib.aecf_supcon_ml_sym_workspace_bytes(rows, cols, d)
    forms = [("pooled multi-label, overlap (three blocks)", "pool_ov", pool_ws),
             ("pooled multi-label, jaccard (three blocks)", "pool_jac", pool_ws),
             ("(a) pooled supervised, one label (three blocks)", "pool_label", lib.aecf_supcon_pool_sym_workspace_bytes(rows, cols, d)),
             ("(b) cross-view multi-label, overlap (one block)", "cross_ov", cross_ws),
             ("(b) cross-view multi-label, jaccard (one block)", "cross_jac", cross_ws),
             ("(c) NT-Xent (three blocks, no labels)", "ntxent", lib.aecf_ntxent_sym_workspace_bytes(rows, cols, d))]
    if args.trace:
        for _, form, _ in forms:
            for _ in range(4):
                step(form)
        torch.cuda.synchronize()
        print("supcon_ml_pool_tile_time: 4 steps of every form done")
        return

    weighted = float((((sq[:256, None] & sk[None, :4096]) != 0).float()).mean())
    values = []
    for _, form, _ in forms:
        for _ in range(WARMUP):
            loss = step(form)
        values.append(float(loss.detach()))
    times = [[] for _ in forms]
    for _ in range(SAMPLES):
        for i, (_, form, _) in enumerate(forms):
            times[i].append(sample(form))
    print(f"contrastive loss of one rank, forward + backward, {rows} x {cols} x {d}, bf16, learnable T; sets of {CLASSES} classes at "
          f"density {DENSITY} ({weighted:.2f} of the pairs share a class); sample = {STEPS} steps, median [min .. max] of {SAMPLES} "
          f"samples, forms in turn")
    for (label, _, ws), ts, v in zip(forms, times, values):
        print(f"{label:<50} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]  workspace {ws / 2**20:8.1f} MiB  "
              f"loss {v:.6f}", flush=True)
    med = [statistics.median(ts) for ts in times]
    for k, name in ((0, "overlap"), (1, "jaccard")):
        print(f"pooled multi-label {name} / (a) pooled one-label: {med[k] / med[2]:.3f}   / (b) cross-view multi-label {name}: "
              f"{med[k] / med[3 + k]:.3f} (3 by MFMA flops)   / (c) NT-Xent: {med[k] / med[5]:.3f}", flush=True)
    print("peak device memory of one forward + backward above what is allocated before it (torch.cuda.max_memory_allocated):")
    for label, form, _ in forms:
        print(f"{label:<50} {peak(form) / 2**20:10.1f} MiB", flush=True)

    # ---- per-call breakdown through the C ABI
    with torch.no_grad():
        na, nb = losses.l2_normalize(za).detach(), losses.l2_normalize(zb).detach()
    aa, ba = na_all.detach(), nb_all.detach()
    t = torch.tensor([0.1], dtype=torch.float32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    wsb = pool_ws
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)       # the forms run one after the other: one workspace serves
    assert wsb >= lib.aecf_ntxent_sym_workspace_bytes(rows, cols, d) and wsb >= cross_ws
    col_stats, col_sums, loss_rows = torch.empty(3, cols, **f32), torch.empty(cols, **f32), torch.empty(rows, **f32)
    d_a, d_b = torch.empty(rows, d, dtype=bf, device=dev), torch.empty(rows, d, dtype=bf, device=dev)
    d_aa, d_ba = torch.empty(cols, d, dtype=bf, device=dev), torch.empty(cols, d, dtype=bf, device=dev)
    d_t, up = torch.empty(1, **f32), torch.ones(1, **f32)
    s = _stream()
    calls = {}
    for w, name in ((OV, "overlap"), (JAC, "jaccard")):
        calls[f"aecf_supcon_ml_pool_sym_pass1 {name} (EPI_SETS + 2 EPI_SETS_SELF + sums)"] = lambda w=w: lib.aecf_supcon_ml_pool_sym_pass1(
            rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(nb), _ptr(aa), _ptr(ba), _ptr(sq), _ptr(sk), w, _ptr(ws), wsb,
            _ptr(col_stats), s)
        calls[f"aecf_supcon_ml_pool_sym_loss {name}"] = lambda: lib.aecf_supcon_ml_pool_sym_loss(
            rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(ba), _ptr(col_stats), _ptr(ws), wsb, _ptr(loss_rows), s)
        calls[f"aecf_supcon_ml_pool_sym_grads {name} (3 set weights passes + 6 products)"] = lambda w=w: lib.aecf_supcon_ml_pool_sym_grads(
            rows, cols, off, d, _ptr(t), MIN_T, coef, _ptr(na), _ptr(nb), _ptr(aa), _ptr(ba), _ptr(sq), _ptr(sk), w, _ptr(ws), wsb,
            _ptr(up), _lib.AECF_BF16, _ptr(d_a), _ptr(d_b), _ptr(d_aa), _ptr(d_ba), _ptr(d_t), s)
    calls.update({
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
    })
    for w, name in ((OV, "overlap"), (JAC, "jaccard")):
        calls[f"aecf_supcon_ml_sym_pass1 {name} (EPI_SETS + sums)"] = lambda w=w: lib.aecf_supcon_ml_sym_pass1(
            rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(ba), _ptr(sq), _ptr(sk), w, _ptr(ws), wsb, _ptr(col_stats), s)
        calls[f"aecf_supcon_ml_sym_loss {name}"] = lambda: lib.aecf_supcon_ml_sym_loss(
            rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(ba), _ptr(col_stats), _ptr(ws), wsb, _ptr(loss_rows), s)
        calls[f"aecf_supcon_ml_sym_grads {name} (set weights pass + da + db)"] = lambda w=w: lib.aecf_supcon_ml_sym_grads(
            rows, cols, off, d, _ptr(t), MIN_T, coef, _ptr(na), _ptr(ba), _ptr(sq), _ptr(sk), w, _ptr(ws), wsb, _ptr(up), _lib.AECF_BF16,
            _ptr(d_a), _ptr(d_ba), _ptr(d_t), s)
    spent = {k: [] for k in calls}
    for _ in range(2 + 9):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            status = call()
            e1.record()
            torch.cuda.synchronize()
            if status != 0:
                raise SystemExit(f"supcon_ml_pool_tile_time: {name} answered {status}")
            spent[name].append(e0.elapsed_time(e1))
    print("per call through the C ABI, device events around one call, median [min .. max] of 9 after 2 warm-up rounds "
          "(the gradients calls hold the weights passes and the gradient products):")
    for name, ts in spent.items():
        ts = ts[2:]
        print(f"{name:<76} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]", flush=True)


if __name__ == "__main__":
    main()
