"""Timing and peak memory of the tile-GEMM form of the symmetric multi-label contrastive loss on one GPU at the size of BASELINE
configs[2]: one rank's share, 8192 local rows against 65536 gathered rows, d = 768, learnable temperature, forward + backward
(normalise of the local rows, the loss, every gradient), under both weightings, against what it stands between, on the same
inputs in the same process:

  * the symmetric streaming call it replaces -- two losses._SupConMlDirection, as multilabel_contrastive(low_memory=True) runs
    them, on the same sets;
  * the single-label tile form (losses._SupConSymmetric, labels as in tools/supcon_tile_time.py) and symmetric InfoNCE on the tile
    form (losses._NceSymmetric): the same three GEMMs with a sparse label epilogue and with none.

The gathered rows of both views and the sets are made here instead of by an all-gather (they do not contain the local rows, so the
forms do the same work but do not evaluate the same number); everything after the gather is the code multilabel_contrastive runs
(its autograd functions on the normalised rows).  Sets as in tools/supcon_ml_time.py: multi-hot rows over 15 classes, each class
present with probability 0.2, packed by aecf_label_sets_pack.  A sample is the device-event time of STEPS steps; the forms are
sampled in turn (alternating, so that drift hits all alike) and the median, minimum and maximum over SAMPLES samples are printed,
then for each weighting whether the tile form's range lies wholly below the streaming form's (the condition), the ratios to the
single-label and InfoNCE tile forms (reported, not gated), torch.cuda.max_memory_allocated of one forward + backward of each above
what is allocated before the call, and a per-call breakdown of the three entry points through the C ABI (device events around
each call, median of 9) beside aecf_supcon_sym_pass1 and aecf_nce_sym_pass1_dt: the cost of the dense set epilogue.

    python tools/supcon_ml_tile_time.py [--rows 8192] [--cols 65536] [--d 768]

Per-kernel times (logits pass, weights pass, da, db) come from a kernel trace of a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/supcon_ml_tile_time.py --trace-form tile_jaccard
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
FORMS = ["tile_overlap", "tile_jaccard", "stream_overlap", "stream_jaccard", "single", "nce"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--cols", type=int, default=65536)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--trace-form", choices=FORMS, default=None,
                    help="run 8 steps of this one form and exit: the run to put under a kernel trace (per-kernel times)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("supcon_ml_tile_time: no GPU (a time from anything else says nothing)")
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
    hot = (torch.rand(cols, CLASSES, generator=g) < DENSITY).to(dev)
    sk = losses.pack_label_sets(hot)
    sq = sk[off:off + rows].clone()
    ls = torch.tensor(2.3, device=dev, requires_grad=True)
    params = [za, zb, na_all, nb_all, ls]
    coef = 0.5 / cols
    weighting = {"overlap": _lib.AECF_SETS_OVERLAP, "jaccard": _lib.AECF_SETS_JACCARD}

    def step(form):
        for p in params:
            p.grad = None
        t = (1 / ls.exp()).reshape(1)
        na = losses.l2_normalize(za)
        kind, _, w = form.partition("_")
        if kind == "tile":
            loss = losses._SupConMlSymmetric.apply(na, nb_all, sq, sk, weighting[w], off, t, coef, None, MIN_T)
        elif kind == "stream":
            nb = losses.l2_normalize(zb)
            loss = losses._SupConMlDirection.apply(na, nb_all, sq, sk, weighting[w], off, t, coef, MIN_T, True) \
                + losses._SupConMlDirection.apply(nb, na_all, sq, sk, weighting[w], off, t, coef, MIN_T, True)
        elif kind == "single":
            loss = losses._SupConSymmetric.apply(na, nb_all, lq, lk, off, t, coef, None, MIN_T)
        else:
            loss, _ = losses._NceSymmetric.apply(na, nb_all, None, off, t, coef, None, 2, 0.0, MIN_T, 1.0)
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
        print(f"supcon_ml_tile_time: 8 steps of {args.trace_form} done")
        return

    lib = _lib.load()
    tile_ws, stream_ws = lib.aecf_supcon_ml_sym_workspace_bytes(rows, cols, d), 2 * lib.aecf_supcon_ml_workspace_bytes(rows, cols, d)
    labels = {"tile_overlap": ("multi-label overlap, tile form (both directions)", tile_ws),
              "tile_jaccard": ("multi-label jaccard, tile form (both directions)", tile_ws),
              "stream_overlap": ("multi-label overlap, streaming (two directions)", stream_ws),
              "stream_jaccard": ("multi-label jaccard, streaming (two directions)", stream_ws),
              "single": ("single-label, tile form (both directions)", lib.aecf_supcon_sym_workspace_bytes(rows, cols, d)),
              "nce": ("InfoNCE, tile form (both directions)", lib.aecf_nce_sym_workspace_bytes(rows, cols, d))}
    values = {}
    for form in FORMS:
        for _ in range(WARMUP):
            loss = step(form)
        values[form] = float(loss.detach())
    times = {form: [] for form in FORMS}
    for _ in range(SAMPLES):
        for form in FORMS:
            times[form].append(sample(form))
    inter = (sq[:, None] & sk[None, :8192]) != 0
    print(f"symmetric loss of one rank, forward + backward, {rows} x {cols} x {d}, bf16, learnable T; sample = {STEPS} steps, "
          f"median [min .. max] of {SAMPLES} samples, forms in turn; sets: {CLASSES} classes at density {DENSITY}, "
          f"{hot.float().sum(dim=1).mean().item():.2f} classes per row, about {inter.float().mean().item() * cols:.0f} weighted positives per row")
    for form in FORMS:
        ts, (label, ws) = times[form], labels[form]
        print(f"{label:<50} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]  workspace {ws / 2**20:8.1f} MiB  "
              f"loss {values[form]:.6f}", flush=True)
    med = {form: statistics.median(ts) for form, ts in times.items()}
    for w in ("overlap", "jaccard"):
        print(f"{w}: streaming / tile, medians: {med['stream_' + w] / med['tile_' + w]:.3f}   "
              f"(ranges disjoint, the tile form's wholly below: {max(times['tile_' + w]) < min(times['stream_' + w])})   "
              f"tile / single-label tile: {med['tile_' + w] / med['single']:.3f}   tile / InfoNCE tile: {med['tile_' + w] / med['nce']:.3f}"
              f"   (the last two reported, not gated)", flush=True)
    print("peak device memory of one forward + backward above what is allocated before it (torch.cuda.max_memory_allocated):")
    for form in FORMS:
        print(f"{labels[form][0]:<50} {peak(form) / 2**20:10.1f} MiB", flush=True)

    # ---- per-call breakdown through the C ABI
    with torch.no_grad():
        na = losses.l2_normalize(za).detach()
    nb = nb_all.detach()
    t = torch.tensor([0.1], dtype=torch.float32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    ws = torch.empty(tile_ws, dtype=torch.uint8, device=dev)
    stats, col_sums, loss_rows = torch.empty(3, cols, **f32), torch.empty(cols, **f32), torch.empty(rows, **f32)
    da, db = torch.empty(rows, d, dtype=bf, device=dev), torch.empty(cols, d, dtype=bf, device=dev)
    d_t, up = torch.empty(1, **f32), torch.ones(1, **f32)
    nwsb = lib.aecf_nce_sym_workspace_bytes(rows, cols, d)
    nws = torch.empty(nwsb, dtype=torch.uint8, device=dev)
    s = _stream()
    calls = {}
    for w in ("overlap", "jaccard"):
        wi = weighting[w]
        calls[f"aecf_supcon_ml_sym_pass1 {w} (logits + set epilogue + sums)"] = lambda wi=wi: lib.aecf_supcon_ml_sym_pass1(
            rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(nb), _ptr(sq), _ptr(sk), wi, _ptr(ws), tile_ws, _ptr(stats), s)
        calls[f"aecf_supcon_ml_sym_loss {w}"] = lambda: lib.aecf_supcon_ml_sym_loss(
            rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(nb), _ptr(stats), _ptr(ws), tile_ws, _ptr(loss_rows), s)
        calls[f"aecf_supcon_ml_sym_grads {w} (weights + da + db)"] = lambda wi=wi: lib.aecf_supcon_ml_sym_grads(
            rows, cols, off, d, _ptr(t), MIN_T, coef, _ptr(na), _ptr(nb), _ptr(sq), _ptr(sk), wi, _ptr(ws), tile_ws, _ptr(up),
            _lib.AECF_BF16, _ptr(da), _ptr(db), _ptr(d_t), s)
    calls["aecf_supcon_sym_pass1 (logits + sparse label epilogue + sums)"] = lambda: lib.aecf_supcon_sym_pass1(
        rows, cols, off, d, _ptr(t), MIN_T, _ptr(na), _ptr(nb), _ptr(lq), _ptr(lk), _ptr(ws), tile_ws, _ptr(stats), s)
    calls["aecf_nce_sym_pass1_dt (logits + sums, no labels)"] = lambda: lib.aecf_nce_sym_pass1_dt(
        rows, cols, d, _ptr(t), MIN_T, _ptr(na), _ptr(nb), _ptr(nws), nwsb, _ptr(col_sums), s)
    spent = {k: [] for k in calls}
    for _ in range(2 + 9):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            status = call()
            e1.record()
            torch.cuda.synchronize()
            if status != 0:
                raise SystemExit(f"supcon_ml_tile_time: {name} answered {status}")
            spent[name].append(e0.elapsed_time(e1))
    print("per call through the C ABI, device events around one call, median [min .. max] of 9 after 2 warm-up rounds "
          "(the gradients calls hold the weights pass and both gradient products):")
    for name, ts in spent.items():
        ts = ts[2:]
        print(f"{name:<66} {statistics.median(ts):8.3f} ms [{min(ts):8.3f} .. {max(ts):8.3f}]", flush=True)


if __name__ == "__main__":
    main()
