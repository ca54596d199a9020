"""Runnable counterpart of the reference's example trainer around the fusion path (behaviour
of ``train_both_models`` / ``main`` in ``xrays/train_xrays_example.py:312-427, 736-783`` for the AECF model): AdamW
(lr 1e-4, weight decay 0.01) + BCEWithLogits, curriculum masking and missing-modality training switched on at epoch 40 of
60, per-epoch validation mAP with and without each modality -- data-parallel over the GPUs of one node.

    python -m aecf_amd.train_xray --epochs 60 --switch-epoch 40                     # one GPU
    python -m torch.distributed.run --nproc-per-node 4 --master-addr 127.0.0.1 -m aecf_amd.train_xray   # DP x 4
    python -m aecf_amd.train_xray --param-dtype bfloat16 --max-grad-norm 1.0        # bf16 model, float32 masters, clipping
    python -m aecf_amd.train_xray --ema-decay 0.999                                 # + validation of the averaged weights
    python -m aecf_amd.train_xray --full-metrics                                    # + tie-exact mAP, AUROC, macro F1, all ranks
    python -m aecf_amd.train_xray --loss asymmetric --pos-weight auto               # the library's multi-label loss, class balance
    python -m aecf_amd.train_xray --calibration --calibrate temperature             # + ECE, Brier, NLL; a temperature fit at the end
    python -m aecf_amd.train_xray --param-dtype bfloat16 --fused-head               # classifier[3] + loss in one call, no logits
    python -m aecf_amd.train_xray --bootstrap 1000                                  # + 95 % intervals and paired differences at the end

The reference trains on precomputed CLIP features of a chest X-ray set that is not part of its repository
(``.MISSING_LARGE_BLOBS``); ``--data train.pt,val.pt`` loads such files (dicts with image / text / labels), otherwise a
synthetic set of the same shape is generated (CLIP-like 512-d features whose label signal is split between the
modalities, so that the fusion has something to learn).  Plots and the baseline model of the reference script are
reporting code outside the path and are not rebuilt; its sklearn metrics (``calculate_metrics``, ref :260-295) are served by
``--full-metrics`` through ``aecf_amd.metrics.multilabel_metrics``, every rank evaluating its shard of the validation set.
``--loss`` / ``--pos-weight auto`` replace the torch criterion (ref :327, 366, 374) by ``aecf_amd.losses.MultilabelLoss`` on the
logits as the model leaves them; with neither flag the torch ``BCEWithLogitsLoss`` line runs as before.  ``--fused-head`` (needs
``--param-dtype bfloat16``, implies ``--loss bce`` if none is given) trains through ``aecf_amd.losses.MultilabelHead`` sharing
``classifier[3]``'s parameters: the model hands over that layer's input and no training logits exist; validation keeps using the
logits.  ``--calibration``
adds the pooled ECE, Brier score and NLL of the three modality plans to every epoch's row (``aecf_amd.metrics.
multilabel_calibration``, every rank on its shard); ``--calibrate MODE`` fits a scaling on the validation logits with all
modalities present after the last epoch (``fit_calibration``) and reports the three plans' ECE and NLL before and after it.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch
import torch.distributed as dist

from . import dp
from .losses import MLHEAD_WIDTHS, MultilabelHead, MultilabelLoss, class_balance_weights
from .metrics import bootstrap_compare, fit_calibration, multilabel_calibration, multilabel_metrics
from .optim import EmaModel, FusedAdamW
from .xray import AECFModel


def synthetic_split(n: int, num_classes: int, dim: int, seed: int, device, proto_seed: int = 1234):
    gp = torch.Generator().manual_seed(proto_seed)        # the class prototypes are the "world": same for every split
    proto_img = torch.randn(num_classes, dim, generator=gp)
    proto_txt = torch.randn(num_classes, dim, generator=gp)
    g = torch.Generator().manual_seed(seed)
    labels = (torch.rand(n, num_classes, generator=g) < 0.2).float()
    half = num_classes // 2                       # the first classes show in the image, the rest in the text
    li, lt = labels.clone(), labels.clone()
    li[:, half:] *= 0.25
    lt[:, :half] *= 0.25
    image = li @ proto_img + 1.5 * torch.randn(n, dim, generator=g)
    text = lt @ proto_txt + 1.5 * torch.randn(n, dim, generator=g)
    return image.to(device), text.to(device), labels.to(device)


def mean_average_precision(scores: torch.Tensor, labels: torch.Tensor) -> float:
    """Macro average precision over the classes that have a positive (what sklearn's average_precision_score computes
    per class, ref xrays/train_xrays_example.py:260-295), on the device."""
    order = scores.argsort(dim=0, descending=True)
    hit = labels.gather(0, order)
    tp = hit.cumsum(0)
    prec = tp / torch.arange(1, scores.shape[0] + 1, device=scores.device, dtype=scores.dtype).unsqueeze(1)
    npos = labels.sum(0)
    ap = (prec * hit).sum(0) / npos.clamp_min(1.0)
    keep = npos > 0
    return float(ap[keep].mean()) if bool(keep.any()) else 0.0


@torch.no_grad()
def evaluate(model: AECFModel, image, text, labels, drop: str, batch: int = 4096) -> float:
    model.eval()
    outs = []
    for i in range(0, image.shape[0], batch):
        im, tx = image[i:i + batch], text[i:i + batch]
        if drop == "images":
            im = torch.zeros_like(im)
        elif drop == "texts":
            tx = torch.zeros_like(tx)
        outs.append(model(im, tx).float())
    return mean_average_precision(torch.cat(outs), labels)


@torch.no_grad()
def evaluate_full(model: AECFModel, image, text, labels, drop: str, rank: int, world: int, batch: int = 4096) -> dict:
    """Tie-exact mAP, macro AUROC and macro F1 of the whole validation set (aecf_amd.metrics.multilabel_metrics): this rank
    runs the model on its ``dp.shard_bounds`` rows and the ranks join their logits inside the call, so every rank must make
    it.  The logits are scored in the model's dtype, as they are."""
    model.eval()
    lo, hi = dp.shard_bounds(image.shape[0], rank, world)
    outs = []
    for i in range(lo, hi, batch):
        im, tx = image[i:min(i + batch, hi)], text[i:min(i + batch, hi)]
        if drop == "images":
            im = torch.zeros_like(im)
        elif drop == "texts":
            tx = torch.zeros_like(tx)
        outs.append(model(im, tx))
    logits = torch.cat(outs) if outs else torch.empty(0, labels.shape[1], dtype=next(model.parameters()).dtype, device=image.device)
    m = multilabel_metrics(logits, labels[lo:hi], group=dist.group.WORLD if world > 1 else None)
    return dict(val_map_exact=m["map"], val_auroc=m["macro_auroc"], val_macro_f1=m["macro_f1"])


def _full_metric_rows(prefix: str, model: AECFModel, image, text, labels, rank: int, world: int) -> dict:
    row = {}
    for drop, suffix in (("none", ""), ("images", "_no_images"), ("texts", "_no_texts")):
        for name, value in evaluate_full(model, image, text, labels, drop, rank, world).items():
            row[prefix + name + suffix] = float(value) if rank == 0 else None
    return row


PLANS = (("none", ""), ("images", "_no_images"), ("texts", "_no_texts"))


@torch.no_grad()
def shard_logits(model: AECFModel, image, text, labels, drop: str, rank: int, world: int, batch: int = 4096):
    """this rank's ``dp.shard_bounds`` rows of the validation set through the model: (logits in the model's dtype, labels)"""
    model.eval()
    lo, hi = dp.shard_bounds(image.shape[0], rank, world)
    outs = []
    for i in range(lo, hi, batch):
        im, tx = image[i:min(i + batch, hi)], text[i:min(i + batch, hi)]
        if drop == "images":
            im = torch.zeros_like(im)
        elif drop == "texts":
            tx = torch.zeros_like(tx)
        outs.append(model(im, tx))
    logits = torch.cat(outs) if outs else torch.empty(0, labels.shape[1], dtype=next(model.parameters()).dtype, device=image.device)
    return logits, labels[lo:hi]


def _calibration_rows(prefix: str, model: AECFModel, image, text, labels, rank: int, world: int, scale=None, bias=None,
                      names=("ece", "brier", "nll"), tag: str = "") -> dict:
    """pooled calibration values of the three modality plans, a collective: every rank scores its shard"""
    row = {}
    group = dist.group.WORLD if world > 1 else None
    for drop, suffix in PLANS:
        logits, y = shard_logits(model, image, text, labels, drop, rank, world)
        m = multilabel_calibration(logits, y, scale=scale, bias=bias, group=group)
        for name in names:
            row[f"{prefix}val_{name}{tag}{suffix}"] = float(m[name]) if rank == 0 else None
    return row


BOOT_SCORES = (("map", "map"), ("macro_auroc", "auroc"), ("macro_f1", "macro_f1"))      # bootstrap_metrics' name, the row's


def _bootstrap_row(model: AECFModel, image, text, labels, rank: int, world: int, n_boot: int, seed: int) -> dict:
    """Point value and 95 % interval of mAP, macro AUROC and macro F1 for the three modality plans, and the PAIRED differences
    full - no_images and full - no_texts (aecf_amd.metrics.bootstrap_compare: the same resampled rows on both sides) with
    the share of resamples at or below zero.  A collective: every rank scores its shard."""
    group = dist.group.WORLD if world > 1 else None
    logits = {}
    for drop, _ in PLANS:
        logits[drop], y = shard_logits(model, image, text, labels, drop, rank, world)
    row = dict(bootstrap=n_boot, bootstrap_seed=seed)
    val = lambda t: float(t) if rank == 0 else None
    for drop, suffix in PLANS[1:]:
        cmp = bootstrap_compare(logits["none"], logits[drop], y, n_boot=n_boot, seed=seed, group=group)
        for (name, short), (side, sfx) in ((s, p) for s in BOOT_SCORES for p in (("a", ""), ("b", suffix))):
            m = cmp[side]
            row[f"val_{short}{sfx}"] = val(m[name])
            row[f"val_{short}{sfx}_ci"] = [val(m[name + "_ci"][0]), val(m[name + "_ci"][1])]
        for name, short in BOOT_SCORES:
            row[f"val_{short}_minus{suffix}"] = val(cmp[name])
            row[f"val_{short}_minus{suffix}_ci"] = [val(cmp[name + "_ci"][0]), val(cmp[name + "_ci"][1])]
            row[f"val_{short}_minus{suffix}_p_le0"] = val(cmp[name + "_p_le0"])
    return row


LOSS_FORMS = {"bce": (0.0, 0.0, 0.0), "focal": (2.0, 2.0, 0.0), "asymmetric": (0.0, 4.0, 0.05)}     # gamma+, gamma-, margin


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--switch-epoch", type=int, default=40, help="curriculum masking + missing-modality training from here")
    ap.add_argument("--batch", type=int, default=64, help="GLOBAL batch per step (the reference's 64), sharded over the ranks")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--samples", type=int, default=8192)
    ap.add_argument("--val-samples", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=15)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--data", default=None, help="train.pt,val.pt with image/text/labels tensors (default: synthetic)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default=None, help="state_dict file written by rank 0 at the end (ref :766-772)")
    ap.add_argument("--param-dtype", choices=("float32", "bfloat16"), default="float32",
                    help="bfloat16: the model and its inputs in bf16, FusedAdamW keeps float32 master weights and moments")
    ap.add_argument("--max-grad-norm", type=float, default=None, help="clip the global gradient norm inside the optimiser step")
    ap.add_argument("--ema-decay", type=float, default=None,
                    help="keep an exponential moving average of the weights inside the optimiser step and validate it too")
    ap.add_argument("--full-metrics", action="store_true",
                    help="also report tie-exact mAP, macro AUROC and macro F1 (val_map_exact, val_auroc, val_macro_f1 and their "
                         "_no_images / _no_texts / ema_ forms), evaluated by every rank on its shard of the validation set")
    ap.add_argument("--loss", choices=tuple(LOSS_FORMS), default=None,
                    help="the library's multi-label loss on the logits as they are: bce, focal (gamma 2) or asymmetric "
                         "(gamma- 4, margin 0.05); unknown labels (NaN or < 0) are left out.  Default: torch's BCEWithLogitsLoss")
    ap.add_argument("--pos-weight", choices=("auto",), default=None,
                    help="auto: per-class n_neg / n_pos of the training labels as pos_weight (implies --loss bce if none is given)")
    ap.add_argument("--fused-head", action="store_true",
                    help="train classifier[3] and the loss as one fused call on the layer's input (losses.MultilabelHead): no "
                         "training logits exist.  Needs --param-dtype bfloat16; implies --loss bce if none is given")
    ap.add_argument("--calibration", action="store_true",
                    help="also report the pooled ECE (15 bins), Brier score and NLL of the validation logits (val_ece, val_brier, "
                         "val_nll and their _no_images / _no_texts forms), evaluated by every rank on its shard")
    ap.add_argument("--calibrate", choices=("temperature", "class_temperature", "platt"), default=None,
                    help="after the last epoch fit this scaling on the validation logits with all modalities present and report "
                         "the three plans' ECE and NLL before and after it, and the fitted temperature")
    ap.add_argument("--bootstrap", type=int, default=0, metavar="R",
                    help="after the last epoch report 95 %% percentile-bootstrap intervals (R resamples of the validation rows) of "
                         "mAP, macro AUROC and macro F1 for the three modality plans, and the paired differences full - no_images "
                         "and full - no_texts with their intervals; evaluated by every rank on its shard")
    ap.add_argument("--bootstrap-seed", type=int, default=0, help="seed of the resamples (the same rows for every plan)")
    args = ap.parse_args(argv)
    if args.bootstrap < 0:
        ap.error("--bootstrap takes a number of resamples >= 1 (0: off)")
    if args.fused_head:
        if args.param_dtype != "bfloat16":
            ap.error("--fused-head needs --param-dtype bfloat16 (the fused head serves bfloat16 features and weights)")
        if args.hidden not in MLHEAD_WIDTHS:
            ap.error(f"--fused-head needs --hidden in {MLHEAD_WIDTHS}")
        args.loss = args.loss or "bce"

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dev_index = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        backend = os.environ.get("AECF_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)

    if args.data:
        tr, va = (torch.load(p, map_location=device) for p in args.data.split(","))
        image, text, labels = tr["image"].float(), tr["text"].float(), tr["labels"].float()
        v_image, v_text, v_labels = va["image"].float(), va["text"].float(), va["labels"].float()
        args.classes = labels.shape[1]
    else:
        image, text, labels = synthetic_split(args.samples, args.classes, 512, args.seed + 1, device)
        v_image, v_text, v_labels = synthetic_split(args.val_samples, args.classes, 512, args.seed + 2, device)

    low = args.param_dtype == "bfloat16"
    if low:
        image, text, v_image, v_text = (t.bfloat16() for t in (image, text, v_image, v_text))
    torch.manual_seed(args.seed + 17 * rank)                       # replicas differ until the broadcast below
    model = AECFModel(image.shape[1], text.shape[1], args.classes, args.hidden).to(device)
    if low:
        model = model.bfloat16()
    params = list(model.parameters())
    dp.broadcast_parameters(params + list(model.buffers()))
    bucket = dp.FlatGradBucket(params) if world > 1 else None
    opt = FusedAdamW(params, lr=args.lr, weight_decay=0.01,                 # ref :322-323 (torch.optim.AdamW's update, one launch)
                     master_weights=low, max_grad_norm=args.max_grad_norm, ema_decay=args.ema_decay)
    ema = EmaModel(model, opt) if args.ema_decay is not None else None      # (every rank keeps the same averages)
    fused_loss = args.loss is not None or args.pos_weight is not None
    if fused_loss:
        gamma_pos, gamma_neg, margin = LOSS_FORMS[args.loss or "bce"]
        crit = MultilabelLoss(pos_weight=class_balance_weights(labels) if args.pos_weight == "auto" else None,
                              gamma_pos=gamma_pos, gamma_neg=gamma_neg, margin=margin,
                              group=dist.group.WORLD if world > 1 else None)     # the global mean over the valid labels of all ranks
        head = None
        if args.fused_head:                 # the same options on the layer's own parameter objects
            head = MultilabelHead.from_linear(model.classifier[3], pos_weight=crit.pos_weight, gamma_pos=gamma_pos,
                                              gamma_neg=gamma_neg, margin=margin, group=crit.group)
    else:
        crit, head = torch.nn.BCEWithLogitsLoss(), None
    n = image.shape[0]
    steps = (n + args.batch - 1) // args.batch                              # the short last batch is kept (DataLoader default)
    perm_gen = torch.Generator(device=device).manual_seed(args.seed + 3)    # same permutation on every rank
    mask_gen = torch.Generator(device=device).manual_seed(args.seed + 4)    # same global mask uniforms on every rank
    miss_gen = torch.Generator(device=device).manual_seed(args.seed + 5)    # same global missing-modality draws on every rank
    history = []
    for epoch in range(args.epochs):
        if epoch == args.switch_epoch:                                      # ref :346-349
            model.toggle_curriculum(True)
            model.missing_modality_training = True
        model.train()
        perm = torch.randperm(n, device=device, generator=perm_gen)
        t0 = time.perf_counter()
        loss_sum = torch.zeros((), device=device)
        ent_sum = torch.zeros((), device=device)
        for it in range(steps):
            idx = perm[it * args.batch:(it + 1) * args.batch]
            b = idx.numel()                                                 # < args.batch in the last step of an epoch
            lo, hi = dp.shard_bounds(b, rank, world)
            sel = idx[lo:hi]
            u = torch.rand(b, 1, 2, device=device, generator=mask_gen)[lo:hi]       # (every rank draws: the streams stay aligned)
            missing = None
            if model.missing_modality_training:
                da, db = model.draw_missing(b, device, generator=miss_gen)  # the GLOBAL batch's draws; this rank's rows
                missing = (da[lo:hi], db[lo:hi])
            if hi <= lo:                                # fewer rows than ranks: this rank only joins the collective
                if head is not None:
                    loss_sum += head.loss(torch.empty(0, args.hidden, dtype=params[0].dtype, device=device), labels[sel]).detach()
                elif fused_loss:                        # (the loss's all-reduce first, as on the ranks that hold rows)
                    loss_sum += crit(torch.empty(0, args.classes, dtype=params[0].dtype, device=device), labels[sel])
                bucket.zero()
                bucket.all_reduce(average=True)
                opt.step()
                continue
            if head is not None:
                hidden, info = model(image[sel], text[sel], return_info=True, mask_uniforms=u, missing=missing, return_hidden=True)
                loss = head.loss(hidden, labels[sel])
            else:
                logits, info = model(image[sel], text[sel], return_info=True, mask_uniforms=u, missing=missing)
                loss = crit(logits, labels[sel]) if fused_loss else crit(logits.float(), labels[sel])
            if bucket is None:
                opt.zero_grad(set_to_none=True)
            else:
                bucket.zero()
            if fused_loss and world > 1:                # already the global loss, its gradient scaled for the averaging bucket
                loss.backward()
            else:
                (loss * dp.shard_loss_scale(hi - lo, b, world)).backward()
            if bucket is not None:
                bucket.all_reduce(average=True)
            opt.step()
            loss_sum += loss.detach()
            if "entropy" in info:
                ent_sum += info["entropy"].float().mean()
        row = dict(epoch=epoch + 1, curriculum=model.curriculum_enabled,
                   train_loss=float(dp.all_reduce_mean_scalar(loss_sum / steps)),
                   gate_entropy=float(dp.all_reduce_mean_scalar(ent_sum / steps)),
                   sec=time.perf_counter() - t0)
        if rank == 0:
            row.update(val_map=evaluate(model, v_image, v_text, v_labels, "none"),
                       val_map_no_images=evaluate(model, v_image, v_text, v_labels, "images"),
                       val_map_no_texts=evaluate(model, v_image, v_text, v_labels, "texts"))
            if ema is not None:
                ema.sync()
                row.update(ema_val_map=evaluate(ema.module, v_image, v_text, v_labels, "none"),
                           ema_val_map_no_images=evaluate(ema.module, v_image, v_text, v_labels, "images"),
                           ema_val_map_no_texts=evaluate(ema.module, v_image, v_text, v_labels, "texts"))
        if args.full_metrics:                                               # a collective evaluation: every rank takes part
            full = _full_metric_rows("", model, v_image, v_text, v_labels, rank, world)
            if ema is not None:
                ema.sync()
                full.update(_full_metric_rows("ema_", ema.module, v_image, v_text, v_labels, rank, world))
            if rank == 0:
                row.update(full)
        if args.calibration:                                                # collective as well
            cal = _calibration_rows("", model, v_image, v_text, v_labels, rank, world)
            if rank == 0:
                row.update(cal)
        if rank == 0:
            print(json.dumps(row), flush=True)
        history.append(row)
        if world > 1:
            dist.barrier()
    if args.calibrate:                                                      # post-hoc calibration: fit once, score the three plans
        logits, y = shard_logits(model, v_image, v_text, v_labels, "none", rank, world)
        fit = fit_calibration(logits, y, mode=args.calibrate, group=dist.group.WORLD if world > 1 else None)
        row = dict(calibrate=args.calibrate)
        row.update(_calibration_rows("", model, v_image, v_text, v_labels, rank, world, names=("ece", "nll")))
        row.update(_calibration_rows("", model, v_image, v_text, v_labels, rank, world, scale=fit["scale"], bias=fit["bias"],
                                     names=("ece", "nll"), tag="_calibrated"))
        if rank == 0:
            row.update(temperature=[float(v) for v in fit["temperature"]], bias=[float(v) for v in fit["bias"]],
                       fitted=[bool(v) for v in fit["fitted"]], converged=[bool(v) for v in fit["converged"]])
            print(json.dumps(row), flush=True)
            if args.calibrate == "temperature":
                print(f"fitted temperature T = {row['temperature'][0]:.6f}", flush=True)
        history.append(row)
    if args.bootstrap:                                                      # collective: every rank scores its shard
        row = _bootstrap_row(model, v_image, v_text, v_labels, rank, world, args.bootstrap, args.bootstrap_seed)
        if rank == 0:
            print(json.dumps(row), flush=True)
        history.append(row)
    if rank == 0 and args.save:
        torch.save({"aecf_state_dict": model.state_dict(), "history": history}, args.save)
    if world > 1:
        dist.destroy_process_group()
    return history


if __name__ == "__main__":
    main()
