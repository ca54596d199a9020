"""The fused classifier head on the device against the float64 reference of tests/mlhead_cases.py: every case through the C ABI
(poisoned outputs and workspace) and through linear_multilabel_loss -- counts equal, floats inside the derived bounds, exact
zeros where every target of a row or class is unknown, bit-equal repeats, Python's bits equal to the C ABI's; the loss-only
pass, frozen features, garbage logits under unknown targets, MultilabelHead, a captured forward + backward replayed with new
inputs, two ranks over one process group, the trainer with --fused-head, and the error paths."""
import datetime
import math
import os
import socket
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from aecf_amd import _lib
from tests import mlhead_cases as H
from tests import mlloss_cases as M

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda:0")
BF = torch.bfloat16
LABEL_KINDS = {"float32": _lib.AECF_F32, "bfloat16": _lib.AECF_BF16, "int8": _lib.AECF_MLLOSS_I8, "uint8": _lib.AECF_MLLOSS_U8,
               "bool": _lib.AECF_MLLOSS_U8}
REDUCTIONS = {"mean": _lib.AECF_MLLOSS_MEAN, "sum": _lib.AECF_MLLOSS_SUM}


def _bf(a, dev=DEV):
    t = torch.from_numpy(a.copy()).to(BF)
    assert np.array_equal(t.float().numpy(), a)                    # the case's values exist in bfloat16
    return t.to(dev)


def _vec(v, dev=DEV):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)


def _labels(c, dev=DEV):
    arr, kind = H.labels_of(c)
    t = torch.from_numpy(arr)
    if kind == "bool":
        t = t.to(torch.bool)
    elif kind == "bfloat16":
        t = t.to(BF)
    return t.to(dev)


def _options(c):
    f = c.form
    return dict(alpha=f.alpha, gamma_pos=f.gp, gamma_neg=f.gn, margin=f.m, label_smoothing=f.eps)


def _f64(t):
    return t.detach().double().cpu().numpy()


def _capi(c, reduction="mean", upstream=None, factor=1.0, dh_f32=False, want=1, h=None, w=None):
    """forward and backward through the C ABI with poisoned outputs and workspace; dict of numpy arrays (dh in float64 of its
    stored values)"""
    from aecf_amd.layer import _ptr, _stream
    lib = _lib.load()
    h = _bf(c.h) if h is None else h
    w = _bf(c.w) if w is None else w
    y = _labels(c)
    yv = y.view(torch.uint8) if y.dtype == torch.bool else y
    n, K = h.shape
    C = w.shape[0]
    bias = _vec(c.bias)
    a = None if not (c.a != 1).any() else _vec(c.a)
    b = None if not (c.b != 1).any() else _vec(c.b)
    f = c.form
    wsb = lib.aecf_mlhead_workspace_bytes(n, C, K)
    assert wsb == H.workspace_layout(n, C, K)
    nan32 = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)
    stats = torch.full((2, C), float("nan"), dtype=torch.float64, device=DEV)
    totals = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    dw_u, db_u, dw, db = nan32(C, K), nan32(C), nan32(C, K), nan32(C)
    dh = torch.full((n, K), float("nan"), dtype=torch.float32 if dh_f32 else BF, device=DEV)
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=DEV)
    args = (n, C, K, _lib.AECF_BF16, LABEL_KINDS[c.kind], _ptr(h), _ptr(w), _ptr(bias), _ptr(yv), _ptr(a), _ptr(b), f.gp, f.gn, f.m,
            f.eps, REDUCTIONS[reduction])
    _lib.check(lib.aecf_mlhead_forward(*args, want, _ptr(stats), _ptr(totals), _ptr(dw_u), _ptr(db_u), _ptr(ws), wsb, _stream()),
               "forward")
    out = {}
    if want:
        ws.fill_(0xFF)
        _lib.check(lib.aecf_mlhead_backward(*args, _ptr(totals), _ptr(up), factor, _ptr(dw_u), _ptr(db_u),
                                            _lib.AECF_F32 if dh_f32 else _lib.AECF_BF16, _ptr(dh), _ptr(dw), _ptr(db), _ptr(ws), wsb,
                                            _stream()), "backward")
        out.update(dh=_f64(dh), dw=_f64(dw), db=_f64(db), dw_u=_f64(dw_u), db_u=_f64(db_u))
    torch.cuda.synchronize()
    tail = totals[2:].view(torch.float32).cpu().numpy()
    assert tail[1] == 0.0
    out.update(loss=tail[0], stats=stats.cpu().numpy(), totals=totals[:2].cpu().numpy())
    return out


def _python(c, reduction="mean", hidden_grad=True, upstream=None, **kw):
    """linear_multilabel_loss with return_per_class and its backward; dict of numpy arrays"""
    from aecf_amd import losses
    h = _bf(c.h).requires_grad_(hidden_grad)
    w = _bf(c.w).requires_grad_(True)
    bias = None if c.bias is None else _vec(c.bias).requires_grad_(True)
    loss, per_class = losses.linear_multilabel_loss(h, w, bias, _labels(c), pos_weight=_vec(c.pos_weight), class_weight=_vec(c.class_weight),
                                                    reduction=reduction, return_per_class=True, **_options(c), **kw)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device == h.device
    assert per_class.shape == (c.w.shape[0],) and per_class.dtype == torch.float32 and not per_class.requires_grad
    (loss if upstream is None else loss * upstream).backward()
    assert w.grad.dtype == BF and (bias is None or bias.grad.dtype == torch.float32)
    assert (h.grad is not None and h.grad.dtype == BF) if hidden_grad else h.grad is None
    return dict(loss=loss.detach().cpu().numpy(), per_class=per_class.cpu().numpy(), dh=None if h.grad is None else h.grad,
                dw=w.grad, db=None if bias is None else bias.grad)


def _check(c, ref, got, what, dh_rounded=True, dw_rounded=False):
    """counts equal, floats inside the bounds, exact zeros where demanded"""
    ratios = dict(loss=M.check_close(got["loss"], ref.loss, ref.loss_bound, f"{what} loss"))
    if "stats" in got:
        ratios["sums"] = M.check_close(got["stats"][0], ref.stats[0], ref.stats_bound, f"{what} class sums")
        assert np.array_equal(got["stats"][1], ref.stats[1]), f"{what}: valid counts"
        assert got["totals"][1] == ref.n_valid, f"{what}: N"
    if "per_class" in got:
        ratios["per_class"] = M.check_close(got["per_class"], ref.per_class, ref.per_class_bound, f"{what} per-class means")
    if got.get("dh") is not None:
        dh = _f64(got["dh"]) if isinstance(got["dh"], torch.Tensor) else got["dh"]
        ratios["dh"] = M.check_close(dh, ref.dh, H.rounded(ref.dh_bound, ref.dh) if dh_rounded else ref.dh_bound, f"{what} dh")
        H.check_zero(dh, ref.zero_rows, f"{what} dh")
    if got.get("dw") is not None:
        dw = _f64(got["dw"]) if isinstance(got["dw"], torch.Tensor) else got["dw"]
        ratios["dw"] = M.check_close(dw, ref.dw, H.rounded(ref.dw_bound, ref.dw) if dw_rounded else ref.dw_bound, f"{what} dW")
        H.check_zero(dw, ref.zero_classes, f"{what} dW")
    if got.get("db") is not None:
        db = _f64(got["db"]) if isinstance(got["db"], torch.Tensor) else got["db"]
        ratios["db"] = M.check_close(db, ref.db, ref.db_bound, f"{what} dbias")
        H.check_zero(db, ref.zero_classes, f"{what} dbias")
    print(f"mlhead {what}: error / bound " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    return ratios


def _same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("name", H.CASE_IDS)
def test_case_through_the_c_abi_and_python(name):
    """loss, class sums, valid counts, N and every element of dh, dW and dbias inside the bounds; exact zeros for fully unknown
    rows and classes and when nothing is valid; two runs bit-equal; the Python surface gives the C ABI's bits (weight.grad is
    the float32 dW cast once to bfloat16)"""
    c = H.case(name)
    ref = H.reference(c)
    got = _capi(c)
    _check(c, ref, got, f"C ABI {name}")
    if ref.n_valid == 0:
        assert got["loss"] == 0.0 and not got["stats"].any() and not got["dh"].any() and not got["dw"].any() and not got["db"].any()
    _same_bits(got, _capi(c))
    py = _python(c)
    _check(c, ref, py, f"linear_multilabel_loss {name}", dw_rounded=True)
    assert np.array_equal(py["loss"], got["loss"])
    assert np.array_equal(_f64(py["dh"]), got["dh"])
    assert np.array_equal(_f64(py["dw"]), _f64(torch.from_numpy(got["dw"]).to(torch.float32).to(BF)))
    if c.bias is not None:
        assert np.array_equal(_f64(py["db"]), got["db"])


@pytest.mark.parametrize("name", ["H2", "H3", "H6", "H7", "H8"])
def test_sum_reduction_upstream_factor_and_float32_dh(name):
    """reduction="sum" (and "mean") with an upstream gradient of -0.5 and a factor of 3, dh stored as float32: no output rounding"""
    c = H.case(name)
    for reduction in ("sum", "mean"):
        ref = H.reference(c, reduction, upstream=-1.5)
        got = _capi(c, reduction, upstream=-0.5, factor=3.0, dh_f32=True)
        _check(c, ref, got, f"C ABI {name} {reduction}, upstream -0.5 x 3, float32 dh", dh_rounded=False)
    py = _python(c, "sum", upstream=-1.5)
    _check(c, H.reference(c, "sum", upstream=-1.5), py, f"linear_multilabel_loss {name} sum, upstream -1.5", dw_rounded=True)


@pytest.mark.parametrize("name", ["H2", "H3", "H6", "H7", "H8", "H10_focal"])
def test_loss_only_pass_and_frozen_features_have_the_bits_of_the_full_call(name):
    """under torch.no_grad() (the pass without the second product) the loss and the stats have the bits of the grad-mode
    forward; with hidden.requires_grad == False (no ROW launch) weight.grad and bias.grad have the bits of the full call"""
    from aecf_amd import losses
    c = H.case(name)
    full = _python(c)
    lo = _capi(c, want=0)
    hi = _capi(c)
    for k in ("loss", "stats", "totals"):
        assert np.array_equal(lo[k], hi[k], equal_nan=True), k
    with torch.no_grad():
        quiet, per_class = losses.linear_multilabel_loss(_bf(c.h).requires_grad_(True), _bf(c.w).requires_grad_(True), _vec(c.bias),
                                                         _labels(c), pos_weight=_vec(c.pos_weight), class_weight=_vec(c.class_weight),
                                                         return_per_class=True, **_options(c))
    assert not quiet.requires_grad and quiet.grad_fn is None
    assert np.array_equal(quiet.cpu().numpy(), full["loss"]) and np.array_equal(per_class.cpu().numpy(), full["per_class"])
    frozen = _python(c, hidden_grad=False)
    assert np.array_equal(frozen["loss"], full["loss"])
    assert torch.equal(frozen["dw"], full["dw"]) and (c.bias is None or torch.equal(frozen["db"], full["db"]))


def test_garbage_logits_under_unknown_targets_change_no_bit():
    """finite garbage in the weight rows of fully unknown classes (H5) and in the feature rows of fully unknown rows (H3_row)
    makes garbage logits under unknown targets only: no bit of the loss, the stats, dh, dW or dbias moves (the garbage rows'
    own gradients are exact zeros either way)"""
    c = H.case("H5")
    ref = H.reference(c)
    w = c.w.copy()
    w[ref.zero_classes] = M.to_bf16(np.float32(300.0) * np.sign(w[ref.zero_classes]) + w[ref.zero_classes])
    assert ref.zero_classes.sum() == 2
    _same_bits(_capi(c), _capi(c, w=_bf(w)))
    c = H.case("H3_row")
    ref = H.reference(c)
    h = c.h.copy()
    h[ref.zero_rows] = M.to_bf16(np.float32(1e4) * h[ref.zero_rows])
    assert ref.zero_rows.sum() == 2
    _same_bits(_capi(c), _capi(c, h=_bf(h)))


def test_multilabel_head_module():
    """state_dict round trip with an nn.Linear, from_linear shares the parameters, forward equals F.linear, loss is the fused
    call with the module's own folded scale vectors"""
    from aecf_amd import losses
    c = H.case("H2")
    ref = H.reference(c)
    lin = torch.nn.Linear(128, 15).to(DEV, BF)
    with torch.no_grad():
        lin.weight.copy_(_bf(c.w))
        lin.bias.copy_(_bf(c.bias))
    head = losses.MultilabelHead.from_linear(lin, pos_weight=_vec(c.pos_weight), class_weight=_vec(c.class_weight))
    assert head.weight is lin.weight and head.bias is lin.bias and set(head.state_dict()) == {"weight", "bias"}
    x = _bf(c.h)
    assert torch.equal(head(x), torch.nn.functional.linear(x, lin.weight, lin.bias))
    other = losses.MultilabelHead(128, 15, pos_weight=c.pos_weight.tolist(), class_weight=c.class_weight.tolist(), device=DEV, dtype=BF)
    other.load_state_dict(lin.state_dict())
    torch.nn.Linear(128, 15).to(DEV, BF).load_state_dict(other.state_dict())
    for m in (head, other):
        m.zero_grad()
        loss = m.loss(x, _labels(c))
        loss.backward()
        got = dict(loss=loss.detach().cpu().numpy(), dw=m.weight.grad, db=m.bias.grad.float())
        assert m.weight.grad.dtype == BF and m.bias.grad.dtype == BF
        M.check_close(got["loss"], ref.loss, ref.loss_bound, "head loss")
        M.check_close(_f64(got["dw"]), ref.dw, H.rounded(ref.dw_bound, ref.dw), "head dW")
        M.check_close(_f64(got["db"]), ref.db, H.rounded(ref.db_bound, ref.db), "head dbias")
    assert lin.weight.grad is head.weight.grad
    assert len(head._folds) == 1


def test_captured_forward_and_backward_replay_with_new_inputs():
    """no host read: forward + backward capture, and three replays with features, labels and the upstream gradient changed in
    place -- the number of valid elements too -- give the three references"""
    from aecf_amd import losses
    base = H.case("H3")
    g = np.random.default_rng(77)
    sets = []
    for i in range(3):
        h = M.to_bf16(g.standard_normal(base.h.shape).astype(np.float32))
        valid = g.random(base.t.shape) >= (0.1 + 0.3 * i)
        t = np.where(valid, (g.random(base.t.shape) < 0.4).astype(np.float32), np.float32(np.nan)).astype(np.float32)
        sets.append((base._replace(h=h, t=t, valid=valid), 0.5 + i))
    opts = _options(base)
    h = torch.zeros(65, 256, dtype=BF, device=DEV, requires_grad=True)
    w, b = _bf(base.w).requires_grad_(True), _vec(base.bias).requires_grad_(True)
    y = torch.zeros(65, 17, device=DEV)
    up = torch.ones((), device=DEV)
    losses.linear_multilabel_loss(h, w, b, y, **opts).backward()      # warm-up outside the capture
    h.grad = w.grad = b.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = losses.linear_multilabel_loss(h, w, b, y, **opts)
        dh, dw, db = torch.autograd.grad(loss, (h, w, b), grad_outputs=up)
    counts = set()
    for i, (c, upstream) in enumerate(sets):
        with torch.no_grad():
            h.copy_(torch.from_numpy(c.h.copy()))
            y.copy_(torch.from_numpy(c.t.copy()))
            up.fill_(upstream)
        graph.replay()
        torch.cuda.synchronize()
        ref = H.reference(c, upstream=upstream)
        counts.add(ref.n_valid)
        _check(c, ref, dict(loss=loss.detach().cpu().numpy(), dh=dh, dw=dw, db=db), f"replay {i}", dw_rounded=True)
    assert len(counts) == 3


# ---------------------------------------------------------------------------------------------- two ranks

TWO_RANK_CASE = "H6"
CUT = 400                                                           # rank 0 holds rows [0, 400), rank 1 the other 700
SPLITS = ("uneven", "empty")


def _two_ranks_worker(rank, world, port, backend, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from aecf_amd import losses
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    limit = datetime.timedelta(seconds=90)          # a collective without its partner raises here instead of hanging
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=limit)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=limit)
    done, error = {}, None
    try:
        c = H.case(TWO_RANK_CASE)
        n = c.h.shape[0]
        for split in SPLITS:
            lo, hi = ((0, CUT) if rank == 0 else (CUT, n)) if split == "uneven" else ((0, n) if rank == 0 else (n, n))
            h = _bf(c.h, dev)[lo:hi].clone().requires_grad_(True)
            w, b = _bf(c.w, dev).requires_grad_(True), _vec(c.bias, dev).requires_grad_(True)
            loss, per_class = losses.linear_multilabel_loss(h, w, b, _labels(c, dev)[lo:hi], pos_weight=_vec(c.pos_weight, dev),
                                                            class_weight=_vec(c.class_weight, dev), group=dist.group.WORLD,
                                                            return_per_class=True, **_options(c))
            loss.backward()
            scales = losses._compute_scales(_vec(c.pos_weight, dev), _vec(c.class_weight, dev), c.form.alpha, c.w.shape[0], dev)
            f = c.form
            _, stats = losses._LinearMultilabelLoss.apply(h.detach(), w.detach(), b.detach(), _labels(c, dev)[lo:hi], *scales, f.gp, f.gn,
                                                          f.m, f.eps, "mean", dist.group.WORLD, False)
            done[split] = dict(loss=loss.detach().cpu().numpy(), per_class=per_class.cpu().numpy(), dh=_f64(h.grad), dw=_f64(w.grad),
                               db=_f64(b.grad), stats=stats.cpu().numpy())
    except Exception:
        error = f"rank {rank}:\n{traceback.format_exc()}"
    finally:
        q.put((rank, done, error))
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks():
    world = 2
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_two_ranks_worker, args=(r, world, port, backend, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = []
    try:
        got = sorted([q.get(timeout=240) for _ in range(world)], key=lambda r: r[0])
        for p in procs:
            p.join(60)
    finally:
        alive = [p for p in procs if p.is_alive()]
        for p in alive:
            p.kill()
        for p in alive:
            p.join(30)
    errors = [e for _, _, e in got if e is not None]
    assert not errors, "\n".join(errors)
    assert not alive and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return [done for _, done, _ in got]


@pytest.mark.parametrize("split", SPLITS)
def test_two_ranks_equal_one_rank(two_ranks, split):
    """uneven shards and an empty shard: the value is the global loss on both ranks (the same bits), inside the one-rank
    bounds, and so are the global per-class means (the stats).  Every rank's gradients carry world / N; averaged over the ranks
    as dp's collectives do they are the one-rank gradients: dh is the shards side by side, halved; dW and dbias are the sum of
    the shards' parts, each inside the bound of ITS rows (a shard's reference with reduction "sum" and an upstream of 1 / N)
    with its one cast to bfloat16."""
    c = H.case(TWO_RANK_CASE)
    ref = H.reference(c, world=2)
    n = c.h.shape[0]
    r0, r1 = (r[split] for r in two_ranks)
    assert np.array_equal(r0["loss"], r1["loss"]) and np.array_equal(r0["per_class"], r1["per_class"])
    M.check_close(r0["loss"], ref.loss, ref.loss_bound, f"two ranks {split}: loss")
    M.check_close(r0["per_class"], ref.per_class, ref.per_class_bound, f"two ranks {split}: per-class means")
    assert np.array_equal(r0["stats"], r1["stats"]) and np.array_equal(r0["stats"][1], ref.stats[1])      # the global valid counts
    M.check_close(r0["stats"][0], ref.stats[0], ref.stats_bound, f"two ranks {split}: class sums")
    bounds = ((0, CUT), (CUT, n)) if split == "uneven" else ((0, n), (n, n))
    dw, dw_b, db, db_b = 0.0, 0.0, 0.0, 0.0
    for r, (lo, hi) in zip((r0, r1), bounds):
        assert r["dh"].shape == (hi - lo, c.h.shape[1])
        if hi == lo:
            assert not r["dw"].any() and not r["db"].any()          # the empty shard: zero parameter gradients
            continue
        part = H.reference(c._replace(h=c.h[lo:hi], t=c.t[lo:hi], valid=c.valid[lo:hi]), "sum", upstream=1.0 / ref.n_valid, world=2)
        M.check_close(r["dh"] / 2.0, part.dh, H.rounded(part.dh_bound, part.dh), f"two ranks {split}: dh of rows {lo}:{hi}")
        assert np.abs(part.dh - ref.dh[lo:hi]).max() <= 1e-12
        dw, dw_b = dw + part.dw, dw_b + H.rounded(part.dw_bound, part.dw)
        db, db_b = db + part.db, db_b + part.db_bound
    assert np.abs(dw - ref.dw).max() <= 1e-12 and np.abs(db - ref.db).max() <= 1e-12
    M.check_close((r0["dw"] + r1["dw"]) / 2.0, ref.dw, dw_b, f"two ranks {split}: dW")
    M.check_close((r0["db"] + r1["db"]) / 2.0, ref.db, db_b, f"two ranks {split}: dbias")
    one = _python(c)
    M.check_close(r0["loss"], one["loss"], ref.loss_bound, "two ranks against one: loss")
    M.check_close(r0["per_class"], one["per_class"], ref.per_class_bound, "two ranks against one: per-class means")


# ---------------------------------------------------------------------------------------------- the trainer

def test_trainer_with_the_fused_head():
    """train_xray.main --param-dtype bfloat16 --fused-head for two epochs of one step each: finite losses and the usual keys.
    The first step's loss against the unfused --loss bce step on the same seed: both see the same features (the same model,
    data and dropout draws), rebuilt here; the fused loss is inside the head's derived bound of the float64 reference on them,
    and the unfused one inside that bound widened by what rounding its logits to bfloat16 costs, mean |g| 2**-8 |z| (and the
    second-order term (1/4) (2**-8 z)**2 / 2)."""
    from aecf_amd import train_xray
    from aecf_amd.xray import AECFModel
    argv = ["--epochs", "2", "--switch-epoch", "1", "--samples", "64", "--val-samples", "128", "--batch", "64", "--classes", "5",
            "--param-dtype", "bfloat16"]
    fused = train_xray.main(argv + ["--fused-head"])
    keys = {"epoch", "curriculum", "train_loss", "gate_entropy", "sec", "val_map", "val_map_no_images", "val_map_no_texts"}
    assert len(fused) == 2
    for row in fused:
        assert set(row) == keys and math.isfinite(row["train_loss"]) and row["train_loss"] > 0 and 0.0 < row["val_map"] <= 1.0
    unfused = train_xray.main(argv + ["--loss", "bce"])
    with pytest.raises(SystemExit):
        train_xray.main(argv[:-2] + ["--fused-head"])               # float32 parameters
    # the first step's features, as main() makes them
    image, text, labels = train_xray.synthetic_split(64, 5, 512, 1, DEV)
    torch.manual_seed(0)
    model = AECFModel(512, 512, 5, 256).to(DEV).bfloat16().train()
    perm = torch.randperm(64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    with torch.no_grad():
        hidden = model(image.bfloat16()[perm], text.bfloat16()[perm], return_hidden=True)
    lin = model.classifier[3]
    ones = np.ones(5, dtype=np.float32)
    c = H.Case(M.FORMS["bce"], hidden.float().cpu().numpy(), lin.weight.float().detach().cpu().numpy(), lin.bias.float().detach().cpu().numpy(),
               labels[perm].cpu().numpy(), np.ones((64, 5), dtype=bool), "float32", None, None, ones, ones)
    ref = H.reference(c)
    r = M.check_close(fused[0]["train_loss"], ref.loss, ref.loss_bound, "the fused first step's loss")
    z = np.abs(ref.z) * H.UB
    logit_rounding = float((np.abs(ref.g) * z + 0.125 * z * z).mean()) * M.SECOND_ORDER
    M.check_close(unfused[0]["train_loss"], ref.loss, 2 * ref.loss_bound + logit_rounding, "the unfused first step's loss")
    M.check_close(fused[0]["train_loss"], unfused[0]["train_loss"], 3 * ref.loss_bound + logit_rounding, "fused against unfused")
    print(f"mlhead trainer: first step fused {fused[0]['train_loss']:.7f} unfused {unfused[0]['train_loss']:.7f} reference {ref.loss:.7f} "
          f"(fused error / bound {r:.3f}; logit rounding allows {logit_rounding:.2e})")


def test_train_step_with_a_head():
    """xray.train_step(head=...) on both routings: the step runs through head.loss, updates classifier[3] and returns a finite loss"""
    from aecf_amd import losses
    from aecf_amd.xray import AECFModel, train_step
    g = torch.Generator().manual_seed(9)
    image, text = torch.randn(64, 512, generator=g).to(DEV, BF), torch.randn(64, 512, generator=g).to(DEV, BF)
    labels = (torch.rand(64, 15, generator=g) < 0.2).to(DEV)
    for static in (False, True):
        torch.manual_seed(4)
        model = AECFModel(512, 512, 15).to(DEV).bfloat16().train()
        model.static_routing = static
        head = losses.MultilabelHead.from_linear(model.classifier[3], gamma_neg=4.0, margin=0.05)
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        before = model.classifier[3].weight.detach().clone()
        hidden = model(image, text, return_hidden=True)
        assert hidden.shape == (64, 256) and model(image, text).shape == (64, 15)
        loss, info = train_step(model, opt, None, image, text, labels, head=head)
        assert math.isfinite(float(loss)) and float(loss) > 0 and not torch.equal(before, model.classifier[3].weight)
        assert all(torch.isfinite(p).all() for p in model.parameters())


def test_error_paths():
    from aecf_amd import losses
    c = H.case("H2")
    h, w, b, y = _bf(c.h), _bf(c.w), _vec(c.bias), _labels(c)
    alt = "use F.linear"
    with pytest.raises(NotImplementedError, match=f"bfloat16 hidden and weight only.*{alt}"):
        losses.linear_multilabel_loss(h.float(), w.float(), b, y)
    with pytest.raises(NotImplementedError, match=f"bfloat16 hidden and weight only.*{alt}"):
        losses.linear_multilabel_loss(h.half(), w.half(), b, y)
    with pytest.raises(NotImplementedError, match=f"serves K in .*got K = 192.*{alt}"):
        losses.linear_multilabel_loss(torch.zeros(4, 192, dtype=BF, device=DEV), torch.zeros(3, 192, dtype=BF, device=DEV), None,
                                      torch.zeros(4, 3, device=DEV))
    with pytest.raises(NotImplementedError, match=f"C <= 65536.*{alt}"):
        losses.linear_multilabel_loss(torch.zeros(1, 128, dtype=BF, device=DEV), torch.zeros(65537, 128, dtype=BF, device=DEV), None,
                                      torch.zeros(1, 65537, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match=r"hidden \[n, K\] and weight \[C, K\]"):
        losses.linear_multilabel_loss(h, w[:, :64], b, y)
    with pytest.raises(ValueError, match=r"targets \[n, C\] = \[33, 15\]"):
        losses.linear_multilabel_loss(h, w, b, y[:-1])
    with pytest.raises(ValueError, match=r"bias \[C\] = \[15\]"):
        losses.linear_multilabel_loss(h, w, b[:-1], y)
    with pytest.raises(TypeError, match="targets, got torch.int64"):
        losses.linear_multilabel_loss(h, w, b, y.long())
    with pytest.raises(ValueError, match="there is no 'none'"):
        losses.linear_multilabel_loss(h, w, b, y, reduction="none")
    with pytest.raises(ValueError, match=r"margin must lie in \[0, 1\)"):
        losses.linear_multilabel_loss(h, w, b, y, margin=1.0)
    with pytest.raises(ValueError, match="gamma_pos must be finite and >= 0"):
        losses.linear_multilabel_loss(h, w, b, y, gamma_pos=float("inf"))
    with pytest.raises(ValueError, match=r"pos_weight must hold one value per class, \[15\]"):
        losses.linear_multilabel_loss(h, w, b, y, pos_weight=torch.ones(14, device=DEV))
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.linear_multilabel_loss(h, w.cpu(), b, y)
    hg = h.clone().requires_grad_(True)
    up = torch.ones((), device=DEV, requires_grad=True)
    (gh,) = torch.autograd.grad(losses.linear_multilabel_loss(hg, w, b, y), hg, grad_outputs=up, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):   # a second backward, through the first, is refused
        gh.sum().backward()
    assert losses.linear_multilabel_loss(h, w, b, y).grad_fn is None   # nothing requires a gradient
