"""The multi-label classification loss on the device against the float64 reference of tests/mlloss_cases.py: every case and
logits dtype through the C ABI and through multilabel_loss (loss, per-class means and every gradient element inside the derived
bounds, exact zeros, infinities and NaN where the reference has them, bit-equal repeats), the label dtypes, torch's own
binary_cross_entropy_with_logits on the device, the error paths, a captured forward + backward replayed with new inputs, two
ranks over one process group, class_balance_weights, MultilabelLoss as the criterion of a graphed step, and the trainer."""
import copy
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
from tests import mlloss_cases as M

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda:0")
TORCH_DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
ABI_DTYPES = {"float32": _lib.AECF_F32, "bfloat16": _lib.AECF_BF16, "float16": _lib.AECF_F16}
REDUCTIONS = {"mean": _lib.AECF_MLLOSS_MEAN, "sum": _lib.AECF_MLLOSS_SUM}


def _logits(c, dtype, dev=DEV):
    x = torch.from_numpy(c.x.copy()).to(TORCH_DTYPES[dtype])
    assert np.array_equal(x.float().numpy(), c.x, equal_nan=True)              # the case's values exist in its dtype
    return x.to(dev)


def _vec(v, dev=DEV):
    return None if v is None else torch.from_numpy(v.copy()).to(dev)


def _options(c):
    f = c.form
    return dict(alpha=f.alpha, gamma_pos=f.gp, gamma_neg=f.gn, margin=f.m, label_smoothing=f.eps)


def _capi(c, dtype, reduction="mean", upstream=None, factor=1.0):
    """forward and backward through the C ABI with poisoned outputs; (loss float32, stats [2, C], totals (sum, N), dlogits) as
    numpy (the gradient in float64 of its stored values)"""
    from aecf_amd.layer import _ptr, _stream
    lib = _lib.load()
    x, y = _logits(c, dtype), torch.from_numpy(c.t.copy()).to(DEV)
    n, C = x.shape
    a = None if not (c.a != 1).any() else _vec(c.a)
    b = None if not (c.b != 1).any() else _vec(c.b)
    f = c.form
    wsb = lib.aecf_mlloss_workspace_bytes(n, C)
    assert wsb == M.workspace_layout(n, C)
    ws = torch.full((wsb,), 0xA5, dtype=torch.uint8, device=DEV)
    stats = torch.full((2, C), float("nan"), dtype=torch.float64, device=DEV)
    totals = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    dx = torch.full_like(x, float("nan"))
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=DEV)
    args = (n, C, ABI_DTYPES[dtype], _lib.AECF_F32, _ptr(x), _ptr(y), _ptr(a), _ptr(b), f.gp, f.gn, f.m, f.eps, REDUCTIONS[reduction])
    _lib.check(lib.aecf_mlloss_forward(*args, _ptr(stats), _ptr(totals), _ptr(ws), wsb, _stream()), "forward")
    _lib.check(lib.aecf_mlloss_backward(*args, _ptr(totals), _ptr(up), factor, _ptr(dx), _stream()), "backward")
    torch.cuda.synchronize()
    tail = totals[2:].view(torch.float32).cpu().numpy()
    assert tail[1] == 0.0
    return tail[0], stats.cpu().numpy(), totals[:2].cpu().numpy(), dx.double().cpu().numpy()


def _python(c, dtype, reduction="mean", labels=None, **kw):
    """multilabel_loss with return_per_class and its backward; (loss, per_class, dlogits) as numpy"""
    from aecf_amd import losses
    x = _logits(c, dtype).requires_grad_(True)
    y = torch.from_numpy(c.t.copy()).to(DEV) if labels is None else labels
    loss, per_class = losses.multilabel_loss(x, y, pos_weight=_vec(c.pos_weight), class_weight=_vec(c.class_weight), reduction=reduction,
                                             return_per_class=True, **_options(c), **kw)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device == x.device
    assert per_class.shape == (c.x.shape[1],) and per_class.dtype == torch.float32 and not per_class.requires_grad
    loss.backward()
    assert x.grad.dtype == x.dtype
    return loss.detach().cpu().numpy(), per_class.cpu().numpy(), x.grad.double().cpu().numpy()


def _check(ref, dtype, loss, per_class, grad, what, stats=None, factor=1.0):
    ratios = dict(loss=M.check_close(loss, ref.loss, ref.loss_bound, f"{what} loss"),
                  grad=M.check_close(grad, ref.grad * factor, M.grad_bound_for(ref, dtype, factor), f"{what} gradient"))
    if per_class is not None:
        ratios["per_class"] = M.check_close(per_class, ref.per_class, ref.per_class_bound, f"{what} per-class means")
    if stats is not None:
        ratios["sums"] = M.check_close(stats[0], ref.stats[0], ref.stats_bound, f"{what} class sums")
        assert np.array_equal(stats[1], ref.stats[1]), f"{what}: valid counts"
    assert not grad[ref.zero_grad].any(), f"{what}: exact zeros at ignored elements and dead terms"
    print(f"mlloss {what}: error / bound " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


@pytest.mark.parametrize("dtype", M.DTYPES)
@pytest.mark.parametrize("name", M.CASE_IDS)
def test_case_through_the_c_abi_and_python(name, dtype):
    """loss, class sums, valid counts, per-class means and every gradient element inside the bounds; exact zeros at
    ignored elements and dead terms and when everything is ignored; infinities as infinities; NaN at the valid NaN logit only;
    two runs bit-equal; the Python surface gives the C ABI's bits"""
    c = M.case(name, dtype)
    ref = M.reference(c)
    loss, stats, totals, grad = _capi(c, dtype)
    _check(ref, dtype, loss, None, grad, f"C ABI {name} {dtype}", stats=stats)
    assert totals[1] == ref.n_valid
    if ref.n_valid == 0:
        assert loss == 0.0 and not stats.any() and not grad.any()
    again = _capi(c, dtype)
    for u, v in zip((loss, stats, totals, grad), again):
        assert np.array_equal(u, v, equal_nan=True)
    py_loss, per_class, py_grad = _python(c, dtype)
    _check(ref, dtype, py_loss, per_class, py_grad, f"multilabel_loss {name} {dtype}")
    assert np.array_equal(py_loss, loss, equal_nan=True) and np.array_equal(py_grad, grad, equal_nan=True)
    if name.startswith("specials"):
        nan = np.zeros_like(c.valid)
        nan[3, M.NAN_CLASS] = True
        assert np.array_equal(np.isnan(grad), nan) and np.isfinite(grad[~nan]).all()
        assert np.array_equal(np.isnan(per_class), np.arange(c.x.shape[1]) == M.NAN_CLASS)
        zeroed = _capi(M.zeroed_ignored(c), dtype)                  # the ignored logits reach no output: the same bits
        for u, v in zip((loss, stats, totals, grad), zeroed):
            assert np.array_equal(u, v, equal_nan=True)


@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("name", ["bce_64x15", "bce_w_2049x80_class", "bce_w_257x17_some"])
def test_against_torch_on_the_device(name, reduction):
    """reduction="sum" and "mean" against the reference and against torch's own float32 binary_cross_entropy_with_logits with
    weight and pos_weight over the valid elements: the loss inside the same bound; an upstream gradient and a factor scale the
    gradient.  torch's float32 gradient is w ((1 + (p - 1) t) sigmoid(x) - p t): a difference of terms up to max(a, b) formed
    from a sigmoid of 2 U relative error in a handful of roundings, so it carries an ABSOLUTE error of up to 8 U max(a, b) times
    the scale where this library's is relative; that much is added to the bound of the gradient comparison."""
    c = M.case(name)
    ref = M.reference(c, reduction)
    loss, stats, _, grad = _capi(c, "float32", reduction, upstream=0.5, factor=3.0)
    _check(ref, "float32", loss, None, grad, f"C ABI {name} {reduction}, upstream 0.5 x 3", stats=stats, factor=1.5)
    py_loss, per_class, py_grad = _python(c, "float32", reduction)
    _check(ref, "float32", py_loss, per_class, py_grad, f"multilabel_loss {name} {reduction}")
    x = _logits(c, "float32").requires_grad_(True)
    valid = torch.from_numpy(c.valid).to(DEV)
    t = torch.where(valid, torch.from_numpy(c.t.copy()).to(DEV), torch.zeros((), device=DEV))
    el = torch.nn.functional.binary_cross_entropy_with_logits(x, t, weight=_vec(c.class_weight), pos_weight=_vec(c.pos_weight),
                                                              reduction="none")
    total = torch.where(valid, el, torch.zeros((), device=DEV)).sum()
    theirs = total / valid.sum() if reduction == "mean" else total
    theirs.backward()
    M.check_close(py_loss, theirs.detach().cpu().numpy(), ref.loss_bound, f"{name} {reduction}: loss against torch")
    theirs_abs = 8 * M.U * np.maximum(c.a, c.b)[None, :] * (1.0 / ref.n_valid if reduction == "mean" else 1.0)
    M.check_close(py_grad, x.grad.double().cpu().numpy(), ref.grad_bound + theirs_abs, f"{name} {reduction}: gradient against torch")


@pytest.mark.parametrize("label_dtype", [torch.bool, torch.uint8, torch.int8, torch.float32, torch.bfloat16, torch.float16])
def test_label_dtypes(label_dtype):
    """bool and uint8 have no unknown value; int8 marks it with -1 (and counts 3 as 1); floating point with NaN and -1"""
    c = M.case("focal_2049x80_some", "bfloat16")
    hard = torch.from_numpy(np.where(c.valid, c.t, 0.0) != 0)
    if label_dtype in (torch.bool, torch.uint8):
        c = c._replace(valid=np.ones_like(c.valid), t=hard.float().numpy())
        labels = hard.to(label_dtype) if label_dtype == torch.bool else hard.to(label_dtype) * 7
    elif label_dtype == torch.int8:
        labels = torch.where(torch.from_numpy(c.valid), hard.to(torch.int8) * 3, torch.tensor(-1, dtype=torch.int8))
    else:
        labels = torch.from_numpy(c.t.copy()).to(label_dtype)
    ref = M.reference(c)
    loss, per_class, grad = _python(c, "bfloat16", labels=labels.to(DEV))
    _check(ref, "bfloat16", loss, per_class, grad, f"labels {label_dtype}")


def test_error_paths():
    from aecf_amd import losses
    c = M.case("asl_64x15_some")
    x, y = _logits(c, "float32"), torch.from_numpy(c.t.copy()).to(DEV)
    with torch.no_grad():                                           # the forward only
        quiet = losses.multilabel_loss(x.clone().requires_grad_(True), y, **_options(c))
    assert not quiet.requires_grad and quiet.grad_fn is None
    assert losses.multilabel_loss(x, y, **_options(c)).grad_fn is None           # logits that need no gradient
    M.check_close(quiet.cpu().numpy(), M.reference(c).loss, M.reference(c).loss_bound, "no_grad loss")
    xg = x.clone().requires_grad_(True)
    up = torch.ones((), device=DEV, requires_grad=True)
    (g,) = torch.autograd.grad(losses.multilabel_loss(xg, y, **_options(c)), xg, grad_outputs=up, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):   # a second backward, through the first, is refused
        g.sum().backward()
    with pytest.raises(ValueError, match="one shape"):
        losses.multilabel_loss(x, y[:-1])
    with pytest.raises(TypeError, match="float32, bfloat16 or float16 logits"):
        losses.multilabel_loss(x.double(), y)
    with pytest.raises(TypeError, match="targets, got torch.int64"):
        losses.multilabel_loss(x, y.long())
    with pytest.raises(ValueError, match="there is no 'none'"):
        losses.multilabel_loss(x, y, reduction="none")
    with pytest.raises(ValueError, match=r"margin must lie in \[0, 1\)"):
        losses.multilabel_loss(x, y, margin=1.0)
    with pytest.raises(ValueError, match=r"label_smoothing must lie in \[0, 1\)"):
        losses.multilabel_loss(x, y, label_smoothing=-0.1)
    with pytest.raises(ValueError, match=r"alpha must lie in \[0, 1\]"):
        losses.multilabel_loss(x, y, alpha=1.5)
    with pytest.raises(ValueError, match="gamma_pos must be finite and >= 0"):
        losses.multilabel_loss(x, y, gamma_pos=float("inf"))
    with pytest.raises(ValueError, match=r"pos_weight must hold one value per class, \[15\]"):
        losses.multilabel_loss(x, y, pos_weight=torch.ones(14, device=DEV))
    with pytest.raises(ValueError, match="class_weight must hold one value per class, 15"):
        losses.multilabel_loss(x, y, class_weight=[1.0] * 16)
    with pytest.raises(NotImplementedError, match="C <= 4096"):
        losses.multilabel_loss(torch.zeros(2, 4097, device=DEV), torch.zeros(2, 4097, device=DEV))


def test_captured_forward_and_backward_replay_with_new_inputs():
    """no host read: forward + backward capture, and three replays with logits and labels changed in place -- the number of
    valid elements too -- give the three references"""
    from aecf_amd import losses
    names = ("asl1_257x17_some", "frac_257x17", "asl1_257x17_some")
    sets = [M.case(nm, "bfloat16") for nm in names]
    sets[2] = sets[2]._replace(x=sets[1].x, valid=~sets[0].valid, t=np.where(~sets[0].valid, np.float32(1.0), np.float32(np.nan)))
    c0 = sets[0]
    opts = dict(gamma_pos=1.0, gamma_neg=4.0, margin=0.05)
    x = torch.zeros(257, 17, dtype=torch.bfloat16, device=DEV, requires_grad=True)
    y = torch.zeros(257, 17, device=DEV)
    losses.multilabel_loss(x, y, **opts).backward()                  # warm-up outside the capture
    x.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, per_class = losses.multilabel_loss(x, y, return_per_class=True, **opts)
        (grad,) = torch.autograd.grad(loss, x)
    counts = set()
    for i, c in enumerate(sets):
        c = c._replace(form=c0.form, a=c0.a, b=c0.b)
        with torch.no_grad():
            x.copy_(torch.from_numpy(c.x.copy()))
            y.copy_(torch.from_numpy(c.t.copy()))
        graph.replay()
        torch.cuda.synchronize()
        ref = M.reference(c)
        counts.add(ref.n_valid)
        _check(ref, "bfloat16", loss.detach().cpu().numpy(), per_class.cpu().numpy(), grad.detach().double().cpu().numpy(), f"replay {i}")
    assert len(counts) == 3


# ---------------------------------------------------------------------------------------------- two ranks

TWO_RANK_CASE = "bce_w_257x17_some"
CUT = 100                                                           # rank 0 holds rows [0, 100), rank 1 the other 157
SPLITS = ("uneven", "ignored", "empty")


def _two_rank_case(split):
    c = M.case(TWO_RANK_CASE)
    if split == "ignored":                                          # every target of rank 1's shard is unknown
        valid = c.valid.copy()
        valid[CUT:] = False
        c = c._replace(valid=valid, t=np.where(valid, c.t, np.float32(np.nan)).astype(np.float32))
    return c


def _without_positives(c, cls=5):
    """the case with every valid target of one class set to 0: a class without a positive"""
    t = c.t.copy()
    t[:, cls] = np.where(c.valid[:, cls], np.float32(0.0), t[:, cls])
    return c._replace(t=t)


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
        for split in SPLITS:
            c = _two_rank_case(split)
            n = c.x.shape[0]
            lo, hi = ((0, CUT) if rank == 0 else (CUT, n)) if split != "empty" else ((0, n) if rank == 0 else (n, n))
            x = _logits(c, "float32", dev)[lo:hi].clone().requires_grad_(True)
            y = torch.from_numpy(c.t.copy()).to(dev)[lo:hi]
            loss, per_class = losses.multilabel_loss(x, y, pos_weight=_vec(c.pos_weight, dev), class_weight=_vec(c.class_weight, dev),
                                                     group=dist.group.WORLD, return_per_class=True)
            loss.backward()
            y_w = torch.from_numpy(_without_positives(c).t.copy()).to(dev)[lo:hi]
            weights = losses.class_balance_weights(y_w, group=dist.group.WORLD, max_weight=6.0)
            done[split] = dict(loss=loss.detach().cpu().numpy(), per_class=per_class.cpu().numpy(), grad=x.grad.double().cpu().numpy(),
                               weights=weights.cpu().numpy())
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


def _balance(c, max_weight=None):
    pos = (c.valid & (c.t != 0)).sum(0).astype(np.float64)
    neg = c.valid.sum(0) - pos
    w = np.where(pos > 0, neg / np.maximum(pos, 1.0), 1.0)
    return (w if max_weight is None else np.minimum(w, max_weight)).astype(np.float32)


@pytest.mark.parametrize("split", SPLITS)
def test_two_ranks_equal_one_rank(two_ranks, split):
    """uneven shards with different valid counts, a fully ignored shard, an empty shard: the value is the global loss on both
    ranks (the same bits), and the gradient every rank holds, averaged over the ranks as dp's collectives do, is the one-rank
    gradient -- both inside the bounds of the reference of all rows and of the one-rank run; class_balance_weights too"""
    c = _two_rank_case(split)
    ref = M.reference(c, world=2)
    one_loss, one_pc, one_grad = _python(c, "float32")
    r0, r1 = (r[split] for r in two_ranks)
    assert np.array_equal(r0["loss"], r1["loss"]) and np.array_equal(r0["per_class"], r1["per_class"])
    averaged = np.concatenate((r0["grad"], r1["grad"])) / 2.0
    assert averaged.shape == c.x.shape
    _check(ref, "float32", r0["loss"], r0["per_class"], averaged, f"two ranks, {split} shards")
    M.check_close(r0["loss"], one_loss, ref.loss_bound, "two ranks against one: loss")
    M.check_close(averaged, one_grad, ref.grad_bound, "two ranks against one: gradient")
    assert np.array_equal(r0["weights"], r1["weights"])
    want = _balance(_without_positives(c), 6.0)                     # class 5 has no positive on either rank: weight 1
    assert want[5] == 1.0 and r0["weights"][5] == 1.0 and (want != 1.0).sum() >= 15
    assert np.allclose(r0["weights"], want, rtol=2.0 ** -22, atol=0)


def test_class_balance_weights_on_one_rank():
    from aecf_amd import losses
    c = _without_positives(M.case("bce_w_257x17_some"))               # a class without a positive: weight 1
    t = c.t
    want = _balance(c)
    assert want[5] == 1.0 and (want != 1.0).sum() >= 15
    for labels in (torch.from_numpy(t), torch.from_numpy(np.where(c.valid, t, -1)).to(torch.int8)):
        got = losses.class_balance_weights(labels.to(DEV))
        assert got.dtype == torch.float32 and got.device.type == "cuda" and got.shape == (17,)
        assert np.allclose(got.cpu().numpy(), want, rtol=2.0 ** -22, atol=0)
    clamped = losses.class_balance_weights(torch.from_numpy(t).to(DEV), max_weight=2.5)
    assert np.allclose(clamped.cpu().numpy(), np.minimum(want, np.float32(2.5)), rtol=2.0 ** -22, atol=0)
    hard = torch.from_numpy((np.where(c.valid, t, 0.0) != 0))
    everything = c._replace(valid=np.ones_like(c.valid), t=hard.float().numpy())
    assert np.allclose(losses.class_balance_weights(hard.to(DEV)).cpu().numpy(), _balance(everything), rtol=2.0 ** -22, atol=0)
    with pytest.raises(ValueError, match="max_weight must be a positive number"):
        losses.class_balance_weights(hard.to(DEV), max_weight=0.0)


# ---------------------------------------------------------------------------------------------- the graphed step and the trainer

class _Keeping(torch.nn.Module):
    """a criterion that copies the logits it is handed into a fixed device buffer -- a device copy, which captures -- so that
    after a replay the logits the captured loss was computed from can be read"""

    def __init__(self, inner, rows, classes):
        super().__init__()
        self.inner = inner
        self.kept = torch.zeros(rows, classes, device=DEV)

    def forward(self, logits, labels):
        self.kept.copy_(logits.detach())
        return self.inner(logits, labels)


def test_multilabel_loss_in_a_graphed_train_step():
    """MultilabelLoss (focal with alpha folded in, pos_weight and class_weight: scale vectors that exist only as the module's
    fold) as the criterion of a GraphedTrainStep at batch 64.  The criterion keeps the logits it saw, inside the capture too, so
    the replayed loss is held to the derived bound of the reference on the logits of that replay, as the eager train_step's
    loss is on its own; from the same state and draws the two routes' logits agree to the 1e-4 that
    tests/test_xray_static_gpu.py allows between them.  Between the first and the second replay other weighted losses run --
    another module, the functional form with alpha, a burst of small allocations: the graph holds the addresses of the
    module's own vectors, which must still be there."""
    from aecf_amd import losses
    from aecf_amd.xray import AECFModel, GraphedTrainStep, train_step
    torch.manual_seed(5)
    eager = AECFModel(512, 512, 15).to(DEV).train()
    for m in eager.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    graphed_model = copy.deepcopy(eager)
    gw = torch.Generator().manual_seed(2)
    pos_weight, class_weight = (0.5 + 3.0 * torch.rand(15, generator=gw)).to(DEV), (0.5 + torch.rand(15, generator=gw)).to(DEV)
    form = M.Form(gp=2.0, gn=2.0, alpha=0.25)
    crit = _Keeping(losses.MultilabelLoss(pos_weight=pos_weight, class_weight=class_weight, alpha=0.25, gamma_pos=2.0, gamma_neg=2.0), 64, 15)
    a, b = M.fold(form, pos_weight.cpu().numpy(), class_weight.cpu().numpy(), 15)
    opt_e = torch.optim.AdamW(eager.parameters(), lr=1e-3, weight_decay=0.01)
    opt_g = torch.optim.AdamW(graphed_model.parameters(), lr=1e-3, weight_decay=0.01, capturable=True)
    step = GraphedTrainStep(graphed_model, opt_g, crit, 64, 512, 512, 15, DEV, warmup=2)

    def reference_of_kept(labels):
        seen = crit.kept.cpu().numpy().copy()
        return seen, M.reference(M.Case(form, seen, labels.cpu().numpy(), np.ones((64, 15), dtype=bool), None, None, a, b))

    g = torch.Generator().manual_seed(14)
    for replay in range(2):
        image, text = torch.randn(64, 512, generator=g).to(DEV), torch.randn(64, 512, generator=g).to(DEV)
        labels = (torch.rand(64, 15, generator=g) < 0.2).float().to(DEV)
        if replay == 0:
            loss_e = float(train_step(eager, opt_e, crit, image, text, labels)[0])
            logits_e, ref_e = reference_of_kept(labels)
            ratio_e = M.check_close(loss_e, ref_e.loss, ref_e.loss_bound, "eager step's loss")
        loss_g = float(step(image, text, labels))
        logits_g, ref_g = reference_of_kept(labels)
        ratio_g = M.check_close(loss_g, ref_g.loss, ref_g.loss_bound, f"replay {replay}: the captured loss")
        if replay == 0:
            print(f"mlloss graphed step: error / bound eager={ratio_e:.3f} replayed={ratio_g:.3f}, |loss_g - loss_e| = {abs(loss_g - loss_e):.3e}")
            assert np.abs(logits_g - logits_e).max() <= 1e-4 * max(1.0, np.abs(logits_e).max())
            # other weighted losses: their folds and a burst of small allocations must not reach the captured vectors
            x, y = torch.randn(32, 15, device=DEV), (torch.rand(32, 15, device=DEV) < 0.5).float()
            other = losses.MultilabelLoss(pos_weight=torch.full((15,), 50.0, device=DEV), class_weight=torch.full((15,), 70.0, device=DEV),
                                          alpha=0.9)
            other(x, y)
            losses.multilabel_loss(x, y, alpha=0.6, class_weight=[9.0] * 15, pos_weight=[11.0] * 15)
            junk = [torch.full((15,), 1e6, device=DEV) for _ in range(64)]
            torch.cuda.synchronize()
            del other
    assert len(junk) == 64
    for q in graphed_model.parameters():
        assert torch.isfinite(q).all()


class _TodaysCriterion(torch.nn.Module):
    """the trainer's line as it stands without the flags, behind MultilabelLoss's constructor"""

    def __init__(self, **kw):
        super().__init__()
        self.inner = torch.nn.BCEWithLogitsLoss()

    def forward(self, logits, labels):
        return self.inner(logits.float(), labels)


def test_trainer_with_the_fused_loss(monkeypatch):
    """train_xray.main --loss asymmetric --pos-weight auto for two tiny epochs: finite losses and the usual keys.  Without the
    flags the library's loss is never built and the history is, bit for bit, the history of torch's BCEWithLogitsLoss on
    logits.float() driven through the new branch (--loss bce with the criterion swapped for that line)."""
    from aecf_amd import train_xray
    argv = ["--epochs", "2", "--switch-epoch", "1", "--samples", "320", "--val-samples", "128", "--batch", "64", "--classes", "5"]
    history = train_xray.main(argv + ["--loss", "asymmetric", "--pos-weight", "auto"])
    keys = {"epoch", "curriculum", "train_loss", "gate_entropy", "sec", "val_map", "val_map_no_images", "val_map_no_texts"}
    assert len(history) == 2
    for row in history:
        assert set(row) == keys and math.isfinite(row["train_loss"]) and row["train_loss"] > 0 and 0.0 < row["val_map"] <= 1.0
    built = []
    real = train_xray.MultilabelLoss
    monkeypatch.setattr(train_xray, "MultilabelLoss", lambda **kw: built.append(kw) or real(**kw))
    plain = train_xray.main(argv)
    assert not built
    fused = train_xray.main(argv + ["--loss", "bce"])
    assert len(built) == 1 and built[0]["pos_weight"] is None and (built[0]["gamma_pos"], built[0]["gamma_neg"], built[0]["margin"]) == (0, 0, 0)
    monkeypatch.setattr(train_xray, "MultilabelLoss", _TodaysCriterion)
    today = train_xray.main(argv + ["--loss", "bce"])
    strip = lambda rows: [{k: v for k, v in r.items() if k != "sec"} for r in rows]
    assert strip(plain) == strip(today)
    for r, s in zip(strip(plain), strip(fused)):                    # the fused BCE trains the same model within float32 rounding
        assert abs(r["train_loss"] - s["train_loss"]) <= 1e-3 * r["train_loss"]


@pytest.mark.timeout(600)
def test_trainer_two_ranks_with_the_fused_loss():
    """train_xray --loss asymmetric --pos-weight auto on two ranks: 321 samples at batch 64 leave a last batch of one row, so
    rank 1 holds an empty shard there and only joins the loss's all-reduce and the gradient bucket.  Every rank reports the
    global loss, so the first epoch's train_loss is the one-rank run's within float32 rounding of the two summation orders."""
    import json
    import subprocess
    import sys
    from aecf_amd import train_xray
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    argv = ["--epochs", "3", "--switch-epoch", "2", "--samples", "321", "--val-samples", "128", "--batch", "64", "--classes", "5",
            "--loss", "asymmetric", "--pos-weight", "auto"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    if torch.cuda.device_count() < 2:
        env["AECF_DIST_BACKEND"] = "gloo"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), "-m", "aecf_amd.train_xray"] + argv,
                       env=env, capture_output=True, text=True, timeout=560, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(rows) == 3 and [x["curriculum"] for x in rows] == [False, False, True]
    assert all(math.isfinite(x["train_loss"]) and x["train_loss"] > 0 and 0.0 < x["val_map"] <= 1.0 for x in rows)
    one = train_xray.main(argv)
    assert abs(rows[0]["train_loss"] - one[0]["train_loss"]) <= 2e-3 * one[0]["train_loss"], (rows[0], one[0])
