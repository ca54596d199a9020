"""The supervised contrastive loss with a key queue on the tile GEMMs (EPI_SUP, EPI_SUP_Q, the label-aware kernels of
aecf_nce_gemm.hip) and its labelled ring (aecf_key_queue_push_labeled) against float64 at the tile, shard and ragged edges and where
the count of valid slots crosses a tile, through the C ABI with ctypes and through KeyQueue / queued_supervised_contrastive /
fusion_objective, in a captured step and on two ranks.  Cases, queue plans, label plans, the float64 reference and the derived
elementwise bounds are those of tests/queue_supcon_cases.py (tests/test_queue_supcon_cpu.py shows that the bounds hold an emulation
of the arithmetic and catch the wrong rules).

Every shard of a global n x n problem runs as a rank would: aecf_supcon_queue_pass1, the shards' col_stats added in float32 on the
device (the all-reduce), aecf_supcon_queue_loss, aecf_supcon_queue_grads.  Every output and the workspace come from the Guarded
helper of tests/test_abi_guards_gpu.py: the workspace is exactly the documented size and filled with 0xFF (NaN as bf16 and as
float32) before pass 1, the outputs are filled alike -- a finite output was written and read nothing that was not written first."""
import datetime
import functools
import os
import socket
import traceback

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import queue_nce_cases as Q
from tests import queue_supcon_cases as C
from tests.helpers import record_errors
from tests.test_abi_guards_gpu import Guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, BF16, I64 = torch.float32, torch.bfloat16, torch.int64
HALF = 2.0 ** -8
CASE_PLAN_T = [(cid, pid, T) for cid in C.CASE_IDS for pid in C.PLAN_IDS for T in C.TEMPS]
STATS = ("colsum", "colcnt", "colsx")


def _libs():
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = C.make_case(cid)
    return c["a"].to(DEV), c["b"].to(DEV), c["y"].to(DEV)


@functools.lru_cache(maxsize=None)
def _queue(cid, pid, zero_fill=False, unlabeled=False):
    """(Qa, Qb, Ql on the device, V as a device int64); zero_fill: the slots at or above V hold zeros and -1 in place of the garbage
    rows and the live labels; unlabeled: every stored label negative"""
    qa, qb, ql, V = C.make_queue(cid, pid)
    qa, qb, ql = qa.clone(), qb.clone(), ql.clone()
    if zero_fill:
        qa[V:], qb[V:], ql[V:] = 0, 0, -1
    if unlabeled:
        ql[0::2], ql[1::2] = -1, -7
    return qa.to(DEV), qb.to(DEV), ql.to(DEV), torch.tensor([V], dtype=I64, device=DEV)


@functools.lru_cache(maxsize=None)
def _want(cid, pid, T):
    """(T as the kernels read it, float64 reference, bounds), computed once on the device"""
    c = C.make_case(cid)
    a, b, y = _inputs(cid)
    qa, qb, ql, V = C.make_queue(cid, pid)
    t = C.used_temperature(T)
    ref, bnd = C.reference(a, b, y, qa, qb, ql, V, c["shards"], t, c["coef"], C.score_error(c["a"], c["b"], qa, qb, V))
    return t, ref, bnd


def _run(cid, pid, T, grad_dtype=F32, zero_fill=False, short=False, unlabeled=False):
    """every shard as a rank runs it; outputs laid out as C.reference.  unlabeled: every batch and slot label negative.  short: hand
    the first call a workspace size one byte short and return its status with the buffers it must not have touched."""
    _lib, lib, _ptr, _stream = _libs()
    c = C.make_case(cid)
    a, b, y = _inputs(cid)
    if unlabeled:
        y = torch.where(torch.arange(y.shape[0], device=DEV) % 2 == 0, -1, -7).to(I64)
    qa, qb, ql, qv = _queue(cid, pid, zero_fill, unlabeled)
    q_cap = qa.shape[0]
    n, d = a.shape
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    gd = Guarded(DEV)
    held, stats = [], []
    for lo, hi in c["shards"]:
        rows = hi - lo
        al, bl, yl = a[lo:hi].contiguous(), b[lo:hi].contiguous(), y[lo:hi].contiguous()
        wsb = lib.aecf_supcon_queue_workspace_bytes(rows, n, q_cap, d)
        assert wsb == C.workspace_bytes_py(rows, n, q_cap, d)
        ws = gd.new(wsb, 0xFF)
        cs = gd.tensor((3, n), F32, 0xFF)
        if short:
            status = lib.aecf_supcon_queue_pass1(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(bl), _ptr(qa), _ptr(qb), q_cap,
                                                 _ptr(qv), _ptr(b), _ptr(yl), _ptr(y), _ptr(ql), _ptr(ws), wsb - 1, _ptr(cs), _stream())
            torch.cuda.synchronize()
            gd.check()
            return status, ws, cs
        assert lib.aecf_supcon_queue_pass1(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(bl), _ptr(qa), _ptr(qb), q_cap, _ptr(qv),
                                           _ptr(b), _ptr(yl), _ptr(y), _ptr(ql), _ptr(ws), wsb, _ptr(cs), _stream()) == 0
        held.append((al, bl, yl, ws, wsb))
        stats.append(cs)
    total = stats[0].clone()
    for cs in stats[1:]:
        total += cs                                              # the all-reduce: float32, rank order
    gdt = _lib.AECF_BF16 if grad_dtype == BF16 else _lib.AECF_F32
    lrows = gd.tensor((n,), F32, 0xFF)
    da_loc, db_loc = gd.tensor((n, d), grad_dtype, 0xFF), gd.tensor((n, d), grad_dtype, 0xFF)
    out = dict(colsum=[s[0] for s in stats], colcnt=[s[1] for s in stats], colsx=[s[2] for s in stats], loss_rows=lrows,
               da_loc=da_loc, db_loc=db_loc, db_all=[], dT=[])
    for (lo, hi), (al, bl, yl, ws, wsb) in zip(c["shards"], held):
        rows = hi - lo
        lr_s = gd.tensor((rows,), F32, 0xFF)
        o1, o2, o3 = gd.tensor((rows, d), grad_dtype, 0xFF), gd.tensor((rows, d), grad_dtype, 0xFF), gd.tensor((n, d), grad_dtype, 0xFF)
        d_t = gd.tensor((1,), F32, 0xFF)
        assert lib.aecf_supcon_queue_loss(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(b), q_cap, _ptr(total), _ptr(ws), wsb,
                                          _ptr(lr_s), _stream()) == 0
        assert lib.aecf_supcon_queue_grads(rows, n, lo, d, _ptr(Tt), C.MIN_T, c["coef"], _ptr(al), _ptr(bl), _ptr(qa), _ptr(qb), q_cap,
                                           _ptr(qv), _ptr(b), _ptr(yl), _ptr(y), _ptr(ql), _ptr(ws), wsb, None, gdt, _ptr(o1), _ptr(o2),
                                           _ptr(o3), _ptr(d_t), _stream()) == 0
        torch.cuda.synchronize()
        lrows[lo:hi], da_loc[lo:hi], db_loc[lo:hi] = lr_s, o1, o2
        out["db_all"].append(o3)
        out["dT"].append(float(d_t))
    gd.check()
    return out


@functools.lru_cache(maxsize=None)
def _measured(cid, pid, T):
    return _run(cid, pid, T)


def _tensors(out):
    for name, v in out.items():
        if name != "dT":
            for k, t in enumerate(v if isinstance(v, list) else [v]):
                yield f"{name}[{k}]", t


def _judge(label, cid, pid, T, out, bf16=False):
    """print the line of the profile, record it, assert every output finite and every ratio <= 1 -- no element is skipped; a bound
    of zero (the counts, an empty product, a matched sum without a match) asks for the exact value"""
    _, ref, bnd = _want(cid, pid, T)
    got = dict(out)
    for name, t in _tensors(out):
        assert bool(torch.isfinite(t).all()), (cid, pid, T, name)
    got["db_all_sum"] = sum(g.double() for g in out["db_all"])    # the shares, added in float64 for the comparison
    r = C.ratios(got, ref, bnd, bf16=bf16)
    assert set(r) == set(C.OUTPUTS)
    sig = C.signal(ref, bnd)
    print(f"queue_supcon_parity case {cid} plan {pid} T {T}{label}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items())
          + " | value/bound " + " ".join(f"{n}={sig[n]:.3g}" for n in r))
    record_errors(f"queue_supcon_parity_{cid}_{pid}", T=T, **r)
    for n, v in r.items():
        assert v <= 1.0, (cid, pid, T, label, n, v)


# ---- 1. the C ABI against float64 ----

@pytest.mark.parametrize("cid,pid,T", CASE_PLAN_T)
def test_inside_the_derived_bounds(cid, pid, T):
    """every shard's three column statistics, the loss rows, the three gradients (the shares of the gathered one also added up
    against the summed bounds) and every shard's share of dT, float32 gradients"""
    _judge(" (float32 gradients)", cid, pid, T, _measured(cid, pid, T))


@pytest.mark.parametrize("cid,pid,T", CASE_PLAN_T)
def test_bf16_gradients_inside_the_bounds_and_rounded_once(cid, pid, T):
    """bf16 gradients lie inside the bounds with one rounding more, and have the bits of the float32 outputs rounded to nearest
    even: the two products on d_a_loc were summed in float32 first.  The loss rows, col_stats and dT know no gradient dtype."""
    out, f32 = _run(cid, pid, T, grad_dtype=BF16), _measured(cid, pid, T)
    _judge(" (bf16 gradients)", cid, pid, T, out, bf16=True)
    for (name, x), (_, y) in zip(_tensors(out), _tensors(f32)):
        if name.split("[")[0] in C.GRADS:
            assert x.dtype == BF16 and torch.equal(x, y.to(BF16)), (cid, pid, T, name)
        else:
            assert torch.equal(x, y), (cid, pid, T, name)
    assert out["dT"] == f32["dT"]


# ---- 2. bit identities ----

@pytest.mark.parametrize("cid,pid", [(cid, pid) for cid in C.CASE_IDS for pid in ("Q0", "Q2", "Q3", "Q4")])
def test_without_labels_it_is_queued_info_nce_bit_for_bit(cid, pid):
    """every batch label and every slot label negative (-1 and -7, equal ones among them): the column sums of E, loss rows, the
    three gradients and dT have the bits of aecf_nce_queue_pass1 / _loss / _grads; counts and matched sums are exact zeros"""
    from tests import test_queue_nce_gpu as TQ
    T = 0.07
    got, nce = _run(cid, pid, T, unlabeled=True), TQ._measured(cid, pid, T)
    for k, cs in enumerate(nce["colsum"]):
        assert torch.equal(got["colsum"][k], cs), (cid, pid, k)
        assert bool((got["colcnt"][k] == 0).all()) and bool((got["colsx"][k] == 0).all()), (cid, pid, k)
    for name in ("loss_rows", "da_loc", "db_loc"):
        assert torch.equal(got[name], nce[name]), (cid, pid, name)
    for k, db in enumerate(nce["db_all"]):
        assert torch.equal(got["db_all"][k], db), (cid, pid, k)
    assert got["dT"] == nce["dT"], (cid, pid)


@pytest.mark.parametrize("cid,T", [(cid, T) for cid in C.CASE_IDS for T in C.TEMPS])
def test_empty_queue_has_the_bits_of_the_supervised_tile_form(cid, T):
    """plan Q0 (V = 0, every slot garbage with a live label): the three column statistics, loss_rows, d_a_loc, d_b_all and dT have
    the bits of aecf_supcon_sym_pass1 / _loss / _grads on the same rows and labels, and d_b_loc is exact zeros"""
    from tests import test_supcon_tile_gpu as TS
    got, sup = _measured(cid, "Q0", T), TS._measured(cid, T)
    for name in STATS:
        for k, cs in enumerate(sup[name]):
            assert torch.equal(got[name][k], cs), (cid, name, k)
    assert torch.equal(got["loss_rows"], sup["loss_rows"]) and torch.equal(got["da_loc"], sup["da"]), cid
    for k, db in enumerate(sup["db"]):
        assert torch.equal(got["db_all"][k], db), (cid, k)
    assert got["dT"] == sup["dT"], cid
    assert bool((got["db_loc"] == 0).all())


@pytest.mark.parametrize("cid,pid", [(cid, pid) for cid in ("S2", "S3", "S4") for pid in ("Q0", "Q2", "Q3")])
def test_garbage_and_live_labels_above_the_count_reach_nothing(cid, pid):
    """unit rows and rows of 3e38 with labels live rows carry in the slots at or above V against zeros and -1 there: every output
    has the same bits"""
    T = 0.07
    out, zero = _measured(cid, pid, T), _run(cid, pid, T, zero_fill=True)
    for (name, x), (_, y) in zip(_tensors(out), _tensors(zero)):
        assert torch.equal(x, y), (cid, pid, name)
    assert out["dT"] == zero["dT"]


def test_workspace_one_byte_short_is_refused_with_nothing_written():
    status, ws, cs = _run("S3", "Q3", 0.07, short=True)
    assert status == -4
    assert bool((ws == 0xFF).all()) and bool((cs.view(torch.uint8) == 0xFF).all())


# ---- 3. the labelled ring ----

def _push(lib, _ptr, _stream, q_cap, d, sa, sb, sl, qa, qb, ql, state):
    n = sa.shape[0]
    assert lib.aecf_key_queue_push_labeled(q_cap, d, n, _ptr(sa) if n else None, _ptr(sb) if n else None,
                                           _ptr(sl) if sl is not None and n else None, _ptr(qa), _ptr(qb), _ptr(ql), _ptr(state),
                                           _stream()) == 0


@pytest.mark.parametrize("cid", ["S2", "S3"])
def test_labelled_ring_equals_the_host_model(cid):
    """keys, labels, cursor and valid after Q4's three pushes of 130 rows into 300 slots (wrapped), after a push of more rows than
    the capacity, after a push of no rows, after a push WITHOUT labels (-1 in the slots it fills, the others kept) and a labelled
    one behind it; twice the same pushes give the same bits"""
    _, lib, _ptr, _stream = _libs()
    d = C.make_case(cid)["a"].shape[1]
    q_cap = C.PLANS["Q4"][0]
    g = torch.Generator().manual_seed(7300)
    rows = lambda m: (C._unit(torch.randn(m, d, generator=g)).to(BF16), C._unit(torch.randn(m, d, generator=g)).to(BF16))
    big, bare = rows(q_cap + 77), rows(41)
    big_l = torch.arange(q_cap + 77, dtype=I64) * 3 - 5
    src, lab = Q.push_sources(cid), C.push_labels(cid)
    pushes = [(s, l) for s, l in zip(src, lab)] + [(big, big_l), ((big[0][:0], big[1][:0]), big_l[:0]), (bare, None), (src[0], lab[0])]
    runs = []
    for _ in range(2):
        gd = Guarded(DEV)
        qa, qb, ql = gd.tensor((q_cap, d), BF16, 0), gd.tensor((q_cap, d), BF16, 0), gd.tensor((q_cap,), I64, 0xFF)
        state = gd.tensor((2,), I64, 0)
        ma, mb, ml, ms = torch.zeros(q_cap, d, dtype=BF16), torch.zeros(q_cap, d, dtype=BF16), torch.full((q_cap,), -1, dtype=I64), [0, 0]
        for k, ((sa, sb), sl) in enumerate(pushes):
            _push(lib, _ptr, _stream, q_cap, d, sa.to(DEV), sb.to(DEV), None if sl is None else sl.to(DEV), qa, qb, ql, state)
            C.ring_push(ma, mb, ml, ms, sa, sb, sl)
            torch.cuda.synchronize()
            assert state.tolist() == ms, (cid, k, state.tolist(), ms)
            assert torch.equal(qa.cpu(), ma) and torch.equal(qb.cpu(), mb) and torch.equal(ql.cpu(), ml), (cid, k)
            if k == 2:
                want_a, want_b, want_l, _ = C.make_queue(cid, "Q4")
                assert torch.equal(qa.cpu(), want_a) and torch.equal(qb.cpu(), want_b) and torch.equal(ql.cpu(), want_l)
            if k == 5:
                assert int((ql == -1).sum()) == 41
        gd.check()
        runs.append((qa.clone(), qb.clone(), ql.clone(), state.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*runs))


# ---- 4. the Python surface ----

PY_T = 0.07


@functools.lru_cache(maxsize=None)
def _views():
    """views (n = 300, d = 192) whose normalised rows are case S3's unit rows, scaled by powers of two (exact in bf16), and S3's
    labels"""
    c = C.make_case("S3")
    g = torch.Generator().manual_seed(7401)
    scale = 2.0 ** torch.randint(-1, 3, (c["a"].shape[0], 1), generator=g).float()
    return (c["a"].float() * scale).to(BF16).to(DEV), (c["b"].float() * scale.flip(0)).to(BF16).to(DEV), c["y"].to(DEV)


def _lib_ws(rows, cols, q_cap, d):
    return _libs()[1].aecf_supcon_queue_workspace_bytes(rows, cols, q_cap, d)


def _filled_queue(labels=True):
    """a KeyQueue of 513 slots holding plan Q3's 257 keys and labels of case S3 (pushed as they are), zeros and -1 above them"""
    from aecf_amd import losses
    qa, qb, ql, V = C.make_queue("S3", "Q3")
    queue = losses.KeyQueue(qa.shape[0], qa.shape[1], DEV, labels=labels)
    queue.push(qa[:V].to(DEV), qb[:V].to(DEV), normalize=False, labels=ql[:V].to(DEV) if labels else None)
    return queue


def _surface_ratios(za, zb, y, queue_a, queue_b, queue_l, V, T, loss, dza, dzb, dT):
    """loss, the bf16 gradients of both (unnormalised) views and dT against the float64 reference on the unit rows the kernels
    read (the library's own l2_normalize outputs), taken back through the documented normalise backward: the chain of
    tests/test_queue_nce_gpu.py over this module's reference."""
    from aecf_amd import losses
    from tests.test_nce_stream_gpu import _after_normalise
    n = za.shape[0]
    with torch.no_grad():
        na, nb = losses.l2_normalize(za), losses.l2_normalize(zb)
    t, coef = C.used_temperature(T), 0.5 / n
    ref, bnd = C.reference(na, nb, y, queue_a.to(DEV), queue_b.to(DEV), queue_l.to(DEV), V, [(0, n)], t, coef,
                           C.score_error(na, nb, queue_a, queue_b, V))
    want_loss = coef * float(ref["loss_rows"].sum())
    # the float32 sum of the rows (a tree: fewer than 2^4 roundings) and the product with coef
    b_loss = coef * float(bnd["loss_rows"].sum()) + 2.0 ** -19 * abs(want_loss)
    r = dict(loss=abs(float(loss) - want_loss) / b_loss,
             dT=abs(float(dT) - ref["dT"][0]) / (bnd["dT"][0] + 2.0 ** -23 * abs(ref["dT"][0])))
    for name, z, zn, terms, got in (("dza", za, na, [(ref["da_loc"], bnd["da_loc"])], dza),
                                    ("dzb", zb, nb, [(ref["db_loc"], bnd["db_loc"]), (ref["db_all"][0], bnd["db_all"][0])], dzb)):
        g_ref = sum(v for v, _ in terms)
        e_g = sum(b_ + HALF * (v.abs() + b_) for v, b_ in terms)                # each output rounded to bf16 once
        if len(terms) > 1:
            e_g = e_g + HALF * (sum(v.abs() for v, _ in terms) + e_g)           # one addition in bf16
        inv = 1.0 / z.double().norm(dim=1, keepdim=True)
        want, bound = _after_normalise(zn.double(), inv, g_ref, e_g)
        assert got.dtype == BF16 and bool(torch.isfinite(got).all())
        r[name] = float(((got.double() - want).abs() / (bound + HALF * got.double().abs())).max())
    return r


def test_python_surface_inside_the_bounds():
    """queued_supervised_contrastive on S3's rows and labels against a queue holding Q3's keys and labels, with a tensor
    temperature: loss, both gradients and dT; under torch.no_grad() the value has the same bits; a float temperature gives the
    same bits, and int32 labels those of the same classes as int64"""
    from aecf_amd import losses
    za, zb, y = _views()
    queue = _filled_queue()
    assert queue.state.tolist() == [257, 257] and queue.version == 1
    qa, qb, ql, V = C.make_queue("S3", "Q3")
    assert torch.equal(queue.keys_a[:V].cpu(), qa[:V]) and bool((queue.keys_a[V:] == 0).all())
    assert torch.equal(queue.labels[:V].cpu(), ql[:V]) and bool((queue.labels[V:] == -1).all())
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    Tt = torch.tensor(PY_T, dtype=F32, device=DEV, requires_grad=True)
    loss = losses.queued_supervised_contrastive(a, b, y, queue, temperature=Tt)
    loss.backward()
    with torch.no_grad():
        quiet = losses.queued_supervised_contrastive(za, zb, y, queue, temperature=Tt)
    torch.cuda.synchronize()
    assert torch.equal(quiet, loss.detach()) and not quiet.requires_grad
    a2, b2 = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    plain = losses.queued_supervised_contrastive(a2, b2, y, queue, temperature=PY_T)
    plain.backward()
    assert torch.equal(plain.detach(), loss.detach()) and torch.equal(a2.grad, a.grad) and torch.equal(b2.grad, b.grad)
    with torch.no_grad():                                                   # int32 labels are widened on the device
        small = torch.where(y >= 2 ** 31, y % 97, y)
        assert torch.equal(losses.queued_supervised_contrastive(za, zb, small.to(torch.int32), queue, temperature=PY_T),
                           losses.queued_supervised_contrastive(za, zb, small, queue, temperature=PY_T))
    r = _surface_ratios(za, zb, y, queue.keys_a.cpu(), queue.keys_b.cpu(), queue.labels.cpu(), V, PY_T, loss.detach(), a.grad, b.grad,
                        Tt.grad)
    print(f"queue_supcon_parity queued_supervised_contrastive S3 Q3 T {PY_T}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    record_errors("queue_supcon_python", T=PY_T, **r)
    assert all(v <= 1.0 for v in r.values()), r


def test_python_push_between_forward_and_backward_is_refused():
    from aecf_amd import losses
    za, zb, y = _views()
    queue = _filled_queue()
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    loss = losses.queued_supervised_contrastive(a, b, y, queue)
    queue.push(za, zb, labels=y)
    with pytest.raises(RuntimeError, match="loss, backward, push"):
        loss.backward()


def test_python_second_backward_raises():
    from aecf_amd import losses
    za, zb, y = _views()
    queue = _filled_queue()
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    loss = losses.queued_supervised_contrastive(a, b, y, queue)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="runs once per forward"):
        loss.backward()


def test_python_label_ring_is_asked_for_and_an_unlabelled_queue_keeps_its_call():
    """a queue without a label ring is refused by the loss (ValueError) and refuses labels= (ValueError); its plain push gives the
    bits of a labelled queue's key rings; a labelled queue pushed to without labels holds -1 in the slots that push filled"""
    from aecf_amd import losses
    za, zb, y = _views()
    bare, full = _filled_queue(labels=False), _filled_queue()
    assert bare.labels is None
    with pytest.raises(ValueError, match="label ring"):
        losses.queued_supervised_contrastive(za, zb, y, bare)
    with pytest.raises(ValueError, match="label ring"):
        bare.push(za, zb, labels=y)
    assert bare.version == 1
    bare.push(za, zb)
    full.push(za, zb)                                                      # 300 rows behind 257 into 513 slots: wraps by 44
    torch.cuda.synchronize()
    assert bare.state.tolist() == full.state.tolist() == [44, 513]
    assert torch.equal(bare.keys_a, full.keys_a) and torch.equal(bare.keys_b, full.keys_b)
    _, _, ql, V = C.make_queue("S3", "Q3")
    assert bool((full.labels[V:] == -1).all()) and bool((full.labels[:44] == -1).all())
    assert torch.equal(full.labels[44:V].cpu(), ql[44:V])


def test_python_refuses_what_it_does_not_serve():
    from aecf_amd import losses
    za, zb, y = _views()
    queue = _filled_queue()
    with pytest.raises(NotImplementedError, match="bfloat16"):
        losses.queued_supervised_contrastive(za.float(), zb.float(), y, queue)
    with pytest.raises(NotImplementedError, match="d % 64"):
        losses.queued_supervised_contrastive(za[:, :96].contiguous(), zb[:, :96].contiguous(), y, queue)
    with pytest.raises(NotImplementedError, match="min_temperature"):
        losses.queued_supervised_contrastive(za, zb, y, queue, min_temperature=1e-3)
    with pytest.raises(NotImplementedError, match="key queue of the rows' width"):
        losses.queued_supervised_contrastive(za[:, :128].contiguous(), zb[:, :128].contiguous(), y, queue)
    with pytest.raises(TypeError, match="KeyQueue"):
        losses.queued_supervised_contrastive(za, zb, y, None)
    with pytest.raises(ValueError, match="one class per local row"):
        losses.queued_supervised_contrastive(za, zb, y[:-1], queue)
    with pytest.raises(TypeError, match="int64 or int32"):
        queue.push(za, zb, labels=y.float())
    # the bound on the counts, named: 300 rows + 2^24 - 299 slots.  The refusal comes before any launch and before any buffer is
    # read, so a small queue stands in for 2^24 slots of storage: only its stated capacity is raised.
    wide = losses.KeyQueue(16, 192, DEV, labels=True)
    wide.capacity = 2 ** 24 - 299
    with pytest.raises(NotImplementedError, match=r"capacity <= 2\^24"):
        losses.queued_supervised_contrastive(za, zb, y, wide)
    wide.capacity = 2 ** 24 - 300
    assert _lib_ws(300, 300, wide.capacity, 192) > 0                        # (one slot less is served by the library)


def test_fusion_objective_takes_both_queue_forms():
    """contrastive="queued" and "supervised_queued" give the bits of the direct calls, value and gradients; queue handed to a form
    that takes none, or missing where one is needed, raises ValueError"""
    from aecf_amd import losses
    za, zb, y = _views()
    queue = _filled_queue()
    task = torch.tensor(0.625, device=DEV)

    def both(direct, **kw):
        a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
        want = task + 1.0 * direct(a, b)
        want.backward()
        a2, b2 = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
        got = losses.fusion_objective(task, None, None, a2, b2, temperature=PY_T, queue=queue, **kw)
        got.backward()
        assert torch.equal(got.detach(), want.detach()) and torch.equal(a2.grad, a.grad) and torch.equal(b2.grad, b.grad), kw

    both(lambda a, b: losses.queued_info_nce(a, b, queue, PY_T), contrastive="queued")
    both(lambda a, b: losses.queued_supervised_contrastive(a, b, y, queue, PY_T), contrastive="supervised_queued", labels=y)
    with pytest.raises(ValueError, match="queue is taken by"):
        losses.fusion_objective(task, None, None, za, zb, contrastive="supervised", labels=y, queue=queue)
    with pytest.raises(ValueError, match="needs queue"):
        losses.fusion_objective(task, None, None, za, zb, contrastive="supervised_queued", labels=y)
    with pytest.raises(ValueError, match="needs labels"):
        losses.fusion_objective(task, None, None, za, zb, contrastive="supervised_queued", queue=queue)


# ---- 5. a captured step: forward + backward + labelled push ----

def test_captured_step_follows_labels_changed_in_place():
    """ONE graph holds queued_supervised_contrastive, its backward and the labelled push, starting at V = 0 with 300 slots and 130
    rows.  After each of three replays with fresh rows AND fresh labels written in place, loss and gradients lie inside the bounds
    for the queue and label ring the host model predicts (empty, 130 keys, 260 keys), and the rings equal the model (the third
    push wraps)."""
    from aecf_amd import losses
    n, d, q_cap = 130, 128, 300
    g = torch.Generator().manual_seed(7500)

    def fresh():
        a = C._unit(torch.randn(n, d, generator=g))
        z = C._unit(torch.randn(n, d, generator=g))
        b = 0.8 * a + 0.6 * C._unit(z - (z * a).sum(1, keepdim=True) * a)
        scale = 2.0 ** torch.randint(-1, 3, (n, 1), generator=g).float()
        lab = torch.randint(-2, 20, (n,), generator=g)                     # about 6 rows a class, one row in eleven unlabeled
        return (a * scale).to(BF16).to(DEV), (b * scale.flip(0)).to(BF16).to(DEV), lab.to(I64)

    queue = losses.KeyQueue(q_cap, d, DEV, labels=True)
    za0, zb0, y0 = fresh()
    a, b, y = za0.clone().requires_grad_(True), zb0.clone().requires_grad_(True), y0.to(DEV)
    T = torch.tensor(PY_T, dtype=F32, device=DEV, requires_grad=True)

    def step():
        loss = losses.queued_supervised_contrastive(a, b, y, queue, temperature=T)
        loss.backward()
        queue.push(a, b, labels=y)
        return loss

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            a.grad = b.grad = T.grad = None
            step()
    torch.cuda.current_stream().wait_stream(s)
    a.grad = b.grad = T.grad = None
    with torch.no_grad():                                                   # the warm-up filled the queue: start over at V = 0
        queue.keys_a.zero_(), queue.keys_b.zero_(), queue.state.zero_(), queue.labels.fill_(-1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    torch.cuda.synchronize()
    assert queue.state.tolist() == [0, 0]                                   # (captured, not run)
    ma, mb, ml, ms = torch.zeros(q_cap, d, dtype=BF16), torch.zeros(q_cap, d, dtype=BF16), torch.full((q_cap,), -1, dtype=I64), [0, 0]
    for k in range(3):
        za, zb, lab = fresh()
        with torch.no_grad():
            a.copy_(za), b.copy_(zb), y.copy_(lab)
        graph.replay()
        torch.cuda.synchronize()
        r = _surface_ratios(za, zb, lab.to(DEV), ma, mb, ml, ms[1], PY_T, loss.detach(), a.grad, b.grad, T.grad)
        print(f"queue_supcon_parity captured step, replay {k} (V = {ms[1]}): " + " ".join(f"{x}={v:.3f}" for x, v in r.items()))
        record_errors(f"queue_supcon_capture_{k}", T=PY_T, **r)
        assert all(v <= 1.0 for v in r.values()), (k, r)
        with torch.no_grad():
            na, nb = losses.l2_normalize(za).cpu(), losses.l2_normalize(zb).cpu()
        C.ring_push(ma, mb, ml, ms, na, nb, lab)
        assert queue.state.tolist() == ms, (k, queue.state.tolist(), ms)
        assert torch.equal(queue.keys_a.cpu(), ma) and torch.equal(queue.keys_b.cpu(), mb) and torch.equal(queue.labels.cpu(), ml), k
    assert ms == [90, 300]


# ---- 6. two ranks ----

TWO_RANKS_CAP = 400         # 301 history rows, then the batch's 301: the second push wraps


def _history():
    """the 301 rows of an earlier step (unnormalised) and their labels (the batch's classes, shifted by five rows), dealt over the
    ranks like the batch"""
    from tests import losses_two_ranks_cases as K
    g = torch.Generator().manual_seed(7600)
    return (torch.randn(K.N, K.D, generator=g).to(BF16), torch.randn(K.N, K.D, generator=g).to(BF16), K.label_plan().roll(5))


def _two_ranks_worker(rank, world, port, backend, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from aecf_amd import dp, losses
    from tests import losses_two_ranks_cases as K
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    limit = datetime.timedelta(seconds=90)          # a collective without its partner raises here instead of hanging
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=limit)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=limit)
    done, error = {}, None
    try:
        inp = K.inputs()
        lo, hi = dp.shard_bounds(K.N, rank, world)
        za, zb = inp["za"][lo:hi].to(dev).requires_grad_(True), inp["zb"][lo:hi].to(dev).requires_grad_(True)
        y = inp["labels"][lo:hi].to(dev)
        ha, hb, hl = _history()
        queue = losses.KeyQueue(TWO_RANKS_CAP, K.D, dev, labels=True)
        queue.push(ha[lo:hi].to(dev), hb[lo:hi].to(dev), group=dist.group.WORLD, labels=hl[lo:hi].to(dev))
        T = torch.tensor(K.T0, dtype=F32, device=dev, requires_grad=True)
        loss = losses.queued_supervised_contrastive(za, zb, y, queue, temperature=T, group=dist.group.WORLD)
        loss.backward()
        with torch.no_grad():
            quiet = losses.queued_supervised_contrastive(za, zb, y, queue, temperature=T, group=dist.group.WORLD)
        queue.push(za.detach(), zb.detach(), group=dist.group.WORLD, labels=y)
        torch.cuda.synchronize()
        # gradients follow the data-parallel convention (averaged over ranks later): undo the factor `world`
        done = dict(loss=float(loss.detach()), quiet=float(quiet), dT=float(T.grad / world),
                    dza=(za.grad.float() / world).cpu().numpy(), dzb=(zb.grad.float() / world).cpu().numpy(),
                    keys_a=queue.keys_a.float().cpu().numpy(), keys_b=queue.keys_b.float().cpu().numpy(),
                    labels=queue.labels.cpu().numpy(), state=queue.state.tolist())
    except Exception:
        error = f"rank {rank}:\n{traceback.format_exc()}"
    finally:
        q.put((rank, done, error))
        dist.destroy_process_group()


@pytest.mark.timeout(420)
def test_two_ranks_against_the_one_rank_batch():
    """Two worker processes over uneven shards (151 and 150 of 301 rows): each pushes its rows and labels of an earlier step (the
    queue gathers both), runs queued_supervised_contrastive forward and backward and pushes the batch.  The loss is one number on
    both ranks and the global loss; each rank's gradients are its rows of the float64 reference of the whole batch; the ranks'
    shares of dT add up to it; the value under torch.no_grad() has the same bits; both ranks' rings and states are bit-equal and
    equal the host model.  Bounds: the chain of tests/losses_two_ranks_cases.py (caller_view, ratios) over this module's reference
    with shards = the two ranks."""
    import numpy as np
    from aecf_amd import losses
    from tests import losses_two_ranks_cases as K
    world = K.WORLD
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
        got = sorted([q.get(timeout=300) for _ in range(world)], key=lambda r: r[0])
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
    res = [done for _, done, _ in got]
    inp = K.inputs()
    ha, hb, hl = _history()
    with torch.no_grad():
        na, nb = losses.l2_normalize(inp["za"].to(DEV)).cpu(), losses.l2_normalize(inp["zb"].to(DEV)).cpu()
        nha, nhb = losses.l2_normalize(ha.to(DEV)).cpu(), losses.l2_normalize(hb.to(DEV)).cpu()
    ma, mb, ml, ms = (torch.zeros(TWO_RANKS_CAP, K.D, dtype=BF16), torch.zeros(TWO_RANKS_CAP, K.D, dtype=BF16),
                      torch.full((TWO_RANKS_CAP,), -1, dtype=I64), [0, 0])
    C.ring_push(ma, mb, ml, ms, nha, nhb, hl)
    V = ms[1]
    t, coef = C.used_temperature(K.T0), 0.5 / K.N
    ref, bnd = C.reference(na, nb, inp["labels"], ma, mb, ml, V, K.SHARDS, t, coef * world, C.score_error(na, nb, ma, mb, V))
    scale = lambda v, b: (v / world, b / world)
    laid = dict(a=dict(own=scale(ref["da_loc"], bnd["da_loc"]), shares=None),
                b=dict(own=scale(ref["db_loc"], bnd["db_loc"]), shares=[[scale(v, b)] for v, b in zip(ref["db_all"], bnd["db_all"])]),
                dT=[v / world for v in ref["dT"]], b_dT=[v / world for v in bnd["dT"]])
    laid["loss"] = coef * float(ref["loss_rows"].sum())
    laid["b_loss"] = coef * float(bnd["loss_rows"].sum()) + 2.0 ** -19 * abs(laid["loss"])
    view = K.caller_view(laid, inp["za"], inp["zb"], na, nb)
    assert res[0]["loss"] == res[1]["loss"]
    for r in res:
        assert r["quiet"] == r["loss"]
        r["dza"], r["dzb"] = torch.from_numpy(r["dza"]), torch.from_numpy(r["dzb"])
    ratios = K.ratios(laid, view, res)
    print(f"queue_supcon_parity two ranks N {K.N} d {K.D} T {K.T0} V {V}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    record_errors("queue_supcon_two_ranks", T=K.T0, **ratios)
    assert not K.outside(ratios), ratios
    C.ring_push(ma, mb, ml, ms, na, nb, inp["labels"])
    for r in res:
        assert r["state"] == ms
        assert np.array_equal(r["keys_a"], ma.float().numpy()) and np.array_equal(r["keys_b"], mb.float().numpy())
        assert np.array_equal(r["labels"], ml.numpy())
    assert np.array_equal(res[0]["keys_a"], res[1]["keys_a"]) and np.array_equal(res[0]["labels"], res[1]["labels"])
