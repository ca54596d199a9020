"""The tile-GEMM InfoNCE (aecf_nce_gemm.hip) against float64 at its tile, patch, split and ragged edges, through the C ABI with
ctypes and once through info_nce on two ranks.  Cases, inputs, the float64 reference and the derived elementwise bounds are those
of tests/nce_tile_cases.py (tests/test_nce_tile_cpu.py shows that the bounds hold an emulation of the arithmetic and catch one
lost or doubled key or row).

One direction: aecf_nce_fwd_bwd_dt (min_temperature 0.025, T a device scalar) and aecf_nce_fwd_bwd handed the tile workspace.
Symmetric: every shard of a global n x n problem as a rank would run it -- aecf_nce_sym_pass1[_dt], the shards' column sums added
in float32 (the all-reduce), aecf_nce_sym_loss[_dt], aecf_nce_sym_grads[_dt].

Every output and the workspace come from the Guarded helper of tests/test_abi_guards_gpu.py: the workspace is exactly the
documented size and filled with 0xFF (NaN as bf16 and as float32) before pass 1, the outputs are filled alike -- a finite output
was written and read nothing that was not written first (the padding of E, u and v, the slabs of an empty K split, the tdot
slots that reuse pass 1's row-sum partials)."""
import functools
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import nce_tile_cases as C
from tests.helpers import record_errors
from tests.test_abi_guards_gpu import Guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32 = torch.float32
DIRECTION_T = [(cid, T) for cid in C.DIRECTION for T in C.TEMPS]
SYMMETRIC_T = [(cid, T) for cid in C.SYMMETRIC for T in C.TEMPS]
NAN_WORDS = 0x7FC07FC0                  # another poison: quiet NaNs as bf16 pairs and as float32


def _libs():
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = C.make_case(cid)
    return c["a"].to(DEV), c["b"].to(DEV)


@functools.lru_cache(maxsize=None)
def _want(cid, T, upstream=1.0):
    """(T as the kernels read it, float64 reference, bounds) of a case at coef * upstream, computed once on the device; the score
    error inside the bounds comes from torch's CPU products"""
    c = C.make_case(cid)
    a, b = _inputs(cid)
    t = C.used_temperature(T)
    ref, bnd = C.reference(a, b, c["off"], c["shards"], t, c["coef"] * upstream, c["sym"], C.score_error(cid))
    return t, ref, bnd


def _workspace(gd, rows, cols, d, poison):
    lib = _libs()[1]
    wsb = lib.aecf_nce_sym_workspace_bytes(rows, cols, d)
    assert wsb == C.workspace_bytes_py(rows, cols, d)
    ws = gd.new(wsb, 0xFF)
    if poison != 0xFF:
        ws.view(torch.int32).fill_(poison)
    return ws, wsb


def _run_direction(cid, T, dt=True, poison=0xFF):
    """aecf_nce_fwd_bwd_dt (dt) or aecf_nce_fwd_bwd on the tile workspace; outputs laid out as C.reference"""
    _lib, lib, _ptr, _stream = _libs()
    c = C.make_case(cid)
    a, b = _inputs(cid)
    (rows, d), cols, off = a.shape, b.shape[0], c["off"]
    gd = Guarded(DEV)
    lr, da, db = gd.tensor((rows,), F32, 0xFF), gd.tensor((rows, d), F32, 0xFF), gd.tensor((cols, d), F32, 0xFF)
    d_t = gd.tensor((1,), F32, 0xFF)
    ws, wsb = _workspace(gd, rows, cols, d, poison)
    if dt:
        Tt = torch.tensor([T], dtype=F32, device=DEV)
        status = lib.aecf_nce_fwd_bwd_dt(rows, cols, off, d, _lib.AECF_BF16, _ptr(Tt), C.MIN_T, c["coef"], _ptr(a), _ptr(b), _ptr(lr),
                                         _ptr(da), _ptr(db), _ptr(d_t), _ptr(ws), wsb, _stream())
    else:
        status = lib.aecf_nce_fwd_bwd(rows, cols, off, d, _lib.AECF_BF16, T, c["coef"], _ptr(a), _ptr(b), _ptr(lr), _ptr(da), _ptr(db),
                                      _ptr(ws), wsb, _stream())
    torch.cuda.synchronize()
    assert status == 0
    gd.check()
    out = dict(loss_rows=lr, da=da, db=[db])
    if dt:
        out["dT"] = [float(d_t)]
    return out


def _run_symmetric(cid, T, dt=True, poison=0xFF, grad_dtype=F32, upstream=None):
    """Every shard as a rank runs it: pass 1, the column sums added in float32 in rank order, the loss, the gradients (the
    workspace is spent by them).  dt: the _dt entries (T a device scalar) with each shard's share of dT."""
    _lib, lib, _ptr, _stream = _libs()
    c = C.make_case(cid)
    a, b = _inputs(cid)
    n, d = a.shape
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    up = None if upstream is None else torch.tensor([upstream], dtype=F32, device=DEV)
    gd = Guarded(DEV)
    held, colsum = [], []
    for lo, hi in c["shards"]:
        rows = hi - lo
        al = a[lo:hi].contiguous()
        ws, wsb = _workspace(gd, rows, n, d, poison)
        cs = gd.tensor((n,), F32, 0xFF)
        if dt:
            status = lib.aecf_nce_sym_pass1_dt(rows, n, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(b), _ptr(ws), wsb, _ptr(cs), _stream())
        else:
            status = lib.aecf_nce_sym_pass1(rows, n, d, T, _ptr(al), _ptr(b), _ptr(ws), wsb, _ptr(cs), _stream())
        assert status == 0
        held.append((al, ws, wsb))
        colsum.append(cs)
    col_total = colsum[0].clone()
    for cs in colsum[1:]:
        col_total += cs
    gdt = _lib.AECF_BF16 if grad_dtype == torch.bfloat16 else _lib.AECF_F32
    lr, da = gd.tensor((n,), F32, 0xFF), gd.tensor((n, d), grad_dtype, 0xFF)
    out = dict(colsum=colsum, loss_rows=lr, da=da, db=[])
    if dt:
        out["dT"] = []
    for (lo, hi), (al, ws, wsb) in zip(c["shards"], held):
        rows = hi - lo
        lr_s, da_s, db_s = gd.tensor((rows,), F32, 0xFF), gd.tensor((rows, d), grad_dtype, 0xFF), gd.tensor((n, d), grad_dtype, 0xFF)
        d_t = gd.tensor((1,), F32, 0xFF)
        if dt:
            status = lib.aecf_nce_sym_loss_dt(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(b), _ptr(col_total), _ptr(ws), wsb,
                                              _ptr(lr_s), 0, 2, 0.0, None, 1.0, None, None, _stream())
            assert status == 0
            status = lib.aecf_nce_sym_grads_dt(rows, n, lo, d, _ptr(Tt), C.MIN_T, c["coef"], _ptr(al), _ptr(b), _ptr(ws), wsb, _ptr(up),
                                               gdt, _ptr(da_s), _ptr(db_s), _ptr(d_t), _stream())
        else:
            status = lib.aecf_nce_sym_loss(rows, n, lo, d, T, _ptr(al), _ptr(b), _ptr(col_total), _ptr(ws), wsb, _ptr(lr_s), 0, 2, 0.0,
                                           None, 1.0, None, None, _stream())
            assert status == 0
            status = lib.aecf_nce_sym_grads(rows, n, lo, d, T, c["coef"], _ptr(al), _ptr(b), _ptr(ws), wsb, _ptr(up), gdt, _ptr(da_s),
                                            _ptr(db_s), _stream())
        assert status == 0
        torch.cuda.synchronize()
        lr[lo:hi], da[lo:hi] = lr_s, da_s
        out["db"].append(db_s)
        if dt:
            out["dT"].append(float(d_t))
    gd.check()
    return out


@functools.lru_cache(maxsize=None)
def _measured(cid, T, dt=True):
    return (_run_symmetric if cid in C.SYMMETRIC else _run_direction)(cid, T, dt=dt)


def _tensors(out):
    for name, v in out.items():
        if name != "dT":
            for k, t in enumerate(v if isinstance(v, list) else [v]):
                yield f"{name}[{k}]", t


def _judge(label, cid, T, out, bf16=False, upstream=1.0):
    """print the line of the profile, record it, assert every ratio <= 1 and every output finite"""
    _, ref, bnd = _want(cid, T, upstream)
    got = dict(out)
    for name, t in _tensors(out):
        assert bool(torch.isfinite(t).all()), (cid, T, name)
    if not bf16:
        got["db_sum"] = sum(g.double() for g in out["db"])
    r = C.ratios(got, ref, bnd, bf16=bf16)
    if bf16:
        # a sum of shares rounded to bf16 one by one: every share's rounding joins the summed bounds
        total = sum(g.double() for g in out["db"])
        r["db_sum"] = float(((total - ref["db_sum"]).abs() / (bnd["db_sum"] + 2.0 ** -8 * sum(g.double().abs() for g in out["db"]))).max())
    sig = C.signal(ref, bnd)
    print(f"nce_tile_parity case {cid} T {T}{label}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items())
          + " | value/bound " + " ".join(f"{n}={sig[n]:.3g}" for n in r))
    record_errors(f"nce_tile_parity_{cid}", T=T, **r)
    for n, v in r.items():
        assert v <= 1.0, (cid, T, label, n, v)
    return r


@pytest.mark.parametrize("cid,T", DIRECTION_T)
def test_direction_inside_the_derived_bounds(cid, T):
    """aecf_nce_fwd_bwd_dt with the tile workspace: loss_rows, dq, dk and dT of every case, elementwise"""
    _judge(" (aecf_nce_fwd_bwd_dt)", cid, T, _measured(cid, T))


@pytest.mark.parametrize("cid,T", DIRECTION_T)
def test_direction_float_entry_gives_the_same_bits(cid, T):
    """aecf_nce_fwd_bwd (T a host float) on the same workspace size: the tile form again, bit for bit"""
    one, two = _measured(cid, T), _measured(cid, T, dt=False)
    for (name, x), (_, y) in zip(_tensors(one), _tensors(two)):
        assert torch.equal(x, y), (cid, T, name)


@pytest.mark.parametrize("cid,T", SYMMETRIC_T)
def test_symmetric_inside_the_derived_bounds(cid, T):
    """the _dt entries over every shard: column sums, loss rows, da, the share of db and of dT per shard, and the shares of db
    added up against the summed bounds"""
    _judge(" (aecf_nce_sym_*_dt)", cid, T, _measured(cid, T))


@pytest.mark.parametrize("cid,T", SYMMETRIC_T)
def test_symmetric_float_entries_give_the_same_bits(cid, T):
    one, two = _measured(cid, T), _measured(cid, T, dt=False)
    for (name, x), (_, y) in zip(_tensors(one), _tensors(two)):
        assert torch.equal(x, y), (cid, T, name)


@pytest.mark.parametrize("cid", ["D2", "D3", "S6"])
def test_another_poison_gives_the_same_bits(cid):
    """The empty-split and one-step-split cases once more on a workspace filled with other NaNs: nothing is read before it is
    written, so the bits cannot move (dT included: the tdot slots of an empty split hold what this call stored there)."""
    T = 0.07
    one = _measured(cid, T)
    two = (_run_symmetric if cid in C.SYMMETRIC else _run_direction)(cid, T, poison=NAN_WORDS)
    for (name, x), (_, y) in zip(_tensors(one), _tensors(two)):
        assert torch.equal(x, y), (cid, name)
    assert one["dT"] == two["dT"] and all(math.isfinite(v) for v in two["dT"])


@pytest.mark.parametrize("cid", ["S3", "S6"])
def test_symmetric_bf16_gradients_scaled_on_the_device(cid):
    """aecf_nce_sym_grads with bf16 outputs and an upstream of 0.375 in device memory, after a fresh pass 1 and loss: inside the
    bounds taken at coef * 0.375 plus 2^-8 |value|.  S3: one K split, the da GEMM rounds and stores; S6: the slab sum rounds."""
    T, up = 0.07, 0.375
    out = _run_symmetric(cid, T, dt=False, grad_dtype=torch.bfloat16, upstream=up)
    assert out["da"].dtype == torch.bfloat16
    plain = _measured(cid, T, dt=False)
    assert torch.equal(out["loss_rows"], plain["loss_rows"])               # (the loss knows no upstream)
    _judge(" (aecf_nce_sym_grads, bf16, upstream 0.375)", cid, T, out, bf16=True, upstream=up)


# ---- the entropy regulariser riding in aecf_nce_sym_loss ----

def _entropy_values(n, special):
    g = torch.Generator().manual_seed(177 + n)
    h = torch.rand(n, generator=g) * 1.2
    if n >= 3:
        h[0], h[n // 2], h[n - 1] = float("nan"), float("inf"), float("-inf")
    elif special is not None:
        h[0] = special
    return h


@functools.lru_cache(maxsize=None)
def _rider_stage(cid, T):
    """pass 1 of a one-shard case on a poisoned workspace and the loss without the rider"""
    _lib, lib, _ptr, _stream = _libs()
    a, b = _inputs(cid)
    n, d = a.shape
    gd = Guarded(DEV)
    ws, wsb = _workspace(gd, n, n, d, 0xFF)
    cs, lr = gd.tensor((n,), F32, 0xFF), gd.tensor((n,), F32, 0xFF)
    assert lib.aecf_nce_sym_pass1(n, n, d, T, _ptr(a), _ptr(b), _ptr(ws), wsb, _ptr(cs), _stream()) == 0
    assert lib.aecf_nce_sym_loss(n, n, 0, d, T, _ptr(a), _ptr(b), _ptr(cs), _ptr(ws), wsb, _ptr(lr), 0, 3, 0.7, None, 0.5, None, None,
                                 _stream()) == 0
    torch.cuda.synchronize()
    gd.check()
    return gd, ws, wsb, cs, lr


@pytest.mark.parametrize("last_seq_len", [1, 3])
@pytest.mark.parametrize("n_entropy", [1, 255, 256, 257, 1000])
def test_entropy_rider(n_entropy, last_seq_len):
    """aecf_nce_sym_loss on case S3: entropy_loss = max(mean((nan_to_num(H) - target)^2), 0) and d_entropy = upstream * 2 / n *
    (H - target) (0 at non-finite entries) against float64 to a relative 2^-20 -- at most 16 float32 roundings for n <= 1000 in 256
    strided sums plus the tree -- with NaN, +inf and -inf among the entries (n = 1: each of them, and a finite one, in turn); the
    loss rows are the bits of the call without the rider, which are the bits test_symmetric_inside_the_derived_bounds judged."""
    _lib, lib, _ptr, _stream = _libs()
    cid, T, target_frac, upstream = "S3", 0.07, 0.7, 0.5
    a, b = _inputs(cid)
    n, d = a.shape
    _, ws, wsb, cs, plain = _rider_stage(cid, T)
    assert torch.equal(plain, _measured(cid, T, dt=False)["loss_rows"])
    target = float(torch.tensor((math.log(last_seq_len) if last_seq_len > 1 else 0.0) * target_frac, dtype=F32))
    for special in ([None] if n_entropy >= 3 else [None, float("nan"), float("inf"), float("-inf")]):
        h = _entropy_values(n_entropy, special)
        gd = Guarded(DEV)
        lr, e_loss, d_ent = gd.tensor((n,), F32, 0xFF), gd.tensor((1,), F32, 0xFF), gd.tensor((n_entropy,), F32, 0xFF)
        hd = h.to(DEV)
        status = lib.aecf_nce_sym_loss(n, n, 0, d, T, _ptr(a), _ptr(b), _ptr(cs), _ptr(ws), wsb, _ptr(lr), n_entropy, last_seq_len,
                                       target_frac, _ptr(hd), upstream, _ptr(e_loss), _ptr(d_ent), _stream())
        torch.cuda.synchronize()
        assert status == 0
        gd.check()
        h64 = h.double()
        delta = torch.nan_to_num(h64, nan=0.0, posinf=1.0, neginf=0.0) - target
        want_loss = max(float((delta * delta).mean()), 0.0)
        want_d = torch.where(torch.isfinite(h64), upstream * 2.0 / n_entropy * delta, torch.zeros_like(delta))
        got_d = d_ent.cpu().double()
        assert abs(float(e_loss) - want_loss) <= 2.0 ** -20 * want_loss, (n_entropy, last_seq_len, special, float(e_loss), want_loss)
        assert bool(((got_d - want_d).abs() <= 2.0 ** -20 * want_d.abs()).all()), (n_entropy, last_seq_len, special)
        assert bool((got_d[~torch.isfinite(h64)] == 0).all())
        assert torch.equal(lr, plain), (n_entropy, last_seq_len, special)


# ---- the Python surface: info_nce on two ranks with uneven shards ----

NCE_N, NCE_D, NCE_SHARDS, NCE_T = 513, 128, [(0, 300), (300, 513)], 0.07


def _info_nce_views():
    """views whose normalised rows are the twin-carrying unit rows of make_rows, scaled by powers of two (exact in bf16)"""
    a, b, _ = C.make_rows(NCE_N, NCE_D, NCE_SHARDS, 5200)
    g = torch.Generator().manual_seed(5201)
    scale = 2.0 ** torch.randint(-1, 3, (NCE_N, 1), generator=g).float()
    return (a.float() * scale).to(torch.bfloat16), (b.float() * scale.flip(0)).to(torch.bfloat16)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _info_nce_worker(rank, world, port, backend, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from aecf_amd import losses
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        za, zb = _info_nce_views()
        lo, hi = NCE_SHARDS[rank]
        a = za[lo:hi].to(dev).requires_grad_(True)
        b = zb[lo:hi].to(dev).requires_grad_(True)
        Tt = torch.tensor(NCE_T, dtype=F32, device=dev, requires_grad=True)
        loss = losses.info_nce(a, b, temperature=Tt)
        loss.backward()
        torch.cuda.synchronize()
        # gradients follow the data-parallel convention (averaged over ranks later): undo the factor `world` (a power of two)
        q.put((rank, float(loss.detach()), (a.grad.float() / world).cpu().numpy(), (b.grad.float() / world).cpu().numpy(),
               float(Tt.grad) / world))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_info_nce_two_ranks_uneven_shards_tensor_temperature():
    """info_nce with a tensor temperature on two ranks holding 300 and 213 rows of a 513 x 128 problem (the second rank's block
    ends at the last column: row_offset + rows == cols): the loss every rank reports, each rank's rows of dza and dzb and the
    ranks' shares of dT against the float64 global objective on the unit rows the kernels read, taken back through the
    documented normalise backward.  Bounds: the da / db bounds at coef = 0.5 / n plus 2^-8 |value| for each bf16 output, the bf16
    sum of the two ranks' shares of db (one more rounding), _after_normalise of tests/test_nce_stream_gpu.py, the rounding of
    the result.  na and nb are the library's own l2_normalize outputs: the normalise forward is not this file's subject."""
    from aecf_amd import losses
    from tests.test_nce_stream_gpu import _after_normalise
    world = 2
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_info_nce_worker, args=(r, world, port, backend, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    za, zb = (z.to(DEV) for z in _info_nce_views())
    with torch.no_grad():
        na, nb = losses.l2_normalize(za), losses.l2_normalize(zb)
    t, coef, half = C.used_temperature(NCE_T), 0.5 / NCE_N, 2.0 ** -8
    s_err = float((na.cpu().float() @ nb.cpu().float().T - na.cpu().double() @ nb.cpu().double().T).abs().max())
    ref, bnd = C.reference(na, nb, 0, NCE_SHARDS, t, coef, 1, s_err)
    want_loss = coef * float(ref["loss_rows"].sum())
    # each rank's float32 sum of its rows (a tree: fewer than 2^4 roundings), the sum over ranks and the two operations that
    # hand every rank the global value
    b_loss = coef * float(bnd["loss_rows"].sum()) + 2.0 ** -19 * abs(want_loss)
    r = dict(loss=max(abs(x[1] - want_loss) for x in res) / b_loss)
    r["dT"] = max(abs(x[4] - ref["dT"][k]) / (bnd["dT"][k] + 2.0 ** -23 * abs(ref["dT"][k])) for k, x in enumerate(res))
    r["dT_sum"] = abs(sum(x[4] for x in res) - sum(ref["dT"])) / (sum(bnd["dT"]) + 2.0 ** -23 * abs(sum(ref["dT"])))
    e_da = bnd["da"] + half * (ref["da"].abs() + bnd["da"])
    e_sh = [b_ + half * (v.abs() + b_) for v, b_ in zip(ref["db"], bnd["db"])]
    e_db = sum(e_sh) + half * (ref["db_sum"].abs() + sum(e_sh))
    sig = {}
    for name, z, zn, g_ref, e_g, col in (("dza", za, na, ref["da"], e_da, 2), ("dzb", zb, nb, ref["db_sum"], e_db, 3)):
        inv = 1.0 / z.double().norm(dim=1, keepdim=True)
        want, bound = _after_normalise(zn.double(), inv, g_ref, e_g)
        got = torch.cat([torch.from_numpy(x[col]) for x in res], 0).to(DEV).double()
        assert got.shape == want.shape and bool(torch.isfinite(got).all())
        r[name] = float(((got - want).abs() / (bound + half * got.abs())).max())
        sig[name] = float((want.abs() / (bound + half * got.abs())).max())
    print(f"nce_tile_parity info_nce two ranks 300 + 213 of n {NCE_N} d {NCE_D} T {NCE_T} ({backend}): "
          + " ".join(f"{k}={v:.3f}" for k, v in r.items())
          + f" | value/bound loss={abs(want_loss) / b_loss:.3g} dT_sum={abs(sum(ref['dT'])) / sum(bnd['dT']):.3g} "
          + " ".join(f"{k}={v:.3g}" for k, v in sig.items()))
    record_errors("nce_tile_python_info_nce", T=NCE_T, **r)
    assert all(v <= 1.0 for v in r.values()), r
