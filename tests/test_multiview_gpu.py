"""Multi-view InfoNCE (aecf_nce_multi_pass1 / _loss / _grads, losses.multiview_info_nce) against float64 and against the two-view
entry points, through the C ABI with ctypes, through the Python surface and once through it on two ranks.  Cases, inputs, the float64 reference and the derived
elementwise bounds are those of tests/multiview_cases.py (tests/test_multiview_cpu.py shows that the bounds hold an emulation of
the arithmetic and catch a product on the wrong view, a segment reading the wrong keys, a lost pair and a lost 1 / P).

C ABI: every shard of a global n x n problem as a rank would run it -- pass 1, the shards' [P][n] column sums added in float32
(the all-reduce), the loss, the gradients.  Every output and the workspace come from the Guarded helper of
tests/test_abi_guards_gpu.py, sized exactly as documented and filled with 0xFF (NaN as bf16 and as float32): a finite output was
written, and read nothing that was not written first."""
import functools
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import multiview_cases as C
from tests import nce_tile_cases as N
from tests.test_abi_guards_gpu import Guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
CASE_T = [(cid, T) for cid in C.CASES for T in C.TEMPS]


def _libs():
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


@functools.lru_cache(maxsize=None)
def _want(cid, T):
    c = C.make_case(cid)
    t = N.used_temperature(T)
    ref, bnd = C.reference(c["x"].to(DEV), c["shards"], c["anchor"], t, c["coef"], C.score_errors(cid))
    return t, ref, bnd


def _run_multi(x, shards, anchor, T, coef, grad_dtype=F32, grads=True):
    """Every shard as a rank runs it; outputs laid out as C.reference (the workspace is spent by the gradients)."""
    _lib, lib, _ptr, _stream = _libs()
    n, M, d = x.shape
    k = -1 if anchor is None else anchor
    P = len(C.pairs(M, anchor))
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    gd = Guarded(DEV)
    held, colsum = [], []
    for lo, hi in shards:
        rows = hi - lo
        xl = x[lo:hi].contiguous()
        wsb = lib.aecf_nce_multi_workspace_bytes(rows, n, d, M, k)
        assert wsb == C.workspace_bytes_py(rows, n, d, M, k)
        ws = gd.new(wsb, 0xFF)
        cs = gd.tensor((P, n), F32, 0xFF)
        assert lib.aecf_nce_multi_pass1(rows, n, d, M, k, _ptr(Tt), C.MIN_T, _ptr(xl), _ptr(x), _ptr(ws), wsb, _ptr(cs), _stream()) == 0
        held.append((xl, ws, wsb))
        colsum.append(cs)
    col_total = colsum[0].clone()
    for cs in colsum[1:]:
        col_total += cs
    gdt = _lib.AECF_BF16 if grad_dtype == BF16 else _lib.AECF_F32
    lr, dx = gd.tensor((P, n), F32, 0xFF), gd.tensor((n, M, d), grad_dtype, 0xFF)
    out = dict(colsum=colsum, loss_rows=lr)
    if grads:
        out.update(dx_loc=dx, dx_all=[], dT=[])
    for (lo, hi), (xl, ws, wsb) in zip(shards, held):
        rows = hi - lo
        lr_s = gd.tensor((P, rows), F32, 0xFF)
        assert lib.aecf_nce_multi_loss(rows, n, lo, d, M, k, _ptr(Tt), C.MIN_T, _ptr(xl), _ptr(x), _ptr(col_total), _ptr(ws), wsb,
                                       _ptr(lr_s), _stream()) == 0
        lr[:, lo:hi] = lr_s
        if grads:
            dx_s, dxa_s = gd.tensor((rows, M, d), grad_dtype, 0xFF), gd.tensor((n, M, d), grad_dtype, 0xFF)
            d_t = gd.tensor((1,), F32, 0xFF)
            assert lib.aecf_nce_multi_grads(rows, n, lo, d, M, k, _ptr(Tt), C.MIN_T, coef, _ptr(xl), _ptr(x), _ptr(ws), wsb, None, gdt,
                                            _ptr(dx_s), _ptr(dxa_s), _ptr(d_t), _stream()) == 0
            torch.cuda.synchronize()
            dx[lo:hi] = dx_s
            out["dx_all"].append(dxa_s)
            out["dT"].append(float(d_t))
    torch.cuda.synchronize()
    gd.check()
    return out


def _run_two_view(a, b, shards, T, coef, grad_dtype=F32, grads=True):
    """aecf_nce_sym_pass1_dt / _loss_dt / _grads_dt on contiguous a, b [n, d], shard by shard: colsum, loss_rows, da, db, dT"""
    _lib, lib, _ptr, _stream = _libs()
    n, d = a.shape
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    held, colsum = [], []
    for lo, hi in shards:
        rows = hi - lo
        al = a[lo:hi].contiguous()
        wsb = lib.aecf_nce_sym_workspace_bytes(rows, n, d)
        ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)
        cs = torch.empty(n, dtype=F32, device=DEV)
        assert lib.aecf_nce_sym_pass1_dt(rows, n, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(b), _ptr(ws), wsb, _ptr(cs), _stream()) == 0
        held.append((al, ws, wsb))
        colsum.append(cs)
    col_total = colsum[0].clone()
    for cs in colsum[1:]:
        col_total += cs
    gdt = _lib.AECF_BF16 if grad_dtype == BF16 else _lib.AECF_F32
    out = dict(colsum=colsum, loss_rows=torch.empty(n, dtype=F32, device=DEV), da=torch.empty(n, d, dtype=grad_dtype, device=DEV), db=[], dT=[])
    for (lo, hi), (al, ws, wsb) in zip(shards, held):
        rows = hi - lo
        lr_s = torch.empty(rows, dtype=F32, device=DEV)
        assert lib.aecf_nce_sym_loss_dt(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(b), _ptr(col_total), _ptr(ws), wsb, _ptr(lr_s),
                                        0, 2, 0.0, None, 1.0, None, None, _stream()) == 0
        out["loss_rows"][lo:hi] = lr_s
        if grads:
            da_s, db_s = torch.empty(rows, d, dtype=grad_dtype, device=DEV), torch.empty(n, d, dtype=grad_dtype, device=DEV)
            d_t = torch.empty(1, dtype=F32, device=DEV)
            assert lib.aecf_nce_sym_grads_dt(rows, n, lo, d, _ptr(Tt), C.MIN_T, coef, _ptr(al), _ptr(b), _ptr(ws), wsb, None, gdt,
                                             _ptr(da_s), _ptr(db_s), _ptr(d_t), _stream()) == 0
            out["da"][lo:hi] = da_s
            out["db"].append(db_s)
            out["dT"].append(float(d_t))
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _measured(cid, T, grad_dtype=F32):
    c = C.make_case(cid)
    return _run_multi(c["x"].to(DEV), c["shards"], c["anchor"], T, c["coef"], grad_dtype)


@pytest.mark.parametrize("grad_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cid,T", CASE_T)
def test_c_abi_inside_the_derived_bounds(cid, T, grad_dtype):
    """loss_rows, dx_loc, every shard's dx_all, their sum, the shards' column sums and dT of every case, elementwise"""
    out = _measured(cid, T, grad_dtype)
    _, ref, bnd = _want(cid, T)
    bf16 = grad_dtype == BF16
    got = dict(out)
    for name in ("loss_rows", "dx_loc"):
        assert bool(torch.isfinite(out[name]).all()), (cid, T, name)
    for t in out["colsum"] + out["dx_all"]:
        assert bool(torch.isfinite(t).all()), (cid, T)
    total = sum(g.double() for g in out["dx_all"])
    if not bf16:
        got["dx_all_sum"] = total
    r = C.ratios(got, ref, bnd, bf16=bf16)
    if bf16:
        # a sum of shares rounded to bf16 one by one: every share's rounding joins the summed bounds
        b = bnd["dx_all_sum"] + 2.0 ** -8 * sum(g.double().abs() for g in out["dx_all"])
        err = (total - ref["dx_all_sum"]).abs()
        assert not bool((err[b == 0] != 0).any())
        r["dx_all_sum"] = float((err / b.clamp_min(1e-300)).max())
    print(f"multiview_parity case {cid} T {T} {'bf16' if bf16 else 'f32'}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items()))
    for name, v in r.items():
        assert v <= 1.0, (cid, T, name, v)


@pytest.mark.parametrize("cid", ["V2", "V4"])
def test_every_pair_has_the_bits_of_the_two_view_passes(cid):
    """col_sums[p] and loss_rows[p] against aecf_nce_sym_pass1_dt / _loss_dt on contiguous copies of the two views"""
    c = C.make_case(cid)
    x = c["x"].to(DEV)
    out = _measured(cid, 0.07)
    for p, (m, n) in enumerate(C.pairs(c["views"], c["anchor"])):
        two = _run_two_view(x[:, m].contiguous(), x[:, n].contiguous(), c["shards"], 0.07, c["coef"], grads=False)
        for k in range(len(c["shards"])):
            assert torch.equal(out["colsum"][k][p], two["colsum"][k]), (cid, p, k)
        assert torch.equal(out["loss_rows"][p], two["loss_rows"]), (cid, p)


@pytest.mark.parametrize("grad_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("sid", ["S3", "S4"])
def test_two_views_reduce_to_the_two_view_form(sid, grad_dtype):
    c = N.make_symmetric(sid)
    a, b = c["a"].to(DEV), c["b"].to(DEV)
    x = torch.stack([a, b], dim=1).contiguous()
    two = _run_two_view(a, b, c["shards"], 0.07, c["coef"], grad_dtype)
    out = _run_multi(x, c["shards"], None, 0.07, c["coef"], grad_dtype)
    assert torch.equal(out["loss_rows"][0], two["loss_rows"])
    assert torch.equal(out["dx_loc"][:, 0], two["da"])
    assert not bool(out["dx_loc"][:, 1].any())
    for k in range(len(c["shards"])):
        assert torch.equal(out["colsum"][k][0], two["colsum"][k]), k
        assert torch.equal(out["dx_all"][k][:, 1], two["db"][k]), k
        assert not bool(out["dx_all"][k][:, 0].any())
        assert out["dT"][k] == two["dT"][k], k


@pytest.mark.parametrize("cid", ["V3", "V3A"])
def test_views_without_a_role_are_written_as_zeros(cid):
    """the outputs start as NaN: every element is written, and a view with no pair in a role holds exact zeros"""
    c = C.make_case(cid)
    da, db = C.roles(c["views"], c["anchor"])
    for grad_dtype in (F32, BF16):
        out = _measured(cid, 0.07, grad_dtype)
        assert bool(torch.isfinite(out["dx_loc"]).all())
        for v in range(c["views"]):
            if v not in da:
                assert not bool(out["dx_loc"][:, v].any()), (cid, v)
            else:
                assert bool(out["dx_loc"][:, v].any()), (cid, v)
            for share in out["dx_all"]:
                assert bool(torch.isfinite(share).all())
                assert bool(share[:, v].any()) == (v in db), (cid, v)
    assert sorted(set(range(c["views"])) - set(da)) == ([2] if cid == "V3" else [3])
    assert sorted(set(range(c["views"])) - set(db)) == ([0] if cid == "V3" else [0, 1])


def _definition(x64, t, anchor):
    """float64: (1 / P) sum over the pairs of the symmetric InfoNCE of the normalised views"""
    z = x64 / x64.norm(dim=-1, keepdim=True)
    pr = C.pairs(x64.shape[1], anchor)
    total = 0.0
    for m, n in pr:
        s = z[:, m] @ z[:, n].T / t
        total = total + (torch.logsumexp(s, dim=1) + torch.logsumexp(s, dim=0) - 2.0 * s.diagonal()).sum()
    return total * (0.5 / x64.shape[0] / len(pr))


@pytest.mark.parametrize("shape,anchor", [((300, 3, 192), None), ((257, 8, 128), None), ((300, 4, 192), 2)])
def test_python_surface_against_float64_and_the_loop_of_info_nce(shape, anchor):
    """Value inside the summed per-row bounds (taken on the rows the library normalised); the gradient on x at most 1.5 times as
    far from float64 autograd of the definition as the loop of info_nce over the pairs, which rounds every pair's gradient to
    bf16 before autograd adds them (the 1.5: the noise of a maximum over elements).  Measured on an MI355X, maximum absolute
    error of x.grad, multi-view / loop:  [300, 3, 192] 7.04e-07 / 7.04e-07;  [257, 8, 128] 3.13e-07 / 3.79e-07;  [300, 4, 192]
    anchor 2 4.76e-07 / 4.76e-07 (with at most two partners per view the largest error is the same element in both: it is set by
    the bf16 rounding of the normalised rows and of the final gradient, which both forms share; at 8 views the loop's 7 roundings
    per view show).  dL/dT: 1.1e-04, 7.2e-04 and 2.3e-04 of 6.6, 7.3 and 6.9 in both forms."""
    from aecf_amd import losses
    g = torch.Generator().manual_seed(77 + shape[1])
    b, M, d = shape
    base = torch.randn(b, 1, d, generator=g)
    x0 = ((base + 0.75 * torch.randn(b, M, d, generator=g)) * (1.0 + torch.rand(b, M, 1, generator=g))).to(BF16).to(DEV)
    pr = C.pairs(M, anchor)

    x64 = x0.double().requires_grad_(True)
    t64 = torch.tensor(0.07, dtype=torch.float64, device=DEV, requires_grad=True)
    _definition(x64, t64, anchor).backward()

    x = x0.clone().requires_grad_(True)
    T = torch.tensor(0.07, device=DEV, requires_grad=True)
    loss = losses.multiview_info_nce(x, temperature=T, anchor=anchor)
    loss.backward()
    assert x.grad.dtype == BF16 and x.grad.shape == x.shape and loss.dtype == F32

    xl = x0.clone().requires_grad_(True)
    Tl = torch.tensor(0.07, device=DEV, requires_grad=True)
    loop = sum(losses.info_nce(xl[:, m].contiguous(), xl[:, n].contiguous(), temperature=Tl) for m, n in pr) / len(pr)
    loop.backward()

    with torch.no_grad():
        nx = losses.l2_normalize(x0.reshape(b * M, d)).reshape(b, M, d)
    s_errs = []
    for m, n in pr:
        u, v = nx[:, m].cpu(), nx[:, n].cpu()
        s_errs.append(float(((u.float() @ v.float().T).double() - u.double() @ v.double().T).abs().max()))
    coef = 0.5 / b / len(pr)
    ref, bnd = C.reference(nx, [(0, b)], anchor, N.used_temperature(0.07), coef, tuple(s_errs))
    # the value is float32 loss_rows.sum() * coef: beside the rows' own bounds, a float32 sum of P b <= 2^12 positive terms in a
    # tree of depth <= 14 (a thread's few terms, then the halvings), the rounding of coef and the product: 16 h = 2^-20 of the value
    want = coef * float(ref["loss_rows"].sum())
    slack = coef * float(bnd["loss_rows"].sum()) + 2.0 ** -20 * want
    assert abs(float(loss.detach()) - want) <= slack, (float(loss.detach()), want, slack)

    err = float((x.grad.double() - x64.grad).abs().max())
    err_loop = float((xl.grad.double() - x64.grad).abs().max())
    t_err, t_err_loop = abs(float(T.grad) - float(t64.grad)), abs(float(Tl.grad) - float(t64.grad))
    print(f"multiview_python shape {shape} anchor {anchor}: loss {float(loss.detach()):.6f} (float64 {float(_definition(x0.double(), 0.07, anchor)):.6f}) "
          f"max |d x.grad| {err:.3e} loop {err_loop:.3e} ratio {err / err_loop:.2f} | |d T.grad| {t_err:.3e} loop {t_err_loop:.3e} "
          f"of {float(t64.grad):.3e}")
    assert err <= 1.5 * err_loop, (err, err_loop)

    views = [x0[:, m].clone().requires_grad_(True) for m in range(M)]
    T2 = torch.tensor(0.07, device=DEV, requires_grad=True)
    loss2 = losses.multiview_info_nce(views, temperature=T2, anchor=anchor)
    loss2.backward()
    assert torch.equal(loss2, loss) and torch.equal(T2.grad, T.grad)
    assert torch.equal(torch.stack([v.grad for v in views], dim=1), x.grad)
    with pytest.raises(RuntimeError, match="runs once per forward"):
        l3 = losses.multiview_info_nce(x, temperature=T, anchor=anchor)
        l3.backward(retain_graph=True)
        l3.backward()


def test_refusals_name_the_limit_and_the_loop():
    from aecf_amd import losses
    for bad, what in ((torch.zeros(8, 3, 128, device=DEV), "bfloat16"), (torch.zeros(8, 3, 96, dtype=BF16, device=DEV), "d % 64"),
                      (torch.zeros(8, 3, 4160, dtype=BF16, device=DEV), "4096")):
        with pytest.raises(NotImplementedError, match="loop of info_nce over the pairs") as e:
            losses.multiview_info_nce(bad)
        assert what in str(e.value)
    with pytest.raises(NotImplementedError, match="min_temperature >= 0.025.*loop of info_nce over the pairs"):
        losses.multiview_info_nce(torch.zeros(8, 3, 128, dtype=BF16, device=DEV), min_temperature=0.02)


def test_captured_step_replays_new_inputs_and_temperature():
    from aecf_amd import losses
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(300, 3, 192, generator=g).to(BF16).to(DEV)
    x1 = (torch.randn(300, 1, 192, generator=g) + 0.5 * torch.randn(300, 3, 192, generator=g)).to(BF16).to(DEV)
    x = x0.clone().requires_grad_(True)
    T = torch.tensor(0.07, device=DEV, requires_grad=True)

    def step():
        return losses.multiview_info_nce(x, temperature=T)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            x.grad = T.grad = None
            step().backward()
    torch.cuda.current_stream().wait_stream(s)
    x.grad = T.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
        loss.backward()
    with torch.no_grad():
        T.copy_(torch.tensor(0.05))
        x.copy_(x1)
    graph.replay()
    torch.cuda.synchronize()
    got = (loss.detach().clone(), x.grad.clone(), T.grad.clone())
    x2 = x1.clone().requires_grad_(True)
    T2 = torch.tensor(0.05, device=DEV, requires_grad=True)
    want = losses.multiview_info_nce(x2, temperature=T2)
    want.backward()
    assert torch.equal(got[0], want.detach())
    assert torch.equal(got[1], x2.grad)
    assert torch.equal(got[2], T2.grad)


N2, M2, D2 = 301, 3, 128            # two uneven shards: 151 and 150 rows


def _two_rank_x():
    g = torch.Generator().manual_seed(9)
    return (torch.randn(N2, 1, D2, generator=g) + 0.8 * torch.randn(N2, M2, D2, generator=g)).to(BF16)


def _multiview_worker(rank, world, port, backend, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from aecf_amd import dp, losses
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lo, hi = dp.shard_bounds(N2, rank, world)
        x = _two_rank_x()[lo:hi].to(dev).requires_grad_(True)
        T = torch.tensor(0.07, device=dev, requires_grad=True)
        loss = losses.multiview_info_nce(x, temperature=T)      # one all-gather of the block, one all-reduce of [P, b_all]
        loss.backward()
        torch.cuda.synchronize()
        # gradients follow the data-parallel convention (averaged over ranks later): undo the factor `world`
        q.put((rank, lo, hi, float(loss.detach()), (x.grad.float() / world).cpu().numpy(), float(T.grad) / world))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_equal_one_rank():
    """The data-parallel path of the Python function, as tests/test_dp_gpu.py tests info_nce's and with its tolerances: the loss
    on every rank is the global one, the gradient of a rank's rows and the ranks' shares of dL/dT added up are those of the
    one-rank full batch (the shares of dx_all are rounded to bf16 per rank before the reduce-scatter: 2^-8 of the largest
    element covers them several times)."""
    from aecf_amd import losses
    world = 2
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_multiview_worker, args=(r, world, port, backend, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    x = _two_rank_x().to(DEV).requires_grad_(True)
    T = torch.tensor(0.07, device=DEV, requires_grad=True)
    want = losses.multiview_info_nce(x, temperature=T)
    want.backward()
    for rank, lo, hi, loss, gx, gt in res:
        assert abs(loss - float(want.detach())) < 2e-3 * abs(float(want.detach()))
        rx = x.grad[lo:hi].float().cpu()
        assert (torch.from_numpy(gx) - rx).abs().max() / rx.abs().max() < 2e-2
    assert abs(sum(r[5] for r in res) - float(T.grad)) < 2e-3 * abs(float(T.grad))
