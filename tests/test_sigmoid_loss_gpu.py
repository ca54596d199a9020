"""The pairwise sigmoid (SigLIP) contrastive loss: losses.sigmoid_contrastive and the C ABI behind it (aecf_sig_pass1 /
aecf_sig_grads), with a learnable temperature and bias held in device memory.

The yardstick is float64 autograd of the header's formulas on the same bf16-rounded unit-norm rows the kernels read:

    Tc = max(T, min_temperature);  l_ij = a_i . b_j / Tc + bias;  L = 1/C sum_ij softplus(-y_ij l_ij),  y = +1 on j == off + i, else -1

Bounds are the project's own for the tile-form contrastive kernels (tests/test_nce_gemm_gpu.py, test_nce_temperature_gpu.py):
loss 2e-3, dT and dbias 5e-3, da / db rel_err 1.5e-2 (the weights are rounded once to bf16), loss rows 1e-3."""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.helpers import record_errors, rel_err

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LOSS, SCALAR_GRAD, ROW_GRAD, LOSS_ROWS = 2e-3, 5e-3, 1.5e-2, 1e-3
# (n, d) x (T, bias) whose dT and dbias are well conditioned (|sum terms| / sum |terms| between 0.45 and 1 in float64)
SHAPES = [(333, 256), (1000, 512)]
PARAMS = [(0.1, -10.0), (0.1, -2.0), (0.07, -5.0)]


def _views(n, d, dtype=torch.bfloat16, seed=3):
    """The inputs of tests/test_nce_temperature_gpu.py::_views."""
    g = torch.Generator().manual_seed(seed)
    za = torch.randn(n, d, generator=g)
    zb = 0.8 * za + 0.6 * torch.randn(n, d, generator=g)
    return za.to(dtype).to(DEV), zb.to(dtype).to(DEV)


def _normed(za, zb):
    from aecf_amd import losses
    return losses.l2_normalize(za).detach(), losses.l2_normalize(zb).detach()


def _rel(got, want):
    got, want = (float(x.detach()) if isinstance(x, torch.Tensor) else float(x) for x in (got, want))
    return abs(got - want) / abs(want)


def _ref(a, b, T, bias, off=0, min_t=1e-3, coef=None):
    """float64 autograd of the objective for rows a [R, d] (positives at column off + i) against b [C, d]; a and b may carry a
    graph (see _through_norm).  Returns loss, loss rows (without coef) and the gradients on a, b, T and the bias."""
    a = a.double() if a.requires_grad else a.detach().double().requires_grad_(True)
    b = b.double() if b.requires_grad else b.detach().double().requires_grad_(True)
    t = torch.tensor(float(T), dtype=torch.float64, device=a.device, requires_grad=True)
    bs = torch.tensor(float(bias), dtype=torch.float64, device=a.device, requires_grad=True)
    l = a @ b.T / torch.clamp(t, min=min_t) + bs
    y = -torch.ones_like(l)
    i = torch.arange(a.shape[0], device=a.device)
    y[i, off + i] = 1.0
    terms = torch.nn.functional.softplus(-y * l)
    coef = 1.0 / b.shape[0] if coef is None else coef
    loss = coef * terms.sum()
    ga, gb, gt, gbs = torch.autograd.grad(loss, [a, b, t, bs], retain_graph=True)
    return dict(loss=loss.item(), rows=terms.sum(1).detach(), da=ga, db=gb, dT=gt.item(), dbias=gbs.item(), graph=(loss, a, b))


def _sig_call(a, b, off, T, bias, min_t=1e-3, coef=None, gdt=torch.float32, upstream=None, guard=0):
    """aecf_sig_pass1 + aecf_sig_grads through the C ABI on a workspace of exactly aecf_sig_workspace_bytes (+ guard bytes)."""
    from aecf_amd import _lib
    from aecf_amd.layer import _DTYPES, _ptr, _stream
    lib = _lib.load()
    rows, d = a.shape
    cols = b.shape[0]
    coef = 1.0 / cols if coef is None else coef
    f32 = dict(dtype=torch.float32, device=DEV)
    wsb = lib.aecf_sig_workspace_bytes(rows, cols, d)
    assert wsb > 0
    ws = torch.full((wsb + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    lr, dbias, dT = torch.empty(rows, **f32), torch.empty(1, **f32), torch.empty(1, **f32)
    da, db = torch.empty(rows, d, dtype=gdt, device=DEV), torch.empty(cols, d, dtype=gdt, device=DEV)
    _lib.check(lib.aecf_sig_pass1(rows, cols, off, d, _ptr(T), min_t, _ptr(bias), _ptr(a), _ptr(b), _ptr(ws), wsb, _ptr(lr),
                                  _ptr(dbias), _stream()), "aecf_sig_pass1")
    _lib.check(lib.aecf_sig_grads(rows, cols, off, d, _ptr(T), min_t, coef, _ptr(a), _ptr(b), _ptr(ws), wsb, _ptr(upstream),
                                  _DTYPES[gdt], _ptr(da), _ptr(db), _ptr(dT), _stream()), "aecf_sig_grads")
    torch.cuda.synchronize()
    return dict(rows=lr, loss=float(lr.double().sum()) * coef, dbias=float(dbias) * coef, dT=float(dT), da=da, db=db,
                ws=ws, wsb=wsb, raw=(lr, dbias, dT, da, db))


def _scalars(T, bias):
    return torch.tensor([T], device=DEV), torch.tensor([bias], device=DEV)


# measured on the MI355X (errors against float64, maxima over the six cases): loss 9.0e-8, logit_scale.grad 5.4e-5, bias.grad 6.1e-8,
# za.grad 7.2e-3, zb.grad 7.4e-3 (the last two carry the bf16 rounding of g and of the normalise backward)
@pytest.mark.parametrize("T,bias", PARAMS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_sigmoid_contrastive_matches_float64(n, d, T, bias):
    """sigmoid_contrastive with tensor temperature and bias, gradients on za, zb, logit_scale (T = 1 / exp(ls)) and the bias.
    The float64 reference reads the bf16-rounded unit rows the kernels read and differentiates through a float64 normalise."""
    from aecf_amd import losses
    za, zb = _views(n, d)
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    ls = torch.tensor(math.log(1.0 / T), device=DEV, requires_grad=True)
    bs = torch.tensor(bias, device=DEV, requires_grad=True)
    loss = losses.sigmoid_contrastive(a, b, temperature=1 / ls.exp(), bias=bs)
    loss.backward()
    t_used = float(1 / ls.detach().exp())

    def through_norm(z, unit):                      # value: the bf16 unit rows; gradient: through the float64 normalise
        z64 = z.detach().double().requires_grad_(True)
        u = z64 / z64.norm(dim=1, keepdim=True)
        return z64, u + (unit.double() - u).detach()

    na, nb = _normed(za, zb)
    a64, ua = through_norm(za, na)
    b64, ub = through_norm(zb, nb)
    want = _ref(ua, ub, t_used, bias)
    wa, wb = torch.autograd.grad(want["graph"][0], [a64, b64])
    errs = dict(loss=_rel(loss, want["loss"]), dT=_rel(ls.grad, want["dT"] * (-t_used)), dbias=_rel(bs.grad, want["dbias"]),
                da=rel_err(a.grad, wa), db=rel_err(b.grad, wb))
    print(f"sigmoid parity ({n}, {d}, T {T}, bias {bias}): " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    record_errors("sigmoid_parity", n=n, d=d, T=T, bias=bias, **errs)
    assert errs["loss"] < LOSS
    assert errs["dT"] < SCALAR_GRAD and errs["dbias"] < SCALAR_GRAD
    assert errs["da"] < ROW_GRAD and errs["db"] < ROW_GRAD


def _grads(fn, za, zb):
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    loss = fn(a, b)
    loss.backward()
    return loss.detach(), a.grad, b.grad


def test_float_temperature_and_bias_are_bit_identical_to_tensors():
    from aecf_amd import losses
    za, zb = _views(320, 256)
    got = _grads(lambda a, b: losses.sigmoid_contrastive(a, b, temperature=0.07, bias=-5.0), za, zb)
    T, bs = torch.tensor(0.07, device=DEV), torch.tensor([-5.0], device=DEV)
    want = _grads(lambda a, b: losses.sigmoid_contrastive(a, b, temperature=T, bias=bs), za, zb)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    # fusion_objective routes "sigmoid" to the same loss
    cm_free = _grads(lambda a, b: losses.fusion_objective(torch.zeros((), device=DEV), None, None, a, b, temperature=0.07,
                                                          min_temperature=1e-3, contrastive="sigmoid", bias=-5.0), za, zb)
    for x, y in zip(cm_free, want):
        assert torch.equal(x, y)


def test_below_min_temperature_clamps_and_has_zero_grad():
    from aecf_amd import losses
    za, zb = _views(320, 256)
    T = torch.tensor(0.01, device=DEV, requires_grad=True)
    bs = torch.tensor(-5.0, device=DEV, requires_grad=True)
    got = _grads(lambda a, b: losses.sigmoid_contrastive(a, b, temperature=T, bias=bs, min_temperature=0.05), za, zb)
    want = _grads(lambda a, b: losses.sigmoid_contrastive(a, b, temperature=0.05, bias=-5.0, min_temperature=0.05), za, zb)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert float(T.grad) == 0.0 and float(bs.grad) != 0.0
    ref = _ref(*_normed(za, zb), 0.01, -5.0, min_t=0.05)
    assert _rel(got[0], ref["loss"]) < LOSS and ref["dT"] == 0.0
    assert _rel(bs.grad, ref["dbias"]) < SCALAR_GRAD


# measured on the MI355X (maxima over the five cases): loss rows 4.2e-7, loss 4.2e-7, dbias 5.1e-7, dT 3.2e-4, da 1.4e-3, db 1.7e-3
@pytest.mark.parametrize("rows,cols,off", [(1, 1, 0), (65, 257, 100), (63, 300, 200), (257, 300, 43), (256, 512, 256)])
def test_ragged_shapes_offsets_and_guard_band(rows, cols, off):
    """Row and column counts that fill no tile, positives at an offset: every output against float64 (a padded position that
    entered a sum would add softplus(bias) or a sigmoid to it), and the bytes after the workspace stay as they were."""
    d = 128
    za, zb = _views(cols, d, seed=11)
    na, nb = _normed(za, zb)
    a = na[off:off + rows].contiguous()
    T, bs = _scalars(0.1, -2.0)
    up = torch.tensor([0.75], device=DEV)
    got = _sig_call(a, nb, off, T, bs, upstream=up, guard=4096)
    want = _ref(a, nb, 0.1, -2.0, off=off)
    assert bool((got["ws"][got["wsb"]:] == 0xA5).all())
    errs = dict(rows=rel_err(got["rows"], want["rows"]), loss=_rel(got["loss"], want["loss"]), dbias=_rel(got["dbias"], want["dbias"]),
                dT=_rel(got["dT"], 0.75 * want["dT"]), da=rel_err(got["da"], 0.75 * want["da"]), db=rel_err(got["db"], 0.75 * want["db"]))
    print(f"sigmoid edges ({rows}, {cols}, off {off}): " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    record_errors("sigmoid_edges", n_rows=rows, n_cols=cols, off=off, **errs)
    assert errs["rows"] < LOSS_ROWS and errs["loss"] < LOSS
    assert errs["dbias"] < SCALAR_GRAD and errs["dT"] < SCALAR_GRAD
    assert errs["da"] < ROW_GRAD and errs["db"] < ROW_GRAD


def test_saturated_logits_stay_finite_and_small_sigmoids_survive_bf16():
    """1 / T = 1000 (logits far past the float32 exponent range of exp) and a bias of -30 (sigmoid ~ e^-30): no NaN, and the
    gradients keep their relative accuracy -- nothing underflows in the bf16 g."""
    za, zb = _views(300, 128, seed=5)
    na, nb = _normed(za, zb)
    for T, bias in [(1e-3, 0.0), (1.0, -30.0)]:
        Tt, bs = _scalars(T, bias)
        got = _sig_call(na, nb, 0, Tt, bs)
        want = _ref(na, nb, T, bias)
        assert all(bool(torch.isfinite(x).all()) for x in got["raw"])
        assert _rel(got["loss"], want["loss"]) < LOSS
        assert rel_err(got["da"], want["da"]) < ROW_GRAD and rel_err(got["db"], want["db"]) < ROW_GRAD


# measured on the MI355X ((333, 256) / (1000, 512)): loss 3.2e-8 / 3.4e-8, dbias 3.8e-9 / 1.4e-9, dT 5.4e-5 / 1.1e-5, loss rows 7.0e-7 /
# 1.0e-6, da 1.9e-3 / 1.9e-3, db 1.8e-3 / 2.1e-3
@pytest.mark.parametrize("n,d", SHAPES)
def test_emulated_ranks_sum_to_the_global_values(n, d):
    """Two emulated ranks (rows [0, n/3) and [n/3, n) against all columns), modelled on _sym_shards of the temperature tests:
    nothing is exchanged between the passes, the shares add up to the global float64 values, and a second run gives the same bits."""
    za, zb = _views(n, d)
    na, nb = _normed(za, zb)
    T, bs = _scalars(0.1, -10.0)
    want = _ref(na, nb, 0.1, -10.0)
    cut = n // 3

    def run():
        return [_sig_call(na[lo:hi].contiguous(), nb, lo, T, bs) for lo, hi in [(0, cut), (cut, n)]]

    parts = run()
    errs = dict(loss=_rel(sum(p["loss"] for p in parts), want["loss"]), dbias=_rel(sum(p["dbias"] for p in parts), want["dbias"]),
                dT=_rel(sum(p["dT"] for p in parts), want["dT"]), rows=rel_err(torch.cat([p["rows"] for p in parts]), want["rows"]),
                da=rel_err(torch.cat([p["da"] for p in parts]), want["da"]), db=rel_err(parts[0]["db"] + parts[1]["db"], want["db"]))
    print(f"sigmoid shards ({n}, {d}): " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    record_errors("sigmoid_shards", n=n, d=d, **errs)
    assert errs["loss"] < LOSS and errs["rows"] < LOSS_ROWS
    assert errs["dbias"] < SCALAR_GRAD and errs["dT"] < SCALAR_GRAD
    assert errs["da"] < ROW_GRAD and errs["db"] < ROW_GRAD
    for p, q in zip(parts, run()):                  # fixed-order reductions: same inputs, same bits
        assert all(torch.equal(x, y) for x, y in zip(p["raw"], q["raw"]))


def test_captured_step_reads_temperature_and_bias_at_replay():
    from aecf_amd import losses
    za, zb = _views(512, 256)
    a = za.clone().requires_grad_(True)
    T = torch.tensor(0.1, device=DEV, requires_grad=True)
    bs = torch.tensor(-10.0, device=DEV, requires_grad=True)

    def step():
        return losses.sigmoid_contrastive(a, zb, temperature=T, bias=bs)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            a.grad = T.grad = bs.grad = None
            step().backward()
    torch.cuda.current_stream().wait_stream(s)
    a.grad = T.grad = bs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
        loss.backward()
    with torch.no_grad():
        T.copy_(torch.tensor(0.07))
        bs.copy_(torch.tensor(-5.0))
    graph.replay()
    torch.cuda.synchronize()
    got = (loss.detach().clone(), a.grad.clone(), T.grad.clone(), bs.grad.clone())
    a2 = za.clone().requires_grad_(True)
    T2 = torch.tensor(0.07, device=DEV, requires_grad=True)
    b2 = torch.tensor(-5.0, device=DEV, requires_grad=True)
    want = losses.sigmoid_contrastive(a2, zb, temperature=T2, bias=b2)
    want.backward()
    assert torch.equal(got[0], want.detach())
    assert torch.equal(got[1], a2.grad)
    assert torch.equal(got[2], T2.grad) and torch.equal(got[3], b2.grad)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


N2, D2 = 640, 256
COLLECTIVES = ("all_gather_into_tensor", "all_gather", "all_reduce", "reduce_scatter_tensor", "broadcast", "all_to_all_single")


def _two_rank_views():
    g = torch.Generator().manual_seed(4)
    za = torch.randn(N2, D2, generator=g).to(torch.bfloat16)
    zb = (0.7 * za.float() + 0.6 * torch.randn(N2, D2, generator=g)).to(torch.bfloat16)
    return za, zb


def _step(za, zb, dev):
    """(loss, T, bias, za.grad, zb.grad) of one sigmoid_contrastive step on this rank's rows."""
    from aecf_amd import losses
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    T = torch.tensor(0.1, device=dev, requires_grad=True)
    bs = torch.tensor(-10.0, device=dev, requires_grad=True)
    loss = losses.sigmoid_contrastive(a, b, temperature=T, bias=bs)
    return loss, T, bs, a, b


def _worker(rank, world, port, backend, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from aecf_amd import dp
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        calls = []
        for name in COLLECTIVES:                    # count what the loss issues (dp and losses call them through the module)
            def counted(*args, _fn=getattr(dist, name), _name=name, **kw):
                calls.append((_name, args[0].numel() if isinstance(args[0], torch.Tensor) else -1))
                return _fn(*args, **kw)
            setattr(dist, name, counted)
        za, zb = _two_rank_views()
        lo, hi = dp.shard_bounds(N2, rank, world)
        loss, T, bs, a, b = _step(za[lo:hi].to(dev), zb[lo:hi].to(dev), dev)
        forward = list(calls)
        loss.backward()
        backward = calls[len(forward):]
        del calls[:]
        dp.all_reduce_grads([T, bs])                # the training loop's reduction (average) on the replicated parameters
        torch.cuda.synchronize()
        q.put((rank, float(loss.detach()), float(T.grad), float(bs.grad), (a.grad.float() / world).cpu(), (b.grad.float() / world).cpu(),
               forward, backward))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_equal_one_rank_with_one_gather_and_one_scalar_reduce():
    world = 2
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, backend, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    za, zb = _two_rank_views()
    loss, T, bs, a, b = _step(za.to(DEV), zb.to(DEV), DEV)
    loss.backward()
    half = N2 // world
    for rank, l2, gt, gb, ga, gzb, forward, backward in res:
        assert _rel(l2, loss) < 2e-3                                    # the global value on every rank
        assert _rel(gt, T.grad) < 2e-3 and _rel(gb, bs.grad) < 2e-3     # averaged gradients = one-rank gradients
        # this rank's rows (the local term carries `world`): bf16 gradients of the same float32 sums in another order
        rows = slice(rank * half, (rank + 1) * half)
        assert rel_err(ga, a.grad[rows].float().cpu()) < ROW_GRAD and rel_err(gzb, b.grad[rows].float().cpu()) < ROW_GRAD
        # exactly one all-gather (the rows of view b) and one scalar all-reduce (the returned value) in the forward ...
        assert sorted(n for n, _ in forward) == ["all_gather_into_tensor", "all_reduce"], forward
        assert dict(forward)["all_reduce"] == 1 and dict(forward)["all_gather_into_tensor"] == N2 * D2
        # ... and nothing between the logits pass and the gradient products: the backward's only collective is the gather's own
        # reduce-scatter (an all-reduce + slice where the backend has none)
        assert len(backward) == 1 and backward[0][0] in ("reduce_scatter_tensor", "all_reduce"), backward
        assert backward[0][1] in (N2 * D2, half * D2)


def test_config3_size_against_float64_on_a_subset():
    """BASELINE configs[2]: 8192 local rows (row_offset 8192) against 65536 gathered keys, d = 768.  float64 on a fixed subset:
    the loss rows and da of 64 rows (every column enters them), db of 64 columns (every local row enters them), half of them
    positives' columns.  Measured on the MI355X: loss rows 4.6e-7, da 2.0e-3, db 2.2e-3."""
    from aecf_amd import _lib
    rows, cols, d, off = 8192, 65536, 768, 8192
    need = _lib.load().aecf_sig_workspace_bytes(rows, cols, d)
    if torch.cuda.mem_get_info(DEV)[0] < need + (6 << 30):
        pytest.skip("not enough free device memory for the configs[2]-size block")
    za, zb = _views(cols, d, seed=5)
    na, nb = _normed(za, zb)
    del za, zb
    a = na[off:off + rows].contiguous()
    T, bs = _scalars(0.1, -10.0)
    got = _sig_call(a, nb, off, T, bs)
    assert got["wsb"] < (rows * cols * 2) * 1.25 + (64 << 20)        # g + the float32 split slabs of da + O(rows + cols) partials
    g = torch.Generator().manual_seed(1)
    ri = torch.randperm(rows, generator=g)[:64].sort().values.to(DEV)
    ci = torch.cat([off + ri[:32], torch.randperm(cols, generator=g)[:32].to(DEV)])
    a64, b64 = a.double(), nb.double()

    def g_of(l, r_idx, c_idx):                      # coef / Tc * (sigmoid(l) - [positive]) for rows r_idx x columns c_idx
        pos = (off + r_idx)[:, None] == c_idx[None, :]
        return (torch.sigmoid(l) - pos.double()) / cols / 0.1, pos

    l_r = a64[ri] @ b64.T / 0.1 - 10.0                                 # [64, cols]
    w_r, pos_r = g_of(l_r, ri, torch.arange(cols, device=DEV))
    want_rows = torch.nn.functional.softplus(torch.where(pos_r, -l_r, l_r)).sum(1)
    want_da = w_r @ b64
    l_c = a64 @ b64[ci].T / 0.1 - 10.0                                 # [rows, 64]
    w_c, _ = g_of(l_c, torch.arange(rows, device=DEV), ci)
    want_db = w_c.T @ a64
    errs = dict(rows=rel_err(got["rows"][ri], want_rows), da=rel_err(got["da"][ri], want_da), db=rel_err(got["db"][ci], want_db))
    print("sigmoid configs[2] size: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    record_errors("sigmoid_config3", **errs)
    assert bool(torch.isfinite(got["da"]).all()) and bool(torch.isfinite(got["db"]).all())
    assert errs["rows"] < LOSS_ROWS and errs["da"] < ROW_GRAD and errs["db"] < ROW_GRAD
