"""A learnable InfoNCE temperature: T as a one-element float32 device tensor, read by the kernels (max(T, min_temperature)) and
differentiated by them (aecf_*_dt).  Checked against float64 autograd of the same objective on the same bf16-rounded
unit-norm rows, against the float path bit for bit, under graph capture and over two ranks."""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _views(n, d, dtype=torch.bfloat16, seed=3):
    g = torch.Generator().manual_seed(seed)
    za = torch.randn(n, d, generator=g)
    zb = 0.8 * za + 0.6 * torch.randn(n, d, generator=g)
    return za.to(dtype).to(DEV), zb.to(dtype).to(DEV)


def _ref(na, nb, T, coef=None):
    """float64 symmetric InfoNCE of unit-norm rows (positives on the diagonal) and dL/dT."""
    a, b = na.detach().double(), nb.detach().double()
    t = torch.tensor(float(T), dtype=torch.float64, device=a.device, requires_grad=True)
    s = a @ b.T / t
    i = torch.arange(a.shape[0], device=a.device)
    coef = 0.5 / a.shape[0] if coef is None else coef
    loss = coef * ((torch.logsumexp(s, 1) - s[i, i]).sum() + (torch.logsumexp(s, 0) - s[i, i]).sum())
    loss.backward()
    return loss.item(), t.grad.item()


def _ref_direction(q, k, T, coef):
    """float64 InfoNCE of unit-norm local rows q against the keys k (positives at column i) and dL/dT."""
    a, b = q.detach().double(), k.detach().double()
    t = torch.tensor(float(T), dtype=torch.float64, device=a.device, requires_grad=True)
    s = a @ b.T / t
    i = torch.arange(a.shape[0], device=a.device)
    loss = coef * (torch.logsumexp(s, 1) - s[i, i]).sum()
    loss.backward()
    return loss.item(), t.grad.item()


def _normed(za, zb):
    from aecf_amd import losses
    return losses.l2_normalize(za).detach(), losses.l2_normalize(zb).detach()


def _rel(got, want):
    return abs(got - want) / abs(want)


# measured on the MI355X (relative error of T.grad against float64): sym (333, 256) 6.4e-5, sym (1000, 512) 4.8e-6,
# streaming (333, 256) 6.3e-7, float32 materialising (320, 256) 2.6e-6
@pytest.mark.parametrize("n,d,dtype,min_t,bound", [
    (333, 256, torch.bfloat16, 0.025, 5e-3),        # symmetric tile GEMMs
    (1000, 512, torch.bfloat16, 0.025, 5e-3),
    (333, 256, torch.bfloat16, 0.01, 5e-3),         # min_temperature < 0.025: streaming form
    (320, 256, torch.float32, 0.025, 1e-5),         # float32: materialising form
    ((512, 16385), 128, torch.bfloat16, 0.025, 5e-3),   # (rows, cols): one direction on the streaming workspace; of its 32 key
])                                                      # splits of 544 columns the last is empty
def test_temperature_grad_matches_float64(n, d, dtype, min_t, bound):
    from aecf_amd import losses
    T = torch.tensor(0.07, device=DEV, requires_grad=True)
    if isinstance(n, tuple):
        rows, cols = n
        za, zb = _views(cols, d, dtype)
        q, k = _normed(za[:rows], zb)
        loss = losses._NceDirection.apply(q, k, 0, T, 1.0 / rows, True, min_t)
        want_loss, want_g = _ref_direction(q, k, 0.07, 1.0 / rows)
    else:
        za, zb = _views(n, d, dtype)
        loss = losses.info_nce(za, zb, temperature=T, min_temperature=min_t)
        want_loss, want_g = _ref(*_normed(za, zb), 0.07)
    loss.backward()
    assert T.grad is not None and T.grad.shape == T.shape
    assert _rel(float(loss), want_loss) < (1e-5 if dtype == torch.float32 else 2e-3)
    err = _rel(float(T.grad), want_g)
    print(f"T.grad rel err {err:.2e} ({n}, {d}, {dtype}, min_t {min_t})")
    assert err < bound


def _sym_shards(na, nb, T, bounds, min_t=0.025):
    """The symmetric form on emulated ranks (rows lo:hi each, row offsets, column sums added as the all-reduce would):
    (loss, sum over shards of d_temperature)."""
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    lib = _lib.load()
    n, d = nb.shape
    f32 = dict(dtype=torch.float32, device=DEV)
    parts = []
    for lo, hi in bounds:
        a = na[lo:hi].contiguous()
        wsb = lib.aecf_nce_sym_workspace_bytes(hi - lo, n, d)
        ws, cs = torch.empty(wsb, dtype=torch.uint8, device=DEV), torch.empty(n, **f32)
        _lib.check(lib.aecf_nce_sym_pass1_dt(hi - lo, n, d, _ptr(T), min_t, _ptr(a), _ptr(nb), _ptr(ws), wsb, _ptr(cs), _stream()),
                   "pass1_dt")
        parts.append((lo, hi, a, ws, wsb, cs))
    col = sum(p[5] for p in parts)
    loss, dts = 0.0, []
    for lo, hi, a, ws, wsb, _ in parts:
        rows = torch.empty(hi - lo, **f32)
        _lib.check(lib.aecf_nce_sym_loss_dt(hi - lo, n, lo, d, _ptr(T), min_t, _ptr(a), _ptr(nb), _ptr(col), _ptr(ws), wsb, _ptr(rows),
                                            0, 2, 0.0, None, 1.0, None, None, _stream()), "loss_dt")
        up, dt = torch.ones(1, **f32), torch.empty(1, **f32)
        da = torch.empty(hi - lo, d, dtype=torch.bfloat16, device=DEV)
        db = torch.empty(n, d, dtype=torch.bfloat16, device=DEV)
        _lib.check(lib.aecf_nce_sym_grads_dt(hi - lo, n, lo, d, _ptr(T), min_t, 0.5 / n, _ptr(a), _ptr(nb), _ptr(ws), wsb, _ptr(up),
                                             _lib.AECF_BF16, _ptr(da), _ptr(db), _ptr(dt), _stream()), "grads_dt")
        loss += float(rows.sum()) * 0.5 / n
        dts.append(dt)
    return loss, sum(float(x) for x in dts), [x.clone() for x in dts]


@pytest.mark.parametrize("n,d", [(333, 256), (1000, 512)])
def test_sym_shards_sum_to_the_global_temperature_grad(n, d):
    za, zb = _views(n, d)
    na, nb = _normed(za, zb)
    T = torch.tensor([0.07], device=DEV)
    want_loss, want_g = _ref(na, nb, 0.07)
    cut = n // 3
    loss, g, first = _sym_shards(na, nb, T, [(0, cut), (cut, n)])
    assert _rel(loss, want_loss) < 2e-3
    assert _rel(g, want_g) < 5e-3
    _, g2, again = _sym_shards(na, nb, T, [(0, cut), (cut, n)])
    assert all(torch.equal(x, y) for x, y in zip(first, again))            # fixed-order reductions: same inputs, same bits


def test_logit_scale_chains_through_every_public_entry():
    import aecf_amd
    from aecf_amd import losses
    za, zb = _views(256, 256)
    want_loss, want_g = _ref(*_normed(za, zb), 0.07)
    want = want_g * (-0.07)                                   # dT/dlogit_scale = -T for T = exp(-logit_scale)
    cm = aecf_amd.CurriculumMasking().to(DEV)
    cm._last_seq_len = 3
    ent = torch.rand(256, 1, device=DEV)
    for name in ("info_nce", "contrastive_entropy_loss", "fusion_objective", "contrastive_streaming"):
        ls = torch.tensor(math.log(1 / 0.07), device=DEV, requires_grad=True)
        T = 1 / ls.exp()
        if name == "info_nce":
            loss = losses.info_nce(za, zb, temperature=T)
        elif name == "contrastive_entropy_loss":
            loss = losses.contrastive_entropy_loss(za, zb, cm, ent, temperature=T)
        elif name == "contrastive_streaming":                  # _LossDirection + _NceDirection
            loss = losses.contrastive_entropy_loss(za, zb, cm, ent, temperature=T, min_temperature=0.01)
        else:
            loss = losses.fusion_objective(torch.zeros((), device=DEV), cm, ent, za, zb, temperature=T)
        loss.float().backward()
        assert _rel(float(ls.grad), want) < 5e-3, name


def _grads(fn, za, zb):
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    loss = fn(a, b)
    loss.float().backward()
    return loss.detach(), a.grad, b.grad


@pytest.mark.parametrize("form", ["sym", "streaming", "float32", "loss_streaming"])
def test_tensor_temperature_is_bit_identical_to_float(form):
    import aecf_amd
    from aecf_amd import losses
    dtype = torch.float32 if form == "float32" else torch.bfloat16
    za, zb = _views(320, 256, dtype)
    T = 0.07 if form in ("sym", "float32") else 0.02          # (0.02: the float path takes the streaming form)
    Tt = torch.tensor(T, device=DEV)
    cm = aecf_amd.CurriculumMasking().to(DEV)
    ent = torch.rand(320, 1, device=DEV)
    if form == "loss_streaming":
        f = lambda t, m: (lambda a, b: losses.contrastive_entropy_loss(a, b, cm, ent, temperature=t, min_temperature=m))
    else:
        f = lambda t, m: (lambda a, b: losses.info_nce(a, b, temperature=t, min_temperature=m))
    got = _grads(f(Tt, 0.01 if T < 0.025 else 0.025), za, zb)
    want = _grads(f(T, 0.025), za, zb)
    for x, y in zip(got, want):
        assert torch.equal(x, y), form


def test_below_min_temperature_clamps_and_has_zero_grad():
    from aecf_amd import losses
    za, zb = _views(320, 256)
    T = torch.tensor(0.01, device=DEV, requires_grad=True)
    got = _grads(lambda a, b: losses.info_nce(a, b, temperature=T), za, zb)
    want = _grads(lambda a, b: losses.info_nce(a, b, temperature=0.025), za, zb)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert float(T.grad) == 0.0


def test_captured_step_reads_the_temperature_at_replay():
    import aecf_amd
    from aecf_amd import losses
    za, zb = _views(512, 256)
    cm = aecf_amd.CurriculumMasking().to(DEV)
    ent = torch.rand(512, 1, device=DEV)
    a = za.clone().requires_grad_(True)
    T = torch.tensor(0.07, device=DEV, requires_grad=True)

    def step():
        nb = losses.l2_normalize(zb)
        return losses.gathered_contrastive_entropy_loss(a, nb, 0, cm, ent, temperature=T)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            a.grad = T.grad = None
            step().float().backward()
    torch.cuda.current_stream().wait_stream(s)
    a.grad = T.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
        loss.float().backward()
    with torch.no_grad():
        T.copy_(torch.tensor(0.05))
    graph.replay()
    torch.cuda.synchronize()
    got = (loss.detach().clone(), a.grad.clone(), T.grad.clone())
    a2 = za.clone().requires_grad_(True)
    T2 = torch.tensor(0.05, device=DEV, requires_grad=True)
    want_loss = losses.gathered_contrastive_entropy_loss(a2, losses.l2_normalize(zb), 0, cm, ent, temperature=T2)
    want_loss.float().backward()
    assert torch.equal(got[0], want_loss.detach())
    assert torch.equal(got[1], a2.grad)
    assert torch.equal(got[2], T2.grad)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


N2, D2 = 640, 256


def _two_rank_views():
    g = torch.Generator().manual_seed(4)
    za = torch.randn(N2, D2, generator=g).to(torch.bfloat16)
    zb = (0.7 * za.float() + 0.6 * torch.randn(N2, D2, generator=g)).to(torch.bfloat16)
    return za, zb


def _t_grads(za, zb, lo, dev, nb_all_fn):
    """T.grad of info_nce and of gathered_contrastive_entropy_loss (this rank's rows za, zb)."""
    import aecf_amd
    from aecf_amd import losses
    out = []
    for which in ("info_nce", "gathered"):
        T = torch.tensor(0.07, device=dev, requires_grad=True)
        if which == "info_nce":
            loss = losses.info_nce(za, zb, temperature=T)
        else:
            cm = aecf_amd.CurriculumMasking().to(dev)
            ent = torch.zeros(za.shape[0], 1, device=dev)
            loss = losses.gathered_contrastive_entropy_loss(za, nb_all_fn(losses.l2_normalize(zb)), lo, cm, ent, temperature=T)
        loss.float().backward()
        out.append(T)
    return out


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
        za, zb = _two_rank_views()
        lo, hi = dp.shard_bounds(N2, rank, world)
        ts = _t_grads(za[lo:hi].to(dev), zb[lo:hi].to(dev), lo, dev, lambda nb: dp.all_gather_rows(nb))
        dp.all_reduce_grads(ts)                    # the training loop's reduction (average) on the replicated temperature
        torch.cuda.synchronize()
        q.put((rank, [float(t.grad) for t in ts]))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_temperature_grad_equals_one_rank():
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
    want = [float(t.grad) for t in _t_grads(za.to(DEV), zb.to(DEV), 0, DEV, lambda nb: nb)]
    for rank, got in res:
        for name, g, w in zip(("info_nce", "gathered"), got, want):
            assert _rel(g, w) < 2e-3, (rank, name, g, w)
