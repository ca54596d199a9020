"""FusedAdamW(ema_decay=...): the moving average kept in the step's own launch (aecf_adamw_mp_ema_step, aecf_ema_update)
against its float64 restatement (tests/ema_cases.py).  A multi-step check restates each step from the GPU's own previous
average and the weight the step STORED, so the bound is the single-step one: 2^-24 (om |w' - e| + |E|) 1.01 + 2^-126.
Shapes: 1, 7, 8, 9, 2047, 2048, 2049, 4097 elements (a lane's 8 and a block's 2048 from both sides, two blocks and a tail),
one empty tensor, one view offset by one element (the scalar path), 26 tensors in all (25 non-empty: a second launch group);
the C-ABI test adds a tensor whose ``ema`` is NULL."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import ema_cases as E

pytestmark = pytest.mark.gpu

HYPER = dict(betas=(0.9, 0.98), eps=1e-8, weight_decay=0.05)
LR = 3e-3
NUMELS = list(E.SIZES) + [0, 2049] + [17 + i for i in range(15)]      # index 9 is the offset view
VIEW = 9
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
# (parameter dtype, masters, gradient dtype; None: the parameter's)
CONFIGS = [(F32, False, None), (BF, True, None), (BF, True, F32), (BF, False, None), (BF, False, F32), (F16, False, None),
           (F16, False, F32)]
_ids = lambda c: f"{str(c[0])[6:]}{'+master' if c[1] else ''}-g{'param' if c[2] is None else 'f32'}"
npf = lambda t: t.detach().float().cpu().numpy()


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


class Bag(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t) for t in tensors])


def _tensors(dev, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(NUMELS):
        t = torch.randn(n + (i == VIEW), generator=g).to(dev, dtype)
        out.append(t[1:] if i == VIEW else t)         # contiguous, 4 or 2 bytes off a 16-byte boundary
    assert out[VIEW].data_ptr() % 16 != 0 and out[VIEW].is_contiguous()
    return out


def _grads(ps, gen, dtype, scale=1.0, skip=()):
    out = []
    for i, p in enumerate(ps):
        out.append(None if i in skip else (torch.randn(p.shape, generator=gen) * scale).to(p.device, dtype or p.dtype))
    return out


def _set(ps, grads):
    for p, g in zip(ps, grads):
        p.grad_dtype = None                           # (a float32 gradient beside a 16-bit parameter)
        p.grad = None if g is None else g.clone()


def _stored(opt, p):
    """The weight as the step stored it, in float32."""
    return opt.state[p].get("master", p).detach().float()


def _inside(opt, ps, before, beta, where):
    """Every average inside the single-step bound from (its value before the step, the stored weight after it)."""
    worst = 0.0
    for i, p in enumerate(ps):
        if p.numel() == 0:
            continue
        x = E.excess(npf(opt.state[p]["ema"]), npf(_stored(opt, p)), before[i], beta)
        assert x <= 1.0, (where, i, x)
        worst = max(worst, x)
    return worst


def _emas(opt, ps):
    return [npf(opt.state[p]["ema"]) if "ema" in opt.state[p] else npf(_stored(opt, p)) for p in ps]


@pytest.mark.parametrize("beta", E.BETAS)
@pytest.mark.parametrize("config", CONFIGS, ids=_ids)
def test_bounds_rounding_and_the_twin_without_ema(config, beta):
    """1. five steps: every ema element inside the bound, ema_out == ema.to(dtype), everything else bit-equal to a twin."""
    from aecf_amd.optim import EmaModel, FusedAdamW
    dev = _dev()
    dtype, masters, gdt = config
    bag = Bag(_tensors(dev, dtype, 1))
    ps = list(bag.ps)
    twin = [p.detach().clone().requires_grad_() for p in ps]
    lr = lambda: torch.tensor(LR, device=dev)         # (a tensor lr: the twin takes aecf_adamw_mp_step for float32 too)
    opt = FusedAdamW(ps, lr=lr(), master_weights=masters, ema_decay=beta, **HYPER)
    ot = FusedAdamW(twin, lr=lr(), master_weights=masters, **HYPER)
    ema = EmaModel(bag, opt)
    g = torch.Generator().manual_seed(2)
    worst = 0.0
    for step in range(5):
        grads = _grads(ps, g, gdt, 10.0 ** (step % 3 - 1))
        _set(ps, grads)
        _set(twin, grads)
        before = _emas(opt, ps)
        versions = [q._version for q in ema.module.ps]
        opt.step()
        ot.step()
        worst = max(worst, _inside(opt, ps, before, beta, step))
        for i, (p, t, q) in enumerate(zip(ps, twin, ema.module.ps)):
            if p.numel() == 0:
                continue
            st, tt = opt.state[p], ot.state[t]
            assert torch.equal(p, t), (step, i)
            for key in ("exp_avg", "exp_avg_sq", "step") + (("master",) if masters else ()):
                assert torch.equal(st[key], tt[key]), (step, i, key)
            assert ("master" in st) == masters and st["ema"].dtype == F32
            assert torch.equal(q, st["ema"].to(dtype)), (step, i)              # bit for bit (float32: the same tensor)
            assert q._version > versions[i]
            if dtype == F32:
                assert q.data_ptr() == st["ema"].data_ptr()
    print("max |error| / bound", worst)
    assert float(opt.state[ps[0]]["step"]) == 5.0


def _raw(dev, seed):
    """One table over every (parameter dtype, gradient dtype, master) pair at 1, 7, 9 and 2049 elements, an empty tensor, a
    misaligned average, one tensor without an average and a float32 parameter with an ema_out: 40 tensors, two launch groups."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for pdt, master, gdt in CONFIGS + [(F32, False, BF), (F32, False, F16)]:
        for n in (1, 7, 9, 2049):
            rows.append(dict(pdt=pdt, gdt=gdt or pdt, master=master, n=n))
    rows.insert(5, dict(pdt=BF, gdt=BF, master=True, n=0))
    rows.append(dict(pdt=BF, gdt=F32, master=True, n=2049, off=True))
    rows.append(dict(pdt=F16, gdt=F16, master=False, n=4097, no_ema=True))
    rows.append(dict(pdt=F32, gdt=F32, master=False, n=2048, out_f32=True))
    for r in rows:
        n = r["n"]
        r["p"] = torch.randn(n, generator=g).to(dev, r["pdt"])
        r["g"] = torch.randn(n, generator=g).to(dev, r["gdt"])
        r["master"] = r["p"].float() * (1 + 2.0 ** -12) if r["master"] else None
        r["m"] = (torch.randn(n, generator=g) * 0.1).to(dev)
        r["v"] = (torch.rand(n, generator=g) * 0.1).to(dev)
        r["step"] = torch.tensor(3.0, device=dev)
        e = torch.randn(n + 1, generator=g).to(dev)
        r["ema"] = None if r.get("no_ema") else (e[1:] if r.get("off") else e[:-1].clone())
        r["out"] = torch.zeros(n, device=dev, dtype=r["pdt"]) if (r["pdt"] != F32 or r.get("out_f32")) else None
    return rows


def _clone_rows(rows):
    out = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()} for r in rows]
    for r in out:
        if r.get("off"):                               # (a clone is aligned again: keep the average one element off)
            r["ema"] = torch.cat([r["ema"][:1], r["ema"]])[1:]
    return out


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _abi_step(lib, rows, ticket, *, ema):
    from aecf_amd.optim import _DTYPES
    n = len(rows)
    i32, i64 = ctypes.c_int32 * n, ctypes.c_int64 * n
    col = lambda k: _ptrs([r[k] for r in rows])
    head = (n, col("p"), col("g"), col("master"), col("m"), col("v"), col("step"), i64(*[r["n"] for r in rows]),
            i32(*[_DTYPES[r["pdt"]] for r in rows]), i32(*[_DTYPES[r["gdt"]] for r in rows]), ticket.data_ptr(), LR, 0.9, 0.98, 1e-8,
            0.05, None, None, None, None, None)
    stream = torch.cuda.current_stream().cuda_stream
    if ema:
        return lib.aecf_adamw_mp_ema_step(*head, col("ema"), col("out"), 0.99, None, stream)
    return lib.aecf_adamw_mp_step(*head, stream)


def test_fused_equals_step_plus_stand_alone():
    """2. aecf_adamw_mp_ema_step == aecf_adamw_mp_step, then aecf_ema_update on the stored weights: bit for bit, every dtype
    pair; a NULL ema leaves that tensor a plain step; an ema_out beside a float32 parameter is not written."""
    from aecf_amd import _lib
    from aecf_amd.optim import _DTYPES
    dev = _dev()
    lib = _lib.load()
    a = _raw(dev, 3)
    b = _clone_rows(a)
    assert a[-3]["ema"].data_ptr() % 16 != 0 and b[-3]["ema"].data_ptr() % 16 != 0
    ticket = torch.zeros(65 * 2, dtype=torch.int32, device=dev)
    ema0 = [None if r["ema"] is None else npf(r["ema"]) for r in a]
    assert _abi_step(lib, a, ticket, ema=True) == 0
    assert _abi_step(lib, b, ticket, ema=False) == 0
    rest = [r for r in b if r["ema"] is not None]
    n = len(rest)
    src = [r["p"] if r["master"] is None else r["master"] for r in rest]
    assert lib.aecf_ema_update(n, _ptrs(src), (ctypes.c_int32 * n)(*[_DTYPES[s.dtype] for s in src]), _ptrs([r["ema"] for r in rest]),
                               _ptrs([r["out"] for r in rest]), (ctypes.c_int32 * n)(*[_DTYPES[r["pdt"]] for r in rest]),
                               (ctypes.c_int64 * n)(*[r["n"] for r in rest]), 0.99, None, None, None,
                               torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert int(ticket.abs().sum()) == 0                                        # the launches left their tickets zero
    moved = 0
    for i, (x, y) in enumerate(zip(a, b)):
        for key in ("p", "master", "m", "v", "step", "ema", "out"):
            if x[key] is not None:
                assert torch.equal(x[key], y[key]), (i, key)
        if x["n"] and x["ema"] is not None:
            moved += 1
            assert E.excess(npf(x["ema"]), npf(x["p"] if x["master"] is None else x["master"]), ema0[i], 0.99) <= 1.0, i
            if x["pdt"] != F32:
                assert torch.equal(x["out"], x["ema"].to(x["pdt"])), i
        assert float(x["step"]) == (4.0 if x["n"] else 3.0)
    assert moved == len(a) - 2
    assert float(a[-1]["out"].abs().sum()) == 0.0                               # beside a float32 parameter: ignored
    assert float(a[-2]["out"].abs().sum()) == 0.0 and a[-2]["ema"] is None     # no average: no output either


def test_a_bf16_weight_of_one_stands_still_and_its_average_follows_the_master():
    """3. lr = 1e-4: 50 updates of at most 1e-4 with gradients of uneven size sum to 2.4e-3, below half a bf16 ulp above 1
    (2^-8): the parameter's bits never change, the float32 average moves with the master, strictly upwards."""
    from aecf_amd.optim import EmaModel, FusedAdamW
    dev = _dev()
    beta = 0.9
    bag = Bag([torch.ones(3000, dtype=BF, device=dev)])
    (p,) = bag.ps
    opt = FusedAdamW([p], lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, master_weights=True, ema_decay=beta)
    ema = EmaModel(bag, opt)
    prev = npf(opt.state[p]["ema"])
    assert np.all(prev == 1.0)
    for step in range(50):
        p.grad = torch.full_like(p, -1.0 if step % 5 == 0 else -0.02)
        opt.step()
        now = npf(opt.state[p]["ema"])
        assert E.excess(now, npf(opt.state[p]["master"]), prev, beta) <= 1.0, step
        assert np.all(now > prev), step
        prev = now
    assert torch.equal(p, torch.ones_like(p))                                   # the bits stood still
    master = opt.state[p]["master"]
    assert float(master.min()) > 1.002 and float(master.max()) < 1.0 + 2.0 ** -8
    assert np.all(prev > 1.001) and np.all(prev < npf(master))
    assert torch.equal(ema.module.ps[0], torch.ones_like(p))                    # ema.to(bf16) has not reached the next bf16 yet


def _state(opt, ps, ema):
    out = []
    for p, q in zip(ps, ema.module.ps):
        out += [p.detach().clone(), q.detach().clone()] + [v.detach().clone() for _, v in sorted(opt.state[p].items())]
    return out


def test_skipped_steps_move_no_average():
    """4. a real GradScaler overflow, and a non-finite norm under max_grad_norm: no average, ema_out or step counter changes
    (gradient-less parameters included); the next clean step moves them."""
    from aecf_amd.optim import EmaModel, FusedAdamW
    dev = _dev()
    beta = 0.9
    # GradScaler: f16 parameters with masters; the last parameter never gets a gradient
    bag = Bag([t for t in _tensors(dev, F16, 4)[:12]])
    ps = list(bag.ps)
    opt = FusedAdamW(ps, lr=LR, master_weights=True, ema_decay=beta, **HYPER)
    ema = EmaModel(bag, opt)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=1000)
    live = [p for p in ps[:-1] if p.numel()]

    def run(factor):
        opt.zero_grad(set_to_none=True)
        scaler.scale(sum((p.float() * factor).sum() for p in live)).backward()
        scaler.step(opt)
        scaler.update()

    run(0.5)
    before = _state(opt, ps, ema)
    run(100.0)                                                                  # 100 * 1024 overflows float16
    assert not bool(torch.isfinite(ps[0].grad).all()) and scaler.get_scale() == 512.0
    assert all(torch.equal(x, y) for x, y in zip(before, _state(opt, ps, ema)))
    prev = _emas(opt, ps)
    run(0.5)
    _inside(opt, ps, prev, beta, "after the overflow")
    assert all(not np.array_equal(a, b) for a, b, p in list(zip(prev, _emas(opt, ps), ps))[:-1] if p.numel())
    assert ps[-1].grad is None and float(opt.state[ps[0]]["step"]) == 2.0
    # max_grad_norm: an inf in one gradient (data, not a fault)
    bag = Bag(_tensors(dev, BF, 5)[:12])
    ps = list(bag.ps)
    opt = FusedAdamW(ps, lr=LR, master_weights=True, max_grad_norm=1.0, ema_decay=beta, **HYPER)
    ema = EmaModel(bag, opt)
    g = torch.Generator().manual_seed(6)
    _set(ps, _grads(ps, g, None, skip=(11,)))
    opt.step()
    before = _state(opt, ps, ema)
    grads = _grads(ps, g, None, skip=(11,))
    grads[4].view(-1)[3] = float("inf")
    _set(ps, grads)
    opt.step()
    assert float(opt.skipped_steps) == 1
    assert all(torch.equal(x, y) for x, y in zip(before, _state(opt, ps, ema)))
    prev = _emas(opt, ps)
    _set(ps, _grads(ps, g, None, skip=(11,)))
    opt.step()
    _inside(opt, ps, prev, beta, "after the inf")
    assert all(not np.array_equal(a, b) for a, b, p in list(zip(prev, _emas(opt, ps), ps))[:-1] if p.numel())
    assert all(torch.equal(q, opt.state[p]["ema"].to(BF)) for p, q in zip(ps, ema.module.ps) if p.numel())


@pytest.mark.parametrize("config", [(F32, False, None), (BF, True, None), (F16, False, None)], ids=_ids)
def test_a_parameter_without_a_gradient_still_moves_its_average(config):
    """5. no gradient in step 2 of 3 (tensors 3, 6 and the offset view): the weight stays, its average moves towards it."""
    from aecf_amd.optim import EmaModel, FusedAdamW
    dev = _dev()
    dtype, masters, gdt = config
    beta = 0.9
    bag = Bag(_tensors(dev, dtype, 7))
    ps = list(bag.ps)
    opt = FusedAdamW(ps, lr=LR, master_weights=masters, ema_decay=beta, **HYPER)
    ema = EmaModel(bag, opt)
    g = torch.Generator().manual_seed(8)
    idle = (3, 6, VIEW)
    for step in range(3):
        _set(ps, _grads(ps, g, gdt, skip=idle if step == 1 else ()))
        before = _emas(opt, ps)
        weights = [_stored(opt, p).clone() for p in ps]
        opt.step()
        _inside(opt, ps, before, beta, step)
        if step == 1:
            for i in idle:
                assert torch.equal(_stored(opt, ps[i]), weights[i]) and float(opt.state[ps[i]]["step"]) == 1.0
                assert not np.array_equal(npf(opt.state[ps[i]]["ema"]), before[i]), i
    for p, q in zip(ps, ema.module.ps):
        if p.numel():
            assert torch.equal(q, opt.state[p]["ema"].to(dtype))


def test_captured_training_step_follows_a_device_decay():
    """6. forward, backward and step of a two-layer bf16 model in ONE graph; beta is a device tensor changed between replays."""
    from aecf_amd.optim import EmaModel, FusedAdamW
    dev = _dev()
    torch.manual_seed(9)
    model = torch.nn.Sequential(torch.nn.Linear(64, 48), torch.nn.Tanh(), torch.nn.Linear(48, 5)).to(dev, BF)
    ps = list(model.parameters())
    decay = torch.tensor(0.5, device=dev)
    opt = FusedAdamW(ps, lr=torch.tensor(LR, device=dev), master_weights=True, ema_decay=decay, **HYPER)
    ema = EmaModel(model, opt)
    x = torch.randn(32, 64, device=dev).to(BF)

    def step():
        opt.zero_grad(set_to_none=True)
        model(x).float().pow(2).mean().backward()
        opt.step()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        step()
    for beta in (0.9, 0.0, 0.9999):
        decay.fill_(beta)
        x.copy_(torch.randn(32, 64, device=dev))
        before = _emas(opt, ps)
        graph.replay()
        torch.cuda.synchronize()
        ema.after_replay()
        _inside(opt, ps, before, beta, beta)
        for i, (p, q) in enumerate(zip(ps, ema.module.parameters())):
            assert torch.equal(q, opt.state[p]["ema"].to(BF))
            assert not np.array_equal(npf(opt.state[p]["ema"]), before[i])
    assert float(opt.state[ps[0]]["step"]) == 5.0                               # two eager steps, three replays


def test_ema_model_on_a_bf16_pool_and_ema_weights():
    """7. after 3 steps the EmaModel's pool in eval mode equals a FRESH pool loaded with ema.to(bf16) (its inference caches
    followed the raw writes); ``with opt.ema_weights()`` gives the same output from the live pool and restores its bits."""
    import aecf_amd
    from aecf_amd.optim import EmaModel, FusedAdamW
    dev = _dev()
    torch.manual_seed(10)
    E_, M, H, B = 128, 3, 4, 64

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.query, self.pool = aecf_amd.create_fusion_pool(E_, M, num_heads=H)

        def forward(self, x):
            return self.pool(self.query.expand(x.shape[0], -1, -1), x)

    net = Net().to(dev, BF)
    ps = list(net.parameters())
    opt = FusedAdamW(ps, lr=2e-3, master_weights=True, ema_decay=0.5)
    ema = EmaModel(net, opt)
    x = torch.randn(B, M, E_, device=dev).to(BF)
    dy = torch.randn(B, 1, E_, device=dev)
    ema.module.eval()
    with torch.no_grad():
        y0 = ema.module(x).clone()                                              # fills the copy's caches
    for _ in range(3):
        net.train()
        opt.zero_grad(set_to_none=True)
        (net(x).float() * dy).sum().backward()
        opt.step()
    with torch.no_grad():
        y1 = ema.module(x).clone()
    fresh = Net().to(dev, BF).eval()
    fresh.load_state_dict({k: opt.state[p]["ema"].to(BF) for (k, p) in net.named_parameters()}, strict=False)
    with torch.no_grad():
        y2 = fresh(x)
    assert torch.equal(y1, y2) and not torch.equal(y1, y0)
    net.eval()
    keep = [p.detach().clone() for p in ps]
    with torch.no_grad():
        live = net(x).clone()
        with opt.ema_weights():
            y3 = net(x).clone()
        back = net(x).clone()
    assert torch.equal(y3, y1) and not torch.equal(live, y1)
    assert torch.equal(back, live) and all(torch.equal(p, k) for p, k in zip(ps, keep))
    assert all(torch.equal(p, opt.state[p]["master"].to(BF)) for p in ps)


def test_state_dict_round_trip_continues_bit_equal():
    """8a. two steps, state_dict() into a new optimiser (new averages, loaded as float32), two more steps on both."""
    from aecf_amd.optim import FusedAdamW
    dev = _dev()
    pa = [t.requires_grad_() for t in _tensors(dev, BF, 11)[:12]]
    oa = FusedAdamW(pa, lr=LR, master_weights=True, ema_decay=0.99, **HYPER)
    g = torch.Generator().manual_seed(12)
    for _ in range(2):
        _set(pa, _grads(pa, g, None))
        oa.step()
    pb = [p.detach().clone().requires_grad_() for p in pa]
    ob = FusedAdamW(pb, lr=LR, master_weights=True, ema_decay=0.99, **HYPER)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    # and one whose loaded state has no average: it starts from the weights at its next step
    bare = copy.deepcopy(oa.state_dict())
    for st in bare["state"].values():
        st.pop("ema", None)
    pc = [p.detach().clone().requires_grad_() for p in pa]
    oc = FusedAdamW(pc, lr=LR, master_weights=True, ema_decay=0.5, **HYPER)
    oc.load_state_dict(bare)
    for k in range(2):
        grads = _grads(pa, g, None)
        for ps_, o in ((pa, oa), (pb, ob)) + (((pc, oc),) if k == 0 else ()):
            _set(ps_, grads)
            o.step()
    for i, (a, b, c) in enumerate(zip(pa, pb, pc)):
        if a.numel() == 0:
            continue
        loaded = npf(bare["state"][i]["master"])
        assert E.excess(npf(oc.state[c]["ema"]), npf(oc.state[c]["master"]), loaded, 0.5) <= 1.0, i
        assert ob.state[b]["ema"].dtype == F32
        for key in ("ema", "master", "exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(oa.state[a][key], ob.state[b][key]), key
        assert torch.equal(a, b)


def test_graphed_train_step_starts_from_the_restored_weights():
    """8b. a GraphedTrainStep on a fresh optimiser with ema_decay: the capture steps' averages come back as the weights."""
    from aecf_amd.optim import EmaModel, FusedAdamW
    from aecf_amd.xray import AECFModel, GraphedTrainStep
    dev = _dev()
    torch.manual_seed(13)
    model = AECFModel(512, 512, 15).to(dev).train()
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01, ema_decay=0.9)
    start = [p.detach().clone() for p in model.parameters()]
    step = GraphedTrainStep(model, opt, torch.nn.BCEWithLogitsLoss(), 64, 512, 512, 15, dev, warmup=2)
    for p, s in zip(model.parameters(), start):
        st = opt.state[p]
        assert torch.equal(p, s) and torch.equal(st["ema"], s) and float(st["step"]) == 0.0
        assert float(st["exp_avg"].abs().sum()) == 0.0
    g = torch.Generator().manual_seed(14)
    image, text = torch.randn(64, 512, generator=g).to(dev), torch.randn(64, 512, generator=g).to(dev)
    labels = (torch.rand(64, 15, generator=g) < 0.2).float().to(dev)
    assert math.isfinite(float(step(image, text, labels)))
    for p, s in zip(model.parameters(), start):
        assert E.excess(npf(opt.state[p]["ema"]), npf(p), npf(s), 0.9) <= 1.0
    # with an EmaModel attached before the capture, its tensors come back too
    model2 = AECFModel(512, 512, 15).to(dev).train()
    opt2 = FusedAdamW(model2.parameters(), lr=1e-3, weight_decay=0.01, ema_decay=0.9)
    ema2 = EmaModel(model2, opt2)
    GraphedTrainStep(model2, opt2, torch.nn.BCEWithLogitsLoss(), 64, 512, 512, 15, dev, warmup=2)
    for (k, p), q in zip(model2.named_parameters(), ema2.module.parameters()):
        assert torch.equal(q, p) and q.data_ptr() == opt2.state[p]["ema"].data_ptr(), k
        assert float(opt2.state[p]["step"]) == 0.0


def test_trainer_with_ema_decay(monkeypatch):
    """8c. train_xray.main --ema-decay 0.99 at the tiny sizes of the bf16 trainer test: both models are validated."""
    from aecf_amd import train_xray
    made = []

    class Recording(train_xray.FusedAdamW):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            made.append(self)

    monkeypatch.setattr(train_xray, "FusedAdamW", Recording)
    history = train_xray.main(["--epochs", "2", "--switch-epoch", "1", "--samples", "320", "--val-samples", "128", "--batch", "64",
                               "--ema-decay", "0.99"])
    assert len(history) == 2
    for row in history:
        assert math.isfinite(row["train_loss"]) and 0.0 < row["val_map"] <= 1.0 and 0.0 < row["ema_val_map"] <= 1.0
        assert {"ema_val_map_no_images", "ema_val_map_no_texts"} <= set(row)
    (opt,) = made
    assert opt.ema_decay == 0.99
    for grp in opt.param_groups:
        for p in grp["params"]:
            st = opt.state[p]
            assert st["ema"].dtype == F32 and not torch.equal(st["ema"], p.detach().float())
