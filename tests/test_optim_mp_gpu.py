"""FusedAdamW's mixed-precision step (aecf_adamw_mp_step, aecf_grad_norm) against AdamW restated in float64 with plain torch
CPU ops (``Ref`` below).  The restatement takes exactly what the kernel sees: low-precision gradients widened exactly, the
float32 roundings of the hyper-parameters, the same lr, scale and clip coefficient.  Where a parameter has no master, the
kernel's input of a step is the ROUNDED parameter of the step before, so such a step is restated from that input (``w_in``):
the bound is one round-to-nearest of a float32 value that is itself within 2e-6."""
import copy
import math

import pytest
import torch

from tests.helpers import hot_shape_inputs, record_errors, rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-6                                            # the bound tests/test_optim_gpu.py holds aecf_adamw_step to
HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
HYPER = dict(betas=(0.9, 0.98), eps=1e-8, weight_decay=0.05)
SHAPES = [(256, 512), (256,), (3, 7, 5), (1,), (1031,), (64, 64)] + [(17 + i, 3) for i in range(25)]
f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
cpu64 = lambda t: t.detach().double().cpu()


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _params(dev, seed, n, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g).to(dev, dtype).requires_grad_() for s in SHAPES[:n]]


def _set_grads(ps, gen, scale=1.0, dtype=None, skip=()):
    for i, p in enumerate(ps):
        if i in skip:
            p.grad = None
            continue
        p.grad_dtype = None                           # (a float32 gradient beside a 16-bit parameter)
        p.grad = (torch.randn(p.shape, generator=gen) * scale).to(p.device, dtype or p.dtype)


class Ref:
    """torch/optim/adamw.py (amsgrad off) in float64 on the CPU."""

    def __init__(self, weights, betas, eps, weight_decay):
        self.w = [cpu64(w) for w in weights]
        self.m = [torch.zeros_like(w) for w in self.w]
        self.v = [torch.zeros_like(w) for w in self.w]
        self.t = [0] * len(self.w)
        self.b1, self.b2, self.eps, self.wd = f32(betas[0]), f32(betas[1]), f32(eps), f32(weight_decay)

    def step(self, grads, lr, gmul=1.0, w_in=None):
        lr = f32(lr)
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = cpu64(g) * gmul
            self.t[i] += 1
            w = (self.w[i] if w_in is None else cpu64(w_in[i])) * (1.0 - lr * self.wd)
            self.m[i] = self.b1 * self.m[i] + (1.0 - self.b1) * g
            self.v[i] = self.b2 * self.v[i] + (1.0 - self.b2) * g * g
            denom = self.v[i].sqrt() / math.sqrt(1.0 - self.b2 ** self.t[i]) + self.eps
            self.w[i] = w - lr / (1.0 - self.b1 ** self.t[i]) * (self.m[i] / denom)


def _check_state(opt, ps, ref, weight_key=None, tol=TOL):
    errs = []
    for i, p in enumerate(ps):
        st = opt.state[p]
        errs.append(max(rel_err(st["exp_avg"].cpu(), ref.m[i]), rel_err(st["exp_avg_sq"].cpu(), ref.v[i])))
        if weight_key is not None:
            errs.append(rel_err((st[weight_key] if weight_key == "master" else p).detach().cpu(), ref.w[i]))
        assert st["exp_avg"].dtype == st["exp_avg_sq"].dtype == torch.float32
        assert float(st["step"]) == ref.t[i], i
    print("state rel err max", max(errs))
    assert max(errs) < tol, errs
    return max(errs)


def _ulps(a, b):
    o = lambda x: (lambda i: torch.where(i < 0, -(i & 0x7FFFFFFF), i))(x.detach().contiguous().view(torch.int32).long())
    return int((o(a) - o(b)).abs().max())


@pytest.mark.parametrize("n_tensors", [5, 31])
def test_float32_through_the_mp_entry_point(n_tensors):
    """1. float32 parameters forced onto aecf_adamw_mp_step by a tensor lr; the ulp distance from aecf_adamw_step is recorded."""
    from aecf_amd.optim import FusedAdamW
    dev = _dev()
    pa = _params(dev, 1, n_tensors)
    pb = [p.detach().clone().requires_grad_() for p in pa]
    oa = FusedAdamW(pa, lr=torch.tensor(3e-3, device=dev), **HYPER)
    ob = FusedAdamW(pb, lr=3e-3, **HYPER)
    ref = Ref(pa, **HYPER)
    g = torch.Generator().manual_seed(2)
    for step in range(7):
        _set_grads(pa, g, 10.0 ** (step % 3 - 1), skip=(1,) if step == 3 else ())
        for a, b in zip(pa, pb):
            b.grad = None if a.grad is None else a.grad.clone()
        ref.step([p.grad for p in pa], 3e-3)
        oa.step()
        ob.step()
    err = _check_state(oa, pa, ref, "param")
    ulps = max(max(_ulps(a, b), _ulps(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]),
                   _ulps(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])) for a, b in zip(pa, pb))
    print("ulps from aecf_adamw_step", ulps)
    record_errors(f"optim_mp_f32_n{n_tensors}", rel=err, ulps_from_adamw_step=ulps)


@pytest.mark.parametrize("gdt", ["param", "float32"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_low_precision_parameters_without_masters(dtype, gdt):
    """2. moments at 2e-6; the parameter within one rounding of the float64 step from the parameter the kernel read."""
    from aecf_amd.optim import FusedAdamW
    dev = _dev()
    ps = _params(dev, 3, 6, dtype)
    opt = FusedAdamW(ps, lr=3e-3, **HYPER)
    ref = Ref(ps, **HYPER)
    g = torch.Generator().manual_seed(4)
    worst = 0.0
    for step in range(7):
        _set_grads(ps, g, 10.0 ** (step % 3 - 1), dtype=None if gdt == "param" else torch.float32)
        ref.step([p.grad for p in ps], 3e-3, w_in=ps)
        opt.step()
        for p, want in zip(ps, ref.w):
            assert p.dtype == dtype and "master" not in opt.state[p]
            excess = (cpu64(p) - want).abs() - (HALF_ULP[dtype] * want.abs() + TOL * want.abs().max())
            worst = max(worst, float(((cpu64(p) - want).abs() / want.abs().clamp_min(1e-30)).max()))
            assert float(excess.max()) <= 0.0, (step, float(excess.max()))
    err = _check_state(opt, ps, ref)
    record_errors(f"optim_mp_nomaster_{str(dtype)[6:]}_g{gdt}", moments=err, param_elementwise_rel=worst)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_masters_follow_float64_and_the_parameter_is_their_rounding(dtype):
    """3. the master within 2e-6 after 7 steps, the working copy == master.to(dtype) after every step."""
    from aecf_amd.optim import FusedAdamW
    dev = _dev()
    ps = _params(dev, 5, 31, dtype)
    opt = FusedAdamW(ps, lr=3e-3, master_weights=True, **HYPER)
    ref = Ref(ps, **HYPER)
    g = torch.Generator().manual_seed(6)
    for step in range(7):
        _set_grads(ps, g, 10.0 ** (step % 3 - 1), dtype=torch.float32 if step == 5 else None)
        ref.step([p.grad for p in ps], 3e-3)
        opt.step()
        for p in ps:
            assert torch.equal(p, opt.state[p]["master"].to(dtype)), step
    record_errors(f"optim_mp_master_{str(dtype)[6:]}", rel=_check_state(opt, ps, ref, "master"))


def test_a_bf16_weight_of_one_stalls_without_a_master_and_moves_with_one():
    """3. lr = 1e-4 moves a weight near 1 by 1e-4 a step, below half a bf16 ulp (2^-9)."""
    from aecf_amd.optim import FusedAdamW
    dev = _dev()
    hyper = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    pa = torch.ones(3000, dtype=torch.bfloat16, device=dev, requires_grad=True)
    pb = pa.detach().clone().requires_grad_()
    oa = FusedAdamW([pa], lr=1e-4, **hyper)
    ob = FusedAdamW([pb], lr=1e-4, master_weights=True, **hyper)
    ref = Ref([pb], **hyper)
    grad = torch.full_like(pa, 0.5)
    for _ in range(40):
        pa.grad, pb.grad = grad, grad
        ref.step([grad], 1e-4)
        oa.step()
        ob.step()
    assert torch.equal(pa, torch.ones_like(pa))
    master = ob.state[pb]["master"]
    assert not torch.equal(pb, torch.ones_like(pb)) and float(pb.detach().float().max()) < 1.0
    err = rel_err(master.cpu(), ref.w[0])
    print("master rel err after 40 steps", err)
    assert err < 40 * TOL
    assert torch.equal(pb, master.to(torch.bfloat16))
    record_errors("optim_mp_stall_master", rel=err)


def _mixed(dev, seed):
    """float32 tensors and bf16 tensors with masters in one optimiser."""
    return _params(dev, seed, 4) + _params(dev, seed + 1, 6, torch.bfloat16)[3:]


def _snapshot(opt, ps):
    out = [p.detach().clone() for p in ps]
    for p in ps:
        out += [v.detach().clone() for _, v in sorted(opt.state[p].items())]
    return out


def test_clipping():
    """4. norm at 1e-6, the update on gradients times min(1, max / (norm + 1e-6)), an exact no-op coefficient, an inf skipped."""
    from aecf_amd import optim
    dev = _dev()
    lr = lambda: torch.tensor(3e-3, device=dev)       # (a tensor lr: the run without clipping takes the same entry point)
    pa, pb, pc = _mixed(dev, 7), _mixed(dev, 7), _mixed(dev, 7)
    oa = optim.FusedAdamW(pa, lr=lr(), master_weights=True, max_grad_norm=1.0, **HYPER)
    ob = optim.FusedAdamW(pb, lr=lr(), master_weights=True, max_grad_norm=1e9, **HYPER)
    oc = optim.FusedAdamW(pc, lr=lr(), master_weights=True, **HYPER)
    ref = Ref(pa, **HYPER)
    g = torch.Generator().manual_seed(8)
    for step in range(3):
        _set_grads(pa, g, 10.0 ** (step - 1))
        for a, b, c in zip(pa, pb, pc):
            b.grad, c.grad = a.grad.clone(), a.grad.clone()
        kept = [p.grad.clone() for p in pa]
        norm64 = math.sqrt(sum(float(cpu64(p.grad).pow(2).sum()) for p in pa))
        coef64 = min(1.0, 1.0 / (norm64 + 1e-6))
        assert coef64 < 1.0                           # this case clips
        ref.step([p.grad for p in pa], 3e-3, gmul=coef64)
        oa.step()
        ob.step()
        oc.step()
        e_norm = abs(float(oa.last_grad_norm) - norm64) / norm64
        e_free = abs(float(optim.grad_norm(pa)) - norm64) / norm64
        print("grad norm rel err", e_norm, e_free)
        record_errors(f"optim_mp_grad_norm_step{step}", rel=e_norm, rel_norm_only=e_free)
        assert e_norm < 1e-6 and e_free < 1e-6
        assert all(torch.equal(p.grad, k) for p, k in zip(pa, kept))                # gradients are not rewritten
        assert float(ob.last_clip_coef) == 1.0 and float(ob.skipped_steps) == 0      # this case does not clip
        assert all(torch.equal(x, y) for x, y in zip(_snapshot(ob, pb), _snapshot(oc, pc)))
    for i, p in enumerate(pa):                        # (float32 parameters are their own masters)
        w = oa.state[p].get("master", p)
        assert rel_err(w.detach().cpu(), ref.w[i]) < TOL, i
        assert torch.equal(p, w.to(p.dtype))
    _check_state(oa, pa, ref)
    assert float(oa.skipped_steps) == 0
    # an inf in one gradient (data, not a fault): nothing is written, the skip is counted, the next clean step works
    before = _snapshot(oa, pa)
    _set_grads(pa, g)
    pa[2].grad.view(-1)[3] = float("inf")
    oa.step()
    assert all(torch.equal(x, y) for x, y in zip(before, _snapshot(oa, pa)))
    assert float(oa.skipped_steps) == 1 and not math.isfinite(float(oa.last_grad_norm))
    _set_grads(pa, g)
    norm64 = math.sqrt(sum(float(cpu64(p.grad).pow(2).sum()) for p in pa))
    ref.step([p.grad for p in pa], 3e-3, gmul=min(1.0, 1.0 / (norm64 + 1e-6)))
    oa.step()
    _check_state(oa, pa, ref)
    assert rel_err(oa.state[pa[-1]]["master"].cpu(), ref.w[-1]) < TOL and float(oa.skipped_steps) == 1


def test_grad_scaler_on_the_device():
    """5. torch.amp.GradScaler with fp16 parameters and masters: unscale and skip inside the launch, no host sync in step()."""
    from aecf_amd.optim import FusedAdamW
    dev = _dev()
    ps = _params(dev, 9, 5, torch.float16)
    opt = FusedAdamW(ps, lr=3e-3, master_weights=True, **HYPER)
    inner = opt.step

    def guarded(*args, **kwargs):
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            return inner(*args, **kwargs)
        finally:
            torch.cuda.set_sync_debug_mode(mode)

    opt.step = guarded
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=1000)
    ref = Ref(ps, **HYPER)
    g = torch.Generator().manual_seed(10)
    for step in range(3):
        coefs = [torch.randn(p.shape, generator=g).to(dev) for p in ps]
        opt.zero_grad(set_to_none=True)
        loss = sum((p.float() * c).sum() for p, c in zip(ps, coefs))
        scaler.scale(loss).backward()
        ref.step([p.grad for p in ps], 3e-3, gmul=1.0 / 1024.0)       # the fp16 gradients as stored, unscaled exactly
        scaler.step(opt)
        scaler.update()
    assert scaler.get_scale() == 1024.0
    record_errors("optim_mp_grad_scaler", rel=_check_state(opt, ps, ref, "master"))
    assert all(torch.equal(p, opt.state[p]["master"].to(torch.float16)) for p in ps)
    # 100 * 1024 overflows float16: the scaler's flag skips the step on the device and the scale halves
    before = _snapshot(opt, ps)
    opt.zero_grad(set_to_none=True)
    scaler.scale(sum((p.float() * 100.0).sum() for p in ps)).backward()
    assert not bool(torch.isfinite(ps[0].grad).all())
    scaler.step(opt)
    scaler.update()
    assert all(torch.equal(x, y) for x, y in zip(before, _snapshot(opt, ps)))
    assert scaler.get_scale() == 512.0


def test_captured_step_follows_a_device_lr():
    """6. one capture, five replays with new gradients and a new lr.fill_() each; bf16 parameters with masters."""
    from aecf_amd.optim import FusedAdamW
    dev = _dev()
    pa = _params(dev, 11, 5, torch.bfloat16)
    pb = [p.detach().clone().requires_grad_() for p in pa]
    lra, lrb = torch.tensor(1e-2, device=dev), torch.tensor(1e-2, device=dev)
    oa = FusedAdamW(pa, lr=lra, master_weights=True, **HYPER)
    ob = FusedAdamW(pb, lr=lrb, master_weights=True, **HYPER)
    ref = Ref(pa, **HYPER)
    grads = [torch.zeros_like(p) for p in pb]
    for a, b, gbuf in zip(pa, pb, grads):
        a.grad, b.grad = torch.zeros_like(a), gbuf
    ref.step(grads, 1e-2)
    oa.step()
    ob.step()                                         # builds the state outside the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ob.step()
    g = torch.Generator().manual_seed(12)
    for k in range(5):
        rate = 1e-2 / (k + 2)
        _set_grads(pa, g)
        for a, gbuf in zip(pa, grads):
            gbuf.copy_(a.grad)
        lra.fill_(rate)
        lrb.fill_(rate)
        ref.step([p.grad for p in pa], rate)
        oa.step()
        graph.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert rel_err(ob.state[b]["master"].cpu(), oa.state[a]["master"].cpu()) < TOL
        assert rel_err(ob.state[b]["master"].cpu(), ref.w[i]) < TOL
        assert float(ob.state[b]["step"]) == float(oa.state[a]["step"]) == 6.0
        assert torch.equal(b, ob.state[b]["master"].to(torch.bfloat16))


def test_state_dict_round_trip_and_a_torch_adamw_state():
    """7. FusedAdamW -> state_dict -> FusedAdamW continues bit for bit; a torch.optim.AdamW state of bf16 parameters loads."""
    from aecf_amd.optim import FusedAdamW
    dev = _dev()
    pa = _params(dev, 13, 5, torch.bfloat16)
    oa = FusedAdamW(pa, lr=3e-3, master_weights=True, **HYPER)
    g = torch.Generator().manual_seed(14)
    for _ in range(3):
        _set_grads(pa, g)
        oa.step()
    pb = [p.detach().clone().requires_grad_() for p in pa]
    ob = FusedAdamW(pb, lr=3e-3, master_weights=True, **HYPER)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    for a, b in zip(pa, pb):
        assert ob.state[b]["master"].dtype == ob.state[b]["exp_avg"].dtype == torch.float32
    for _ in range(2):
        _set_grads(pa, g)
        for a, b in zip(pa, pb):
            b.grad = a.grad.clone()
        oa.step()
        ob.step()
    assert all(torch.equal(x, y) for x, y in zip(_snapshot(oa, pa), _snapshot(ob, pb)))
    # torch.optim.AdamW on bf16 parameters: bf16 moments, no master, step counters on the host
    pt = _params(dev, 15, 5, torch.bfloat16)
    ot = torch.optim.AdamW(pt, lr=3e-3, **HYPER)
    for _ in range(2):
        _set_grads(pt, g)
        ot.step()
    assert ot.state[pt[0]]["exp_avg"].dtype == torch.bfloat16
    pf = [p.detach().clone().requires_grad_() for p in pt]
    of = FusedAdamW(pf, lr=3e-3, master_weights=True, **HYPER)
    of.load_state_dict(copy.deepcopy(ot.state_dict()))
    moments = [of.state[p]["exp_avg"].float().clone() for p in pf]
    _set_grads(pf, g)
    of.step()
    for p, m0 in zip(pf, moments):
        st = of.state[p]
        assert st["exp_avg"].dtype == st["exp_avg_sq"].dtype == st["master"].dtype == torch.float32
        assert float(st["step"]) == 3.0 and torch.equal(p, st["master"].to(torch.bfloat16))
        want = f32(0.9) * cpu64(m0) + (1.0 - f32(0.9)) * cpu64(p.grad)              # the widened moment continued
        assert rel_err(st["exp_avg"].cpu(), want) < TOL


def test_bf16_pool_trained_with_masters_and_clipping_then_inference():
    """8. the inference caches of a bf16 pool see the updates made through aecf_adamw_mp_step."""
    import aecf_amd
    from aecf_amd.optim import FusedAdamW
    dev, bf = _dev(), torch.bfloat16
    B, M, E, H = 256, 3, 512, 8
    d = hot_shape_inputs(11, B=B, M=M, E=E, H=H)
    pool = aecf_amd.MultimodalAttentionPool(E, num_heads=H)
    a = pool.attention
    with torch.no_grad():
        for p, k in ((a.in_proj_weight, "w_in"), (a.in_proj_bias, "b_in"), (a.out_proj.weight, "w_out"), (a.out_proj.bias, "b_out")):
            p.copy_(d[k])
    pool = pool.to(dev, bf)
    q = torch.nn.Parameter(d["query"].to(dev, bf))
    x, dy = d["x"].to(dev, bf), d["dy"].to(dev)
    opt = FusedAdamW(list(pool.parameters()) + [q], lr=2e-3, master_weights=True, max_grad_norm=1.0)
    pool.eval()
    with torch.no_grad():
        y0 = pool(q.expand(B, -1, -1), x).clone()      # fills the caches
    for _ in range(3):
        pool.train()
        opt.zero_grad(set_to_none=True)
        y = pool(q.expand(B, -1, -1), x)
        (y.float() * dy).sum().backward()
        opt.step()
    for p in list(pool.parameters()) + [q]:
        assert torch.equal(p, opt.state[p]["master"].to(bf))
    pool.eval()
    with torch.no_grad():
        y1 = pool(q.expand(B, -1, -1), x)
    fresh = aecf_amd.MultimodalAttentionPool(E, num_heads=H).to(dev, bf).eval()
    fresh.load_state_dict(pool.state_dict())
    q2 = torch.nn.Parameter(q.detach().clone())
    with torch.no_grad():
        y2 = fresh(q2.expand(B, -1, -1), x)
    assert torch.equal(y1, y2)
    assert rel_err(y1.float().cpu(), y0.float().cpu()) > 1e-2         # the three steps moved the output: a stale cache would not pass
    assert float(opt.skipped_steps) == 0


def test_trainer_in_bf16_with_clipping(monkeypatch):
    """9. train_xray.main --param-dtype bfloat16 --max-grad-norm 1.0: finite losses, every parameter the rounding of its master."""
    from aecf_amd import train_xray
    made = []

    class Recording(train_xray.FusedAdamW):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            made.append(self)

    monkeypatch.setattr(train_xray, "FusedAdamW", Recording)
    history = train_xray.main(["--epochs", "2", "--switch-epoch", "1", "--samples", "320", "--val-samples", "128", "--batch", "64",
                               "--param-dtype", "bfloat16", "--max-grad-norm", "1.0"])
    assert len(history) == 2 and all(math.isfinite(row["train_loss"]) for row in history)
    (opt,) = made
    assert opt.master_weights and opt.max_grad_norm == 1.0 and math.isfinite(float(opt.last_grad_norm))
    low = [p for grp in opt.param_groups for p in grp["params"] if p.dtype == torch.bfloat16]
    assert low and len(low) == sum(len(grp["params"]) for grp in opt.param_groups)
    for p in low:
        st = opt.state[p]
        assert 1.0 <= float(st["step"]) <= 10.0                        # (5 steps an epoch)
        assert st["master"].dtype == torch.float32 and torch.equal(p, st["master"].to(torch.bfloat16))
