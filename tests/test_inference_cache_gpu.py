"""Inference after the parameters or the query change: the pool's inference caches (the kernels' preparation behind
AECF_PREP_READY and the bf16 copies of float32 master weights, aecf_amd/layer.py) must never serve a stale result.

Every test runs an inference forward so that the caches fill, changes the parameters or the query by one route, runs the
forward again and checks the second result three ways:
  (a) against the float64 CPU oracle on the parameters and query as they are AFTER the change, read back from the device, at
      the bound the suite uses for that tensor and dtype (the oracle reads what the kernels read: the activation-dtype view);
  (b) bit for bit against the same call on a copy of the module that starts without caches (the kernels are deterministic);
  (c) the oracle before and after the change differ by at least 10x the bound of (a), so a stale result cannot pass (a).
Headline shape [256, 3, 512], 8 heads: bf16, float32, and float32 master weights under bf16 activations ("master")."""
import copy

import pytest
import torch
import torch.nn as nn

from tests.helpers import BF16_BOUNDS, f32grad_bounds, hot_shape_inputs, rel_err

pytestmark = pytest.mark.gpu

B, M, E, H = 256, 3, 512, 8
FP32_TOL = 1e-5                                    # the fp32 parity bound (tests/test_pool_gpu.py)
CASES = {"bf16": (torch.bfloat16, torch.bfloat16), "f32": (torch.float32, torch.float32),
         "master": (torch.float32, torch.bfloat16)}       # (parameter dtype, activation dtype)
LR = 2e-3                                          # one AdamW step moves y by ~17 % and the weights by ~14 % of their maximum


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _bounds(case):
    if case == "bf16":
        return BF16_BOUNDS
    if case == "master":
        return f32grad_bounds(B, M, E, H)
    g = 2 * FP32_TOL                               # float32 parameter gradients: 2x, as the other fp32 oracle tests
    return dict(y=FP32_TOL, wbar=FP32_TOL, dx=FP32_TOL, dquery=g, dw_in=g, db_in=g, dw_out=g, db_out=g)


def _load(pool, d):
    a = pool.attention
    with torch.no_grad():
        for p, k in ((a.in_proj_weight, "w_in"), (a.in_proj_bias, "b_in"), (a.out_proj.weight, "w_out"), (a.out_proj.bias, "b_out")):
            p.copy_(d[k])


def _setup(case, seed=11):
    import aecf_amd
    pdt, adt = CASES[case]
    dev = _dev()
    d = hot_shape_inputs(seed, B=B, M=M, E=E, H=H)
    pool = aecf_amd.MultimodalAttentionPool(E, num_heads=H)
    _load(pool, d)
    pool = pool.to(dev, pdt)
    q = nn.Parameter(d["query"].to(dev, pdt))
    x = d["x"].to(dev, adt)
    d["dy"], d["dwbar"] = d["dy"].to(dev), d["dwbar"].to(dev)
    return pool, q, x, d


def _fwd(pool, q, x, grad=False):
    with torch.set_grad_enabled(grad):
        y, info = pool(q.expand(x.shape[0], -1, -1), x, return_info=True)
    return y, info["attention_weights"]


def _loss_backward(pool, q, x, d):
    y, w = _fwd(pool, q, x, grad=True)
    ((y.float() * d["dy"]).sum() + (w.float() * d["dwbar"]).sum()).backward()
    return y, w


def _ref(pool, q, x, d=None):
    """float64 oracle on the module's parameters and the query as they are now (the activation-dtype view the kernels read)."""
    from oracle import aecf_oracle as O
    adt, e, h = x.dtype, pool.embed_dim, pool.num_heads
    c = lambda t_: None if t_ is None else t_.detach().to(adt).double().cpu()
    a = pool.attention
    qe = c(q).reshape(1, 1, e).expand(x.shape[0], -1, -1)
    xx = c(x)
    w_in, b_in, w_out, b_out = c(a.in_proj_weight), c(a.in_proj_bias), c(a.out_proj.weight), c(a.out_proj.bias)
    f = O.mha_forward(qe, xx, xx, w_in, b_in, w_out, b_out, h)
    out = dict(y=f["y"], wbar=f["wbar"])
    if d is not None:
        b = O.mha_backward(qe, xx, xx, w_in, b_in, w_out, h, f, d["dy"].double().cpu(), d["dwbar"].double().cpu())
        out.update(dx=b["dkey"] + b["dvalue"], dquery=b["dquery"].sum(0, keepdim=True), dw_in=b["dw_in"], db_in=b["db_in"],
                   dw_out=b["dw_out"], db_out=b["db_out"])
    return out


def _grads(pool, q, x):
    a = pool.attention
    return dict(dx=x.grad, dquery=q.grad, dw_in=a.in_proj_weight.grad, db_in=a.in_proj_bias.grad,
                dw_out=a.out_proj.weight.grad, db_out=a.out_proj.bias.grad)


def _assert_close(got, want, bounds, what):
    for k, g in got.items():
        e = rel_err(g.detach().float().cpu(), want[k])
        assert e < bounds[k], (what, k, e, bounds[k])


def _assert_moved(before, after, bounds, what):
    for k in ("y", "wbar"):
        e = rel_err(after[k], before[k])
        assert e >= 10 * bounds[k], (what, "the change does not move the oracle enough to tell a stale result", k, e)


def _fresh(pool):
    """A copy of the module that starts without any cached state."""
    other = copy.deepcopy(pool)
    other.invalidate_cast_cache()
    other.zero_grad(set_to_none=True)
    return other


def _check_no_grad(pool, q, x, before, bounds, what):
    """(a), (b), (c) of an inference forward without gradient recording."""
    y, w = _fwd(pool, q, x)
    after = _ref(pool, q, x)
    _assert_moved(before, after, bounds, what)
    _assert_close(dict(y=y, wbar=w), after, bounds, what)
    y2, w2 = _fwd(_fresh(pool), q, x)
    assert torch.equal(y, y2) and torch.equal(w, w2), what


# ---- FusedAdamW (writes the parameters through raw pointers) ----------------------------------------------------------------
@pytest.mark.parametrize("case", ["f32", "master"])
def test_fused_adamw_step_then_eval_no_grad_forward(case):
    from aecf_amd.optim import FusedAdamW
    pool, q, x, d = _setup(case)
    opt = FusedAdamW(list(pool.parameters()) + [q], lr=LR)
    pool.eval()
    _fwd(pool, q, x)                                                  # fills the caches
    before = _ref(pool, q, x)
    pool.train()
    _loss_backward(pool, q, x, d)
    opt.step()
    pool.eval()
    _check_no_grad(pool, q, x, before, _bounds(case), case)


@pytest.mark.parametrize("case", ["f32", "master"])
def test_fused_adamw_step_in_eval_mode_with_autograd(case):
    """Fine-tuning with dropout off: eval mode with gradients; the cached preparation also feeds the backward."""
    from aecf_amd.optim import FusedAdamW
    pool, q, x, d = _setup(case)
    opt = FusedAdamW(list(pool.parameters()) + [q], lr=LR)
    pool.eval()
    _loss_backward(pool, q, x, d)
    before = _ref(pool, q, x)
    opt.step()
    opt.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    y, w = _loss_backward(pool, q, xg, d)
    after = _ref(pool, q, x, d)
    bounds = _bounds(case)
    _assert_moved(before, after, bounds, case)
    got = dict(y=y, wbar=w, **_grads(pool, q, xg))
    _assert_close(got, after, bounds, case)
    other = _fresh(pool)
    q2, x2 = nn.Parameter(q.detach().clone()), x.clone().requires_grad_(True)
    y2, w2 = _loss_backward(other, q2, x2, d)
    assert torch.equal(y, y2) and torch.equal(w, w2) and torch.equal(xg.grad, x2.grad), case


@pytest.mark.parametrize("case", ["f32", "master"])
def test_fused_adamw_steps_between_no_grad_forwards_in_train_mode(case):
    """Metrics / EMA-teacher pattern: the module stays in train mode, no-grad forwards between the optimizer steps."""
    from aecf_amd.optim import FusedAdamW
    pool, q, x, d = _setup(case)
    opt = FusedAdamW(list(pool.parameters()) + [q], lr=LR)
    pool.train()
    _fwd(pool, q, x)
    for k in range(2):
        before = _ref(pool, q, x)
        opt.zero_grad(set_to_none=True)
        _loss_backward(pool, q, x, d)
        opt.step()
        _check_no_grad(pool, q, x, before, _bounds(case), (case, k))


# ---- torch's AdamW: foreach moves the version counters, the fused kernel does not (the optimizer step hook covers it) -------
@pytest.mark.parametrize("impl", ["foreach", "fused"])
@pytest.mark.parametrize("case", ["bf16", "f32", "master"])
def test_torch_adamw_step_then_eval_no_grad_forward(case, impl):
    pool, q, x, d = _setup(case)
    kw = dict(foreach=True) if impl == "foreach" else dict(fused=True)
    opt = torch.optim.AdamW(list(pool.parameters()) + [q], lr=LR, **kw)
    pool.eval()
    _fwd(pool, q, x)
    before = _ref(pool, q, x)
    _loss_backward(pool, q, x, d)                                     # (eval mode: the cached preparation serves it)
    opt.step()
    _check_no_grad(pool, q, x, before, _bounds(case), (case, impl))


# ---- the example model's captured training step ----------------------------------------------------------------------------
def _xray_batch(n, dev, seed):
    g = torch.Generator().manual_seed(seed)
    image, text = torch.randn(n, 512, generator=g), torch.randn(n, 512, generator=g)
    image[::5] = 0.0
    text[1::7] = 0.0
    labels = (torch.rand(n, 15, generator=g) < 0.2).float()
    return image.to(dev), text.to(dev), labels.to(dev)


class _PoolProbe:
    """The last (query, key) the model's pool was called with and its output."""

    def __init__(self, pool):
        self.handle = pool.register_forward_hook(self)

    def __call__(self, module, args, out):
        self.q, self.x, self.y = args[0][:1].detach(), args[1].detach(), out[0].detach()


@pytest.mark.parametrize("opt_kind", ["fused", "torch_capturable"])
def test_graphed_train_step_replays_then_eval_forward(opt_kind):
    from aecf_amd.optim import FusedAdamW
    from aecf_amd.xray import AECFModel, GraphedTrainStep
    dev = _dev()
    torch.manual_seed(21)
    model = AECFModel(512, 512, 15).to(dev).train()
    if opt_kind == "fused":
        opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    else:
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.01, capturable=True)
    step = GraphedTrainStep(model, opt, torch.nn.BCEWithLogitsLoss(), 64, 512, 512, 15, dev, warmup=2)
    for k in range(2):
        step(*_xray_batch(64, dev, 30 + k))
    image, text, _ = _xray_batch(200, dev, 99)
    model.eval()
    probe = _PoolProbe(model.attention_pool)
    with torch.no_grad():
        model(image, text)                                            # fills the pool's caches
    pool = model.attention_pool
    before = _ref(pool, probe.q, probe.x)
    for k in range(2):                                                # (the graph replays whatever mode the model is in)
        step(*_xray_batch(64, dev, 40 + k))
    with torch.no_grad():
        logits = model(image, text)
    probe.handle.remove()
    after = _ref(pool, probe.q, probe.x)
    bounds = _bounds("f32")
    _assert_moved(before, after, bounds, opt_kind)
    _assert_close(dict(y=probe.y), after, bounds, opt_kind)
    other = copy.deepcopy(model)
    for m in other.modules():
        if hasattr(m, "invalidate_cast_cache"):
            m.invalidate_cast_cache()
    with torch.no_grad():
        assert torch.equal(logits, other(image, text))


def test_train_xray_loop_in_miniature():
    """train_xray's loop: FusedAdamW steps, evaluate() under model.eval() + no_grad, more steps, evaluate() again."""
    from aecf_amd import train_xray
    from aecf_amd.optim import FusedAdamW
    from aecf_amd.xray import AECFModel
    dev = _dev()
    torch.manual_seed(22)
    model = AECFModel(512, 512, 15).to(dev)
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    crit = torch.nn.BCEWithLogitsLoss()
    v_image, v_text, v_labels = _xray_batch(300, dev, 77)
    maps = []
    for epoch in range(2):
        model.train()
        for it in range(3):
            image, text, labels = _xray_batch(64, dev, 100 * epoch + it)
            loss = crit(model(image, text), labels)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        maps.append(train_xray.evaluate(model, v_image, v_text, v_labels, "none"))
    with torch.no_grad():
        logits = model(v_image, v_text)
    fresh = AECFModel(512, 512, 15).to(dev)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    with torch.no_grad():
        want = fresh(v_image, v_text)
    assert torch.equal(logits, want)
    assert maps[-1] == train_xray.evaluate(fresh, v_image, v_text, v_labels, "none")


# ---- a query computed per call --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["bf16", "f32", "master"])
def test_computed_query_does_not_alias_the_previous_one(case):
    """q = f(z) with a new z per call, freed between calls: the caching allocator hands the new query the old one's block, at
    version 0 both -- the same address and version must not pass for the same query."""
    from aecf_amd.layer import _shared_query_base
    pool, _, x, _ = _setup(case)
    pdt = CASES[case][0]
    dev = x.device
    g = torch.Generator(device=dev).manual_seed(5)
    proj = torch.randn(64, E, device=dev, generator=g).to(pdt) * ((2.0 / E) ** 0.5 / 8)    # q ~ N(0, 2/E) as create_fusion_pool's
    f = lambda z_: (z_ @ proj).view(1, 1, E)
    f(torch.randn(1, 64, device=dev, generator=g).to(pdt))            # (warm the GEMM path)
    pool.eval()
    z = torch.randn(1, 64, device=dev, generator=g).to(pdt)
    q = f(z)
    qb = _shared_query_base(q.expand(B, -1, -1))
    ptr, ver = qb.data_ptr(), qb._version
    _fwd(pool, q, x)
    before = _ref(pool, q, x)
    del q, qb, z
    z = torch.randn(1, 64, device=dev, generator=g).to(pdt)
    q = f(z)
    qb = _shared_query_base(q.expand(B, -1, -1))
    assert qb.data_ptr() == ptr and qb._version == ver, "precondition: the new query reuses the old one's block and version"
    del qb
    _check_no_grad(pool, q, x, before, _bounds(case), case)


# ---- routes the version counters and storage already see: regression guards ------------------------------------------------
@pytest.mark.parametrize("route", ["new_parameter", "load_state_dict", "load_state_dict_assign", "data_assign"])
@pytest.mark.parametrize("case", ["bf16", "f32", "master"])
def test_parameter_replacement_routes(case, route):
    pool, q, x, _ = _setup(case)
    pdt = CASES[case][0]
    pool.eval()
    dev = x.device
    for k in range(3):                                                # a few checkpoints, one after the other
        _fwd(pool, q, x)
        before = _ref(pool, q, x)
        e = hot_shape_inputs(50 + k, B=B, M=M, E=E, H=H)
        new = {"attention.in_proj_weight": e["w_in"], "attention.in_proj_bias": e["b_in"],
               "attention.out_proj.weight": e["w_out"], "attention.out_proj.bias": e["b_out"]}
        new = {n: v.to(dev, pdt) for n, v in new.items()}
        a = pool.attention
        if route == "new_parameter":
            a.in_proj_weight = nn.Parameter(new["attention.in_proj_weight"])
            a.out_proj.weight = nn.Parameter(new["attention.out_proj.weight"])
            with torch.no_grad():
                a.in_proj_bias.copy_(new["attention.in_proj_bias"])
                a.out_proj.bias.copy_(new["attention.out_proj.bias"])
        elif route == "load_state_dict":
            pool.load_state_dict(new)
        elif route == "load_state_dict_assign":
            pool.load_state_dict(new, assign=True)
        else:
            for n, v in new.items():
                pool.get_parameter(n).data = v
        _check_no_grad(pool, q, x, before, _bounds(case), (case, route, k))


# ---- a captured inference forward ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["bf16", "f32", "master"])
def test_captured_eval_forward_prepares_for_itself(case):
    """An eval forward captured after a cache hit: its replays must see the parameters as they are when they run."""
    pool, q, x, _ = _setup(case)
    pool.eval()
    _fwd(pool, q, x)
    _fwd(pool, q, x)                                                  # a hit: this is what the capture would find
    before = _ref(pool, q, x)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        y_s, info_s = pool(q.expand(B, -1, -1), x, return_info=True)
    e = hot_shape_inputs(60, B=B, M=M, E=E, H=H)
    a = pool.attention
    with torch.no_grad():
        for p, k in ((a.in_proj_weight, "w_in"), (a.in_proj_bias, "b_in"), (a.out_proj.weight, "w_out"), (a.out_proj.bias, "b_out")):
            p.copy_(e[k])
    graph.replay()
    torch.cuda.synchronize()
    after = _ref(pool, q, x)
    bounds = _bounds(case)
    _assert_moved(before, after, bounds, case)
    y, w = y_s.clone(), info_s["attention_weights"].clone()
    _assert_close(dict(y=y, wbar=w), after, bounds, case)
    y2, w2 = _fwd(_fresh(pool), q, x)
    assert torch.equal(y, y2) and torch.equal(w, w2), case
    # ... and the eager forward after it sees the new parameters as well
    y3, w3 = _fwd(pool, q, x)
    assert torch.equal(y3, y2) and torch.equal(w3, w2), case
    del graph


# ---- nothing changes: the caches keep hitting --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["bf16", "f32", "master"])
def test_steady_inference_keeps_hitting_the_cache(case):
    pool, q, x, _ = _setup(case)
    pool.eval()
    y0, w0 = _fwd(pool, q, x)
    buf = pool._prep_cache[1]
    casts = {k: v[1] for k, v in pool._cast_cache.items()}
    assert (len(casts) == 4) == (case == "master")
    for n in (B, 77, 1024, B):
        xn = x[:n] if n <= B else x.repeat(n // B + 1, 1, 1)[:n].contiguous()
        y, w = _fwd(pool, q, xn)
        assert pool._prep_cache[1] is buf, n
        assert all(pool._cast_cache[k][1] is v for k, v in casts.items()), n
        if n == B:
            assert torch.equal(y, y0) and torch.equal(w, w0)
    with torch.no_grad():                                             # no_grad in train mode keeps hitting as well
        pool.train()
        _fwd(pool, q, x)
        buf = pool._prep_cache[1]
        _fwd(pool, q, x)
        assert pool._prep_cache[1] is buf
