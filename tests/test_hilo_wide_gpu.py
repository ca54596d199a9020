"""The hi/lo weight-gradient products (AECF_HILO_GRADS) at d = 768, d = 1024 and M = 4: float32 master parameters under bf16
activations get float32-accurate parameter gradients there by default (PoolOptions.hilo_grads = None), as at d = 256 / 512.

  * parity against the float64 oracle at every new family, ragged batches, 8 heads and one 4-head case: dW_in, db_in, dW_out,
    db_out and the float32-stored query gradient < 1e-4; y, the head-averaged weights and dx within the bf16 bounds;
  * magnitude stress at d = 1024, M = 4 (upstream gradients of 2^-40; inputs of 2^10 with the logits held);
  * hilo_grads = False still runs the default products (and allocates no low part of o);
  * properties: a re-run is bit-identical, dy x 2 doubles every gradient exactly, batch halves add up;
  * the caller's buffers: NaN-poisoned guard bands around every buffer of one hi/lo forward + backward per family;
  * data parallel: dp.attach(pool, world=2) stores the oracle's gradients / 2 within the same bounds."""
import ctypes

import pytest
import torch

from tests.helpers import BF16_BOUNDS, BF16_F32GRAD_BOUNDS, rel_err

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32
HILO_TOL = 1e-4
PARAMS = ("dw_in", "db_in", "dw_out", "db_out")


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _hilo_built(B, M, E, H):
    from aecf_amd import _lib
    desc = _lib.PoolDesc(B, M, E, H, _lib.AECF_BF16, 1, 1, 0.15, 0.7, 1e-8)
    return _lib.load().aecf_pool_hilo_bwd_workspace_bytes(ctypes.byref(desc)) > 0


class _Case:
    """Seeded bf16-representable parameters (float32 masters) and inputs; loss y . dy + wbar . dwbar."""

    def __init__(self, B, M, E, H, seed=23, x_scale=1.0, dy_scale=1.0):
        import aecf_amd
        self.B, self.M, self.E, self.H = B, M, E, H
        g = torch.Generator().manual_seed(seed + B + 7 * M + E + H)
        r = lambda *s: torch.randn(*s, generator=g)
        bf = lambda t_: t_.to(bf16).double()
        x = bf(r(B, M, E) * torch.linspace(1.0, 2.0, M).view(1, M, 1)) * x_scale
        w_in = bf(r(3 * E, E) / E ** 0.5)
        w_in[E:2 * E] /= x_scale                                # the key projection scaled back: the logits stay what they were
        self.ref = dict(x=x, w_in=w_in, b_in=bf(r(3 * E) * 0.05), w_out=bf(r(E, E) / E ** 0.5), b_out=bf(r(E) * 0.05),
                        q=bf(r(1, 1, E) * (2.0 / E) ** 0.5), dy=bf(r(B, 1, E)) * dy_scale, dwbar=bf(r(B, 1, M)) * dy_scale)
        pool = aecf_amd.MultimodalAttentionPool(E, num_heads=H)
        a = pool.attention
        with torch.no_grad():
            for p, k in ((a.in_proj_weight, "w_in"), (a.in_proj_bias, "b_in"), (a.out_proj.weight, "w_out"),
                         (a.out_proj.bias, "b_out")):
                p.copy_(self.ref[k])
        self.dev = _dev()
        self.pool = pool.to(self.dev, f32).train()
        self.q = torch.nn.Parameter(self.ref["q"].to(self.dev, f32))

    def run(self, rows=None, dy_mul=1.0):
        pool, dev = self.pool, self.dev
        sl = slice(None) if rows is None else rows
        for p in list(pool.parameters()) + [self.q]:
            p.grad = None
        x = self.ref["x"][sl].to(dev, bf16).requires_grad_(True)
        B = x.shape[0]
        y, info = pool(self.q.expand(B, -1, -1), x, return_info=True)
        w = info["attention_weights"]
        dy = self.ref["dy"][sl].to(dev, f32) * dy_mul
        dwbar = self.ref["dwbar"][sl].to(dev, f32) * dy_mul
        ((y.float() * dy).sum() + (w.float() * dwbar).sum()).backward()
        torch.cuda.synchronize()
        a = pool.attention
        got = dict(y=y, wbar=w, dx=x.grad, dquery=self.q.grad, dw_in=a.in_proj_weight.grad, db_in=a.in_proj_bias.grad,
                   dw_out=a.out_proj.weight.grad, db_out=a.out_proj.bias.grad)
        return {k: t_.detach().clone() for k, t_ in got.items()}

    def oracle(self):
        from oracle import aecf_oracle as O
        c, B, H = self.ref, self.B, self.H
        q = c["q"].expand(B, -1, -1)
        f = O.mha_forward(q, c["x"], c["x"], c["w_in"], c["b_in"], c["w_out"], c["b_out"], H)
        b = O.mha_backward(q, c["x"], c["x"], c["w_in"], c["b_in"], c["w_out"], H, f, c["dy"], c["dwbar"])
        return dict(y=f["y"], wbar=f["wbar"], dx=b["dkey"] + b["dvalue"], dquery=b["dquery"].sum(0, keepdim=True),
                    dw_in=b["dw_in"], db_in=b["db_in"], dw_out=b["dw_out"], db_out=b["db_out"])


def _errors(got, want):
    return {k: rel_err(got[k].double().cpu(), want[k]) for k in want}


def _assert_hilo_bounds(errs, what):
    for k in PARAMS + ("dquery",):
        assert errs[k] < HILO_TOL, (what, k, errs[k])
    for k in ("y", "wbar", "dx"):
        assert errs[k] < BF16_BOUNDS[k], (what, k, errs[k])


@pytest.fixture
def forward_calls(monkeypatch):
    """What the layer hands aecf_pool_forward: (flags, saved_v, saved_o_lo) per call."""
    from aecf_amd import _lib
    lib = _lib.load()
    orig = lib.aecf_pool_forward
    calls = []

    def spy(desc, args, stream):
        a = args._obj
        calls.append((a.flags, a.saved_v, a.saved_o_lo))
        return orig(desc, args, stream)

    monkeypatch.setattr(lib, "aecf_pool_forward", spy)
    return calls


# (B, M, E, H): every M at d = 768, d = 1024 at M = 2 and 4, d = 512 at M = 4; ragged batches; one case with 4 heads
PARITY = [
    (700, 1, 768, 8), (1100, 2, 768, 8), (4133, 3, 768, 8), (1100, 4, 768, 8), (700, 4, 768, 4),
    (1100, 2, 1024, 8), (700, 4, 1024, 8), (4133, 4, 512, 8), (1100, 4, 256, 8),
]


@pytest.mark.parametrize("B,M,E,H", PARITY, ids=[f"B{b}_M{m}_E{e}_H{h}" for b, m, e, h in PARITY])
def test_float32_master_gradients_are_float32_accurate(B, M, E, H, forward_calls):
    from aecf_amd import _lib
    assert _hilo_built(B, M, E, H)
    c = _Case(B, M, E, H)
    assert c.pool.options.hilo_grads is None                  # the default: on by itself for float32-stored gradients
    got = c.run()
    flags, saved_v, saved_o_lo = forward_calls[-1]
    assert flags & _lib.AECF_HILO_GRADS and saved_o_lo        # the hi/lo products ran ...
    assert not saved_v                                        # ... and the forward kept no per-modality V for them
    for k in PARAMS + ("dquery",):
        assert got[k].dtype == f32, k
    _assert_hilo_bounds(_errors(got, c.oracle()), (B, M, E, H))


@pytest.mark.parametrize("stress", ["tiny_grads", "large_inputs"])
def test_magnitude_stress_d1024_m4(stress):
    # (the low parts are bf16 numbers 2^-9 below their high parts: upstream gradients of 2^-40 put them near 1e-15, well inside
    #  bf16's float32 exponent range; inputs of 2^10 keep every product finite)
    kw = dict(dy_scale=2.0 ** -40) if stress == "tiny_grads" else dict(x_scale=2.0 ** 10)
    c = _Case(1100, 4, 1024, 8, seed=63, **kw)
    _assert_hilo_bounds(_errors(c.run(), c.oracle()), stress)


def test_default_products_still_reachable(forward_calls):
    from aecf_amd import _lib
    c = _Case(1100, 2, 768, 8)
    c.pool.options.hilo_grads = False
    got = c.run()
    flags, saved_v, saved_o_lo = forward_calls[-1]
    assert not flags & _lib.AECF_HILO_GRADS and not saved_o_lo
    assert saved_v                                            # (the default score gradient reads the saved V at d = 768)
    errs = _errors(got, c.oracle())
    for k in PARAMS + ("dquery", "y", "wbar", "dx"):
        assert errs[k] < BF16_F32GRAD_BOUNDS[k], (k, errs[k])
    assert max(errs[k] for k in ("dw_in", "dw_out")) > HILO_TOL   # the default products' operand roundings are visible


@pytest.mark.parametrize("B,M,E,H", [(4133, 4, 1024, 8), (1100, 2, 768, 8)])
def test_properties_at_new_shapes(B, M, E, H):
    c = _Case(B, M, E, H)
    full = c.run()
    again = c.run()
    for k in full:
        assert torch.equal(again[k], full[k]), ("re-run", k)
    twice = c.run(dy_mul=2.0)
    for k in PARAMS + ("dquery", "dx"):
        assert torch.equal(twice[k], full[k] * 2), ("dy x 2", k)
    h = B // 2
    lo, hi = c.run(rows=slice(0, h)), c.run(rows=slice(h, B))
    for k in PARAMS + ("dquery",):
        assert rel_err(lo[k] + hi[k], full[k]) < 2e-5, ("halves", k)


@pytest.mark.parametrize("B,M,E,H", [(1100, 2, 768, 8), (515, 4, 1024, 8), (700, 4, 512, 8)])
def test_hilo_calls_stay_inside_the_callers_buffers(B, M, E, H):
    from aecf_amd import _lib
    from aecf_amd.layer import _stream
    from tests.test_abi_guards_gpu import Guarded
    lib = _lib.load()
    dev = _dev()
    gd = Guarded(dev)
    desc = _lib.PoolDesc(B, M, E, H, _lib.AECF_BF16, 1, 1, 0.3, 0.7, 1e-8)
    hilo_bytes = lib.aecf_pool_hilo_bwd_workspace_bytes(ctypes.byref(desc))
    assert hilo_bytes > 0
    g = torch.Generator(device=dev).manual_seed(B + E)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    x = rnd(B, M, E).to(bf16)
    q = (rnd(E) * 0.3).to(bf16)
    w_in = (rnd(3 * E, E) / E ** 0.5).to(bf16)
    b_in = (rnd(3 * E) * 0.05).to(bf16)
    w_out = (rnd(E, E) / E ** 0.5).to(bf16)
    b_out = (rnd(E) * 0.05).to(bf16)
    dy = rnd(B, E).to(bf16)
    u = torch.rand(B, M, device=dev, generator=g)
    nan = 0xFF
    y = gd.tensor((B, E), bf16, nan)
    attn_w = gd.tensor((B, M), f32, nan)
    probs = gd.tensor((B, H, M), f32, nan)
    saved_o = gd.tensor((B, E), bf16, nan)
    saved_o_lo = gd.tensor((B, E), bf16, nan)
    masked_w, entropy, mask_rate = gd.tensor((B, M), f32, nan), gd.tensor((B,), f32, nan), gd.tensor((B,), f32, nan)
    saved_prep = gd.new(lib.aecf_pool_prep_bytes(ctypes.byref(desc)))
    ent_partial = gd.tensor(((B + 255) // 256,), f32, nan)
    fwd_ws_bytes = lib.aecf_pool_fwd_workspace_bytes(ctypes.byref(desc))
    fwd_ws = gd.new(fwd_ws_bytes)
    p = lambda t_: None if t_ is None else t_.data_ptr()
    flags = _lib.AECF_HILO_GRADS
    fa = _lib.PoolFwdArgs(p(x), p(q), p(w_in), p(b_in), p(w_out), p(b_out), None, p(u), p(y), p(attn_w), p(masked_w), p(entropy),
                          p(mask_rate), p(probs), p(saved_o), None, p(fwd_ws), fwd_ws_bytes, None, None, None, None, None,
                          p(saved_prep), None, 0.7 * float(torch.log(torch.tensor(float(M)))), flags, p(ent_partial), 0, 0, 0,
                          None, p(saved_o_lo), 0)
    _lib.check(lib.aecf_pool_forward(ctypes.byref(desc), ctypes.byref(fa), _stream()), "aecf_pool_forward")
    torch.cuda.synchronize()
    gd.check()
    for name, t_ in (("y", y), ("attn_w", attn_w), ("probs", probs), ("saved_o", saved_o), ("saved_o_lo", saved_o_lo)):
        assert torch.isfinite(t_.float()).all(), name
    # the low part is what it says: o - float(bf16(o)) is below half an ulp of o
    assert bool((saved_o_lo.float().abs() <= saved_o.float().abs() * 2.0 ** -8 + 1e-30).all())
    dx = gd.tensor((B, M, E), bf16, nan)
    dquery, dw_in, db_in = gd.tensor((E,), f32, nan), gd.tensor((3 * E, E), f32, nan), gd.tensor((3 * E,), f32, nan)
    dw_out, db_out = gd.tensor((E, E), f32, nan), gd.tensor((E,), f32, nan)
    bwd_ws = gd.new(hilo_bytes)
    ba = _lib.PoolBwdArgs(p(x), p(q), p(w_in), p(b_in), p(w_out), p(dy), None, None, p(attn_w), p(probs), p(saved_o), None,
                          p(dx), p(dquery), p(dw_in), p(db_in), p(dw_out), p(db_out), p(bwd_ws), hilo_bytes, None, _lib.AECF_F32,
                          flags, p(saved_prep), None, p(saved_o_lo), 1.0)
    _lib.check(lib.aecf_pool_backward(ctypes.byref(desc), ctypes.byref(ba), _stream()), "aecf_pool_backward")
    torch.cuda.synchronize()
    gd.check()
    for name, t_ in (("dx", dx), ("dquery", dquery), ("dw_in", dw_in), ("db_in", db_in), ("dw_out", dw_out), ("db_out", db_out)):
        assert torch.isfinite(t_.float()).all(), name
    ba.workspace_bytes = hilo_bytes - 1                       # one byte short is refused before anything is launched
    assert lib.aecf_pool_backward(ctypes.byref(desc), ctypes.byref(ba), _stream()) == -4


def test_data_parallel_float32_masters_d768():
    from aecf_amd import dp
    c = _Case(1100, 2, 768, 8)
    plain = c.run()
    st = dp.attach(c.pool, world=2)
    try:
        assert st.grad_scale == 0.5
        got = c.run()
        assert st.is_scaled(c.q)
    finally:
        dp.detach(c.pool)
    want = c.oracle()
    scaled = set(PARAMS) | {"dquery"}
    for k in want:
        ref = want[k] / 2 if k in scaled else want[k]
        e = rel_err(got[k].double().cpu(), ref)
        assert e < (HILO_TOL if k in scaled else BF16_BOUNDS[k]), (k, e)
    for k in scaled:                                          # bit for bit: the unattached run's gradients times 0.5
        assert torch.equal(got[k], plain[k] * 0.5), k
