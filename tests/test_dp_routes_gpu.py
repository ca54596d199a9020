"""What a data-parallel pool stores before the collective, on every route, against the float64 oracle.

``dp.attach(pool, world=w)`` (no process group needed) promises that until the collective runs each parameter gradient -- and
the gradient of a leaf fusion query the call expands -- holds this rank's gradient divided by ``w``, while ``dx`` and any other
query (per-sample, computed) stay unscaled like inputs.  Every case runs one forward and backward over the whole batch
(loss y . dy + wbar . dwbar, as tests/test_inference_cache_gpu.py) and checks:
  * every gradient against the float64 oracle on the activation-dtype view of the parameters (``oracle.aecf_oracle``), the
    scaled ones divided by ``w``, at the suite's per-tensor bounds;
  * w = 2: bit for bit against an unattached run on the same inputs, scaled gradients times 0.5;
  * the route the case is meant to take (fused ``_PoolFunction`` or general ``_MhaFunction``), so a case cannot drift.
w = 3 is there so that code relying on a power of two cannot pass."""
import ctypes

import pytest
import torch
import torch.nn as nn

from tests.helpers import BF16_BOUNDS, f32grad_bounds, rel_err

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32
FP32_TOL = 1e-5
# general kernels in bf16: Q, K, V and their gradients are materialised in bf16 (tests/test_pool_gpu_shapes.py,
# test_bf16_head_dim_16_runs_on_the_general_kernels, asserts the same bound on every tensor)
GENERAL_BF16_TOL = 1e-2

# id: (B, M, E, H, parameter dtype, activation dtype, variant)
FUSED = {
    "bf16_B2048_M3_E512_H8": (2048, 3, 512, 8, bf16, bf16, None),
    "bf16_B300_M3_E512_H8": (300, 3, 512, 8, bf16, bf16, None),
    "bf16_M3_E256_H4": (512, 3, 256, 4, bf16, bf16, None),
    "bf16_M2_E768_H8": (256, 2, 768, 8, bf16, bf16, None),
    "bf16_M4_E1024_H8": (256, 4, 1024, 8, bf16, bf16, None),
    "bf16_M3_E128_H4": (512, 3, 128, 4, bf16, bf16, None),
    "f32_M4_E128_H4": (300, 4, 128, 4, f32, f32, None),
    "f32_M3_E512_H8": (256, 3, 512, 8, f32, f32, None),
    "master_M3_E512_H8": (256, 3, 512, 8, f32, bf16, None),
    "master_M4_E512_H8": (256, 4, 512, 8, f32, bf16, None),
}
GENERAL = {
    "attn_mask_bool2d": (200, 3, 128, 4, f32, f32, "attn_mask"),
    "key_is_not_value": (200, 3, 128, 4, f32, f32, "kv"),
    "float_key_padding_mask": (200, 3, 128, 4, f32, f32, "float_kpm"),
    "per_sample_queries": (200, 3, 128, 4, f32, f32, "per_sample"),
    "M9": (96, 9, 128, 4, f32, f32, None),
    "padded_E40_H2": (64, 3, 40, 2, f32, f32, None),
    "bf16_head_size_16": (128, 3, 128, 8, bf16, bf16, None),
    "dropout_0.25": (96, 3, 128, 4, f32, f32, "dropout"),
}
CASES = {**{k: v + ("fused",) for k, v in FUSED.items()}, **{k: v + ("general",) for k, v in GENERAL.items()}}
PARAMS = ("dw_in", "db_in", "dw_out", "db_out")


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _fused_kernels_take(B, M, E, H, dt):
    """The predicate the layer routes by (``_pool_facts``): the shared-query kernels accept the shape."""
    from aecf_amd import _lib
    desc = _lib.PoolDesc(B, M, E, H, {bf16: _lib.AECF_BF16, f32: _lib.AECF_F32}[dt], 0, 1, 0.15, 0.7, 1e-8)
    return _lib.load().aecf_pool_check(ctypes.byref(desc)) == 0


def _bounds(case):
    B, M, E, H, pdt, adt, _, route = CASES[case]
    if adt == f32:
        g = 2 * FP32_TOL
        return dict(y=FP32_TOL, wbar=FP32_TOL, dx=FP32_TOL, dkey=FP32_TOL, dvalue=FP32_TOL, dquery=g, dw_in=g, db_in=g,
                    dw_out=g, db_out=g)
    if route == "general":
        return {k: GENERAL_BF16_TOL for k in ("y", "wbar", "dx", "dquery") + PARAMS}
    return f32grad_bounds(B, M, E, H) if pdt != adt else BF16_BOUNDS


class _Case:
    """Seeded bf16-representable parameters and inputs for one case, and a pool holding them."""

    def __init__(self, case, seed=17):
        import aecf_amd
        B, M, E, H, pdt, adt, variant, route = CASES[case]
        self.B, self.M, self.E, self.H, self.adt, self.variant, self.route = B, M, E, H, adt, variant, route
        g = torch.Generator().manual_seed(seed + B + M + E)
        r = lambda *s: torch.randn(*s, generator=g)
        bf = lambda t_: t_.to(bf16).double()
        dev = _dev()
        self.dev = dev
        x = bf(r(B, M, E) * torch.linspace(1.0, 2.0, M).view(1, M, 1))
        self.ref = dict(x=x, v=bf(r(B, M, E)) if variant == "kv" else x, w_in=bf(r(3 * E, E) / E ** 0.5),
                        b_in=bf(r(3 * E) * 0.05), w_out=bf(r(E, E) / E ** 0.5), b_out=bf(r(E) * 0.05),
                        q=bf(r(B if variant == "per_sample" else 1, 1, E) * (2.0 / E) ** 0.5),
                        dy=bf(r(B, 1, E)), dwbar=bf(r(B, 1, M)))
        self.kpm = None
        if variant == "float_kpm":                         # additive, torch semantics for a float key_padding_mask
            self.kpm = (torch.rand(B, M, generator=g) * -2.0).double()
        self.attn_mask = None
        if variant == "attn_mask":
            self.attn_mask = torch.tensor([[False, True, False]])
        pool = aecf_amd.MultimodalAttentionPool(E, num_heads=H, dropout=0.25 if variant == "dropout" else 0.0)
        a = pool.attention
        with torch.no_grad():
            for p, k in ((a.in_proj_weight, "w_in"), (a.in_proj_bias, "b_in"), (a.out_proj.weight, "w_out"),
                         (a.out_proj.bias, "b_out")):
                p.copy_(self.ref[k])
        self.pool = pool.to(dev, pdt).train()
        self.q = nn.Parameter(self.ref["q"].to(dev, pdt))

    def run(self, monkeypatch):
        """Forward + backward on the whole batch; returns the gradients and the uniforms of the dropout draw."""
        from aecf_amd import layer
        pool, dev, adt = self.pool, self.dev, self.adt
        for p in list(pool.parameters()) + [self.q]:
            p.grad = None
        x = self.ref["x"].to(dev, adt).requires_grad_(True)
        v = self.ref["v"].to(dev, adt).requires_grad_(True) if self.variant == "kv" else x
        q = self.q if self.variant == "per_sample" else self.q.expand(self.B, -1, -1)      # (master weights: a float32 query)
        kpm = None if self.kpm is None else self.kpm.to(dev, f32)
        am = None if self.attn_mask is None else self.attn_mask.to(dev)
        taken = []
        for name in ("_PoolFunction", "_MhaFunction"):
            fn = getattr(layer, name)
            monkeypatch.setattr(fn, "apply", (lambda orig, tag: lambda *a: (taken.append(tag), orig(*a))[1])(fn.apply, name))
        torch.manual_seed(31)
        y, info = pool(q, x, v, key_padding_mask=kpm, attn_mask=am, return_info=True)
        monkeypatch.undo()
        assert taken == (["_PoolFunction"] if self.route == "fused" else ["_MhaFunction"]), taken
        w = info["attention_weights"]
        ((y.float() * self.ref["dy"].to(dev, f32)).sum() + (w.float() * self.ref["dwbar"].to(dev, f32)).sum()).backward()
        torch.cuda.synchronize()
        u = None
        if self.variant == "dropout":                      # the module's own torch.rand draw, reproduced by seed
            torch.manual_seed(31)
            u = torch.rand(self.B * self.H, 1, self.M, device=dev).double().cpu()
        a = pool.attention
        got = dict(y=y.detach(), wbar=w.detach(), dquery=self.q.grad, dw_in=a.in_proj_weight.grad, db_in=a.in_proj_bias.grad,
                   dw_out=a.out_proj.weight.grad, db_out=a.out_proj.bias.grad)
        if self.variant == "kv":
            got.update(dkey=x.grad, dvalue=v.grad)
        else:
            got["dx"] = x.grad
        return {k: t_.detach().clone() for k, t_ in got.items()}, u

    def oracle(self, u):
        from oracle import aecf_oracle as O
        c, B, H, M = self.ref, self.B, self.H, self.M
        # the activation-dtype view of the parameters is what the kernels read; every value here is bf16-representable
        q = c["q"] if self.variant == "per_sample" else c["q"].expand(B, -1, -1)
        am = None
        if self.attn_mask is not None:
            am = self.attn_mask
        if self.kpm is not None:
            am = self.kpm.view(B, 1, 1, M).expand(B, H, 1, M).reshape(B * H, 1, M)
        p_drop = 0.25 if u is not None else 0.0
        f = O.mha_forward(q, c["x"], c["v"], c["w_in"], c["b_in"], c["w_out"], c["b_out"], H, None, am, u, p_drop)
        b = O.mha_backward(q, c["x"], c["v"], c["w_in"], c["b_in"], c["w_out"], H, f, c["dy"], c["dwbar"])
        out = dict(y=f["y"], wbar=f["wbar"], dw_in=b["dw_in"], db_in=b["db_in"], dw_out=b["dw_out"], db_out=b["db_out"],
                   dquery=b["dquery"] if self.variant == "per_sample" else b["dquery"].sum(0, keepdim=True))
        if self.variant == "kv":
            out.update(dkey=b["dkey"], dvalue=b["dvalue"])
        else:
            out["dx"] = b["dkey"] + b["dvalue"]
        return out


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_attached_gradients_are_the_oracle_over_world(case, world, monkeypatch):
    from aecf_amd import dp
    c = _Case(case)
    B, M, E, H, _, adt, _, route = CASES[case]
    assert _fused_kernels_take(B, M, E, H, adt) == (route == "fused" or c.variant is not None), case
    plain, u = c.run(monkeypatch) if world == 2 else (None, None)
    st = dp.attach(c.pool, world=world)
    try:
        assert st.grad_scale == 1.0 / world
        got, u = c.run(monkeypatch)
        shared = c.variant != "per_sample"
        assert st.is_scaled(c.q) == shared                  # a per-sample query is an input: all_reduce_grads divides it
    finally:
        dp.detach(c.pool)
    want = c.oracle(u)
    if u is not None:
        assert 0.1 < float((u < 0.25).double().mean()) < 0.4                       # the draw drops about a quarter
    scaled = set(PARAMS) | ({"dquery"} if shared else set())
    bounds = _bounds(case)
    for k, g in got.items():
        ref = want[k] / world if k in scaled else want[k]
        e = rel_err(g.float().cpu(), ref)
        assert e < bounds[k], (case, world, k, e, bounds[k])
    if plain is not None:                                   # w = 2: bit for bit, the scaled gradients times 0.5
        for k, g in got.items():
            ref = (plain[k].float() * 0.5).to(plain[k].dtype) if k in scaled else plain[k]
            assert torch.equal(g, ref), (case, k)
