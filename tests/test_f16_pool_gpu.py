"""float16 through the fusion pool, curriculum masking, entropy loss, the functional SDPA path and the general MHA path (ABI v10).

The truth is the float64 CPU oracle (oracle/aecf_oracle.py) run on the float16-representable inputs and parameters the kernels
read.  Errors are rel_err (max-abs over max-abs).  Bounds follow the bf16 convention, 1e-3 plus one output rounding:
float32-stored tensors (float32-master gradients included) 1e-3, float16-stored tensors 1e-3 + 2^-11.  Measured errors are
recorded with tests/helpers.record_errors."""
import copy
import ctypes
import math

import pytest
import torch
import torch.nn as nn

from tests.helpers import record_errors, rel_err

pytestmark = pytest.mark.gpu

F16 = torch.float16
F16_BOUND = 1e-3 + 2.0 ** -11
F32_BOUND = 1e-3
F16_MAX = 65504.0


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _h(t_):
    """the float16-representable float32 tensor nearest to t_ (what the kernels read)"""
    return t_.to(F16).to(torch.float32)


def _inputs(seed, B, M, E, H, bias=True, T=1):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)
    d = dict(B=B, M=M, E=E, H=H)
    d["x"] = _h(r(B, M, E) * torch.linspace(1.0, 2.0, M).view(1, M, 1))
    d["query"] = _h(r(1, 1, E) * (2.0 / E) ** 0.5 * 4.0)
    d["w_in"] = _h(r(3 * E, E) * (1.0 / E) ** 0.5)
    d["b_in"] = _h(r(3 * E) * 0.05) if bias else None
    d["w_out"] = _h(r(E, E) * (1.0 / E) ** 0.5)
    d["b_out"] = _h(r(E) * 0.05) if bias else None
    d["dy"] = _h(r(B, T, E))
    d["dwbar"] = _h(r(B, T, M) * 0.5)
    d["u"] = torch.rand(B, T, M, generator=g)
    return d


def _pool(d, pdt, curriculum=None, **kw):
    import aecf_amd
    E, H = d["E"], d["H"]
    pool = aecf_amd.MultimodalAttentionPool(E, num_heads=H, bias=d["b_in"] is not None, curriculum_masking=curriculum, **kw)
    a = pool.attention
    with torch.no_grad():
        a.in_proj_weight.copy_(d["w_in"])
        a.out_proj.weight.copy_(d["w_out"])
        if d["b_in"] is not None:
            a.in_proj_bias.copy_(d["b_in"])
            a.out_proj.bias.copy_(d["b_out"])
    return pool.to(_dev(), pdt)


def _grads(pool, q):
    a = pool.attention
    g = dict(dquery=q.grad, dw_in=a.in_proj_weight.grad, dw_out=a.out_proj.weight.grad)
    if a.in_proj_bias is not None:
        g.update(db_in=a.in_proj_bias.grad, db_out=a.out_proj.bias.grad)
    return g


def _oracle(d, kpm=None):
    from oracle import aecf_oracle as O
    c = lambda t_: None if t_ is None else t_.double()
    B, E, H = d["B"], d["E"], d["H"]
    q = c(d["query"]).expand(B, -1, -1)
    x = c(d["x"])
    f = O.mha_forward(q, x, x, c(d["w_in"]), c(d["b_in"]), c(d["w_out"]), c(d["b_out"]), H,
                      None if kpm is None else kpm.bool())
    b = O.mha_backward(q, x, x, c(d["w_in"]), c(d["b_in"]), c(d["w_out"]), H, f, c(d["dy"]), c(d["dwbar"]))
    b["dquery"] = b["dquery"].sum(0, keepdim=True)
    b["dx"] = b["dkey"] + b["dvalue"]
    return f, b


def _run_fused(d, pdt, qdt, mode="train", kpm=None):
    """forward + backward of the fused route with float16 activations; pdt / qdt: parameter / query dtype"""
    import aecf_amd
    dev = _dev()
    cm = None if mode == "none" else aecf_amd.CurriculumMasking(0.3)
    pool = _pool(d, pdt, cm)
    pool.train(mode != "eval")
    q = nn.Parameter(d["query"].to(dev, qdt))
    x = d["x"].to(dev, F16).requires_grad_(True)
    kw = {} if mode != "train" else dict(uniforms=d["u"].to(dev))
    y, info = pool(q.expand(d["B"], -1, -1), x, key_padding_mask=None if kpm is None else kpm.to(dev), return_info=True, **kw)
    w = info["attention_weights"]
    ((y.float() * d["dy"].to(dev)).sum() + (w.float() * d["dwbar"].to(dev)).sum()).backward()
    torch.cuda.synchronize()
    return pool, q, x, y, info


FUSED = [  # (B, M, E, H, bias)
    (300, 1, 128, 4, True),      # head_dim 32
    (300, 2, 256, 4, True),      # 64
    (300, 3, 512, 8, True),      # 64, the headline layout
    (300, 4, 768, 6, True),      # 128
    (300, 8, 1024, 8, True),     # 128
    (300, 3, 512, 16, False),    # 32, no bias
    (5000, 3, 256, 2, True),     # 128, several batch splits
]


@pytest.mark.parametrize("B,M,E,H,bias", FUSED, ids=[f"B{c[0]}_M{c[1]}_E{c[2]}_H{c[3]}{'' if c[4] else '_nobias'}" for c in FUSED])
def test_fused_f16_parameters_train(B, M, E, H, bias):
    """float16 parameters and activations, train mode with given uniforms: every output and gradient against the oracle,
    all stored in float16."""
    from oracle import aecf_oracle as O
    d = _inputs(100 + M * 7 + E, B, M, E, H, bias)
    pool, q, x, y, info = _run_fused(d, F16, F16)
    f, b = _oracle(d)
    assert y.dtype == F16 and info["attention_weights"].dtype == F16 and info["entropy"].dtype == F16
    assert info["mask_rate"].dtype == (torch.float32 if M > 1 else F16)    # ref :275 (and the one-key early-out, :160-167)
    grads = _grads(pool, q)
    assert all(g.dtype == F16 for g in grads.values()) and x.grad.dtype == F16
    m = O.curriculum_mask_train(f["wbar"], d["u"].double(), 0.3)
    errs = dict(y=rel_err(y.cpu(), f["y"]), wbar=rel_err(info["attention_weights"].cpu(), f["wbar"]),
                entropy=rel_err(info["entropy"].cpu(), m["entropy"]), dx=rel_err(x.grad.cpu(), b["dx"]))
    errs.update({k: rel_err(v.cpu(), b[k]) for k, v in grads.items()})
    record_errors(f"f16_fused_B{B}_M{M}_E{E}_H{H}", **errs)
    for k, e in errs.items():
        assert e < F16_BOUND, (k, e)
    # the mask rate is that of the returned masked weights (the pattern itself: test_fused_f16_mask_equals_oracle_on_kernel_weights)
    masked = info["masked_attention_weights"].float().cpu()
    if M > 1:
        assert torch.allclose(info["mask_rate"].cpu(), 1.0 - (masked != 0).float().mean(-1), atol=1e-6)
        assert float(info["mask_rate"].mean()) > 0.0


def test_fused_f16_mask_equals_oracle_on_kernel_weights():
    """The mask pattern bit for bit: the oracle fed the kernel's own float32 head-averaged weights and the same uniforms
    (as tests/test_pool_gpu.py does for bf16 / float32)."""
    from aecf_amd.layer import _PoolFunction
    from oracle import aecf_oracle as O
    dev = _dev()
    d = _inputs(7, 8192, 3, 128, 4)
    x, q = d["x"].to(dev, F16), d["query"].reshape(-1).to(dev, F16)
    U = d["u"].reshape(8192, 3)
    for p_base, k in ((0.15, 1), (1.0, 1), (0.7, 2)):
        y, attn_w, masked, ent, rate, _ = _PoolFunction.apply(
            x, q, d["w_in"].to(dev, F16), None, d["w_out"].to(dev, F16), None, None, U.to(dev), 4, 1, k, p_base, 0.7, 1e-8, True)
        r = O.curriculum_mask_train(attn_w.cpu(), U, p_base, 0.7, k)
        assert torch.equal((masked != 0).cpu(), r["masked"] != 0)
        assert torch.equal(rate.cpu(), r["mask_rate"])
        assert torch.allclose(masked.cpu(), r["masked"], rtol=1e-6, atol=1e-8)
        assert torch.allclose(ent.cpu(), r["entropy"], rtol=1e-5, atol=1e-6)


def test_fused_f16_key_padding_mask():
    """key_padding_mask on the fused route, rows with one modality left included"""
    B, M, E, H = 512, 4, 256, 4
    d = _inputs(21, B, M, E, H)
    g = torch.Generator().manual_seed(5)
    kpm = torch.rand(B, M, generator=g) < 0.4
    kpm[:, 0] = False                                    # at least one modality per row
    kpm[:64, 1:] = True                                  # the first 64 rows: ONLY modality 0 left
    pool, q, x, y, info = _run_fused(d, F16, F16, mode="none", kpm=kpm)
    f, b = _oracle(d, kpm)
    errs = dict(y=rel_err(y.cpu(), f["y"]), wbar=rel_err(info["attention_weights"].cpu(), f["wbar"]),
                dx=rel_err(x.grad.cpu(), b["dx"]))
    errs.update({k: rel_err(v.cpu(), b[k]) for k, v in _grads(pool, q).items()})
    record_errors("f16_fused_kpm", **errs)
    for k, e in errs.items():
        assert e < F16_BOUND, (k, e)
    w = info["attention_weights"].float().cpu().squeeze(1)
    assert torch.all(w[:64, 0] == 1.0) and torch.all(w[kpm] == 0)


@pytest.mark.parametrize("mode", ["eval", "none"])
def test_fused_f16_eval_and_no_curriculum(mode):
    d = _inputs(31, 700, 3, 512, 8)
    pool, q, x, y, info = _run_fused(d, F16, F16, mode=mode)
    f, b = _oracle(d)
    errs = dict(y=rel_err(y.cpu(), f["y"]), wbar=rel_err(info["attention_weights"].cpu(), f["wbar"]),
                dx=rel_err(x.grad.cpu(), b["dx"]))
    errs.update({k: rel_err(v.cpu(), b[k]) for k, v in _grads(pool, q).items()})
    if mode == "eval":
        from oracle import aecf_oracle as O
        errs["entropy"] = rel_err(info["entropy"].detach().cpu(), O.curriculum_mask_eval(f["wbar"])["entropy"])
        assert info["mask_rate"].dtype == F16
    record_errors(f"f16_fused_{mode}", **errs)
    for k, e in errs.items():
        assert e < F16_BOUND, (k, e)


def test_fused_f16_in_kernel_draw_equals_uniforms():
    """The statistics kernel's own Philox draw equals the uniforms= path bit for bit (float16 activations)"""
    import aecf_amd
    dev = _dev()
    d = _inputs(41, 3000, 3, 512, 8)
    pool = _pool(d, F16, aecf_amd.CurriculumMasking(0.5)).train()
    q = d["query"].to(dev, F16)
    x = d["x"].to(dev, F16)
    torch.cuda.manual_seed(777)
    y1, i1 = pool(q.expand(3000, -1, -1), x, return_info=True)
    torch.cuda.manual_seed(777)
    u = torch.rand(3000, 1, 3, device=dev)
    y2, i2 = pool(q.expand(3000, -1, -1), x, return_info=True, uniforms=u)
    assert torch.equal(y1, y2)
    assert torch.equal(i1["masked_attention_weights"], i2["masked_attention_weights"])
    assert torch.equal(i1["mask_rate"], i2["mask_rate"])
    assert float(i1["mask_rate"].mean()) > 0.05                       # the masks do something


@pytest.mark.parametrize("amp", [False, True], ids=["f32_masters", "amp_f32_query"])
def test_f32_masters_under_f16_activations(amp):
    """float32 master parameters under float16 activations (amp: the fusion query a float32 Parameter as well -- the AMP
    pattern; else a float16 one): the parameter gradients are float32-stored and within 1e-3 of the oracle."""
    d = _inputs(51, 2000, 3, 512, 8)
    pool, q, x, y, info = _run_fused(d, torch.float32, torch.float32 if amp else F16)
    f, b = _oracle(d)
    grads = _grads(pool, q)
    assert all(g.dtype == torch.float32 for k, g in grads.items() if k != "dquery")
    assert grads["dquery"].dtype == (torch.float32 if amp else F16)
    assert y.dtype == F16 and x.grad.dtype == F16
    errs = {k: rel_err(v.cpu(), b[k]) for k, v in grads.items()}
    record_errors(f"f16_masters_{'amp' if amp else 'f16q'}", y=rel_err(y.cpu(), f["y"]), dx=rel_err(x.grad.cpu(), b["dx"]), **errs)
    assert rel_err(y.cpu(), f["y"]) < F16_BOUND and rel_err(x.grad.cpu(), b["dx"]) < F16_BOUND
    for k, e in errs.items():
        assert e < (F16_BOUND if (k == "dquery" and not amp) else F32_BOUND), (k, e)


def test_amp_grad_scaler_loop():
    """The AMP pattern under torch.amp.GradScaler and AdamW: at a normal scale the unscaled gradients equal the gradients of
    an unscaled backward within the bound; at a scale that overflows the float16 intermediates the gradients hold a non-finite
    value, the scaler skips the step and the parameters stay unchanged bit for bit."""
    import aecf_amd
    dev = _dev()
    B, M, E, H = 1024, 3, 512, 8
    d = _inputs(61, B, M, E, H)
    pool = _pool(d, torch.float32, aecf_amd.CurriculumMasking(0.3)).train()
    q = nn.Parameter(d["query"].to(dev))
    params = [q] + list(pool.parameters())
    opt = torch.optim.AdamW(params, lr=1e-3)
    x = d["x"].to(dev, F16)
    dy = d["dy"].to(dev)

    def loss_of():
        u = d["u"].to(dev)
        y, info = pool(q.expand(B, -1, -1), x, return_info=True, uniforms=u)
        return (y.float() * dy).sum() + 1e-2 * pool.curriculum_masking.entropy_loss(info["entropy"]).float()

    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 8)
    for step in range(3):
        want = torch.autograd.grad(loss_of(), params)
        opt.zero_grad(set_to_none=True)
        scaler.scale(loss_of()).backward()
        scaler.unscale_(opt)
        for p, w in zip(params, want):
            assert p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all())
            assert rel_err(p.grad.cpu(), w.cpu()) < F32_BOUND, (step, tuple(p.shape), rel_err(p.grad.cpu(), w.cpu()))
        before = [p.detach().clone() for p in params]
        scaler.step(opt)
        scaler.update()
        assert any(not torch.equal(p, b_) for p, b_ in zip(params, before))          # a real step was taken
    # a scale that overflows float16: dy * 2^24 is beyond 65504
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 24)
    opt.zero_grad(set_to_none=True)
    scaler.scale(loss_of()).backward()
    assert any(not bool(torch.isfinite(p.grad).all()) for p in params)
    before = [p.detach().clone() for p in params]
    scale0 = scaler.get_scale()
    scaler.step(opt)
    scaler.update()
    assert all(torch.equal(p, b_) for p, b_ in zip(params, before))
    assert scaler.get_scale() < scale0


# ---------------- general route ----------------
def _general_oracle(qry, key, val, pool, H, kpm=None, attn_mask=None, drop_u=None, drop_p=0.0, dy=None, dwbar=None):
    from oracle import aecf_oracle as O
    a = pool.attention
    c = lambda t_: None if t_ is None else t_.detach().double().cpu()
    f = O.mha_forward(c(qry), c(key), c(val), c(a.in_proj_weight), c(a.in_proj_bias), c(a.out_proj.weight), c(a.out_proj.bias),
                      H, kpm, attn_mask, drop_u, drop_p)
    b = O.mha_backward(c(qry), c(key), c(val), c(a.in_proj_weight), c(a.in_proj_bias), c(a.out_proj.weight), H, f, dy, dwbar)
    return f, b


GENERAL = ["per_sample", "bool_mask", "float_mask", "float_kpm", "seq_first", "padded_e96", "dropout"]


@pytest.mark.parametrize("case", GENERAL)
def test_general_route_f16(case):
    """The general kernels in float16: per-sample queries with tgt_len > 1 and key != value throughout, plus one option per
    case; float16 parameters, every output and gradient against the oracle."""
    dev = _dev()
    B, T, S, E, H = 48, 3, 5, 128, 4
    if case == "padded_e96":
        E, H = 96, 3
    g = torch.Generator().manual_seed(GENERAL.index(case))
    r = lambda *shape: _h(torch.randn(*shape, generator=g))
    d = dict(B=B, M=S, E=E, H=H, w_in=r(3 * E, E) / math.sqrt(E), b_in=r(3 * E) * 0.05, w_out=r(E, E) / math.sqrt(E),
             b_out=r(E) * 0.05)
    drop = 0.25 if case == "dropout" else 0.0
    pool = _pool(d, F16, batch_first=case != "seq_first", dropout=drop).train(case == "dropout")
    qry, key, val = r(B, T, E), r(B, S, E), r(B, S, E) * 1.5
    dy, dwbar = r(B, T, E), r(B, T, S) * 0.5
    kpm = attn_mask = kpm_dev = mask_dev = None
    if case in ("bool_mask", "float_mask"):
        am = torch.rand(T, S, generator=g) < 0.3
        am[:, 0] = False
        attn_mask = am if case == "bool_mask" else torch.where(am, torch.tensor(-1e4), torch.randn(T, S, generator=g))
        mask_dev = attn_mask.to(dev)
    if case == "float_kpm":
        kb = torch.rand(B, S, generator=g) < 0.3
        kb[:, 0] = False
        kpm_dev = torch.where(kb, torch.tensor(float("-inf")), torch.zeros(())).to(dev)
        kpm = kb
    qd, kd, vd = (t_.to(dev, F16).requires_grad_(True) for t_ in (qry, key, val))
    args = (qd, kd, vd) if case != "seq_first" else tuple(t_.transpose(0, 1) for t_ in (qd, kd, vd))
    if case == "dropout":
        torch.cuda.manual_seed(99)
    y, info = pool(*args, key_padding_mask=kpm_dev, attn_mask=mask_dev, return_info=True)
    drop_u = None
    if case == "dropout":                                     # the layer's draw: torch.rand(B*H, T, S) from the default generator
        torch.cuda.manual_seed(99)
        drop_u = torch.rand(B * H, T, S, device=dev).cpu().double()
    if case == "seq_first":
        y = y.transpose(0, 1)
    w = info["attention_weights"]
    ((y.float() * dy.to(dev)).sum() + (w.float() * dwbar.to(dev)).sum()).backward()
    f, b = _general_oracle(qry, key, val, pool, H, None if kpm is None else kpm, attn_mask, drop_u, drop, dy.double(),
                           dwbar.double())
    a = pool.attention
    errs = dict(y=rel_err(y.detach().cpu(), f["y"]), wbar=rel_err(w.detach().cpu(), f["wbar"]),
                dquery=rel_err(qd.grad.cpu(), b["dquery"]), dkey=rel_err(kd.grad.cpu(), b["dkey"]),
                dvalue=rel_err(vd.grad.cpu(), b["dvalue"]), dw_in=rel_err(a.in_proj_weight.grad.cpu(), b["dw_in"]),
                db_in=rel_err(a.in_proj_bias.grad.cpu(), b["db_in"]), dw_out=rel_err(a.out_proj.weight.grad.cpu(), b["dw_out"]),
                db_out=rel_err(a.out_proj.bias.grad.cpu(), b["db_out"]))
    record_errors(f"f16_general_{case}", **errs)
    assert y.dtype == F16 and a.in_proj_weight.grad.dtype == F16
    for k, e in errs.items():
        assert e < F16_BOUND, (case, k, e)


# ---------------- functional and stand-alone pieces ----------------
def test_sdpa_and_functional_pool_f16():
    import aecf_amd
    from aecf_amd.layer import _scaled_dot_product_attention
    from oracle import aecf_oracle as O
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    q, k, v = (_h(torch.randn(64, n, 96, generator=g)) for n in (4, 7, 7))
    dout = _h(torch.randn(64, 4, 96, generator=g))
    qd, kd, vd = (t_.to(dev, F16).requires_grad_(True) for t_ in (q, k, v))
    out = _scaled_dot_product_attention(qd, kd, vd)
    (out.float() * dout.to(dev)).sum().backward()
    want = O.sdpa(q.double(), k.double(), v.double())
    dq, dk, dv = O.sdpa_backward(q.double(), k.double(), v.double(), dout.double())
    errs = dict(out=rel_err(out.detach().cpu(), want), dq=rel_err(qd.grad.cpu(), dq), dk=rel_err(kd.grad.cpu(), dk),
                dv=rel_err(vd.grad.cpu(), dv))
    record_errors("f16_sdpa", **errs)
    assert out.dtype == F16 and all(e < F16_BOUND for e in errs.values()), errs
    fo = aecf_amd.multimodal_attention_pool(qd.detach(), kd.detach(), vd.detach())      # the projection-free path
    assert fo.dtype == F16 and torch.equal(fo, out.detach())
    # a pool of fresh float32 parameters under float16 inputs (num_heads > 1 leaves the projection-free path)
    torch.manual_seed(0)
    fp = aecf_amd.multimodal_attention_pool(qd.detach()[:, :1, :64].contiguous(), kd.detach()[..., :64].contiguous(), num_heads=2)
    assert fp.dtype == F16 and fp.shape == (64, 1, 64) and bool(torch.isfinite(fp).all())


def test_curriculum_masking_f16_weights():
    import aecf_amd
    from oracle import aecf_oracle as O
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    w = _h(torch.softmax(torch.randn(2000, 1, 5, generator=g) * 2.0, -1))
    U = torch.rand(2000, 1, 5, generator=g)
    cm = aecf_amd.CurriculumMasking(base_mask_prob=0.6).to(dev).train()
    masked, info = cm(w.to(dev, F16), uniforms=U.to(dev))
    want = O.curriculum_mask_train(w.double(), U.double(), 0.6)
    assert masked.dtype == F16 and info["entropy"].dtype == F16
    assert torch.equal(masked.cpu() != 0, want["masked"] != 0)
    assert rel_err(masked.cpu(), want["masked"]) < F16_BOUND
    assert rel_err(info["entropy"].cpu(), want["entropy"]) < F16_BOUND


def test_entropy_loss_f16_with_non_finite_entries():
    import aecf_amd
    from oracle import aecf_oracle as O
    dev = _dev()
    for n in (1000, 20000):                                   # the one-block and the two-launch forms
        e = _h(torch.rand(n, generator=torch.Generator().manual_seed(n)) * 1.2)
        e[3], e[10], e[17] = float("nan"), float("inf"), float("-inf")
        cm = aecf_amd.CurriculumMasking()
        cm._last_seq_len = 3
        ed = e.to(dev, F16).requires_grad_(True)
        loss = cm.entropy_loss(ed)
        loss.backward()
        want = O.entropy_loss(e.double(), 3, 0.7)
        dwant = O.entropy_loss_backward(e.double(), 3, 0.7)
        assert loss.dtype == F16
        assert abs(float(loss) - float(want)) <= F16_BOUND * abs(float(want))
        assert rel_err(ed.grad.cpu(), dwant) < F16_BOUND
        assert float(ed.grad[3]) == 0.0 and float(ed.grad[10]) == 0.0


# ---------------- properties at the headline shape ----------------
def test_f16_headline_determinism_and_batch_independence():
    """[65536, 3, 512], 8 heads, float16 parameters: a second identical step is bit-identical, and rows 0..1023 computed alone
    equal the same rows of the full batch (outputs, attention weights, dx)."""
    import aecf_amd
    dev = _dev()
    B, M, E, H = 65536, 3, 512, 8
    d = _inputs(71, B, M, E, H)
    pool = _pool(d, F16, aecf_amd.CurriculumMasking(0.3)).train()
    q = nn.Parameter(d["query"].to(dev, F16))
    x_all = d["x"].to(dev, F16)
    dy, dw, u = d["dy"].to(dev), d["dwbar"].to(dev), d["u"].to(dev)

    def step(rows):
        for p in [q] + list(pool.parameters()):
            p.grad = None
        x = x_all[:rows].clone().requires_grad_(True)
        y, info = pool(q.expand(rows, -1, -1), x, return_info=True, uniforms=u[:rows])
        ((y.float() * dy[:rows]).sum() + (info["attention_weights"].float() * dw[:rows]).sum()).backward()
        return [y, info["attention_weights"], info["masked_attention_weights"], x.grad] + [p.grad.clone() for p in [q] + list(pool.parameters())]

    a, b = step(B), step(B)
    for i, (s, t_) in enumerate(zip(a, b)):
        assert torch.equal(s, t_), i
    c = step(1024)
    for i in range(4):
        assert torch.equal(a[i][:1024], c[i]), i
    assert all(bool(torch.isfinite(t_).all()) for t_ in a)


def test_f16_inference_cache_after_optimizer_step():
    """Eval-mode inference in float16 reuses the preparation while the parameters stand still and recomputes after an
    optimizer step: the result equals a cache-free copy of the module bit for bit and the oracle on the new parameters."""
    import aecf_amd
    dev = _dev()
    B, M, E, H = 65536, 3, 512, 8
    d = _inputs(81, B, M, E, H)
    pool = _pool(d, F16, aecf_amd.CurriculumMasking(0.3)).eval()
    q = nn.Parameter(d["query"].to(dev, F16))
    x = d["x"].to(dev, F16)
    with torch.no_grad():
        y0 = pool(q.expand(B, -1, -1), x)
        assert pool._prep_cache is not None
        y1 = pool(q.expand(B, -1, -1), x)
    assert torch.equal(y0, y1)
    # (SGD: AdamW on float16 parameters themselves divides by second moments that underflow in float16 -- 0.001 g^2 < 2^-24 --
    #  and writes inf / NaN, torch's behaviour for any module; float16 training keeps float32 masters, test_amp_grad_scaler_loop)
    opt = torch.optim.SGD([q] + list(pool.parameters()), lr=2e-3)
    for p in [q] + list(pool.parameters()):
        p.grad = torch.randn_like(p)
    opt.step()
    with torch.no_grad():
        y2 = pool(q.expand(B, -1, -1), x)
        fresh = copy.deepcopy(pool)
        fresh.invalidate_cast_cache()
        y3 = fresh(q.expand(B, -1, -1), x)
    assert bool(torch.isfinite(y2).all())
    assert torch.equal(y2, y3)
    assert not torch.equal(y2, y0)
    d2 = dict(d, query=q.detach().float().cpu().reshape(1, 1, E), w_in=pool.attention.in_proj_weight.detach().float().cpu(),
              b_in=pool.attention.in_proj_bias.detach().float().cpu(), w_out=pool.attention.out_proj.weight.detach().float().cpu(),
              b_out=pool.attention.out_proj.bias.detach().float().cpu(), B=4096, x=d["x"][:4096], dy=d["dy"][:4096],
              dwbar=d["dwbar"][:4096])
    f, _ = _oracle(d2)
    assert rel_err(y2[:4096].cpu(), f["y"]) < F16_BOUND


# ---------------- conversion and refusals ----------------
def test_cast_f32_to_f16_known_answers():
    """aecf_cast_f32_to_f16 against Tensor.half() bit for bit: ties to even, overflow to inf, subnormals, NaN -- the conversion
    every float16 store of the kernels uses (aecf_common.h: f32_to_f16_bits / pack_f16x2)."""
    from aecf_amd import _lib
    from aecf_amd.layer import _stream
    dev = _dev()
    e = 2.0 ** -11
    special = [1.0 + e, 1.0 + 3 * e, -(1.0 + e), 1.0 + 5 * e, 65504.0, 65519.0, 65520.0, 65536.0, 1e6, -1e6, float("inf"),
               float("-inf"), 2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -25, 2.0 ** -26, 1e-8, -1e-8, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25,
               6.1e-5, 0.0, -0.0, 1.0 / 3.0, float("nan")]
    g = torch.Generator().manual_seed(1)
    rnd = torch.cat([torch.randn(20000, generator=g) * 10.0 ** torch.randint(-9, 6, (20000,), generator=g).float(),
                     torch.randint(-2 ** 31, 2 ** 31 - 1, (5000,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)])
    srcs = [torch.tensor(special, dtype=torch.float32), rnd, rnd[:13].clone()]      # (13: the tail loop of a block)
    d_src = [s.to(dev) for s in srcs]
    d_dst = [torch.empty(s.numel(), dtype=F16, device=dev) for s in srcs]
    n = len(srcs)
    vp = ctypes.c_void_p
    _lib.check(_lib.load().aecf_cast_f32_to_f16(n, (vp * n)(*[s.data_ptr() for s in d_src]), (vp * n)(*[t_.data_ptr() for t_ in d_dst]),
                                                (ctypes.c_int64 * n)(*[s.numel() for s in srcs]), _stream()), "aecf_cast_f32_to_f16")
    for s, got in zip(srcs, d_dst):
        want = s.half()
        got = got.cpu()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)
        assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16))
    assert float(d_dst[0][0]) == 1.0 and float(d_dst[0][1]) == 1.0 + 4 * e and math.isinf(float(d_dst[0][6]))
    assert float(d_dst[0][5]) == F16_MAX


def test_f16_refusals_hold():
    import aecf_amd
    from aecf_amd import dp, losses, xray
    dev = _dev()
    z = torch.randn(64, 128, device=dev, dtype=F16)
    with pytest.raises(NotImplementedError):
        losses.info_nce(z, z)
    with pytest.raises(ValueError):
        xray.modality_frontend(z)
    with pytest.raises(ValueError):
        xray.front_pair(z, z)
    pool = aecf_amd.MultimodalAttentionPool(128, num_heads=4).to(dev)
    x = torch.randn(8, 3, 128, device=dev)
    with pytest.raises(NotImplementedError):
        pool(x[:, :1].double(), x.double())                     # float64 is not built
    dp.attach(pool, world=1)
    try:
        with pytest.raises(NotImplementedError, match="data-parallel"):
            pool(x[:, :1].half(), x.half())
        pool16 = aecf_amd.MultimodalAttentionPool(128, num_heads=4).to(dev, F16)
        dp.attach(pool16, world=1)
        with pytest.raises(NotImplementedError, match="data-parallel"):
            pool16(x[:, :1].half(), x.half())
        dp.detach(pool16)
        pool(x[:, :1], x)                                        # float32 still runs attached
    finally:
        dp.detach(pool)
