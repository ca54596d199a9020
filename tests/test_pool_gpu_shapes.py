"""GPU parity sweep over the shapes the kernels template on: modality count 1..8, head count 1..16, embed sizes that
exercise ragged tiles (64, 192, 768, 1024), head sizes 16..256, batch sizes that are not multiples of any tile,
with and without key_padding_mask / gradient on the attention weights.  Checked against the CPU oracle.  The kernels
that serve shapes outside the weight-stationary engine are reached by shape here (E = 64 / 128 / 192, M >= 5), not by
a switch: the library has none."""
import pytest
import torch

from tests.helpers import assert_bf16_bounds, f32grad_bounds, record_errors, rel_err

pytestmark = pytest.mark.gpu

# (B, M, E, H)
SHAPES = [
    (1, 1, 64, 1),        # a single sample, a single modality (L <= 1 early-out of the masking)
    (37, 2, 64, 2),
    (100, 5, 128, 4),
    (77, 8, 128, 2),      # M = 8: the largest instantiation
    (130, 3, 192, 2),     # E = 192: ragged 128-wide tiles, head_dim 96
    (65, 2, 768, 8),      # BASELINE configs[2] shape (head_dim 96 spans tile boundaries)
    (70, 4, 1024, 8),     # BASELINE configs[4] shape
    (129, 3, 256, 16),    # 16 heads (head_dim 16: fp32 only)
    (200, 3, 512, 2),     # head_dim 256
    (513, 6, 64, 1),
    (96, 2, 512, 16),     # 16 heads of 32: two extra K-steps of the key-side term in the weight-stationary dx kernel
    (50, 4, 512, 4),      # M = 4: the largest modality count the weight-stationary kernels take
    (33, 1, 256, 4),      # E = 256 (one column group), a single modality
    (1100, 3, 512, 8),    # several row chunks per column group, ragged last step
]


def _case(B, M, E, H, dtype, kpm, seed):
    import aecf_amd
    from aecf_amd import layer
    from oracle import aecf_oracle as O
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    bf = lambda t_: t_.to(torch.bfloat16).float()
    x = bf(rnd(B, M, E) * torch.linspace(0.5, 2.0, M).view(1, M, 1))
    q = bf(rnd(1, 1, E) * 0.4)
    w_in = bf(rnd(3 * E, E) / E ** 0.5)
    b_in = bf(rnd(3 * E) * 0.05)
    w_out = bf(rnd(E, E) / E ** 0.5)
    b_out = bf(rnd(E) * 0.05)
    dy = bf(rnd(B, 1, E))
    dw = rnd(B, 1, M)
    U = torch.rand(B, 1, M, generator=g)
    mask = None
    if kpm and M > 1:
        mask = torch.rand(B, M, generator=g) < 0.3
        mask[:, 0] = False

    pool = aecf_amd.MultimodalAttentionPool(E, num_heads=H, curriculum_masking=aecf_amd.CurriculumMasking(0.3))
    with torch.no_grad():
        pool.attention.in_proj_weight.copy_(w_in)
        pool.attention.in_proj_bias.copy_(b_in)
        pool.attention.out_proj.weight.copy_(w_out)
        pool.attention.out_proj.bias.copy_(b_out)
    pool = pool.to(dev).train()                       # fp32 master parameters; activations in `dtype`
    xd = x.to(dev, dtype).requires_grad_(True)
    qd = q.to(dev).requires_grad_(True)
    out, info = pool(qd.to(dtype).expand(B, -1, -1) if dtype != torch.float32 else qd.expand(B, -1, -1), xd,
                     key_padding_mask=None if mask is None else mask.to(dev), return_info=True, uniforms=U)
    loss = (out.float() * dy.to(dev)).sum() + (info["attention_weights"].float() * dw.to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()

    qe = q.expand(B, -1, -1)
    f = O.mha_forward(qe, x, x, w_in, b_in, w_out, b_out, H, mask)
    b = O.mha_backward(qe, x, x, w_in, b_in, w_out, H, f, dy, dw)
    c = lambda t_: t_.detach().float().cpu()
    a = pool.attention
    got = dict(y=c(out), wbar=c(info["attention_weights"]), dx=c(xd.grad), dw_in=c(a.in_proj_weight.grad),
               db_in=c(a.in_proj_bias.grad), dw_out=c(a.out_proj.weight.grad), db_out=c(a.out_proj.bias.grad),
               dq=c(qd.grad))
    want = dict(y=f["y"], wbar=f["wbar"], dx=b["dkey"] + b["dvalue"], dw_in=b["dw_in"], db_in=b["db_in"],
                dw_out=b["dw_out"], db_out=b["db_out"], dq=b["dquery"].sum(0, keepdim=True))
    errs = {k: rel_err(got[k], want[k]) for k in got}
    if dtype != torch.float32:
        record_errors(f"sweep:B{B}_M{M}_E{E}_H{H}_{'kpm' if kpm else 'nomask'}", **errs)
    # masking of the kernel's own weights (the oracle on the kernel's float32 weights is the contract)
    if M > 1:
        m = O.curriculum_mask_train(c(info["attention_weights"]) if dtype == torch.float32 else f["wbar"], U, 0.3)
        agree = float(((c(info["masked_attention_weights"]) != 0) == (m["masked"] != 0)).float().mean())
    else:
        agree = 1.0
        assert float(info["entropy"].abs().max()) == 0.0 and float(info["mask_rate"].abs().max()) == 0.0
    return errs, agree


@pytest.mark.parametrize("shape", SHAPES, ids=[f"B{b}_M{m}_E{e}_H{h}" for b, m, e, h in SHAPES])
@pytest.mark.parametrize("kpm", [False, True], ids=["nomask", "kpm"])
def test_shapes_fp32(shape, kpm):
    B, M, E, H = shape
    errs, agree = _case(B, M, E, H, torch.float32, kpm, seed=B + M + E + H)
    for k, e in errs.items():
        assert e < 1e-5, (shape, k, e)
    assert agree == 1.0


@pytest.mark.parametrize("shape", [s for s in SHAPES if (s[2] // s[3]) % 32 == 0],
                         ids=[f"B{b}_M{m}_E{e}_H{h}" for b, m, e, h in SHAPES if (e // h) % 32 == 0])
@pytest.mark.parametrize("kpm", [False, True], ids=["nomask", "kpm"])
def test_shapes_bf16(shape, kpm):
    B, M, E, H = shape
    if kpm and M == 1:
        pytest.skip("a single modality cannot be padded away")
    errs, agree = _case(B, M, E, H, torch.bfloat16, kpm, seed=B + M + E + H + 1)
    # per tensor (tests/helpers.py): dquery = W_q^T (scale W_k u), u = ds^T x is a cancellation of bf16-rounded terms (ds
    # sums to zero over the modalities) -- the loosest of the outputs (4.4e-3 measured)
    assert_bf16_bounds(errs, f32grad_bounds(B, M, E, H), shape)
    assert agree > 0.99


def test_bf16_head_dim_16_runs_on_the_general_kernels():
    """head_dim 16 is not a bf16 MFMA K-step multiple: the shared-query kernels refuse it, the general path serves it."""
    B, M, E, H = 48, 3, 256, 16
    errs, agree = _case(B, M, E, H, torch.bfloat16, False, seed=3)
    # the general path materialises Q, K, V and their gradients in bf16 (as the reference module does in bf16), so it
    # carries a few more roundings than the collapsed shared-query kernels: 1e-2 of the largest magnitude
    for k, e in errs.items():
        assert e < 1e-2, (k, e)


_BACK_TO_BACK_SCRIPT = r"""
import json, sys, torch
sys.path.insert(0, {root!r})
import aecf_amd
dev = torch.device("cuda:0")
torch.manual_seed(3)
E, H, M = 128, 4, 3
q, pool = aecf_amd.create_fusion_pool(E, M, mask_prob=0.3, num_heads=H)
pool = pool.to(dev, torch.bfloat16).train()
q = torch.nn.Parameter(q.detach().to(dev, torch.bfloat16))
g = torch.Generator(device=dev).manual_seed(5)
# 50 steps queued back to back with DIFFERENT tensors and 12 distinct batch sizes, no synchronisation in between
sizes = [64 + 16 * (i % 12) for i in range(50)]
xs = [torch.randn(b, M, E, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True) for b in sizes]
dys = [torch.randn(b, 1, E, device=dev, generator=g).to(torch.bfloat16) for b in sizes]
us = [torch.rand(b, 1, M, device=dev, generator=g) for b in sizes]
torch.cuda.synchronize()
outs = []
for x, dy, u in zip(xs, dys, us):
    y, info = pool(q.expand(x.shape[0], -1, -1), x, return_info=True, uniforms=u)
    y.backward(dy)
    outs.append((y.detach(), info["masked_attention_weights"], x.grad))
torch.cuda.synchronize()
import hashlib
h = hashlib.sha256()
for y, m, dx in outs:
    for t_ in (y, m, dx):
        h.update(t_.float().cpu().numpy().tobytes())
h.update(pool.attention.in_proj_weight.grad.float().cpu().numpy().tobytes())
print("RESULT " + h.hexdigest())
"""


def test_unsynchronised_steps_back_to_back():
    """50 unsynchronised forward+backward steps on different tensors and 12 shapes (workspaces and saved buffers are recycled by
    the allocator while earlier launches are still queued) give bit-identical results run to run, with kernel arguments in host
    or in device memory (HIP_FORCE_DEV_KERNARG), and with the tiled kernels."""
    import os
    import subprocess
    import sys
    from tests.helpers import ROOT
    digests = {}
    for name, knobs in (("host_kernarg", {"HIP_FORCE_DEV_KERNARG": "0"}), ("dev_kernarg", {"HIP_FORCE_DEV_KERNARG": "1"}),
                        ("again", {"HIP_FORCE_DEV_KERNARG": "1"})):
        env = dict(os.environ, **knobs)
        out = subprocess.run([sys.executable, "-c", _BACK_TO_BACK_SCRIPT.format(root=ROOT)], env=env, capture_output=True,
                             text=True, timeout=280)
        assert out.returncode == 0, (name, out.stderr[-2000:])
        digests[name] = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]
    assert len(set(digests.values())) == 1, digests
