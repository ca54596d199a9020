"""The score path of the shared-query pool backward on the device, per block and with dy, dwbar and the entropy gradient apart.

Cases, truths, bounds and what they can see: tests/pool_score_cases.py and tests/test_pool_score_cpu.py.  Every case names the
score kernel it must reach (dsu_ws_kernel with and without the low tiles, dscore_v_kernel from the saved V, bwd_g_kernel's
recompute pass) and pins it: ``aecf_pool_wants_saved_v``, ``aecf_pool_hilo_bwd_workspace_bytes`` and the restated launcher
conditions agree on the route, and the call goes through ``_PoolFunction``.  Each case runs
  * ``dy`` alone through the layer (the loss never touches info['attention_weights']: d_attn_w arrives as None), and once more
    with an all-zero d_attn_w: bit for bit the same six gradients;
  * ``dwbar`` alone (dy arrives as None), one case per route also under a boolean key_padding_mask;
  * ``dent`` alone: eval mode with a CurriculumMasking attached, loss entropy . gH, the truth formed from the float32 weights
    the forward saved for its backward (the kernel's own), which must round to the info['attention_weights'] it returned;
  * both dy and dwbar: the float64 sum of the separate truths, within the same per-block bounds.
Every block must lie inside its bound; with dy absent dw_out, db_out and the v blocks of dw_in / db_in are exactly zero, and the k
block of db_in (zero in exact arithmetic under any upstream) stays below bound(db_in.q) x max|db_in.q|.  error / bound per block
is recorded as ``pool_score_<case>_<upstream>`` (helpers.record_errors)."""
import ctypes

import pytest
import torch
import torch.nn as nn

from tests import pool_score_cases as C
from tests.helpers import record_errors, rel_err

pytestmark = pytest.mark.gpu

CASE_IDS = list(C.CASES)
SIX = ("dx", "dquery", "dw_in", "db_in", "dw_out", "db_out")


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _pin_route(case):
    from aecf_amd import _lib
    adt, pdt, B, M, E, H, route = C.CASES[case]
    lib = _lib.load()
    code = {C.bf16: _lib.AECF_BF16, C.f16: _lib.AECF_F16, C.f32: _lib.AECF_F32}[adt]
    desc = _lib.PoolDesc(B, M, E, H, code, 0, 1, 0.15, 0.7, 1e-8)
    assert lib.aecf_pool_check(ctypes.byref(desc)) == 0
    takes = adt == C.bf16 and C.dsu_ws_takes(M, E, H)
    # no saved V exactly where dsu_ws_kernel takes the shape (the one hi / lo case without room for its low tiles included:
    # tests/test_pool_score_cpu.py, test_route_and_ragged_last_chunk)
    assert (lib.aecf_pool_wants_saved_v(ctypes.byref(desc)) == 0) == takes
    hilo = adt == C.bf16 and lib.aecf_pool_hilo_bwd_workspace_bytes(ctypes.byref(desc)) > 0
    assert (hilo and C.is_master(case)) == (route in ("dsu_ws_lo", "bwd_g"))
    assert C.expected_route(case) == route


def _run(case, upstream, monkeypatch, kpm=False):
    """One forward and backward through the layer under the upstream ('dy', 'dy0' = dy with an all-zero d_attn_w, 'dwbar',
    'both', 'dent'): the six gradients as the device stored them, and the float32 weights the forward saved."""
    import aecf_amd
    from aecf_amd import layer
    adt, pdt, B, M, E, H, _ = C.CASES[case]
    dev = _dev()
    d = C.inputs(case, C.dent_scale(case) if upstream == "dent" else 1.0)
    cm = aecf_amd.CurriculumMasking() if upstream == "dent" else None
    pool = aecf_amd.MultimodalAttentionPool(E, num_heads=H, curriculum_masking=cm)
    a = pool.attention
    with torch.no_grad():
        for p, k in ((a.in_proj_weight, "w_in"), (a.in_proj_bias, "b_in"), (a.out_proj.weight, "w_out"), (a.out_proj.bias, "b_out")):
            p.copy_(d[k])
    pool = pool.to(dev, pdt)
    pool = pool.eval() if upstream == "dent" else pool.train()
    a = pool.attention
    q = nn.Parameter(d["query"].to(dev, pdt))
    x = d["x"].to(dev, adt).requires_grad_(True)
    taken, nodes = [], []
    for name in ("_PoolFunction", "_MhaFunction"):
        fn = getattr(layer, name)

        def wrap(orig, tag):
            def call(*args):
                out = orig(*args)
                taken.append(tag)
                nodes.append(out[0].grad_fn)
                return out
            return call
        monkeypatch.setattr(fn, "apply", wrap(fn.apply, name))
    y, info = pool(q.expand(B, -1, -1), x, key_padding_mask=d["kpm"].to(dev) if kpm else None, return_info=True)
    monkeypatch.undo()
    assert taken == ["_PoolFunction"], taken
    w = info["attention_weights"]
    w32 = nodes[0].saved_tensors[7].detach()               # attn_w: float32 [B, M], what the backward reads
    assert w32.dtype == torch.float32 and tuple(w32.shape) == (B, M)
    assert float((w32.view(B, 1, M) - w.detach().float()).abs().max()) <= (0.0 if adt == C.f32 else 2.0 ** -8)    # one rounding apart
    up = lambda k: d[k].to(dev, torch.float32)
    if upstream == "dy":
        loss = (y.float() * up("dy")).sum()
    elif upstream == "dy0":
        loss = (y.float() * up("dy")).sum() + (w.float() * torch.zeros(B, 1, M, device=dev)).sum()
    elif upstream == "dwbar":
        loss = (w.float() * up("dwbar")).sum()
    elif upstream == "both":
        loss = (y.float() * up("dy")).sum() + (w.float() * up("dwbar")).sum()
    else:
        assert info["entropy"].requires_grad and tuple(info["entropy"].shape) == (B, 1)
        loss = (info["entropy"].float() * up("gH")).sum()
    loss.backward()
    torch.cuda.synchronize()
    got = dict(dx=x.grad, dquery=q.grad, dw_in=a.in_proj_weight.grad, db_in=a.in_proj_bias.grad, dw_out=a.out_proj.weight.grad,
               db_out=a.out_proj.bias.grad)
    assert got["dx"].dtype == adt and all(got[k].dtype == pdt for k in SIX[1:])
    return {k: t_.detach().clone() for k, t_ in got.items()}, w32.detach().cpu()


def _blocks(got, E):
    return C.blocks(C.as_result({k: t_.double().cpu() for k, t_ in got.items()}), E)


def _check(case, tag, got, want, bnd, dy_absent):
    """error / bound of every checked block, printed and recorded before anything is asserted; then the zero blocks"""
    r = {n: rel_err(got[n], want[n]) / b for n, b in bnd.items()}
    qmax = float(want["db_in.q"].abs().max())
    r["db_in.k"] = float(got["db_in.k"].abs().max()) / (bnd["db_in.q"] * qmax)
    print("%s %s: error / bound  %s" % (case, tag, "  ".join("%s %.3f" % (n, v) for n, v in r.items())))
    record_errors("pool_score_%s_%s" % (case, tag), **{n.replace(".", "_"): v for n, v in r.items()})
    for n, v in r.items():
        assert v < 1.0, (case, tag, n, v, "error %.3e" % (v * bnd.get(n, bnd["db_in.q"])))
    if dy_absent:
        for n in C.ZERO_WITHOUT_DY:
            assert float(got[n].abs().max()) == 0.0, (case, tag, n)


@pytest.mark.parametrize("case", CASE_IDS)
def test_dy_alone_and_the_null_weight_gradient(case, monkeypatch):
    _pin_route(case)
    E = C.shape(case)[2]
    got, _ = _run(case, "dy", monkeypatch)
    want, bnd, _ = C.reference(case, "dy")
    zero, _ = _run(case, "dy0", monkeypatch)
    for k in SIX:                                           # d_attn_w == NULL and d_attn_w == 0: the same bits
        assert torch.equal(got[k], zero[k]), (case, k)
    _check(case, "dy", _blocks(got, E), want, bnd, dy_absent=False)


@pytest.mark.parametrize("case", CASE_IDS)
def test_dwbar_alone(case, monkeypatch):
    E = C.shape(case)[2]
    got, _ = _run(case, "dwbar", monkeypatch)
    want, bnd, _ = C.reference(case, "dwbar")
    _check(case, "dwbar", _blocks(got, E), want, bnd, dy_absent=True)


@pytest.mark.parametrize("case", C.KPM_CASES)
def test_dwbar_alone_under_a_key_padding_mask(case, monkeypatch):
    E = C.shape(case)[2]
    got, _ = _run(case, "dwbar", monkeypatch, kpm=True)
    want, bnd, _ = C.reference(case, "dwbar", True)
    _check(case, "dwbar_kpm", _blocks(got, E), want, bnd, dy_absent=True)
    blocked = C.inputs(case)["kpm"].to(got["dx"].device)
    assert float(got["dx"][blocked].abs().max()) == 0.0     # a blocked key has p = 0 in every head: no gradient reaches its row


@pytest.mark.parametrize("case", CASE_IDS)
def test_entropy_gradient_alone(case, monkeypatch):
    E = C.shape(case)[2]
    got, w32 = _run(case, "dent", monkeypatch)
    assert float(C.clamp_distance(w32.double()).min()) > 5e-5                # the kernel's own rows are clear of the clamps too
    want = C.truth(case, "dent", w_kernel=w32)
    bnd, _ = C.bounds(case, "dent", want, w_kernel=w32)
    _check(case, "dent", _blocks(got, E), want, bnd, dy_absent=True)


@pytest.mark.parametrize("case", CASE_IDS)
def test_superposition_of_dy_and_dwbar(case, monkeypatch):
    E = C.shape(case)[2]
    got, _ = _run(case, "both", monkeypatch)
    both, bnd, _ = C.reference(case, "both")
    a, b = C.reference(case, "dy")[0], C.reference(case, "dwbar")[0]
    want = {n: a[n] + b[n] for n in both}
    assert all(rel_err(want[n], both[n]) < 1e-12 for n in bnd)
    _check(case, "both", _blocks(got, E), want, bnd, dy_absent=False)
