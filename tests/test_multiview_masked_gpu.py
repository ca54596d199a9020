"""Multi-view InfoNCE with missing views (aecf_nce_multi_masked_pair_coef / _pass1 / _loss / _grads, aecf_l2norm_masked_*,
losses.multiview_info_nce(..., key_padding_mask=...)) against float64, through the C ABI with ctypes, through the Python surface
and once through it on two ranks.  Cases, mask plans, the float64 reference and the derived elementwise bounds are those of
tests/multiview_masked_cases.py (tests/test_multiview_masked_cpu.py shows that the two float64 formulations agree, that the bounds
hold an emulation of the arithmetic and that they catch six broken masking rules).

C ABI: every shard of a global n x n problem as a rank would run it, with ITS rows of the mask as pres_loc and the whole mask as
pres_all -- pair_coef, pass 1, the shards' [P][n] column sums added in float32 (the all-reduce), the loss, the gradients.  The
absent slots of x keep their data (finite): the kernels must exclude them by the bytes.  Every output and the workspace come from
the Guarded helper of tests/test_abi_guards_gpu.py, filled with 0xFF (NaN as bf16 and as float32).  An element whose bound is 0
-- a loss row, a column sum or a gradient slot outside the pair's rows -- must be an exact zero."""
import functools
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import multiview_cases as C
from tests import multiview_masked_cases as K
from tests import nce_tile_cases as N
from tests.test_abi_guards_gpu import Guarded
from tests.test_multiview_gpu import _run_multi

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
CASE_PLAN_T = [(cid, plan, T) for cid in K.CASES for plan in K.PLANS for T in K.TEMPS]


def _libs():
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


@functools.lru_cache(maxsize=None)
def _want(cid, plan, T):
    c = C.make_case(cid)
    t = N.used_temperature(T)
    ref, bnd = K.reference(c["x"].to(DEV), K.make_mask(cid, plan), c["shards"], c["anchor"], t, C.score_errors(cid))
    return t, ref, bnd


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory_behind():
    """The measured outputs and references are shared between the tests of this module and dropped with it, and the allocator's
    cached blocks with them: tests that run later measure peaks of the caching allocator, whose block reuse depends on what lies
    cached."""
    yield
    import gc
    _measured.cache_clear()
    _want.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def _run_masked(x, absent, shards, anchor, T, grad_dtype=F32):
    """Every shard as a rank runs it; outputs laid out as K.reference (the workspace is spent by the gradients)."""
    _lib, lib, _ptr, _stream = _libs()
    n, M, d = x.shape
    k = -1 if anchor is None else anchor
    P = len(C.pairs(M, anchor))
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    pres_all = K.presence_bytes(absent).to(DEV)
    want_coef = torch.tensor(K.pair_coefs(absent, anchor), dtype=torch.float64).to(F32)     # float64, rounded once
    gd = Guarded(DEV)
    held, colsum = [], []
    for lo, hi in shards:
        rows = hi - lo
        xl, pl = x[lo:hi].contiguous(), pres_all[lo:hi].clone()
        wsb = lib.aecf_nce_multi_masked_workspace_bytes(rows, n, d, M, k)
        assert wsb == C.workspace_bytes_py(rows, n, d, M, k)
        ws = gd.new(wsb, 0xFF)
        cs = gd.tensor((P, n), F32, 0xFF)
        pc = gd.tensor((P,), F32, 0xFF)
        assert lib.aecf_nce_multi_masked_pair_coef(n, M, k, _ptr(pres_all), _ptr(pc), _stream()) == 0
        assert lib.aecf_nce_multi_masked_pass1(rows, n, d, M, k, _ptr(Tt), C.MIN_T, _ptr(xl), _ptr(x), _ptr(pl), _ptr(pres_all), _ptr(ws),
                                               wsb, _ptr(cs), _stream()) == 0
        assert torch.equal(pc.cpu(), want_coef), (pc, want_coef)
        held.append((xl, pl, ws, wsb, pc))
        colsum.append(cs)
    col_total = colsum[0].clone()
    for cs in colsum[1:]:
        col_total += cs
    gdt = _lib.AECF_BF16 if grad_dtype == BF16 else _lib.AECF_F32
    lr, dx = gd.tensor((P, n), F32, 0xFF), gd.tensor((n, M, d), grad_dtype, 0xFF)
    out = dict(colsum=colsum, loss_rows=lr, dx_loc=dx, dx_all=[], dT=[], pair_coef=held[0][4])
    for (lo, hi), (xl, pl, ws, wsb, pc) in zip(shards, held):
        rows = hi - lo
        lr_s = gd.tensor((P, rows), F32, 0xFF)
        assert lib.aecf_nce_multi_masked_loss(rows, n, lo, d, M, k, _ptr(Tt), C.MIN_T, _ptr(xl), _ptr(x), _ptr(pl), _ptr(pres_all),
                                              _ptr(col_total), _ptr(ws), wsb, _ptr(lr_s), _stream()) == 0
        lr[:, lo:hi] = lr_s
        dx_s, dxa_s = gd.tensor((rows, M, d), grad_dtype, 0xFF), gd.tensor((n, M, d), grad_dtype, 0xFF)
        d_t = gd.tensor((1,), F32, 0xFF)
        assert lib.aecf_nce_multi_masked_grads(rows, n, lo, d, M, k, _ptr(Tt), C.MIN_T, _ptr(pc), _ptr(xl), _ptr(x), _ptr(pl), _ptr(ws), wsb,
                                               None, gdt, _ptr(dx_s), _ptr(dxa_s), _ptr(d_t), _stream()) == 0
        torch.cuda.synchronize()
        dx[lo:hi] = dx_s
        out["dx_all"].append(dxa_s)
        out["dT"].append(float(d_t))
    torch.cuda.synchronize()
    gd.check()
    return out


@functools.lru_cache(maxsize=None)
def _measured(cid, plan, T, grad_dtype=F32):
    c = C.make_case(cid)
    return _run_masked(c["x"].to(DEV), K.make_mask(cid, plan), c["shards"], c["anchor"], T, grad_dtype)


@pytest.mark.parametrize("grad_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cid,plan,T", CASE_PLAN_T)
def test_c_abi_inside_the_derived_bounds(cid, plan, T, grad_dtype):
    """loss_rows, dx_loc, every shard's dx_all, their sum, the shards' column sums, dT and the value of every case and plan,
    elementwise; exact zeros outside a pair's rows"""
    out = _measured(cid, plan, T, grad_dtype)
    _, ref, bnd = _want(cid, plan, T)
    bf16 = grad_dtype == BF16
    got = {name: out[name] for name in ("colsum", "loss_rows", "dx_loc", "dx_all", "dT")}
    got["loss"] = float((out["loss_rows"].sum(dim=1) * out["pair_coef"]).sum())
    total = sum(g.double() for g in out["dx_all"])
    if not bf16:
        got["dx_all_sum"] = total
    r = K.ratios(got, ref, bnd, bf16=bf16)
    if bf16 and "dx_all" in r:
        # a sum of shares rounded to bf16 one by one: every share's rounding joins the summed bounds
        b = bnd["dx_all_sum"] + 2.0 ** -8 * sum(g.double().abs() for g in out["dx_all"])
        err = (total - ref["dx_all_sum"]).abs()
        assert not bool((err[b == 0] != 0).any())
        r["dx_all_sum"] = float((err / b.clamp_min(1e-300)).max())
    print(f"multiview_masked_parity case {cid} plan {plan} T {T} {'bf16' if bf16 else 'f32'}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items()))
    for name, v in r.items():
        assert v <= 1.0, (cid, plan, T, name, v)
    absent = K.make_mask(cid, plan).to(DEV)
    assert not bool(out["dx_loc"][absent].any())                    # the gradient at an absent (row, view) is an exact zero
    for share in out["dx_all"]:
        assert not bool(share[absent].any())
    if plan == "K3":                                                # the empty pair: zeros everywhere, out of P'
        assert float(out["pair_coef"][0]) == 0.0 and not bool(out["loss_rows"][0].any())
        assert all(not bool(cs[0].any()) for cs in out["colsum"])


@pytest.mark.parametrize("grad_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cid", K.CASES)
def test_all_present_has_the_bits_of_the_unmasked_calls(cid, grad_dtype):
    """K0: column sums, loss rows, dx_loc, dx_all and dT against aecf_nce_multi_* at coef = 0.5 / n / P on the same inputs"""
    c = C.make_case(cid)
    P = len(C.pairs(c["views"], c["anchor"]))
    for T in K.TEMPS:
        out = _measured(cid, "K0", T, grad_dtype)
        plain = _run_multi(c["x"].to(DEV), c["shards"], c["anchor"], T, 0.5 / c["x"].shape[0] / P, grad_dtype)
        assert torch.equal(out["loss_rows"], plain["loss_rows"]) and torch.equal(out["dx_loc"], plain["dx_loc"]), (cid, T)
        for k in range(len(c["shards"])):
            assert torch.equal(out["colsum"][k], plain["colsum"][k]), (cid, T, k)
            assert torch.equal(out["dx_all"][k], plain["dx_all"][k]), (cid, T, k)
            assert out["dT"][k] == plain["dT"][k], (cid, T, k)


def test_a_pair_of_one_row_adds_nothing():
    """K4: n_p = 1 -- the row is its own only key: its loss row is 0 to rounding (inside its bound), its weights cancel"""
    out = _measured("V3", "K4", 0.07)
    _, ref, bnd = _want("V3", "K4", 0.07)
    h = C.make_case("V3")["x"].shape[0] // 2
    assert float(out["pair_coef"][0]) == float(torch.tensor(0.5 / 3, dtype=F32)) and int((out["loss_rows"][0] != 0).sum()) <= 1
    assert abs(float(out["loss_rows"][0, h])) <= float(bnd["loss_rows"][0, h]) and abs(float(ref["loss_rows"][0, h])) <= 1e-12


def test_an_absent_twin_is_no_key():
    """K5: the twin r' of row r lacks a view of pair 0 and keeps its data: with r' kept as a key, row r's loss would move by about
    ln 2 (thousands of bounds).  Stated against the unmasked loss row of r, which does hold that key."""
    c = C.make_case("V3")
    absent = K.make_mask("V3", "K5")
    out, plain = _measured("V3", "K5", 0.025), _measured("V3", "K0", 0.025)
    _, ref, bnd = _want("V3", "K5", 0.025)
    n0 = C.pairs(c["views"], c["anchor"])[0][1]
    seen = 0
    for rp, r in c["twins"]:
        if bool(absent[rp, n0]):
            moved = float(plain["loss_rows"][0, r] - out["loss_rows"][0, r])
            assert moved > 1.0 and moved > 1000 * float(bnd["loss_rows"][0, r]), (rp, r, moved)    # two directions: about 2 ln 2
            assert float(out["loss_rows"][0, rp]) == 0.0
            seen += 1
    assert seen >= 3


# ---- the masked normalisation and poison in the absent slots (K6) ----
POISON = ("nan", "inf", "3e38", "rows")


def _poisoned(x0, absent, kind, g):
    x = x0.clone()
    if kind == "nan":
        x[absent] = float("nan")
    elif kind == "inf":
        x[absent] = float("inf")
    elif kind == "3e38":
        x[absent] = 3e38
    elif kind == "rows":
        x[absent] = (5.0 * torch.randn(int(absent.sum()), x0.shape[-1], generator=g)).to(x0.dtype).to(x0.device)
    else:
        x[absent] = 0.0
    return x


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_masked_normalisation_matches_the_plain_one_and_ignores_absent_slots(dtype):
    _lib, lib, _ptr, _stream = _libs()
    g = torch.Generator().manual_seed(41)
    b, M, d = 301, 3, 192
    x0 = (3.0 * torch.randn(b, M, d, generator=g)).to(dtype).to(DEV)
    absent = (torch.rand(b, M, generator=g) > 0.7).to(DEV)
    mask = absent.to(torch.uint8).reshape(-1).contiguous()
    dzn = torch.randn(b * M, d, generator=g).to(DEV)
    dt = _lib.AECF_BF16 if dtype == BF16 else _lib.AECF_F32
    zn0 = torch.empty(b * M, d, dtype=dtype, device=DEV)
    inv0 = torch.empty(b * M, dtype=F32, device=DEV)
    dz0 = torch.empty_like(zn0)
    assert lib.aecf_l2norm_forward(b * M, d, dt, 1e-12, _ptr(x0), _ptr(zn0), _ptr(inv0), _stream()) == 0
    assert lib.aecf_l2norm_backward(b * M, d, dt, _ptr(zn0), _ptr(inv0), _ptr(dzn), _ptr(dz0), _stream()) == 0
    flat = absent.reshape(-1)
    for kind in ("zero",) + POISON:
        x = _poisoned(x0, absent, kind, g)
        gd = Guarded(DEV)
        zn, inv, pres, dz = gd.tensor((b * M, d), dtype, 0xFF), gd.tensor((b * M,), F32, 0xFF), gd.tensor((b,), torch.uint8, 0xFF), \
            gd.tensor((b * M, d), dtype, 0xFF)
        assert lib.aecf_l2norm_masked_forward(b * M, d, M, dt, 1e-12, _ptr(x), _ptr(mask), _ptr(zn), _ptr(inv), _ptr(pres), _stream()) == 0
        bad = dzn.clone()
        if kind != "zero":
            bad[flat] = float("nan")                    # what arrives at an absent slot does not matter either
        assert lib.aecf_l2norm_masked_backward(b * M, d, dt, _ptr(zn), _ptr(inv), _ptr(bad), _ptr(mask), _ptr(dz), _stream()) == 0
        torch.cuda.synchronize()
        gd.check()
        assert torch.equal(zn[~flat], zn0[~flat]) and torch.equal(inv[~flat], inv0[~flat]) and torch.equal(dz[~flat], dz0[~flat]), kind
        for t in (zn[flat], inv[flat], dz[flat]):       # +0, bit for bit
            assert not bool(t.view(torch.int16 if t.dtype == BF16 else torch.int32).any()), kind
        assert torch.equal(pres, K.presence_bytes(absent)), kind


def _masked_step(losses, x0, absent, T0=0.07, anchor=None, as_views=False):
    x = x0.clone().requires_grad_(True)
    T = torch.tensor(T0, device=DEV, requires_grad=True)
    arg = [x[:, m] for m in range(x.shape[1])] if as_views else x
    loss = losses.multiview_info_nce(arg, temperature=T, anchor=anchor, key_padding_mask=absent)
    loss.backward()
    return loss.detach(), x.grad, T.grad


def test_poison_in_the_absent_slots_changes_no_bit():
    """K6 on the random plan: the absent slots of x hold NaN, +inf, 3e38 or unrelated finite rows -- loss, x.grad and dL/dT have
    the bits of the zero-filled run, and the gradient at every absent slot is an exact zero"""
    from aecf_amd import losses
    c = C.make_case("V3")
    absent = K.make_mask("V3", "K1").to(DEV)
    g = torch.Generator().manual_seed(43)
    x0 = (c["x"].float() * (1.0 + torch.rand(300, 3, 1, generator=g))).to(BF16).to(DEV)
    want = _masked_step(losses, _poisoned(x0, absent, "zero", g), absent)
    assert bool(torch.isfinite(want[0])) and bool(torch.isfinite(want[1]).all()) and bool(torch.isfinite(want[2]).all())
    assert not bool(want[1][absent].view(torch.int16).any())
    for kind in POISON:
        got = _masked_step(losses, _poisoned(x0, absent, kind, g), absent)
        for a, b in zip(got, want):
            assert torch.equal(a, b), kind
        assert not bool(got[1][absent].view(torch.int16).any()), kind


def test_unrelated_rows_in_the_absent_slots_change_no_bit_of_the_c_abi():
    """the same at the C ABI, which is handed the normalised rows: finite data in the absent slots against zeros there"""
    c = C.make_case("V2")
    absent = K.make_mask("V2", "K1")
    x = c["x"].to(DEV)
    xz = x.clone()
    xz[absent.to(DEV)] = 0.0
    a = _run_masked(x, absent, c["shards"], c["anchor"], 0.07, BF16)
    b = _run_masked(xz, absent, c["shards"], c["anchor"], 0.07, BF16)
    assert torch.equal(a["loss_rows"], b["loss_rows"]) and torch.equal(a["dx_loc"], b["dx_loc"]) and a["dT"] == b["dT"]
    for k in range(len(c["shards"])):
        assert torch.equal(a["colsum"][k], b["colsum"][k]) and torch.equal(a["dx_all"][k], b["dx_all"][k])


# ---- the Python surface ----
def _loop_of_info_nce(losses, x0, absent, anchor, T0=0.07):
    """what a caller does today: info_nce over index_select-ed subsets, pair by pair (a host read of every pair's rows)"""
    xl = x0.clone().requires_grad_(True)
    Tl = torch.tensor(T0, device=DEV, requires_grad=True)
    terms = []
    for m, n in C.pairs(x0.shape[1], anchor):
        idx = torch.nonzero(~absent[:, m] & ~absent[:, n]).flatten()
        if idx.numel():
            terms.append(losses.info_nce(xl[:, m].index_select(0, idx), xl[:, n].index_select(0, idx), temperature=Tl))
    loop = sum(terms) / len(terms)
    loop.backward()
    return loop.detach(), xl.grad, Tl.grad


@pytest.mark.parametrize("shape,anchor,plan", [((300, 3, 192), None, "K1"), ((300, 3, 192), None, "K3"), ((257, 8, 128), None, "K1"),
                                               ((300, 4, 192), 2, "K1"), ((300, 4, 192), 2, "K2")])
def test_python_surface_against_float64_autograd_of_the_definition(shape, anchor, plan):
    """float64 autograd of the definition on the UNNORMALISED input (normalised in float64; the mean over the non-empty pairs of
    info_nce on the pair's rows).  The library rounds the normalised rows to bf16 first, as the loop of info_nce over
    index_select-ed subsets does, and that rounding sets the distance of both from float64: loss, x.grad and dL/dT may be at most
    1.5 times as far from it as the loop is (the 1.5: the noise of a maximum over elements), plus, for the two scalars, their own
    derived bound on the rows the library normalised.  The value is also judged against float64 on those normalised rows, inside
    the summed bounds of the loss rows.  The sequence-of-views input gives the same bits."""
    from aecf_amd import losses
    cid = {(300, 3, 192): "V3", (257, 8, 128): "V8", (300, 4, 192): "V3A"}[shape]
    absent_cpu = K.make_mask(cid, plan)
    absent = absent_cpu.to(DEV)
    g = torch.Generator().manual_seed(79 + shape[1])
    b, M, d = shape
    base = torch.randn(b, 1, d, generator=g)
    x0 = ((base + 0.75 * torch.randn(b, M, d, generator=g)) * (1.0 + torch.rand(b, M, 1, generator=g))).to(BF16).to(DEV)
    x0 = _poisoned(x0, absent, "rows", g)

    x64 = x0.double().requires_grad_(True)
    t64 = torch.tensor(0.07, dtype=torch.float64, device=DEV, requires_grad=True)
    l64 = K.compacted_loss(x64 / x64.norm(dim=-1, keepdim=True), absent, anchor, t64)
    l64.backward()
    assert not bool(x64.grad[absent].any())

    loss, gx, gt = _masked_step(losses, x0, absent, anchor=anchor)
    assert gx.dtype == BF16 and gx.shape == x0.shape and loss.dtype == F32
    assert not bool(gx[absent].view(torch.int16).any())
    l_loop, gx_loop, gt_loop = _loop_of_info_nce(losses, x0, absent, anchor)

    with torch.no_grad():
        nx, _ = losses._L2NormMaskedSlots.apply(x0.reshape(b * M, d), absent.to(torch.uint8).reshape(-1).contiguous(), M, 1e-12)
        nx = nx.reshape(b, M, d)
    s_errs = []
    for m, n in C.pairs(M, anchor):
        u, v = nx[:, m].cpu(), nx[:, n].cpu()
        s_errs.append(float(((u.float() @ v.float().T).double() - u.double() @ v.double().T).abs().max()))
    ref, bnd = K.reference(nx, absent_cpu, [(0, b)], anchor, N.used_temperature(0.07), tuple(s_errs))
    assert abs(float(loss) - ref["loss"]) <= bnd["loss"], (float(loss), ref["loss"], bnd["loss"])

    err = float((gx.double() - x64.grad).abs().max())
    err_loop = float((gx_loop.double() - x64.grad).abs().max())
    l_err, l_err_loop = abs(float(loss) - float(l64.detach())), abs(float(l_loop) - float(l64.detach()))
    t_err, t_err_loop = abs(float(gt) - float(t64.grad)), abs(float(gt_loop) - float(t64.grad))
    print(f"multiview_masked_python shape {shape} anchor {anchor} plan {plan}: loss {float(loss):.6f} float64 {float(l64.detach()):.6f} "
          f"|d loss| {l_err:.3e} loop {l_err_loop:.3e} | max |d x.grad| {err:.3e} loop {err_loop:.3e} | |d T.grad| {t_err:.3e} loop "
          f"{t_err_loop:.3e} of {float(t64.grad):.3e}")
    assert err <= 1.5 * err_loop, (err, err_loop)
    assert l_err <= 1.5 * l_err_loop + bnd["loss"], (l_err, l_err_loop)
    assert t_err <= 1.5 * t_err_loop + bnd["dT"][0], (t_err, t_err_loop)

    loss2, gx2, gt2 = _masked_step(losses, x0, absent, anchor=anchor, as_views=True)
    assert torch.equal(loss2, loss) and torch.equal(gx2, gx) and torch.equal(gt2, gt)
    loss3, gx3, gt3 = _masked_step(losses, x0, absent.to(torch.uint8), anchor=anchor)       # uint8 is the same mask
    assert torch.equal(loss3, loss) and torch.equal(gx3, gx) and torch.equal(gt3, gt)


def test_no_view_anywhere_is_a_zero_loss_with_zero_gradients():
    from aecf_amd import losses
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(70, 3, 128, generator=g).to(BF16).to(DEV)
    absent = torch.ones(70, 3, dtype=torch.bool, device=DEV)
    absent[:, 0] = False                                            # one view per row: no pair has a row
    loss, gx, gt = _masked_step(losses, x0, absent)
    assert float(loss) == 0.0 and not bool(gx.any()) and float(gt) == 0.0


def test_no_mask_is_the_call_without_the_argument_and_all_present_is_close_to_it():
    """None: today's path, bit for bit.  An all-present mask: the same loss rows and weights (see the K0 test), the value summed
    pair by pair -- two float32 sums of the same P b <= 2^12 positive terms, each within 2^-20 of the exact sum: 2^-19 of the value;
    the gradients have the unmasked bits."""
    from aecf_amd import losses
    g = torch.Generator().manual_seed(11)
    x0 = (torch.randn(300, 1, 192, generator=g) + 0.6 * torch.randn(300, 3, 192, generator=g)).to(BF16).to(DEV)

    def run(**kw):
        x = x0.clone().requires_grad_(True)
        T = torch.tensor(0.07, device=DEV, requires_grad=True)
        loss = losses.multiview_info_nce(x, temperature=T, **kw)
        loss.backward()
        return loss.detach(), x.grad, T.grad

    plain, none = run(), run(key_padding_mask=None)
    for a, b in zip(plain, none):
        assert torch.equal(a, b)
    full = run(key_padding_mask=torch.zeros(300, 3, dtype=torch.bool, device=DEV))
    assert abs(float(full[0]) - float(plain[0])) <= 2.0 ** -19 * float(plain[0])
    assert torch.equal(full[1], plain[1]) and torch.equal(full[2], plain[2])


def test_captured_step_follows_a_mask_changed_in_place():
    from aecf_amd import losses
    g = torch.Generator().manual_seed(5)
    x0 = (torch.randn(300, 1, 192, generator=g) + 0.5 * torch.randn(300, 3, 192, generator=g)).to(BF16).to(DEV)
    m0, m1 = K.make_mask("V3", "K1").to(DEV), K.make_mask("V3", "K3").to(DEV)
    x = x0.clone().requires_grad_(True)
    T = torch.tensor(0.07, device=DEV, requires_grad=True)
    mask = m0.clone()

    def step():
        return losses.multiview_info_nce(x, temperature=T, key_padding_mask=mask)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            x.grad = T.grad = None
            step().backward()
    torch.cuda.current_stream().wait_stream(s)
    x.grad = T.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
        loss.backward()
    with torch.no_grad():
        T.copy_(torch.tensor(0.05))
        mask.copy_(m1)
    graph.replay()
    torch.cuda.synchronize()
    got = (loss.detach().clone(), x.grad.clone(), T.grad.clone())
    want = _masked_step(losses, x0, m1, T0=0.05)
    other = _masked_step(losses, x0, m0, T0=0.05)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(got[0], other[0])


N2, M2, D2 = 301, 3, 128            # two uneven shards: 151 and 150 rows


def _two_rank_inputs():
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(N2, 1, D2, generator=g) + 0.8 * torch.randn(N2, M2, D2, generator=g)).to(BF16)
    absent = torch.rand(N2, M2, generator=g) > 0.7
    absent[:150, 1] = True                                          # the shards' masks differ: rank 0 holds no pair with view 1
    return x, absent


def _masked_worker(rank, world, port, backend, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from aecf_amd import dp, losses
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lo, hi = dp.shard_bounds(N2, rank, world)
        x0, absent = _two_rank_inputs()
        x = x0[lo:hi].to(dev).requires_grad_(True)
        T = torch.tensor(0.07, device=dev, requires_grad=True)
        loss = losses.multiview_info_nce(x, temperature=T, key_padding_mask=absent[lo:hi].to(dev))
        loss.backward()
        torch.cuda.synchronize()
        q.put((rank, lo, hi, float(loss.detach()), (x.grad.float() / world).cpu().numpy(), float(T.grad) / world))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_equal_one_rank():
    """as tests/test_multiview_gpu.py::test_two_ranks_equal_one_rank and with its tolerances, with a mask that differs between the
    two uneven shards: every rank derives the pairs' row counts from the gathered presence bytes"""
    from aecf_amd import losses
    world = 2
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_masked_worker, args=(r, world, port, backend, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    x0, absent = _two_rank_inputs()
    want, gx, gt = _masked_step(losses, x0.to(DEV), absent.to(DEV))
    for rank, lo, hi, loss, gxr, gtr in res:
        assert abs(loss - float(want)) < 2e-3 * abs(float(want))
        rx = gx[lo:hi].float().cpu()
        assert (torch.from_numpy(gxr) - rx).abs().max() / rx.abs().max() < 2e-2
        assert not (torch.from_numpy(gxr)[absent[lo:hi]] != 0).any()
    assert abs(sum(r[5] for r in res) - float(gt)) < 2e-3 * abs(float(gt))
