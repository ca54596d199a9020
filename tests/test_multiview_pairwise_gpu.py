"""Multi-view InfoNCE with a temperature and a weight per pair (aecf_nce_multi_pp_pair_coef / _pass1 / _loss / _grads,
losses.multiview_info_nce(x, temperature=[P], pair_weights=[P])) against float64, against the two-view entry points and against
the one-temperature forms, through the C ABI with ctypes, through the Python surface and once through it on two ranks.  Cases,
temperatures, weights, mask plans, the float64 reference and the derived elementwise bounds -- the new bound of every dT_p among
them -- are those of tests/multiview_pairwise_cases.py (tests/test_multiview_pairwise_cpu.py shows that the reference is the float64
autograd of the definition, that the bounds hold an emulation of the arithmetic, and what they catch).

C ABI: every shard of a global n x n problem as a rank would run it -- the pair coefficients, pass 1, the shards' [P][n] column
sums added in float32 (the all-reduce), the loss, the gradients.  Every output and the workspace come from the Guarded helper of
tests/test_abi_guards_gpu.py, sized exactly as documented and filled with 0xFF (NaN as bf16 and as float32)."""
import functools
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import multiview_cases as C
from tests import multiview_masked_cases as K
from tests import multiview_pairwise_cases as Q
from tests import nce_tile_cases as N
from tests.test_abi_guards_gpu import Guarded
from tests.test_multiview_gpu import _run_multi, _run_two_view
from tests.test_multiview_masked_gpu import _run_masked

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
# (case, plan): plan None is the form without presence bytes (both pointers NULL)
RUNS = [(cid, None) for cid in Q.CASES] + [(cid, plan) for cid in ("V2", "V4") for plan in Q.PLANS] + [("V3A", "KE")]


def _libs():
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


def _absent(cid, plan):
    c = C.make_case(cid)
    return torch.zeros(c["x"].shape[0], c["views"], dtype=torch.bool) if plan is None else Q.make_mask(cid, plan)


@functools.lru_cache(maxsize=None)
def _want(cid, plan):
    c = C.make_case(cid)
    return Q.reference(c["x"].to(DEV), _absent(cid, plan), c["shards"], c["anchor"], Q.temperatures(cid), Q.weights(cid),
                       C.score_errors(cid))


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory_behind():
    yield
    import gc
    _measured.cache_clear()
    _want.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def _run_pp(x, absent, shards, anchor, temps, weights, grad_dtype=F32, masked=True, with_dt=True):
    """Every shard as a rank runs it; outputs laid out as Q.reference (the workspace is spent by the gradients).  masked False:
    the presence pointers are NULL (absent must be all False)."""
    _lib, lib, _ptr, _stream = _libs()
    n, M, d = x.shape
    k = -1 if anchor is None else anchor
    P = len(C.pairs(M, anchor))
    Tt = torch.tensor(temps, dtype=F32, device=DEV)
    Wt = None if weights is None else torch.tensor(weights, dtype=F32, device=DEV)
    pres_all = K.presence_bytes(absent).to(DEV) if masked else None
    want_coef = torch.tensor(Q.pair_coefs(absent, anchor, weights), dtype=torch.float64).to(F32)        # float64, rounded once
    gd = Guarded(DEV)
    held, colsum = [], []
    for lo, hi in shards:
        rows = hi - lo
        xl = x[lo:hi].contiguous()
        pl = pres_all[lo:hi].clone() if masked else None
        wsb = lib.aecf_nce_multi_pp_workspace_bytes(rows, n, d, M, k)
        assert wsb == Q.workspace_bytes_py(rows, n, d, M, k)
        ws = gd.new(wsb, 0xFF)
        cs = gd.tensor((P, n), F32, 0xFF)
        pc = gd.tensor((P,), F32, 0xFF)
        assert lib.aecf_nce_multi_pp_pair_coef(n, M, k, _ptr(pres_all), _ptr(Wt), _ptr(pc), _stream()) == 0
        assert lib.aecf_nce_multi_pp_pass1(rows, n, d, M, k, _ptr(Tt), C.MIN_T, _ptr(xl), _ptr(x), _ptr(pl), _ptr(pres_all), int(with_dt),
                                           _ptr(ws), wsb, _ptr(cs), _stream()) == 0
        got_coef = pc.cpu()
        # 0.5 / n_p / (W / w_p) against 0.5 / n_p * w_p / W, both float64: one float32 ulp where the two round apart
        assert bool(((got_coef - want_coef).abs() <= 2.0 ** -23 * want_coef).all()) and bool(((got_coef == 0) == (want_coef == 0)).all())
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
        assert lib.aecf_nce_multi_pp_loss(rows, n, lo, d, M, k, _ptr(Tt), C.MIN_T, _ptr(xl), _ptr(x), _ptr(pl), _ptr(pres_all),
                                          _ptr(col_total), _ptr(ws), wsb, _ptr(lr_s), _stream()) == 0
        lr[:, lo:hi] = lr_s
        dx_s, dxa_s = gd.tensor((rows, M, d), grad_dtype, 0xFF), gd.tensor((n, M, d), grad_dtype, 0xFF)
        d_t = gd.tensor((P,), F32, 0xFF) if with_dt else None
        assert lib.aecf_nce_multi_pp_grads(rows, n, lo, d, M, k, _ptr(Tt), C.MIN_T, _ptr(pc), _ptr(xl), _ptr(x), _ptr(pl), _ptr(ws), wsb,
                                           None, gdt, _ptr(dx_s), _ptr(dxa_s), _ptr(d_t), _stream()) == 0
        torch.cuda.synchronize()
        dx[lo:hi] = dx_s
        out["dx_all"].append(dxa_s)
        if with_dt:
            out["dT"].append(d_t.clone())
    torch.cuda.synchronize()
    gd.check()
    out["loss"] = float((lr.double().sum(1) * out["pair_coef"].double()).sum())
    if with_dt:
        out["dT_sum"] = sum(t.double() for t in out["dT"])
    else:
        del out["dT"]
    return out


@functools.lru_cache(maxsize=None)
def _measured(cid, plan, grad_dtype=F32):
    c = C.make_case(cid)
    return _run_pp(c["x"].to(DEV), _absent(cid, plan), c["shards"], c["anchor"], Q.temperatures(cid), Q.weights(cid), grad_dtype,
                   masked=plan is not None)


@pytest.mark.parametrize("grad_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cid,plan", RUNS)
def test_c_abi_inside_the_derived_bounds(cid, plan, grad_dtype):
    """loss_rows, the shards' column sums, dx_loc, every shard's dx_all, their sum, the value and EVERY dT_p of every shard,
    elementwise; an output whose bound is zero (the pair of weight 0, the clamped temperature, an empty pair, an absent slot) must be
    an exact zero"""
    out = _measured(cid, plan, grad_dtype)
    ref, bnd = _want(cid, plan)
    bf16 = grad_dtype == BF16
    got = {k: v for k, v in out.items() if k != "pair_coef"}
    total = sum(g.double() for g in out["dx_all"])
    if not bf16:
        got["dx_all_sum"] = total
    r = Q.ratios(got, ref, bnd, bf16=bf16)
    if bf16:
        b = bnd["dx_all_sum"] + 2.0 ** -8 * sum(g.double().abs() for g in out["dx_all"])
        err = (total - ref["dx_all_sum"]).abs()
        assert not bool((err[b == 0] != 0).any())
        r["dx_all_sum"] = float((err / b.clamp_min(1e-300)).max())
    print(f"multiview_pairwise_parity case {cid} plan {plan} {'bf16' if bf16 else 'f32'}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items()))
    for name, v in r.items():
        assert v <= 1.0, (cid, plan, name, v)


@pytest.mark.parametrize("cid", ["V2", "V4", "V8"])
def test_every_pair_has_the_bits_of_the_two_view_passes_at_its_own_temperature(cid):
    """col_sums[p] and loss_rows[p] against aecf_nce_sym_pass1_dt / _loss_dt on contiguous copies of the two views at temps[p]"""
    c = C.make_case(cid)
    x = c["x"].to(DEV)
    out = _measured(cid, None)
    for p, (m, n) in enumerate(C.pairs(c["views"], c["anchor"])):
        two = _run_two_view(x[:, m].contiguous(), x[:, n].contiguous(), c["shards"], Q.temperatures(cid)[p], c["coef"], grads=False)
        for k in range(len(c["shards"])):
            assert torch.equal(out["colsum"][k][p], two["colsum"][k]), (cid, p, k)
        assert torch.equal(out["loss_rows"][p], two["loss_rows"]), (cid, p)


@pytest.mark.parametrize("grad_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cid,plan", [("V2", None), ("V3A", None), ("V4", None), ("V2", "K2"), ("V2", "KE")])
def test_equal_temperatures_and_uniform_weights_have_the_bits_of_the_scalar_call(cid, plan, grad_dtype):
    """column sums, loss rows and both gradient tensors bit for bit (weights None and weights all 0.3); the sum of the dT_p, over the
    shards, against the scalar call's dT inside the sum of the two derived bounds -- they are formed by different routes"""
    c = C.make_case(cid)
    x, absent = c["x"].to(DEV), _absent(cid, plan)
    P = Q.n_pairs(cid)
    if plan is None:
        one = _run_multi(x, c["shards"], c["anchor"], 0.07, c["coef"] / P, grad_dtype)
        _, b1 = C.reference(x, c["shards"], c["anchor"], N.used_temperature(0.07), c["coef"] / P, C.score_errors(cid))
    else:
        one = _run_masked(x, absent, c["shards"], c["anchor"], 0.07, grad_dtype)
        _, b1 = K.reference(x, absent, c["shards"], c["anchor"], N.used_temperature(0.07), C.score_errors(cid))
    t = (N.used_temperature(0.07),) * P
    r2, b2 = Q.reference(x, absent, c["shards"], c["anchor"], t, None, C.score_errors(cid))
    for w in (None, (0.3,) * P):
        out = _run_pp(x, absent, c["shards"], c["anchor"], t, w, grad_dtype, masked=plan is not None)
        assert torch.equal(out["loss_rows"], one["loss_rows"]) and torch.equal(out["dx_loc"], one["dx_loc"]), (cid, plan, w)
        for k in range(len(c["shards"])):
            assert torch.equal(out["colsum"][k], one["colsum"][k]) and torch.equal(out["dx_all"][k], one["dx_all"][k]), (cid, plan, w, k)
            assert float(((out["dT"][k].double() - r2["dT"][k]).abs() / b2["dT"][k].clamp_min(1e-300)).max()) <= 1.0
        # a shard's SHARE differs between the routes (the scalar call books the column term of a row with that row, this form
        # with the shard that holds the column's partial sums): the shares of all shards are compared added up
        got, want = float(out["dT_sum"].sum()), sum(one["dT"])
        slack = float(b2["dT_sum"].sum()) + sum(b1["dT"])
        print(f"multiview_pairwise_scalar case {cid} plan {plan}: sum dT_p {got:.6e} scalar dT {want:.6e} slack {slack:.3e}")
        assert abs(got - want) <= slack, (cid, plan, got, want, slack)


def test_a_zero_weight_gives_exact_zeros():
    """V3A, anchor 2: pair 0 = (0, 2) has weight 0 and view 0 no other pair -- dT_0 and the whole gradient of view 0 are exact
    zeros in every shard and both output dtypes, while every other view with a role gets a gradient"""
    c = C.make_case("V3A")
    for grad_dtype in (F32, BF16):
        for plan in (None, "KE"):
            out = _measured("V3A", plan, grad_dtype)
            assert float(out["pair_coef"][0]) == 0.0
            assert not bool(out["dx_loc"][:, 0].any()) and bool(out["dx_loc"][:, 1].any())
            for k in range(len(c["shards"])):
                assert float(out["dT"][k][0]) == 0.0 and float(out["dT"][k][1]) != 0.0
                assert not bool(out["dx_all"][k][:, 0].any()) and bool(out["dx_all"][k][:, 2].any())


@pytest.mark.parametrize("cid,plan", [("V2", "K2"), ("V2", "KE"), ("V4", "K2"), ("V4", "KE")])
def test_masked_form_writes_exact_zeros_outside_the_pairs(cid, plan):
    """the gradient at an absent (row, view) is an exact zero; an empty pair has coefficient 0 and dT_p == 0 and is left out of the
    normalisation of the weights (the live coefficients are those of the definition, asserted in _run_pp)"""
    c = C.make_case(cid)
    absent = Q.make_mask(cid, plan).to(DEV)
    cnt, live = K.pair_counts(Q.make_mask(cid, plan), c["anchor"])
    for grad_dtype in (F32, BF16):
        out = _measured(cid, plan, grad_dtype)
        assert not bool(out["dx_loc"][absent].any())
        for k in range(len(c["shards"])):
            assert not bool(out["dx_all"][k][absent].any())
            for p, n_p in enumerate(cnt):
                if n_p == 0:
                    assert float(out["pair_coef"][p]) == 0.0 and float(out["dT"][k][p]) == 0.0
                    assert not bool(out["loss_rows"][p].any()) and not bool(out["colsum"][k][p].any())
    if plan == "KE":
        assert cnt[-1] == 0 and live == len(cnt) - 1
        w = Q.weights(cid)
        want = [0.5 / n_p * w[p] / sum(w[:-1]) if n_p else 0.0 for p, n_p in enumerate(cnt)]
        assert torch.allclose(out["pair_coef"].double().cpu(), torch.tensor(want, dtype=torch.float64), rtol=2.0 ** -22, atol=0.0)


def test_without_a_temperature_gradient_the_plain_logits_instance_gives_the_same_bits():
    """with_dt = 0 and d_temperatures NULL: the instance without the second sweep; every other output keeps its bits"""
    c = C.make_case("V2")
    for plan in (None, "K2"):
        a = _measured("V2", plan)
        b = _run_pp(c["x"].to(DEV), _absent("V2", plan), c["shards"], c["anchor"], Q.temperatures("V2"), Q.weights("V2"), F32,
                    masked=plan is not None, with_dt=False)
        assert torch.equal(a["loss_rows"], b["loss_rows"]) and torch.equal(a["dx_loc"], b["dx_loc"])
        for k in range(len(c["shards"])):
            assert torch.equal(a["colsum"][k], b["colsum"][k]) and torch.equal(a["dx_all"][k], b["dx_all"][k])


def _definition(x64, t64, w, anchor, absent=None):
    """float64 on raw rows: the normalisation, then Q.definition"""
    z = x64 / x64.norm(dim=-1, keepdim=True).clamp_min(1e-300)
    if absent is None:
        absent = torch.zeros(x64.shape[:2], dtype=torch.bool, device=x64.device)
    else:
        z = torch.where(absent[:, :, None], torch.zeros((), dtype=z.dtype, device=z.device), z)
    return Q.definition(z, absent, anchor, t64, w)


@pytest.mark.parametrize("shape,anchor,masked", [((300, 3, 192), None, False), ((257, 8, 128), None, False), ((300, 4, 192), 2, True)])
def test_python_surface_against_float64_and_the_loop_of_info_nce(shape, anchor, masked):
    """The value and every dT_p inside the bounds of the cases file (taken on the rows the library normalised: neither passes
    through the backward of the normalisation); the gradient on x at most 1.5 times as far from float64 autograd of the
    definition as the loop of info_nce over the pairs, each at its own temperature and weight, which is what a user would write
    without this form (the 1.5: the noise of a maximum over elements, as in tests/test_multiview_gpu.py)."""
    from aecf_amd import losses
    g = torch.Generator().manual_seed(177 + shape[1])
    b, M, d = shape
    base = torch.randn(b, 1, d, generator=g)
    x0 = ((base + 0.75 * torch.randn(b, M, d, generator=g)) * (1.0 + torch.rand(b, M, 1, generator=g))).to(BF16).to(DEV)
    pr = C.pairs(M, anchor)
    P = len(pr)
    temps = [Q.f32(0.03 * (0.4 / 0.03) ** (p / max(P - 1, 1))) for p in range(P)]
    temps[-1] = Q.f32(0.02)                                                     # below min_temperature: clamped, no gradient
    w = [0.0] + [1.0 + 0.5 * p for p in range(1, P)]
    absent = (torch.rand(b, M, generator=g) > 0.8) if masked else None
    kw = dict(anchor=anchor, pair_weights=w)
    if masked:
        kw["key_padding_mask"] = absent.to(DEV)

    x64 = x0.double().requires_grad_(True)
    t64 = torch.tensor(temps, dtype=torch.float64, device=DEV, requires_grad=True)
    _definition(x64, t64, w, anchor, kw.get("key_padding_mask")).backward()

    x = x0.clone().requires_grad_(True)
    T = torch.tensor(temps, device=DEV, requires_grad=True)
    loss = losses.multiview_info_nce(x, temperature=T, **kw)
    loss.backward()
    assert x.grad.dtype == BF16 and x.grad.shape == x.shape and loss.dtype == F32 and T.grad.shape == (P,)
    assert float(T.grad[-1]) == 0.0 and float(T.grad[0]) == 0.0

    with torch.no_grad():
        if masked:
            nx = losses._L2NormMaskedSlots.apply(x0.reshape(b * M, d), absent.to(DEV).view(torch.uint8).reshape(b * M).contiguous(), M, 1e-12)[0]
            nx = nx.reshape(b, M, d)
        else:
            nx = losses.l2_normalize(x0.reshape(b * M, d)).reshape(b, M, d)
    ab = absent if masked else torch.zeros(b, M, dtype=torch.bool)
    s_errs = []
    for m, n in pr:
        u, v = nx[:, m].cpu(), nx[:, n].cpu()
        s_errs.append(float(((u.float() @ v.float().T).double() - u.double() @ v.double().T).abs().max()))
    ref, bnd = Q.reference(nx, ab, [(0, b)], anchor, tuple(temps), tuple(w), tuple(s_errs))
    assert abs(float(loss.detach()) - ref["loss"]) <= bnd["loss"], (float(loss.detach()), ref["loss"], bnd["loss"])
    rt = Q.ratios(dict(dT_sum=T.grad.detach()), ref, bnd)["dT_sum"]
    assert rt <= 1.0, rt

    # the loop a user would write: one info_nce per pair at its own temperature and weight (live pairs of the unmasked forms only)
    err = float((x.grad.double() - x64.grad).abs().max())
    msg = (f"multiview_pairwise_python shape {shape} anchor {anchor} masked {masked}: loss {float(loss.detach()):.6f} dT ratio {rt:.3f} "
           f"max |d T.grad| {float((T.grad.double() - t64.grad).abs().max()):.3e} of {float(t64.grad.abs().max()):.3e} max |d x.grad| {err:.3e}")
    if not masked:
        xl = x0.clone().requires_grad_(True)
        Tl = torch.tensor(temps, device=DEV, requires_grad=True)
        loop = sum(w[p] * losses.info_nce(xl[:, m].contiguous(), xl[:, n].contiguous(), temperature=Tl[p].reshape(1))
                   for p, (m, n) in enumerate(pr)) / sum(w)
        loop.backward()
        err_loop = float((xl.grad.double() - x64.grad).abs().max())
        msg += f" loop {err_loop:.3e} ratio {err / err_loop:.2f}"
        assert err <= 1.5 * err_loop, (err, err_loop)
        assert abs(float(loop.detach()) - float(loss.detach())) <= 1e-4 * abs(float(loss.detach()))
    else:
        # the loop needs a host read per pair here; the masked gradients are judged elementwise through the C ABI above, so this is
        # the plumbing alone: exact zeros in the absent slots, and the whole gradient within 2^-6 of float64's in norm
        assert not bool(x.grad[absent.to(DEV)].any())
        assert float((x.grad.double() - x64.grad).norm()) <= 2.0 ** -6 * float(x64.grad.norm())
    print(msg)


def test_forms_of_the_arguments():
    """a sequence and a tensor of temperatures give the same bits; a scalar temperature with weights is spread over the pairs; all
    weights zero is a zero loss with zero gradients; a device tensor of weights is normalised on the device"""
    from aecf_amd import losses
    g = torch.Generator().manual_seed(31)
    x0 = (torch.randn(130, 1, 128, generator=g) + 0.7 * torch.randn(130, 3, 128, generator=g)).to(BF16).to(DEV)
    temps, w = [0.05, 0.1, 0.3], [2.0, 0.5, 1.0]

    def run(temperature, **kw):
        x = x0.clone().requires_grad_(True)
        loss = losses.multiview_info_nce(x, temperature=temperature, **kw)
        loss.backward()
        return loss.detach(), x.grad

    T = torch.tensor(temps, device=DEV, requires_grad=True)
    a = run(T, pair_weights=w)
    b = run(temps, pair_weights=torch.tensor(w, device=DEV))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and T.grad is not None and bool(torch.isfinite(T.grad).all())
    Ts = torch.tensor(0.07, device=DEV, requires_grad=True)
    c = run(Ts, pair_weights=[1.0, 1.0, 1.0])
    d = run(torch.tensor(0.07, device=DEV))
    assert torch.equal(c[1], d[1]) and abs(float(c[0]) - float(d[0])) <= 2.0 ** -18 * float(d[0]) and Ts.grad.shape == Ts.shape
    Tz = torch.tensor(temps, device=DEV, requires_grad=True)
    z = run(Tz, pair_weights=[0.0, 0.0, 0.0])
    assert float(z[0]) == 0.0 and not bool(z[1].any()) and not bool(Tz.grad.any())
    with pytest.raises(ValueError, match="P = 3"):
        losses.multiview_info_nce(x0, temperature=torch.full((2,), 0.07, device=DEV))


def test_captured_step_follows_temperatures_changed_in_place():
    from aecf_amd import losses
    g = torch.Generator().manual_seed(5)
    x0 = (torch.randn(300, 1, 192, generator=g) + 0.5 * torch.randn(300, 3, 192, generator=g)).to(BF16).to(DEV)
    x = x0.clone().requires_grad_(True)
    T = torch.tensor([0.07, 0.1, 0.2], device=DEV, requires_grad=True)
    W = torch.tensor([1.0, 2.0, 0.5], device=DEV)

    def step():
        return losses.multiview_info_nce(x, temperature=T, pair_weights=W)

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
        T.copy_(torch.tensor([0.05, 0.3, 0.02]))
        W.copy_(torch.tensor([0.5, 0.0, 3.0]))
    graph.replay()
    torch.cuda.synchronize()
    got = (loss.detach().clone(), x.grad.clone(), T.grad.clone())
    x2 = x0.clone().requires_grad_(True)
    T2 = torch.tensor([0.05, 0.3, 0.02], device=DEV, requires_grad=True)
    want = losses.multiview_info_nce(x2, temperature=T2, pair_weights=torch.tensor([0.5, 0.0, 3.0], device=DEV))
    want.backward()
    assert torch.equal(got[0], want.detach())
    assert torch.equal(got[1], x2.grad)
    assert torch.equal(got[2], T2.grad) and float(T2.grad[1]) == 0.0 and float(T2.grad[2]) == 0.0 and float(T2.grad[0]) != 0.0


N2, M2, D2 = 301, 3, 128            # two uneven shards: 151 and 150 rows
TEMPS2, WEIGHTS2 = [0.05, 0.1, 0.3], [1.0, 2.0, 0.5]


def _two_rank_x():
    g = torch.Generator().manual_seed(19)
    return (torch.randn(N2, 1, D2, generator=g) + 0.8 * torch.randn(N2, M2, D2, generator=g)).to(BF16)


def _pairwise_worker(rank, world, port, backend, q):
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
        x = _two_rank_x()[lo:hi].to(dev).requires_grad_(True)
        T = torch.tensor(TEMPS2, device=dev, requires_grad=True)
        loss = losses.multiview_info_nce(x, temperature=T, pair_weights=WEIGHTS2)
        loss.backward()
        torch.cuda.synchronize()
        # gradients follow the data-parallel convention (averaged over ranks later): undo the factor `world`
        q.put((rank, lo, hi, float(loss.detach()), (x.grad.float() / world).cpu().numpy(), (T.grad / world).cpu().numpy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_equal_one_rank():
    """The data-parallel path of the Python function in the style and with the tolerances of tests/test_multiview_gpu.py: the loss
    on every rank is the global one, the gradient of a rank's rows and the ranks' shares of every dL/dT_p added up are those of the
    one-rank full batch -- the column term of dT_p uses the all-reduced column sums, so no further exchange is needed."""
    from aecf_amd import losses
    world = 2
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_pairwise_worker, args=(r, world, port, backend, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    x = _two_rank_x().to(DEV).requires_grad_(True)
    T = torch.tensor(TEMPS2, device=DEV, requires_grad=True)
    want = losses.multiview_info_nce(x, temperature=T, pair_weights=WEIGHTS2)
    want.backward()
    for rank, lo, hi, loss, gx, gt in res:
        assert abs(loss - float(want.detach())) < 2e-3 * abs(float(want.detach()))
        rx = x.grad[lo:hi].float().cpu()
        assert (torch.from_numpy(gx) - rx).abs().max() / rx.abs().max() < 2e-2
    gt = torch.from_numpy(res[0][5]) + torch.from_numpy(res[1][5])
    assert bool(((gt - T.grad.cpu()).abs() < 2e-3 * T.grad.cpu().abs()).all()), (gt, T.grad)
