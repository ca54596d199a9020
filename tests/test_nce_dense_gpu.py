"""The materialising InfoNCE (nce_generic_fwd_bwd behind aecf_nce_fwd_bwd / aecf_nce_fwd_bwd_dt: float32 rows, and bf16 rows of
no streaming width below T = 0.025) and l2_normalize against float64 at their edges, through the C ABI with ctypes and through
losses.info_nce.  Cases, inputs, the float64 references and the derived elementwise bounds are those of
tests/nce_dense_cases.py (tests/test_nce_dense_cpu.py shows that the bounds hold an emulation of the arithmetic and catch a lost
or doubled key, a misplaced positive, an ignored offset, a dropped row or column sweep, an unscaled G and a wrong dT).

Every output and the workspace come from the Guarded helper of tests/test_abi_guards_gpu.py: the workspace is exactly as long as
the materialising form carves (nce_dense_cases.workspace_bytes_py) and filled with 0xFF (NaN as bf16 and as float32) before the
call, the outputs are filled alike -- a finite output was written and read nothing that was not written first (the tdot slots
parked in the kT region, which transpose_rect then overwrites)."""
import functools
import math

import pytest
import torch

from tests import nce_dense_cases as C
from tests.helpers import record_errors
from tests.test_abi_guards_gpu import Guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
CASE_PARAMS = [(cid, T) for cid in C.CASES for T in C.temps_of(cid)]
NAN_WORDS = 0x7FC07FC0                  # another poison: quiet NaNs as bf16 pairs and as float32
ABI_MIN_T = 1e-3                        # under every temperature of the table (and under the tile form's 0.025)
OK, BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = 0, -1, -2, -3, -4


def _libs():
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


def _code(dtype):
    _lib = _libs()[0]
    return {BF16: _lib.AECF_BF16, F32: _lib.AECF_F32, torch.float16: _lib.AECF_F16}[dtype]


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = C.make_case(cid)
    return c["q"].to(DEV), c["k"].to(DEV)


@functools.lru_cache(maxsize=None)
def _want(cid, T, min_t=None, shard=None):
    """(float64 reference, bounds) of a case or of its row shard [lo, hi) at T as the kernels read it, computed once on the
    device; the score error inside the bf16 bounds comes from torch's CPU products of the whole case"""
    c = C.make_case(cid)
    q, k = _inputs(cid)
    lo, hi = shard or (0, q.shape[0])
    mt = None if min_t is None else C.used_temperature(min_t)
    ref = C.reference(q[lo:hi], k, c["off"] + lo, C.used_temperature(T), c["coef"], mt)
    return ref, C.bounds(ref, q[lo:hi], k, c["off"] + lo, c["coef"], C.score_error(cid))


def _call(q, k, off, T, coef, entry, min_t=ABI_MIN_T, poison=0xFF, short=0, dtype=None, null_t=False):
    """One call of aecf_nce_fwd_bwd (entry "host": T a float argument), aecf_nce_fwd_bwd_dt ("dt": T on the device, dT wanted) or
    the latter with d_temperature == NULL ("dt_null") on guarded, poisoned buffers; the workspace is the materialising form's own
    size minus ``short`` bytes.  Returns (status, outputs, workspace); the guards are checked."""
    _lib, lib, _ptr, _stream = _libs()
    dtype = dtype or q.dtype
    rows, (cols, d) = q.shape[0], k.shape
    q, k = q.contiguous(), k.contiguous()
    gd = Guarded(DEV)
    wsb = C.workspace_bytes_py(q.shape[0], cols, d, q.dtype) - short
    ws = gd.new(wsb, 0xFF)
    if poison != 0xFF:
        ws[:wsb // 4 * 4].view(torch.int32).fill_(poison)
    out = dict(loss_rows=gd.tensor((q.shape[0],), F32, 0xFF), dq=gd.tensor((q.shape[0], d), F32, 0xFF), dk=gd.tensor((cols, d), F32, 0xFF))
    if entry == "host":
        status = lib.aecf_nce_fwd_bwd(rows, cols, off, d, _code(dtype), T, coef, _ptr(q), _ptr(k), _ptr(out["loss_rows"]), _ptr(out["dq"]),
                                      _ptr(out["dk"]), _ptr(ws), wsb, _stream())
    else:
        Tt = None if null_t else torch.tensor([T], dtype=F32, device=DEV)
        if entry == "dt":
            out["dT"] = gd.tensor((1,), F32, 0xFF)
        status = lib.aecf_nce_fwd_bwd_dt(rows, cols, off, d, _code(dtype), _ptr(Tt), min_t, coef, _ptr(q), _ptr(k), _ptr(out["loss_rows"]),
                                         _ptr(out["dq"]), _ptr(out["dk"]), _ptr(out.get("dT")), _ptr(ws), wsb, _stream())
    torch.cuda.synchronize()
    gd.check()
    return status, out, ws


def _run_case(cid, T, entry="dt", shard=None, **kw):
    c = C.make_case(cid)
    q, k = _inputs(cid)
    lo, hi = shard or (0, q.shape[0])
    _lib, lib, _, _ = _libs()
    rows, (cols, d) = hi - lo, k.shape
    public = lib.aecf_nce_workspace_bytes(rows, cols, d, _code(q.dtype))
    mine = C.workspace_bytes_py(rows, cols, d, q.dtype)
    assert public == mine if q.dtype == F32 else public >= mine
    status, out, _ = _call(q[lo:hi], k, c["off"] + lo, T, c["coef"], entry, **kw)
    assert status == OK, (cid, T, entry, status)
    return out


@functools.lru_cache(maxsize=None)
def _measured(cid, T):
    return _run_case(cid, T)


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """the shared inputs, references and outputs live on the device for this module only: drop them and the blocks they leave
    in torch's caching allocator afterwards (tests that measure a peak of allocated bytes are served from that cache)"""
    yield
    for cached in (_inputs, _want, _measured):
        cached.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _same_bits(one, two, what, names=("loss_rows", "dq", "dk", "dT")):
    for name in names:
        assert bool(torch.isfinite(one[name]).all()), (what, name)
        assert torch.equal(one[name], two[name]), (what, name)


def _judge(label, name, got, ref, bnd, **tags):
    """print the line of the profile, record it, assert every output finite and every ratio <= 1"""
    got = dict(got)
    for n in ("loss_rows", "dq", "dk"):
        assert bool(torch.isfinite(got[n].double()).all()), (label, n)
    if "dT" in got:
        got["dT"] = float(got["dT"])
        assert math.isfinite(got["dT"]), label
    r = C.ratios(got, ref, bnd)
    vb = C.value_over_bound(ref, bnd)
    print(f"nce_dense_parity {label}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items())
          + " | value/bound " + " ".join(f"{n}={vb[n]:.3g}" for n in r))
    record_errors(name, **tags, **r, **{f"value_{n}": vb[n] for n in r})
    for n, v in r.items():
        assert v <= 1.0, (label, n, v)
    return r


@pytest.mark.parametrize("cid,T", CASE_PARAMS)
def test_case_inside_the_derived_bounds(cid, T):
    """loss rows, dq, dk and dT of aecf_nce_fwd_bwd_dt, element by element; then aecf_nce_fwd_bwd at the same float T: inside the
    same bounds and, as include/aecf_hip.h promises, the same bits -- as is the _dt entry without a d_temperature"""
    ref, bnd = _want(cid, T)
    dt = _measured(cid, T)
    r = _judge(f"case {cid} T {T}", f"nce_dense_parity_{cid}", dt, ref, bnd, T=T)
    assert set(r) == set(C.OUTPUTS)
    host = _run_case(cid, T, entry="host")
    _judge(f"case {cid} T {T} (host T)", f"nce_dense_host_{cid}", host, ref, bnd, T=T)
    _same_bits(dt, host, (cid, T, "host T"), names=("loss_rows", "dq", "dk"))
    _same_bits(dt, _run_case(cid, T, entry="dt_null"), (cid, T, "no d_temperature"), names=("loss_rows", "dq", "dk"))


@pytest.mark.parametrize("cid", ["M3", "M4", "B2", "M6"])
def test_another_poison_gives_the_same_bits(cid):
    """The same call on a workspace filled with other NaNs: nothing is read before it is written (the tdot slots in the kT
    region, the padding of each region) and the reductions run in a fixed order, so the bits cannot move -- dT included."""
    T = C.temps_of(cid)[0]
    _same_bits(_measured(cid, T), _run_case(cid, T, poison=NAN_WORDS), (cid, "poison"))


def test_clamped_temperature():
    """M3 with a device T of 0.005 under min_temperature 0.01: the bits of the T = 0.01 run, dT exactly zero, inside the bounds of
    the clamped reference"""
    at = _run_case("M3", 0.01, min_t=0.01)
    low = _run_case("M3", 0.005, min_t=0.01)
    _same_bits(low, at, "clamp", names=("loss_rows", "dq", "dk"))
    assert float(low["dT"]) == 0.0 and float(at["dT"]) != 0.0
    _same_bits(at, _measured("M3", 0.01), "min_temperature == T")
    ref, bnd = _want("M3", 0.005, 0.01)
    assert ref["dT"] == 0.0
    _judge("case M3 T 0.005 min_temperature 0.01", "nce_dense_clamp_M3", low, ref, bnd, T=0.005)


@pytest.mark.parametrize("cid,cut", [("M4", 37), ("B2", 129)])
def test_emulated_ranks(cid, cut):
    """Two row shards [0, cut) and [cut, rows), each run as a rank would with row_offset = the case's offset + lo: every piece
    against the shard's own bounds; the concatenated loss rows and dq and the added dk and dT against the float64 of the WHOLE
    problem with the shards' bounds concatenated / added."""
    T = C.temps_of(cid)[0]
    rows = C.CASES[cid][1][0]
    whole, _ = _want(cid, T)
    pieces, bounds = [], []
    for lo, hi in ((0, cut), (cut, rows)):
        got = _run_case(cid, T, shard=(lo, hi))
        ref, bnd = _want(cid, T, shard=(lo, hi))
        _judge(f"case {cid} T {T} rows [{lo}, {hi})", f"nce_dense_shard_{cid}", got, ref, bnd, T=T, lo=lo, hi=hi)
        pieces.append(got)
        bounds.append(bnd)
    total = dict(loss_rows=torch.cat([p["loss_rows"] for p in pieces]), dq=torch.cat([p["dq"] for p in pieces]),
                 dk=sum(p["dk"].double() for p in pieces), dT=sum(float(p["dT"]) for p in pieces))
    bsum = dict(loss_rows=torch.cat([b["loss_rows"] for b in bounds]), dq=torch.cat([b["dq"] for b in bounds]),
                dk=sum(b["dk"] for b in bounds), dT=sum(b["dT"] for b in bounds))
    _judge(f"case {cid} T {T} shards at {cut} put together", f"nce_dense_shards_{cid}", total, whole, bsum, T=T, cut=cut)


REFUSALS = [
    # what, dtype of the buffers, dtype code passed, (rows, cols, off, d), keyword arguments of _call, status
    ("cols % 64 != 0 (float32)", F32, F32, (10, 100, 0, 64), {}, UNSUPPORTED),
    ("d % 64 != 0 (float32)", F32, F32, (10, 64, 0, 96), {}, UNSUPPORTED),
    ("d % 64 != 0 (bf16)", BF16, BF16, (10, 64, 0, 96), {}, UNSUPPORTED),
    ("float16", torch.float16, torch.float16, (10, 64, 0, 64), {}, UNSUPPORTED),
    ("row_offset + rows > cols", F32, F32, (10, 64, 55, 64), {}, BAD_DIMS),
    ("row_offset < 0", F32, F32, (10, 64, -1, 64), {}, BAD_DIMS),
    ("workspace one byte short (float32)", F32, F32, (10, 64, 0, 64), dict(short=1), WORKSPACE),
    ("workspace one byte short (bf16)", BF16, BF16, (10, 64, 0, 192), dict(short=1), WORKSPACE),
]


@pytest.mark.parametrize("what,bdt,dtype,shape,kw,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(what, bdt, dtype, shape, kw, status):
    """both entries answer the status before anything is written: every output and the workspace still hold their poison"""
    rows, cols, off, d = shape
    g = torch.Generator().manual_seed(8300)
    q = C._unit(torch.randn(rows, d, generator=g)).to(bdt).to(DEV)
    k = C._unit(torch.randn(cols, d, generator=g)).to(bdt).to(DEV)
    T = 0.02 if bdt == BF16 else 0.07
    for entry in ("host", "dt", "dt_null"):
        got, out, ws = _call(q, k, off, T, 0.5 / cols, entry, dtype=dtype, **kw)
        assert got == status, (what, entry, got)
        for name, x in list(out.items()) + [("workspace", ws)]:
            assert bool((x.view(torch.uint8) == 0xFF).all()), (what, entry, name)


def test_null_temperature_is_refused():
    q, k = _inputs("M1")
    got, out, ws = _call(q, k, 63, 0.07, 0.5 / 64, "dt", null_t=True)
    assert got == NULL_POINTER
    for name, x in list(out.items()) + [("workspace", ws)]:
        assert bool((x.view(torch.uint8) == 0xFF).all()), name


# ---- l2_normalize through the C ABI ----
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n,d", C.L2_SHAPES)
def test_l2norm_inside_the_derived_bounds(n, d, dtype):
    """aecf_l2norm_forward and aecf_l2norm_backward on guarded, poisoned buffers: zn, inv_norm and dz elementwise against
    float64 -- the backward at the stored zn and inv_norm -- with an all-zero row, a row under eps, a row of norm 1e15 and a row
    with one dominant element"""
    _lib, lib, _ptr, _stream = _libs()
    eps = C.used_temperature(C.L2_EPS)
    worst = dict(zn=0.0, inv_norm=0.0, dz=0.0)
    for z, kinds in C.l2_inputs(n, d, dtype):
        z = z.to(DEV)
        gd = Guarded(DEV)
        zn, inv, dz = gd.tensor((n, d), dtype, 0xFF), gd.tensor((n,), F32, 0xFF), gd.tensor((n, d), dtype, 0xFF)
        assert lib.aecf_l2norm_forward(n, d, _code(dtype), C.L2_EPS, _ptr(z), _ptr(zn), _ptr(inv), _stream()) == OK
        g = torch.Generator().manual_seed(n + d)
        dzn = torch.randn(n, d, generator=g).to(DEV)
        assert lib.aecf_l2norm_backward(n, d, _code(dtype), _ptr(zn), _ptr(inv), _ptr(dzn), _ptr(dz), _stream()) == OK
        torch.cuda.synchronize()
        gd.check()
        for x in (zn, inv, dz):
            assert bool(torch.isfinite(x.float()).all()), (n, d, kinds)
        ref, bnd, _ = C.l2_forward_reference(z, eps)
        want, b_dz = C.l2_backward_reference(zn, inv, dzn)
        worst["zn"] = max(worst["zn"], C.l2_ratio(zn, ref["zn"], bnd["zn"]))
        worst["inv_norm"] = max(worst["inv_norm"], C.l2_ratio(inv, ref["inv_norm"], bnd["inv_norm"]))
        worst["dz"] = max(worst["dz"], C.l2_ratio(dz, want, b_dz))
        for r, kind in kinds.items():
            if kind == "zero":
                assert float(zn[r].float().abs().max()) == 0.0
            if kind in ("zero", "tiny"):
                assert abs(float(inv[r]) * eps - 1.0) <= 4.0 * C.H          # inv_norm = 1 / eps
    name = "bf16" if dtype == BF16 else "f32"
    print(f"nce_dense_parity l2norm {name} {n} x {d}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    record_errors("nce_dense_l2norm", n=n, d=d, bf16=dtype == BF16, **worst)
    for k, v in worst.items():
        assert v <= 1.0, (n, d, name, k, v)


# ---- the Python surface ----
def _views(n, d, seed, twins=0):
    """two views whose rows pair up at a cosine near 0.8; ``twins``: that many rows of zb, spread over the rows, are copies of
    the row before them -- the row before then holds half of its softmax at any T, and the copy's own row has lost its positive,
    so the loss and every gradient carry weight at a low T too"""
    g = torch.Generator().manual_seed(seed)
    za = 3.0 * torch.randn(n, d, generator=g)
    zb = 2.0 * (0.8 * za / 3.0 + 0.6 * torch.randn(n, d, generator=g))
    for t in range(twins):
        r = 1 + t * (n - 1) // twins
        zb[r] = zb[r - 1]
    return za, zb


def _surface_loss_bound(refs, bnds, coef, n):
    """loss = float(coef) sum(rows of a|b) + float(coef) sum(rows of b|a): the kernels' rows within their bounds, two float32 sums
    of n rows (any order: g(n) of the magnitudes), float(coef) and the products (2 h), the last addition (h)"""
    mags = sum(float((r["loss_rows"].abs() + b["loss_rows"]).sum()) for r, b in zip(refs, bnds))
    return coef * (sum(float(b["loss_rows"].sum()) for b in bnds) + (C.gamma(n) + 3.0 * C.H) * mags)


def test_python_surface_float32():
    """losses.info_nce on float32 rows (n = 192, d = 64, T = 0.07; a float and a tensor temperature) against the float64 of the
    whole chain -- normalise, both directions, the gradient through the normalisation (oracle.aecf_oracle.info_nce and
    info_nce_backward; dT from the references of tests/nce_dense_cases.py).  The tolerances are the derived bounds carried through:
    the rows the directions see are within e_in = r_inv + h of the reference's (l2_normalize's forward bound), so each direction's
    bounds are taken with that e_in; the gradient on a view's unit rows is dq of one direction plus dk of the other (their bounds
    added, one float32 addition); the normalisation's backward carries that through (nce_dense_cases.l2_backward_chain)."""
    from aecf_amd import losses
    from oracle import aecf_oracle as O
    n, d, T = 192, 64, 0.07
    za, zb = _views(n, d, 8400)
    t, coef = C.used_temperature(T), 0.5 / n
    eps = C.used_temperature(C.L2_EPS)
    za64, zb64 = za.double().to(DEV), zb.double().to(DEV)
    fa, _, r_inv = C.l2_forward_reference(za64, eps)
    fb, _, _ = C.l2_forward_reference(zb64, eps)
    e_in = r_inv + C.H
    na, nb = fa["zn"], fb["zn"]
    refs = [C.reference(na, nb, 0, t, coef), C.reference(nb, na, 0, t, coef)]
    bnds = [C.bounds(refs[0], na, nb, 0, coef, e_in=e_in), C.bounds(refs[1], nb, na, 0, coef, e_in=e_in)]
    want_loss = coef * float(refs[0]["loss_rows"].sum() + refs[1]["loss_rows"].sum())
    b_loss = _surface_loss_bound(refs, bnds, coef, n)
    g_a, g_b = refs[0]["dq"] + refs[1]["dk"], refs[0]["dk"] + refs[1]["dq"]
    bg_a = bnds[0]["dq"] + bnds[1]["dk"]
    bg_b = bnds[0]["dk"] + bnds[1]["dq"]
    bg_a, bg_b = bg_a + C.H * (g_a.abs() + bg_a), bg_b + C.H * (g_b.abs() + bg_b)
    dza, b_dza = C.l2_backward_chain(na, fa["inv_norm"], g_a, bg_a, e_in, r_inv)
    dzb, b_dzb = C.l2_backward_chain(nb, fb["inv_norm"], g_b, bg_b, e_in, r_inv)
    want_dt = refs[0]["dT"] + refs[1]["dT"]
    b_dt = bnds[0]["dT"] + bnds[1]["dT"]
    b_dt += C.H * (abs(want_dt) + b_dt)
    # the oracle's chain is the one above
    o_loss = float(O.info_nce(za64.cpu(), zb64.cpu(), t))
    o_dza, o_dzb = O.info_nce_backward(za64.cpu(), zb64.cpu(), t)
    assert abs(o_loss - want_loss) <= 1e-12 * abs(want_loss)
    assert float((o_dza.to(DEV) - dza).abs().max()) <= 1e-12 * float(dza.abs().max())
    assert float((o_dzb.to(DEV) - dzb).abs().max()) <= 1e-12 * float(dzb.abs().max())
    for form in ("float", "tensor"):
        x, y = za.to(DEV).requires_grad_(True), zb.to(DEV).requires_grad_(True)
        Tt = torch.tensor(T, device=DEV, requires_grad=True) if form == "tensor" else T
        loss = losses.info_nce(x, y, temperature=Tt)
        loss.backward()
        assert loss.dtype == F32 and x.grad.dtype == F32
        r = dict(loss=abs(float(loss.detach()) - o_loss) / b_loss, dza=C.l2_ratio(x.grad, o_dza.to(DEV), b_dza),
                 dzb=C.l2_ratio(y.grad, o_dzb.to(DEV), b_dzb))
        vb = dict(loss=abs(o_loss) / b_loss, dza=float((dza.abs() / b_dza).max()), dzb=float((dzb.abs() / b_dzb).max()))
        if form == "tensor":
            r["dT"], vb["dT"] = abs(float(Tt.grad) - want_dt) / b_dt, abs(want_dt) / b_dt
        print(f"nce_dense_parity info_nce float32 {n} x {n} d {d} T {T} ({form} T): " + " ".join(f"{k}={v:.3f}" for k, v in r.items())
              + " | value/bound " + " ".join(f"{k}={vb[k]:.3g}" for k in r))
        record_errors("nce_dense_python_f32", T=T, tensor=form == "tensor", **r)
        for k, v in r.items():
            assert v <= 1.0, (form, k, v)


def test_python_surface_bf16():
    """losses.info_nce on bf16 rows of no streaming width below the tile form's temperature (n = 192, d = 192, T = 0.02): neither
    the symmetric tile form nor the streaming form takes it.  The loss and the gradient on the unit rows against the float64 of
    both directions AT the library's own bf16 unit rows (the bf16 bounds; each direction's gradient rounded to bf16 once, their
    sum once more), the gradient on the inputs against the float64 backward of the normalisation at the stored rows and the
    gradient handed to it (inv_norm within r_inv of the float64 one)."""
    from aecf_amd import losses
    n, d, T = 192, 192, 0.02
    za, zb = _views(n, d, 8500, twins=8)
    za, zb = za.to(BF16).to(DEV), zb.to(BF16).to(DEV)
    assert not losses._sym_supported(za, T, n) and not losses._stream_form(za, n)
    t, coef = C.used_temperature(T), 0.5 / n
    eps = C.used_temperature(C.L2_EPS)
    x, y = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    na, nb = losses.l2_normalize(x), losses.l2_normalize(y)
    na.retain_grad()
    nb.retain_grad()
    with torch.no_grad():
        for z, zn in ((za, na), (zb, nb)):
            ref, bnd, _ = C.l2_forward_reference(z, eps)
            assert C.l2_ratio(zn, ref["zn"], bnd["zn"]) <= 1.0
    loss = losses.info_nce(za, zb, temperature=T)           # the same rows: l2_normalize is deterministic
    low = losses._stream_form(na, n)
    share = losses._NceDirection.apply(na, nb, 0, T, coef, low) + losses._NceDirection.apply(nb, na, 0, T, coef, low)
    assert torch.equal(loss, share.detach())
    share.backward()
    nad, nbd = na.detach(), nb.detach()
    s_err = max(C.score_error_of(nad, nbd), C.score_error_of(nbd, nad))
    refs = [C.reference(nad, nbd, 0, t, coef), C.reference(nbd, nad, 0, t, coef)]
    bnds = [C.bounds(refs[0], nad, nbd, 0, coef, s_err), C.bounds(refs[1], nbd, nad, 0, coef, s_err)]
    want_loss = coef * float(refs[0]["loss_rows"].sum() + refs[1]["loss_rows"].sum())
    b_loss = _surface_loss_bound(refs, bnds, coef, n)
    r, vb = dict(loss=abs(float(loss) - want_loss) / b_loss), dict(loss=abs(want_loss) / b_loss)
    r_inv = C.l2_forward_reference(za, eps)[2]
    for name, zin, zn, k0, k1 in (("a", x, na, 0, 1), ("b", y, nb, 1, 0)):
        one, two = refs[k0]["dq"], refs[k1]["dk"]
        b1 = bnds[k0]["dq"] + C.EPS_P * (one.abs() + bnds[k0]["dq"])
        b2 = bnds[k1]["dk"] + C.EPS_P * (two.abs() + bnds[k1]["dk"])
        g = one + two
        bg = b1 + b2
        bg = bg + C.EPS_P * (g.abs() + bg)
        assert zn.grad.dtype == BF16
        r[f"dn{name}"], vb[f"dn{name}"] = C.l2_ratio(zn.grad, g, bg), float((g.abs() / bg).max())
        inv64 = 1.0 / zin.detach().double().norm(dim=1).clamp_min(eps)
        dz, b_dz = C.l2_backward_chain(zn.detach().double(), inv64, zn.grad.double(), torch.zeros_like(g), 0.0, r_inv, out_bf16=True)
        r[f"dz{name}"], vb[f"dz{name}"] = C.l2_ratio(zin.grad, dz, b_dz), float((dz.abs() / b_dz).max())
    print(f"nce_dense_parity info_nce bf16 {n} x {n} d {d} T {T}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items())
          + " | value/bound " + " ".join(f"{k}={vb[k]:.3g}" for k in r))
    record_errors("nce_dense_python_bf16", T=T, **r)
    for k, v in r.items():
        assert v <= 1.0, (k, v)


def test_python_surface_refuses_float32_rows_off_the_64_grid():
    from aecf_amd import losses
    za, zb = _views(100, 64, 8600)
    with pytest.raises(RuntimeError, match="aecf_nce_fwd_bwd"):
        losses.info_nce(za.to(DEV), zb.to(DEV), temperature=0.07)
