"""The streaming InfoNCE (aecf_nce_flash.hip on aecf_flash_stream.h) against float64 at its split, tile and low-temperature
edges, through the C ABI with ctypes.  Cases, inputs, the float64 reference and the derived elementwise bounds are those of
tests/nce_stream_cases.py (tests/test_nce_stream_cpu.py shows that the bounds catch one lost or doubled key).

Pinning the form.  aecf_nce_fwd_bwd_dt is called with min_temperature = 1e-3: the tile form refuses any bound below 0.025
whatever workspace it is handed, so the streaming kernels run -- at T = 0.07 as at T = 0.005 (T is a device scalar).  The float
entry aecf_nce_fwd_bwd is used at T = 0.02 only: at T = 0.07 it takes the tile form whenever the workspace is at least that
form's size, and at small shapes the streaming workspace exceeds it ((64, 700, d = 1024): two splits of 64 x 1026 floats
against a 256 x 768 bf16 block), so such a call would not prove which kernel ran.

Every output and the workspace come from the Guarded helper of tests/test_abi_guards_gpu.py: the workspace is exactly
aecf_nce_stream_workspace_bytes long and, like the payloads, prefilled with 0xFF (NaN patterns): an output that is finite was
written, and a slot of case H's empty split that entered the combine would show."""
import functools
import math

import pytest
import torch

from tests import nce_stream_cases as C
from tests.helpers import record_errors
from tests.test_abi_guards_gpu import Guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MIN_T = 1e-3
ERR_WORKSPACE = -4
F32 = torch.float32
OUTPUTS = ("loss_rows", "dq", "dk", "dT")
CASE_T = [(cid, T) for cid in C.CASES for T in (0.07, 0.005)]


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = C.make_case(cid)
    return c["q"].to(DEV), c["k"].to(DEV), c["off"]


@functools.lru_cache(maxsize=None)
def _want(cid, T):
    """(T as the kernels read it, coef, float64 reference, bounds) of a case, computed once on the device in float64; the
    score error inside eps_x comes from torch's CPU products"""
    q, k, off = _inputs(cid)
    cols = k.shape[0]
    t, coef = C.used_temperature(T), 1.0 / cols
    ref = C.reference(q, k, off, t, coef)
    bnd = C.bounds(ref, q, k, off, t, coef, C.eps_x(C.score_error(cid), t, cols))
    del ref["S"]
    return t, coef, ref, bnd


def _buffers(gd, rows, cols, d, fill=0xFF):
    return dict(loss_rows=gd.tensor((rows,), F32, fill), dq=gd.tensor((rows, d), F32, fill), dk=gd.tensor((cols, d), F32, fill),
                dT=gd.tensor((1,), F32, fill))


def _call_dt(q, k, off, T, coef, out, ws, wsb, ent=None):
    """aecf_nce_fwd_bwd_dt, or with ``ent`` = (n, last_seq_len, target, entropy, upstream, entropy_loss, d_entropy)
    aecf_loss_fwd_bwd_dt; T: a device scalar.  Returns the status."""
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    lib = _lib.load()
    rows, d = q.shape
    cols = k.shape[0]
    if ent is None:
        return lib.aecf_nce_fwd_bwd_dt(rows, cols, off, d, _lib.AECF_BF16, _ptr(T), MIN_T, coef, _ptr(q), _ptr(k), _ptr(out["loss_rows"]),
                                       _ptr(out["dq"]), _ptr(out["dk"]), _ptr(out["dT"]), _ptr(ws), wsb, _stream())
    n, last, target, h, upstream, e_loss, d_ent = ent
    return lib.aecf_loss_fwd_bwd_dt(rows, cols, off, d, _ptr(T), MIN_T, coef, _ptr(q), _ptr(k), _ptr(out["loss_rows"]), _ptr(out["dq"]),
                                    _ptr(out["dk"]), _ptr(out["dT"]), n, last, target, _ptr(h), upstream, _ptr(e_loss), _ptr(d_ent),
                                    _ptr(ws), wsb, _stream())


def _stream_bytes(rows, cols, d):
    from aecf_amd import _lib
    wsb = _lib.load().aecf_nce_stream_workspace_bytes(rows, cols, d, _lib.AECF_BF16)
    assert wsb == C.workspace_bytes_py(rows, cols, d)
    return wsb


@functools.lru_cache(maxsize=None)
def _measured(cid, T):
    """One case at one temperature: the call on a 0xFF-filled workspace of exactly the documented size, the same call on a
    zero-filled one, and a call with the size one byte short -- run once, judged by the tests below."""
    q, k, off = _inputs(cid)
    (rows, d), cols = q.shape, k.shape[0]
    coef = 1.0 / cols
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    wsb = _stream_bytes(rows, cols, d)
    gd = Guarded(DEV)
    out = _buffers(gd, rows, cols, d)
    ws = gd.new(wsb, 0xFF)
    status = _call_dt(q, k, off, Tt, coef, out, ws, wsb)
    torch.cuda.synchronize()
    gd2 = Guarded(DEV)
    again = _buffers(gd2, rows, cols, d)
    ws2 = gd2.new(wsb, 0)
    status2 = _call_dt(q, k, off, Tt, coef, again, ws2, wsb)
    torch.cuda.synchronize()
    gd3 = Guarded(DEV)
    short = _buffers(gd3, rows, cols, d)
    ws3 = gd3.new(wsb, 0xFF)
    status3 = _call_dt(q, k, off, Tt, coef, short, ws3, wsb - 1)
    torch.cuda.synchronize()
    return dict(out=out, again=again, short=short, guards=(gd, gd2, gd3), status=(status, status2, status3), ws3=ws3)


def _ratios(out, ref, bnd):
    return C.ratios(dict(loss_rows=out["loss_rows"], dq=out["dq"], dk=out["dk"], dT=float(out["dT"])), ref, bnd)


@pytest.mark.parametrize("cid,T", CASE_T)
def test_outputs_inside_the_derived_bounds(cid, T):
    """loss_rows, dq, dk and d_temperature of every case, elementwise, at T = 0.07 and at T = 0.005 (logits up to +-200: the
    online maximum and its rescale carry the result)."""
    m = _measured(cid, T)
    assert m["status"][0] == 0
    _, _, ref, bnd = _want(cid, T)
    r = _ratios(m["out"], ref, bnd)
    sig = C.signal(ref, bnd)
    print(f"nce_stream_parity case {cid} T {T}: " + " ".join(f"{n}={r[n]:.3f}" for n in OUTPUTS)
          + " | value/bound " + " ".join(f"{n}={sig[n]:.3g}" for n in OUTPUTS))
    record_errors(f"nce_stream_parity_{cid}", T=T, **r)
    for n in OUTPUTS:
        assert r[n] <= 1.0, (cid, T, n, r[n])


@pytest.mark.parametrize("cid,T", CASE_T)
def test_guards_intact_and_every_output_written(cid, T):
    """No byte outside the buffers changed, and no output kept its NaN fill or picked one up from the workspace (case H: the
    combine read no slot of the empty split)."""
    m = _measured(cid, T)
    m["guards"][0].check()
    for n in OUTPUTS:
        assert bool(torch.isfinite(m["out"][n]).all()), (cid, T, n)


@pytest.mark.parametrize("cid,T", CASE_T)
def test_workspace_contents_do_not_matter(cid, T):
    """The same call on a zero-filled workspace: bit-identical outputs (fixed-order sums, nothing read before it is written)."""
    m = _measured(cid, T)
    assert m["status"][1] == 0
    m["guards"][1].check()
    for n in OUTPUTS:
        assert torch.equal(m["out"][n], m["again"][n]), (cid, T, n)


@pytest.mark.parametrize("cid,T", CASE_T)
def test_workspace_one_byte_short_is_refused(cid, T):
    m = _measured(cid, T)
    assert m["status"][2] == ERR_WORKSPACE
    m["guards"][2].check()
    for n in OUTPUTS:
        assert bool((m["short"][n].view(torch.uint8) == 0xFF).all()), (cid, T, n)
    assert bool((m["ws3"] == 0xFF).all())


@pytest.mark.parametrize("cid", ["C", "F"])
def test_float_entry_below_the_tile_forms_temperature(cid):
    """aecf_nce_fwd_bwd at T = 0.02, where the tile form refuses the temperature: the streaming kernels with a host float T."""
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    T = 0.02
    q, k, off = _inputs(cid)
    (rows, d), cols = q.shape, k.shape[0]
    t, coef, ref, bnd = _want(cid, T)
    wsb = _stream_bytes(rows, cols, d)
    gd = Guarded(DEV)
    out = _buffers(gd, rows, cols, d)
    ws = gd.new(wsb, 0xFF)
    _lib.check(_lib.load().aecf_nce_fwd_bwd(rows, cols, off, d, _lib.AECF_BF16, T, coef, _ptr(q), _ptr(k), _ptr(out["loss_rows"]),
                                            _ptr(out["dq"]), _ptr(out["dk"]), _ptr(ws), wsb, _stream()), "aecf_nce_fwd_bwd")
    torch.cuda.synchronize()
    gd.check()
    assert bool((out["dT"].view(torch.uint8) == 0xFF).all())          # (not an argument of this entry)
    r = C.ratios(dict(out, dT=ref["dT"]), ref, bnd)
    del r["dT"]
    print(f"nce_stream_parity case {cid} T {T} (float entry): " + " ".join(f"{n}={v:.3f}" for n, v in r.items()))
    record_errors(f"nce_stream_parity_{cid}", T=T, **r)
    for n, v in r.items():
        assert bool(torch.isfinite(out[n]).all()) and v <= 1.0, (cid, n, v)


# ---- the entropy regulariser riding in the combine launch ----

def _entropy_values(n, special):
    g = torch.Generator().manual_seed(77 + n)
    h = torch.rand(n, generator=g) * 1.2
    if n >= 3:
        h[0], h[n // 2], h[n - 1] = float("nan"), float("inf"), float("-inf")
    elif special is not None:
        h[0] = special
    return h


@functools.lru_cache(maxsize=None)
def _rider_off(cid, T):
    """aecf_loss_fwd_bwd_dt with n_entropy = 0 and no entropy pointers: the contrastive outputs the rider must not move"""
    q, k, off = _inputs(cid)
    (rows, d), cols = q.shape, k.shape[0]
    wsb = _stream_bytes(rows, cols, d)
    gd = Guarded(DEV)
    out = _buffers(gd, rows, cols, d)
    ws = gd.new(wsb, 0xFF)
    status = _call_dt(q, k, off, torch.tensor([T], dtype=F32, device=DEV), 1.0 / cols, out, ws, wsb, ent=(0, 3, 0.7, None, 0.5, None, None))
    torch.cuda.synchronize()
    assert status == 0
    gd.check()
    return out


@pytest.mark.parametrize("last_seq_len", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_entropy_rider(n, last_seq_len):
    """aecf_loss_fwd_bwd_dt on case C: entropy_loss = max(mean((nan_to_num(H) - target)^2), 0) and d_entropy = upstream * 2 / n *
    (H - target) (0 at non-finite entries) against float64 to a relative 2^-20 -- at most 16 float32 roundings for n <= 1000 in
    256 strided sums plus the tree -- with NaN, +inf and -inf among the entries (n = 1: each of them, and a finite one, in
    turn); and the contrastive outputs are the bits of the same call with n_entropy = 0 and NULL entropy pointers (which are in
    turn the bits of aecf_nce_fwd_bwd_dt)."""
    cid, T, target_frac, upstream = "C", 0.005, 0.7, 0.5
    q, k, off = _inputs(cid)
    (rows, d), cols = q.shape, k.shape[0]
    coef = 1.0 / cols
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    wsb = _stream_bytes(rows, cols, d)
    plain = _rider_off(cid, T)
    for name in OUTPUTS:
        assert torch.equal(plain[name], _measured(cid, T)["out"][name]), name
    # the target as the library forms it: the double product, rounded to float32 once
    target = float(torch.tensor((math.log(last_seq_len) if last_seq_len > 1 else 0.0) * target_frac, dtype=F32))
    for special in ([None] if n >= 3 else [None, float("nan"), float("inf"), float("-inf")]):
        h = _entropy_values(n, special)
        gd = Guarded(DEV)
        out = _buffers(gd, rows, cols, d)
        e_loss, d_ent = gd.tensor((1,), F32, 0xFF), gd.tensor((n,), F32, 0xFF)
        ws = gd.new(wsb, 0xFF)
        status = _call_dt(q, k, off, Tt, coef, out, ws, wsb, ent=(n, last_seq_len, target_frac, h.to(DEV), upstream, e_loss, d_ent))
        torch.cuda.synchronize()
        assert status == 0
        gd.check()
        h64 = h.double()
        delta = torch.nan_to_num(h64, nan=0.0, posinf=1.0, neginf=0.0) - target
        want_loss = max(float((delta * delta).mean()), 0.0)
        want_d = torch.where(torch.isfinite(h64), upstream * 2.0 / n * delta, torch.zeros_like(delta))
        got_d = d_ent.cpu().double()
        assert abs(float(e_loss) - want_loss) <= 2.0 ** -20 * want_loss, (n, last_seq_len, special, float(e_loss), want_loss)
        assert bool(((got_d - want_d).abs() <= 2.0 ** -20 * want_d.abs()).all()), (n, last_seq_len, special)
        assert bool((got_d[~torch.isfinite(h64)] == 0).all())
        for name in OUTPUTS:
            assert torch.equal(out[name], plain[name]), (n, last_seq_len, name)


# ---- the Python surface ----

def test_nce_direction_function_low_memory():
    """_NceDirection.apply(q, k, off, T, coef, True) on case C at T = 0.02: the loss and the bf16 gradients on q and on k against
    float64, each inside its bound plus 2^-8 |value| for the rounding of the float32 result to bf16."""
    from aecf_amd.losses import _NceDirection
    cid, T = "C", 0.02
    q0, k0, off = _inputs(cid)
    t, coef, ref, bnd = _want(cid, T)
    q, k = q0.clone().requires_grad_(True), k0.clone().requires_grad_(True)
    loss = _NceDirection.apply(q, k, off, T, coef, True)
    loss.backward()
    assert q.grad.dtype == torch.bfloat16 and k.grad.dtype == torch.bfloat16
    want_loss = coef * float(ref["loss_rows"].sum())
    # float32 sum of the rows (fewer than 2^4 roundings), one product
    assert abs(float(loss.detach()) - want_loss) <= coef * float(bnd["loss_rows"].sum()) + 2.0 ** -20 * abs(want_loss)
    r = {}
    for name, got in (("dq", q.grad), ("dk", k.grad)):
        got = got.double()
        r[name] = float(((got - ref[name]).abs() / (bnd[name] + 2.0 ** -8 * got.abs())).max())
    print(f"nce_stream_parity case {cid} T {T} (_NceDirection, bf16 gradients): " + " ".join(f"{n}={v:.3f}" for n, v in r.items()))
    record_errors("nce_stream_python_direction", T=T, **r)
    assert r["dq"] <= 1.0 and r["dk"] <= 1.0, r


def _after_normalise(zn, inv, g, e_g):
    """The normalise backward dz = (g - zn (zn . g)) inv (include/aecf_hip.h, aecf_l2norm_backward) is linear in g, so an
    elementwise error e_g of g becomes at most (e_g + |zn| (|zn| . e_g)) inv.  Its own float32 arithmetic -- the inverse
    norm's sum, root and quotient, four strided fmaf and six reduction steps of the dot, the product, the difference, the
    scaling: fewer than 16 roundings per element -- adds 2^-20 of the same expression on |g| + e_g.  Returns (float64 dz of
    g, the bound before the final rounding to bf16)."""
    azn = zn.abs()
    through = lambda v: (v + azn * (azn * v).sum(1, keepdim=True)) * inv
    want = (g - zn * (zn * g).sum(1, keepdim=True)) * inv
    return want, through(e_g) + 2.0 ** -20 * through(g.abs() + e_g)


def test_info_nce_tensor_temperature_low_minimum():
    """info_nce(za, zb, temperature = a device tensor holding 0.02, min_temperature = 1e-3) with case C inside it: view b is the
    case's 2049 keys, rows 700 .. 764 of view a are its 65 queries (so those rows see the case's logits, sentinels included,
    across 5 splits of 416 keys, the last 385 = 12 tiles + 1), and the other rows of view a lie at a cosine of about 0.25 to their
    partner, where the softmax at T = 0.02 is not saturated.  Rows are scaled by powers of two, so the normalise has work to do.
    Both directions run the streaming kernels.  Reference: float64 on the bf16 unit rows the kernels read, taken back
    through the documented normalise backward.  Bounds: each direction's dq / dk bound plus 2^-8 |value| for its rounding to
    bf16, the bf16 sum of the two contributions to a view (one more rounding), _after_normalise, and the rounding of the
    result.  na and nb are the library's own l2_normalize outputs: the normalise forward is not checked here (it is outside
    this file's subject; tests/test_losses_gpu.py holds it against torch)."""
    from aecf_amd import losses
    (rows, n, off, d), T = C.CASES["C"][0], 0.02
    case = C.make_case("C")
    g = torch.Generator().manual_seed(4100)
    kb = case["k"].float()
    a = C._unit(0.25 * kb + 0.97 * C._unit(torch.randn(n, d, generator=g)))
    a[off:off + rows] = case["q"].float()
    scale = 2.0 ** torch.randint(-1, 3, (n, 1), generator=g).float()
    za = (a * scale).to(torch.bfloat16).to(DEV).requires_grad_(True)
    zb = (kb * scale.flip(0)).to(torch.bfloat16).to(DEV).requires_grad_(True)
    Tt = torch.tensor(T, dtype=F32, device=DEV, requires_grad=True)
    loss = losses.info_nce(za, zb, temperature=Tt, min_temperature=MIN_T)
    loss.backward()
    t, coef = C.used_temperature(T), 0.5 / n
    with torch.no_grad():
        na, nb = losses.l2_normalize(za.detach()), losses.l2_normalize(zb.detach())
    s32 = na.cpu().float() @ nb.cpu().float().T
    ex = C.eps_x(float((s32.double() - na.cpu().double() @ nb.cpu().double().T).abs().max()), t, n)
    ab = C.reference(na, nb, 0, t, coef)
    ba = C.reference(nb, na, 0, t, coef)
    b_ab, b_ba = C.bounds(ab, na, nb, 0, t, coef, ex), C.bounds(ba, nb, na, 0, t, coef, ex)
    want_loss = coef * float(ab["loss_rows"].sum() + ba["loss_rows"].sum())
    assert abs(float(loss.detach()) - want_loss) <= coef * float(b_ab["loss_rows"].sum() + b_ba["loss_rows"].sum()) + 2.0 ** -20 * abs(want_loss)
    want_dt, b_dt = ab["dT"] + ba["dT"], b_ab["dT"] + b_ba["dT"]
    r = dict(dT=abs(float(Tt.grad) - want_dt) / (b_dt + 2.0 ** -23 * abs(want_dt)))      # (+ the float32 sum of the two terms)
    half = 2.0 ** -8
    sig = {}
    for name, z, zn, own, own_b, other, other_b in (("dza", za, na, ab["dq"], b_ab["dq"], ba["dk"], b_ba["dk"]),
                                                     ("dzb", zb, nb, ba["dq"], b_ba["dq"], ab["dk"], b_ab["dk"])):
        e_own, e_other = own_b + half * (own.abs() + own_b), other_b + half * (other.abs() + other_b)
        g_ref = own + other
        e_g = e_own + e_other + half * (g_ref.abs() + e_own + e_other)
        inv = 1.0 / z.detach().double().norm(dim=1, keepdim=True)
        want, bound = _after_normalise(zn.double(), inv, g_ref, e_g)
        got = z.grad.double()
        r[name] = float(((got - want).abs() / (bound + half * got.abs())).max())
        sig[name] = float((want.abs() / (bound + half * got.abs())).max())
    print(f"nce_stream_parity info_nce n {n} d {d} T {T}: " + " ".join(f"{k_}={v:.3f}" for k_, v in r.items())
          + f" | value/bound dT={abs(want_dt) / b_dt:.3g} " + " ".join(f"{k_}={v:.3g}" for k_, v in sig.items()))
    record_errors("nce_stream_python_info_nce", T=T, **r)
    assert all(v <= 1.0 for v in r.values()), r
