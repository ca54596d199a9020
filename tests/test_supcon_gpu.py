"""The streaming supervised contrastive loss (aecf_supcon_flash.hip on aecf_flash_stream.h) against float64 at the split and tile
edges of tests/nce_stream_cases.py with the label plan of tests/supcon_cases.py, through the C ABI with ctypes, and its Python
surface (losses._SupConDirection, losses.supervised_contrastive, fusion_objective(contrastive="supervised")).  The float64
reference and the elementwise bounds are those of tests/supcon_cases.py, derived from the design's roundings
(tests/test_supcon_cpu.py shows that they catch a lost positive, a 32-bit label compare and unlabeled rows matched as a class).

Every output and the workspace come from the Guarded helper of tests/test_abi_guards_gpu.py: the workspace is exactly
aecf_supcon_workspace_bytes long and, like the payloads, prefilled with 0xFF (NaN patterns): an output that is finite was
written, and a slot of case H's empty split that entered a merge would show.  min_temperature = 1e-3, coef = 1 / cols."""
import functools

import pytest
import torch

from tests import nce_stream_cases as C
from tests import supcon_cases as S
from tests.helpers import record_errors
from tests.test_abi_guards_gpu import Guarded
from tests.test_nce_stream_gpu import _after_normalise

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MIN_T = 1e-3
ERR_WORKSPACE = -4
F32 = torch.float32
OUTPUTS = ("loss_rows", "dq", "dk", "dT")
CASE_T = [(cid, T) for cid in S.CASE_IDS for T in S.TEMPS]


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = C.make_case(S.base(cid))
    L = S.labels(cid)
    return c["q"].to(DEV), c["k"].to(DEV), c["off"], L["lq"].to(DEV), L["lk"].to(DEV)


@functools.lru_cache(maxsize=None)
def _want(cid, T):
    """(T as the kernels read it, coef, float64 reference, bounds) of a case, computed once on the device in float64; the
    score error inside eps_x comes from torch's CPU products"""
    q, k, off, lq, lk = _inputs(cid)
    cols = k.shape[0]
    t, coef = C.used_temperature(T), 1.0 / cols
    M = S.match_matrix(lq, lk, off)
    ref = S.reference(q, k, M, t, coef)
    bnd = S.bounds(ref, q, k, M, t, coef, C.eps_x(C.score_error(S.base(cid)), t, cols))
    return t, coef, S.slim(ref), bnd


def _buffers(gd, rows, cols, d, fill=0xFF):
    return dict(loss_rows=gd.tensor((rows,), F32, fill), dq=gd.tensor((rows, d), F32, fill), dk=gd.tensor((cols, d), F32, fill),
                dT=gd.tensor((1,), F32, fill))


def _call(q, k, off, lq, lk, T, coef, out, ws, wsb, grads=True):
    """aecf_supcon_fwd_bwd; T: a device scalar; grads False: the loss-only mode (dq = dk = d_temperature = NULL)"""
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    rows, d = q.shape
    g = (lambda t_: _ptr(t_)) if grads else (lambda t_: None)
    return _lib.load().aecf_supcon_fwd_bwd(rows, k.shape[0], off, d, _ptr(T), MIN_T, coef, _ptr(q), _ptr(k), _ptr(lq), _ptr(lk),
                                           _ptr(out["loss_rows"]), g(out["dq"]), g(out["dk"]), g(out["dT"]), _ptr(ws), wsb, _stream())


def _ws_bytes(rows, cols, d):
    from aecf_amd import _lib
    wsb = _lib.load().aecf_supcon_workspace_bytes(rows, cols, d)
    assert wsb == S.workspace_bytes_py(rows, cols, d)
    return wsb


def _run(q, k, off, lq, lk, T, fill=0xFF, short=0, grads=True):
    """one call on fresh guarded buffers: (status, outputs, workspace, guards)"""
    (rows, d), cols = q.shape, k.shape[0]
    wsb = _ws_bytes(rows, cols, d)
    gd = Guarded(DEV)
    out = _buffers(gd, rows, cols, d)
    ws = gd.new(wsb, fill)
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    status = _call(q, k, off, lq, lk, Tt, 1.0 / cols, out, ws, wsb - short, grads)
    torch.cuda.synchronize()
    return status, out, ws, gd


@functools.lru_cache(maxsize=None)
def _measured(cid, T):
    """One case at one temperature: the call on a 0xFF-filled workspace of exactly the documented size, the same call on a
    zero-filled one, a call with the size one byte short and a loss-only call -- run once, judged by the tests below."""
    args = _inputs(cid)
    return dict(full=_run(*args, T), zero=_run(*args, T, fill=0), short=_run(*args, T, short=1), loss=_run(*args, T, grads=False))


def _ratios(out, ref, bnd):
    return C.ratios(dict(loss_rows=out["loss_rows"], dq=out["dq"], dk=out["dk"], dT=float(out["dT"])), ref, bnd)


@pytest.mark.parametrize("cid,T", CASE_T)
def test_outputs_inside_the_derived_bounds(cid, T):
    """loss_rows, dq, dk and d_temperature of every case, elementwise, at T = 0.07 and at T = 0.005; all finite, so every element
    was written (and no slot of an empty split was read); guards intact"""
    status, out, _, gd = _measured(cid, T)["full"]
    assert status == 0
    _, _, ref, bnd = _want(cid, T)
    r = _ratios(out, ref, bnd)
    sig = C.signal(ref, bnd)
    print(f"supcon_parity case {cid} T {T}: " + " ".join(f"{n}={r[n]:.3f}" for n in OUTPUTS)
          + " | value/bound " + " ".join(f"{n}={sig[n]:.3g}" for n in OUTPUTS))
    record_errors(f"supcon_parity_{cid}", T=T, **r)
    gd.check()
    for n in OUTPUTS:
        assert bool(torch.isfinite(out[n]).all()), (cid, T, n)
        assert r[n] <= 1.0, (cid, T, n, r[n])


@pytest.mark.parametrize("cid,T", CASE_T)
def test_workspace_contents_do_not_matter(cid, T):
    """The same call on a zero-filled workspace: bit-identical outputs (fixed-order sums, nothing read before it is written)."""
    m = _measured(cid, T)
    status, again, _, gd = m["zero"]
    assert status == 0
    gd.check()
    for n in OUTPUTS:
        assert torch.equal(m["full"][1][n], again[n]), (cid, T, n)


@pytest.mark.parametrize("cid,T", CASE_T)
def test_workspace_one_byte_short_is_refused(cid, T):
    status, out, ws, gd = _measured(cid, T)["short"]
    assert status == ERR_WORKSPACE
    gd.check()
    for n in OUTPUTS:
        assert bool((out[n].view(torch.uint8) == 0xFF).all()), (cid, T, n)
    assert bool((ws == 0xFF).all())


@pytest.mark.parametrize("cid,T", CASE_T)
def test_loss_only_call_has_the_same_loss_bits(cid, T):
    """dq = dk = d_temperature = NULL: loss_rows as in the full call, nothing else touched"""
    m = _measured(cid, T)
    status, out, _, gd = m["loss"]
    assert status == 0
    gd.check()
    assert torch.equal(out["loss_rows"], m["full"][1]["loss_rows"])
    for n in ("dq", "dk", "dT"):
        assert bool((out[n].view(torch.uint8) == 0xFF).all()), (cid, T, n)


@pytest.mark.parametrize("T", S.TEMPS)
def test_without_shared_labels_it_is_info_nce(T):
    """Case C with every label -1, and with all labels distinct and non-negative: the same bits, inside the InfoNCE bounds of the
    InfoNCE reference (tests/nce_stream_cases.py)."""
    q, k, off, _, _ = _inputs("C")
    cols = k.shape[0]
    none = torch.full((cols,), -1, dtype=torch.int64, device=DEV)
    distinct = torch.arange(cols, dtype=torch.int64, device=DEV) * (2 ** 33 + 1)
    s1, a, _, g1 = _run(q, k, off, none[off:off + q.shape[0]], none, T)
    s2, b, _, g2 = _run(q, k, off, distinct[off:off + q.shape[0]], distinct, T)
    assert s1 == 0 and s2 == 0
    g1.check()
    g2.check()
    for n in OUTPUTS:
        assert torch.equal(a[n], b[n]), (T, n)
    t, coef = C.used_temperature(T), 1.0 / cols
    ref = C.reference(q, k, off, t, coef)
    bnd = C.bounds(ref, q, k, off, t, coef, C.eps_x(C.score_error("C"), t, cols))
    r = _ratios(a, ref, bnd)
    print(f"supcon_parity case C T {T} (no shared labels, InfoNCE bounds): " + " ".join(f"{n}={r[n]:.3f}" for n in OUTPUTS))
    record_errors("supcon_as_info_nce_C", T=T, **r)
    for n in OUTPUTS:
        assert r[n] <= 1.0, (T, n, r[n])


def test_temperature_below_the_minimum_is_clamped():
    """Case C with *T = 5e-4 < min_temperature = 1e-3: d_temperature == 0 exactly, every other output the bits of *T = 1e-3."""
    args = _inputs("C")
    s1, low, _, g1 = _run(*args, 5e-4)
    s2, at, _, g2 = _run(*args, 1e-3)
    assert s1 == 0 and s2 == 0
    g1.check()
    g2.check()
    assert float(low["dT"]) == 0.0 and float(at["dT"]) != 0.0
    for n in ("loss_rows", "dq", "dk"):
        assert torch.equal(low[n], at[n]), n


# ---- the Python surface ----

def test_direction_function():
    """_SupConDirection on case C at T = 0.02: the loss and the bf16 gradients on q and on k against float64, each inside its
    bound plus 2^-8 |value| for the rounding of the float32 result to bf16."""
    from aecf_amd.losses import _SupConDirection
    cid, T = "C", 0.02
    q0, k0, off, lq, lk = _inputs(cid)
    t, coef, ref, bnd = _want(cid, T)
    q, k = q0.clone().requires_grad_(True), k0.clone().requires_grad_(True)
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    loss = _SupConDirection.apply(q, k, lq, lk, off, Tt, coef, MIN_T, True)
    loss.backward()
    assert q.grad.dtype == torch.bfloat16 and k.grad.dtype == torch.bfloat16
    want_loss = coef * float(ref["loss_rows"].sum())
    # float32 sum of the rows (fewer than 2^4 roundings), one product
    assert abs(float(loss.detach()) - want_loss) <= coef * float(bnd["loss_rows"].sum()) + 2.0 ** -20 * abs(want_loss)
    r = {}
    for name, got in (("dq", q.grad), ("dk", k.grad)):
        got = got.double()
        r[name] = float(((got - ref[name]).abs() / (bnd[name] + 2.0 ** -8 * got.abs())).max())
    print(f"supcon_parity case {cid} T {T} (_SupConDirection, bf16 gradients): " + " ".join(f"{n}={v:.3f}" for n, v in r.items()))
    record_errors("supcon_python_direction", T=T, **r)
    assert r["dq"] <= 1.0 and r["dk"] <= 1.0, r


@functools.lru_cache(maxsize=None)
def _batch(cid):
    """A batch that holds a case: view b is the case's keys, rows off .. off + rows - 1 of view a are its queries and the other
    rows of view a lie at a cosine of about 0.25 to their partner; rows scaled by powers of two, so the normalise has work to do
    (built as test_info_nce_tensor_temperature_low_minimum of tests/test_nce_stream_gpu.py builds its batch).  The labels of all
    n rows are the case's key labels: the plan of tests/supcon_cases.py on every row, lq = lk[off : off + rows]."""
    (rows, n, off, d) = C.CASES[cid][0]
    case = C.make_case(cid)
    g = torch.Generator().manual_seed(4100)
    kb = case["k"].float()
    a = C._unit(0.25 * kb + 0.97 * C._unit(torch.randn(n, d, generator=g)))
    a[off:off + rows] = case["q"].float()
    scale = 2.0 ** torch.randint(-1, 3, (n, 1), generator=g).float()
    za = (a * scale).to(torch.bfloat16).to(DEV)
    zb = (kb * scale.flip(0)).to(torch.bfloat16).to(DEV)
    return za, zb, S.labels(cid)["lk"].to(DEV)


def test_supervised_contrastive_tensor_temperature_low_minimum():
    """supervised_contrastive(za, zb, labels, temperature = a device tensor holding 0.02, min_temperature = 1e-3) with case C
    inside a 2049-row batch.  Reference: float64 on the bf16 unit rows the kernels read, taken back through the documented
    normalise backward.  Bounds: each direction's dq / dk bound plus 2^-8 |value| for its rounding to bf16, the bf16 sum of the
    two contributions to a view (one more rounding), _after_normalise, and the rounding of the result.  Under torch.no_grad()
    the value has the same bits and the call's peak memory is strictly lower (no gradient buffers)."""
    from aecf_amd import losses
    T = 0.02
    za0, zb0, labels = _batch("C")
    n = za0.shape[0]
    za, zb = za0.clone().requires_grad_(True), zb0.clone().requires_grad_(True)
    Tt = torch.tensor(T, dtype=F32, device=DEV, requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        quiet = losses.supervised_contrastive(za, zb, labels, temperature=Tt, min_temperature=MIN_T)
    torch.cuda.synchronize()
    peak_quiet = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = losses.supervised_contrastive(za, zb, labels, temperature=Tt, min_temperature=MIN_T)
    torch.cuda.synchronize()
    peak_grad = torch.cuda.max_memory_allocated()
    loss.backward()
    assert torch.equal(quiet, loss.detach()) and not quiet.requires_grad
    print(f"supcon peak memory: with gradients {peak_grad}, under no_grad {peak_quiet}")
    assert peak_quiet < peak_grad

    t, coef = C.used_temperature(T), 0.5 / n
    with torch.no_grad():
        na, nb = losses.l2_normalize(za.detach()), losses.l2_normalize(zb.detach())
    s32 = na.cpu().float() @ nb.cpu().float().T
    ex = C.eps_x(float((s32.double() - na.cpu().double() @ nb.cpu().double().T).abs().max()), t, n)
    M = S.match_matrix(labels, labels, 0)
    ab, ba = S.reference(na, nb, M, t, coef), S.reference(nb, na, M, t, coef)
    b_ab, b_ba = S.bounds(ab, na, nb, M, t, coef, ex), S.bounds(ba, nb, na, M, t, coef, ex)
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
    print(f"supcon_parity supervised_contrastive n {n} T {T}: " + " ".join(f"{k_}={v:.3f}" for k_, v in r.items())
          + f" | value/bound dT={abs(want_dt) / b_dt:.3g} " + " ".join(f"{k_}={v:.3g}" for k_, v in sig.items()))
    record_errors("supcon_python_supervised_contrastive", T=T, **r)
    assert all(v <= 1.0 for v in r.values()), r


def test_python_refuses_what_the_kernels_do_not_serve():
    from aecf_amd import losses
    lab = torch.zeros(64, dtype=torch.int64, device=DEV)
    for z in (torch.zeros(64, 192, dtype=torch.bfloat16, device=DEV), torch.zeros(64, 256, dtype=torch.float32, device=DEV)):
        with pytest.raises(NotImplementedError, match=r"128, 256, 384, 512, 768, 1024"):
            losses.supervised_contrastive(z, z, lab)
    z = torch.zeros(64, 256, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="labels"):
        losses.supervised_contrastive(z, z, lab.cpu())
    with pytest.raises(ValueError, match="labels"):
        losses.supervised_contrastive(z, z, lab[:63])
    with pytest.raises(TypeError, match="labels"):
        losses.supervised_contrastive(z, z, lab.float())


def test_fusion_objective_takes_the_supervised_term():
    """fusion_objective(..., contrastive="supervised", labels=...) == task + supervised_contrastive(...), bit for bit; int32
    labels are widened to the same answer"""
    from aecf_amd import losses
    za, zb, labels = _batch("D")
    task = torch.tensor(0.625, dtype=F32, device=DEV)
    got = losses.fusion_objective(task, None, None, za, zb, contrastive="supervised", labels=labels, temperature=0.07)
    term = losses.supervised_contrastive(za, zb, labels, temperature=0.07)
    assert torch.equal(got, task + term)
    small = torch.where(labels > 2 ** 31 - 1, labels % 1000 + 500000, labels)            # (fits int32; another plan, same for both)
    assert torch.equal(losses.supervised_contrastive(za, zb, small.to(torch.int32), temperature=0.07),
                       losses.supervised_contrastive(za, zb, small, temperature=0.07))


def test_captured_step_reads_temperature_and_labels_at_replay():
    """forward + backward inside torch.cuda.graph on case D's batch; new values written in place into the temperature tensor and
    the labels; the replay equals an eager call on the new values bit for bit (no host read anywhere)."""
    from aecf_amd import losses
    za, zb, labels = _batch("D")
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    T = torch.tensor(0.07, dtype=F32, device=DEV, requires_grad=True)
    lab = torch.full_like(labels, -1)

    def step():
        return losses.supervised_contrastive(a, b, lab, temperature=T, min_temperature=MIN_T)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            a.grad = b.grad = T.grad = None
            step().backward()
    torch.cuda.current_stream().wait_stream(s)
    a.grad = b.grad = T.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
        loss.backward()
    with torch.no_grad():
        T.copy_(torch.tensor(0.02))
        lab.copy_(labels)
    graph.replay()
    torch.cuda.synchronize()
    got = (loss.detach().clone(), a.grad.clone(), b.grad.clone(), T.grad.clone())
    a2, b2 = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    T2 = torch.tensor(0.02, dtype=F32, device=DEV, requires_grad=True)
    want = losses.supervised_contrastive(a2, b2, labels, temperature=T2, min_temperature=MIN_T)
    want.backward()
    plain = losses.supervised_contrastive(za, zb, torch.full_like(labels, -1), temperature=T2.detach(), min_temperature=MIN_T)
    assert not torch.equal(plain, want.detach())                  # the labels matter to the value the replay must reach
    assert torch.equal(got[0], want.detach())
    assert torch.equal(got[1], a2.grad) and torch.equal(got[2], b2.grad)
    assert torch.equal(got[3], T2.grad)
