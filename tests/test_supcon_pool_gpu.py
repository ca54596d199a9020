"""The pooled contrastive losses (aecf_supcon_pool_fwd_bwd: the SELF instances of aecf_supcon_flash.hip on aecf_flash_stream.h)
against float64 on the case table of tests/supcon_pool_cases.py -- an excluded key alone in a split, alone in a sub-tile, in the
first tiles, beside the partner --, through the C ABI with ctypes, and their Python surface (losses._SupConPoolDirection,
losses.supervised_contrastive(intra_view=True), losses.nt_xent, fusion_objective(contrastive="nt_xent")).  The float64 reference
and the elementwise bounds are those of tests/supcon_pool_cases.py (tests/test_supcon_pool_cpu.py shows that they catch a
forgotten exclusion and an excluded key counted as a positive).

Every output and the workspace come from the Guarded helper of tests/test_abi_guards_gpu.py, as in tests/test_supcon_gpu.py: the
workspace is exactly aecf_supcon_workspace_bytes long and, like the payloads, prefilled with 0xFF (NaN patterns), so an output
that is finite was written.  min_temperature = 1e-3, coef = 1 / cols."""
import functools

import pytest
import torch

from tests import nce_stream_cases as C
from tests import supcon_pool_cases as P
from tests.helpers import record_errors
from tests.test_abi_guards_gpu import Guarded
from tests.test_nce_stream_gpu import _after_normalise

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MIN_T = 1e-3
ERR_WORKSPACE = -4
F32 = torch.float32
OUTPUTS = ("loss_rows", "dq", "dk", "dT")
CASE_T = [(cid, T) for cid in P.CASE_IDS for T in P.TEMPS]


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = P.make_case(cid)
    return c["q"].to(DEV), c["k"].to(DEV), c["off"], c["self_off"], c["lq"].to(DEV), c["lk"].to(DEV)


def _reference(q, k, off, self_off, lq, lk, t, coef, s_err):
    """(float64 reference, bounds) of one direction on the device of its inputs"""
    excl = P.excluded(q.shape[0], k.shape[0], self_off, q.device)
    M = P.match_matrix(lq, lk, off, self_off)
    ref = P.reference(q, k, M, excl, t, coef)
    return ref, P.bounds(ref, q, k, M, t, coef, C.eps_x(s_err, t, k.shape[0]))


@functools.lru_cache(maxsize=None)
def _want(cid, T):
    """(T as the kernels read it, coef, float64 reference, bounds) of a case, computed once on the device in float64; the
    score error inside eps_x comes from torch's CPU products"""
    q, k, off, self_off, lq, lk = _inputs(cid)
    t, coef = C.used_temperature(T), 1.0 / k.shape[0]
    ref, bnd = _reference(q, k, off, self_off, lq, lk, t, coef, P.score_error(cid))
    return t, coef, {n: ref[n] for n in OUTPUTS}, bnd


def _buffers(gd, rows, cols, d, fill=0xFF):
    return dict(loss_rows=gd.tensor((rows,), F32, fill), dq=gd.tensor((rows, d), F32, fill), dk=gd.tensor((cols, d), F32, fill),
                dT=gd.tensor((1,), F32, fill))


def _call(q, k, off, self_off, lq, lk, T, coef, out, ws, wsb, grads=True):
    """aecf_supcon_pool_fwd_bwd; T: a device scalar; grads False: the loss-only mode (dq = dk = d_temperature = NULL)"""
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    rows, d = q.shape
    g = (lambda t_: _ptr(t_)) if grads else (lambda t_: None)
    return _lib.load().aecf_supcon_pool_fwd_bwd(rows, k.shape[0], off, self_off, d, _ptr(T), MIN_T, coef, _ptr(q), _ptr(k), _ptr(lq),
                                                _ptr(lk), _ptr(out["loss_rows"]), g(out["dq"]), g(out["dk"]), g(out["dT"]), _ptr(ws),
                                                wsb, _stream())


def _run(q, k, off, self_off, lq, lk, T, fill=0xFF, short=0, grads=True):
    """one call on fresh guarded buffers: (status, outputs, workspace, guards)"""
    from aecf_amd import _lib
    (rows, d), cols = q.shape, k.shape[0]
    wsb = _lib.load().aecf_supcon_workspace_bytes(rows, cols, d)
    assert wsb > 0
    gd = Guarded(DEV)
    out = _buffers(gd, rows, cols, d)
    ws = gd.new(wsb, fill)
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    status = _call(q, k, off, self_off, lq, lk, Tt, 1.0 / cols, out, ws, wsb - short, grads)
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
def test_outputs_inside_the_bounds(cid, T):
    """loss_rows, dq, dk and d_temperature of every case, elementwise, at T = 0.07 and at T = 0.005; all finite (an all -inf
    sub-tile or split must not leave a NaN), so every element was written; guards intact"""
    status, out, _, gd = _measured(cid, T)["full"]
    assert status == 0
    _, _, ref, bnd = _want(cid, T)
    r = _ratios(out, ref, bnd)
    sig = C.signal(ref, bnd)
    print(f"supcon_pool_parity case {cid} T {T}: " + " ".join(f"{n}={r[n]:.3f}" for n in OUTPUTS)
          + " | value/bound " + " ".join(f"{n}={sig[n]:.3g}" for n in OUTPUTS))
    record_errors(f"supcon_pool_parity_{cid}", T=T, **r)
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


@pytest.mark.parametrize("T", P.TEMPS)
def test_only_the_partner_survives_exactly_zero(T):
    """P1: one row, its partner and itself.  lse is the partner's x, the softmax is 1 on it and so is match / n: the loss and
    every gradient are 0 exactly, whatever the temperature"""
    status, out, _, gd = _measured("P1", T)["full"]
    assert status == 0
    gd.check()
    for n in OUTPUTS:
        assert bool((out[n] == 0).all()), (T, n, out[n])


def test_row_shards_add_up_to_the_one_call():
    """P3's 65 rows as two row shards (32 + 33) against the same keys, each with its own offsets, as two ranks would call: the
    concatenated loss_rows lie inside the one-call reference's bounds, and so does the sum (in float64) of the two dk shares
    inside its dk bound -- that bound is a sum over the rows, so it IS the sum of the shards' bounds."""
    q, k, off, self_off, lq, lk = _inputs("P3")
    for T in P.TEMPS:
        _, _, ref, bnd = _want("P3", T)
        cut = 32
        s1, a, _, g1 = _run(q[:cut].contiguous(), k, off, self_off, lq[:cut].contiguous(), lk, T)
        s2, b, _, g2 = _run(q[cut:].contiguous(), k, off + cut, self_off + cut, lq[cut:].contiguous(), lk, T)
        assert s1 == 0 and s2 == 0
        g1.check()
        g2.check()
        got = dict(loss_rows=torch.cat([a["loss_rows"], b["loss_rows"]]), dq=torch.cat([a["dq"], b["dq"]]),
                   dk=a["dk"].double() + b["dk"].double(), dT=float(a["dT"]) + float(b["dT"]))
        r = C.ratios(got, ref, bnd)
        print(f"supcon_pool_parity case P3 T {T} (two row shards): " + " ".join(f"{n}={r[n]:.3f}" for n in OUTPUTS))
        record_errors("supcon_pool_shards_P3", T=T, **r)
        for n in OUTPUTS:
            assert r[n] <= 1.0, (T, n, r[n])


# ---- the Python surface ----

def test_direction_function():
    """_SupConPoolDirection on P3 at T = 0.07: the loss and the bf16 gradients on q and on the pool against float64, each inside
    its bound plus 2^-8 |value| for the rounding of the float32 result to bf16."""
    from aecf_amd.losses import _SupConPoolDirection
    cid, T = "P3", 0.07
    q0, k0, off, self_off, lq, lk = _inputs(cid)
    t, coef, ref, bnd = _want(cid, T)
    q, k = q0.clone().requires_grad_(True), k0.clone().requires_grad_(True)
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    loss = _SupConPoolDirection.apply(q, k, lq, lk, off, self_off, Tt, coef, MIN_T, True)
    loss.backward()
    assert q.grad.dtype == torch.bfloat16 and k.grad.dtype == torch.bfloat16
    want_loss = coef * float(ref["loss_rows"].sum())
    # float32 sum of the rows (fewer than 2^4 roundings), one product
    assert abs(float(loss.detach()) - want_loss) <= coef * float(bnd["loss_rows"].sum()) + 2.0 ** -20 * abs(want_loss)
    r = {}
    for name, got in (("dq", q.grad), ("dk", k.grad)):
        got = got.double()
        r[name] = float(((got - ref[name]).abs() / (bnd[name] + 2.0 ** -8 * got.abs())).max())
    print(f"supcon_pool_parity case {cid} T {T} (_SupConPoolDirection, bf16 gradients): " + " ".join(f"{n}={v:.3f}" for n, v in r.items()))
    record_errors("supcon_pool_python_direction", T=T, **r)
    assert r["dq"] <= 1.0 and r["dk"] <= 1.0, r
    with torch.no_grad():
        quiet = _SupConPoolDirection.apply(q0, k0, lq, lk, off, self_off, Tt, coef, MIN_T, False)
    assert torch.equal(quiet, loss.detach())


@functools.lru_cache(maxsize=None)
def _batch():
    """A batch of 300 rows per view that holds P7: view b is the case's keys (its rows 100 .. 162 are exact copies of the case's
    queries, so the pool holds duplicates of anchors beside the anchors themselves), rows 237 .. 299 of view a are its queries
    and the other rows of view a lie at a cosine of about 0.25 to their partner; rows scaled by powers of two, so the normalise
    has work to do (built as tests/test_supcon_gpu.py builds its batch).  The labels of all rows are the case's key labels."""
    (rows, n, off, _, d) = P.CASES["P7"][0]
    case = P.make_case("P7")
    g = torch.Generator().manual_seed(5100)
    kb = case["k"].float()
    a = C._unit(0.25 * kb + 0.97 * C._unit(torch.randn(n, d, generator=g)))
    a[off:off + rows] = case["q"].float()
    scale = 2.0 ** torch.randint(-1, 3, (n, 1), generator=g).float()
    za = (a * scale).to(torch.bfloat16).to(DEV)
    zb = (kb * scale.flip(0)).to(torch.bfloat16).to(DEV)
    return za, zb, case["lk"].to(DEV)


def _pool_check(name, call, labels, T):
    """``call(za, zb, Tt)`` = one of the pooled losses on the batch; reference: float64 over the 2 B x 2 B pool of the bf16 unit
    rows the kernels read, the diagonal removed, both halves of the anchors (view a with partner offset 0 and itself at B, view
    b the other way round), taken back through the documented normalise backward.  Bounds: each direction's dq / dk bound plus
    2^-8 |value| for its rounding to bf16; a view's gradient is the bf16 sum of three such terms (its dq and its half of both
    dk) in two additions of an order autograd chooses, each rounding at most 2^-8 of the absolute sum so far; then
    _after_normalise and the rounding of the result.  Under torch.no_grad() the value has the same bits."""
    from aecf_amd import losses
    za0, zb0, _ = _batch()
    n = za0.shape[0]
    za, zb = za0.clone().requires_grad_(True), zb0.clone().requires_grad_(True)
    Tt = torch.tensor(T, dtype=F32, device=DEV, requires_grad=True)
    with torch.no_grad():
        quiet = call(za, zb, Tt)
    loss = call(za, zb, Tt)
    loss.backward()
    assert torch.equal(quiet, loss.detach()) and not quiet.requires_grad

    t, coef = C.used_temperature(T), 0.5 / n
    with torch.no_grad():
        na, nb = losses.l2_normalize(za.detach()), losses.l2_normalize(zb.detach())
    pool, lab2 = torch.cat([nb, na]), torch.cat([labels, labels])
    pc = pool.cpu()
    s_err = float(((pc.float() @ pc.float().T).double() - pc.double() @ pc.double().T).abs().max())
    A, bA = _reference(na, pool, 0, n, labels, lab2, t, coef, s_err)
    B, bB = _reference(nb, pool, n, 0, labels, lab2, t, coef, s_err)
    want_loss = coef * float(A["loss_rows"].sum() + B["loss_rows"].sum())
    assert abs(float(loss.detach()) - want_loss) <= coef * float(bA["loss_rows"].sum() + bB["loss_rows"].sum()) + 2.0 ** -20 * abs(want_loss)
    want_dt, b_dt = A["dT"] + B["dT"], bA["dT"] + bB["dT"]
    r = dict(dT=abs(float(Tt.grad) - want_dt) / (b_dt + 2.0 ** -23 * abs(want_dt)))      # (+ the float32 sum of the two terms)
    half = 2.0 ** -8
    sig = {}
    for vname, z, zn, own, own_b, lo in (("dza", za, na, A["dq"], bA["dq"], n), ("dzb", zb, nb, B["dq"], bB["dq"], 0)):
        terms = [(own, own_b), (A["dk"][lo:lo + n], bA["dk"][lo:lo + n]), (B["dk"][lo:lo + n], bB["dk"][lo:lo + n])]
        g_ref = sum(v for v, _ in terms)
        e_sum = sum(b_ + half * (v.abs() + b_) for v, b_ in terms)              # each term rounded to bf16 once
        mass = sum(v.abs() for v, _ in terms) + e_sum
        r1 = half * mass
        e_g = e_sum + r1 + half * (mass + r1)                                   # two additions in bf16
        inv = 1.0 / z.detach().double().norm(dim=1, keepdim=True)
        want, bound = _after_normalise(zn.double(), inv, g_ref, e_g)
        got = z.grad.double()
        r[vname] = float(((got - want).abs() / (bound + half * got.abs())).max())
        sig[vname] = float((want.abs() / (bound + half * got.abs())).max())
    print(f"supcon_pool_parity {name} n {n} T {T}: " + " ".join(f"{k_}={v:.3f}" for k_, v in r.items())
          + f" | value/bound dT={abs(want_dt) / b_dt:.3g} " + " ".join(f"{k_}={v:.3g}" for k_, v in sig.items()))
    record_errors(f"supcon_pool_python_{name}", T=T, **r)
    assert all(v <= 1.0 for v in r.values()), r
    return loss.detach()


def test_supervised_contrastive_intra_view():
    """supervised_contrastive(za, zb, labels, temperature = a device tensor holding 0.07, min_temperature = 1e-3,
    intra_view=True) on the batch that holds P7"""
    from aecf_amd import losses
    _, _, labels = _batch()
    _pool_check("supervised_intra_view", lambda a, b, t: losses.supervised_contrastive(a, b, labels, temperature=t, min_temperature=MIN_T,
                                                                                      intra_view=True), labels, 0.07)


def test_nt_xent():
    """nt_xent on the same batch is the pooled loss with every label -1, and not the labeled one"""
    from aecf_amd import losses
    za, zb, labels = _batch()
    none = torch.full_like(labels, -1)
    got = _pool_check("nt_xent", lambda a, b, t: losses.nt_xent(a, b, temperature=t, min_temperature=MIN_T), none, 0.07)
    same = losses.supervised_contrastive(za, zb, none, temperature=0.07, min_temperature=MIN_T, intra_view=True)
    other = losses.supervised_contrastive(za, zb, labels, temperature=0.07, min_temperature=MIN_T, intra_view=True)
    assert torch.equal(got, same) and not torch.equal(got, other)


def test_cross_view_path_is_untouched():
    """intra_view=False is the call without the argument, bit for bit, in both implementations; and the pooled loss is another"""
    from aecf_amd import losses
    za, zb, labels = _batch()
    for low_memory in (True, False):
        assert torch.equal(losses.supervised_contrastive(za, zb, labels, temperature=0.07, low_memory=low_memory, intra_view=False),
                           losses.supervised_contrastive(za, zb, labels, temperature=0.07, low_memory=low_memory))
    assert not torch.equal(losses.supervised_contrastive(za, zb, labels, temperature=0.07, intra_view=True),
                           losses.supervised_contrastive(za, zb, labels, temperature=0.07))
    with pytest.raises(NotImplementedError, match="intra-view"):
        losses.supervised_contrastive(za, zb, labels, low_memory=False, intra_view=True)
    assert torch.equal(losses.supervised_contrastive(za, zb, labels, temperature=0.07, low_memory=None, intra_view=True),
                       losses.supervised_contrastive(za, zb, labels, temperature=0.07, intra_view=True))
    z = torch.zeros(64, 192, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(NotImplementedError, match=r"128, 256, 384, 512, 768, 1024"):
        losses.nt_xent(z, z)


def test_fusion_objective_takes_nt_xent_and_intra_view():
    """fusion_objective(..., contrastive="nt_xent") == task + nt_xent(...), and contrastive="supervised" with intra_view=True ==
    task + supervised_contrastive(..., intra_view=True), bit for bit"""
    from aecf_amd import losses
    za, zb, labels = _batch()
    task = torch.tensor(0.625, dtype=F32, device=DEV)
    got = losses.fusion_objective(task, None, None, za, zb, contrastive="nt_xent", temperature=0.07)
    assert torch.equal(got, task + losses.nt_xent(za, zb, temperature=0.07))
    got = losses.fusion_objective(task, None, None, za, zb, contrastive="supervised", labels=labels, temperature=0.07, intra_view=True)
    assert torch.equal(got, task + losses.supervised_contrastive(za, zb, labels, temperature=0.07, intra_view=True))


def test_captured_step_reads_temperature_and_labels_at_replay():
    """forward + backward of the pooled loss inside torch.cuda.graph; new values written in place into the temperature tensor
    and the labels; the replay equals an eager call on the new values bit for bit (no host read anywhere)."""
    from aecf_amd import losses
    za, zb, labels = _batch()
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    T = torch.tensor(0.07, dtype=F32, device=DEV, requires_grad=True)
    lab = torch.full_like(labels, -1)

    def step():
        return losses.supervised_contrastive(a, b, lab, temperature=T, min_temperature=MIN_T, intra_view=True)

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
    want = losses.supervised_contrastive(a2, b2, labels, temperature=T2, min_temperature=MIN_T, intra_view=True)
    want.backward()
    plain = losses.nt_xent(za, zb, temperature=T2.detach(), min_temperature=MIN_T)
    assert not torch.equal(plain, want.detach())                  # the labels matter to the value the replay must reach
    assert torch.equal(got[0], want.detach())
    assert torch.equal(got[1], a2.grad) and torch.equal(got[2], b2.grad)
    assert torch.equal(got[3], T2.grad)
