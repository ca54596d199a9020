"""The streaming multi-label supervised contrastive loss (aecf_supcon_ml_flash.hip on aecf_flash_stream.h) against float64 at the
split and tile edges of tests/nce_stream_cases.py with the set plan of tests/supcon_ml_cases.py, through the C ABI with ctypes, and
its Python surface (losses.pack_label_sets, losses._SupConMlDirection, losses.multilabel_contrastive,
fusion_objective(contrastive="multilabel")).  The float64 reference and the elementwise bounds are those of
tests/supcon_ml_cases.py, derived from the design's roundings (tests/test_supcon_ml_cpu.py shows that they catch a 32-bit and,
low-word popcounts, the wrong weighting, a partner weighted by its sets and empty sets that match).

Every output and the workspace come from the Guarded helper of tests/test_abi_guards_gpu.py: the workspace is exactly
aecf_supcon_ml_workspace_bytes long and, like the payloads, prefilled with 0xFF (NaN patterns): an output that is finite was
written, and a slot of case H's empty split that entered a merge would show.  min_temperature = 1e-3, coef = 1 / cols."""
import functools

import pytest
import torch

from tests import nce_stream_cases as C
from tests import supcon_ml_cases as S
from tests.helpers import record_errors
from tests.test_abi_guards_gpu import Guarded
from tests.test_nce_stream_gpu import _after_normalise

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MIN_T = 1e-3
ERR_WORKSPACE = -4
F32 = torch.float32
OUTPUTS = ("loss_rows", "dq", "dk", "dT")
WEIGHTING = {"overlap": 0, "jaccard": 1}
CASE_T_W = [(cid, T, w) for cid in S.CASE_IDS for T in S.TEMPS for w in S.WEIGHTINGS]


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = C.make_case(S.base(cid))
    L = S.sets(cid)
    return c["q"].to(DEV), c["k"].to(DEV), c["off"], L["sq"].to(DEV), L["sk"].to(DEV)


@functools.lru_cache(maxsize=None)
def _want(cid, T, weighting):
    """(T as the kernels read it, coef, float64 reference, bounds) of a case, computed once on the device in float64; the
    score error inside eps_x comes from torch's CPU products"""
    q, k, off, sq, sk = _inputs(cid)
    cols = k.shape[0]
    t, coef = C.used_temperature(T), 1.0 / cols
    ref = S.reference(q, k, S.weights(sq, sk, off, weighting), t, coef)
    bnd = S.bounds(ref, q, k, t, coef, C.eps_x(C.score_error(S.base(cid)), t, cols))
    return t, coef, S.slim(ref), bnd


def _buffers(gd, rows, cols, d, fill=0xFF):
    return dict(loss_rows=gd.tensor((rows,), F32, fill), dq=gd.tensor((rows, d), F32, fill), dk=gd.tensor((cols, d), F32, fill),
                dT=gd.tensor((1,), F32, fill))


def _call(q, k, off, sq, sk, weighting, T, coef, out, ws, wsb, grads=True):
    """aecf_supcon_ml_fwd_bwd; T: a device scalar; grads False: the loss-only mode (dq = dk = d_temperature = NULL)"""
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    rows, d = q.shape
    g = (lambda t_: _ptr(t_)) if grads else (lambda t_: None)
    return _lib.load().aecf_supcon_ml_fwd_bwd(rows, k.shape[0], off, d, _ptr(T), MIN_T, coef, _ptr(q), _ptr(k), _ptr(sq), _ptr(sk),
                                              WEIGHTING[weighting], _ptr(out["loss_rows"]), g(out["dq"]), g(out["dk"]), g(out["dT"]),
                                              _ptr(ws), wsb, _stream())


def _ws_bytes(rows, cols, d):
    from aecf_amd import _lib
    wsb = _lib.load().aecf_supcon_ml_workspace_bytes(rows, cols, d)
    assert wsb == S.workspace_bytes_py(rows, cols, d)
    return wsb


def _run(q, k, off, sq, sk, weighting, T, fill=0xFF, short=0, grads=True):
    """one call on fresh guarded buffers: (status, outputs, workspace, guards)"""
    (rows, d), cols = q.shape, k.shape[0]
    wsb = _ws_bytes(rows, cols, d)
    gd = Guarded(DEV)
    out = _buffers(gd, rows, cols, d)
    ws = gd.new(wsb, fill)
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    status = _call(q, k, off, sq, sk, weighting, Tt, 1.0 / cols, out, ws, wsb - short, grads)
    torch.cuda.synchronize()
    return status, out, ws, gd


@functools.lru_cache(maxsize=None)
def _measured(cid, T, weighting):
    """One case at one temperature and weighting: the call on a 0xFF-filled workspace of exactly the documented size, the same
    call on a zero-filled one, a call with the size one byte short and a loss-only call -- run once, judged by the tests below."""
    args = _inputs(cid) + (weighting,)
    return dict(full=_run(*args, T), zero=_run(*args, T, fill=0), short=_run(*args, T, short=1), loss=_run(*args, T, grads=False))


def _ratios(out, ref, bnd):
    return C.ratios(dict(loss_rows=out["loss_rows"], dq=out["dq"], dk=out["dk"], dT=float(out["dT"])), ref, bnd)


@pytest.mark.parametrize("cid,T,weighting", CASE_T_W)
def test_outputs_inside_the_derived_bounds(cid, T, weighting):
    """loss_rows, dq, dk and d_temperature of every case, elementwise, at T = 0.07 and at T = 0.005, under both weightings; all
    finite, so every element was written (and no slot of an empty split was read); guards intact"""
    status, out, _, gd = _measured(cid, T, weighting)["full"]
    assert status == 0
    _, _, ref, bnd = _want(cid, T, weighting)
    r = _ratios(out, ref, bnd)
    sig = C.signal(ref, bnd)
    print(f"supcon_ml_parity case {cid} {weighting} T {T}: " + " ".join(f"{n}={r[n]:.3f}" for n in OUTPUTS)
          + " | value/bound " + " ".join(f"{n}={sig[n]:.3g}" for n in OUTPUTS))
    record_errors(f"supcon_ml_parity_{cid}_{weighting}", T=T, **r)
    gd.check()
    for n in OUTPUTS:
        assert bool(torch.isfinite(out[n]).all()), (cid, T, weighting, n)
        assert r[n] <= 1.0, (cid, T, weighting, n, r[n])


@pytest.mark.parametrize("cid,T,weighting", CASE_T_W)
def test_workspace_contents_do_not_matter(cid, T, weighting):
    """The same call on a zero-filled workspace: bit-identical outputs (fixed-order sums, nothing read before it is written)."""
    m = _measured(cid, T, weighting)
    status, again, _, gd = m["zero"]
    assert status == 0
    gd.check()
    for n in OUTPUTS:
        assert torch.equal(m["full"][1][n], again[n]), (cid, T, weighting, n)


@pytest.mark.parametrize("cid,T,weighting", CASE_T_W)
def test_workspace_one_byte_short_is_refused(cid, T, weighting):
    status, out, ws, gd = _measured(cid, T, weighting)["short"]
    assert status == ERR_WORKSPACE
    gd.check()
    for n in OUTPUTS:
        assert bool((out[n].view(torch.uint8) == 0xFF).all()), (cid, T, weighting, n)
    assert bool((ws == 0xFF).all())


@pytest.mark.parametrize("cid,T,weighting", CASE_T_W)
def test_loss_only_call_has_the_same_loss_bits(cid, T, weighting):
    """dq = dk = d_temperature = NULL: loss_rows as in the full call, nothing else touched"""
    m = _measured(cid, T, weighting)
    status, out, _, gd = m["loss"]
    assert status == 0
    gd.check()
    assert torch.equal(out["loss_rows"], m["full"][1]["loss_rows"])
    for n in ("dq", "dk", "dT"):
        assert bool((out[n].view(torch.uint8) == 0xFF).all()), (cid, T, weighting, n)


# ---- against the single-label kernels ----

def _run_single(q, k, off, lq, lk, T):
    """aecf_supcon_fwd_bwd on fresh guarded buffers (as tests/test_supcon_gpu.py calls it)"""
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    (rows, d), cols = q.shape, k.shape[0]
    lib = _lib.load()
    wsb = lib.aecf_supcon_workspace_bytes(rows, cols, d)
    gd = Guarded(DEV)
    out = _buffers(gd, rows, cols, d)
    ws = gd.new(wsb, 0xFF)
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    status = lib.aecf_supcon_fwd_bwd(rows, cols, off, d, _ptr(Tt), MIN_T, 1.0 / cols, _ptr(q), _ptr(k), _ptr(lq), _ptr(lk),
                                     _ptr(out["loss_rows"]), _ptr(out["dq"]), _ptr(out["dk"]), _ptr(out["dT"]), _ptr(ws), wsb, _stream())
    torch.cuda.synchronize()
    return status, out, gd


def _class_labels(cols, off, rows, seed):
    """one class in 0 .. 63 per key, about one key in five unlabeled (-1), class 63 and class 0 in use; lq = lk[off : off + rows]"""
    g = torch.Generator().manual_seed(seed)
    lk = torch.randint(0, 64, (cols,), generator=g)
    lk[torch.rand(cols, generator=g) < 0.2] = -1
    lk[off], lk[(off + rows) % cols] = 63, 63
    lk[0 if off else cols - 1] = 0
    lk = lk.to(DEV)
    return lk[off:off + rows].clone(), lk


@pytest.mark.parametrize("cid", ("C", "F"))
@pytest.mark.parametrize("T", S.TEMPS)
@pytest.mark.parametrize("weighting", S.WEIGHTINGS)
def test_one_hot_sets_give_the_bits_of_the_single_label_call(cid, T, weighting):
    """One class per row (classes < 64, -1 <-> the empty set): w is exactly 0 or 1, every product with it is exact and every sum
    is the single-label kernels' sum, so all four outputs of aecf_supcon_ml_fwd_bwd equal those of aecf_supcon_fwd_bwd bit for
    bit, under both weightings."""
    q, k, off, _, _ = _inputs(cid)
    lq, lk = _class_labels(k.shape[0], off, q.shape[0], 77)
    assert int((lk == 63).sum()) >= 2 and int((lk < 0).sum()) >= 1
    s1, one, g1 = _run_single(q, k, off, lq, lk, T)
    s2, ml, _, g2 = _run(q, k, off, S.one_hot_sets(lq), S.one_hot_sets(lk), weighting, T)
    assert s1 == 0 and s2 == 0
    g1.check()
    g2.check()
    for n in OUTPUTS:
        assert bool(torch.isfinite(ml[n]).all()) and torch.equal(ml[n], one[n]), (cid, T, weighting, n)


@pytest.mark.parametrize("weighting", S.WEIGHTINGS)
def test_all_empty_sets_give_the_bits_of_the_all_unlabeled_call(weighting):
    """Case C with every set empty against aecf_supcon_fwd_bwd with every label -1 (InfoNCE): the same bits.  Pairwise disjoint
    sets give them too: the first 64 local rows hold one class each, all 64 classes in use, and no other key holds any."""
    q, k, off, _, _ = _inputs("C")
    rows, cols = q.shape[0], k.shape[0]
    none = torch.full((cols,), -1, dtype=torch.int64, device=DEV)
    empty = torch.zeros(cols, dtype=torch.int64, device=DEV)
    disjoint = empty.clone()
    disjoint[off:off + 64] = torch.ones(64, dtype=torch.int64, device=DEV) << torch.arange(64, device=DEV)      # 64 rows, 64 classes
    for T in S.TEMPS:
        s1, one, g1 = _run_single(q, k, off, none[off:off + rows], none, T)
        s2, a, _, g2 = _run(q, k, off, empty[off:off + rows], empty, weighting, T)
        s3, b, _, g3 = _run(q, k, off, disjoint[off:off + rows], disjoint, weighting, T)
        assert s1 == 0 and s2 == 0 and s3 == 0
        for g in (g1, g2, g3):
            g.check()
        for n in OUTPUTS:
            assert torch.equal(a[n], one[n]) and torch.equal(b[n], one[n]), (weighting, T, n)


# ---- the packing kernel ----

@pytest.mark.parametrize("classes", (1, 15, 63, 64))
@pytest.mark.parametrize("dtype", (torch.bool, torch.uint8, torch.bfloat16, torch.float16, torch.float32), ids=str)
def test_label_sets_pack_matches_torch(classes, dtype):
    """aecf_label_sets_pack through the C ABI on a guarded output, and losses.pack_label_sets, against the torch restatement at
    1, 63, 64 and 65 rows: members at about 30 %, values that are not 1, -0.0 (no member) in the float kinds; the bits from
    `classes` up stay 0 and nothing outside the [rows] words is written"""
    from aecf_amd import _lib, losses
    from aecf_amd.layer import _ptr, _stream
    kind = {torch.bool: 3, torch.uint8: 3, torch.bfloat16: 0, torch.float16: 2, torch.float32: 1}[dtype]
    g = torch.Generator().manual_seed(classes)
    for rows in (1, 63, 64, 65):
        member = torch.rand(rows, classes, generator=g) < 0.3
        member[rows // 2] = True                                      # a full row: every class, the last one included
        member[0, :] = False                                          # an empty row
        if dtype == torch.bool:
            hot = member
        elif dtype == torch.uint8:
            hot = member.to(torch.uint8) * torch.randint(1, 256, (rows, classes), generator=g).to(torch.uint8)
        else:
            hot = torch.where(member, torch.randn(rows, classes, generator=g).abs() + 0.5, torch.tensor(-0.0)).to(dtype)
            hot = torch.where(member & (torch.rand(rows, classes, generator=g) < 0.5), -hot, hot)
        if rows == 1:
            hot = hot.clone()
            hot[0, classes - 1] = True if dtype == torch.bool else 1       # (the only row: give it the last class)
        hot = hot.to(DEV)
        want = S.pack_torch(hot)
        assert bool((want != 0).any())
        gd = Guarded(DEV)
        sets = gd.tensor((rows,), torch.int64, 0xFF)
        assert _lib.load().aecf_label_sets_pack(rows, classes, kind, _ptr(hot), _ptr(sets), _stream()) == 0
        torch.cuda.synchronize()
        gd.check()
        assert torch.equal(sets, want), (classes, dtype, rows)
        assert torch.equal(losses.pack_label_sets(hot), want)
        if classes == 64 and rows > 1:
            assert int(sets[rows // 2]) == -1                         # every class: class 63 is the sign bit


def test_temperature_below_the_minimum_is_clamped():
    """Case C with *T = 5e-4 < min_temperature = 1e-3: d_temperature == 0 exactly, every other output the bits of *T = 1e-3."""
    args = _inputs("C") + ("jaccard",)
    s1, low, _, g1 = _run(*args, 5e-4)
    s2, at, _, g2 = _run(*args, 1e-3)
    assert s1 == 0 and s2 == 0
    g1.check()
    g2.check()
    assert float(low["dT"]) == 0.0 and float(at["dT"]) != 0.0
    for n in ("loss_rows", "dq", "dk"):
        assert torch.equal(low[n], at[n]), n


# ---- the Python surface ----

@pytest.mark.parametrize("weighting", S.WEIGHTINGS)
def test_direction_function_at_a_row_offset(weighting):
    """_SupConMlDirection on case C (local rows 700 .. 764 of 2049 keys: what a data-parallel rank in the middle calls) at
    T = 0.02: the loss and the bf16 gradients on q and on k against float64, each inside its bound plus 2^-8 |value| for the
    rounding of the float32 result to bf16."""
    from aecf_amd.losses import _SupConMlDirection
    cid, T = "C", 0.02
    q0, k0, off, sq, sk = _inputs(cid)
    assert off > 0
    t, coef, ref, bnd = _want(cid, T, weighting)
    q, k = q0.clone().requires_grad_(True), k0.clone().requires_grad_(True)
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    loss = _SupConMlDirection.apply(q, k, sq, sk, WEIGHTING[weighting], off, Tt, coef, MIN_T, True)
    loss.backward()
    assert q.grad.dtype == torch.bfloat16 and k.grad.dtype == torch.bfloat16
    want_loss = coef * float(ref["loss_rows"].sum())
    # float32 sum of the rows (fewer than 2^4 roundings), one product
    assert abs(float(loss.detach()) - want_loss) <= coef * float(bnd["loss_rows"].sum()) + 2.0 ** -20 * abs(want_loss)
    r = {}
    for name, got in (("dq", q.grad), ("dk", k.grad)):
        got = got.double()
        r[name] = float(((got - ref[name]).abs() / (bnd[name] + 2.0 ** -8 * got.abs())).max())
    print(f"supcon_ml_parity case {cid} {weighting} T {T} (_SupConMlDirection, bf16 gradients): "
          + " ".join(f"{n}={v:.3f}" for n, v in r.items()))
    record_errors(f"supcon_ml_python_direction_{weighting}", T=T, **r)
    assert r["dq"] <= 1.0 and r["dk"] <= 1.0, r


@functools.lru_cache(maxsize=None)
def _batch(cid):
    """A batch that holds a case (built as _batch of tests/test_supcon_gpu.py builds its own): view b is the case's keys, rows
    off .. off + rows - 1 of view a are its queries and the other rows of view a lie at a cosine of about 0.25 to their partner;
    rows scaled by powers of two.  The sets of all n rows are the case's key sets: the plan of tests/supcon_ml_cases.py on every
    row."""
    (rows, n, off, d) = C.CASES[cid][0]
    case = C.make_case(cid)
    g = torch.Generator().manual_seed(4100)
    kb = case["k"].float()
    a = C._unit(0.25 * kb + 0.97 * C._unit(torch.randn(n, d, generator=g)))
    a[off:off + rows] = case["q"].float()
    scale = 2.0 ** torch.randint(-1, 3, (n, 1), generator=g).float()
    za = (a * scale).to(torch.bfloat16).to(DEV)
    zb = (kb * scale.flip(0)).to(torch.bfloat16).to(DEV)
    return za, zb, S.sets(cid)["sk"].to(DEV)


@pytest.mark.parametrize("weighting", S.WEIGHTINGS)
def test_multilabel_contrastive_tensor_temperature_low_minimum(weighting):
    """multilabel_contrastive(za, zb, sets, weighting, temperature = a device tensor holding 0.02, min_temperature = 1e-3) with
    case C inside a 2049-row batch, the sets given as a [b, 64] bool multi-hot tensor (packed by the kernel) and again as ready
    masks: the same bits.  Reference: float64 on the bf16 unit rows the kernels read, taken back through the documented
    normalise backward.  Bounds: each direction's dq / dk bound plus 2^-8 |value| for its rounding to bf16, the bf16 sum of the
    two contributions to a view (one more rounding), _after_normalise, and the rounding of the result.  Under torch.no_grad()
    the value has the same bits and the call's peak memory is strictly lower (no gradient buffers)."""
    from aecf_amd import losses
    T = 0.02
    za0, zb0, sets = _batch("C")
    n = za0.shape[0]
    hot = S.unpack(sets).bool()
    assert hot.shape == (n, 64) and bool(hot[:, 63].any()) and torch.equal(losses.pack_label_sets(hot), sets)
    za, zb = za0.clone().requires_grad_(True), zb0.clone().requires_grad_(True)
    Tt = torch.tensor(T, dtype=F32, device=DEV, requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        quiet = losses.multilabel_contrastive(za, zb, sets, weighting, temperature=Tt, min_temperature=MIN_T)
    torch.cuda.synchronize()
    peak_quiet = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = losses.multilabel_contrastive(za, zb, sets, weighting, temperature=Tt, min_temperature=MIN_T)
    torch.cuda.synchronize()
    peak_grad = torch.cuda.max_memory_allocated()
    loss.backward()
    assert torch.equal(quiet, loss.detach()) and not quiet.requires_grad
    print(f"supcon_ml peak memory: with gradients {peak_grad}, under no_grad {peak_quiet}")
    assert peak_quiet < peak_grad

    za2, zb2 = za0.clone().requires_grad_(True), zb0.clone().requires_grad_(True)
    T2 = torch.tensor(T, dtype=F32, device=DEV, requires_grad=True)
    again = losses.multilabel_contrastive(za2, zb2, hot, weighting, temperature=T2, min_temperature=MIN_T)
    again.backward()
    assert torch.equal(again.detach(), loss.detach()) and torch.equal(T2.grad, Tt.grad)
    assert torch.equal(za2.grad, za.grad) and torch.equal(zb2.grad, zb.grad)

    t, coef = C.used_temperature(T), 0.5 / n
    with torch.no_grad():
        na, nb = losses.l2_normalize(za.detach()), losses.l2_normalize(zb.detach())
    s32 = na.cpu().float() @ nb.cpu().float().T
    ex = C.eps_x(float((s32.double() - na.cpu().double() @ nb.cpu().double().T).abs().max()), t, n)
    w = S.weights(sets, sets, 0, weighting)
    ab, ba = S.reference(na, nb, w, t, coef), S.reference(nb, na, w, t, coef)
    b_ab, b_ba = S.bounds(ab, na, nb, t, coef, ex), S.bounds(ba, nb, na, t, coef, ex)
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
    print(f"supcon_ml_parity multilabel_contrastive {weighting} n {n} T {T}: " + " ".join(f"{k_}={v:.3f}" for k_, v in r.items())
          + f" | value/bound dT={abs(want_dt) / b_dt:.3g} " + " ".join(f"{k_}={v:.3g}" for k_, v in sig.items()))
    record_errors(f"supcon_ml_python_multilabel_contrastive_{weighting}", T=T, **r)
    assert all(v <= 1.0 for v in r.values()), r


def test_python_refuses_what_the_kernels_do_not_serve():
    from aecf_amd import losses
    sets = torch.zeros(64, dtype=torch.int64, device=DEV)
    for z in (torch.zeros(64, 192, dtype=torch.bfloat16, device=DEV), torch.zeros(64, 256, dtype=torch.float32, device=DEV)):
        with pytest.raises(NotImplementedError, match=r"128, 256, 384, 512, 768, 1024"):
            losses.multilabel_contrastive(z, z, sets)
    z = torch.zeros(64, 256, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="label sets"):
        losses.multilabel_contrastive(z, z, sets.cpu())
    with pytest.raises(ValueError, match="label sets"):
        losses.multilabel_contrastive(z, z, sets[:63])
    with pytest.raises(TypeError, match="int64"):
        losses.multilabel_contrastive(z, z, sets.to(torch.int32))
    with pytest.raises(NotImplementedError, match="at most 64 classes"):
        losses.multilabel_contrastive(z, z, torch.zeros(64, 80, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match="weighting"):
        losses.multilabel_contrastive(z, z, sets, "dice")


def test_fusion_objective_takes_the_multilabel_term():
    """fusion_objective(..., contrastive="multilabel", labels=sets, label_weighting=w) == task + multilabel_contrastive(...), bit
    for bit, for both weightings (which differ) and for a float32 multi-hot tensor of 15 classes"""
    from aecf_amd import losses
    za, zb, sets = _batch("D")
    task = torch.tensor(0.625, dtype=F32, device=DEV)
    terms = {}
    for w in S.WEIGHTINGS:
        got = losses.fusion_objective(task, None, None, za, zb, contrastive="multilabel", labels=sets, label_weighting=w, temperature=0.07)
        terms[w] = losses.multilabel_contrastive(za, zb, sets, w, temperature=0.07)
        assert torch.equal(got, task + terms[w])
    assert not torch.equal(terms["overlap"], terms["jaccard"])
    default = losses.fusion_objective(task, None, None, za, zb, contrastive="multilabel", labels=sets, temperature=0.07)
    assert torch.equal(default, task + terms["overlap"])
    hot15 = S.unpack(sets)[:, :15].float()
    got = losses.fusion_objective(task, None, None, za, zb, contrastive="multilabel", labels=hot15, label_weighting="jaccard", temperature=0.07)
    assert torch.equal(got, task + losses.multilabel_contrastive(za, zb, S.pack_torch(hot15), "jaccard", temperature=0.07))


def test_captured_step_reads_temperature_and_sets_at_replay():
    """forward + backward inside torch.cuda.graph on case D's batch, the sets a bool multi-hot tensor packed inside the captured
    step; new values written in place into the temperature tensor and the multi-hot tensor; the replay equals an eager call on
    the new values bit for bit (no host read anywhere)."""
    from aecf_amd import losses
    za, zb, sets = _batch("D")
    hot_new = S.unpack(sets).bool()
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    T = torch.tensor(0.07, dtype=F32, device=DEV, requires_grad=True)
    hot = torch.zeros_like(hot_new)

    def step():
        return losses.multilabel_contrastive(a, b, hot, "jaccard", temperature=T, min_temperature=MIN_T)

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
        hot.copy_(hot_new)
    graph.replay()
    torch.cuda.synchronize()
    got = (loss.detach().clone(), a.grad.clone(), b.grad.clone(), T.grad.clone())
    a2, b2 = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    T2 = torch.tensor(0.02, dtype=F32, device=DEV, requires_grad=True)
    want = losses.multilabel_contrastive(a2, b2, sets, "jaccard", temperature=T2, min_temperature=MIN_T)
    want.backward()
    plain = losses.multilabel_contrastive(za, zb, torch.zeros_like(sets), "jaccard", temperature=T2.detach(), min_temperature=MIN_T)
    assert not torch.equal(plain, want.detach())                  # the sets matter to the value the replay must reach
    assert torch.equal(got[0], want.detach())
    assert torch.equal(got[1], a2.grad) and torch.equal(got[2], b2.grad)
    assert torch.equal(got[3], T2.grad)
