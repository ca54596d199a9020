"""The tile-GEMM form of the symmetric multi-label contrastive loss (EPI_SETS_OV / EPI_SETS_JAC and set_weights_kernel of
aecf_nce_gemm.hip) against float64 at its tile, patch, shard and ragged edges, through the C ABI with ctypes and through
multilabel_contrastive.  Cases, class sets, the float64 reference and the derived elementwise bounds are those of
tests/supcon_ml_tile_cases.py (tests/test_supcon_ml_tile_cpu.py shows that the bounds hold an emulation of the arithmetic and catch
the broken weight rules).

Every shard of a global n x n problem runs as a rank would: aecf_supcon_ml_sym_pass1, the shards' column statistics added in
float32 on the device (the all-reduce), aecf_supcon_ml_sym_loss, aecf_supcon_ml_sym_grads.  Every output and the workspace come
from the Guarded helper of tests/test_abi_guards_gpu.py: the workspace is exactly the documented size and filled with 0xFF (NaN as
bf16 and as float32) before pass 1, the outputs are filled alike -- a finite output was written and read nothing that was not
written first."""
import functools

import pytest
import torch

from tests import nce_stream_cases as NS
from tests import supcon_ml_cases as ML
from tests import supcon_ml_tile_cases as C
from tests import supcon_tile_cases as ST
from tests.helpers import record_errors
from tests.test_abi_guards_gpu import Guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
WEIGHTING = {"overlap": 0, "jaccard": 1}
CASE_W_T = [(cid, w, T) for cid in C.ALL_IDS for w in C.WEIGHTINGS for T in C.TEMPS]


def _libs():
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = C.make_case(cid)
    return c["a"].to(DEV), c["b"].to(DEV), c["sr"].to(DEV), c["sc"].to(DEV)


@functools.lru_cache(maxsize=None)
def _want(cid, weighting, T, upstream=1.0):
    """(T as the kernels read it, float64 reference, bounds) at coef * upstream, computed once on the device"""
    c = C.make_case(cid)
    a, b, sr, sc = _inputs(cid)
    t = C.used_temperature(T)
    ref, bnd = C.reference(a, b, sr, sc, weighting, c["shards"], t, c["coef"] * upstream, C.score_error(cid))
    return t, ref, bnd


def _run(cid, weighting, T, grad_dtype=F32, upstream=None, poison=0xFF, sets=None, short=False):
    """every shard as a rank runs it; outputs laid out as C.reference.  sets: (sr, sc) in place of the case's.  short: hand the
    first call a workspace size one byte short and return its status with the buffers it must not have touched."""
    _lib, lib, _ptr, _stream = _libs()
    c = C.make_case(cid)
    a, b, sr, sc = _inputs(cid)
    if sets is not None:
        sr, sc = sets
    n, d = a.shape
    w = WEIGHTING[weighting]
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    up = None if upstream is None else torch.tensor([upstream], dtype=F32, device=DEV)
    gd = Guarded(DEV)
    held, stats = [], []
    for lo, hi in c["shards"]:
        rows = hi - lo
        al, sl = a[lo:hi].contiguous(), sr[lo:hi].contiguous()
        wsb = lib.aecf_supcon_ml_sym_workspace_bytes(rows, n, d)
        assert wsb == C.workspace_bytes_py(rows, n, d)
        ws = gd.new(wsb, poison)
        cs = gd.tensor((3, n), F32, 0xFF)
        if short:
            status = lib.aecf_supcon_ml_sym_pass1(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(b), _ptr(sl), _ptr(sc), w, _ptr(ws),
                                                  wsb - 1, _ptr(cs), _stream())
            torch.cuda.synchronize()
            gd.check()
            return status, ws, cs
        assert lib.aecf_supcon_ml_sym_pass1(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(b), _ptr(sl), _ptr(sc), w, _ptr(ws), wsb,
                                            _ptr(cs), _stream()) == 0
        held.append((al, sl, ws, wsb))
        stats.append(cs)
    total = stats[0].clone()
    for cs in stats[1:]:
        total += cs                                              # the all-reduce: float32, rank order
    gdt = _lib.AECF_BF16 if grad_dtype == BF16 else _lib.AECF_F32
    lrows, da = gd.tensor((n,), F32, 0xFF), gd.tensor((n, d), grad_dtype, 0xFF)
    out = dict(colsum=[s[0] for s in stats], colcnt=[s[1] for s in stats], colsx=[s[2] for s in stats], loss_rows=lrows, da=da,
               db=[], dT=[])
    for (lo, hi), (al, sl, ws, wsb) in zip(c["shards"], held):
        rows = hi - lo
        lr_s, da_s, db_s = gd.tensor((rows,), F32, 0xFF), gd.tensor((rows, d), grad_dtype, 0xFF), gd.tensor((n, d), grad_dtype, 0xFF)
        d_t = gd.tensor((1,), F32, 0xFF)
        assert lib.aecf_supcon_ml_sym_loss(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(b), _ptr(total), _ptr(ws), wsb,
                                           _ptr(lr_s), _stream()) == 0
        assert lib.aecf_supcon_ml_sym_grads(rows, n, lo, d, _ptr(Tt), C.MIN_T, c["coef"], _ptr(al), _ptr(b), _ptr(sl), _ptr(sc), w,
                                            _ptr(ws), wsb, _ptr(up), gdt, _ptr(da_s), _ptr(db_s), _ptr(d_t), _stream()) == 0
        torch.cuda.synchronize()
        lrows[lo:hi], da[lo:hi] = lr_s, da_s
        out["db"].append(db_s)
        out["dT"].append(float(d_t))
    gd.check()
    return out


@functools.lru_cache(maxsize=None)
def _measured(cid, weighting, T):
    return _run(cid, weighting, T)


def _tensors(out):
    for name, v in out.items():
        if name != "dT":
            for k, t in enumerate(v if isinstance(v, list) else [v]):
                yield f"{name}[{k}]", t


def _same_bits(one, two, what, names=None):
    for (name, x), (_, y) in zip(_tensors(one), _tensors(two)):
        if names is None or name.split("[")[0] in names:
            assert torch.equal(x, y), (what, name)
    if names is None or "dT" in names:
        assert one["dT"] == two["dT"], (what, one["dT"], two["dT"])


def _ratios(out, ref, bnd, bf16=False, cases=C):
    got = dict(out)
    if not bf16:
        got["db_sum"] = sum(g.double() for g in out["db"])
    r = cases.ratios(got, ref, bnd, bf16=bf16)
    if bf16:
        # a sum of shares rounded to bf16 one by one: every share's rounding joins the summed bounds
        total = sum(g.double() for g in out["db"])
        r["db_sum"] = float(((total - ref["db_sum"]).abs() / (bnd["db_sum"] + 2.0 ** -8 * sum(g.double().abs() for g in out["db"]))).max())
    return r


def _judge(label, cid, weighting, T, out, bf16=False, upstream=1.0):
    """print the line of the profile, record it, assert every ratio <= 1 and every output finite"""
    _, ref, bnd = _want(cid, weighting, T, upstream)
    for name, t in _tensors(out):
        assert bool(torch.isfinite(t).all()), (cid, weighting, T, name)
    r = _ratios(out, ref, bnd, bf16)
    sig = C.signal(ref, bnd)
    print(f"supcon_ml_tile_parity case {cid} {weighting} T {T}{label}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items())
          + " | value/bound " + " ".join(f"{n}={sig[n]:.3g}" for n in r))
    record_errors(f"supcon_ml_tile_parity_{cid}_{weighting}", T=T, **r)
    for n, v in r.items():
        assert v <= 1.0, (cid, weighting, T, label, n, v)


@pytest.mark.parametrize("cid,weighting,T", CASE_W_T)
def test_inside_the_derived_bounds(cid, weighting, T):
    """the three column statistics of every shard, loss rows, da, every shard's share of db and of dT, and the shares of db added
    up against the summed bounds, float32 gradients"""
    _judge(" (float32 gradients)", cid, weighting, T, _measured(cid, weighting, T))


@pytest.mark.parametrize("cid,weighting", [("S3m", "overlap"), ("S4", "jaccard")])
def test_bf16_gradients_and_an_upstream_scalar_inside_the_derived_bounds(cid, weighting):
    """bf16 gradient outputs and an upstream of 0.375 in device memory: the bounds at coef * 0.375 plus 2^-8 |value|; the loss
    rows and column statistics know no upstream"""
    T = 0.07
    out = _run(cid, weighting, T, grad_dtype=BF16, upstream=0.375)
    assert out["da"].dtype == BF16
    _same_bits(out, _measured(cid, weighting, T), (cid, weighting), names=("colsum", "colcnt", "colsx", "loss_rows"))
    _judge(" (bf16 gradients, upstream 0.375)", cid, weighting, T, out, bf16=True, upstream=0.375)


def _disjoint_sets(n):
    """pairwise disjoint sets: 64 rows spread over all of them carry one class each (class 63 among them), the rest are empty"""
    s = torch.zeros(n, dtype=torch.int64)
    for k in range(min(64, n)):
        s[(k * (n - 1)) // 63 if n > 64 else k] = ML.mask([k])
    return s.to(DEV)


@pytest.mark.parametrize("sets", ["all_empty", "pairwise_disjoint"])
@pytest.mark.parametrize("cid", ["S2", "S3", "S4"])
def test_without_shared_classes_it_is_symmetric_info_nce_bit_for_bit(cid, sets):
    """all sets empty, or pairwise disjoint: the column sums of E, loss rows, da, db and dT have the bits of aecf_nce_sym_pass1_dt /
    _loss_dt / _grads_dt on the same inputs under both weightings; no column has a weight"""
    from tests.test_nce_tile_gpu import _run_symmetric
    n = _inputs(cid)[0].shape[0]
    words = torch.zeros(n, dtype=torch.int64, device=DEV) if sets == "all_empty" else _disjoint_sets(n)
    if sets == "pairwise_disjoint":
        assert int((words != 0).sum()) == 64                     # all 64 classes, once each
    for T in C.TEMPS:
        want = _run_symmetric(cid, T, dt=True)
        for weighting in C.WEIGHTINGS:
            got = _run(cid, weighting, T, sets=(words, words))
            for k in range(len(want["colsum"])):
                assert torch.equal(got["colsum"][k], want["colsum"][k]), (cid, T, k)
                assert not bool(got["colcnt"][k].any()) and not bool(got["colsx"][k].any())
                assert torch.equal(got["db"][k], want["db"][k]), (cid, T, k)
            assert torch.equal(got["loss_rows"], want["loss_rows"]) and torch.equal(got["da"], want["da"]), (cid, T)
            assert got["dT"] == want["dT"], (cid, T)


@pytest.mark.parametrize("cid", ["S3", "S4"])
def test_one_hot_sets_are_the_single_label_tile_form(cid):
    """one-hot sets (classes < 64, unlabeled = the empty set): overlap and Jaccard give the same bits as each other; the column sums
    of E and of w have the bits of aecf_supcon_sym_pass1 on the matching int64 labels (the counts are exact in any order);
    everything else sits inside the bounds of tests/supcon_tile_cases.py -- widened by nothing: the two forms sum in orders of the
    same depth (16 + 2 + 2 and 8 + 4 + 1 inside a tile, then sup_sums_kernel)"""
    from tests.test_supcon_tile_gpu import _run as run_single
    c = C.make_case(cid)
    a, b, _, _ = _inputs(cid)
    n = a.shape[0]
    lab = C.one_hot_labels(n).to(DEV)
    words = ML.one_hot_sets(lab)
    for T in C.TEMPS:
        ov, ja = _run(cid, "overlap", T, sets=(words, words)), _run(cid, "jaccard", T, sets=(words, words))
        _same_bits(ov, ja, (cid, T))
        single = run_single(cid, T, labels=(lab, lab))
        _same_bits(ov, single, (cid, T), names=("colsum", "colcnt"))
        t = C.used_temperature(T)
        ref, bnd = ST.reference(a, b, lab, lab, c["shards"], t, c["coef"], C.score_error(cid))
        r = _ratios(ov, ref, bnd, cases=ST)
        print(f"supcon_ml_tile_parity one-hot {cid} T {T}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
        assert all(v <= 1.0 for v in r.values()), (cid, T, r)


@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
@pytest.mark.parametrize("cid", ["S2", "S4"])
def test_against_two_streaming_directions(cid, weighting):
    """aecf_supcon_ml_fwd_bwd twice on the whole block (a against b, b against a; d = 128 and 256, which it serves) against the tile
    form run shard by shard: loss rows, da, the summed db and dT differ by no more than the two forms' bounds added up"""
    from tests.test_supcon_ml_gpu import _run as run_stream
    c = C.make_case(cid)
    a, b, sr, sc = _inputs(cid)
    n = a.shape[0]
    T = 0.07
    t, _, bnd = _want(cid, weighting, T)
    tile = _measured(cid, weighting, T)
    st_ab, ab, _, g1 = run_stream(a, b, 0, sr, sc, weighting, T)
    st_ba, ba, _, g2 = run_stream(b, a, 0, sr, sc, weighting, T)
    assert st_ab == 0 and st_ba == 0
    g1.check(); g2.check()
    scale = c["coef"] * n                                        # (the streaming helper runs at coef = 1 / cols)
    ex = NS.eps_x(C.score_error(cid), t, n)
    sb = C.stream_bounds(a, b, sr, sc, weighting, t, c["coef"], ex)
    pairs = dict(loss_rows=(tile["loss_rows"].double(), ab["loss_rows"].double() + ba["loss_rows"].double(), bnd["loss_rows"] + sb["loss_rows"]),
                 da=(tile["da"].double(), scale * (ab["dq"].double() + ba["dk"].double()), bnd["da"] + sb["da"]),
                 db=(sum(g.double() for g in tile["db"]), scale * (ab["dk"].double() + ba["dq"].double()), bnd["db_sum"] + sb["db"]))
    r = {k: float(((x - y).abs() / e).max()) for k, (x, y, e) in pairs.items()}
    r["dT"] = abs(sum(tile["dT"]) - scale * (float(ab["dT"]) + float(ba["dT"]))) / (sum(bnd["dT"]) + sb["dT"])
    print(f"supcon_ml_tile_parity against streaming {cid} {weighting}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), (cid, weighting, r)


@pytest.mark.parametrize("cid,weighting", [("S2", "jaccard"), ("S4", "overlap")])
def test_zero_filled_workspace_gives_the_same_bits(cid, weighting):
    """nothing of the workspace is read before it is written: zeros in place of NaNs cannot move a bit"""
    _same_bits(_measured(cid, weighting, 0.07), _run(cid, weighting, 0.07, poison=0x00), cid)


def test_workspace_one_byte_short_is_refused_with_nothing_written():
    status, ws, cs = _run("S3", "jaccard", 0.07, short=True)
    assert status == -4
    assert bool((ws == 0xFF).all()) and bool((cs.view(torch.uint8) == 0xFF).all())


@pytest.mark.parametrize("cid,weighting", [("S2", "overlap"), ("S3", "jaccard")])
def test_temperature_below_the_minimum_is_clamped(cid, weighting):
    """*T = 0.01 < min_temperature = 0.025: dT is exactly 0, every other output has the bits of *T = 0.025"""
    low, at = _run(cid, weighting, 0.01), _run(cid, weighting, C.MIN_T)
    assert all(v == 0.0 for v in low["dT"]) and any(v != 0.0 for v in at["dT"])
    _same_bits(low, at, cid, names=("colsum", "colcnt", "colsx", "loss_rows", "da", "db"))


# ---- the Python surface ----

PY_T = 0.07


@functools.lru_cache(maxsize=None)
def _views(cid="S3"):
    """views whose normalised rows are a case's unit rows, scaled by powers of two (exact in bf16), and the case's sets.  S3
    (d = 192) is served by the tile form alone; S2 (d = 128) by both forms."""
    c = C.make_case(cid)
    g = torch.Generator().manual_seed(5401)
    scale = 2.0 ** torch.randint(-1, 3, (c["a"].shape[0], 1), generator=g).float()
    return (c["a"].float() * scale).to(BF16).to(DEV), (c["b"].float() * scale.flip(0)).to(BF16).to(DEV), c["sc"].to(DEV)


def _call(low_memory="default", weighting="jaccard", T=PY_T, through_objective=False, cid="S3"):
    """(loss, dza, dzb, dT) of one forward + backward of multilabel_contrastive on the views of a case"""
    from aecf_amd import losses
    za, zb, sets = _views(cid)
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    Tt = torch.tensor(T, dtype=F32, device=DEV, requires_grad=True)
    kw = {} if low_memory == "default" else dict(low_memory=low_memory)
    if through_objective:
        loss = losses.fusion_objective(torch.zeros((), dtype=F32, device=DEV), None, None, a, b, temperature=Tt,
                                       min_temperature=C.MIN_T, contrastive="multilabel", labels=sets, label_weighting=weighting, **kw)
    else:
        loss = losses.multilabel_contrastive(a, b, sets, weighting, temperature=Tt, min_temperature=C.MIN_T, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), a.grad, b.grad, Tt.grad


@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
def test_python_tile_form_inside_the_bounds(weighting):
    """multilabel_contrastive(low_memory=False) on case S3 with a tensor temperature: the loss, the bf16 gradients of both views and
    dT against the float64 one-block reference on the unit rows the kernels read, taken back through the documented normalise
    backward.  Bounds: the da / db bounds at coef = 0.5 / n plus 2^-8 |value| for each bf16 output, _after_normalise of
    tests/test_nce_stream_gpu.py, the rounding of the result.  na and nb are the library's own l2_normalize outputs."""
    from aecf_amd import losses
    from tests.test_nce_stream_gpu import _after_normalise
    za, zb, sets = _views()
    n = za.shape[0]
    loss, dza, dzb, dT = _call(False, weighting)
    assert dza.dtype == BF16 and dzb.dtype == BF16
    with torch.no_grad():
        na, nb = losses.l2_normalize(za), losses.l2_normalize(zb)
    t, coef, half = C.used_temperature(PY_T), 0.5 / n, 2.0 ** -8
    s_err = float((na.cpu().float() @ nb.cpu().float().T - na.cpu().double() @ nb.cpu().double().T).abs().max())
    ref, bnd = C.reference(na, nb, sets, sets, weighting, [(0, n)], t, coef, s_err)
    want_loss = coef * float(ref["loss_rows"].sum())
    # the float32 sum of the rows (a tree: fewer than 2^4 roundings) and the product with coef
    b_loss = coef * float(bnd["loss_rows"].sum()) + 2.0 ** -19 * abs(want_loss)
    r = dict(loss=abs(float(loss) - want_loss) / b_loss,
             dT=abs(float(dT) - ref["dT"][0]) / (bnd["dT"][0] + 2.0 ** -23 * abs(ref["dT"][0])))
    for name, z, zn, g_ref, b_g, got in (("dza", za, na, ref["da"], bnd["da"], dza), ("dzb", zb, nb, ref["db"][0], bnd["db"][0], dzb)):
        e_g = b_g + half * (g_ref.abs() + b_g)
        inv = 1.0 / z.double().norm(dim=1, keepdim=True)
        want, bound = _after_normalise(zn.double(), inv, g_ref, e_g)
        assert bool(torch.isfinite(got).all())
        r[name] = float(((got.double() - want).abs() / (bound + half * got.double().abs())).max())
    print(f"supcon_ml_tile_parity multilabel_contrastive(low_memory=False) S3 {weighting} T {PY_T}: "
          + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    record_errors(f"supcon_ml_tile_python_{weighting}", T=PY_T, **r)
    assert all(v <= 1.0 for v in r.values()), r


def _equal(one, two):
    return all(torch.equal(x, y) for x, y in zip(one, two))


def _parent_streaming(cid, weighting):
    """the function as it stood before the keyword: two _SupConMlDirection calls on the normalised views, one rank"""
    from aecf_amd import losses
    za, zb, sets = _views(cid)
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    Tt = torch.tensor(PY_T, dtype=F32, device=DEV, requires_grad=True)
    t = losses._temperature_arg(Tt, a, C.MIN_T)
    na, nb = losses.l2_normalize(a), losses.l2_normalize(b)
    coef, w = 0.5 / float(nb.shape[0]), losses.SET_WEIGHTINGS[weighting]
    loss = (losses._SupConMlDirection.apply(na, nb, sets, sets, w, 0, t, coef, float(C.MIN_T), True)
            + losses._SupConMlDirection.apply(nb, na, sets, sets, w, 0, t, coef, float(C.MIN_T), True))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), a.grad, b.grad, Tt.grad


def test_python_forms_are_chosen_as_documented():
    """True and the default are the streaming path with the bits it had before the keyword; None takes the tile form at d = 192,
    which the streaming form refuses (True raises there), and where both run; fusion_objective hands low_memory on"""
    from aecf_amd import losses
    tile3 = _call(False)
    assert _equal(_call(None), tile3)
    assert _equal(_call(False, through_objective=True), tile3)
    za, zb, sets = _views()
    for kw in (dict(), dict(low_memory=True)):
        with pytest.raises(NotImplementedError, match="d in"):   # (the streaming form does not serve d = 192)
            losses.multilabel_contrastive(za, zb, sets, "jaccard", **kw)
    with pytest.raises(NotImplementedError, match="d in"):       # (below the tile form's temperature bound nothing serves d = 192)
        losses.multilabel_contrastive(za, zb, sets, "jaccard", min_temperature=1e-3, low_memory=None)
    for weighting in C.WEIGHTINGS:
        tile, stream = _call(False, weighting, cid="S2"), _call(True, weighting, cid="S2")
        assert _equal(stream, _parent_streaming("S2", weighting))
        assert not _equal(tile, stream)                          # (two implementations: the bits differ)
        assert _equal(_call(None, weighting, cid="S2"), tile)
        assert _equal(_call("default", weighting, cid="S2"), stream)
        assert _equal(_call(False, weighting, through_objective=True, cid="S2"), tile)
        assert _equal(_call("default", weighting, through_objective=True, cid="S2"), stream)


def test_python_tile_form_refuses_what_it_does_not_serve():
    from aecf_amd import losses
    za, zb, sets = _views()
    with pytest.raises(NotImplementedError, match="bfloat16"):
        losses.multilabel_contrastive(za.float(), zb.float(), sets, low_memory=False)
    with pytest.raises(NotImplementedError, match=r"d % 64 == 0 with 64 <= d <= 4096 \(got d = 100\)"):
        losses.multilabel_contrastive(za[:, :100].contiguous(), zb[:, :100].contiguous(), sets, low_memory=False)
    with pytest.raises(NotImplementedError, match="min_temperature"):
        losses.multilabel_contrastive(za, zb, sets, min_temperature=1e-3, low_memory=False)
    with pytest.raises(ValueError, match="low_memory"):
        losses.multilabel_contrastive(za, zb, sets, low_memory="no")


def test_python_second_backward_raises():
    from aecf_amd import losses
    za, zb, sets = _views()
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    loss = losses.multilabel_contrastive(a, b, sets, "jaccard", low_memory=False)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="runs once per forward"):
        loss.backward()


def test_captured_step_reads_temperature_and_sets_at_replay():
    """forward + backward of the tile form inside torch.cuda.graph; new values written in place into the temperature tensor and the
    sets; the replay equals an eager call on the new values bit for bit (no host read anywhere)."""
    from aecf_amd import losses
    za, zb, sets = _views()
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    T = torch.tensor(0.07, dtype=F32, device=DEV, requires_grad=True)
    words = torch.zeros_like(sets)

    def step():
        return losses.multilabel_contrastive(a, b, words, "jaccard", temperature=T, low_memory=False)

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
        T.copy_(torch.tensor(0.04))
        words.copy_(sets)
    graph.replay()
    torch.cuda.synchronize()
    got = (loss.detach().clone(), a.grad.clone(), b.grad.clone(), T.grad.clone())
    want = _call(False, "jaccard", T=0.04)
    plain = losses.multilabel_contrastive(za, zb, torch.zeros_like(sets), "jaccard", temperature=0.04, low_memory=False)
    assert not torch.equal(plain, want[0])                        # the sets matter to the value the replay must reach
    assert _equal(got, want)
