"""The tile-GEMM form of the pooled multi-label contrastive loss (EPI_SETS_OV / EPI_SETS_JAC and their row-only SELF forms,
sup_pool_combine_kernel, the two set_weights_kernel variants and the reused kernels of aecf_nce_gemm.hip) against float64 at its
tile, shard and ragged edges, with weighted positives on every boundary the geometry names, through the C ABI with ctypes and
through pooled_multilabel_contrastive / fusion_objective.  Cases, the float64 reference and the derived elementwise bounds are those
of tests/supcon_ml_pool_tile_cases.py (tests/test_supcon_ml_pool_tile_cpu.py shows that the bounds hold an emulation of the
arithmetic and catch the wrong rules).

Every shard of a global n x n problem runs as a rank would: aecf_supcon_ml_pool_sym_pass1, the shards' col_stats added in float32
on the device (the all-reduce), aecf_supcon_ml_pool_sym_loss, aecf_supcon_ml_pool_sym_grads.  Every output and the workspace come
from the Guarded helper of tests/test_abi_guards_gpu.py, as in tests/test_supcon_pool_tile_gpu.py: guard bands on both sides that
must be untouched after the calls, the workspace exactly the documented size and filled with 0xFF (NaN as bf16 and as float32)
before pass 1, the outputs filled alike -- a finite output was written and read nothing that was not written first."""
import functools

import pytest
import torch

from tests import supcon_ml_cases as ML
from tests import supcon_ml_pool_tile_cases as C
from tests import supcon_ml_tile_cases as MT
from tests import supcon_pool_tile_cases as PT
from tests.helpers import record_errors
from tests.test_abi_guards_gpu import Guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
WEIGHTING = {"overlap": 0, "jaccard": 1}
CASE_W_T = [(cid, w, T) for cid in C.CASE_IDS for w in C.WEIGHTINGS for T in C.TEMPS]
HALF = 2.0 ** -8


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


def _run(cid, weighting, T, grad_dtype=F32, upstream=None, short=False, sets=None, blocks=False):
    """every shard as a rank runs it; outputs laid out as C.reference.  short: hand the first call a workspace size one byte short
    and return its status with the buffers it must not have touched.  sets: (sr, sc) in place of the case's.  blocks: also keep,
    per shard, a copy of the stored E blocks (X | Y | Z: the head of the workspace) as pass 1 left them."""
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
    held, stats, stored = [], [], []
    for lo, hi in c["shards"]:
        rows = hi - lo
        al, bl, sl = a[lo:hi].contiguous(), b[lo:hi].contiguous(), sr[lo:hi].contiguous()
        wsb = lib.aecf_supcon_ml_pool_sym_workspace_bytes(rows, n, d)
        assert wsb == C.workspace_bytes_py(rows, n, d)
        ws = gd.new(wsb, 0xFF)
        cs = gd.tensor((3, n), F32, 0xFF)
        if short:
            status = lib.aecf_supcon_ml_pool_sym_pass1(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(bl), _ptr(a), _ptr(b), _ptr(sl),
                                                       _ptr(sc), w, _ptr(ws), wsb - 1, _ptr(cs), _stream())
            torch.cuda.synchronize()
            gd.check()
            return status, ws, cs
        assert lib.aecf_supcon_ml_pool_sym_pass1(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(bl), _ptr(a), _ptr(b), _ptr(sl),
                                                 _ptr(sc), w, _ptr(ws), wsb, _ptr(cs), _stream()) == 0
        if blocks:
            g = C.N.geometry(rows, n, d)
            stored.append(ws[:3 * g["Rp"] * g["Cp"] * 2].clone().view(3, -1))
        held.append((al, bl, sl, ws, wsb))
        stats.append(cs)
    total = stats[0].clone()
    for cs in stats[1:]:
        total += cs                                              # the all-reduce: float32, rank order
    gdt = _lib.AECF_BF16 if grad_dtype == BF16 else _lib.AECF_F32
    lrows = gd.tensor((n,), F32, 0xFF)
    da_loc, db_loc = gd.tensor((n, d), grad_dtype, 0xFF), gd.tensor((n, d), grad_dtype, 0xFF)
    out = dict(colsum=[s[0] for s in stats], colw=[s[1] for s in stats], colwx=[s[2] for s in stats], loss_rows=lrows, da_loc=da_loc,
               db_loc=db_loc, da_all=[], db_all=[], dT=[])
    for (lo, hi), (al, bl, sl, ws, wsb) in zip(c["shards"], held):
        rows = hi - lo
        lr_s = gd.tensor((rows,), F32, 0xFF)
        o1, o2 = gd.tensor((rows, d), grad_dtype, 0xFF), gd.tensor((rows, d), grad_dtype, 0xFF)
        o3, o4 = gd.tensor((n, d), grad_dtype, 0xFF), gd.tensor((n, d), grad_dtype, 0xFF)
        d_t = gd.tensor((1,), F32, 0xFF)
        assert lib.aecf_supcon_ml_pool_sym_loss(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(b), _ptr(total), _ptr(ws), wsb,
                                                _ptr(lr_s), _stream()) == 0
        assert lib.aecf_supcon_ml_pool_sym_grads(rows, n, lo, d, _ptr(Tt), C.MIN_T, c["coef"], _ptr(al), _ptr(bl), _ptr(a), _ptr(b),
                                                 _ptr(sl), _ptr(sc), w, _ptr(ws), wsb, _ptr(up), gdt, _ptr(o1), _ptr(o2), _ptr(o3),
                                                 _ptr(o4), _ptr(d_t), _stream()) == 0
        torch.cuda.synchronize()
        lrows[lo:hi], da_loc[lo:hi], db_loc[lo:hi] = lr_s, o1, o2
        out["da_all"].append(o3)
        out["db_all"].append(o4)
        out["dT"].append(float(d_t))
    gd.check()
    if blocks:
        out["blocks"] = stored
    return out


@functools.lru_cache(maxsize=None)
def _measured(cid, weighting, T):
    return _run(cid, weighting, T)


def _tensors(out):
    for name, v in out.items():
        if name not in ("dT", "blocks"):
            for k, t in enumerate(v if isinstance(v, list) else [v]):
                yield f"{name}[{k}]", t


def _judge(label, cid, weighting, T, out, upstream=1.0, bf16=False):
    """print the line of the profile, record it, assert every output finite and every ratio <= 1 -- no element is skipped.  bf16:
    every gradient output was rounded once to bf16: 2^-8 (|value| + bound) joins its bound (for the shares added up: every
    share's)."""
    _, ref, bnd = _want(cid, weighting, T, upstream)
    got = {k: v for k, v in out.items() if k != "blocks"}
    for name, t in _tensors(out):
        assert bool(torch.isfinite(t).all()), (cid, weighting, T, name)
    for name in ("da_all", "db_all"):
        got[name + "_sum"] = sum(g.double() for g in out[name])   # the shares, added in float64 for the comparison
    if bf16:
        bnd = dict(bnd)
        for name in ("da_loc", "db_loc"):
            bnd[name] = bnd[name] + HALF * (ref[name].abs() + bnd[name])
        for name in ("da_all", "db_all"):
            bnd[name] = [b + HALF * (r.abs() + b) for r, b in zip(ref[name], bnd[name])]
            bnd[name + "_sum"] = sum(bnd[name])
    r = C.ratios(got, ref, bnd)
    assert set(r) == set(C.OUTPUTS)
    sig = C.signal(ref, bnd)
    print(f"supcon_ml_pool_tile_parity case {cid} {weighting} T {T}{label}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items())
          + " | value/bound " + " ".join(f"{n}={sig[n]:.3g}" for n in r))
    record_errors(f"supcon_ml_pool_tile_parity_{cid}_{weighting}", T=T, **r)
    for n, v in r.items():
        assert v <= 1.0, (cid, weighting, T, label, n, v)


@pytest.mark.parametrize("cid,weighting,T", CASE_W_T)
def test_inside_the_derived_bounds(cid, weighting, T):
    """every shard's col_stats (sums of E, of w, of w * raw score), the loss rows, the four gradients (the shares of the two
    gathered ones also added up against the summed bounds) and every shard's share of dT, float32 gradients"""
    _judge(" (float32 gradients)", cid, weighting, T, _measured(cid, weighting, T))


@pytest.mark.parametrize("cid,weighting,T", CASE_W_T)
def test_bf16_gradients_inside_the_bounds_and_the_float32_ones_rounded_once(cid, weighting, T):
    """every gradient output in bf16 lies within its bound plus its one rounding, and has the bits of the float32 output rounded
    to nearest even: where two products land on one output they were summed in float32 first.  The loss rows, col_stats and dT know
    no gradient dtype."""
    out, f32 = _run(cid, weighting, T, grad_dtype=BF16), _measured(cid, weighting, T)
    _judge(" (bf16 gradients)", cid, weighting, T, out, bf16=True)
    for (name, x), (_, y) in zip(_tensors(out), _tensors(f32)):
        if name.split("[")[0] in C.GRADS:
            assert x.dtype == BF16 and torch.equal(x, y.to(BF16)), (cid, weighting, T, name)
        else:
            assert torch.equal(x, y), (cid, weighting, T, name)
    assert out["dT"] == f32["dT"]


@pytest.mark.parametrize("cid,weighting", [("S2", "jaccard"), ("S3m", "overlap"), ("S4", "jaccard")])
def test_upstream_scalar_scales_the_gradients(cid, weighting):
    """an upstream of 0.375 in device memory: the gradients and dT within the bounds taken at coef * 0.375; the loss rows and
    col_stats have the bits of the call without it"""
    T = 0.07
    out, plain = _run(cid, weighting, T, upstream=0.375), _measured(cid, weighting, T)
    for (name, x), (_, y) in zip(_tensors(out), _tensors(plain)):
        if name.split("[")[0] in C.STATS + ("loss_rows",):
            assert torch.equal(x, y), (cid, name)
    _judge(" (upstream 0.375)", cid, weighting, T, out, upstream=0.375)
    assert not torch.equal(out["da_loc"], plain["da_loc"])


def _disjoint_sets(n):
    """pairwise disjoint sets: 64 rows spread over all of them carry one class each (class 63 among them), the rest are empty"""
    s = torch.zeros(n, dtype=torch.int64)
    for k in range(min(64, n)):
        s[(k * (n - 1)) // 63 if n > 64 else k] = ML.mask([k])
    return s.to(DEV)


@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
@pytest.mark.parametrize("sets", ["all_empty", "pairwise_disjoint"])
@pytest.mark.parametrize("cid", ["S2", "S3e", "S4"])
def test_without_shared_classes_every_output_has_the_bits_of_nt_xent(cid, sets, weighting):
    """every set empty (S3e is that case), and pairwise disjoint sets: the loss rows, the four gradients, dT and row 0 of col_stats
    are torch.equal to aecf_ntxent_sym_pass1 / _loss / _grads on the same rows, and so are the stored E blocks of Y and Z as pass 1
    leaves them; the weight sums and weighted sums are 0"""
    from tests import test_ntxent_tile_gpu as NT
    _lib, lib, _ptr, _stream = _libs()
    T = 0.07
    c = C.make_case(cid)
    a, b, _, _ = _inputs(cid)
    n, d = a.shape
    if sets == "all_empty":
        words = torch.zeros(n, dtype=torch.int64, device=DEV)
        if cid == "S3e":
            assert torch.equal(words, _inputs(cid)[2]) and torch.equal(words, _inputs(cid)[3])
    else:
        words = _disjoint_sets(n)
        assert int((words != 0).sum()) == min(64, n)
    out, want = _run(cid, weighting, T, sets=(words, words), blocks=True), NT._measured(C.base(cid), T)
    for k in range(len(out["colsum"])):
        assert torch.equal(out["colsum"][k], want["colsum"][k]), (cid, k)
        assert not bool(out["colw"][k].any()) and not bool(out["colwx"][k].any()), (cid, k)
        assert torch.equal(out["da_all"][k], want["da_all"][k]) and torch.equal(out["db_all"][k], want["db_all"][k]), (cid, k)
    for name in ("loss_rows", "da_loc", "db_loc"):
        assert torch.equal(out[name], want[name]), (cid, name)
    assert out["dT"] == want["dT"]
    # the stored blocks: NT-Xent's pass 1 on every shard, its workspace begins with the same three blocks
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    for k, (lo, hi) in enumerate(c["shards"]):
        rows = hi - lo
        al, bl = a[lo:hi].contiguous(), b[lo:hi].contiguous()
        wsb = lib.aecf_ntxent_sym_workspace_bytes(rows, n, d)
        ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)
        cs = torch.empty(n, dtype=F32, device=DEV)
        assert lib.aecf_ntxent_sym_pass1(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(bl), _ptr(a), _ptr(b), _ptr(ws), wsb, _ptr(cs),
                                         _stream()) == 0
        torch.cuda.synchronize()
        g = C.N.geometry(rows, n, d)
        theirs = ws[:3 * g["Rp"] * g["Cp"] * 2].view(3, -1)
        for q, name in enumerate("XYZ"):
            assert torch.equal(out["blocks"][k][q], theirs[q]), (cid, k, name)


@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
@pytest.mark.parametrize("cid", ["S2", "S3", "S4"])
def test_stored_blocks_of_y_and_z_have_the_bits_of_nt_xent_with_weights_present(cid, weighting):
    """the plan's dense weights change nothing in the E loop: the stored E blocks of Y and Z (and of X) after pass 1 have the bits of
    aecf_ntxent_sym_pass1's, the excluded key 0 in both"""
    _lib, lib, _ptr, _stream = _libs()
    T = 0.07
    c = C.make_case(cid)
    a, b, _, _ = _inputs(cid)
    n, d = a.shape
    out = _run(cid, weighting, T, blocks=True)
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    for k, (lo, hi) in enumerate(c["shards"]):
        rows = hi - lo
        al, bl = a[lo:hi].contiguous(), b[lo:hi].contiguous()
        wsb = lib.aecf_ntxent_sym_workspace_bytes(rows, n, d)
        ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=DEV)
        cs = torch.empty(n, dtype=F32, device=DEV)
        assert lib.aecf_ntxent_sym_pass1(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(bl), _ptr(a), _ptr(b), _ptr(ws), wsb, _ptr(cs),
                                         _stream()) == 0
        torch.cuda.synchronize()
        g = C.N.geometry(rows, n, d)
        theirs = ws[:3 * g["Rp"] * g["Cp"] * 2].view(3, -1)
        for q, name in enumerate("XYZ"):
            assert torch.equal(out["blocks"][k][q], theirs[q]), (cid, k, name)


@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
@pytest.mark.parametrize("cid", ["S2", "S3m", "S4"])
def test_col_stats_of_block_x_have_the_bits_of_the_cross_view_form(cid, weighting):
    """outside a rank's own range col_stats holds the column statistics of block X alone: the bits of aecf_supcon_ml_sym_pass1 on the
    same inputs, all three quantities; inside it block Z's sums of E were added and row 0 is larger"""
    from tests import test_supcon_ml_tile_gpu as XV
    T = 0.07
    c = C.make_case(cid)
    n = c["a"].shape[0]
    got, cross = _measured(cid, weighting, T), XV._measured(cid, weighting, T)
    for k, (lo, hi) in enumerate(c["shards"]):
        outside = torch.ones(n, dtype=torch.bool, device=DEV)
        outside[lo:hi] = False
        for mine, theirs in zip(C.STATS, ("colsum", "colcnt", "colsx")):
            assert torch.equal(got[mine][k][outside], cross[theirs][k][outside]), (cid, k, mine)
        if n > 1:
            assert bool((got["colsum"][k][lo:hi] > cross["colsum"][k][lo:hi]).all()), (cid, k)
        assert bool((got["colw"][k][lo:hi] >= cross["colcnt"][k][lo:hi]).all()), (cid, k)


@pytest.mark.parametrize("cid", ["S3", "S4"])
def test_one_hot_sets_are_the_single_label_pooled_form(cid):
    """one-hot sets (classes < 64, unlabeled = the empty set): under both weightings every output lies within the bounds of
    tests/supcon_pool_tile_cases.py against that module's reference on the matching int64 labels, and the column sums of E have
    the bits of aecf_supcon_pool_sym_pass1; the two weightings give the same bits as each other (a quotient 1 / 1 is exact)"""
    from tests import test_supcon_pool_tile_gpu as SP
    c = C.make_case(cid)
    a, b, _, _ = _inputs(cid)
    n = a.shape[0]
    lab = MT.one_hot_labels(n).to(DEV)
    words = ML.one_hot_sets(lab)
    for T in C.TEMPS:
        single = SP._run(cid, T, labels=lab)
        t = C.used_temperature(T)
        ref, bnd = PT.reference(a, b, lab, c["shards"], t, c["coef"], C.score_error(cid))
        runs = {}
        for weighting in C.WEIGHTINGS:
            out = runs[weighting] = _run(cid, weighting, T, sets=(words, words))
            for name, x in _tensors(out):
                assert bool(torch.isfinite(x).all()), (cid, weighting, T, name)
            got = dict(colsum=out["colsum"], colcnt=out["colw"], colsx=out["colwx"], loss_rows=out["loss_rows"], da_loc=out["da_loc"],
                       db_loc=out["db_loc"], da_all=out["da_all"], db_all=out["db_all"], dT=out["dT"])
            for name in ("da_all", "db_all"):
                got[name + "_sum"] = sum(g.double() for g in out[name])
            r = PT.ratios(got, ref, bnd)
            assert set(r) == set(PT.OUTPUTS)
            print(f"supcon_ml_pool_tile_parity one-hot {cid} {weighting} T {T}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
            assert all(v <= 1.0 for v in r.values()), (cid, weighting, T, r)
            for k in range(len(out["colsum"])):
                assert torch.equal(out["colsum"][k], single["colsum"][k]), (cid, weighting, T, k)
                assert torch.equal(out["colw"][k], single["colcnt"][k]), (cid, weighting, T, k)     # (integers: exact in any order)
        for (name, x), (_, y) in zip(_tensors(runs["overlap"]), _tensors(runs["jaccard"])):
            assert torch.equal(x, y), (cid, T, name)
        assert runs["overlap"]["dT"] == runs["jaccard"]["dT"]


def test_workspace_one_byte_short_is_refused_with_nothing_written():
    status, ws, cs = _run("S3", "jaccard", 0.07, short=True)
    assert status == -4
    assert bool((ws == 0xFF).all()) and bool((cs.view(torch.uint8) == 0xFF).all())


# ---- the Python surface ----

PY_T = 0.07


@functools.lru_cache(maxsize=None)
def _views(cid="S3"):
    """views whose normalised rows are a case's unit rows, scaled by powers of two (exact in bf16), and the case's sets"""
    c = C.make_case(cid)
    g = torch.Generator().manual_seed(5601)
    scale = 2.0 ** torch.randint(-1, 3, (c["a"].shape[0], 1), generator=g).float()
    return (c["a"].float() * scale).to(BF16).to(DEV), (c["b"].float() * scale.flip(0)).to(BF16).to(DEV), c["sc"].to(DEV)


def _call(weighting="jaccard", T=PY_T, tensor_t=True, task=None, cid="S3", sets=None, **more):
    """(loss, dza, dzb[, dT]) of one forward + backward of pooled_multilabel_contrastive (task: through fusion_objective on that
    task loss)"""
    from aecf_amd import losses
    za, zb, words = _views(cid)
    if sets is not None:
        words = sets
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    Tt = torch.tensor(T, dtype=F32, device=DEV, requires_grad=True) if tensor_t else T
    if task is not None:
        loss = losses.fusion_objective(task, None, None, a, b, temperature=Tt, contrastive="multilabel_pool", labels=words,
                                       label_weighting=weighting, **more)
    else:
        loss = losses.pooled_multilabel_contrastive(a, b, words, weighting, temperature=Tt, **more)
    loss.backward()
    torch.cuda.synchronize()
    return (loss.detach(), a.grad, b.grad) + ((Tt.grad,) if tensor_t else ())


def _equal(one, two):
    return len(one) == len(two) and all(torch.equal(x, y) for x, y in zip(one, two))


@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
@pytest.mark.parametrize("cid", ["S3", "S4"])
def test_python_surface_inside_the_bounds(cid, weighting):
    """pooled_multilabel_contrastive on one rank with a tensor temperature: the loss, the bf16 gradients of both views and dT
    against the float64 three-block reference on the unit rows the kernels read, taken back through the documented normalise
    backward.  On one rank a view's gradient is the bf16 sum of two bf16 outputs (its local and its gathered role): each bound plus
    2^-8 |value| for its rounding, 2^-8 of the absolute sum for the addition; then _after_normalise of tests/test_nce_stream_gpu.py
    and the rounding of the result.  Under torch.no_grad() the value has the same bits."""
    from aecf_amd import losses
    from tests.test_nce_stream_gpu import _after_normalise
    za, zb, words = _views(cid)
    n = za.shape[0]
    loss, dza, dzb, dT = _call(weighting, cid=cid)
    assert dza.dtype == BF16 and dzb.dtype == BF16
    with torch.no_grad():
        quiet = losses.pooled_multilabel_contrastive(za, zb, words, weighting, temperature=torch.tensor(PY_T, dtype=F32, device=DEV))
        na, nb = losses.l2_normalize(za), losses.l2_normalize(zb)
    assert torch.equal(quiet, loss) and not quiet.requires_grad
    t, coef = C.used_temperature(PY_T), 0.5 / n
    s_err = 0.0
    for x, y in ((na, nb), (na, na), (nb, nb)):
        x, y = x.cpu(), y.cpu()
        s_err = max(s_err, float(((x.float() @ y.float().T).double() - x.double() @ y.double().T).abs().max()))
    ref, bnd = C.reference(na, nb, words, words, weighting, [(0, n)], t, coef, s_err)
    want_loss = coef * float(ref["loss_rows"].sum())
    # the float32 sum of the rows (a tree: fewer than 2^4 roundings) and the product with coef
    b_loss = coef * float(bnd["loss_rows"].sum()) + 2.0 ** -19 * abs(want_loss)
    r = dict(loss=abs(float(loss) - want_loss) / b_loss,
             dT=abs(float(dT) - ref["dT"][0]) / (bnd["dT"][0] + 2.0 ** -23 * abs(ref["dT"][0])))
    for name, z, zn, loc, gathered, got in (("dza", za, na, "da_loc", "da_all", dza), ("dzb", zb, nb, "db_loc", "db_all", dzb)):
        terms = [(ref[loc], bnd[loc]), (ref[gathered][0], bnd[gathered][0])]
        g_ref = sum(v for v, _ in terms)
        e_sum = sum(b_ + HALF * (v.abs() + b_) for v, b_ in terms)              # each output rounded to bf16 once
        e_g = e_sum + HALF * (sum(v.abs() for v, _ in terms) + e_sum)           # one addition in bf16
        inv = 1.0 / z.double().norm(dim=1, keepdim=True)
        want, bound = _after_normalise(zn.double(), inv, g_ref, e_g)
        assert bool(torch.isfinite(got).all())
        r[name] = float(((got.double() - want).abs() / (bound + HALF * got.double().abs())).max())
    print(f"supcon_ml_pool_tile_parity pooled_multilabel_contrastive {cid} {weighting} T {PY_T}: "
          + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    record_errors(f"supcon_ml_pool_tile_python_{cid}_{weighting}", T=PY_T, **r)
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
def test_fusion_objective_and_multi_hot_sets_give_the_same_bits(weighting):
    """fusion_objective(contrastive="multilabel_pool") is task + pooled_multilabel_contrastive bit for bit, loss and gradients, with
    low_memory None or False, and ignores intra_view; a multi-hot bool input and the packed int64 masks give the same bits; a float
    and a tensor temperature too"""
    task = torch.tensor(0.25, dtype=F32, device=DEV)
    alone = _call(weighting)
    through = _call(weighting, task=task)
    assert torch.equal(through[0], task + alone[0]) and _equal(through[1:], alone[1:])
    assert _equal(_call(weighting, task=task, low_memory=False, intra_view=True), through)
    words = _views()[2]
    multi_hot = ML.unpack(words) != 0
    assert multi_hot.dtype == torch.bool and multi_hot.shape == (words.shape[0], 64)
    assert _equal(_call(weighting, sets=multi_hot), alone)
    assert _equal(_call(weighting, tensor_t=False), alone[:3])
    assert not _equal(_call("overlap" if weighting == "jaccard" else "jaccard"), alone)


def test_python_second_backward_raises():
    from aecf_amd import losses
    za, zb, words = _views()
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    loss = losses.pooled_multilabel_contrastive(a, b, words, "jaccard")
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="runs once per forward"):
        loss.backward()


def test_python_refuses_what_it_does_not_serve():
    from aecf_amd import losses
    za, zb, words = _views()
    with pytest.raises(NotImplementedError, match="bfloat16"):
        losses.pooled_multilabel_contrastive(za.float(), zb.float(), words)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        losses.pooled_multilabel_contrastive(za.half(), zb.half(), words)
    with pytest.raises(NotImplementedError, match=r"d % 64 == 0 with 64 <= d <= 4096 \(got d = 96\)"):
        losses.pooled_multilabel_contrastive(za[:, :96].contiguous(), zb[:, :96].contiguous(), words)
    with pytest.raises(NotImplementedError, match="min_temperature"):
        losses.pooled_multilabel_contrastive(za, zb, words, min_temperature=1e-3)
    with pytest.raises(ValueError, match="weighting"):
        losses.pooled_multilabel_contrastive(za, zb, words, "dice")
    with pytest.raises(ValueError, match="one set per local row"):
        losses.pooled_multilabel_contrastive(za, zb, words[:-1])
    with pytest.raises(TypeError, match="int64"):
        losses.pooled_multilabel_contrastive(za, zb, words.to(torch.int32))
    with pytest.raises(ValueError, match="equal shape"):
        losses.pooled_multilabel_contrastive(za, zb[:-1], words)
    with pytest.raises(NotImplementedError, match="no streaming form"):
        losses.fusion_objective(torch.zeros((), device=DEV), None, None, za, zb, contrastive="multilabel_pool", labels=words,
                                low_memory=True)


def test_captured_step_reads_temperature_and_sets_at_replay():
    """forward + backward inside torch.cuda.graph on one stream; new values written in place into the temperature tensor and the
    sets; the replay equals an eager call on the new values bit for bit (no host read anywhere)."""
    from aecf_amd import losses
    za, zb, sets = _views()
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    T = torch.tensor(0.07, dtype=F32, device=DEV, requires_grad=True)
    words = torch.zeros_like(sets)

    def step():
        return losses.pooled_multilabel_contrastive(a, b, words, "jaccard", temperature=T)

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
    want = _call("jaccard", T=0.04)
    plain = losses.pooled_multilabel_contrastive(za, zb, torch.zeros_like(sets), "jaccard", temperature=0.04)
    assert not torch.equal(plain, want[0])                        # the sets matter to the value the replay must reach
    assert _equal(got, want)
