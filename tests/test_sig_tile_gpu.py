"""The tile-GEMM sigmoid (SigLIP) loss (aecf_sig_pass1 / aecf_sig_grads) against float64 at its tile, patch, split and ragged
edges, through the C ABI with ctypes and once through losses.sigmoid_contrastive.  Cases, inputs, the float64 reference and the
derived elementwise bounds are those of tests/sig_tile_cases.py (tests/test_sig_tile_cpu.py shows that the bounds hold an
emulation of the arithmetic and catch a lost or doubled key, a padded row or column let in, a misplaced positive and a band
tile on the plain path).

Every output and the workspace come from the Guarded helper of tests/test_abi_guards_gpu.py: the workspace is exactly
aecf_sig_workspace_bytes long and filled with 0xFF (NaN as bf16 and as float32) before pass 1, the outputs are filled alike -- a
finite output was written and read nothing that was not written first (the padding of g, the slabs of an empty K split, the
tdot slots)."""
import functools
import math

import pytest
import torch

from tests import sig_tile_cases as C
from tests.helpers import record_errors
from tests.test_abi_guards_gpu import Guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
CASE_PARAMS = [(cid, T, bias) for cid in C.CASES for T, bias in C.PARAMS]
NAN_WORDS = 0x7FC07FC0                  # another poison: quiet NaNs as bf16 pairs and as float32


def _libs():
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = C.make_case(cid)
    return c["a"].to(DEV), c["b"].to(DEV)


@functools.lru_cache(maxsize=None)
def _want(cid, T, bias, upstream=1.0, shard=None):
    """(T and bias as the kernels read them, float64 reference, bounds) of a case or of its row shard [lo, hi) at coef * upstream,
    computed once on the device; the score error inside the bounds comes from torch's CPU products of the whole case"""
    c = C.make_case(cid)
    a, b = _inputs(cid)
    lo, hi = shard or (0, a.shape[0])
    t, bs = C.used_temperature(T), C.used_temperature(bias)
    ref, bnd = C.reference(a[lo:hi], b, c["off"] + lo, t, bs, c["coef"], upstream, C.score_error(cid))
    return t, bs, ref, bnd


def _run(a, b, off, T, bias, coef, poison=0xFF, upstreams=(None,), gdt=F32):
    """aecf_sig_pass1 once, then aecf_sig_grads once per entry of ``upstreams`` (None: no upstream pointer) on the same workspace.
    Returns the pass-1 outputs and one (da, db, dT) per upstream."""
    _lib, lib, _ptr, _stream = _libs()
    (rows, d), cols = a.shape, b.shape[0]
    a = a.contiguous()
    gd = Guarded(DEV)
    wsb = lib.aecf_sig_workspace_bytes(rows, cols, d)
    assert wsb == C.workspace_bytes_py(rows, cols, d)
    ws = gd.new(wsb, 0xFF)
    if poison != 0xFF:
        ws[:wsb // 4 * 4].view(torch.int32).fill_(poison)
    Tt, bt = torch.tensor([T], dtype=F32, device=DEV), torch.tensor([bias], dtype=F32, device=DEV)
    lr, dbias = gd.tensor((rows,), F32, 0xFF), gd.tensor((1,), F32, 0xFF)
    assert lib.aecf_sig_pass1(rows, cols, off, d, _ptr(Tt), C.MIN_T, _ptr(bt), _ptr(a), _ptr(b), _ptr(ws), wsb, _ptr(lr), _ptr(dbias),
                              _stream()) == 0
    out = dict(loss_rows=lr, dbias=dbias, grads=[])
    code = _lib.AECF_BF16 if gdt == BF16 else _lib.AECF_F32
    for up in upstreams:
        ut = None if up is None else torch.tensor([up], dtype=F32, device=DEV)
        da, db, d_t = gd.tensor((rows, d), gdt, 0xFF), gd.tensor((cols, d), gdt, 0xFF), gd.tensor((1,), F32, 0xFF)
        assert lib.aecf_sig_grads(rows, cols, off, d, _ptr(Tt), C.MIN_T, coef, _ptr(a), _ptr(b), _ptr(ws), wsb, _ptr(ut), code, _ptr(da),
                                  _ptr(db), _ptr(d_t), _stream()) == 0
        out["grads"].append(dict(da=da, db=db, dT=d_t))
    torch.cuda.synchronize()
    gd.check()
    return out


def _flat(out, k=0):
    """the five outputs of a run laid out as C.reference"""
    g = out["grads"][k]
    return dict(loss_rows=out["loss_rows"], dbias=float(out["dbias"]), dT=float(g["dT"]), da=g["da"], db=g["db"])


def _run_case(cid, T, bias, shard=None, **kw):
    c = C.make_case(cid)
    a, b = _inputs(cid)
    lo, hi = shard or (0, a.shape[0])
    return _run(a[lo:hi], b, c["off"] + lo, T, bias, c["coef"], **kw)


@functools.lru_cache(maxsize=None)
def _measured(cid, T, bias):
    return _run_case(cid, T, bias)


def _tensors(out):
    yield "loss_rows", out["loss_rows"]
    yield "dbias", out["dbias"]
    for k, g in enumerate(out["grads"]):
        for name in ("da", "db", "dT"):
            yield f"{name}[{k}]", g[name]


def _same_bits(one, two, what):
    for (name, x), (_, y) in zip(_tensors(one), _tensors(two)):
        assert bool(torch.isfinite(x.float()).all()), (what, name)
        assert torch.equal(x, y), (what, name)


def _judge(label, name, got, ref, bnd, bf16=False, **tags):
    """print the line of the profile, record it, assert every output finite and every ratio <= 1"""
    for n in ("loss_rows", "da", "db"):
        assert bool(torch.isfinite(got[n].float()).all()), (label, n)
    assert math.isfinite(got["dbias"]) and math.isfinite(got["dT"]), label
    r = C.ratios(got, ref, bnd, bf16=bf16)
    vb = C.value_over_bound(ref, bnd)
    print(f"sig_tile_parity {label}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items())
          + " | value/bound " + " ".join(f"{n}={vb[n]:.3g}" for n in r))
    record_errors(name, **tags, **r, **{f"value_{n}": vb[n] for n in r})
    assert set(r) == set(C.OUTPUTS)
    for n, v in r.items():
        assert v <= 1.0, (label, n, v)
    return r


@pytest.mark.parametrize("cid,T,bias", CASE_PARAMS)
def test_case_inside_the_derived_bounds(cid, T, bias):
    """loss rows, dbias, dT, da and db (float32) of every case at both parameter pairs, element by element"""
    _, _, ref, bnd = _want(cid, T, bias)
    _judge(f"case {cid} T {T} bias {bias}", f"sig_tile_parity_{cid}", _flat(_measured(cid, T, bias)), ref, bnd, T=T, bias=bias)


@pytest.mark.parametrize("cid", ["G4", "G6", "G7", "G8", "G9"])
def test_another_poison_and_a_second_run_give_the_same_bits(cid):
    """The same call on a workspace filled with other NaNs, and once more on the first poison: nothing is read before it is written
    (the padding of g, the slabs of G6's empty split, G7's one-step split, the tdot slots -- dT is among the outputs compared) and
    the reductions run in a fixed order, so the bits cannot move."""
    T, bias = C.PARAMS[0]
    one = _measured(cid, T, bias)
    _same_bits(one, _run_case(cid, T, bias, poison=NAN_WORDS), (cid, "poison"))
    _same_bits(one, _run_case(cid, T, bias), (cid, "second run"))


@pytest.mark.parametrize("cid", ["G4", "G8"])
def test_bf16_gradients_twice_over_one_logits_pass(cid):
    """aecf_sig_pass1 once, aecf_sig_grads twice on the same workspace with bf16 outputs and a device upstream of 1 and then of
    0.375: g is read and not modified, so the second run meets the bounds taken at coef * 0.375 plus 2^-8 |value| as the first
    meets those at coef.  G4: 3 splits, the slab sum rounds; G8: the SPLITX map."""
    T, bias = C.PARAMS[0]
    out = _run_case(cid, T, bias, upstreams=(1.0, 0.375), gdt=BF16)
    plain = _measured(cid, T, bias)
    assert torch.equal(out["loss_rows"], plain["loss_rows"]) and torch.equal(out["dbias"], plain["dbias"])
    for k, up in enumerate((1.0, 0.375)):
        assert out["grads"][k]["da"].dtype == BF16
        _, _, ref, bnd = _want(cid, T, bias, up)
        _judge(f"case {cid} T {T} bias {bias} (bf16 gradients, upstream {up}, call {k + 1} of 2)", f"sig_tile_bf16_{cid}", _flat(out, k),
               ref, bnd, bf16=True, T=T, bias=bias, upstream=up)
    # a float32 upstream of 1 and no upstream at all: the same float32 sums, the bits of the plain run once rounded
    assert torch.equal(out["grads"][0]["da"], plain["grads"][0]["da"].to(BF16))
    assert torch.equal(out["grads"][0]["dT"], plain["grads"][0]["dT"])


@pytest.mark.parametrize("cid,cut", [("G5", 256), ("G5", 700), ("G8", 129)])
def test_emulated_ranks(cid, cut):
    """Two row shards [0, cut) and [cut, rows), each run as a rank would with off = the case's offset + lo: every piece against the
    shard's own bounds; the concatenated loss rows and da and the added db, dbias and dT against the float64 of the WHOLE problem
    with the shards' bounds concatenated / added."""
    T, bias = C.PARAMS[0]
    rows = C.CASES[cid][0][0]
    shards = [(0, cut), (cut, rows)]
    _, _, whole, _ = _want(cid, T, bias)
    pieces, bounds = [], []
    for lo, hi in shards:
        got = _flat(_run_case(cid, T, bias, shard=(lo, hi)))
        _, _, ref, bnd = _want(cid, T, bias, shard=(lo, hi))
        _judge(f"case {cid} T {T} bias {bias} rows [{lo}, {hi})", f"sig_tile_shard_{cid}", got, ref, bnd, T=T, bias=bias, lo=lo, hi=hi)
        pieces.append(got)
        bounds.append(bnd)
    total = dict(loss_rows=torch.cat([p["loss_rows"] for p in pieces]), da=torch.cat([p["da"] for p in pieces]),
                 db=sum(p["db"].double() for p in pieces), dbias=sum(p["dbias"] for p in pieces), dT=sum(p["dT"] for p in pieces))
    bsum = dict(loss_rows=torch.cat([x["loss_rows"] for x in bounds]), da=torch.cat([x["da"] for x in bounds]),
                db=sum(x["db"] for x in bounds), dbias=sum(x["dbias"] for x in bounds), dT=sum(x["dT"] for x in bounds))
    _judge(f"case {cid} T {T} bias {bias} shards at {cut} put together", f"sig_tile_shards_{cid}", total, whole, bsum, T=T, bias=bias,
           cut=cut)


def test_saturated_logits_inside_the_derived_bounds():
    """T = 0.01 and bias 0 on the saturation case: positives and negatives whose n = l log2 e lies within 1 of +-126 on both sides
    of the clamp of sig_terms (asserted on the float64 scores), every output elementwise inside the bounds"""
    c = C.make_saturated()
    a, b = c["a"].to(DEV), c["b"].to(DEV)
    t, bs = C.used_temperature(C.SAT_T), C.SAT_BIAS
    n = (a.double() @ b.double().T) / t * C.LOG2E
    n = torch.stack([n[r, j] for r, j in c["marks"]])
    for lo, hi in ((125.0, 126.0), (126.0, 127.0), (-126.0, -125.0), (-127.0, -126.0)):
        assert int(((n > lo) & (n < hi)).sum()) >= 2, (lo, hi)
    ref, bnd = C.reference(a, b, c["off"], t, bs, c["coef"], 1.0, C.score_error_of(c["a"], c["b"]))
    got = _flat(_run(a, b, c["off"], C.SAT_T, C.SAT_BIAS, c["coef"]))
    _judge(f"saturated 48 x 300 d 128 T {C.SAT_T} bias {C.SAT_BIAS}", "sig_tile_saturated", got, ref, bnd, T=C.SAT_T, bias=C.SAT_BIAS)


def test_python_surface_takes_the_tile_form():
    """losses.sigmoid_contrastive on G4's keys as a square problem (its 300 queries at their rows 511 .. 810, seeded unit rows
    elsewhere): the loss against float64 on the library's own l2_normalize outputs, within coef times the summed bounds of the
    loss rows plus the float32 sum and product that form it (a tree sum of 1300 rows: fewer than 2^4 roundings; the product by
    float(coef): 2^-19 of the value in all).  The default takes the tile form: the bits of low_memory=False, which are
    float(coef) times the float32 sum of the loss rows aecf_sig_pass1 returns for the same rows."""
    from aecf_amd import losses
    T, bias = C.PARAMS[0]
    c = C.make_case("G4")
    rows, off, cols = c["a"].shape[0], c["off"], c["b"].shape[0]
    g = torch.Generator().manual_seed(7200)
    za = C._unit(torch.randn(cols, c["a"].shape[1], generator=g)).to(BF16)
    za[off:off + rows] = c["a"]
    za, zb = za.to(DEV), c["b"].to(DEV)
    Tt, bt = torch.tensor(T, device=DEV, requires_grad=True), torch.tensor(bias, device=DEV, requires_grad=True)

    def run(low_memory):
        x, y = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
        loss = losses.sigmoid_contrastive(x, y, temperature=Tt, bias=bt, low_memory=low_memory)
        loss.backward()
        return loss.detach(), x.grad, y.grad

    auto, tile = run(None), run(False)
    for x, y in zip(auto, tile):
        assert torch.equal(x, y)
    assert auto[1].dtype == BF16
    with torch.no_grad():
        na, nb = losses.l2_normalize(za), losses.l2_normalize(zb)
    coef = 1.0 / cols
    abi = _run(na, nb, 0, T, bias, coef)
    assert torch.equal(auto[0], abi["loss_rows"].sum() * coef)
    t, bs = C.used_temperature(T), C.used_temperature(bias)
    ref, bnd = C.reference(na, nb, 0, t, bs, coef, 1.0, C.score_error_of(na, nb))
    want = coef * float(ref["loss_rows"].sum())
    bound = coef * float(bnd["loss_rows"].sum()) + 2.0 ** -19 * abs(want)
    ratio = abs(float(auto[0]) - want) / bound
    print(f"sig_tile_parity sigmoid_contrastive {cols} x {cols} d {za.shape[1]} T {T} bias {bias}: loss={ratio:.3f} | value/bound "
          f"loss={abs(want) / bound:.3g}")
    record_errors("sig_tile_python_surface", T=T, bias=bias, loss=ratio)
    assert ratio <= 1.0, ratio
