"""CPU-only tests of what tests/test_supcon_ml_tile_gpu.py stands on (tests/supcon_ml_tile_cases.py): the four entry points of the
tile-GEMM multi-label contrastive loss load, their workspace query agrees with the documented layout, the set plan has the
properties its docstring names (read back from the words), the float64 one-block reference equals the sum of two streaming-form
reference directions, an emulation of the design's arithmetic stays inside the derived bounds at every case, weighting and
temperature, and the bounds have teeth -- the same emulation with one broken rule leaves them.  The refusals of the entry points
(order and codes) are host code too: the pointers handed over are bogus."""
import functools
import os

import pytest
import torch

from aecf_amd import _lib
from tests import nce_tile_cases as N
from tests import supcon_ml_cases as ML
from tests import supcon_ml_tile_cases as C

BAD = 0x10          # never dereferenced: every call that gets it must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4
NAMES = ("aecf_supcon_ml_sym_workspace_bytes", "aecf_supcon_ml_sym_pass1", "aecf_supcon_ml_sym_loss", "aecf_supcon_ml_sym_grads")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _want(cid, weighting, T):
    c = C.make_case(cid)
    t = C.used_temperature(T)
    ref, bnd = C.reference(c["a"], c["b"], c["sr"], c["sc"], weighting, c["shards"], t, c["coef"], C.score_error(cid))
    return t, ref, bnd


@functools.lru_cache(maxsize=None)
def _state(cid, T):
    c = C.make_case(cid)
    return N.emulate_pass1(c["a"], c["b"], c["shards"], C.used_temperature(T))


def _ratios(cid, weighting, T, mutation=None):
    c = C.make_case(cid)
    t, ref, bnd = _want(cid, weighting, T)
    out = C.emulate(c["a"], c["b"], c["sr"], c["sc"], weighting, c["shards"], t, c["coef"], mutation=mutation, state=_state(cid, T))
    out["db_sum"] = sum(x.double() for x in out["db"])
    r = C.ratios(out, ref, bnd)
    for name in r:                                               # (a row without any weight divides by zero: not a number is outside)
        vals = out[name] if isinstance(out[name], list) else [out[name]]
        if not all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in vals):
            r[name] = float("inf")
    return r


def test_symbols_are_declared_bound_and_exported(lib):
    assert lib.aecf_abi_version() == 10
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aecf_hip.h")).read()
    bound = {s[0] for s in _lib._SYMBOLS}
    for name in NAMES:
        assert getattr(lib, name) is not None and name in bound and name + "(" in header, name


def test_workspace_bytes_match_the_documented_layout(lib):
    for cid in C.CASE_IDS:
        (n, d), shards, _, _ = N.SYMMETRIC[cid]
        for lo, hi in shards:
            assert lib.aecf_supcon_ml_sym_workspace_bytes(hi - lo, n, d) == C.workspace_bytes_py(hi - lo, n, d), (cid, lo)
    assert lib.aecf_supcon_ml_sym_workspace_bytes(8192, 65536, 768) == C.workspace_bytes_py(8192, 65536, 768)
    assert lib.aecf_supcon_ml_sym_workspace_bytes(64, 64, 96) == 0
    assert lib.aecf_supcon_ml_sym_workspace_bytes(64, 2 ** 24 + 1, 64) == 0
    assert lib.aecf_supcon_ml_sym_workspace_bytes(64, 2 ** 24, 64) > 0
    assert lib.aecf_supcon_ml_sym_workspace_bytes(0, 64, 64) == 0


def test_set_plan_has_the_properties_it_names():
    """read back from the words: the weights are symmetric and dense, every twin pair carries a fractional Jaccard weight, the
    heavy set sits in every whole row tile of S4 (the tenth holds one row, a twin), some rows meet it in class 63 alone and the low-word twins above bit 31 only"""
    for cid in C.CASE_IDS:
        c = C.make_case(cid)
        n = c["sr"].shape[0]
        ov, ja = C.weights(c["sr"], c["sc"], "overlap"), C.weights(c["sr"], c["sc"], "jaccard")
        assert torch.equal(ov, ov.T) and torch.equal(ja, ja.T), cid
        assert bool(((ja > 0) == (ov > 0)).all()) and bool((ja <= 1).all())
        for rp, r in c["twins"]:
            assert float(ov[r, rp]) == 1.0 and float(ja[r, rp]) in (1.0 / 3.0, 0.5), (cid, rp, r)
        empty = [i for i in range(n) if int(c["sr"][i]) == 0]
        assert all(float(ov[i].sum()) == 1.0 for i in empty)                   # an empty set: the partner only
        if n >= 257:
            assert len(empty) >= n // 8                                      # (every 4th row, less those the plan overwrote)
            assert float((ov.sum(1) - 1).mean()) > 0.15 * n                    # dense: far from the sparse single-label case
    c = C.make_case("S4")
    heavy, sign, low = c["heavy"], c["sign"], c["low"]
    assert len(heavy) == 60 and {i // 256 for i in heavy} == set(range(9)) and len(low) == 6 and len(sign) > 20
    assert any(lo <= i < hi for i in heavy for lo, hi in c["shards"][1:])
    hw = ML.mask(C.HEAVY)
    assert hw < 0 and all(int(c["sr"][i]) == hw for i in heavy)
    for i in sign:
        both = int(c["sr"][i]) & hw
        assert ML.classes_of(both) == [63] and both & 0xFFFFFFFF == 0
    for i in low:
        w = int(c["sr"][i])
        assert (w & hw) & 0xFFFFFFFF == w & 0xFFFFFFFF == hw & 0xFFFFFFFF and ML.classes_of(w & hw) == [25]
    ja = C.weights(c["sr"], c["sc"], "jaccard")
    assert float(ja[heavy[0], sign[0]]) == 0.25 and float(ja[heavy[0], low[0]]) == 0.25
    m = C.make_case("S3m")
    assert ML.classes_of(int(m["sr"][2])) == list(C.S3M_SET) and int(m["sc"][2]) != int(m["sr"][2])
    assert float(C.weights(m["sr"], m["sc"], "overlap")[2].sum()) == 1.0         # no column holds it: the partner still counts


@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
@pytest.mark.parametrize("cid", C.ALL_IDS)
def test_one_block_reference_is_two_streaming_directions(cid, weighting):
    """loss rows, da, the summed db and dT of the one-block form against tests/supcon_ml_cases.reference run twice (a against b with
    the weight matrix, b against a with its transpose): float64 against float64, 1e-12 of the largest value or of 1"""
    c = C.make_case(cid)
    t = C.used_temperature(0.07)
    _, ref, _ = _want(cid, weighting, 0.07)
    two = C.two_directions(c["a"], c["b"], c["sr"], c["sc"], weighting, t, c["coef"])
    for name, got, want in (("loss_rows", ref["loss_rows"], two["loss_rows"]), ("da", ref["da"], two["da"]),
                            ("db", ref["db_sum"], two["db"])):
        assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0), (cid, name)
    assert abs(sum(ref["dT"]) - two["dT"]) <= 1e-12 * max(abs(two["dT"]), 1.0), cid


@pytest.mark.parametrize("T", C.TEMPS)
@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
@pytest.mark.parametrize("cid", C.ALL_IDS)
def test_emulation_sits_inside_the_bounds(cid, weighting, T):
    r = _ratios(cid, weighting, T)
    _, ref, bnd = _want(cid, weighting, T)
    sig = C.signal(ref, bnd)
    print(f"supcon_ml_tile emulation {cid} {weighting} T {T}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items())
          + " | value/bound " + " ".join(f"{k}={sig[k]:.3g}" for k in r))
    assert all(v <= 1.0 for v in r.values()), (cid, weighting, T, r)


def _boundary_positive(cid):
    """(row r, column r') of a twin pair whose r' is the first column of a column tile: a weighted positive on a tile boundary"""
    c = C.make_case(cid)
    for rp, r in c["twins"]:
        if rp % 256 == 0 and rp > 0:
            return r, rp
    raise AssertionError("no twin on a tile boundary")


# (rule, case, weighting, the outputs of which at least one must leave its bound)
MUTATIONS = [
    ("and32", "S4", "overlap", ("loss_rows", "colcnt")),          # the rows that meet the heavy set in class 63 lose it
    ("and32", "S4", "jaccard", ("loss_rows", "colcnt")),
    ("pop_lo", "S4", "jaccard", ("loss_rows", "colcnt")),         # the low-word twins weigh 1 for 1/4
    ("partner_by_sets", "S3", "overlap", ("loss_rows", "da", "db")),    # an empty row loses its only positive
    ("partner_by_sets", "S3m", "jaccard", ("loss_rows", "da", "db")),
    ("partner_twice", "S3", "overlap", ("loss_rows", "da", "db")),
    ("partner_twice", "S3", "jaccard", ("loss_rows", "da", "db")),
    ("row_lost", "S3", "jaccard", ("loss_rows", "da", "db")),
    ("col_lost", "S3", "jaccard", ("loss_rows", "da", "db", "colcnt", "colsx")),
    ("row_weight_sum", "S3m", "overlap", ("da", "db")),
    ("row_weight_sum", "S3m", "jaccard", ("da", "db")),
    ("union_inter", "S3", "overlap", ("loss_rows", "colcnt")),
    ("union_inter", "S3", "jaccard", ("loss_rows", "colcnt")),
]


@pytest.mark.parametrize("kind,cid,weighting,where", MUTATIONS, ids=[f"{m[0]}-{m[2]}" for m in MUTATIONS])
def test_broken_rules_leave_the_bounds(kind, cid, weighting, where):
    """each wrong rule, in the emulation, is outside the bounds (or not a number) on at least one of the outputs named"""
    T = 0.07
    mutation = (kind,) + _boundary_positive(cid) if kind in ("row_lost", "col_lost") else (kind,)
    r = _ratios(cid, weighting, T, mutation)
    print(f"supcon_ml_tile mutation {kind} on {cid} {weighting}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
    assert any(not (r[name] <= 1.0) for name in where), (kind, r)
    if kind == "row_lost":
        assert r["colcnt"] <= 1.0 and r["colsx"] <= 1.0         # (the column statistics still hold it)


def test_refusals_in_order(lib):
    """sizes, then the shape support and the weighting, then NULL pointers, then the workspace size -- before any pointer is read"""
    n, d, f = 300, 192, lib.aecf_supcon_ml_sym_workspace_bytes(300, 300, 192)
    p1 = lambda rows=n, cols=n, off=0, dd=d, t=BAD, mt=0.025, a=BAD, st=BAD, w=0, ws=BAD, wsb=f, cs=BAD: lib.aecf_supcon_ml_sym_pass1(
        rows, cols, off, dd, t, mt, a, BAD, st, BAD, w, ws, wsb, cs, None)
    assert p1(rows=0) == BAD_DIMS and p1(off=1) == BAD_DIMS and p1(mt=0.0) == BAD_DIMS and p1(cols=2 ** 31, dd=96) == BAD_DIMS
    assert p1(rows=0, w=7) == BAD_DIMS
    assert p1(dd=96, t=None) == UNSUPPORTED and p1(mt=0.0249, t=None) == UNSUPPORTED
    assert p1(rows=1, cols=2 ** 24 + 1, t=None) == UNSUPPORTED
    assert p1(w=2, t=None) == UNSUPPORTED and p1(w=-1, t=None, wsb=0) == UNSUPPORTED and p1(w=1, wsb=f - 1) == WORKSPACE
    assert p1(t=None, wsb=0) == NULL_POINTER and p1(st=None, wsb=0) == NULL_POINTER and p1(cs=None, wsb=0) == NULL_POINTER
    assert p1(wsb=f - 1) == WORKSPACE
    ls = lambda rows=n, dd=d, cs=BAD, wsb=f, lr=BAD: lib.aecf_supcon_ml_sym_loss(rows, n, 0, dd, BAD, 0.025, BAD, BAD, cs, BAD, wsb, lr, None)
    assert ls(rows=n + 1) == BAD_DIMS and ls(dd=96, cs=None) == UNSUPPORTED and ls(cs=None, wsb=0) == NULL_POINTER
    assert ls(lr=None, wsb=0) == NULL_POINTER and ls(wsb=f - 1) == WORKSPACE
    gr = lambda rows=n, dd=d, gdt=_lib.AECF_F32, st=BAD, w=1, da=BAD, wsb=f, up=None, dtp=None: lib.aecf_supcon_ml_sym_grads(
        rows, n, 0, dd, BAD, 0.025, 1.0, BAD, BAD, st, BAD, w, BAD, wsb, up, gdt, da, BAD, dtp, None)
    assert gr(rows=-1) == BAD_DIMS and gr(dd=96, da=None) == UNSUPPORTED and gr(gdt=_lib.AECF_F16, da=None) == UNSUPPORTED
    assert gr(w=2, da=None) == UNSUPPORTED
    assert gr(da=None, wsb=0) == NULL_POINTER and gr(st=None, wsb=0) == NULL_POINTER and gr(wsb=f - 1) == WORKSPACE
