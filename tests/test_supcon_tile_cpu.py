"""CPU-only tests of what tests/test_supcon_tile_gpu.py stands on (tests/supcon_tile_cases.py): the three entry points of the
tile-GEMM supervised contrastive loss load, their workspace query agrees with the documented layout, the float64 one-block
reference equals the sum of two streaming-form reference directions, an emulation of the design's arithmetic stays inside the
derived bounds, and the bounds have teeth -- the same emulation with one label positive lost, a 32-bit compare, unlabeled rows
taken as a class, the partner counted twice or a wrong count in a matched weight leaves them.  The refusals of the entry points
(order and codes) are host code too: the pointers handed over are bogus."""
import functools
import os

import pytest
import torch

from aecf_amd import _lib
from tests import nce_tile_cases as N
from tests import supcon_tile_cases as C

BAD = 0x10          # never dereferenced: every call that gets it must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _want(cid, T):
    c = C.make_case(cid)
    t = C.used_temperature(T)
    ref, bnd = C.reference(c["a"], c["b"], c["lr"], c["lc"], c["shards"], t, c["coef"], C.score_error(cid))
    return t, ref, bnd


@functools.lru_cache(maxsize=None)
def _state(cid, T):
    c = C.make_case(cid)
    return N.emulate_pass1(c["a"], c["b"], c["shards"], C.used_temperature(T))


def _ratios(cid, T, mutation=None):
    c = C.make_case(cid)
    t, ref, bnd = _want(cid, T)
    out = C.emulate(c["a"], c["b"], c["lr"], c["lc"], c["shards"], t, c["coef"], mutation=mutation, state=_state(cid, T))
    out["db_sum"] = sum(x.double() for x in out["db"])
    return C.ratios(out, ref, bnd)


def test_symbols_and_abi_version(lib):
    assert lib.aecf_abi_version() == 10
    for name in ("aecf_supcon_sym_workspace_bytes", "aecf_supcon_sym_pass1", "aecf_supcon_sym_loss", "aecf_supcon_sym_grads"):
        assert getattr(lib, name) is not None


def test_workspace_bytes_match_the_documented_layout(lib):
    for cid in C.CASE_IDS:
        (n, d), shards, _, _ = N.SYMMETRIC[cid]
        for lo, hi in shards:
            assert lib.aecf_supcon_sym_workspace_bytes(hi - lo, n, d) == C.workspace_bytes_py(hi - lo, n, d), (cid, lo)
    assert lib.aecf_supcon_sym_workspace_bytes(8192, 65536, 768) == C.workspace_bytes_py(8192, 65536, 768)
    assert lib.aecf_supcon_sym_workspace_bytes(64, 64, 96) == 0
    assert lib.aecf_supcon_sym_workspace_bytes(64, 2 ** 24 + 1, 64) == 0
    assert lib.aecf_supcon_sym_workspace_bytes(64, 2 ** 24, 64) > 0
    assert lib.aecf_supcon_sym_workspace_bytes(0, 64, 64) == 0


def test_label_plan_is_symmetric_and_dense_enough():
    for cid in C.CASE_IDS:
        c = C.make_case(cid)
        m = C.match_matrix(c["lr"], c["lc"])
        assert torch.equal(m, m.T), cid
        assert int(m.sum(1).max()) <= 61
        for rp, r in c["twins"]:
            assert bool(m[r, rp]) and bool(m[rp, r]), (cid, rp, r)
    c = C.make_case("S4")
    assert int(C.match_matrix(c["lr"], c["lc"]).sum(1).max()) == 60 and len(c["large"]) == 60
    neg = c["lr"][c["lr"] < 0]
    assert set(neg.tolist()) == {-1, -7}
    m = C.make_case("S3m")
    assert int(m["lr"][2]) != int(m["lc"][2]) and int(m["lr"][2]) > C.LARGE


@pytest.mark.parametrize("cid", C.ALL_IDS)
def test_one_block_reference_is_two_streaming_directions(cid):
    """loss rows, da, the summed db and dT of the one-block form against tests/supcon_cases.reference run twice (a against b with
    the match matrix, b against a with its transpose): float64 against float64, 1e-12 of the largest value or of 1"""
    c = C.make_case(cid)
    t = C.used_temperature(0.07)
    _, ref, _ = _want(cid, 0.07)
    two = C.two_directions(c["a"], c["b"], c["lr"], c["lc"], t, c["coef"])
    for name, got, want in (("loss_rows", ref["loss_rows"], two["loss_rows"]), ("da", ref["da"], two["da"]),
                            ("db", ref["db_sum"], two["db"])):
        assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0), (cid, name)
    assert abs(sum(ref["dT"]) - two["dT"]) <= 1e-12 * max(abs(two["dT"]), 1.0), cid


@pytest.mark.parametrize("T", C.TEMPS)
@pytest.mark.parametrize("cid", C.ALL_IDS)
def test_emulation_sits_inside_the_bounds(cid, T):
    r = _ratios(cid, T)
    print(f"supcon_tile emulation {cid} T {T}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), (cid, T, r)


def _boundary_positive(cid):
    """(row r, column r') of a twin pair whose r' is the first column of a column tile: a positive by label on a tile boundary"""
    c = C.make_case(cid)
    for rp, r in c["twins"]:
        if rp % 256 == 0 and rp > 0:
            return r, rp
    raise AssertionError("no twin on a tile boundary")


MUTATIONS = [
    ("row_lost", "S3", ("loss_rows", "da", "db")),       # (a pair of its own class: both positives score alike, the mean stays)
    ("col_lost", "S3", ("loss_rows", "da", "db", "colcnt", "colsx")),
    ("compare32", "S3", ("loss_rows", "colcnt")),
    ("unlabeled", "S3", ("loss_rows", "colcnt")),
    ("partner_twice", "S3", ("da", "db")),
    ("row_count", "S3m", ("da", "db")),
]


@pytest.mark.parametrize("kind,cid,where", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutations_leave_the_bounds(kind, cid, where):
    """each wrong rule, in the emulation, is outside the bounds on at least one of the outputs named"""
    T = 0.07
    mutation = (kind,) + _boundary_positive(cid) if kind in ("row_lost", "col_lost") else (kind,)
    r = _ratios(cid, T, mutation)
    print(f"supcon_tile mutation {kind} on {cid}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
    assert max(r[name] for name in where) > 1.0, (kind, r)
    if kind == "row_lost":
        assert r["colcnt"] == 0.0 and r["colsx"] <= 1.0         # (the column statistics still hold it)


def test_refusals_in_order(lib):
    """sizes, then the shape support, then NULL pointers, then the workspace size -- before any pointer is read"""
    n, d, f = 300, 192, lib.aecf_supcon_sym_workspace_bytes(300, 300, 192)
    p1 = lambda rows=n, cols=n, off=0, dd=d, t=BAD, mt=0.025, a=BAD, lab=BAD, ws=BAD, wsb=f, cs=BAD: lib.aecf_supcon_sym_pass1(
        rows, cols, off, dd, t, mt, a, BAD, lab, BAD, ws, wsb, cs, None)
    assert p1(rows=0) == BAD_DIMS and p1(off=1) == BAD_DIMS and p1(mt=0.0) == BAD_DIMS and p1(cols=2 ** 31, dd=96) == BAD_DIMS
    assert p1(dd=96, t=None) == UNSUPPORTED and p1(mt=0.0249, t=None) == UNSUPPORTED
    assert p1(rows=1, cols=2 ** 24 + 1, t=None) == UNSUPPORTED
    assert p1(t=None, wsb=0) == NULL_POINTER and p1(lab=None, wsb=0) == NULL_POINTER and p1(cs=None, wsb=0) == NULL_POINTER
    assert p1(wsb=f - 1) == WORKSPACE
    ls = lambda rows=n, dd=d, cs=BAD, wsb=f, lr=BAD: lib.aecf_supcon_sym_loss(rows, n, 0, dd, BAD, 0.025, BAD, BAD, cs, BAD, wsb, lr, None)
    assert ls(rows=n + 1) == BAD_DIMS and ls(dd=96, cs=None) == UNSUPPORTED and ls(cs=None, wsb=0) == NULL_POINTER
    assert ls(lr=None, wsb=0) == NULL_POINTER and ls(wsb=f - 1) == WORKSPACE
    gr = lambda rows=n, dd=d, gdt=_lib.AECF_F32, lab=BAD, da=BAD, wsb=f, up=None, dtp=None: lib.aecf_supcon_sym_grads(
        rows, n, 0, dd, BAD, 0.025, 1.0, BAD, BAD, lab, BAD, BAD, wsb, up, gdt, da, BAD, dtp, None)
    assert gr(rows=-1) == BAD_DIMS and gr(dd=96, da=None) == UNSUPPORTED and gr(gdt=_lib.AECF_F16, da=None) == UNSUPPORTED
    assert gr(da=None, wsb=0) == NULL_POINTER and gr(lab=None, wsb=0) == NULL_POINTER and gr(wsb=f - 1) == WORKSPACE
