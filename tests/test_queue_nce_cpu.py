"""CPU-only tests of what tests/test_queue_nce_gpu.py stands on (tests/queue_nce_cases.py): the entry points of the symmetric
InfoNCE with a key queue load, refuse in their documented order, and the workspace query agrees with the documented layout; the
Python surface checks its arguments; the float64 reference agrees with float64 autograd of the definition; an emulation of the
design's arithmetic stays inside the derived bounds on every case x plan x temperature; and the bounds have teeth -- the same
emulation with one broken rule leaves a named output's bound (the factor is asserted above 1 and printed).  The refusals are host
code: the pointers handed over are bogus."""
import functools
import os

import pytest
import torch

from aecf_amd import _lib
from tests import nce_tile_cases as N
from tests import queue_nce_cases as C

BAD = 0x10          # never dereferenced: every call that gets it must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4
NAMES = ("aecf_nce_queue_workspace_bytes", "aecf_nce_queue_pass1", "aecf_nce_queue_loss", "aecf_nce_queue_grads", "aecf_key_queue_push")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _want(cid, pid, T):
    c = C.make_case(cid)
    qa, qb, V = C.make_queue(cid, pid)
    t = C.used_temperature(T)
    ref, bnd = C.reference(c["a"], c["b"], qa, qb, V, c["shards"], t, c["coef"], C.score_error(c["a"], c["b"], qa, qb, V))
    return t, ref, bnd


def _ratios(cid, pid, T, mutation=None):
    c = C.make_case(cid)
    t, ref, bnd = _want(cid, pid, T)
    qa, qb, V = C.make_queue(cid, pid, "newest" if mutation == "newest" else None)
    order = None
    if mutation == "ring_order":
        q_cap = qa.shape[0]
        order = torch.tensor([(sum(C.Q4_PUSHES) + k) % q_cap for k in range(q_cap)])
    out = C.emulate(c["a"], c["b"], qa, qb, V, c["shards"], t, c["coef"], mutation=None if mutation == "newest" else mutation,
                    push_order=order)
    out["db_all_sum"] = sum(x.double() for x in out["db_all"])
    return C.ratios(out, ref, bnd)


def test_symbols_are_declared_bound_and_exported(lib):
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aecf_hip.h")).read()
    bound = {s[0] for s in _lib._SYMBOLS}
    for name in NAMES:
        assert getattr(lib, name) is not None and name in bound and name + "(" in header, name


def test_workspace_bytes_match_the_documented_layout(lib):
    for cid in C.CASE_IDS:
        (n, d), shards, _, _ = N.SYMMETRIC[cid]
        for lo, hi in shards:
            for q_cap, _ in C.PLANS.values():
                assert lib.aecf_nce_queue_workspace_bytes(hi - lo, n, q_cap, d) == C.workspace_bytes_py(hi - lo, n, q_cap, d), (cid, lo, q_cap)
    for q_cap in (8192, 65536):
        assert lib.aecf_nce_queue_workspace_bytes(8192, 65536, q_cap, 768) == C.workspace_bytes_py(8192, 65536, q_cap, 768)
    assert lib.aecf_nce_queue_workspace_bytes(64, 64, 65536, 256) == C.workspace_bytes_py(64, 64, 65536, 256)
    assert lib.aecf_nce_queue_workspace_bytes(64, 64, 256, 96) == 0          # d % 64
    assert lib.aecf_nce_queue_workspace_bytes(64, 64, 256, 4160) == 0        # d > 4096
    assert lib.aecf_nce_queue_workspace_bytes(65, 64, 256, 64) == 0          # rows > cols
    assert lib.aecf_nce_queue_workspace_bytes(64, 64, 0, 64) == 0            # no capacity
    assert lib.aecf_nce_queue_workspace_bytes(64, 64, 2 ** 31, 64) == 0
    assert lib.aecf_nce_queue_workspace_bytes(64, 64, 1, 64) > 0


def test_refusals_in_order(lib):
    """sizes, then the shape support, then NULL pointers, then the workspace size -- before any pointer is read"""
    n, d, q, f = 300, 192, 513, lib.aecf_nce_queue_workspace_bytes(300, 300, 513, 192)
    p1 = lambda rows=n, cols=n, off=0, dd=d, t=BAD, mt=0.025, al=BAD, bl=BAD, qa=BAD, qb=BAD, qc=q, qv=BAD, ba=BAD, ws=BAD, wsb=f, cs=BAD: \
        lib.aecf_nce_queue_pass1(rows, cols, off, dd, t, mt, al, bl, qa, qb, qc, qv, ba, ws, wsb, cs, None)
    assert p1(rows=0) == BAD_DIMS and p1(off=1) == BAD_DIMS and p1(off=-1) == BAD_DIMS and p1(mt=0.0) == BAD_DIMS
    assert p1(cols=2 ** 31, dd=96) == BAD_DIMS and p1(rows=n + 1, t=None) == BAD_DIMS
    assert p1(qc=0, dd=96) == BAD_DIMS and p1(qc=2 ** 31, t=None) == BAD_DIMS
    assert p1(dd=96, t=None) == UNSUPPORTED and p1(mt=0.0249, t=None) == UNSUPPORTED and p1(dd=4160, t=None) == UNSUPPORTED
    for name in ("t", "al", "bl", "qa", "qb", "qv", "ba", "ws", "cs"):
        assert p1(wsb=0, **{name: None}) == NULL_POINTER, name
    assert p1(wsb=f - 1) == WORKSPACE
    ls = lambda rows=n, dd=d, t=BAD, al=BAD, ba=BAD, qc=q, cs=BAD, ws=BAD, wsb=f, lr=BAD: \
        lib.aecf_nce_queue_loss(rows, n, 0, dd, t, 0.025, al, ba, qc, cs, ws, wsb, lr, None)
    assert ls(rows=n + 1) == BAD_DIMS and ls(qc=0) == BAD_DIMS and ls(dd=96, cs=None) == UNSUPPORTED
    for name in ("t", "al", "ba", "cs", "ws", "lr"):
        assert ls(wsb=0, **{name: None}) == NULL_POINTER, name
    assert ls(wsb=f - 1) == WORKSPACE
    gr = lambda rows=n, dd=d, gdt=_lib.AECF_F32, t=BAD, al=BAD, bl=BAD, qa=BAD, qb=BAD, qc=q, qv=BAD, ba=BAD, ws=BAD, wsb=f, up=None, \
        o1=BAD, o2=BAD, o3=BAD, dtp=None: lib.aecf_nce_queue_grads(rows, n, 0, dd, t, 0.025, 1.0, al, bl, qa, qb, qc, qv, ba, ws, wsb, up,
                                                                   gdt, o1, o2, o3, dtp, None)
    assert gr(rows=-1) == BAD_DIMS and gr(dd=96, o1=None) == UNSUPPORTED and gr(gdt=_lib.AECF_F16, o1=None) == UNSUPPORTED
    for name in ("t", "al", "bl", "qa", "qb", "qv", "ba", "ws", "o1", "o2", "o3"):
        assert gr(wsb=0, **{name: None}) == NULL_POINTER, name
    assert gr(wsb=f - 1) == WORKSPACE                                    # (upstream and d_temperature may be NULL)
    push = lambda qc=q, dd=d, n_=4, sa=BAD, sb=BAD, qa=BAD, qb=BAD, st=BAD: lib.aecf_key_queue_push(qc, dd, n_, sa, sb, qa, qb, st, None)
    assert push(qc=0) == BAD_DIMS and push(n_=-1) == BAD_DIMS and push(dd=0) == BAD_DIMS and push(qc=2 ** 31) == BAD_DIMS
    assert push(dd=12, st=None) == UNSUPPORTED
    for name in ("sa", "sb", "qa", "qb", "st"):
        assert push(**{name: None}) == NULL_POINTER, name


def test_python_argument_checks():
    from aecf_amd import losses
    with pytest.raises(ValueError, match="capacity"):
        losses.KeyQueue(0, 128, "cuda")
    with pytest.raises(ValueError, match="d % 8"):
        losses.KeyQueue(16, 12, "cuda")
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.KeyQueue(16, 128, "cpu")
    z = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.queued_info_nce(z, z, None)


def test_ring_model():
    """the host model of the ring: plain fills, the wrap of Q4's three pushes, n > q_cap, n = 0"""
    q_cap, d = 5, 8
    rows = lambda lo, hi: torch.arange(lo, hi, dtype=torch.float32)[:, None].expand(hi - lo, d).to(torch.bfloat16)
    qa, qb, st = torch.zeros(q_cap, d, dtype=torch.bfloat16), torch.zeros(q_cap, d, dtype=torch.bfloat16), [0, 0]
    C.ring_push(qa, qb, st, rows(1, 4), -rows(1, 4))
    assert st == [3, 3] and qa[:, 0].tolist() == [1, 2, 3, 0, 0]
    C.ring_push(qa, qb, st, rows(4, 8), -rows(4, 8))
    assert st == [2, 5] and qa[:, 0].tolist() == [6, 7, 3, 4, 5] and qb[:, 0].tolist() == [-6, -7, -3, -4, -5]
    C.ring_push(qa, qb, st, rows(8, 8), -rows(8, 8))
    assert st == [2, 5] and qa[:, 0].tolist() == [6, 7, 3, 4, 5]
    C.ring_push(qa, qb, st, rows(10, 22), -rows(10, 22))                    # 12 rows into 5 slots: the last 5, cursor 2 + 12 = 4 mod 5
    assert st == [4, 5] and qa[:, 0].tolist() == [18, 19, 20, 21, 17]
    qa, _, V = C.make_queue("S2", "Q4")
    src = C.push_sources("S2")
    assert V == 300 and torch.equal(qa[:90], src[2][0][40:]) and torch.equal(qa[90:130], src[0][0][90:]) and torch.equal(qa[130:260], src[1][0])


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_reference_is_the_definition(cid):
    """``reference`` over one shard against float64 autograd of the definition (logsumexp over [batch | queue keys] in both
    directions), plan Q3: float64 against float64"""
    c = C.make_case(cid)
    qa, qb, V = C.make_queue(cid, "Q3")
    worst, dT = C.autograd_check(c["a"], c["b"], qa, qb, V, C.used_temperature(0.07), c["coef"])
    print(f"queue_nce autograd check {cid}: loss and gradients {worst:.3g} dT {dT:.3g}")
    assert worst <= 1e-12 and dT <= 1e-10, (cid, worst, dT)


def test_plans_put_the_count_on_the_tile_edges():
    """Q3: one whole tile below V, ONE column in the crossed tile (the twin), a whole tile above V, a ragged capacity; the slots at
    or above V hold rows of 3e38 and unit rows; the twins are bit-identical to the partner keys"""
    assert C.PLANS["Q3"] == (513, 257) and C.PLANS["Q2"] == (256, 255) and C.PLANS["Q0"][1] == 0 and C.PLANS["Q1"] == (1, 1)
    for cid in C.CASE_IDS:
        c = C.make_case(cid)
        r = C.twin_row(cid)
        for pid in C.PLAN_IDS:
            qa, qb, V = C.make_queue(cid, pid)
            assert bool(torch.isfinite(qa.float()).all()) and bool(torch.isfinite(qb.float()).all())
            if pid != "Q4" and V < qa.shape[0]:
                assert float(qb[V:].float().abs().max()) > 1e38
            if V >= 2:
                slot = 89 if pid == "Q4" else V - 1
                assert torch.equal(qb[slot], c["b"][r]) and torch.equal(qa[slot], c["a"][r]), (cid, pid)


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_emulation_lies_inside_every_bound(cid):
    worst = {}
    for pid in C.PLAN_IDS:
        for T in C.TEMPS:
            r = _ratios(cid, pid, T)
            assert set(r) == set(C.OUTPUTS)
            for name, v in r.items():
                assert v <= 1.0, (cid, pid, T, name, v)
                worst[name] = max(worst.get(name, 0.0), v)
    print(f"queue_nce emulation {cid}, largest error / bound over the plans and temperatures: "
          + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


# mutation -> where it is judged (a case with a shard at an offset for the rules about ranges, a wrapped ring for the ring's)
JUDGED = {"one_direction": ("S2", "Q3"), "swapped": ("S3", "Q3"), "v_ignored": ("S3", "Q3"), "lw_local": ("S2", "Q2"),
          "by_value": ("S3", "Q3"), "ring_order": ("S3", "Q4"), "newest": ("S3", "Q4")}


@pytest.mark.parametrize("mutation", list(C.MUTATIONS))
def test_broken_rule_leaves_its_bound(mutation):
    cid, pid = JUDGED[mutation]
    name = C.MUTATIONS[mutation]
    T = 0.07
    good, bad = _ratios(cid, pid, T), _ratios(cid, pid, T, mutation)
    print(f"queue_nce mutation {mutation} on {cid} {pid} T {T}: {name} leaves its bound by a factor of {bad[name]:.3g} "
          f"(unbroken: {good[name]:.3f})")
    assert good[name] <= 1.0 and bad[name] > 1.0, (mutation, good[name], bad[name])
