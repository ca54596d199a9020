"""CPU-only tests of what tests/test_queue_supcon_gpu.py stands on (tests/queue_supcon_cases.py): the entry points of the supervised
contrastive loss with a key queue load, refuse in their documented order, and the workspace query agrees with the documented
layout; the Python surface checks its arguments; the float64 reference agrees with float64 autograd of the definition; the label
plans put what they promise on the slots; an emulation of the design's arithmetic stays inside the derived bounds on every case x
plan x temperature; and the bounds have teeth -- the same emulation with one broken rule leaves a named output's bound (the factor
is asserted above 1 and printed).  The refusals are host code: the pointers handed over are bogus."""
import functools
import math
import os
import re

import pytest
import torch

from aecf_amd import _lib
from tests import nce_tile_cases as N
from tests import queue_nce_cases as Q
from tests import queue_supcon_cases as C

BAD = 0x10          # never dereferenced: every call that gets it must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4
NAMES = ("aecf_supcon_queue_workspace_bytes", "aecf_supcon_queue_pass1", "aecf_supcon_queue_loss", "aecf_supcon_queue_grads",
         "aecf_key_queue_push_labeled")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _want(cid, pid, T, last_unlabeled=False):
    c = C.make_case(cid)
    qa, qb, ql, V = C.make_queue(cid, pid, None, last_unlabeled)
    t = C.used_temperature(T)
    ref, bnd = C.reference(c["a"], c["b"], c["y"], qa, qb, ql, V, c["shards"], t, c["coef"], C.score_error(c["a"], c["b"], qa, qb, V))
    return t, ref, bnd


def _ratios(cid, pid, T, mutation=None):
    c = C.make_case(cid)
    ring = mutation if mutation in ("label_order", "stale") else None
    last_unlabeled = mutation in ("stale", "stale_plan")        # "stale_plan": the unbroken ring on the plan "stale" is judged on
    t, ref, bnd = _want(cid, pid, T, last_unlabeled)
    qa, qb, ql, V = C.make_queue(cid, pid, ring, last_unlabeled)
    out = C.emulate(c["a"], c["b"], c["y"], qa, qb, ql, V, c["shards"], t, c["coef"],
                    mutation=None if ring or mutation == "stale_plan" else mutation)
    out["db_all_sum"] = sum(x.double() for x in out["db_all"])
    return C.ratios(out, ref, bnd)


def test_symbols_are_declared_bound_and_exported(lib):
    """the header's prototypes and the ctypes table agree on every new entry point: the same names, the same number of arguments"""
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aecf_hip.h")).read()
    bound = {s[0]: s for s in _lib._SYMBOLS}
    for name in NAMES:
        assert getattr(lib, name) is not None and name in bound and name + "(" in header, name
        proto = header[header.index(name + "("):]
        proto = re.sub(r"/\*.*?\*/", "", proto[proto.index("(") + 1:proto.index(");")], flags=re.S)
        args = proto.count(",") + 1                             # (the prototypes hold no nested parentheses)
        assert args == len(bound[name][2]), (name, args, len(bound[name][2]))


def test_workspace_bytes_match_the_documented_layout(lib):
    for cid in C.CASE_IDS:
        (n, d), shards, _, _ = N.SYMMETRIC[cid]
        for lo, hi in shards:
            for q_cap, _ in C.PLANS.values():
                assert lib.aecf_supcon_queue_workspace_bytes(hi - lo, n, q_cap, d) == C.workspace_bytes_py(hi - lo, n, q_cap, d), (cid, lo, q_cap)
    for q_cap in (8192, 65536):
        assert lib.aecf_supcon_queue_workspace_bytes(8192, 65536, q_cap, 768) == C.workspace_bytes_py(8192, 65536, q_cap, 768)
    assert lib.aecf_supcon_queue_workspace_bytes(64, 64, 65536, 256) == C.workspace_bytes_py(64, 64, 65536, 256)
    assert lib.aecf_supcon_queue_workspace_bytes(64, 64, 256, 96) == 0          # d % 64
    assert lib.aecf_supcon_queue_workspace_bytes(64, 64, 256, 4160) == 0        # d > 4096
    assert lib.aecf_supcon_queue_workspace_bytes(65, 64, 256, 64) == 0          # rows > cols
    assert lib.aecf_supcon_queue_workspace_bytes(64, 64, 0, 64) == 0            # no capacity
    assert lib.aecf_supcon_queue_workspace_bytes(64, 64, 2 ** 31, 64) == 0
    assert lib.aecf_supcon_queue_workspace_bytes(64, 64, 1, 64) > 0
    # the served bound on the counts: cols + q_cap <= 2^24, whichever of the two is large
    assert lib.aecf_supcon_queue_workspace_bytes(64, 64, 2 ** 24 - 64, 64) > 0
    assert lib.aecf_supcon_queue_workspace_bytes(64, 64, 2 ** 24 - 63, 64) == 0
    assert lib.aecf_supcon_queue_workspace_bytes(64, 2 ** 24 - 256, 256, 64) > 0
    assert lib.aecf_supcon_queue_workspace_bytes(64, 2 ** 24 - 255, 256, 64) == 0


def test_refusals_in_order(lib):
    """sizes, then the shape support, then NULL pointers, then the workspace size -- before any pointer is read"""
    n, d, q, f = 300, 192, 513, lib.aecf_supcon_queue_workspace_bytes(300, 300, 513, 192)
    p1 = lambda rows=n, cols=n, off=0, dd=d, t=BAD, mt=0.025, al=BAD, bl=BAD, qa=BAD, qb=BAD, qc=q, qv=BAD, ba=BAD, lr=BAD, lc=BAD, lq=BAD, \
        ws=BAD, wsb=f, cs=BAD: lib.aecf_supcon_queue_pass1(rows, cols, off, dd, t, mt, al, bl, qa, qb, qc, qv, ba, lr, lc, lq, ws, wsb, cs,
                                                           None)
    assert p1(rows=0) == BAD_DIMS and p1(off=1) == BAD_DIMS and p1(off=-1) == BAD_DIMS and p1(mt=0.0) == BAD_DIMS
    assert p1(cols=2 ** 31, dd=96) == BAD_DIMS and p1(rows=n + 1, t=None) == BAD_DIMS
    assert p1(qc=0, dd=96) == BAD_DIMS and p1(qc=2 ** 31, t=None) == BAD_DIMS
    assert p1(dd=96, t=None) == UNSUPPORTED and p1(mt=0.0249, t=None) == UNSUPPORTED and p1(dd=4160, t=None) == UNSUPPORTED
    assert p1(qc=2 ** 24 - n + 1, t=None) == UNSUPPORTED                 # cols + q_cap > 2^24
    for name in ("t", "al", "bl", "qa", "qb", "qv", "ba", "lr", "lc", "lq", "ws", "cs"):
        assert p1(wsb=0, **{name: None}) == NULL_POINTER, name
    assert p1(wsb=f - 1) == WORKSPACE
    ls = lambda rows=n, dd=d, t=BAD, al=BAD, ba=BAD, qc=q, cs=BAD, ws=BAD, wsb=f, lr=BAD: \
        lib.aecf_supcon_queue_loss(rows, n, 0, dd, t, 0.025, al, ba, qc, cs, ws, wsb, lr, None)
    assert ls(rows=n + 1) == BAD_DIMS and ls(qc=0) == BAD_DIMS and ls(dd=96, cs=None) == UNSUPPORTED
    assert ls(qc=2 ** 24, cs=None) == UNSUPPORTED
    for name in ("t", "al", "ba", "cs", "ws", "lr"):
        assert ls(wsb=0, **{name: None}) == NULL_POINTER, name
    assert ls(wsb=f - 1) == WORKSPACE
    gr = lambda rows=n, dd=d, gdt=_lib.AECF_F32, t=BAD, al=BAD, bl=BAD, qa=BAD, qb=BAD, qc=q, qv=BAD, ba=BAD, lr=BAD, lc=BAD, lq=BAD, ws=BAD, \
        wsb=f, up=None, o1=BAD, o2=BAD, o3=BAD, dtp=None: lib.aecf_supcon_queue_grads(
            rows, n, 0, dd, t, 0.025, 1.0, al, bl, qa, qb, qc, qv, ba, lr, lc, lq, ws, wsb, up, gdt, o1, o2, o3, dtp, None)
    assert gr(rows=-1) == BAD_DIMS and gr(dd=96, o1=None) == UNSUPPORTED and gr(gdt=_lib.AECF_F16, o1=None) == UNSUPPORTED
    for name in ("t", "al", "bl", "qa", "qb", "qv", "ba", "lr", "lc", "lq", "ws", "o1", "o2", "o3"):
        assert gr(wsb=0, **{name: None}) == NULL_POINTER, name
    assert gr(wsb=f - 1) == WORKSPACE                                    # (upstream and d_temperature may be NULL)
    push = lambda qc=q, dd=d, n_=4, sa=BAD, sb=BAD, sl=BAD, qa=BAD, qb=BAD, ql=BAD, st=BAD: \
        lib.aecf_key_queue_push_labeled(qc, dd, n_, sa, sb, sl, qa, qb, ql, st, None)
    assert push(qc=0) == BAD_DIMS and push(n_=-1) == BAD_DIMS and push(dd=0) == BAD_DIMS and push(qc=2 ** 31) == BAD_DIMS
    assert push(dd=12, st=None) == UNSUPPORTED
    for name in ("sa", "sb", "qa", "qb", "ql", "st"):                    # (the source labels may be NULL: -1 is written)
        assert push(**{name: None}) == NULL_POINTER, name


def test_python_argument_checks():
    from aecf_amd import losses
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.KeyQueue(16, 128, "cpu", labels=True)
    z = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.queued_supervised_contrastive(z, z, torch.zeros(4, dtype=torch.int64), None)
    t = torch.zeros(())
    with pytest.raises(ValueError, match="queue is taken by"):
        losses.fusion_objective(t, None, None, z, z, contrastive="info_nce", queue=object())
    with pytest.raises(ValueError, match="needs queue"):
        losses.fusion_objective(t, None, None, z, z, contrastive="queued")
    with pytest.raises(ValueError, match="needs labels"):
        losses.fusion_objective(t, None, None, z, z, contrastive="supervised_queued", queue=object())
    with pytest.raises(ValueError, match="labels are taken by"):
        losses.fusion_objective(t, None, None, z, z, contrastive="queued", queue=object(), labels=torch.zeros(4, dtype=torch.int64))


def test_labelled_ring_model():
    """the host model of the labelled ring: the labels go where the keys go (wrap, n > q_cap), a push without labels writes -1"""
    q_cap, d = 5, 8
    rows = lambda lo, hi: torch.arange(lo, hi, dtype=torch.float32)[:, None].expand(hi - lo, d).to(torch.bfloat16)
    labs = lambda lo, hi: torch.arange(lo, hi, dtype=torch.int64) * 10
    qa, qb, ql, st = torch.zeros(q_cap, d, dtype=torch.bfloat16), torch.zeros(q_cap, d, dtype=torch.bfloat16), \
        torch.full((q_cap,), -1, dtype=torch.int64), [0, 0]
    C.ring_push(qa, qb, ql, st, rows(1, 4), -rows(1, 4), labs(1, 4))
    assert st == [3, 3] and ql.tolist() == [10, 20, 30, -1, -1]
    C.ring_push(qa, qb, ql, st, rows(4, 8), -rows(4, 8), labs(4, 8))
    assert st == [2, 5] and qa[:, 0].tolist() == [6, 7, 3, 4, 5] and ql.tolist() == [60, 70, 30, 40, 50]
    C.ring_push(qa, qb, ql, st, rows(8, 10), -rows(8, 10), None)
    assert st == [4, 5] and qa[:, 0].tolist() == [6, 7, 8, 9, 5] and ql.tolist() == [60, 70, -1, -1, 50]
    C.ring_push(qa, qb, ql, st, rows(10, 22), -rows(10, 22), labs(10, 22))          # 12 rows into 5 slots: the last 5
    assert st == [1, 5] and qa[:, 0].tolist() == [21, 17, 18, 19, 20] and ql.tolist() == [210, 170, 180, 190, 200]


def test_plans_put_the_labels_where_they_are_promised():
    """every kind of label among the valid slots; the twin with a class its row does not carry and row r's label in front of it;
    live labels, the large class included, on the slots at or above V; Q4's labels where the ring leaves them"""
    for cid in C.CASE_IDS:
        c = C.make_case(cid)
        y, r = c["y"], Q.twin_row(cid)
        for pid in C.PLAN_IDS:
            qa, qb, ql, V = C.make_queue(cid, pid)
            q_cap = qa.shape[0]
            assert ql.shape == (q_cap,) and ql.dtype == torch.int64
            if V >= 2:
                slot = 89 if pid == "Q4" else V - 1
                assert torch.equal(qb[slot], c["b"][r]) and int(ql[slot]) != int(y[r]) and int(ql[slot]) >= 0, (cid, pid)
                assert int(ql[slot - 1]) == int(y[r]) and not torch.equal(qb[slot - 1], c["b"][r]), (cid, pid)
            if V >= 30:
                live = ql[:V]
                assert bool((live == C.LARGE).any()) and bool((live == -1).any()) and bool((live == -7).any())
                assert bool(((live > C.LARGE) & (live.to(torch.int32) == 0)).any())        # a distractor: equal in the low 32 bits
                assert bool(((live >= 0) & (live < C.batch_classes(y.shape[0]))).any())
            if V < q_cap and q_cap - V >= 2:
                above = ql[V:]
                assert bool((above == C.LARGE).any()) and bool((above >= 0).all())
    _, _, ql, _ = C.make_queue("S3", "Q4")
    lab = C.push_labels("S3")
    assert torch.equal(ql[:90], lab[2][40:]) and torch.equal(ql[90:130], lab[0][90:]) and torch.equal(ql[130:260], lab[1])
    _, _, ql, _ = C.make_queue("S3", "Q4", None, True)
    assert bool((ql[:90] == -1).all()) and bool((ql[260:] == -1).all()) and torch.equal(ql[130:260], lab[1])


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_reference_is_the_definition(cid):
    """``reference`` over one shard against float64 autograd of the definition written with explicit sets of positives (the
    partner by index, the batch keys and the valid slots by label), plans Q3 and Q4: float64 against float64"""
    c = C.make_case(cid)
    for pid in ("Q3", "Q4"):
        qa, qb, ql, V = C.make_queue(cid, pid)
        worst, dT = C.autograd_check(c["a"], c["b"], c["y"], qa, qb, ql, V, C.used_temperature(0.07), c["coef"])
        print(f"queue_supcon autograd check {cid} {pid}: loss and gradients {worst:.3g} dT {dT:.3g}")
        assert worst <= 1e-12 and dT <= 1e-10, (cid, pid, worst, dT)


@pytest.mark.parametrize("cid", ["S2", "S3"])
def test_reference_joins_its_two_neighbours(cid):
    """with an empty queue the reference is supcon_tile_cases' (loss rows and da), with every label negative queue_nce_cases'"""
    from tests import supcon_tile_cases as S
    c = C.make_case(cid)
    t = C.used_temperature(0.07)
    qa, qb, ql, V = C.make_queue(cid, "Q0")
    ref, _ = C.reference(c["a"], c["b"], c["y"], qa, qb, ql, V, c["shards"], t, c["coef"], 0.0)
    sup, _ = S.reference(c["a"], c["b"], c["y"], c["y"], c["shards"], t, c["coef"], 0.0)
    assert float((ref["loss_rows"] - sup["loss_rows"]).abs().max()) <= 1e-12 and float((ref["da_loc"] - sup["da"]).abs().max()) <= 1e-12
    qa, qb, ql, V = C.make_queue(cid, "Q3")
    none = torch.full_like(c["y"], -1)
    ref, _ = C.reference(c["a"], c["b"], none, qa, qb, torch.full_like(ql, -3), V, c["shards"], t, c["coef"], 0.0)
    nce, _ = Q.reference(c["a"], c["b"], qa, qb, V, c["shards"], t, c["coef"], 0.0)
    for name in ("loss_rows", "da_loc", "db_loc", "db_all_sum"):
        assert float((ref[name] - nce[name]).abs().max()) <= 1e-12, name


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
    print(f"queue_supcon emulation {cid}, largest error / bound over the plans and temperatures: "
          + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


# mutation -> where it is judged (a case with a shard at an offset for the rule about ranges, a wrapped ring for the ring's)
JUDGED = {"labels_ignored": ("S3", "Q3"), "one_direction": ("S3", "Q3"), "count_ignored": ("S3", "Q3"), "unlabeled": ("S3", "Q3"),
          "compare32": ("S3", "Q3"), "stats_local": ("S2", "Q2"), "twin_by_value": ("S3", "Q3"), "label_order": ("S3", "Q4"),
          "stale": ("S3", "Q4")}


@pytest.mark.parametrize("mutation", list(C.MUTATIONS))
def test_broken_rule_leaves_its_bound(mutation):
    cid, pid = JUDGED[mutation]
    name = C.MUTATIONS[mutation]
    T = 0.07
    good, bad = _ratios(cid, pid, T, "stale_plan" if mutation == "stale" else None), _ratios(cid, pid, T, mutation)
    factor = "no number" if math.isinf(bad[name]) else f"{bad[name]:.3g}"
    print(f"queue_supcon mutation {mutation} on {cid} {pid} T {T}: {name} leaves its bound by a factor of {factor} "
          f"(unbroken: {good[name]:.3f})")
    assert good[name] <= 1.0 and bad[name] > 1.0, (mutation, good[name], bad[name])
