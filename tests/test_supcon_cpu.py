"""CPU-only tests of the supervised contrastive loss: aecf_supcon_workspace_bytes / aecf_supcon_fwd_bwd are declared, bound and
exported with the ABI version still 10; the workspace is the documented size; every refusal comes back in the documented order
(sizes, width, NULL pointers, workspace size) before any pointer is read or any kernel is launched -- the pointers handed over
here are deliberately bogus; the Python surface rejects malformed labels and option combinations; and what
tests/test_supcon_gpu.py stands on (tests/supcon_cases.py) has teeth: an emulation of the design's arithmetic stays inside the
derived bounds, and the same emulation with the match rule broken in one of three ways leaves them by a factor of ten at least."""
import functools
import os
import re
import socket

import pytest
import torch

from aecf_amd import _lib
from tests import nce_stream_cases as C
from tests import supcon_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["aecf_supcon_workspace_bytes", "aecf_supcon_fwd_bwd"]
BAD = 0x10          # never dereferenced: every call below must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_supcon_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "aecf_hip.h")).read()
    declared = set(re.findall(r"\b(aecf_[a-z_0-9]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOL_NAMES
        assert hasattr(lib, name)
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10


def test_workspace_bytes_match_the_restatement(lib):
    need = lib.aecf_supcon_workspace_bytes
    assert need(333, 333, 100) == 0 and need(0, 333, 256) == 0 and need(333, 333, 2048) == 0
    for cid, ((rows, cols, _, d), _, _) in C.CASES.items():
        assert need(rows, cols, d) == S.workspace_bytes_py(rows, cols, d), cid
    assert need(8192, 65536, 768) == S.workspace_bytes_py(8192, 65536, 768)


def _call(lib, rows=256, cols=256, off=0, d=256, t=BAD, min_t=1e-3, q=BAD, k=BAD, lq=BAD, lk=BAD, lr=BAD, dq=BAD, dk=BAD, dt=BAD,
          ws=BAD, wsb=1 << 30):
    return lib.aecf_supcon_fwd_bwd(rows, cols, off, d, t, min_t, 1.0 / max(cols, 1), q, k, lq, lk, lr, dq, dk, dt, ws, wsb, None)


def test_fwd_bwd_refuses_in_the_documented_order(lib):
    # 1. sizes (with everything else wrong too)
    for bad in (dict(rows=0), dict(cols=0), dict(d=0), dict(min_t=0.0), dict(min_t=-1.0), dict(off=-1), dict(off=1),
                dict(rows=257)):
        kw = dict(d=100, t=None, lq=None, wsb=0)
        kw.update(bad)
        assert _call(lib, **kw) == BAD_DIMS, bad
    # 2. the width, before any pointer is looked at
    for d in (64, 100, 192, 2048):
        assert _call(lib, d=d, t=None, lk=None, wsb=0) == UNSUPPORTED, d
    # 3. NULL pointers: each of the required ones, the temperature and both label arrays included, and exactly one of dq / dk
    for name in ("t", "q", "k", "lq", "lk", "lr", "ws", "dq", "dk"):
        assert _call(lib, wsb=0, **{name: None}) == NULL_POINTER, name
    assert _call(lib, wsb=0, dq=None, dk=None) == NULL_POINTER              # a loss-only call takes no d_temperature
    # 4. then the workspace size: with gradients, without d_temperature, in the loss-only mode, and one byte short
    assert _call(lib, wsb=16) == WORKSPACE
    assert _call(lib, wsb=16, dt=None) == WORKSPACE
    assert _call(lib, wsb=16, dq=None, dk=None, dt=None) == WORKSPACE
    assert _call(lib, wsb=lib.aecf_supcon_workspace_bytes(256, 256, 256) - 1) == WORKSPACE


def test_python_rejects_malformed_labels():
    from aecf_amd.losses import _labels_arg
    z = torch.zeros(4, 128, dtype=torch.bfloat16)
    ok = torch.zeros(4, dtype=torch.int64)
    assert _labels_arg(ok, z) is ok
    assert _labels_arg(ok.to(torch.int32), z).dtype == torch.int32
    with pytest.raises(TypeError, match="labels"):
        _labels_arg(torch.zeros(4), z)                                       # a float dtype
    with pytest.raises(TypeError, match="labels"):
        _labels_arg([0, 1, 2, 3], z)
    with pytest.raises(ValueError, match="labels"):
        _labels_arg(torch.zeros(5, dtype=torch.int64), z)                    # wrong length
    with pytest.raises(ValueError, match="labels"):
        _labels_arg(torch.zeros(4, 1, dtype=torch.int64), z)
    with pytest.raises(ValueError, match="labels"):
        _labels_arg(torch.zeros(4, dtype=torch.int64, device="meta"), z)     # not where the embeddings live


def test_cpu_tensors_and_option_combinations_are_refused():
    from aecf_amd import losses
    z = torch.zeros(4, 128, dtype=torch.bfloat16)
    lab = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.supervised_contrastive(z, z, lab)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="supervised", labels=lab)
    with pytest.raises(ValueError, match="labels"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="supervised")
    with pytest.raises(ValueError, match="labels"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="info_nce", labels=lab)
    with pytest.raises(ValueError, match="contrastive"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="softmax")


# ---- the label plan, the bounds and their teeth ----

@functools.lru_cache(maxsize=None)
def _setup(cid, T):
    c = C.make_case(S.base(cid))
    L = S.labels(cid)
    q, k, off = c["q"], c["k"], c["off"]
    M = S.match_matrix(L["lq"], L["lk"], off)
    t, coef = C.used_temperature(T), 1.0 / k.shape[0]
    ref = S.reference(q, k, M, t, coef)
    bnd = S.bounds(ref, q, k, M, t, coef, C.eps_x(C.score_error(S.base(cid)), t, k.shape[0]))
    return q, k, off, L, M, t, coef, S.slim(ref), bnd


@pytest.mark.parametrize("cid", S.CASE_IDS)
def test_label_plan_keeps_the_table_loud(cid):
    """every case but A has a row with several positives; C-H have an unlabeled row and a row of the large class; the large class
    and the distractor classes agree in their low 32 bits and nowhere else; a sentinel column carries its row's class"""
    L = S.labels(cid)
    c = C.make_case(S.base(cid))
    off = c["off"]
    n = S.match_matrix(L["lq"], L["lk"], off).sum(dim=1)
    assert int(n.min()) >= 1
    if cid != "A":
        assert int((n > 1).sum()) >= 1
    if cid not in ("A", "B"):
        assert int((L["lq"] < 0).sum()) >= 1 and int((L["lq"] == S.LARGE).sum()) == 1
        assert 1 <= len(L["large"]) <= 60 and len(L["distract"]) >= 1
        for j in L["distract"]:
            v = int(L["lk"][j])
            assert v != S.LARGE and (v & 0xFFFFFFFF) == (S.LARGE & 0xFFFFFFFF)
            assert cid == "C9" or not bool((L["lq"] == v).any())              # no row owns a distractor class
    for j, r in c["sentinels"]:
        assert int(L["lk"][j]) == int(L["lk"][off + r]) >= 0
    if cid == "C9":
        assert int(L["lq"][2]) != int(L["lk"][off + 2]) and int(n[2]) > 1 and bool(S.match_matrix(L["lq"], L["lk"], off)[2, off + 2])


@pytest.mark.parametrize("cid", S.CASE_IDS)
def test_bounds_hold_the_emulation_and_catch_a_broken_match_rule(cid):
    for T in S.TEMPS:
        q, k, off, L, M, t, coef, ref, bnd = _setup(cid, T)
        intact = C.ratios(S.emulate(q, k, M, t, coef), ref, bnd)
        print(f"supcon emulation {cid} T={T}: " + " ".join(f"{n}={v:.3f}" for n, v in intact.items()))
        assert all(v <= 1.0 for v in intact.values()), (cid, T, intact)
        sent = C.make_case(S.base(cid))["sentinels"]
        if sent:                                                # 1. a lost positive at a sentinel column: dk of that column
            j, r = sent[0]
            bad = M.clone()
            bad[r, j] = False
            over = C.ratios(S.emulate(q, k, bad, t, coef), ref, bnd)
            print(f"  lost positive ({r}, {j}): " + " ".join(f"{n}={v:.0f}" for n, v in over.items()))
            assert over["dk"] >= 10.0, (cid, T, over)
        if cid not in ("A", "B"):
            jd = L["distract"][0]                               # 2. the 32-bit compare: row 1 (2^40) takes a distractor key
            assert not bool(M[1, jd]) and (int(L["lq"][1]) & 0xFFFFFFFF) == (int(L["lk"][jd]) & 0xFFFFFFFF)
            bad = M.clone()
            bad[1, jd] = True
            over = C.ratios(S.emulate(q, k, bad, t, coef), ref, bnd)
            print(f"  32-bit compare (1, {jd}): " + " ".join(f"{n}={v:.0f}" for n, v in over.items()))
            assert over["dk"] >= 10.0, (cid, T, over)
            i = 3                                               # 3. unlabeled rows as one class: row 3 takes every unlabeled key
            assert int(L["lq"][i]) == -1
            bad = M.clone()
            bad[i] |= L["lk"] == -1
            assert int(bad[i].sum()) > int(M[i].sum())
            over = C.ratios(S.emulate(q, k, bad, t, coef), ref, bnd)
            print(f"  unlabeled as a class (row {i}): " + " ".join(f"{n}={v:.0f}" for n, v in over.items()))
            assert over["loss_rows"] >= 10.0, (cid, T, over)


# ---- labels travel with the rows ----

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _gather_worker(rank, world, port, out):
    import torch.distributed as dist
    from aecf_amd import dp
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        n = (3, 5)[rank]
        lo = (0, 3)[rank]
        lab = torch.tensor([2 ** 40 + 7, -1, 5, 2 ** 33, 0, -1, 9, 2 ** 62][lo:lo + n], dtype=torch.int64)
        z = (lab.double() % 1000).float()[:, None] * torch.ones(1, 4)
        out.put((rank, dp.all_gather_rows(lab).tolist(), dp.all_gather_rows(z)[:, 0].tolist(),
                 dp.all_gather_rows(lab, sizes=[3, 5]).tolist()))
    finally:
        dist.destroy_process_group()


def test_all_gather_rows_keeps_int64_labels_with_their_rows():
    """gloo, world size 2, 3 and 5 local rows: int64 labels come back in the order of the embeddings' rows, all 64 bits kept"""
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    res = [out.get(timeout=150) for _ in range(world)]
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    want = [2 ** 40 + 7, -1, 5, 2 ** 33, 0, -1, 9, 2 ** 62]
    for _, lab_all, z_all, lab_sized in res:
        assert lab_all == want and lab_sized == want
        assert z_all == [float(v % 1000) for v in want]
