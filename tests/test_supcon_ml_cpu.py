"""CPU-only tests of the multi-label supervised contrastive loss: aecf_supcon_ml_workspace_bytes / aecf_supcon_ml_fwd_bwd /
aecf_label_sets_pack are declared, bound and exported with the ABI version still 10; the workspace is the documented size; every
refusal comes back in the documented order (sizes, width or weighting, NULL pointers, workspace size) before any pointer is read or
any kernel is launched -- the pointers handed over here are deliberately bogus; the Python surface rejects malformed sets, option
combinations and CPU tensors; the packing restated in torch gives the expected words; and what tests/test_supcon_ml_gpu.py stands
on (tests/supcon_ml_cases.py) has teeth: an emulation of the design's arithmetic stays inside the derived bounds at every case,
temperature and weighting, and the same emulation with the weight rule broken in one of five ways leaves them."""
import functools
import os
import re

import pytest
import torch

from aecf_amd import _lib
from tests import nce_stream_cases as C
from tests import supcon_ml_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["aecf_supcon_ml_workspace_bytes", "aecf_supcon_ml_fwd_bwd", "aecf_label_sets_pack"]
BAD = 0x10          # never dereferenced: every call below must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_supcon_ml_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "aecf_hip.h")).read()
    declared = set(re.findall(r"\b(aecf_[a-z_0-9]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOL_NAMES
        assert hasattr(lib, name)
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10
    for macro, value in (("AECF_SETS_OVERLAP", 0), ("AECF_SETS_JACCARD", 1), ("AECF_SETS_U8", 3)):
        assert re.search(rf"#define {macro} {value}\b", header) and getattr(_lib, macro) == value


def test_workspace_bytes_match_the_restatement(lib):
    need = lib.aecf_supcon_ml_workspace_bytes
    assert need(333, 333, 100) == 0 and need(0, 333, 256) == 0 and need(333, 333, 2048) == 0
    for cid, ((rows, cols, _, d), _, _) in C.CASES.items():
        assert need(rows, cols, d) == S.workspace_bytes_py(rows, cols, d) == lib.aecf_supcon_workspace_bytes(rows, cols, d), cid
    assert need(8192, 65536, 768) == S.workspace_bytes_py(8192, 65536, 768)


def _call(lib, rows=256, cols=256, off=0, d=256, t=BAD, min_t=1e-3, q=BAD, k=BAD, sq=BAD, sk=BAD, w=0, lr=BAD, dq=BAD, dk=BAD, dt=BAD,
          ws=BAD, wsb=1 << 30):
    return lib.aecf_supcon_ml_fwd_bwd(rows, cols, off, d, t, min_t, 1.0 / max(cols, 1), q, k, sq, sk, w, lr, dq, dk, dt, ws, wsb, None)


def test_fwd_bwd_refuses_in_the_documented_order(lib):
    # 1. sizes (with everything else wrong too: width, weighting, a NULL, the workspace)
    for bad in (dict(rows=0), dict(cols=0), dict(d=0), dict(min_t=0.0), dict(min_t=-1.0), dict(off=-1), dict(off=1),
                dict(rows=257)):
        kw = dict(d=100, w=2, t=None, sq=None, wsb=0)
        kw.update(bad)
        assert _call(lib, **kw) == BAD_DIMS, bad
    # 2. the width and the weighting, before any pointer is looked at
    for d in (64, 100, 192, 2048):
        assert _call(lib, d=d, t=None, sk=None, wsb=0) == UNSUPPORTED, d
    for w in (-1, 2, 7):
        assert _call(lib, w=w, t=None, sk=None, wsb=0) == UNSUPPORTED, w
    # 3. NULL pointers: each of the required ones, the temperature and both set arrays included, and exactly one of dq / dk
    for w in (0, 1):
        for name in ("t", "q", "k", "sq", "sk", "lr", "ws", "dq", "dk"):
            assert _call(lib, w=w, wsb=0, **{name: None}) == NULL_POINTER, name
        assert _call(lib, w=w, wsb=0, dq=None, dk=None) == NULL_POINTER         # a loss-only call takes no d_temperature
        # 4. then the workspace size: with gradients, without d_temperature, in the loss-only mode, and one byte short
        assert _call(lib, w=w, wsb=16) == WORKSPACE
        assert _call(lib, w=w, wsb=16, dt=None) == WORKSPACE
        assert _call(lib, w=w, wsb=16, dq=None, dk=None, dt=None) == WORKSPACE
        assert _call(lib, w=w, wsb=lib.aecf_supcon_ml_workspace_bytes(256, 256, 256) - 1) == WORKSPACE


def test_pack_refuses_in_the_documented_order(lib):
    pack = lib.aecf_label_sets_pack
    for rows, classes in ((0, 15), (-1, 15), (4, 0), (4, -3), (4, 65)):
        assert pack(rows, classes, 9, None, None, None) == BAD_DIMS, (rows, classes)
    for kind in (-1, 4, 9):
        assert pack(4, 15, kind, None, None, None) == UNSUPPORTED, kind
    for kind in (_lib.AECF_BF16, _lib.AECF_F32, _lib.AECF_F16, _lib.AECF_SETS_U8):
        assert pack(4, 64, kind, None, BAD, None) == NULL_POINTER and pack(4, 1, kind, BAD, None, None) == NULL_POINTER


def test_python_rejects_malformed_sets():
    from aecf_amd.losses import _label_sets_arg
    z = torch.zeros(4, 128, dtype=torch.bfloat16)
    ready = torch.zeros(4, dtype=torch.int64)
    assert _label_sets_arg(ready, z) is ready
    for dtype in (torch.bool, torch.uint8, torch.bfloat16, torch.float16, torch.float32):
        for classes in (1, 15, 64):
            hot = torch.zeros(4, classes, dtype=dtype)
            assert _label_sets_arg(hot, z) is hot
    with pytest.raises(TypeError, match="label sets"):
        _label_sets_arg([0, 1, 2, 3], z)
    with pytest.raises(TypeError, match="int64"):
        _label_sets_arg(ready.to(torch.int32), z)                            # ready masks are int64 and nothing else
    with pytest.raises(TypeError, match="int64"):
        _label_sets_arg(torch.zeros(4), z)
    with pytest.raises(TypeError, match="multi-hot"):
        _label_sets_arg(torch.zeros(4, 15, dtype=torch.int64), z)            # a multi-hot dtype that is not served
    with pytest.raises(TypeError, match="multi-hot"):
        _label_sets_arg(torch.zeros(4, 15, dtype=torch.float64), z)
    with pytest.raises(NotImplementedError, match="at most 64 classes"):
        _label_sets_arg(torch.zeros(4, 65, dtype=torch.bool), z)             # the limit, by name
    with pytest.raises(ValueError, match="label sets"):
        _label_sets_arg(torch.zeros(5, dtype=torch.int64), z)                # wrong length
    with pytest.raises(ValueError, match="label sets"):
        _label_sets_arg(torch.zeros(5, 15, dtype=torch.bool), z)
    with pytest.raises(ValueError, match="label sets"):
        _label_sets_arg(torch.zeros(4, 15, 1, dtype=torch.bool), z)
    with pytest.raises(ValueError, match="label sets"):
        _label_sets_arg(torch.zeros(4, 0, dtype=torch.bool), z)
    with pytest.raises(ValueError, match="label sets"):
        _label_sets_arg(torch.zeros(4, dtype=torch.int64, device="meta"), z)  # not where the embeddings live


def test_cpu_tensors_and_option_combinations_are_refused():
    from aecf_amd import losses
    z = torch.zeros(4, 128, dtype=torch.bfloat16)
    ready = torch.zeros(4, dtype=torch.int64)
    hot = torch.zeros(4, 15, dtype=torch.bool)
    task = torch.zeros(())
    for weighting in S.WEIGHTINGS:
        with pytest.raises(RuntimeError, match="ROCm device"):
            losses.multilabel_contrastive(z, z, ready, weighting)
        with pytest.raises(RuntimeError, match="ROCm device"):
            losses.fusion_objective(task, None, None, z, z, contrastive="multilabel", labels=hot, label_weighting=weighting)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.pack_label_sets(hot)
    with pytest.raises(NotImplementedError, match="at most 64 classes"):
        losses.pack_label_sets(torch.zeros(4, 65, dtype=torch.bool))
    with pytest.raises(ValueError, match="weighting"):
        losses.multilabel_contrastive(z, z, ready, "dice")
    with pytest.raises(ValueError, match="label_weighting"):
        losses.fusion_objective(task, None, None, z, z, contrastive="multilabel", labels=ready, label_weighting="dice")
    with pytest.raises(ValueError, match="labels"):
        losses.fusion_objective(task, None, None, z, z, contrastive="multilabel")
    for form in ("info_nce", "sigmoid"):
        with pytest.raises(ValueError, match="labels"):
            losses.fusion_objective(task, None, None, z, z, contrastive=form, labels=ready)
    with pytest.raises(ValueError, match="contrastive"):
        losses.fusion_objective(task, None, None, z, z, contrastive="multi_label", labels=ready)


# ---- the packing, restated ----

@pytest.mark.parametrize("classes", (1, 15, 63, 64))
def test_packing_restatement_gives_the_expected_words(classes):
    """rows: empty, class 0 alone, the last class alone, every class, every other class; in every dtype the kernel serves, with
    values that are members without being 1 (2, -3.5, 255) and -0.0, which is none"""
    last = classes - 1
    rows = [[], [0], [last], list(range(classes)), list(range(0, classes, 2))]
    want = torch.tensor([S.mask(r) for r in rows], dtype=torch.int64)
    assert int(want[2]) == (-(1 << 63) if classes == 64 else 1 << last)      # class 63 is the sign bit
    hot = torch.zeros(len(rows), classes)
    for i, r in enumerate(rows):
        hot[i, r] = 1.0
    for dtype in (torch.bool, torch.uint8, torch.bfloat16, torch.float16, torch.float32):
        assert torch.equal(S.pack_torch(hot.to(dtype)), want), dtype
    odd = hot * torch.tensor([2.0, -3.5, 255.0]).repeat(classes)[:classes]
    odd[0] = -0.0
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        assert torch.equal(S.pack_torch(odd.to(dtype)), want), dtype
    for word, r in zip(want.tolist(), rows):
        assert S.classes_of(word) == r
    assert torch.equal(S.unpack(want)[:, :classes], hot.double()) and not bool(S.unpack(want)[:, classes:].any())


# ---- the set plan, the bounds and their teeth ----

@functools.lru_cache(maxsize=4)
def _setup(cid, weighting):
    c = C.make_case(S.base(cid))
    L = S.sets(cid)
    return c["q"], c["k"], c["off"], L, S.weights(L["sq"], L["sk"], c["off"], weighting)


def _judged(cid, weighting, T):
    q, k, off, L, w = _setup(cid, weighting)
    t, coef = C.used_temperature(T), 1.0 / k.shape[0]
    ref = S.reference(q, k, w, t, coef)
    bnd = S.bounds(ref, q, k, t, coef, C.eps_x(C.score_error(S.base(cid)), t, k.shape[0]))
    return q, k, off, L, t, coef, S.slim(ref), bnd


@pytest.mark.parametrize("cid", S.CASE_IDS)
def test_set_plan_holds_its_traps(cid):
    """what the plan of tests/supcon_ml_cases.py promises, read back from the words"""
    c = C.make_case(S.base(cid))
    L = S.sets(cid)
    off, sq, sk, h = c["off"], L["sq"], L["sk"], L["heavy"]
    rows = sq.shape[0]
    inter, union, inter_lo, union_lo = S.counts(sq, sk)
    jac, ovl = S.weights(sq, sk, off, "jaccard"), S.weights(sq, sk, off, "overlap")
    i = torch.arange(rows)
    assert bool((jac[i, off + i] == 1).all()) and bool((ovl[i, off + i] == 1).all())          # the partner, by index
    assert bool(((jac > 0) == (ovl > 0)).all()) and bool((jac <= ovl).all())
    for j, r in c["sentinels"]:                                     # a weighted positive, partly overlapping, on every boundary
        assert 0 < float(jac[r, j]) < 1 and float(ovl[r, j]) == 1 and 62 in S.classes_of(int(sk[j]))
    if cid == "A":
        return
    assert S.classes_of(int(sq[h])) == list(S.HEAVY) and int(sq[h]) < 0                       # class 63: a negative int64
    assert 1 <= len(L["large"]) <= 60 and len(L["twins"]) >= 1
    for j in L["large"]:                                            # class 63 alone is shared: nothing in the low word
        assert float(inter[h, j]) == 1 and float(inter_lo[h, j]) == 0 and float(jac[h, j]) == 0.25
    for j in L["twins"]:                                            # equal low words, different high words
        assert float(inter_lo[h, j]) == float(union_lo[h, j]) == 1 and float(union[h, j]) == 4 and float(jac[h, j]) == 0.25
    if rows == 1:
        return
    assert 60 <= int((jac[h] > 0).sum()) <= 75                      # about 60 weighted positives, and over all splits
    _, live, per, _ = C.flash_split_py(rows, sk.shape[0])
    hit = {j // per for j in L["large"]}
    assert set(range(live - 1)) <= hit                              # (the last split may hold a sentinel or local rows alone)
    empty_q, empty_k = sq == 0, sk == 0
    assert int(empty_q.sum()) >= 1 and int((empty_k & ~_local(off, rows, sk.shape[0])).sum()) >= 1
    assert bool((jac[empty_q].sum(dim=1) == 1).all())               # an unlabeled row has its partner alone
    partial = jac[(jac > 0) & (jac < 1)]
    assert len(set(partial.tolist())) >= 4                          # several distinct Jaccard weights
    if cid == "C9":
        assert float(inter[2, off + 2]) == 0 and float(jac[2, off + 2]) == 1 and float(jac[2].sum()) == 1


def _local(off, rows, cols):
    j = torch.arange(cols)
    return (j >= off) & (j < off + rows)


@pytest.mark.parametrize("cid", S.CASE_IDS)
def test_bounds_hold_the_emulation(cid):
    for weighting in S.WEIGHTINGS:
        for T in S.TEMPS:
            q, k, off, L, t, coef, ref, bnd = _judged(cid, weighting, T)
            intact = C.ratios(S.emulate(q, k, S.weights(L["sq"], L["sk"], off, weighting, single=True), t, coef), ref, bnd)
            print(f"supcon_ml emulation {cid} {weighting} T={T}: " + " ".join(f"{n}={v:.3f}" for n, v in intact.items()))
            assert not S.outside(intact), (cid, weighting, T, intact)


@pytest.mark.parametrize("rule", S.RULES)
def test_bounds_catch_a_broken_weight_rule(rule):
    """each broken rule of supcon_ml_cases.weights leaves the bounds on at least one case (here: the cases that are quick on the
    CPU, at T = 0.07), and on case C9 where the rule is the partner's"""
    caught = []
    for cid in ("B", "C", "C9", "D"):
        for weighting in S.WEIGHTINGS:
            if rule == "pop_lo" and weighting == "overlap":
                continue                                            # overlap forms no popcount
            q, k, off, L, t, coef, ref, bnd = _judged(cid, weighting, 0.07)
            over = C.ratios(S.emulate(q, k, S.weights(L["sq"], L["sk"], off, weighting, rule, single=True), t, coef), ref, bnd)
            print(f"  {rule} {cid} {weighting}: " + " ".join(f"{n}={v:.1f}" for n, v in over.items()))
            if S.outside(over):
                caught.append((cid, weighting))
    print(f"{rule}: outside the bounds on {caught}")
    assert caught, rule
    if rule == "partner_by_sets":
        assert ("C9", "overlap") in caught and ("C9", "jaccard") in caught
