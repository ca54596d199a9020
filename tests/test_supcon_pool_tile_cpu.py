"""CPU-only tests of what tests/test_supcon_pool_tile_gpu.py stands on (tests/supcon_pool_tile_cases.py): the four entry points of
the tile-GEMM pooled supervised contrastive loss load, refuse in their documented order, and their workspace query agrees with the
documented layout; the Python surface checks its arguments; the float64 three-block reference adds up to the pooled gradients of
tests/supcon_pool_cases.reference; the label plan composes as the cases' docstring says; an emulation of the design's arithmetic
stays inside the derived bounds on S1 - S4 and on S3 without labels at both temperatures; and the bounds have teeth -- the same
emulation with one broken rule leaves them by a factor of at least 2 on a named output of a named case.  The refusals are host
code: the pointers handed over are bogus."""
import functools
import os

import pytest
import torch

from aecf_amd import _lib
from tests import nce_tile_cases as N
from tests import supcon_pool_tile_cases as C

BAD = 0x10          # never dereferenced: every call that gets it must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4
NAMES = ("aecf_supcon_pool_sym_workspace_bytes", "aecf_supcon_pool_sym_pass1", "aecf_supcon_pool_sym_loss",
         "aecf_supcon_pool_sym_grads")


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
    ref, bnd = C.reference(c["a"], c["b"], c["lab"], c["shards"], t, c["coef"], C.score_error(cid))
    return t, ref, bnd


def _ratios(cid, T, mutation=None):
    c = C.make_case(cid)
    t, ref, bnd = _want(cid, T)
    out = C.emulate(c["a"], c["b"], c["lab"], c["shards"], t, c["coef"], mutation=mutation)
    for name in ("da_all", "db_all"):
        out[name + "_sum"] = sum(x.double() for x in out[name])
    return C.ratios(out, ref, bnd)


def test_symbols_are_declared_bound_and_exported(lib):
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aecf_hip.h")).read()
    bound = {s[0] for s in _lib._SYMBOLS}
    for name in NAMES:
        assert getattr(lib, name) is not None and name in bound and name + "(" in header, name


def test_workspace_bytes_match_the_documented_layout(lib):
    for cid in C.TILE_IDS:
        (n, d), shards, _, _ = N.SYMMETRIC[cid]
        for lo, hi in shards:
            assert lib.aecf_supcon_pool_sym_workspace_bytes(hi - lo, n, d) == C.workspace_bytes_py(hi - lo, n, d), (cid, lo)
    assert lib.aecf_supcon_pool_sym_workspace_bytes(8192, 65536, 768) == C.workspace_bytes_py(8192, 65536, 768)
    assert lib.aecf_supcon_pool_sym_workspace_bytes(64, 64, 96) == 0          # d % 64
    assert lib.aecf_supcon_pool_sym_workspace_bytes(64, 64, 4160) == 0        # d > 4096
    assert lib.aecf_supcon_pool_sym_workspace_bytes(65, 64, 64) == 0          # rows > cols
    assert lib.aecf_supcon_pool_sym_workspace_bytes(0, 64, 64) == 0
    assert lib.aecf_supcon_pool_sym_workspace_bytes(64, 64, 64) > 0
    # 1 + ka <= 2 cols - 1 exact in float32: cols <= 2^23, half the cross-view form's bound
    assert lib.aecf_supcon_pool_sym_workspace_bytes(1, 2 ** 23, 64) > 0
    assert lib.aecf_supcon_pool_sym_workspace_bytes(1, 2 ** 23 + 1, 64) == 0
    assert lib.aecf_supcon_sym_workspace_bytes(1, 2 ** 23 + 1, 64) > 0


def test_refusals_in_order(lib):
    """sizes, then the shape support, then NULL pointers, then the workspace size -- before any pointer is read"""
    n, d, f = 300, 192, lib.aecf_supcon_pool_sym_workspace_bytes(300, 300, 192)
    p1 = lambda rows=n, cols=n, off=0, dd=d, t=BAD, mt=0.025, al=BAD, bl=BAD, aa=BAD, ba=BAD, lr=BAD, lc=BAD, ws=BAD, wsb=f, cs=BAD: \
        lib.aecf_supcon_pool_sym_pass1(rows, cols, off, dd, t, mt, al, bl, aa, ba, lr, lc, ws, wsb, cs, None)
    assert p1(rows=0) == BAD_DIMS and p1(off=1) == BAD_DIMS and p1(off=-1) == BAD_DIMS and p1(mt=0.0) == BAD_DIMS
    assert p1(cols=2 ** 31, dd=96) == BAD_DIMS and p1(rows=n + 1, t=None) == BAD_DIMS
    assert p1(dd=96, t=None) == UNSUPPORTED and p1(mt=0.0249, t=None) == UNSUPPORTED and p1(dd=4160, t=None) == UNSUPPORTED
    assert p1(cols=2 ** 23 + 1, t=None) == UNSUPPORTED
    for name in ("t", "al", "bl", "aa", "ba", "lr", "lc", "ws", "cs"):
        assert p1(wsb=0, **{name: None}) == NULL_POINTER, name
    assert p1(wsb=f - 1) == WORKSPACE
    ls = lambda rows=n, dd=d, t=BAD, al=BAD, ba=BAD, cs=BAD, ws=BAD, wsb=f, lr=BAD: \
        lib.aecf_supcon_pool_sym_loss(rows, n, 0, dd, t, 0.025, al, ba, cs, ws, wsb, lr, None)
    assert ls(rows=n + 1) == BAD_DIMS and ls(dd=96, cs=None) == UNSUPPORTED
    for name in ("t", "al", "ba", "cs", "ws", "lr"):
        assert ls(wsb=0, **{name: None}) == NULL_POINTER, name
    assert ls(wsb=f - 1) == WORKSPACE
    gr = lambda rows=n, dd=d, gdt=_lib.AECF_F32, t=BAD, al=BAD, bl=BAD, aa=BAD, ba=BAD, lr=BAD, lc=BAD, ws=BAD, wsb=f, up=None, \
        o1=BAD, o2=BAD, o3=BAD, o4=BAD, dtp=None: lib.aecf_supcon_pool_sym_grads(rows, n, 0, dd, t, 0.025, 1.0, al, bl, aa, ba, lr, lc, ws,
                                                                                 wsb, up, gdt, o1, o2, o3, o4, dtp, None)
    assert gr(rows=-1) == BAD_DIMS and gr(dd=96, o1=None) == UNSUPPORTED and gr(gdt=_lib.AECF_F16, o1=None) == UNSUPPORTED
    for name in ("t", "al", "bl", "aa", "ba", "lr", "lc", "ws", "o1", "o2", "o3", "o4"):
        assert gr(wsb=0, **{name: None}) == NULL_POINTER, name
    assert gr(wsb=f - 1) == WORKSPACE                                    # (upstream and d_temperature may be NULL)


def test_python_argument_checks():
    from aecf_amd import losses
    z = torch.zeros(4, 128, dtype=torch.bfloat16)
    lab = torch.zeros(4, dtype=torch.int64)
    for bad in ("tile", 0.5, 2):
        with pytest.raises(ValueError, match="low_memory must be True, False or None"):
            losses.pooled_supervised_contrastive(z, z, lab, low_memory=bad)
    for lm in (True, False, None):
        with pytest.raises(RuntimeError, match="ROCm device"):
            losses.pooled_supervised_contrastive(z, z, lab, low_memory=lm)
        with pytest.raises(RuntimeError, match="ROCm device"):                  # (accepted and handed on: the device is what stops it)
            losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="supervised_pool", labels=lab, low_memory=lm)
    with pytest.raises(RuntimeError, match="ROCm device"):                      # (intra_view is ignored for this form)
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="supervised_pool", labels=lab, low_memory=False,
                                intra_view=True)
    with pytest.raises(ValueError, match="low_memory must be True, False or None"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="supervised_pool", labels=lab, low_memory="tile")
    with pytest.raises(ValueError, match="needs labels"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="supervised_pool")
    with pytest.raises(ValueError, match="supervised_pool"):                    # the list of names holds the new one
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="pooled")
    # the old argument combination keeps its answer
    with pytest.raises(NotImplementedError, match="intra-view"):
        losses.supervised_contrastive(z, z, lab, low_memory=False, intra_view=True)


def test_the_label_plan_composes():
    """rows with a label positive, the most positives of one anchor (the partner among them), no excluded key a positive, the
    counts of blocks X and Y equal row by row"""
    assert C.composition("S1") == (0, 1, False, True)
    assert C.composition("S2") == (192, 53, False, True)
    assert C.composition("S3") == (225, 63, False, True)
    assert C.composition("S4") == (1685, 119, False, True)
    assert bool((C.make_case("S3u")["lab"] == -1).all())


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_three_block_reference_adds_up_to_the_pooled_gradients(cid):
    """this module's shares of the four gradients and of dT, added up, against dq and dk of tests/supcon_pool_cases.reference over
    the pool [b | a] of both anchor halves: float64 against float64"""
    c = C.make_case(cid)
    worst, dT = C.pooled_check(c["a"], c["b"], c["lab"], c["shards"], C.used_temperature(0.07), c["coef"])
    print(f"supcon_pool_tile pooled check {cid}: gradients {worst:.3g} dT {dT:.3g}")
    assert worst <= 1e-12 and dT <= 1e-10, (cid, worst, dT)


@pytest.mark.parametrize("T", C.TEMPS)
@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_emulation_sits_inside_the_bounds(cid, T):
    r = _ratios(cid, T)
    _, ref, bnd = _want(cid, T)
    sig = C.signal(ref, bnd)
    print(f"supcon_pool_tile emulation {cid} T {T}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items())
          + " | value/bound " + " ".join(f"{k}={sig[k]:.3g}" for k in r))
    assert set(r) == set(C.OUTPUTS)
    assert all(v <= 1.0 for v in r.values()), (cid, T, r)


# (rule, case, the output that must leave its bound by a factor of at least 2)
MUTATIONS = [
    ("self_positive", "S3", "loss_rows"),
    ("self_positive", "S4", "da_all_sum"),
    ("partner_twice", "S2", "loss_rows"),
    ("partner_twice", "S4", "colcnt"),
    ("y_counts_dropped", "S3", "loss_rows"),
    ("y_counts_dropped", "S4", "da_loc"),
    ("z_local", "S2", "colsx"),
    ("z_local", "S4", "loss_rows"),
    ("wy_minus_rnc", "S3", "da_all_sum"),
    ("wy_minus_rnc", "S4", "da_loc"),
]


@pytest.mark.parametrize("kind,cid,where", MUTATIONS, ids=[f"{m[0]}-{m[1]}" for m in MUTATIONS])
@pytest.mark.parametrize("T", C.TEMPS)
def test_broken_rules_leave_the_bounds(kind, cid, where, T):
    r = _ratios(cid, T, kind)
    print(f"supcon_pool_tile mutation {kind} on {cid} T {T}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
    assert not (r[where] < 2.0), (kind, cid, where, r)
