"""CPU-only tests of what tests/test_supcon_ml_pool_tile_gpu.py stands on (tests/supcon_ml_pool_tile_cases.py): the four entry points
of the tile-GEMM pooled multi-label contrastive loss load, refuse in their documented order, and their workspace query agrees with
the documented layout; the Python surface checks its arguments; the float64 three-block reference adds up to the pooled gradients
of tests/supcon_pool_cases.reference and the excluded key never carries weight; an emulation of the design's arithmetic stays
inside the derived bounds on S1 - S4, S3m and S3e for both weightings at both temperatures; and the bounds have teeth -- the same
emulation with one broken rule leaves them on a named output of a named case by the factor the table states.  The refusals are
host code: the pointers handed over are bogus."""
import functools
import os

import pytest
import torch

from aecf_amd import _lib
from tests import nce_tile_cases as N
from tests import supcon_ml_pool_tile_cases as C

BAD = 0x10          # never dereferenced: every call that gets it must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4
NAMES = ("aecf_supcon_ml_pool_sym_workspace_bytes", "aecf_supcon_ml_pool_sym_pass1", "aecf_supcon_ml_pool_sym_loss",
         "aecf_supcon_ml_pool_sym_grads")


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


def _ratios(cid, weighting, T, rule=None):
    c = C.make_case(cid)
    t, ref, bnd = _want(cid, weighting, T)
    out = C.emulate(c["a"], c["b"], c["sr"], c["sc"], weighting, c["shards"], t, c["coef"], rule=rule)
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
            assert lib.aecf_supcon_ml_pool_sym_workspace_bytes(hi - lo, n, d) == C.workspace_bytes_py(hi - lo, n, d), (cid, lo)
            # (the layout is the pooled single-label form's, shared)
            assert lib.aecf_supcon_ml_pool_sym_workspace_bytes(hi - lo, n, d) == lib.aecf_supcon_pool_sym_workspace_bytes(hi - lo, n, d)
    assert lib.aecf_supcon_ml_pool_sym_workspace_bytes(8192, 65536, 768) == C.workspace_bytes_py(8192, 65536, 768)
    assert lib.aecf_supcon_ml_pool_sym_workspace_bytes(64, 64, 96) == 0       # d % 64
    assert lib.aecf_supcon_ml_pool_sym_workspace_bytes(64, 64, 4160) == 0     # d > 4096
    assert lib.aecf_supcon_ml_pool_sym_workspace_bytes(65, 64, 64) == 0       # rows > cols
    assert lib.aecf_supcon_ml_pool_sym_workspace_bytes(0, 64, 64) == 0
    assert lib.aecf_supcon_ml_pool_sym_workspace_bytes(64, 64, 64) > 0
    # two blocks' overlap weight sums add in float32: cols <= 2^23, half the cross-view multi-label form's bound
    assert lib.aecf_supcon_ml_pool_sym_workspace_bytes(1, 2 ** 23, 64) > 0
    assert lib.aecf_supcon_ml_pool_sym_workspace_bytes(1, 2 ** 23 + 1, 64) == 0
    assert lib.aecf_supcon_ml_sym_workspace_bytes(1, 2 ** 23 + 1, 64) > 0


def test_refusals_in_order(lib):
    """sizes, then the shape support and the weighting, then NULL pointers, then the workspace size -- before any pointer is read.
    The entry points take bf16 rows only (there is no dtype argument to ask for float16 with; the Python surface refuses it, see
    test_python_argument_checks and the GPU tests); a float16 GRADIENT dtype is refused here."""
    n, d, f = 300, 192, lib.aecf_supcon_ml_pool_sym_workspace_bytes(300, 300, 192)
    p1 = lambda rows=n, cols=n, off=0, dd=d, t=BAD, mt=0.025, al=BAD, bl=BAD, aa=BAD, ba=BAD, sr=BAD, sc=BAD, w=0, ws=BAD, wsb=f, \
        cs=BAD: lib.aecf_supcon_ml_pool_sym_pass1(rows, cols, off, dd, t, mt, al, bl, aa, ba, sr, sc, w, ws, wsb, cs, None)
    assert p1(rows=0) == BAD_DIMS and p1(off=1) == BAD_DIMS and p1(off=-1) == BAD_DIMS and p1(mt=0.0) == BAD_DIMS
    assert p1(cols=2 ** 31, dd=96) == BAD_DIMS and p1(rows=n + 1, t=None) == BAD_DIMS
    assert p1(dd=96, t=None) == UNSUPPORTED and p1(mt=0.0249, t=None) == UNSUPPORTED and p1(dd=4160, t=None) == UNSUPPORTED
    assert p1(cols=2 ** 23 + 1, t=None) == UNSUPPORTED
    assert p1(w=2, t=None) == UNSUPPORTED and p1(w=-1, t=None) == UNSUPPORTED and p1(w=1, wsb=0) == WORKSPACE
    for name in ("t", "al", "bl", "aa", "ba", "sr", "sc", "ws", "cs"):
        assert p1(wsb=0, **{name: None}) == NULL_POINTER, name
    assert p1(wsb=f - 1) == WORKSPACE
    ls = lambda rows=n, dd=d, t=BAD, al=BAD, ba=BAD, cs=BAD, ws=BAD, wsb=f, lr=BAD: \
        lib.aecf_supcon_ml_pool_sym_loss(rows, n, 0, dd, t, 0.025, al, ba, cs, ws, wsb, lr, None)
    assert ls(rows=n + 1) == BAD_DIMS and ls(dd=96, cs=None) == UNSUPPORTED
    for name in ("t", "al", "ba", "cs", "ws", "lr"):
        assert ls(wsb=0, **{name: None}) == NULL_POINTER, name
    assert ls(wsb=f - 1) == WORKSPACE
    gr = lambda rows=n, dd=d, gdt=_lib.AECF_F32, t=BAD, al=BAD, bl=BAD, aa=BAD, ba=BAD, sr=BAD, sc=BAD, w=1, ws=BAD, wsb=f, up=None, \
        o1=BAD, o2=BAD, o3=BAD, o4=BAD, dtp=None: lib.aecf_supcon_ml_pool_sym_grads(rows, n, 0, dd, t, 0.025, 1.0, al, bl, aa, ba, sr, sc,
                                                                                    w, ws, wsb, up, gdt, o1, o2, o3, o4, dtp, None)
    assert gr(rows=-1) == BAD_DIMS and gr(dd=96, o1=None) == UNSUPPORTED and gr(gdt=_lib.AECF_F16, o1=None) == UNSUPPORTED
    assert gr(w=2, o1=None) == UNSUPPORTED
    for name in ("t", "al", "bl", "aa", "ba", "sr", "sc", "ws", "o1", "o2", "o3", "o4"):
        assert gr(wsb=0, **{name: None}) == NULL_POINTER, name
    assert gr(wsb=f - 1) == WORKSPACE                                    # (upstream and d_temperature may be NULL)


def test_python_argument_checks():
    from aecf_amd import losses
    z = torch.zeros(4, 128, dtype=torch.bfloat16)
    sets = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="weighting must be 'overlap' or 'jaccard'"):
        losses.pooled_multilabel_contrastive(z, z, sets, weighting="dice")
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.pooled_multilabel_contrastive(z, z, sets)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.pooled_multilabel_contrastive(z, z, torch.zeros(4, 5, dtype=torch.bool), weighting="jaccard")
    # (the set checks of multilabel_contrastive, reached on a device: see the GPU tests; the routing below stops at the device too)
    for lm in (None, False):
        with pytest.raises(RuntimeError, match="ROCm device"):
            losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="multilabel_pool", labels=sets, low_memory=lm)
    with pytest.raises(RuntimeError, match="ROCm device"):                      # (intra_view is ignored for this form)
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="multilabel_pool", labels=sets, intra_view=True,
                                label_weighting="jaccard")
    with pytest.raises(NotImplementedError, match="no streaming form"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="multilabel_pool", labels=sets, low_memory=True)
    with pytest.raises(ValueError, match="needs labels"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="multilabel_pool")
    with pytest.raises(ValueError, match="label_weighting"):
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="multilabel_pool", labels=sets, label_weighting="dice")
    with pytest.raises(ValueError, match="multilabel_pool"):                    # the list of names holds the new one
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="pooled")
    with pytest.raises(ValueError, match="multilabel_pool"):                    # and so does the list of the forms that take labels
        losses.fusion_objective(torch.zeros(()), None, None, z, z, contrastive="nt_xent", labels=sets)


def test_set_argument_checks_come_before_any_launch():
    """dtype and shape of the sets: checked by _label_sets_arg, which the new function shares with multilabel_contrastive"""
    from aecf_amd import losses
    z = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="int64"):
        losses._label_sets_arg(torch.zeros(4, dtype=torch.int32), z)
    with pytest.raises(TypeError, match="multi-hot"):
        losses._label_sets_arg(torch.zeros(4, 5, dtype=torch.int64), z)
    with pytest.raises(ValueError, match="one set per local row"):
        losses._label_sets_arg(torch.zeros(3, dtype=torch.int64), z)
    with pytest.raises(NotImplementedError, match="at most 64 classes"):
        losses._label_sets_arg(torch.zeros(4, 65, dtype=torch.bool), z)


@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
def test_the_plan_composes(weighting):
    """anchors with a weight by label, the most such weights of one anchor over both views; the excluded key never carries weight
    and the partner weighs 1, on every case (S3m's row 2 included: its sets share nothing and the partner still counts)"""
    for cid in C.ALL_IDS:
        anchors, most, excluded_weighs, partner_one = C.composition(cid, weighting)
        n = C.make_case(cid)["a"].shape[0]
        print(f"supcon_ml_pool_tile composition {cid} {weighting}: {anchors} of {2 * n} anchors weighted, at most {most} weights")
        assert not excluded_weighs and partner_one, cid
        assert (anchors == 0) == (cid in ("S1", "S3e")), (cid, anchors)
    assert C.composition("S3", weighting)[0] > 300 and C.composition("S4", weighting)[1] > 1000       # dense, as the timing run


@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
@pytest.mark.parametrize("cid", C.ALL_IDS)
def test_three_block_reference_adds_up_to_the_pooled_gradients(cid, weighting):
    """this module's shares of the four gradients and of dT, added up, against dq and dk of tests/supcon_pool_cases.reference over
    the pool [b | a] of both anchor halves: float64 against float64"""
    c = C.make_case(cid)
    worst, dT = C.pooled_check(c["a"], c["b"], c["sr"], c["sc"], weighting, c["shards"], C.used_temperature(0.07), c["coef"])
    print(f"supcon_ml_pool_tile pooled check {cid} {weighting}: gradients {worst:.3g} dT {dT:.3g}")
    assert worst <= 1e-12 and dT <= 1e-10, (cid, worst, dT)


@pytest.mark.parametrize("T", C.TEMPS)
@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
@pytest.mark.parametrize("cid", C.ALL_IDS)
def test_emulation_sits_inside_the_bounds(cid, weighting, T):
    r = _ratios(cid, weighting, T)
    _, ref, bnd = _want(cid, weighting, T)
    sig = C.signal(ref, bnd)
    print(f"supcon_ml_pool_tile emulation {cid} {weighting} T {T}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items())
          + " | value/bound " + " ".join(f"{k}={sig[k]:.3g}" for k in r))
    assert set(r) == set(C.OUTPUTS)
    assert all(v <= 1.0 for v in r.values()), (cid, weighting, T, r)


# (rule, case, the output that must leave its bound, by at least this factor).  The factors are floors under what this emulation
# gives on the CPU at both temperatures and both weightings (the runs print the figures): about
#   anchor_kept        S3 loss_rows 9e3, S4 da_all_sum 1e4       anchor_by_sets    S3 colwx 7e3, S4 loss_rows 1e3
#   partner_by_sets    inf: an anchor with an empty set (S3) or sets disjoint from its partner's (S3m row 2) gets the weight sum 0,
#                      and its mean, loss row and gradients are no numbers
#   partner_twice      S2 loss_rows 2.6e3, S4 db_all_sum 1.1e3   y_weights_lost    S3 loss_rows 3.5e3, S4 da_loc 60
#   z_at_local_index   S2 colwx 8e5, S4 loss_rows 6.7e4          wy_subtracts_col  S3 da_all_sum 2.6e2, S4 da_loc 19
#   union_inter        S3 loss_rows 8e3, S4 colwx 2.7e5
MUTATIONS = [
    ("anchor_kept", "S3", "loss_rows", 1e3),
    ("anchor_kept", "S4", "da_all_sum", 1e3),
    ("anchor_by_sets", "S3", "colwx", 1e3),
    ("anchor_by_sets", "S4", "loss_rows", 1e2),
    ("partner_by_sets", "S3", "loss_rows", float("inf")),
    ("partner_by_sets", "S3m", "da_loc", float("inf")),
    ("partner_twice", "S2", "loss_rows", 1e3),
    ("partner_twice", "S4", "db_all_sum", 1e2),
    ("y_weights_lost", "S3", "loss_rows", 1e3),
    ("y_weights_lost", "S4", "da_loc", 10.0),
    ("z_at_local_index", "S2", "colwx", 1e4),
    ("z_at_local_index", "S4", "loss_rows", 1e3),
    ("wy_subtracts_col", "S3", "da_all_sum", 1e2),
    ("wy_subtracts_col", "S4", "da_loc", 5.0),
    ("union_inter", "S3", "loss_rows", 1e3),
    ("union_inter", "S4", "colwx", 1e4),
]


@pytest.mark.parametrize("kind,cid,where,least", MUTATIONS, ids=[f"{m[0]}-{m[1]}" for m in MUTATIONS])
@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
@pytest.mark.parametrize("T", C.TEMPS)
def test_broken_rules_leave_the_bounds(kind, cid, where, least, weighting, T):
    r = _ratios(cid, weighting, T, kind)
    print(f"supcon_ml_pool_tile rule {kind} on {cid} {weighting} T {T}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
    assert r[where] >= least, (kind, cid, weighting, where, r)


@pytest.mark.parametrize("weighting", C.WEIGHTINGS)
def test_rules_that_cannot_be_told_apart_are_named(weighting):
    """Two rules change nothing on some cases, and the emulation must say so with a ratio identical to the correct one's: on a
    one-shard case (S3, off = 0) the local index IS the global one, so z_at_local_index shows on S2 and S4 only; with every set
    empty (S3e) a key weighted by its sets weighs 0, so anchor_by_sets shows only where sets exist.  Every rule of C.RULES is in the
    table above with a case on which it does show."""
    assert _ratios("S3", weighting, 0.07, "z_at_local_index") == _ratios("S3", weighting, 0.07)
    assert _ratios("S3e", weighting, 0.07, "anchor_by_sets") == _ratios("S3e", weighting, 0.07)
    assert {m[0] for m in MUTATIONS} == set(C.RULES)
