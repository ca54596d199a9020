"""CPU-only tests of the multi-label bootstrap: the numpy restatement of tests/bootstrap_cases.py (order, Philox draw, walk)
against sklearn with ``sample_weight`` and against the evaluation's own restatement on rows physically repeated by their
weights (integer statistics EQUAL); the aecf_mlboot_* entry points declared, bound and exported with the ABI version still 10,
their workspace answers and their refusals in the documented order before any pointer is read (the pointers handed over here are
bogus); and the broken rules the bounds and equalities must catch."""
import os
import re

import numpy as np
import pytest

from aecf_amd import _lib
from tests import bootstrap_cases as B
from tests import metrics_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["aecf_mlboot_workspace_bytes", "aecf_mlboot_draw_workspace_bytes", "aecf_mlboot_order", "aecf_mlboot_draw", "aecf_mlboot_walk"]
BAD = 0x10          # never dereferenced: every call below must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4
TOL = 1e-12


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------- philox and the draw

def test_philox_known_answers():
    """the known-answer vectors published with Random123 (kat_vectors, philox4x32 10 rounds)"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = B.philox4x32_10([np.array([w], dtype=np.uint64) for w in ctr], key[0], key[1])
        assert tuple(int(g[0]) for g in got) == want


def test_draw_is_a_multinomial_resample_of_rows():
    """every replicate makes n draws; replicate 0 is ones; a replicate depends on (seed, r, n) only; the row is value * n >> 64"""
    for n in (1, 2, 63, 64, 1025):
        w = B.draw_weights(n, 5, seed=(7 << 32) | 9)
        assert np.array_equal(w.sum(1), np.full(5, n)) and np.array_equal(w[0], np.ones(n, dtype=np.int64))
        assert np.array_equal(B.draw_weights(n, 2, seed=(7 << 32) | 9, replicate0=3), w[3:5])
    w = B.draw_weights(1025, 3, seed=1)
    assert not np.array_equal(w[1], w[2]) and not np.array_equal(w[1], B.draw_weights(1025, 2, seed=2)[1])
    assert not np.array_equal(w[1], B.draw_weights(1025, 2, seed=1 << 32)[1])               # the high key word matters
    lo, hi, n = np.array([0xfffffff0], dtype=np.uint64), np.array([0x89abcdef], dtype=np.uint64), 1000003
    assert int(B._row_of(lo, hi, n)[0]) == (((0x89abcdef << 32) | 0xfffffff0) * n) >> 64
    # a uniform row: over 64 replicates of 1025 draws the largest multiplicity stays far from the uint8 limit
    assert B.draw_weights(1025, 64, seed=3).max() < 16


# ---------------------------------------------------------------------------------------------- the restatement

def _weights_with_zeros(s, y, R, seed):
    """drawn weights (37 % zeros), one replicate with every positive of class 0 at weight 0 and one with a single row"""
    w = B.draw_weights(s.shape[0], R, seed)
    w[R - 1] = np.where(y[:, 0], 0, w[R - 1])
    w[R - 2] = 0
    w[R - 2, 0] = 3
    return w


@pytest.mark.parametrize("name", ["n63", "n65", "n257"])
def test_restatement_against_sklearn_sample_weight(name):
    """average_precision_score, roc_auc_score and f1_score with sample_weight per class and replicate within 1e-12; where the
    replicate holds no positive weight AP and F1 are 0 and AUROC NaN, without a negative weight AUROC is NaN"""
    metrics = pytest.importorskip("sklearn.metrics")
    s, y, _, _, seed, thr = B.case(name)
    w = _weights_with_zeros(s, y, 6, seed)
    r = B.restate(s, y, w, thr)
    sc, st = r["scores"], r["stats"]
    seen_empty = False
    for q in range(w.shape[0]):
        keep = w[q] > 0                                        # (sklearn's curves do not drop zero-weight thresholds)
        for c in range(s.shape[1]):
            yc, xc, wc = y[keep, c].astype(int), s[keep, c].astype(np.float64), w[q, keep].astype(np.float64)
            if st["wpos"][q, c] == 0:
                seen_empty = True
                assert sc["ap"][q, c] == 0.0 and np.isnan(sc["auroc"][q, c]) and sc["f1"][q, c] == 0.0
                continue
            assert abs(metrics.average_precision_score(yc, xc, sample_weight=wc) - sc["ap"][q, c]) <= TOL, (name, q, c)
            if st["wvalid"][q, c] > st["wpos"][q, c]:
                assert abs(metrics.roc_auc_score(yc, xc, sample_weight=wc) - sc["auroc"][q, c]) <= TOL, (name, q, c)
            else:
                assert np.isnan(sc["auroc"][q, c])
            pred = (s[keep, c] > thr[c]).astype(int)
            assert abs(metrics.f1_score(yc, pred, sample_weight=wc, zero_division=0) - sc["f1"][q, c]) <= TOL, (name, q, c)
    assert seen_empty


@pytest.mark.parametrize("name,threshold", [("n257", 0.5), ("specials", 0.5), ("quantised", 0.8), ("n1", 0.5)])
def test_restatement_equals_physically_repeated_rows(name, threshold):
    """a replicate's integer statistics EQUAL those of tests/metrics_cases.restate on the rows repeated by their weights (Wpos =
    n_pos, Wvalid, U2 = twice the AUROC share, TP, FP, FN), the scores agree within 1e-12 -- ties, +-0, +-inf, NaN, zero-weight
    positives and a replicate without a positive included"""
    s, y, _, _, seed, _ = B.case(name)
    n, C = s.shape
    w = _weights_with_zeros(s, y, 5, seed) if n > 1 else B.draw_weights(1, 2, seed)
    thr = np.full(C, M.logit_threshold(threshold), dtype=np.float32)
    r = B.restate(s, y, w, thr)
    st, sc = r["stats"], r["scores"]
    for q in range(w.shape[0]):
        s2, y2 = B.repeat_rows(s, y, w[q])
        ref = M.restate(s2, y2, threshold=threshold)
        assert np.array_equal(st["wpos"][q], ref["n_pos"])
        assert np.array_equal(st["wvalid"][q], len(s2) - ref["n_invalid"])
        assert np.array_equal(st["u2"][q], (2 * ref["shares"][1]).astype(np.int64)) and np.array_equal(2 * ref["shares"][1] % 1, np.zeros(C))
        for k, name_k in enumerate(("tp", "fp", "fn")):
            assert np.array_equal(st[name_k][q], ref["shares"][2 + k].astype(np.int64))
        for key in ("ap", "auroc", "f1"):
            assert np.array_equal(np.isnan(sc[key][q]), np.isnan(ref[key]))
            assert np.nanmax(np.abs(sc[key][q] - ref[key]), initial=0.0) <= TOL, (key, q)
        for key in ("map", "macro_auroc", "macro_f1"):
            assert (np.isnan(sc[key][q]) and np.isnan(ref[key])) or abs(sc[key][q] - ref[key]) <= TOL, (key, q)
    if n > 1:
        assert (st["wpos"][:, 0] == 0).any()                   # the replicate without a positive was there


def test_replicate_zero_is_the_evaluation():
    """weights of one: the statistics are multilabel_metrics' counts and the scores its restatement, NaN logits included"""
    for name in ("specials", "quantised"):
        s, y, _ = M.case(name)
        ref = M.restated(name)
        r = B.restate(s, y, np.ones((1, s.shape[0]), dtype=np.int64))
        assert np.array_equal(r["stats"]["wpos"][0], ref["n_pos"])
        for key in ("ap", "auroc", "f1"):
            assert np.nanmax(np.abs(r["scores"][key][0] - ref[key]), initial=0.0) <= TOL
        assert abs(r["scores"]["map"][0] - ref["map"]) <= TOL and abs(r["scores"]["macro_f1"][0] - ref["macro_f1"]) <= TOL


def test_order_is_a_stable_bijection_with_flags():
    s, y, _ = M.case("specials")
    order = B.restate_order(s, y, np.zeros(4, dtype=np.float32))
    for c, e in enumerate(order):
        rows = (e & 0xffffff).astype(np.int64)
        assert sorted(rows) == list(np.flatnonzero(~np.isnan(s[:, c])))
        k = np.where(s[rows, c] == 0, 0.0, s[rows, c])          # -0 ties +0
        assert (k[1:] <= k[:-1]).all()
        tie = k[1:] == k[:-1]                                    # (inf ties inf: compared, not subtracted)
        assert (np.diff(rows)[tie] > 0).all()                   # stable: equal keys in row order
        assert np.array_equal((e[1:] & B.HEAD) != 0, ~tie) and e[0] & B.HEAD
        assert np.array_equal((e & B.POS) != 0, y[rows, c]) and np.array_equal((e & B.PRED) != 0, s[rows, c] > 0)


# ---------------------------------------------------------------------------------------------- broken rules

def test_broken_rules_leave_the_bounds():
    """Each broken rule moves a value by many times its bound or breaks an equality; the smallest factor (error over bound) is
    printed.  On n257 (quarter-grid ties, 10 % positives, 130 replicates): ties walked by position, weights on the positives
    only, unweighted pred counts and classes resampled independently move mAP / macro F1; replicate 0 drawn instead of ones
    moves the point estimate off the evaluation's; a NaN replicate entering the quantile turns a defined limit into NaN; unpaired
    weights give two identical models a difference that is not exactly zero.  The factors: ties by position 5.1e11, weights on
    the positives only 1.1e10 (the smallest), unweighted pred 8.9e10, independent classes 7.2e12, replicate 0 drawn 1.8e12, a
    NaN in the quantile: a NaN limit (inf), unpaired weights 2.6e12."""
    s, y, _, R, seed, thr = B.case("n257")
    n, C = s.shape
    right = B.restated("n257")
    w = right["weights"]
    bounds = B.score_bounds(right["groups"], C)
    factors = {}
    for rule, key in (("position_ties", "map"), ("pos_weights_only", "map"), ("unweighted_pred", "macro_f1"), ("independent_classes", "map")):
        broken = B.restate(s, y, w, thr, rule=rule)["scores"][key][1:]
        moved = np.abs(broken - right["scores"][key][1:])
        factors[rule] = float(moved.min() if rule != "independent_classes" else moved.max()) / bounds[key]
    point = M.restate(s, y)["map"]
    drawn = B.restate(s, y, B.draw_weights(n, 1, seed, rule="drawn_zero"))["scores"]["map"][0]
    assert abs(B.restate(s, y, w[:1])["scores"]["map"][0] - point) <= bounds["map"]
    factors["drawn_zero"] = abs(drawn - point) / bounds["map"]
    # a class with two positives: replicates that drew neither have a NaN AUROC
    y2 = y.copy()
    y2[:, 0] = False
    y2[:2, 0] = True
    au = B.restate(s, y2, w, thr)["scores"]["auroc"][1:, 0]
    assert np.isnan(au).any() and not np.isnan(au).all()
    good = B.percentile_limits(au, 0.95)
    assert not np.isnan(good).any()
    factors["nan_in_quantile"] = float("inf") if np.isnan(np.percentile(au, [2.5, 97.5])).any() else 0.0
    # paired: a model against itself differs by exactly zero in every replicate; under other weights it does not
    a = right["scores"]["map"]
    b = B.restate(s, y, B.draw_weights(n, R, seed + 1), thr)["scores"]["map"]
    assert not (a - a)[1:].any()
    factors["unpaired"] = float(np.abs(B.percentile_limits((a - b)[1:], 0.95)).max()) / (2 * bounds["map"])
    print("bootstrap broken-rule factors: " + " ".join(f"{k}={v:.3g}" for k, v in factors.items()))
    for name, f in factors.items():
        assert f > 1.0, (name, f)


# ---------------------------------------------------------------------------------------------- the C ABI without a GPU

def test_mlboot_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "aecf_hip.h")).read()
    declared = set(re.findall(r"\b(aecf_[a-z_0-9]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOL_NAMES
        assert hasattr(lib, name)
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10
    assert "#define AECF_ABI_VERSION 10" in header and "multi-label bootstrap" in header
    src = open(os.path.join(ROOT, "aecf_amd", "csrc", "aecf_mlboot.hip")).read()
    assert f"MLB_K = {M.K};" in src and f"MLB_TAG = 0x{B.TAG:x}u;" in src         # the sizes the cases are built around
    assert "aecf_mlboot.hip" in open(os.path.join(ROOT, "aecf_amd", "csrc", "Makefile")).read()


def _al(v):
    return (v + 255) // 256 * 256


def test_workspace_bytes_match_the_documented_layout(lib):
    for n_all, C in ((1, 1), (65, 3), (2049, 17), (65536, 80), (1 << 24, 16)):
        assert lib.aecf_mlboot_workspace_bytes(n_all, C) == lib.aecf_mlmetrics_workspace_bytes(n_all, C) > 0
    for n_all, C in ((0, 3), (5, 0), (5, 4097), ((1 << 24) + 1, 1), (65537, 4096)):
        assert lib.aecf_mlboot_workspace_bytes(n_all, C) == 0
    for n_all, R in ((1, 1), (63, 63), (65, 64), (1025, 65), (25600, 4096)):
        assert lib.aecf_mlboot_draw_workspace_bytes(n_all, R) == _al(4 * n_all * ((R + 63) // 64 * 64)), (n_all, R)
    for n_all, R in ((0, 5), (5, 0), (5, 4097), ((1 << 24) + 1, 5), (-1, 5)):
        assert lib.aecf_mlboot_draw_workspace_bytes(n_all, R) == 0


def _order(lib, n=300, C=4, dtype=1, x=BAD, y=BAD, thr=BAD, cc=BAD, order=BAD, ws=BAD, wsb=1 << 30):
    return lib.aecf_mlboot_order(n, C, dtype, x, y, thr, cc, order, ws, wsb, None)


def _draw(lib, n=300, R=65, r0=0, seed=1, counts=None, w=BAD, sat=BAD, ws=BAD, wsb=1 << 30):
    return lib.aecf_mlboot_draw(n, R, r0, seed, counts, w, sat, ws, wsb, None)


def _walk(lib, n=300, C=4, R=65, cc=BAD, order=BAD, w=BAD, stats=BAD):
    return lib.aecf_mlboot_walk(n, C, R, cc, order, w, stats, None)


def test_order_refuses_in_the_documented_order(lib):
    assert _order(lib, n=0, C=5000, dtype=7, x=None, wsb=0) == BAD_DIMS
    assert _order(lib, C=0, dtype=7, x=None, wsb=0) == BAD_DIMS
    assert _order(lib, C=4097, x=None, wsb=0) == UNSUPPORTED
    assert _order(lib, n=(1 << 24) + 1, x=None, wsb=0) == UNSUPPORTED
    assert _order(lib, dtype=3, x=None, wsb=0) == UNSUPPORTED
    for name in ("x", "y", "thr", "cc", "order", "ws"):
        assert _order(lib, wsb=0, **{name: None}) == NULL_POINTER, name
    assert _order(lib, wsb=lib.aecf_mlboot_workspace_bytes(300, 4) - 1) == WORKSPACE


def test_draw_refuses_in_the_documented_order(lib):
    assert _draw(lib, n=0, R=5000, w=None, wsb=0) == BAD_DIMS
    assert _draw(lib, R=0, n=1 << 25, w=None, wsb=0) == BAD_DIMS
    assert _draw(lib, r0=-1, R=5000, w=None, wsb=0) == BAD_DIMS
    assert _draw(lib, r0=(1 << 31) - 64, R=5000, w=None, wsb=0) == BAD_DIMS          # replicate0 + replicates > 2**31
    assert _draw(lib, R=4097, w=None, wsb=0) == UNSUPPORTED
    assert _draw(lib, n=(1 << 24) + 1, w=None, wsb=0) == UNSUPPORTED
    for name in ("w", "sat", "ws"):
        assert _draw(lib, wsb=0, **{name: None}) == NULL_POINTER, name
    assert _draw(lib, wsb=_al(4 * 300 * 128) - 1) == WORKSPACE
    assert _draw(lib, counts=BAD, w=None, ws=None, wsb=0) == NULL_POINTER             # counts given: no workspace, the rest still checked


def test_walk_refuses_in_the_documented_order(lib):
    assert _walk(lib, n=0, C=5000, cc=None) == BAD_DIMS
    assert _walk(lib, R=0, C=5000, cc=None) == BAD_DIMS
    assert _walk(lib, C=4097, cc=None) == UNSUPPORTED
    assert _walk(lib, R=4097, cc=None) == UNSUPPORTED
    for name in ("cc", "order", "w", "stats"):
        assert _walk(lib, **{name: None}) == NULL_POINTER, name


def test_python_refuses_cpu_tensors_and_malformed_arguments():
    torch = pytest.importorskip("torch")
    from aecf_amd import metrics
    x, y = torch.zeros(4, 3), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        metrics.bootstrap_metrics(x, y)
    with pytest.raises(RuntimeError, match="ROCm device"):
        metrics.bootstrap_compare(x, x, y)
    with pytest.raises(ValueError, match="confidence"):
        metrics.bootstrap_metrics(x, y, confidence=1.0)
    assert metrics.__all__ == ["multilabel_metrics"]
    assert metrics._boot_chunk(2048) == 4096 and metrics._boot_chunk(65536) == 1024 and metrics._boot_chunk(1 << 24) == 64
