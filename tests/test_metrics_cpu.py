"""CPU-only tests of the multi-label evaluation: the float64 restatement of tests/metrics_cases.py against sklearn on every case
without NaN and against the reference's own ``calculate_metrics`` (fixture g12); the aecf_mlmetrics_* entry points declared,
bound and exported with the ABI version still 10, their workspace answers and their refusals in the documented order before
any pointer is read (the pointers handed over here are bogus); and the broken rules the bounds must catch."""
import os
import re

import numpy as np
import pytest

from aecf_amd import _lib
from tests import metrics_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["aecf_mlmetrics_workspace_bytes", "aecf_mlmetrics_prepare", "aecf_mlmetrics_counts", "aecf_mlmetrics_finalize"]
BAD = 0x10          # never dereferenced: every call below must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4
NO_NAN = [c for c in M.CASE_IDS if c != "specials"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------- the restatement

@pytest.mark.parametrize("name", NO_NAN)
def test_restatement_against_sklearn(name):
    """average_precision_score, roc_auc_score and f1_score per class within 1e-12 (sklearn sums in its own order).  The
    predictions handed to f1_score are ``logit > 0``, this project's documented rule at threshold 0.5."""
    metrics = pytest.importorskip("sklearn.metrics")
    s, y, _ = M.case(name)
    r = M.restated(name)
    for c in range(s.shape[1]):
        yc, sc = y[:, c].astype(int), s[:, c].astype(np.float64)
        if yc.sum() == 0:
            assert r["ap"][c] == 0.0 and np.isnan(r["auroc"][c]) and r["f1"][c] == 0.0
            continue
        assert abs(metrics.average_precision_score(yc, sc) - r["ap"][c]) <= 1e-12, (name, c)
        if yc.sum() < len(yc):
            assert abs(metrics.roc_auc_score(yc, sc) - r["auroc"][c]) <= 1e-12, (name, c)
        else:
            assert np.isnan(r["auroc"][c])
        assert abs(metrics.f1_score(yc, (sc > 0).astype(int), zero_division=0) - r["f1"][c]) <= 1e-12, (name, c)
    assert r["n_invalid"].sum() == 0 and np.array_equal(r["n_pos"], y.sum(0))


def test_restatement_counts_are_the_pairwise_definition():
    """the sort-and-search counts of ``restate`` against the O(n^2) definition, on the specials case (NaN, +-inf, +-0, denormals)"""
    s, y, _ = M.case("specials")
    r = M.restated("specials")
    assert r["n_invalid"].min() > 0
    for c in range(s.shape[1]):
        valid = ~np.isnan(s[:, c])
        pos = valid & y[:, c]
        k = s[valid, c]
        pk = s[pos, c]
        for i in np.flatnonzero(pos):
            want = [(k >= s[i, c]).sum(), (k > s[i, c]).sum(), (pk >= s[i, c]).sum(), (pk > s[i, c]).sum()]
            assert list(r["counts"][:, c, i]) == want
        assert not r["counts"][:, c, ~pos].any()
    # class 3 holds +0 on the positives and -0 on the negatives only: one tie
    npos, nval = r["n_pos"][3], s.shape[0] - r["n_invalid"][3]
    assert abs(r["ap"][3] - npos / nval) <= 3 * M.U and r["auroc"][3] == 0.5


def test_restatement_reproduces_the_reference_fixture(golden_dir):
    """g12: the reference's calculate_metrics (sklearn on float32 sigmoids) on logits where the sigmoid keeps order and ties"""
    z = np.load(os.path.join(golden_dir, "g12_metrics.npz"))
    r = M.restate(z["logits"], z["labels"])
    assert z["logits"].shape == (300, 6) and r["n_pos"][4] == 0 and r["f1"][5] == 0.0
    assert abs(r["map"] - float(z["map"])) <= 1e-12
    assert abs(r["macro_f1"] - float(z["macro_f1"])) <= 1e-12
    assert np.abs(r["f1"] - z["f1"]).max() <= 1e-12


# ---------------------------------------------------------------------------------------------- broken rules leave the bound

def _factor(broken, right, bound):
    return abs(broken - right) / bound


def test_broken_rules_leave_the_bound():
    """Each broken rule moves its output by many times the bound that output is held to.  The factors (error over bound, printed
    below): > for >= in ge_all 1.1e13 (quantised, mAP); ties by position 1.1e11 in the float64 numpy form of today's
    mean_average_precision and 9.0e10 in the function itself on CPU tensors, whose sort is not stable (quantised, mAP); NaN kept as a key 1.9e13 (specials, mAP); negatives as anchors 1.8e14 (quantised, mAP); the 1/2 dropped 9.5e12
    (quantised, macro AUROC); F1 over the invalid rows 1.3e13 (specials, macro F1)."""
    s, y, _ = M.case("quantised")
    right = M.restated("quantised")
    n, C = s.shape
    b_map = M.macro_bound(M.ap_bound(n), C)
    factors = {}
    factors["gt_for_ge"] = _factor(M.restate(s, y, rule="gt_for_ge")["map"], right["map"], b_map)
    factors["position_ties"] = _factor(M.position_tie_map(s, y), right["map"], b_map)
    torch = pytest.importorskip("torch")
    from aecf_amd.train_xray import mean_average_precision             # the function itself, on CPU tensors in float64
    today = mean_average_precision(torch.from_numpy(s.astype(np.float64)), torch.from_numpy(y.astype(np.float64)))
    factors["mean_average_precision"] = _factor(today, right["map"], b_map)
    factors["neg_anchors"] = _factor(M.restate(s, y, rule="neg_anchors")["map"], right["map"], b_map)
    factors["no_half"] = _factor(M.restate(s, y, rule="no_half")["macro_auroc"], right["macro_auroc"], M.macro_bound(M.AUROC_BOUND, C))
    s2, y2, _ = M.case("specials")
    right2 = M.restated("specials")
    n2, C2 = s2.shape
    factors["nan_key"] = _factor(M.restate(s2, y2, rule="nan_key")["map"], right2["map"], M.macro_bound(M.ap_bound(n2), C2))
    factors["f1_invalid"] = _factor(M.restate(s2, y2, rule="f1_invalid")["macro_f1"], right2["macro_f1"], M.macro_bound(M.F1_BOUND, C2))
    print("metrics broken-rule factors: " + " ".join(f"{k}={v:.3g}" for k, v in factors.items()))
    for name, f in factors.items():
        assert f > 1.0, (name, f)


def test_position_ties_on_a_tie_free_case_agree():
    """the control: without ties today's mean_average_precision formula and the tie-exact one are the same number"""
    s, y, _ = M.case("a_plus")
    assert len(np.unique(s[:, 0])) == s.shape[0]
    assert abs(M.position_tie_map(s, y) - M.restated("a_plus")["map"]) <= M.macro_bound(M.ap_bound(s.shape[0]), 3) + 64 * M.U


# ---------------------------------------------------------------------------------------------- the C ABI without a GPU

def test_mlmetrics_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "aecf_hip.h")).read()
    declared = set(re.findall(r"\b(aecf_[a-z_0-9]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOL_NAMES
        assert hasattr(lib, name)
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10
    assert "#define AECF_ABI_VERSION 10" in header
    src = open(os.path.join(ROOT, "aecf_amd", "csrc", "aecf_metrics.hip")).read()
    assert f"MLM_A = {M.A};" in src and f"MLM_K = {M.K};" in src          # the sizes the cases are built around


def _layout(n_all, C):
    al = lambda v: (v + 255) // 256 * 256
    nch = (n_all + 63) // 64
    Np = nch * 64
    return 3 * al(4 * C * Np) + al(8 * C * nch) + 2 * al(4 * C * nch)


def test_workspace_bytes_match_the_documented_layout(lib):
    for n_all, C in ((1, 1), (63, 3), (64, 3), (65, 3), (2049, 17), (65536, 80), (1 << 24, 16), (65536, 4096)):
        assert lib.aecf_mlmetrics_workspace_bytes(n_all, C) == _layout(n_all, C), (n_all, C)
    # outside the served limits, or no shape at all: 0
    for n_all, C in ((0, 3), (5, 0), (-1, 3), (5, 4097), ((1 << 24) + 1, 1), (65537, 4096)):
        assert lib.aecf_mlmetrics_workspace_bytes(n_all, C) == 0, (n_all, C)


def _prepare(lib, n=300, C=4, dtype=1, x=BAD, y=BAD, cc=BAD, ws=BAD, wsb=1 << 30):
    return lib.aecf_mlmetrics_prepare(n, C, dtype, x, y, cc, ws, wsb, None)


def _counts(lib, n=300, C=4, off=0, rows=300, cc=BAD, out=BAD, ws=BAD, wsb=1 << 30):
    return lib.aecf_mlmetrics_counts(n, C, off, rows, cc, out, ws, wsb, None)


def _finalize(lib, n=300, C=4, off=0, rows=300, thr=0.0, cc=BAD, cn=BAD, sh=BAD, ws=BAD, wsb=1 << 30):
    return lib.aecf_mlmetrics_finalize(n, C, off, rows, thr, cc, cn, sh, ws, wsb, None)


def test_prepare_refuses_in_the_documented_order(lib):
    assert _prepare(lib, n=0, C=5000, dtype=7, x=None, wsb=0) == BAD_DIMS
    assert _prepare(lib, C=0, dtype=7, x=None, wsb=0) == BAD_DIMS
    assert _prepare(lib, C=4097, x=None, wsb=0) == UNSUPPORTED
    assert _prepare(lib, n=(1 << 24) + 1, x=None, wsb=0) == UNSUPPORTED
    assert _prepare(lib, n=65537, C=4096, x=None, wsb=0) == UNSUPPORTED
    assert _prepare(lib, dtype=3, x=None, wsb=0) == UNSUPPORTED
    for name in ("x", "y", "cc", "ws"):
        assert _prepare(lib, wsb=0, **{name: None}) == NULL_POINTER, name
    assert _prepare(lib, wsb=_layout(300, 4) - 1) == WORKSPACE


def test_counts_refuses_in_the_documented_order(lib):
    assert _counts(lib, n=0, C=5000, cc=None, wsb=0) == BAD_DIMS
    assert _counts(lib, rows=-1, C=5000, cc=None, wsb=0) == BAD_DIMS
    assert _counts(lib, off=-1, rows=10, C=5000, cc=None, wsb=0) == BAD_DIMS
    assert _counts(lib, off=1, rows=300, C=5000, cc=None, wsb=0) == BAD_DIMS          # row_offset + rows > n_all
    assert _counts(lib, off=301, rows=0, C=5000, cc=None, wsb=0) == BAD_DIMS
    assert _counts(lib, C=4097, cc=None, wsb=0) == UNSUPPORTED
    for name in ("cc", "out", "ws"):
        assert _counts(lib, wsb=0, **{name: None}) == NULL_POINTER, name
    assert _counts(lib, wsb=16) == WORKSPACE
    assert _counts(lib, rows=0, out=None, wsb=16) == WORKSPACE                        # rows == 0 may leave counts NULL ...
    assert _counts(lib, off=300, rows=0, out=None) == 0                               # ... and launches nothing: AECF_OK, no GPU


def test_finalize_refuses_in_the_documented_order(lib):
    assert _finalize(lib, n=0, C=5000, cc=None, wsb=0) == BAD_DIMS
    assert _finalize(lib, thr=float("nan"), C=5000, cc=None, wsb=0) == BAD_DIMS
    assert _finalize(lib, off=200, rows=101, C=5000, cc=None, wsb=0) == BAD_DIMS
    assert _finalize(lib, C=4097, cc=None, wsb=0) == UNSUPPORTED
    for name in ("cc", "cn", "sh", "ws"):
        assert _finalize(lib, wsb=0, **{name: None}) == NULL_POINTER, name
    assert _finalize(lib, rows=0, cn=None, wsb=16) == WORKSPACE                       # counts may be NULL where rows == 0
    assert _finalize(lib, wsb=16) == WORKSPACE


def test_python_refuses_cpu_tensors_and_malformed_arguments():
    torch = pytest.importorskip("torch")
    from aecf_amd import metrics
    x, y = torch.zeros(4, 3), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        metrics.multilabel_metrics(x, y)
    assert metrics.__all__ == ["multilabel_metrics"]
