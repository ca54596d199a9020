"""The calibration's restatement, emulation and bounds on the CPU (tests/calibration_cases.py): the restatement against
sklearn's calibration_curve, brier_score_loss and log_loss and against a hand-worked ECE, the fit's rule in float64 against
scipy's minimiser, the float32 emulation of the kernels inside the derived bounds, every broken rule outside them, the fit
cases' optima inside the box by a margin, and the presence of the new symbols and functions."""
import math

import numpy as np
import pytest

from tests import calibration_cases as K


def _sklearn():
    try:
        from sklearn.calibration import calibration_curve
        from sklearn.metrics import brier_score_loss, log_loss
    except Exception as e:              # pragma: no cover - environment
        pytest.skip(f"sklearn is not importable: {e}")
    return calibration_curve, brier_score_loss, log_loss


def _draw(n=5000, C=3, B=15, seed=11):
    g = np.random.default_rng(seed)
    x = (2.5 * g.standard_normal((n, C))).astype(np.float32)
    t = (g.random((n, C)) < 1.0 / (1.0 + np.exp(-0.7 * x))).astype(np.float32)
    return K.Case(x, t, B, None, None)


def test_symbols_and_python_surface_exist():
    """(fails on a tree without the feature: the functions and the library's symbols do not exist)"""
    from aecf_amd import _lib, metrics
    assert callable(metrics.multilabel_calibration) and callable(metrics.fit_calibration) and callable(metrics.calibration_edges)
    for name in ("aecf_mlcal_workspace_bytes", "aecf_mlcal_stats", "aecf_mlcal_fit_sums", "aecf_mlcal_fit_update"):
        assert name in _lib.SYMBOL_NAMES
    assert _lib.AECF_ABI_VERSION == 10


def test_bins_equal_sklearns_calibration_curve():
    calibration_curve, _, _ = _sklearn()
    c = _draw()
    ref = K.reference(c)
    p = 1.0 / (1.0 + np.exp(-c.x.astype(np.float64)))
    mismatches = 0
    for k in range(c.x.shape[1]):
        binids = np.searchsorted(np.linspace(0.0, 1.0, c.B + 1)[1:-1], p[:, k])          # sklearn's rule, written out
        mismatches += int((binids != K.bin_of(c.x[:, k], c.B)).sum())
        prob_true, prob_pred = calibration_curve(c.t[:, k], p[:, k], n_bins=c.B, strategy="uniform")
        cnt = ref.stats["bin_count"][k]
        filled = cnt > 0
        assert filled.sum() == prob_true.size
        assert np.array_equal(prob_true, ref.stats["bin_pos"][k][filled] / cnt[filled])
        assert np.abs(prob_pred - ref.stats["bin_conf"][k][filled] / cnt[filled]).max() <= 1e-14
    assert mismatches == 0


def test_brier_and_nll_equal_sklearns():
    _, brier_score_loss, log_loss = _sklearn()
    c = _draw(n=700)
    ref = K.reference(c)
    p = 1.0 / (1.0 + np.exp(-c.x.astype(np.float64)))
    for k in range(c.x.shape[1]):
        assert abs(ref.closing["brier_per_class"][k] - brier_score_loss(c.t[:, k], p[:, k])) <= 1e-12
        assert abs(ref.closing["nll_per_class"][k] - log_loss(c.t[:, k], p[:, k], labels=[0, 1])) <= 1e-12


def test_ece_of_a_hand_worked_example():
    """Twelve elements of one class in 4 bins (edges at p = 1/4, 1/2, 3/4), p (target):
         bin 0: 0.1 (0), 0.2 (0), 0.2 (1)     conf 0.5, pos 1, |gap| 0.5
         bin 1: 0.3 (0), 0.4 (1), 0.5 (0)     conf 1.2, pos 1, |gap| 0.2      (p = 0.5 lies ON an edge: the lower bin)
         bin 2: 0.6 (1), 0.7 (0), 0.7 (1)     conf 2.0, pos 2, |gap| 0.0
         bin 3: 0.8 (1), 0.9 (1), 0.9 (1)     conf 2.6, pos 3, |gap| 0.4
       ECE = (0.5 + 0.2 + 0.0 + 0.4) / 12 = 1.1 / 12;  MCE = max(0.5, 0.2, 0.0, 0.4) / 3 = 1 / 6."""
    p = np.array([0.1, 0.2, 0.2, 0.3, 0.4, 0.6, 0.7, 0.7, 0.5, 0.8, 0.9, 0.9])
    y = np.array([0, 0, 1, 0, 1, 1, 0, 1, 0, 1, 1, 1], dtype=np.float32)
    x = np.log(p / (1 - p)).astype(np.float32)
    x[8] = 0.0                                          # exactly on the edge log(2 / 2) = 0
    ref = K.reference(K.Case(x[:, None], y[:, None], 4, None, None))
    assert ref.stats["bin_count"][0].tolist() == [3, 3, 3, 3] and ref.stats["bin_pos"][0].tolist() == [1, 1, 2, 3]
    assert abs(ref.closing["ece"] - 1.1 / 12) <= 1e-7 and abs(ref.closing["ece_per_class"][0] - 1.1 / 12) <= 1e-7
    assert abs(ref.closing["mce"] - 1.0 / 6) <= 1e-7
    assert abs(ref.closing["macro_ece"] - ref.closing["ece"]) <= 1e-15


@pytest.mark.parametrize("dtype", K.DTYPES)
@pytest.mark.parametrize("name", K.CASE_IDS)
def test_emulation_inside_the_bounds(name, dtype):
    c = K.case(name, dtype)
    ref = K.reference(c, chain=c.x.shape[0])
    assert K.check_stats(K.emulate(c), ref, f"{name} {dtype}") <= 1.0
    g = K.garbage(c)                                    # garbage under unknown targets and in place of NaN logits: the same reference
    rg = K.reference(g, chain=c.x.shape[0])
    for k in K.STAT_NAMES:
        assert np.array_equal(rg.stats[k], ref.stats[k], equal_nan=True), k


RULE_CASES = {"edge_upper": "255x15_b15", "last_bin_loses_inf": "specials_b15", "nan_valid": "specials_b15",
              "unknown_negative": "255x15_b15", "ece_uniform_weight": "2049x17_b15", "div_scale": "255x15_b15",
              "bias_first": "255x15_b15", "mce_empty_bins": "255x15_b15"}


def test_every_broken_rule_leaves_the_bounds(capsys):
    assert set(RULE_CASES) == set(K.STAT_RULES)
    smallest = math.inf
    for rule, name in RULE_CASES.items():
        c = K.case(name)
        ref = K.reference(c, chain=c.x.shape[0])
        assert K.stats_ratio(K.emulate(c), ref) <= 1.0
        factor = K.stats_ratio(K.emulate(c, rule), ref)
        assert factor > 1.0, f"{rule} stays inside the bounds of {name}"
        smallest = min(smallest, factor)
    with capsys.disabled():
        print(f"\ncalibration: smallest error / bound of a broken statistics rule = {smallest:.3g}")
    assert smallest > 1.0


def test_workspace_and_geometry_restated():
    assert K.row_blocks(2048, 15) == (2, 1024) and K.row_blocks(3, 4096) == (1, 3)
    assert K.workspace_layout(2048, 15, 15) == 12032            # 2 slabs x 50 rows x 15 classes x 8 bytes = 12000, to 256
    assert K.edges(1).size == 0 and K.edges(2).tolist() == [0.0]
    e = K.edges(15)
    assert e.dtype == np.float32 and (np.diff(e) > 0).all() and e[7 - 1] < 0 < e[8 - 1]


# ---------------------------------------------------------------------------------------------- the fit

@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", K.FIT_CASE_IDS)
def test_fit_restatement_against_scipy(name, mode):
    """the rule in float64 (parameters kept in float64) ends at scipy's minimiser of the float64 NLL to 1e-9, interior cases"""
    try:
        from scipy.optimize import minimize
    except Exception as e:              # pragma: no cover - environment
        pytest.skip(f"scipy is not importable: {e}")
    c = K.fit_case(name)
    got = K.fit(c, mode, max_iter=64, round32=False)
    for i, classes in enumerate(K.problems(c, mode)):
        if len(classes) == 1 and classes[0] in c.degenerate:
            continue
        free = [0, 1] if mode == "platt" else [0]

        def parts(v):
            return K.true_nll(c, classes, *_theta(v, free))

        r = minimize(lambda v: parts(v)[0], np.array([1.0, 0.0])[free], jac=lambda v: parts(v)[1][free],
                     hess=lambda v: parts(v)[2][np.ix_(free, free)], method="trust-exact", options=dict(gtol=1e-10))
        # scipy stops where it can no longer predict an improvement of the float64 NLL, with a gradient of about 1e-6, i.e.
        # about 1e-7 from the optimum; ONE Newton step from its answer (float64 gradient and Hessian) removes that, and the
        # comparison to 1e-9 is made with the polished point -- and scipy's own answer is held to what it reaches.
        polished = r.x - np.linalg.solve(parts(r.x)[2][np.ix_(free, free)], parts(r.x)[1][free])
        assert np.abs(polished - r.x).max() <= 1e-6
        mine = np.array([got["scale"][i], got["bias"][i]])[free]
        assert got["converged"][i]
        assert np.abs(mine - polished).max() <= 1e-9, (mine, polished)
        assert np.abs(K.optimum(c, classes, mode)[free] - polished).max() <= 1e-9    # the cases file's own Newton optimum too


def _theta(v, free):
    th = np.array([1.0, 0.0])
    th[free] = v
    return th


@pytest.mark.parametrize("name", K.FIT_CASE_IDS)
def test_fit_cases_are_interior_by_a_margin(name):
    """every class not named degenerate has its float64 optimum inside the box by a factor 2 (scale) and by half (bias), it
    converges inside 32 iterations in float64 and in the float32 emulation, and lambda <= 1 when it does"""
    c = K.fit_case(name)
    for mode in K.MODES:
        runs = [K.fit(c, mode), K.fit(c, mode, arith="float32")]
        for i, classes in enumerate(K.problems(c, mode)):
            if len(classes) == 1 and classes[0] in c.degenerate:
                continue
            opt = K.optimum(c, classes, mode)
            assert 2 * K.BOX["scale"][0] <= opt[0] <= K.BOX["scale"][1] / 2 and abs(opt[1]) <= K.BOX["bias"][1] / 2, (mode, i, opt)
            for r in runs:
                assert r["fitted"][i] and r["converged"][i] and r["lam"][i] <= 1.0, (mode, i)
    use = K.used(c)
    for k, kind in c.degenerate.items():
        with np.errstate(invalid="ignore"):
            pos = (c.t[:, k] > 0) & use[:, k]
        if kind == "no_positive":
            assert use[:, k].any() and not pos.any()
        elif kind == "no_negative":
            assert pos.any() and pos.sum() == use[:, k].sum()
        elif kind == "non_finite":
            assert not use[:, k].any()
        else:
            xs = c.x[use[:, k], k]
            assert xs[pos[use[:, k]]].min() > xs[~pos[use[:, k]]].max()


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", K.FIT_CASE_IDS)
def test_fit_emulation_inside_the_bounds(name, mode):
    c = K.fit_case(name)
    for arith in ("float64", "float32"):
        assert K.check_fit(c, mode, K.fit(c, mode, arith=arith), f"{name} {mode} {arith}") <= 1.0


def test_every_broken_fit_rule_leaves_the_bounds(capsys):
    factors = {}
    c = K.fit_case("fit_512x3_shifted")                 # scale and bias coupled: without the cross term the steps zigzag
    assert K.fit_ratio(c, "platt", K.fit(c, "platt", arith="float32")) <= 1.0
    factors["h01_dropped"] = K.fit_ratio(c, "platt", K.fit(c, "platt", arith="float32", rule="h01_dropped"))
    c = K.fit_case("fit_2049x17")                       # classes of different sharpness: the mean of their scales is not the pooled one
    assert K.fit_ratio(c, "temperature", K.fit(c, "temperature", arith="float32")) <= 1.0
    factors["mean_of_class_fits"] = K.fit_ratio(c, "temperature", K.fit(c, "temperature", arith="float32", rule="mean_of_class_fits"))
    c = K.fit_case("fit_400x2_overconfident")           # the first trials overshoot and are rejected
    worst = 0.0
    for it in range(1, 9):
        good = K.fit(c, "class_temperature", max_iter=it, arith="float32")
        assert (good["nll_after"] <= good["nll_before"]).all()
        bad = K.fit(c, "class_temperature", max_iter=it, arith="float32", rule="rejected_trial_returned")
        for k in range(2):                              # the NLL of what the broken rule returns, against the first one
            L = K.true_nll(c, [k], float(bad["scale"][k]), float(bad["bias"][k]))[0]
            worst = max(worst, L / good["nll_before"][k])
    factors["rejected_trial_returned"] = worst          # (c): > 1 means the returned parameters are worse than the identity
    assert set(factors) == set(K.FIT_RULES)
    with capsys.disabled():
        print("\ncalibration: broken fit rules, error / bound: " + " ".join(f"{k}={v:.3g}" for k, v in factors.items()))
    assert all(v > 1.0 for v in factors.values()), factors
