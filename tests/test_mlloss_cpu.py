"""CPU-only tests of the multi-label classification loss: the float64 restatement of tests/mlloss_cases.py against torch's
binary_cross_entropy_with_logits, against a literal transcription of the published asymmetric loss and against its own closed
form; a float32 emulation of the kernels' arithmetic inside the derived bounds, and outside them for every broken rule; the
aecf_mlloss_* entry points declared, bound and exported with the ABI version still 10, their workspace answers and their
refusals in the documented order before any pointer is read (the pointers handed over here are bogus)."""
import os
import re

import numpy as np
import pytest

from aecf_amd import _lib
from tests import mlloss_cases as M

torch = pytest.importorskip("torch")
F = torch.nn.functional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["aecf_mlloss_workspace_bytes", "aecf_mlloss_forward", "aecf_mlloss_backward"]
BAD = 0x10          # never dereferenced: every call below must refuse first
BAD_DIMS, UNSUPPORTED, NULL_POINTER, WORKSPACE = -1, -2, -3, -4
FINITE = [c for c in M.CASE_IDS if not c.startswith("specials")]
f64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _restated(c, reduction="mean", a=None, b=None):
    """(loss, gradient) of the float64 torch restatement by autograd; a, b: other scales than the case's folded ones"""
    x = torch.tensor(c.x, dtype=f64, requires_grad=True)
    a = torch.tensor(c.a, dtype=f64) if a is None else a
    b = torch.tensor(c.b, dtype=f64) if b is None else b
    el = M.restate_elements(x, torch.tensor(c.t, dtype=f64), torch.tensor(c.valid), a, b, c.form)
    n = float(c.valid.sum())
    loss = el.sum() / n if reduction == "mean" and n > 0 else el.sum()
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


# ---------------------------------------------------------------------------------------------- the restatement

@pytest.mark.parametrize("name", [c for c in FINITE if M.CASES[c][0] in ("bce", "bce_w", "bce_soft")])
def test_restatement_against_torch_bce(name):
    """gamma = 0, margin = 0: F.binary_cross_entropy_with_logits in float64 within 1e-12 on value and gradient, with weight,
    pos_weight and soft (smoothed) targets, over the valid elements.  The scales are a = w p and b = w formed in float64 here:
    the float32 fold of the library rounds a once, which is no part of the restatement."""
    c = M.case(name)
    a = b = None
    if c.pos_weight is not None:
        b = torch.tensor(c.class_weight, dtype=f64)
        a = b * torch.tensor(c.pos_weight, dtype=f64)
    loss, grad = _restated(c, a=a, b=b)
    valid = torch.tensor(c.valid)
    x = torch.tensor(c.x, dtype=f64, requires_grad=True)
    t = torch.where(valid, torch.tensor(c.t, dtype=f64), torch.zeros((), dtype=f64))
    tp = t * (1.0 - c.form.eps) + c.form.eps / 2
    w = None if c.class_weight is None else torch.tensor(c.class_weight, dtype=f64)
    p = None if c.pos_weight is None else torch.tensor(c.pos_weight, dtype=f64)
    el = F.binary_cross_entropy_with_logits(x, tp, weight=w, pos_weight=p, reduction="none")
    ref = torch.where(valid, el, torch.zeros((), dtype=f64)).sum() / valid.sum()
    ref.backward()
    assert abs(loss - float(ref.detach())) <= 1e-12
    assert np.abs(grad - x.grad.numpy()).max() <= 1e-12


def test_naive_log1p_of_minus_sigma_misses_the_margin():
    """the reason for the stable forms: log1p(-sigmoid(x)) for log(1 - s) is off by more than 1e-12 at large x in float64"""
    x = torch.tensor([30.0, 33.0, 36.0], dtype=f64)
    naive = -torch.log1p(-torch.sigmoid(x))
    stable = -F.logsigmoid(-x)
    assert float((naive - stable).abs().max()) > 1e-12
    assert float((F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none") - stable).abs().max()) <= 1e-12


@pytest.mark.parametrize("name", ["asl_64x15_some", "asl_2049x80_class", "asl1_257x17_some", "asl1_3x4096"])
def test_restatement_against_the_published_asymmetric_loss(name):
    """Ridnik et al. 2021, written in probability space from the paper without its 1e-8 clamps, hard targets, moderate logits
    (|x| <= 8): p_m = max(p - m, 0), L+ = (1 - p)^g+ log p, L- = p_m^g- log(1 - p_m)"""
    c = M.case(name)
    assert np.abs(c.x).max() <= 8 and c.pos_weight is None
    loss, grad = _restated(c, "sum")
    valid = torch.tensor(c.valid)
    x = torch.tensor(c.x, dtype=f64, requires_grad=True)
    y = torch.where(valid, torch.tensor(c.t, dtype=f64), torch.zeros((), dtype=f64))
    p = torch.sigmoid(x)
    xs_neg = (1 - p + c.form.m).clamp(max=1)
    los = y * torch.log(p) + (1 - y) * torch.log(xs_neg)
    pt = p * y + xs_neg * (1 - y)
    los = los * torch.pow(1 - pt, c.form.gp * y + c.form.gn * (1 - y))
    ref = -torch.where(valid, los, torch.zeros((), dtype=f64)).sum()
    ref.backward()
    assert abs(loss - float(ref.detach())) <= 1e-12 * max(1.0, abs(loss))
    assert np.abs(grad - x.grad.numpy()).max() <= 1e-12


@pytest.mark.parametrize("name", FINITE)
def test_autograd_against_closed_form(name):
    c = M.case(name)
    ref = M.reference(c)
    loss, grad = _restated(c)
    assert abs(loss - ref.loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.abs(grad - ref.grad).max() <= 1e-12
    assert not grad[ref.zero_grad].any() and not ref.grad[ref.zero_grad].any()


def test_closed_form_limits_at_the_specials():
    """loss 0 or +inf and a finite gradient at +-inf; NaN at the valid NaN logit only; nothing from the ignored logits"""
    for name in [n for n in M.CASE_IDS if n.startswith("specials")]:
        c = M.case(name)
        el = M.closed_form(c.x, c.t, c.valid, c.a, c.b, c.form)
        nan = np.zeros_like(c.valid)
        nan[3, M.NAN_CLASS] = True
        assert np.array_equal(np.isnan(el.loss), nan) and np.array_equal(np.isnan(el.grad), nan)
        assert np.isfinite(el.grad[~nan]).all()
        inf_rows = np.isinf(c.x) & c.valid
        assert set(np.unique(el.loss[inf_rows])) <= {0.0, np.inf} or c.form.m > 0
        assert not el.loss[~c.valid].any() and not el.grad[~c.valid].any()
        z = M.zeroed_ignored(c)
        el0 = M.closed_form(z.x, z.t, z.valid, z.a, z.b, z.form)
        assert np.array_equal(el.loss, el0.loss, equal_nan=True) and np.array_equal(el.grad, el0.grad, equal_nan=True)


# ---------------------------------------------------------------------------------------------- float32 emulation and the bounds

@pytest.mark.parametrize("dtype", M.DTYPES)
@pytest.mark.parametrize("name", M.CASE_IDS)
def test_float32_emulation_is_inside_the_bounds(name, dtype):
    """the kernels' operations in float32 numpy stay inside the derived bounds; the emulation adds a class in one chain of n
    rows, so the bound is taken for that chain length"""
    c = M.case(name, dtype)
    for reduction in ("mean", "sum"):
        ref, em = M.reference(c, reduction, n_chain=c.x.shape[0]), M.emulate(c, reduction)
        M.check_close(em["loss"], ref.loss, ref.loss_bound, f"{name} loss")
        M.check_close(em["per_class"], ref.per_class, ref.per_class_bound, f"{name} per class")
        M.check_close(em["grad"], ref.grad, ref.grad_bound, f"{name} gradient")
        assert not em["grad"][ref.zero_grad].any()


def _factor(got, want, bound):
    """largest error over bound; inf where a NaN or an infinity stands at another place than the reference's"""
    got, want, bound = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (got, want, bound)))
    if not np.array_equal(np.isnan(got), np.isnan(want)) or not np.array_equal(np.isinf(got), np.isinf(want)):
        return float("inf")
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - want[fin]) / np.maximum(bound[fin], 1e-300)).max())


def test_broken_rules_leave_the_bound():
    """Each broken rule, emulated in float32, moves a named output out of its derived bound.  The factors (error over bound,
    printed below): ignored elements counted in N 1.9e4 (loss, bce_w_257x17_some); ignored elements excluded by a product with
    0, NaN logits there: inf (gradient, specials_bce_w: NaN where an exact zero belongs); pos_weight on the negatives 4.1e4
    (loss, bce_w_257x17_some); the margin on the positives 8.7e5 (loss, asl_64x15_some); the focal factor not differentiated
    3.0e5 (gradient, focal_257x17); smoothing before the validity test 9.4e3 (loss, bce_soft_64x15_some with unknown targets of
    -0.01); 1 - s by subtraction inf (loss, logits of 20 and above: log 0); the mean over the local N of two shards 38
    (loss, bce_w_257x17_some split 100 / 157)."""
    factors = {}
    c = M.case("bce_w_257x17_some")
    ref = M.reference(c)
    factors["count_ignored"] = _factor(M.emulate(c, rule="count_ignored")["loss"], ref.loss, ref.loss_bound)
    factors["pos_weight_on_negatives"] = _factor(M.emulate(c, rule="pos_weight_on_negatives")["loss"], ref.loss, ref.loss_bound)
    shards = [c._replace(x=c.x[lo:hi], t=c.t[lo:hi], valid=c.valid[lo:hi]) for lo, hi in ((0, 100), (100, 257))]
    assert shards[0].valid.sum() != shards[1].valid.sum() * 100 / 157
    local = np.mean([np.float64(M.emulate(s)["loss"]) for s in shards])
    factors["local_mean"] = _factor(local, ref.loss, M.reference(c, world=2).loss_bound)
    s = M.case("specials_bce_w")
    rs = M.reference(s)
    factors["ignore_by_product"] = _factor(M.emulate(s, rule="ignore_by_product")["grad"], rs.grad, rs.grad_bound)
    a = M.case("asl_64x15_some")
    ra = M.reference(a)
    factors["margin_on_positives"] = _factor(M.emulate(a, rule="margin_on_positives")["loss"], ra.loss, ra.loss_bound)
    fc = M.case("focal_257x17")
    rf = M.reference(fc)
    factors["focal_not_differentiated"] = _factor(M.emulate(fc, rule="focal_not_differentiated")["grad"], rf.grad, rf.grad_bound)
    so = M.case("bce_soft_64x15_some")
    so = so._replace(t=np.where(so.valid, so.t, np.float32(-0.01)).astype(np.float32))
    rso = M.reference(so)
    factors["smooth_ignored"] = _factor(M.emulate(so, rule="smooth_ignored")["loss"], rso.loss, rso.loss_bound)
    b = M.case("bce_64x15")
    b = b._replace(x=(20.0 + np.abs(b.x)).astype(np.float32))
    rb = M.reference(b)
    factors["one_minus_sigma_by_subtraction"] = _factor(M.emulate(b, rule="one_minus_sigma_by_subtraction")["loss"], rb.loss, rb.loss_bound)
    print("mlloss broken-rule factors: " + " ".join(f"{k}={v:.3g}" for k, v in factors.items()))
    assert set(factors) == set(M.RULES)
    for name, f in factors.items():
        assert f > 1.0, (name, f)
    # the controls: the same outputs of the unbroken emulation are inside
    for case_, ref_ in ((c, ref), (s, rs), (a, ra), (fc, rf), (so, rso), (b, rb)):
        em = M.emulate(case_)
        assert _factor(em["loss"], ref_.loss, ref_.loss_bound) <= 1.0 and _factor(em["grad"], ref_.grad, ref_.grad_bound) <= 1.0


# ---------------------------------------------------------------------------------------------- the C ABI without a GPU

def test_mlloss_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "aecf_hip.h")).read()
    declared = set(re.findall(r"\b(aecf_[a-z_0-9]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in _lib.SYMBOL_NAMES
        assert hasattr(lib, name)
    assert lib.aecf_abi_version() == 10 and _lib.AECF_ABI_VERSION == 10
    assert "#define AECF_ABI_VERSION 10" in header
    for macro, value in (("AECF_MLLOSS_U8", 3), ("AECF_MLLOSS_I8", 4), ("AECF_MLLOSS_MEAN", 0), ("AECF_MLLOSS_SUM", 1)):
        assert f"#define {macro} {value}" in header and getattr(_lib, macro) == value
    assert "aecf_mlloss.hip" in open(os.path.join(ROOT, "aecf_amd", "csrc", "Makefile")).read()


def test_workspace_bytes_match_the_documented_layout(lib):
    shapes = sorted({(n, C) for _, n, C, _ in M.CASES.values()} | {(65536, 80), (65536, 4096), (1 << 30, 1), (262144, 4096)})
    for n, C in shapes:
        assert lib.aecf_mlloss_workspace_bytes(n, C) == M.workspace_layout(n, C) > 0, (n, C)
    assert M.row_blocks(2049, 80) == (11, 187) and M.row_blocks(65536, 4096) == (256, 256) and M.row_blocks(64, 15) == (1, 64)
    # outside the served limits, or no shape at all: 0
    for n, C in ((0, 3), (5, 0), (-1, 3), (5, 4097), ((1 << 30) + 1, 1), (262145, 4096)):
        assert lib.aecf_mlloss_workspace_bytes(n, C) == 0, (n, C)


def _forward(lib, n=64, C=15, dtype=1, ldtype=1, x=BAD, y=BAD, ps=None, ns=None, gp=0.0, gn=0.0, m=0.0, eps=0.0, red=0, st=BAD,
             tot=BAD, ws=BAD, wsb=1 << 30):
    return lib.aecf_mlloss_forward(n, C, dtype, ldtype, x, y, ps, ns, gp, gn, m, eps, red, st, tot, ws, wsb, None)


def _backward(lib, n=64, C=15, dtype=1, ldtype=1, x=BAD, y=BAD, ps=None, ns=None, gp=0.0, gn=0.0, m=0.0, eps=0.0, red=0, tot=BAD,
              up=None, factor=1.0, dx=BAD):
    return lib.aecf_mlloss_backward(n, C, dtype, ldtype, x, y, ps, ns, gp, gn, m, eps, red, tot, up, factor, dx, None)


def test_forward_refuses_in_the_documented_order(lib):
    bad = dict(C=5000, dtype=7, x=None, wsb=0)                   # everything after the sizes is wrong too
    assert _forward(lib, n=0, **bad) == BAD_DIMS
    assert _forward(lib, **{**bad, "C": 0}) == BAD_DIMS
    for opt in (dict(gp=-1.0), dict(gn=float("nan")), dict(gp=float("inf")), dict(m=1.0), dict(m=-0.1), dict(eps=1.0), dict(red=2)):
        assert _forward(lib, **bad, **opt) == BAD_DIMS, opt
    assert _forward(lib, C=4097, x=None, wsb=0) == UNSUPPORTED
    assert _forward(lib, n=262145, C=4096, x=None, wsb=0) == UNSUPPORTED
    assert _forward(lib, dtype=3, x=None, wsb=0) == UNSUPPORTED
    assert _forward(lib, ldtype=5, x=None, wsb=0) == UNSUPPORTED
    assert _forward(lib, ldtype=-1, x=None, wsb=0) == UNSUPPORTED
    for name in ("x", "y", "st", "tot", "ws"):
        assert _forward(lib, wsb=0, **{name: None}) == NULL_POINTER, name
    assert _forward(lib, wsb=M.workspace_layout(64, 15) - 1) == WORKSPACE
    assert _forward(lib, ps=BAD, ns=BAD, wsb=0) == WORKSPACE      # the scale vectors may be NULL or not: never read before this


def test_backward_refuses_in_the_documented_order(lib):
    bad = dict(C=5000, dtype=7, x=None)
    assert _backward(lib, n=-3, **bad) == BAD_DIMS
    for opt in (dict(gn=-0.5), dict(m=float("nan")), dict(eps=-0.1), dict(red=-1), dict(factor=float("nan")), dict(factor=float("inf"))):
        assert _backward(lib, **bad, **opt) == BAD_DIMS, opt
    assert _backward(lib, C=4097, x=None) == UNSUPPORTED
    assert _backward(lib, dtype=5, x=None) == UNSUPPORTED
    assert _backward(lib, ldtype=9, x=None) == UNSUPPORTED
    for name in ("x", "y", "tot", "dx"):
        assert _backward(lib, **{name: None}) == NULL_POINTER, name


def test_python_refuses_cpu_tensors_and_malformed_arguments():
    from aecf_amd import losses
    x, y = torch.zeros(4, 3), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.multilabel_loss(x, y)
    with pytest.raises(RuntimeError, match="ROCm device"):
        losses.class_balance_weights(y)
    with pytest.raises(ValueError, match="'mean' or 'sum'"):
        losses.MultilabelLoss(reduction="none")
    with pytest.raises(ValueError, match=r"margin must lie in \[0, 1\)"):
        losses.MultilabelLoss(margin=1.0)
    with pytest.raises(ValueError, match="gamma_neg must be finite and >= 0"):
        losses.MultilabelLoss(gamma_neg=-1.0)
    with pytest.raises(TypeError, match="gamma_pos must be a Python number"):
        losses.MultilabelLoss(gamma_pos="2")
    with pytest.raises(ValueError, match="pos_weight must be finite and not negative"):
        losses.MultilabelLoss(pos_weight=[1.0, -2.0])
    crit = losses.MultilabelLoss(pos_weight=[1.0, 2.0, 3.0], gamma_neg=4.0, margin=0.05)
    assert crit.pos_weight.dtype == torch.float32 and crit.class_weight is None and "margin=0.05" in repr(crit)
    assert (losses.MLLOSS_MAX_CLASSES, losses.MLLOSS_MAX_ELEMENTS) == (M.MAX_CLASSES, M.MAX_ELEMENTS)
