"""Cases, float64 restatement and bounds of the multi-label classification loss (aecf_amd/losses.py: multilabel_loss,
aecf_mlloss_* of the library).

The definition (x a logit, t its target, s = sigmoid(x), class scales a_c and b_c, exponents gp and gn, margin m, smoothing eps):

    t' = t (1 - eps) + eps / 2        q = max(s - m, 0)
    l  = - a_c t' (1 - s)^gp log s  -  b_c (1 - t') q^gn log(1 - q)                        p^0 = 1 for every p
    dl/dx = - a_c t' (1 - s)^gp [ (1 - s) - gp s log s ]
            - b_c (1 - t') s (1 - s) [ gn q^(gn - 1) log(1 - q) - q^gn / (1 - q) ]         second line only where s - m > 0

``restate`` states it in float64 torch with the stable forms (logsigmoid(x) for log s, logsigmoid(-x) for log(1 - s),
sigmoid(-x) for 1 - s) and differentiates it with autograd; ``closed_form`` states loss and gradient in float64 numpy from the
formulas above, independently, with the limits at infinite logits taken by selects (autograd cannot: it forms 0 * inf there).

The bounds are derived from the operations of aecf_amd/csrc/aecf_mlloss.hip, not fitted to a run.  U = 2**-24 is the unit
roundoff of float32; a correctly rounded operation has relative error U.  HIP documents expf, logf and log1pf at 1 ulp, which is
at most 2 U relative.  All quantities below are non-negative, so sums do not cancel and relative errors of a sum are at most
the larger of the addends' plus U.  Per element, first order (the total is multiplied by 1.001 for the second-order terms):

    t'            3 U  (1 - eps and eps / 2 are rounded on the host, one fused or two separate roundings); 0 where eps = 0
    cp = a t'     d(t') + U          cn = b (1 - t')   t' d(t') / (1 - t') + 2 U
    e = exp(-|x|) 2 U                l1p = log1p(e)    2 U from e (e / ((1 + e) log1p(e)) <= 1) + 2 U = 4 U
    r = 1/(1+e)   1 + e: 2 U (e / (1 + e) <= 1 / 2), the division U: 3 U        e r: 6 U        so s and 1 - s: 6 U
    -log s, -log(1 - s) = max(-+x, 0) + l1p: 5 U
    (1 - s)^gp = exp(-gp nl1): the argument carries 5 U + U (gp rounded) + U (product) = 7 U relative, i.e. 7 U gp nl1 absolute,
                 which the exponential turns into expm1(7 U gp nl1) relative, + 2 U of its own; exactly 1 (no error) where gp = 0
    positive term (cp w) nls: d(cp) + d(w) + d(nls) + 2 U
    margin 0:  negative term (cn w') nl1 the same way with w' = exp(-gn nls)
    margin m:  q = s - m: absolute 6 U s + U m (m rounded) + U q;  1 - q = (1 - s) + m: absolute 6 U (1 - s) + U m + U (1 - q)
               -log(1 - q): absolute d(1 - q) / (1 - q) + 2 U |log(1 - q)|
               q^gn = exp(gn log q): argument absolute gn (d(q) / q + 4 U |log q|), through expm1, + 2 U
    l = P + N: the two absolute errors + U |l|
    gradient:  s nls: 12 U;  gp s nls: 14 U;  (1 - s) + gp s nls: 15 U;  positive part d(cp) + d(w) + 17 U, the margin-0 negative
               part alike;  with a margin inner = w/(1-q) + gn (w/q) nlq term by term as above, s (1 - s): 13 U, two more products
    scale:     upstream * factor (U), divided by N in float64 and rounded (U), the product with the element (U): 3 U
    16 bit:    one rounding into the logits' dtype: 2**-8 relative for bfloat16 (8 significant bits), 2**-11 for float16 (2**-25 absolute below its
               normal range)
Values below float32's normal range (|x| > 87.3) carry at most 2**-126 absolute, kept or flushed: TINY (cp + cn)(1 + |x|).

Sums.  A thread adds the losses of the rows it owns in float32, one after the other: at most rows_pb terms (``row_blocks``), so
the float32 part of a class sum is off by at most rows_pb U sum|l| beyond the element errors.  Everything above the thread is
float64 in a fixed order (at most rpi + 64 + 16 + C + world further additions): (n + C + 512) 2**-53 sum|l|.  The reduced loss
is rounded to float32 once (U), the per-class mean too.
"""
import functools
import math
from typing import NamedTuple, Optional

import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -120
SECOND_ORDER = 1.001
U16 = {"float32": 0.0, "bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}
MAX_CLASSES = 4096
MAX_ELEMENTS = 1 << 30


class Form(NamedTuple):
    gp: float = 0.0
    gn: float = 0.0
    m: float = 0.0
    eps: float = 0.0
    alpha: Optional[float] = None
    weights: bool = False           # random pos_weight and class_weight
    soft: bool = False              # soft float targets


FORMS = {
    "bce": Form(),
    "bce_w": Form(weights=True),
    "bce_soft": Form(eps=0.1, soft=True),
    "focal": Form(gp=2.0, gn=2.0, alpha=0.25),
    "asl": Form(gn=4.0, m=0.05),
    "asl1": Form(gp=1.0, gn=4.0, m=0.05),
    "frac": Form(gp=0.5, gn=0.5, m=0.2),
    "margin_only": Form(m=0.05),                # no power at all on the margin's path
}

# name -> (form, n, C, ignore plan)
CASES = {
    "bce_1x1": ("bce", 1, 1, "none"),
    "bce_64x15": ("bce", 64, 15, "none"),
    "bce_w_257x17_some": ("bce_w", 257, 17, "some"),
    "bce_w_2049x80_class": ("bce_w", 2049, 80, "class"),
    "bce_w_5x1031_some": ("bce_w", 5, 1031, "some"),
    "bce_soft_64x15_some": ("bce_soft", 64, 15, "some"),
    "bce_soft_3x4096": ("bce_soft", 3, 4096, "none"),
    "focal_257x17": ("focal", 257, 17, "none"),
    "focal_2049x80_some": ("focal", 2049, 80, "some"),
    "asl_64x15_some": ("asl", 64, 15, "some"),
    "asl_2049x80_class": ("asl", 2049, 80, "class"),
    "asl1_257x17_some": ("asl1", 257, 17, "some"),
    "asl1_3x4096": ("asl1", 3, 4096, "none"),
    "frac_257x17": ("frac", 257, 17, "none"),
    "frac_64x15_all": ("frac", 64, 15, "all"),
    "specials_bce_w": ("bce_w", 24, 5, "specials"),
    "specials_focal": ("focal", 24, 5, "specials"),
    "specials_asl1": ("asl1", 24, 5, "specials"),
    "specials_margin_only": ("margin_only", 24, 5, "specials"),
}
CASE_IDS = list(CASES)
DTYPES = ("float32", "bfloat16", "float16")
SPECIAL_VALUES = (0.0, -0.0, 20.0, -20.0, 88.7, -88.7, 104.0, -104.0, 1e4, -1e4, math.inf, -math.inf)
NAN_CLASS = 4                       # the class of the specials cases that holds the one valid NaN logit


def to_bf16(x: np.ndarray) -> np.ndarray:
    """float32 values rounded to the nearest bfloat16 (ties to even), as float32; infinities and NaN stay"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32).reshape(x.shape)
    return np.where(np.isfinite(x), r, x)


def quantise(x: np.ndarray, dtype: str) -> np.ndarray:
    if dtype == "bfloat16":
        return to_bf16(x)
    if dtype == "float16":
        return x.astype(np.float16).astype(np.float32)
    return x.astype(np.float32)


class Case(NamedTuple):
    form: Form
    x: np.ndarray                   # float32 [n, C], values of the case's dtype
    t: np.ndarray                   # float32 [n, C]; unknown: NaN or -1 (alternating)
    valid: np.ndarray               # bool [n, C]
    pos_weight: Optional[np.ndarray]
    class_weight: Optional[np.ndarray]
    a: np.ndarray                   # float32 [C], the folded scales (ones where there is no weight)
    b: np.ndarray


def fold(form: Form, pos_weight, class_weight, C: int):
    """a = w p (alpha or 1), b = w ((1 - alpha) or 1), in float32 as aecf_amd.losses folds them"""
    one = np.ones(C, dtype=np.float32)
    w = one if class_weight is None else class_weight
    p = one if pos_weight is None else pos_weight
    a, b = w * p, w.copy()
    if form.alpha is not None:
        a = a * np.float32(form.alpha)
        b = b * np.float32(1.0 - form.alpha)
    return a.astype(np.float32), b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name: str, dtype: str = "float32") -> Case:
    form_name, n, C, plan = CASES[name]
    form = FORMS[form_name]
    g = np.random.default_rng(sorted(CASES).index(name) + 1000)
    if form.m > 0:
        x = g.integers(-64, 65, size=(n, C)).astype(np.float32) / 8            # multiples of 1/8: exact in every dtype
    else:
        x = quantise(4.0 * g.standard_normal((n, C)).astype(np.float32), dtype)
    if form.soft:
        t = (g.integers(0, 17, size=(n, C)) / 16).astype(np.float32)
    else:
        t = (g.random((n, C)) < 0.2).astype(np.float32)
    valid = np.ones((n, C), dtype=bool)
    if plan == "some":
        valid = g.random((n, C)) >= 0.3
    elif plan == "class":
        valid[:, C // 2] = False
    elif plan == "all":
        valid[:] = False
    elif plan == "specials":
        # rows 0-11: the special values on valid elements, targets 1, 0, 1, 0 in classes 0-3.  Rows 12-23: ignored
        # elements whose logits hold NaN and +-inf.  Class NAN_CLASS: ordinary values and one valid NaN logit.
        for i, v in enumerate(SPECIAL_VALUES):
            x[i, :4] = v
            t[i, :4] = [1.0, 0.0, 1.0, 0.0]
        x[10:12, :2] = np.array([[30.0], [-30.0]], dtype=np.float32)        # classes 0 and 1 stay finite: +-inf in 2 and 3 only
        x[:12] = quantise(x[:12], dtype)
        valid[12:] = False
        x[12:, :] = np.array([np.nan, np.inf, -np.inf, np.nan], dtype=np.float32)[np.arange(12) % 4][:, None]
        x[3, NAN_CLASS] = np.nan
        valid[3, NAN_CLASS] = True
    unknown = np.where((np.arange(n * C).reshape(n, C) % 2) == 0, np.float32(np.nan), np.float32(-1.0))
    t = np.where(valid, t, unknown).astype(np.float32)
    pw = cw = None
    if form.weights:
        pw = (0.25 + 4.0 * g.random(C)).astype(np.float32)
        cw = (0.5 + g.random(C)).astype(np.float32)
    a, b = fold(form, pw, cw, C)
    if form.m > 0:                  # the discontinuity at s = m must not decide a comparison
        with np.errstate(over="ignore"):
            s = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
        assert not (valid & (np.abs(s - form.m) < 2.0 ** -10)).any()
    return Case(form, x, t, valid, pw, cw, a, b)


def zeroed_ignored(c: Case) -> Case:
    """the same case with zeros in the logits of its ignored elements"""
    return c._replace(x=np.where(c.valid, c.x, np.float32(0.0)).astype(np.float32))


# ---------------------------------------------------------------------------------------------- the restatement (torch, float64)

def restate_elements(x, t, valid, a, b, form: Form):
    """per-element loss [n, C] (0 where not valid) of float64 torch tensors, differentiable in x"""
    import torch
    import torch.nn.functional as F
    gp, gn, m, eps = form.gp, form.gn, form.m, form.eps
    zero = torch.zeros((), dtype=torch.float64)
    ts = torch.where(valid, t, zero)
    tp = ts * (1.0 - eps) + eps / 2
    cp, cn = a * tp, b * (1.0 - tp)
    mp = valid & (cp > 0)
    xp = torch.where(mp, x, zero)                                   # unselected elements see a harmless logit
    wp = 1.0 if gp == 0 else torch.exp(gp * F.logsigmoid(-xp))
    pos = torch.where(mp, cp * wp * -F.logsigmoid(xp), zero)
    mn = valid & (cn > 0)
    if m == 0:
        xn = torch.where(mn, x, zero)
        wn = 1.0 if gn == 0 else torch.exp(gn * F.logsigmoid(xn))
        neg = torch.where(mn, cn * wn * -F.logsigmoid(-xn), zero)
    else:
        alive = mn & ~(torch.sigmoid(x) - m <= 0)                   # a NaN logit stays alive
        xn = torch.where(alive, x, torch.full((), 8.0, dtype=torch.float64))
        q = torch.sigmoid(xn) - m
        wn = 1.0 if gn == 0 else torch.exp(gn * torch.log(q))
        neg = torch.where(alive, cn * wn * -torch.log(torch.sigmoid(-xn) + m), zero)
    return pos + neg


# ---------------------------------------------------------------------------------------------- closed form and bounds (numpy)

class Elements(NamedTuple):
    loss: np.ndarray                # [n, C] float64, 0 where not valid
    grad: np.ndarray                # dl/dx, 0 where not valid
    loss_err: np.ndarray            # absolute float32 error bounds of the kernel's element (before any sum or scale)
    grad_err: np.ndarray
    zero_grad: np.ndarray           # bool: the gradient must be an exact zero


def closed_form(x, t, valid, a, b, form: Form) -> Elements:
    """loss, gradient and their error bounds per element, float64 numpy"""
    gp, gn, m, eps = form.gp, form.gn, form.m, form.eps
    x = x.astype(np.float64)
    with np.errstate(all="ignore"):
        ts = np.where(valid, t.astype(np.float64), 0.0)
        tp = ts * (1.0 - eps) + eps / 2
        a64, b64 = a.astype(np.float64)[None, :], b.astype(np.float64)[None, :]
        cp, cn = a64 * tp, b64 * (1.0 - tp)
        d_tp = 3 * U if eps > 0 else 0.0
        d_cp = d_tp + U
        d_cn = np.where(cn > 0, tp * d_tp / np.where(tp < 1, 1.0 - tp, 1.0), 0.0) + 2 * U
        e = np.exp(-np.abs(x))
        l1p = np.log1p(e)
        r = 1.0 / (1.0 + e)
        up = x >= 0
        sg, s1 = np.where(up, r, e * r), np.where(up, e * r, r)
        nls, nl1 = np.maximum(-x, 0.0) + l1p, np.maximum(x, 0.0) + l1p
        # positive side
        wp = np.ones_like(x) if gp == 0 else np.exp(-gp * nl1)
        d_wp = 0.0 if gp == 0 else np.expm1(7 * U * gp * np.where(np.isfinite(nl1), nl1, 0.0)) + 2 * U
        on_p = valid & (cp > 0)
        P = np.where(on_p, cp * wp * nls, 0.0)
        sl = np.where(sg > 0, sg * nls, 0.0)
        gP = np.where(on_p, -cp * wp * (s1 + gp * sl), 0.0)
        P_err = np.where(np.isfinite(P), P * (d_cp + d_wp + 7 * U), 0.0)
        gP_err = np.abs(gP) * (d_cp + d_wp + 17 * U)
        # negative side
        on_n = valid & (cn > 0)
        if m == 0:
            wn = np.ones_like(x) if gn == 0 else np.exp(-gn * nls)
            d_wn = 0.0 if gn == 0 else np.expm1(7 * U * gn * np.where(np.isfinite(nls), nls, 0.0)) + 2 * U
            N = np.where(on_n, cn * wn * nl1, 0.0)
            sl1 = np.where(s1 > 0, s1 * nl1, 0.0)
            gN = np.where(on_n, cn * wn * (sg + gn * sl1), 0.0)
            N_err = np.where(np.isfinite(N), N * (d_cn + d_wn + 7 * U), 0.0)
            gN_err = np.abs(gN) * (d_cn + d_wn + 17 * U)
            alive = on_n
        else:
            q = sg - m
            alive = on_n & ~(q <= 0)
            qs = np.where(alive & (q > 0), q, 0.5)
            om = np.where(alive, s1 + m, 0.5)
            d_q = (6 * U * sg + U * m + U * qs) / qs
            d_om = (6 * U * s1 + U * m + U * om) / om
            nlq = -np.log(om)
            nlq_err = d_om + 2 * U * nlq
            lq = np.abs(np.log(qs))
            wn = np.ones_like(x) if gn == 0 else np.exp(gn * np.log(qs))
            d_wn = 0.0 if gn == 0 else np.expm1(gn * (d_q + 4 * U * lq)) + 2 * U
            N = np.where(alive, cn * wn * nlq, 0.0)
            N_err = np.where(alive, cn * wn * (nlq_err + nlq * (d_cn + d_wn + 2 * U)), 0.0)
            t1 = wn / om
            t2 = 0.0 if gn == 0 else gn * (wn / qs) * nlq
            inner = t1 + t2
            inner_err = t1 * (d_wn + d_om + U) + t2 * (d_wn + d_q + 4 * U + nlq_err / np.where(nlq > 0, nlq, 1.0)) + U * inner
            gN = np.where(alive, cn * sg * s1 * inner, 0.0)
            gN_err = np.where(alive, np.abs(gN) * (d_cn + 15 * U) + cn * sg * s1 * inner_err, 0.0)
        loss = P + N
        grad = gP + gN
        tiny = TINY * (cp + cn) * (1.0 + np.where(np.isfinite(x), np.abs(x), 0.0))
        loss_err = (P_err + N_err + U * np.where(np.isfinite(loss), np.abs(loss), 0.0) + tiny) * SECOND_ORDER
        grad_err = (gP_err + gN_err + U * np.abs(grad) + tiny) * SECOND_ORDER
        loss = np.where(valid, loss, 0.0)
        grad = np.where(valid, grad, 0.0)
        zero_grad = ~valid | (~on_p & ~alive)
    return Elements(loss, grad, np.where(valid, loss_err, 0.0), np.where(valid, grad_err, 0.0), zero_grad)


def row_blocks(n: int, C: int):
    """(nrb, rows_pb) of aecf_mlloss.hip's mll_row_blocks"""
    want = max((n * C + 16383) // 16384, 1)
    cap = max(min((1 << 20) // C, 1024), 1)
    want = min(want, cap)
    rows_pb = (n + want - 1) // want
    return (n + rows_pb - 1) // rows_pb, rows_pb


def workspace_layout(n: int, C: int) -> int:
    al = lambda v: (v + 255) // 256 * 256
    nrb, _ = row_blocks(n, C)
    return al(8 * nrb * C) + al(4 * nrb * C)


class Reference(NamedTuple):
    loss: float                     # the reduced loss
    per_class: np.ndarray           # mean over the valid elements of each class, 0 where none
    grad: np.ndarray                # d(reduced loss)/dx [n, C] for an upstream gradient of 1
    n_valid: float
    loss_bound: float
    per_class_bound: np.ndarray
    grad_bound: np.ndarray          # [n, C], before the rounding into a 16-bit dtype (``grad_bound_for``)
    zero_grad: np.ndarray
    stats: np.ndarray               # [2, C] loss sums | valid counts
    stats_bound: np.ndarray         # [C] for the loss sums


def reference(c: Case, reduction: str = "mean", n_chain: Optional[int] = None, world: int = 1) -> Reference:
    """the float64 reference of a case and the bounds of the library's outputs.  ``n_chain``: the longest float32 chain of a
    thread (default: rows_pb of the case's shape)."""
    el = closed_form(c.x, c.t, c.valid, c.a, c.b, c.form)
    n, C = c.x.shape
    valid = c.valid
    if n_chain is None:
        n_chain = row_blocks(n, C)[1]
    with np.errstate(all="ignore"):
        sums = el.loss.sum(0)
        counts = valid.sum(0).astype(np.float64)
        mags = np.where(np.isfinite(el.loss), np.abs(el.loss), 0.0).sum(0)
        sums_b = (el.loss_err.sum(0) + (n_chain * U + (n + C + 512 + world) * U64) * mags) * SECOND_ORDER
        N = counts.sum()
        div = N if reduction == "mean" else 1.0
        loss = sums.sum() / div if div > 0 else 0.0
        loss_b = (sums_b.sum() / max(div, 1.0) + (U + 4 * U64) * (abs(loss) if np.isfinite(loss) else 0.0)) * SECOND_ORDER
        per_class = np.where(counts > 0, sums / np.maximum(counts, 1.0), 0.0)
        per_class_b = (sums_b / np.maximum(counts, 1.0) + (U + 4 * U64) * np.where(np.isfinite(per_class), np.abs(per_class), 0.0)) * SECOND_ORDER
        scale = (1.0 / div if div > 0 else 0.0)
        grad = el.grad * scale
        grad_b = (el.grad_err * scale + 3 * U * np.abs(grad)) * SECOND_ORDER
    return Reference(float(loss), per_class, grad, float(N), float(loss_b), per_class_b, grad_b, el.zero_grad,
                     np.stack((sums, counts)), sums_b)


def grad_bound_for(ref: Reference, dtype: str, factor: float = 1.0) -> np.ndarray:
    """the gradient bound [n, C] with the one rounding into ``dtype`` (and an upstream factor)"""
    g = np.abs(ref.grad) * factor
    b = ref.grad_bound * factor + U16[dtype] * g
    if dtype == "float16":
        b = b + 2.0 ** -25
    return b


def check_close(got, want, bound, what: str) -> float:
    """got against want inside bound, elementwise: infinities and NaN must match as such; returns the largest error / bound"""
    got, want, bound = (np.asarray(v, dtype=np.float64) for v in (got, want, bound))
    got, want, bound = np.broadcast_arrays(got, want, bound)
    nan, inf = np.isnan(want), np.isinf(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN at other places than the reference"
    assert np.array_equal(got[inf], want[inf]), f"{what}: infinities differ"
    fin = ~nan & ~inf
    err = np.abs(got[fin] - want[fin])
    lim = bound[fin]
    ratio = float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0
    assert (err <= lim).all(), f"{what}: error / bound = {ratio:.3f} (largest error {err.max():.3e})"
    return ratio


# ---------------------------------------------------------------------------------------------- float32 emulation (and broken rules)

RULES = ("count_ignored", "ignore_by_product", "pos_weight_on_negatives", "margin_on_positives", "focal_not_differentiated",
         "smooth_ignored", "one_minus_sigma_by_subtraction", "local_mean")


def emulate(c: Case, reduction: str = "mean", rule: Optional[str] = None):
    """The kernels' arithmetic in float32 numpy, operation by operation, as dict(loss, per_class, grad).  A class's losses are
    added in ONE float32 chain over all n rows, longer than any thread's: compare against ``reference(c, n_chain=n)``.
    ``rule`` breaks one rule of the definition."""
    f = np.float32
    form = c.form
    gp, gn, m = f(form.gp), f(form.gn), f(form.m)
    ome, he = f(1.0) - f(form.eps), f(0.5) * f(form.eps)
    x, valid = c.x.astype(f), c.valid
    n, C = x.shape
    with np.errstate(all="ignore"):
        tp = c.t.astype(f) * ome + he
        if rule == "smooth_ignored":                    # validity tested after the smoothing
            valid = tp >= 0
        else:
            tp = np.where(valid, tp, f(0.0))
        a, b = c.a[None, :], c.b[None, :]
        if rule == "pos_weight_on_negatives":
            b = a
        cp, cn = a * tp, b * (f(1.0) - tp)
        e = np.exp(-np.abs(x))
        l1p = np.log1p(e)
        r = f(1.0) / (f(1.0) + e)
        er = e * r
        up = x >= 0
        sg, s1 = np.where(up, r, er), np.where(up, er, r)
        nls, nl1 = np.maximum(-x, f(0.0)) + l1p, np.maximum(x, f(0.0)) + l1p
        if rule == "one_minus_sigma_by_subtraction":
            s1 = f(1.0) - sg
            nl1 = -np.log(s1)
        wp = np.ones_like(x) if gp == 0 else np.exp(-gp * nl1)
        nls_p = nls
        if rule == "margin_on_positives":
            sp = np.maximum(sg - m, f(1e-30))
            nls_p = -np.log(sp)
            wp = np.ones_like(x) if gp == 0 else np.exp(gp * np.log1p(-sp))
        on_p = cp > 0
        P = np.where(on_p, (cp * wp) * nls_p, f(0.0))
        sl = np.where(sg > 0, sg * nls, f(0.0))
        fp = f(0.0) if rule == "focal_not_differentiated" else gp * sl
        gP = np.where(on_p, -(cp * wp) * (s1 + fp), f(0.0))
        on_n = cn > 0
        if m == 0:
            wn = np.ones_like(x) if gn == 0 else np.exp(-gn * nls)
            N = np.where(on_n, (cn * wn) * nl1, f(0.0))
            sl1 = np.where(s1 > 0, s1 * nl1, f(0.0))
            fn = f(0.0) if rule == "focal_not_differentiated" else gn * sl1
            gN = np.where(on_n, (cn * wn) * (sg + fn), f(0.0))
        else:
            q = sg - m
            alive = on_n & ~(q <= 0)
            om = s1 + m
            nlq = -np.log(om)
            nlq = np.where(nlq < 0, f(0.0), nlq)            # by select: a NaN stays a NaN
            wn = np.ones_like(x) if gn == 0 else np.exp(gn * np.log(q))
            N = np.where(alive, (cn * wn) * nlq, f(0.0))
            inner = wn / om
            if gn != 0 and rule != "focal_not_differentiated":
                inner = inner + gn * (wn / q) * nlq
            gN = np.where(alive, cn * (sg * s1) * inner, f(0.0))
        l, g = P + N, gP + gN
        assert l.dtype == np.float32 and g.dtype == np.float32
        if rule == "ignore_by_product":
            l, g = l * valid.astype(f), g * valid.astype(f)
        else:
            l, g = np.where(valid, l, f(0.0)), np.where(valid, g, f(0.0))
        sums = np.cumsum(l, axis=0, dtype=f)[-1].astype(np.float64)
        counts = valid.sum(0).astype(np.float64)
        total = sums.sum()
        cnt = float(n * C) if rule == "count_ignored" else counts.sum()
        if reduction == "mean":
            loss = f(total / cnt) if cnt > 0 else f(0.0)
            scale = f(np.float64(f(1.0)) / cnt) if cnt > 0 else f(0.0)
        else:
            loss, scale = f(total), f(1.0)
        per_class = np.where(counts > 0, sums / np.maximum(counts, 1.0), 0.0).astype(f)
        grad = g * scale if rule == "ignore_by_product" else np.where(valid, g * scale, f(0.0))
    return dict(loss=loss, per_class=per_class, grad=grad)
