"""Cases, float64 restatement, float32 emulation and bounds of the multi-label calibration (aecf_amd/metrics.py:
multilabel_calibration and fit_calibration, aecf_mlcal_* of the library).

Definitions (include/aecf_hip.h, "multi-label calibration").  x a logit as stored, y its target (unknown: NaN or < 0; positive
iff non-zero), VALID iff y is known and x is not NaN.  z = float32(float32(x * scale_c) + bias_c), or x where there is neither.
bin = #{j : z > e_j} over the float32 edges e_j = float32(log(j / (B - j))).  p = sigmoid(z); Brier term (1 - p)^2 or p^2, NLL
term -log p or -log(1 - p).  Per class: bin_count, bin_pos, bin_conf (sum of p), brier_sum, nll_sum, n_valid, n_pos, n_invalid.

``restate`` forms z in float32 numpy -- two roundings, the same bits as the library -- and everything after it in float64.
``emulate`` follows the kernels' float32 operations and can break one rule of the definition.

Bounds, from the operations of aecf_amd/csrc/aecf_calibration.hip, not fitted to a run.  U = 2**-24; a correctly rounded
operation has relative error U; expf and log1pf are documented at 1 ulp, at most 2 U.  z carries no error (same bits).

    e = exp(-|z|)    2 U              l1p = log1p(e)   2 U from e (e / ((1 + e) log1p(e)) <= 1) + 2 U = 4 U
    r = 1 / (1 + e)  1 + e: 2 U (e / (1 + e) <= 1 / 2, + U), the division U: 3 U;   e r: 2 + 3 + 1 = 6 U   so p and 1 - p: 6 U
    -log p, -log(1 - p) = max(-+z, 0) + l1p: 4 U + U = 5 U (both addends are >= 0)
    Brier term: a square of p or 1 - p: 2 * 6 U + U = 13 U
    below float32's normal range a value carries at most TINY = 2**-120 absolute, kept or flushed

Sums.  A thread adds the terms of the rows it owns in float32, one after the other: at most ``chain`` = rows_pb terms
(``row_blocks``), so beyond the element errors a float32 sum of non-negative terms is off by at most chain U sum.  Above the
thread everything is float64 in a fixed order, fewer than n + C + 1024 + world additions: (n + C + 1024 + world) 2**-53 sum.
All of it times 1.001 for the second-order terms.  Closing values: ece_c = sum_k |conf_k - pos_k| / n_c inherits
sum_k d(conf_k) / n_c; mce_c the largest d(conf_k) / count_k; brier and nll their sums' bounds over n; the pooled values the
sums of the classes' bounds; the macro values the mean of the classes' bounds; each + 8 * 2**-53 relative for the float64 closing.

The fit.  Sums over the USED elements (valid, finite x) at parameters theta = (scale, bias), s = sigmoid(z), d = s - y (formed
as p or -(1 - p): 6 U), w = s (1 - s) (13 U):  L = sum nll, g1 = sum d x, g0 = sum d, h11 = sum w x^2, h01 = sum w x, h00 = sum w.
    d x: 6 U + U = 7 U |d x| <= 7 U |x|;  the float32 chain adds chain U sum |d x| <= chain U sum |x|;  so with K = 7 + chain
    eps_g1 = 1.001 (K U + (n + C + 1024 + world) 2**-53) sum |x|        eps_g0 = 1.001 ((6 + chain) U + ...) n_used
tau: what the convergence threshold admits.  A converged problem's last accepted step delta came from (H~ + lambda D) delta =
-g~(theta_prev) and was at most s_j = 2**-20 max(1, |theta_j|) in every parameter, and theta = theta_prev + delta was then
rounded to float32 (U |theta_j| more).  So |g(theta)| = |g(theta_prev) + H delta + O(delta^2)| <= (lambda |D| + |H|) |delta| +
|H| U |theta| + curvature <= 3 |H| s with lambda <= 1 (lambda starts at 1e-3 and grows only on rejections; the CPU suite
asserts lambda <= 1 at convergence for every interior case) -- the errors of H~ act on delta only and are second order:
    tau_i = 3.001 sum_j |H_ij| s_j                                      (H the float64 Hessian at the returned parameters)
(a) |g_true(theta)| <= eps_g + tau.  (b) |theta - theta*| <= 1.01 |H^-1| (eps_g + tau) + U |theta| elementwise, |H^-1| the
absolute values of the inverse float64 Hessian at the optimum theta* (the NLL is convex; 1.01 for the Hessian's change over
that distance).
"""
import functools
import math
from typing import NamedTuple, Optional

import numpy as np

from tests.mlloss_cases import SPECIAL_VALUES, check_close, quantise, to_bf16  # noqa: F401  (shared helpers)

U = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -120
SECOND_ORDER = 1.001
MAX_BINS = 32
BOX = dict(scale=(1.0 / 64.0, 64.0), bias=(-16.0, 16.0))
MODES = ("temperature", "class_temperature", "platt")
STAT_NAMES = ("bin_count", "bin_pos", "bin_conf", "brier_sum", "nll_sum", "n_invalid", "n_valid", "n_pos")
CLOSING = ("ece", "mce", "brier", "nll", "ece_per_class", "mce_per_class", "brier_per_class", "nll_per_class", "macro_ece",
           "macro_brier", "macro_nll")


def edges(B: int) -> np.ndarray:
    """the B - 1 inner edges of equal-width probability bins in logit space: float32 of a float64 logarithm"""
    return np.array([math.log(j / (B - j)) for j in range(1, B)], dtype=np.float64).astype(np.float32)


def row_blocks(n: int, C: int):
    """(nrb, rows_pb) of aecf_calibration.hip's cal_row_blocks"""
    want = max((n * C + 16383) // 16384, 1)
    cap = max(min((1 << 19) // C, 1024), 1)
    want = min(want, cap)
    rows_pb = (n + want - 1) // want
    return (n + rows_pb - 1) // rows_pb, rows_pb


def workspace_layout(n: int, C: int, B: int) -> int:
    nrb, _ = row_blocks(n, C)
    return (8 * nrb * max(3 * B + 5, 9) * C + 255) // 256 * 256


# ---------------------------------------------------------------------------------------------- cases

class Case(NamedTuple):
    x: np.ndarray                   # float32 [n, C], values of the case's dtype
    t: np.ndarray                   # float32 [n, C]; unknown: NaN or -1 (alternating)
    B: int
    scale: Optional[np.ndarray]     # float32 [C] or None
    bias: Optional[np.ndarray]


# name -> (n, C, B, ignore plan, affine)
CASES = {
    "1x1_b1": (1, 1, 1, "none", None),
    "255x1_b15": (255, 1, 15, "some", None),
    "256x1_b2": (256, 1, 2, "none", "both"),
    "257x1_b32": (257, 1, 32, "some", "both"),
    "255x15_b15": (255, 15, 15, "some", "both"),
    "256x15_b32": (256, 15, 32, "class", "scale"),
    "257x15_b15": (257, 15, 15, "none", "bias"),
    "2049x17_b15": (2049, 17, 15, "some", "both"),
    "64x80_b15": (64, 80, 15, "some", "both"),
    "64x80_b32": (64, 80, 32, "class", None),
    "3x4096_b15": (3, 4096, 15, "some", "both"),
    "3x4096_b32": (3, 4096, 32, "none", None),
    "64x15_b15_all": (64, 15, 15, "all", "both"),
    "specials_b15": (48, 6, 15, "specials", None),
    "specials_b15_affine": (48, 6, 15, "specials", "both"),
    "overflow_b2": (16, 4, 2, "none", "overflow"),
}
CASE_IDS = list(CASES)
DTYPES = ("float32", "bfloat16", "float16")
NAN_CLASS = 4                       # the class of the specials cases that holds valid NaN logits beside ordinary values
EMPTY_CLASS = 5                     # ... and the one without a valid entry


def nextafter32(v, up: bool) -> np.float32:
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf))


@functools.lru_cache(maxsize=None)
def case(name: str, dtype: str = "float32") -> Case:
    n, C, B, plan, affine = CASES[name]
    g = np.random.default_rng(sorted(CASES).index(name) + 4000)
    x = quantise(3.0 * g.standard_normal((n, C)).astype(np.float32), dtype)
    t = (g.random((n, C)) < 0.3).astype(np.float32)
    valid = np.ones((n, C), dtype=bool)
    scale = bias = None
    if affine in ("both", "scale"):
        scale = (0.25 + 2.0 * g.random(C)).astype(np.float32)
        scale[0] = 0.5                                  # class 0: z = x / 2 exactly, so planted logits land on the edges
    if affine in ("both", "bias"):
        bias = g.standard_normal(C).astype(np.float32)
        bias[0] = 0.0
    if affine == "overflow":                            # z overflows to +-inf: by the product in class 0, by the sum in class 1
        top = 6e4 if dtype == "float16" else 3e38       # (float16 logits: scale and bias are float32 and can still overflow z)
        scale = np.array([3e38 / top * 64.0 if dtype == "float16" else 64.0, 1.0, 1.0, 0.5], dtype=np.float32)
        bias = np.array([0.0, 0.0 if dtype == "float16" else 3e38, 1.0, 0.0], dtype=np.float32)
        x[:4, 0] = quantise(np.array([top / 4, -top / 4, 1.0, -1.0], dtype=np.float32), dtype)
        x[:2, 1] = quantise(np.array([top, -top], dtype=np.float32), dtype)
    if plan == "some":
        valid = g.random((n, C)) >= 0.3
    elif plan == "class":
        valid[:, C // 2] = False
    elif plan == "all":
        valid[:] = False
    # logits exactly on every edge and one float32 step either side of it (class 0; through scale 1/2 where there is one)
    e = edges(B)
    mult = np.float32(2.0) if scale is not None else np.float32(1.0)
    planted = []
    for v in e:
        planted += [np.float32(v) * mult, nextafter32(v, True) * mult, nextafter32(v, False) * mult]
    planted = quantise(np.array(planted, dtype=np.float32), dtype) if planted else np.zeros(0, dtype=np.float32)
    k = min(len(planted), n) if plan != "specials" else 0
    if k:
        rows = g.permutation(n)[:k]
        x[rows, 0] = planted[:k]
        valid[rows, 0] = plan != "all"
    if plan == "specials":
        # rows 0-13: the special values and NaN on valid elements (targets 1, 0, 1, 0 in classes 0-3); rows 14-27: the same
        # logits under unknown targets; the other rows ordinary.  Class NAN_CLASS: ordinary values and two valid NaN logits;
        # class EMPTY_CLASS: no valid entry at all (unknown targets, and a column of NaN logits under known ones is class 3's).
        vals = np.array(SPECIAL_VALUES + (np.nan, np.nan), dtype=np.float32)
        for i, v in enumerate(vals):
            x[i, :4] = v
            t[i, :4] = [1.0, 0.0, 1.0, 0.0]
            x[14 + i, :4] = v
            valid[14 + i, :4] = False
        x[:28] = quantise(x[:28], dtype)
        x[3, NAN_CLASS] = x[9, NAN_CLASS] = np.nan
        t[3, NAN_CLASS], t[9, NAN_CLASS] = 1.0, 0.0
        valid[:, EMPTY_CLASS] = False
        x[::3, EMPTY_CLASS] = np.nan
    unknown = np.where((np.arange(n * C).reshape(n, C) % 2) == 0, np.float32(np.nan), np.float32(-1.0))
    t = np.where(valid, t, unknown).astype(np.float32)
    return Case(x, t, B, scale, bias)


def known(t: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return t >= 0


def garbage(c: Case, seed: int = 7) -> Case:
    """the same case with other garbage in the logits that must reach no output: those of unknown targets and the NaN logits"""
    g = np.random.default_rng(seed)
    junk = np.array([np.nan, np.inf, -np.inf, 1024.0, -7.5, 0.0], dtype=np.float32)[g.integers(0, 6, size=c.x.shape)]
    x = np.where(known(c.t), c.x, junk)
    return c._replace(x=x.astype(np.float32))


def z_float32(x: np.ndarray, scale, bias) -> np.ndarray:
    """the calibrated logit with the library's bits: a rounded product, then a rounded sum; x itself where there is neither"""
    x = x.astype(np.float32)
    if scale is None and bias is None:
        return x
    C = x.shape[1]
    s = np.ones(C, dtype=np.float32) if scale is None else scale.astype(np.float32)
    b = np.zeros(C, dtype=np.float32) if bias is None else bias.astype(np.float32)
    with np.errstate(all="ignore"):
        m = (x * s[None, :]).astype(np.float32)
        return (m + b[None, :]).astype(np.float32)


# ---------------------------------------------------------------------------------------------- closing arithmetic (float64)

def close(st: dict, rule: Optional[str] = None) -> dict:
    """the closing values from per-class statistics (arrays [C, B] and [C])"""
    cnt, pos, conf = (st[k].astype(np.float64) for k in ("bin_count", "bin_pos", "bin_conf"))
    nv = st["n_valid"].astype(np.float64)
    B = cnt.shape[1]

    def one(cnt, pos, conf, brier, nll, n):
        with np.errstate(all="ignore"):
            gap = np.abs(conf - pos)
            if n <= 0:
                return (np.nan,) * 4
            if rule == "ece_uniform_weight":            # the mean of the bins' gaps in place of the count-weighted mean
                ece = float(np.where(cnt > 0, gap / np.maximum(cnt, 1.0), 0.0).sum() / B)
            else:
                ece = float(gap.sum() / n)
            if rule == "mce_empty_bins":                # the quotient formed for every bin, 0 / 0 included
                mce = float(np.max(gap / cnt))
            else:
                mce = float(np.max(np.where(cnt > 0, gap / np.maximum(cnt, 1.0), 0.0)))
            return ece, mce, float(brier / n), float(nll / n)

    C = cnt.shape[0]
    per = np.array([one(cnt[c], pos[c], conf[c], st["brier_sum"][c], st["nll_sum"][c], nv[c]) for c in range(C)]).reshape(C, 4)
    with np.errstate(all="ignore"):
        pooled = one(cnt.sum(0), pos.sum(0), conf.sum(0), st["brier_sum"].sum(), st["nll_sum"].sum(), nv.sum())
    has = nv > 0
    macro = lambda v: float(v[has].mean()) if has.any() else np.nan
    return dict(ece=pooled[0], mce=pooled[1], brier=pooled[2], nll=pooled[3], ece_per_class=per[:, 0], mce_per_class=per[:, 1],
                brier_per_class=per[:, 2], nll_per_class=per[:, 3], macro_ece=macro(per[:, 0]), macro_brier=macro(per[:, 2]),
                macro_nll=macro(per[:, 3]))


# ---------------------------------------------------------------------------------------------- the restatement and its bounds

def _elements64(z: np.ndarray):
    """p, 1 - p, -log p, -log(1 - p) in float64 with the stable forms"""
    z = z.astype(np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(z))
        l1p = np.log1p(e)
        r = 1.0 / (1.0 + e)
        up = z >= 0
        return np.where(up, r, e * r), np.where(up, e * r, r), np.maximum(-z, 0.0) + l1p, np.maximum(z, 0.0) + l1p


def bin_of(z: np.ndarray, B: int) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return (z[..., None] > edges(B)).sum(-1)


class Reference(NamedTuple):
    stats: dict                     # the per-class statistics (STAT_NAMES), integer ones as int64
    closing: dict
    stats_bound: dict               # bin_conf [C, B], brier_sum [C], nll_sum [C]
    closing_bound: dict


def reference(c: Case, chain: Optional[int] = None, world: int = 1) -> Reference:
    """the float64 restatement of a case and the bounds of the library's outputs.  ``chain``: the longest float32 chain of a
    thread (default: rows_pb of the case's shape)."""
    n, C = c.x.shape
    B = c.B
    if chain is None:
        chain = row_blocks(n, C)[1]
    kn = known(c.t)
    nan = np.isnan(c.x)
    valid = kn & ~nan
    pos = valid & (c.t != 0)
    z = z_float32(c.x, c.scale, c.bias)
    p, q, nlp, nlq = _elements64(np.where(valid, z, np.float32(0.0)))
    b = bin_of(np.where(valid, z, np.float32(0.0)), B)
    with np.errstate(all="ignore"):
        brier = np.where(pos, q * q, p * p)
        nll = np.where(pos, nlp, nlq)
        zabs = np.where(np.isfinite(z), np.abs(z.astype(np.float64)), 0.0)
        e_conf, e_brier, e_nll = 6 * U * p + TINY, 13 * U * brier + TINY, 5 * U * np.where(np.isfinite(nll), nll, 0.0) + TINY * (1 + zabs)
    tree = (n + C + 1024 + world) * U64
    cnt = np.zeros((C, B), dtype=np.int64)
    bpos = np.zeros((C, B), dtype=np.int64)
    conf = np.zeros((C, B))
    conf_b = np.zeros((C, B))
    for k in range(B):
        m = valid & (b == k)
        cnt[:, k] = m.sum(0)
        bpos[:, k] = (m & pos).sum(0)
        conf[:, k] = np.where(m, p, 0.0).sum(0)
        conf_b[:, k] = (np.where(m, e_conf, 0.0).sum(0) + (chain * U + tree) * conf[:, k]) * SECOND_ORDER
    with np.errstate(all="ignore"):
        brier_sum = np.where(valid, brier, 0.0).sum(0)
        nll_sum = np.where(valid, nll, 0.0).sum(0)
        fin = lambda v: np.where(np.isfinite(v), v, 0.0)
        brier_b = (np.where(valid, e_brier, 0.0).sum(0) + (chain * U + tree) * brier_sum) * SECOND_ORDER
        nll_b = (np.where(valid, e_nll, 0.0).sum(0) + (chain * U + tree) * fin(np.where(valid, fin(nll), 0.0).sum(0))) * SECOND_ORDER
    stats = dict(bin_count=cnt, bin_pos=bpos, bin_conf=conf, brier_sum=brier_sum, nll_sum=nll_sum,
                 n_invalid=(kn & nan).sum(0).astype(np.int64), n_valid=valid.sum(0).astype(np.int64), n_pos=pos.sum(0).astype(np.int64))
    closing = close(stats)
    nv = stats["n_valid"].astype(np.float64)
    n1 = np.maximum(nv, 1.0)
    N1 = max(nv.sum(), 1.0)
    has = nv > 0
    rel = lambda v: 8 * U64 * np.abs(fin(np.asarray(v, dtype=np.float64)))
    ece_c = conf_b.sum(1) / n1
    mce_c = (conf_b / np.maximum(cnt, 1)).max(1)
    brier_c, nll_c = brier_b / n1, nll_b / n1
    mean = lambda v: float(v[has].mean()) if has.any() else 0.0
    pooled_conf_b = conf_b.sum(0)
    cb = dict(ece=pooled_conf_b.sum() / N1, mce=float((pooled_conf_b / np.maximum(cnt.sum(0), 1)).max()), brier=brier_b.sum() / N1,
              nll=nll_b.sum() / N1, ece_per_class=ece_c, mce_per_class=mce_c, brier_per_class=brier_c, nll_per_class=nll_c,
              macro_ece=mean(ece_c), macro_brier=mean(brier_c), macro_nll=mean(nll_c))
    cb = {k: (np.asarray(v) + rel(closing[k])) * SECOND_ORDER for k, v in cb.items()}
    return Reference(stats, closing, dict(bin_conf=conf_b, brier_sum=brier_b, nll_sum=nll_b), cb)


def check_stats(got: dict, ref: Reference, what: str) -> float:
    """integer statistics EQUAL, float statistics and closing values inside their bounds; the largest error / bound"""
    for k in ("bin_count", "bin_pos", "n_valid", "n_pos", "n_invalid"):
        assert np.array_equal(np.asarray(got[k]), ref.stats[k]), f"{what}: {k} differs"
    worst = 0.0
    for k in ("bin_conf", "brier_sum", "nll_sum"):
        if k in got:
            worst = max(worst, check_close(got[k], ref.stats[k], ref.stats_bound[k], f"{what} {k}"))
    for k in CLOSING:
        if k in got:
            worst = max(worst, check_close(got[k], ref.closing[k], ref.closing_bound[k], f"{what} {k}"))
    return worst


# ---------------------------------------------------------------------------------------------- float32 emulation (and broken rules)

STAT_RULES = ("edge_upper", "last_bin_loses_inf", "nan_valid", "unknown_negative", "ece_uniform_weight", "div_scale", "bias_first",
              "mce_empty_bins")


def _elements32(z: np.ndarray):
    f = np.float32
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(z))
        l1p = np.log1p(e)
        r = f(1.0) / (f(1.0) + e)
        er = e * r
        up = z >= 0
        out = np.where(up, r, er), np.where(up, er, r), np.maximum(-z, f(0.0)) + l1p, np.maximum(z, f(0.0)) + l1p
    assert all(v.dtype == np.float32 for v in out)
    return out


def _chain32(v: np.ndarray) -> np.ndarray:
    """the rows of a class added in ONE float32 chain (longer than any thread's), as float64"""
    if v.shape[0] == 0:
        return np.zeros(v.shape[1])
    return np.cumsum(v.astype(np.float32), axis=0, dtype=np.float32)[-1].astype(np.float64)


def emulate(c: Case, rule: Optional[str] = None) -> dict:
    """The kernels' arithmetic in float32 numpy as dict(statistics and closing values).  A class's terms are added in one
    float32 chain over all n rows: compare against ``reference(c, chain=n)``.  ``rule`` breaks one rule of the definition."""
    f = np.float32
    n, C = c.x.shape
    B = c.B
    kn = known(c.t)
    if rule == "unknown_negative":
        kn = np.ones_like(kn)
    nan = np.isnan(c.x)
    valid = kn if rule == "nan_valid" else kn & ~nan
    with np.errstate(invalid="ignore"):
        pos = valid & (c.t > 0)
    x = c.x.astype(f)
    with np.errstate(all="ignore"):
        if rule in ("div_scale", "bias_first") and (c.scale is not None or c.bias is not None):
            s = np.ones(C, dtype=f) if c.scale is None else c.scale
            b = np.zeros(C, dtype=f) if c.bias is None else c.bias
            z = (x / s[None, :] + b[None, :]).astype(f) if rule == "div_scale" else ((x + b[None, :]) * s[None, :]).astype(f)
        else:
            z = z_float32(x, c.scale, c.bias)
        e = edges(B)
        bins = (z[..., None] >= e).sum(-1) if rule == "edge_upper" else (z[..., None] > e).sum(-1)
        p, q, nlp, nlq = _elements32(z)
        brier = np.where(pos, q * q, p * p)
        nll = np.where(pos, nlp, nlq)
    keep = valid & ~np.isposinf(z) if rule == "last_bin_loses_inf" else valid
    cnt = np.zeros((C, B), dtype=np.int64)
    bpos = np.zeros((C, B), dtype=np.int64)
    conf = np.zeros((C, B))
    for k in range(B):
        m = keep & (bins == k)
        cnt[:, k] = m.sum(0)
        bpos[:, k] = (m & pos).sum(0)
        conf[:, k] = _chain32(np.where(m, p, f(0.0)))
    st = dict(bin_count=cnt, bin_pos=bpos, bin_conf=conf, brier_sum=_chain32(np.where(valid, brier, f(0.0))),
              nll_sum=_chain32(np.where(valid, nll, f(0.0))), n_invalid=(kn & nan & ~valid).sum(0).astype(np.int64),
              n_valid=valid.sum(0).astype(np.int64), n_pos=pos.sum(0).astype(np.int64))
    st.update(close(st, rule))
    return st


def stats_ratio(got: dict, ref: Reference) -> float:
    """the largest error / bound without asserting; inf where an integer statistic, a NaN or an infinity differs"""
    for k in ("bin_count", "bin_pos", "n_valid", "n_pos", "n_invalid"):
        if not np.array_equal(np.asarray(got[k]), ref.stats[k]):
            return math.inf
    worst = 0.0
    pairs = [(k, ref.stats[k], ref.stats_bound[k]) for k in ("bin_conf", "brier_sum", "nll_sum")]
    pairs += [(k, ref.closing[k], ref.closing_bound[k]) for k in CLOSING]
    for k, want, bound in pairs:
        g, w, b = np.broadcast_arrays(np.asarray(got[k], dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound))
        nan, inf = np.isnan(w), np.isinf(w)
        if not np.array_equal(np.isnan(g), nan) or not np.array_equal(g[inf], w[inf]):
            return math.inf
        fin = ~nan & ~inf
        if fin.any():
            worst = max(worst, float((np.abs(g[fin] - w[fin]) / np.maximum(b[fin], 1e-300)).max()))
    return worst


# ---------------------------------------------------------------------------------------------- the fit

FIT_RULES = ("h01_dropped", "mean_of_class_fits", "rejected_trial_returned")


class FitCase(NamedTuple):
    x: np.ndarray                   # float32 [n, C]
    t: np.ndarray                   # float32 [n, C], unknown: NaN or -1
    degenerate: dict                # class -> "no_positive" | "no_negative" | "separable" | "non_finite"


# name -> (n, C, mean and spread of the logits, how sharply the labels follow them, ignore plan, degenerate classes)
FIT_CASES = {
    "fit_257x5": (257, 5, 0.0, 2.0, 0.6, "some", False),
    "fit_2049x17": (2049, 17, 0.5, 2.0, 1.7, "some", False),
    "fit_300x8_degenerate": (300, 8, 0.0, 2.0, 0.8, "none", True),
    "fit_512x3_shifted": (512, 3, 2.5, 2.0, 0.5, "none", False),      # scale and bias strongly coupled: the cross term matters
    "fit_400x2_overconfident": (400, 2, 0.0, 8.0, 1.0, "flipped", False),  # large logits, few of them wrong: no curvature at scale 1,
                                                                            # the first Newton trial overshoots and is rejected
}
FIT_CASE_IDS = list(FIT_CASES)


@functools.lru_cache(maxsize=None)
def fit_case(name: str, dtype: str = "float32") -> FitCase:
    n, C, mean, spread, sharp, plan, degen = FIT_CASES[name]
    g = np.random.default_rng(sorted(FIT_CASES).index(name) + 9000)
    x = quantise((mean + spread * g.standard_normal((n, C))).astype(np.float32), dtype)
    slopes = sharp * (0.6 + 0.8 * g.random(C))
    shifts = 0.5 * g.standard_normal(C)
    prob = 1.0 / (1.0 + np.exp(-(x.astype(np.float64) * slopes[None, :] + shifts[None, :])))
    t = (g.random((n, C)) < prob).astype(np.float32)
    if plan == "flipped":                               # the sign of the logit, 4 % flipped: confident and mostly right
        t = ((x > 0) ^ (g.random((n, C)) < 0.04)).astype(np.float32)
    valid = np.ones((n, C), dtype=bool)
    if plan == "some":
        valid = g.random((n, C)) >= 0.25
    x[g.integers(0, n, 3), g.integers(0, C, 3)] = np.inf           # a few non-finite logits: left out of the fit
    x[g.integers(0, n, 2), g.integers(0, C, 2)] = np.nan
    degenerate = {}
    if degen:
        t[:, 1] = 0.0
        t[:, 2] = 1.0
        t[:, 4] = (x[:, 4] > 0.3).astype(np.float32)
        x[:, 6] = np.where(np.arange(n) % 2 == 0, np.float32(np.inf), np.float32(-np.inf))
        degenerate = {1: "no_positive", 2: "no_negative", 4: "separable", 6: "non_finite"}
    unknown = np.where((np.arange(n * C).reshape(n, C) % 2) == 0, np.float32(np.nan), np.float32(-1.0))
    t = np.where(valid, t, unknown).astype(np.float32)
    return FitCase(x, t, degenerate)


def used(c) -> np.ndarray:
    return known(c.t) & np.isfinite(c.x)


def fit_sums(x: np.ndarray, pos: np.ndarray, use: np.ndarray, scale: float, bias: float, arith: str = "float64") -> np.ndarray:
    """(L, g1, g0, h11, h01, h00, n_used, n_used positives) of ONE class (1-d arrays) at float32 parameters.  ``arith``:
    "float64" -- z in float32 (the library's bits), everything after it in float64; "float32" -- the kernel's float32
    operations, the terms added in one float32 chain."""
    f = np.float32
    xs, ps = x[use].astype(f), pos[use]
    with np.errstate(all="ignore"):
        z = ((xs * f(scale)).astype(f) + f(bias)).astype(f)
        if arith == "float32":
            p, q, nlp, nlq = _elements32(z)
            d = np.where(ps, -q, p)
            w = p * q
            wx = w * xs
            terms = (np.where(ps, nlp, nlq), d * xs, d, wx * xs, wx, w)
            assert all(v.dtype == np.float32 for v in terms)
            sums = [float(np.cumsum(v, dtype=f)[-1]) if v.size else 0.0 for v in terms]
        else:
            p, q, nlp, nlq = _elements64(z)
            x64 = xs.astype(np.float64)
            d = np.where(ps, -q, p)
            w = p * q
            sums = [float(v.sum()) for v in (np.where(ps, nlp, nlq), d * x64, d, w * x64 * x64, w * x64, w)]
    return np.array(sums + [float(use.sum()), float(ps.sum())])


def _step(mode: str, S: np.ndarray, st: dict, trial, rule: Optional[str] = None, round32: bool = True):
    """aecf_calibration.hip's cal_step: one damped Newton step of one problem; returns the parameters to evaluate next"""
    ts, tb = trial
    take = False
    if st["phase"] == 0:
        st.update(lam=1e-3, L0=S[0], L=S[0], steps=0)
        if not (S[6] > 0 and S[7] > 0 and S[7] < S[6]):
            st.update(phase=3, scale=1.0, bias=0.0)
        else:
            st["phase"] = 1
            take = True
    elif st["phase"] == 1:
        if S[0] <= st["L"] + 2.0 ** -14 * abs(st["L"]):
            tol = 2.0 ** -20
            small = abs(ts - st["scale"]) <= tol * max(1.0, abs(ts)) and abs(tb - st["bias"]) <= tol * max(1.0, abs(tb))
            st["lam"] = max(st["lam"] * 0.1, 1e-9)
            st["steps"] += 1
            take = True
            if small:
                st["phase"] = 2
        else:
            st["lam"] = min(st["lam"] * 10.0, 1e12)
    if take:
        st.update(scale=ts, bias=tb, L=min(S[0], st["L"]), g1=S[1], g0=S[2], h11=S[3], h01=S[4], h00=S[5])
    if st["phase"] != 1:
        return st["scale"], st["bias"]
    lam = 1.0 + st["lam"]
    ds = db = 0.0
    if mode == "platt":
        a, d, b = st["h11"] * lam, st["h00"] * lam, (0.0 if rule == "h01_dropped" else st["h01"])
        det = a * d - b * b
        if det > 0:
            ds = -(d * st["g1"] - b * st["g0"]) / det
            db = -(a * st["g0"] - b * st["g1"]) / det
    else:
        a = st["h11"] * lam
        if a > 0:
            ds = -st["g1"] / a
    ns = min(max(st["scale"] + ds, BOX["scale"][0]), BOX["scale"][1])
    nb = min(max(st["bias"] + db, BOX["bias"][0]), BOX["bias"][1])
    if round32:
        ns, nb = float(np.float32(ns)), float(np.float32(nb))
    return ns, nb


def fit(c: FitCase, mode: str, max_iter: int = 32, arith: str = "float64", rule: Optional[str] = None, round32: bool = True) -> dict:
    """The fit's rule restated (``arith="float64"``) or emulated in the kernels' float32 (``arith="float32"``): per problem
    scale, bias, fitted, converged, nll_before, nll_after, lam.  ``round32=False`` keeps the parameters in float64 (for the
    comparison with a float64 minimiser; z is then formed in float64 too)."""
    n, C = c.x.shape
    use = used(c)
    with np.errstate(invalid="ignore"):
        pos = c.t > 0

    def class_sums(cls, s, b):
        if round32:
            return fit_sums(c.x[:, cls], pos[:, cls], use[:, cls], s, b, arith)
        xs, ps = c.x[use[:, cls], cls].astype(np.float64), pos[use[:, cls], cls]
        p, q, nlp, nlq = _elements64(xs * s + b)
        d, w = np.where(ps, -q, p), p * q
        return np.array([np.where(ps, nlp, nlq).sum(), (d * xs).sum(), d.sum(), (w * xs * xs).sum(), (w * xs).sum(), w.sum(),
                         float(xs.size), float(ps.sum())])

    def run(problem_sums, md):
        st, trial = dict(phase=0), (1.0, 0.0)
        for _ in range(max_iter):
            last = trial
            trial = _step(md, problem_sums(*trial), st, trial, rule, round32)
        out = (trial if rule == "rejected_trial_returned" else (st["scale"], st["bias"]))
        return dict(scale=out[0], bias=out[1], fitted=st["phase"] != 3, converged=st["phase"] == 2, nll_before=st["L0"],
                    nll_after=st["L"], lam=st["lam"], last=last)

    if mode == "temperature" and rule != "mean_of_class_fits":
        r = run(lambda s, b: sum(class_sums(k, s, b) for k in range(C)), "temperature")
        return {k: np.array([v]) for k, v in r.items() if k != "last"}
    per = [run(functools.partial(class_sums, k), "class_temperature" if mode == "temperature" else mode) for k in range(C)]
    out = {k: np.array([r[k] for r in per]) for k in per[0] if k != "last"}
    if mode == "temperature":                           # the broken rule: the mean of the per-class fits
        keep = out["fitted"]
        out = {k: np.array([v[keep].mean() if k in ("scale", "bias") else v[keep].sum()]) for k, v in out.items()}
        out["fitted"] = out["converged"] = np.array([True])
    return out


def true_nll(c: FitCase, classes, scale: float, bias: float):
    """float64 NLL, its gradient (2) and Hessian (2 x 2) over the used elements of ``classes`` at (scale, bias), and sum |x|"""
    use = used(c)
    L, g, H, sx, nu = 0.0, np.zeros(2), np.zeros((2, 2)), 0.0, 0
    for k in classes:
        m = use[:, k]
        x = c.x[m, k].astype(np.float64)
        with np.errstate(invalid="ignore"):
            ps = c.t[m, k] > 0
        p, q, nlp, nlq = _elements64(x * scale + bias)
        d, w = np.where(ps, -q, p), p * q
        L += np.where(ps, nlp, nlq).sum()
        g += np.array([(d * x).sum(), d.sum()])
        H += np.array([[(w * x * x).sum(), (w * x).sum()], [(w * x).sum(), w.sum()]])
        sx += np.abs(x).sum()
        nu += x.size
    return L, g, H, sx, nu


def optimum(c: FitCase, classes, mode: str, iters: int = 200):
    """the float64 minimiser of the NLL by plain Newton steps with step halving (to about 1e-14), unclamped"""
    th = np.array([1.0, 0.0])
    free = [0, 1] if mode == "platt" else [0]
    for _ in range(iters):
        L, g, H, _, _ = true_nll(c, classes, *th)
        step = np.zeros(2)
        step[free] = -np.linalg.solve(H[np.ix_(free, free)], g[free])
        f = 1.0
        while f > 1e-12 and not true_nll(c, classes, *(th + f * step))[0] <= L:
            f *= 0.5
        if np.abs(f * step).max() < 1e-15:
            break
        th = th + f * step
    return th


def fit_bounds(c: FitCase, classes, mode: str, theta, world: int = 1):
    """(gradient bound [2], parameter bound [2], float64 gradient at theta, the optimum) of one problem: (a) and (b) above"""
    n, C = c.x.shape
    chain = row_blocks(n, C)[1]
    L, g, H, sx, nu = true_nll(c, classes, float(theta[0]), float(theta[1]))
    tree = (n + C + 1024 + world) * U64
    eps = SECOND_ORDER * np.array([((7 + chain) * U + tree) * sx, ((6 + chain) * U + tree) * nu])
    s = 2.0 ** -20 * np.maximum(1.0, np.abs(np.asarray(theta, dtype=np.float64)))
    free = [0, 1] if mode == "platt" else [0]
    Hf = H[np.ix_(free, free)]
    tau = 3.001 * np.abs(Hf) @ s[free]
    gb = np.zeros(2)
    gb[free] = eps[free] + tau
    opt = optimum(c, classes, mode)
    Ho = true_nll(c, classes, *opt)[2][np.ix_(free, free)]
    pb = np.zeros(2)
    pb[free] = 1.01 * np.abs(np.linalg.inv(Ho)) @ gb[free] + U * np.abs(np.asarray(theta, dtype=np.float64))[free]
    return gb, pb, g, opt


def problems(c: FitCase, mode: str):
    """the class lists of the independent problems of a mode"""
    C = c.x.shape[1]
    return [list(range(C))] if mode == "temperature" else [[k] for k in range(C)]


def check_fit(c: FitCase, mode: str, got: dict, what: str, world: int = 1, strict: bool = True) -> float:
    """(a) - (e) for every problem of a mode; ``got``: arrays per problem (scale, bias, fitted, converged, nll_before,
    nll_after).  Returns the largest error / bound of (a) and (b)."""
    worst = 0.0
    for i, classes in enumerate(problems(c, mode)):
        kind = c.degenerate.get(classes[0]) if len(classes) == 1 else None
        th = np.array([float(got["scale"][i]), float(got["bias"][i])])
        assert BOX["scale"][0] <= th[0] <= BOX["scale"][1] and BOX["bias"][0] <= th[1] <= BOX["bias"][1], f"{what} {i}: outside the box"
        assert got["nll_after"][i] <= got["nll_before"][i], f"{what} problem {i}: the NLL went up"          # (c)
        if kind in ("no_positive", "no_negative", "non_finite"):                                            # (d)
            assert not got["fitted"][i] and th[0] == 1.0 and th[1] == 0.0, f"{what} problem {i}: a degenerate class was fitted"
            continue
        assert got["fitted"][i], f"{what} problem {i}: not fitted"
        if kind == "separable":
            continue
        assert got["converged"][i], f"{what} problem {i}: not converged"                                    # (e)
        gb, pb, g, opt = fit_bounds(c, classes, mode, th, world)
        free = [0, 1] if mode == "platt" else [0]
        if mode != "platt":
            assert th[1] == 0.0, f"{what} problem {i}: a temperature with a bias"
        for j in free:
            ra, rb = abs(g[j]) / gb[j], abs(th[j] - opt[j]) / pb[j]
            assert ra <= 1.0 or not strict, f"{what} problem {i}: gradient / bound = {ra:.3f} in parameter {j}"         # (a)
            assert rb <= 1.0 or not strict, f"{what} problem {i}: parameter error / bound = {rb:.3f} in parameter {j}"  # (b)
            worst = max(worst, ra, rb)
    return worst


def fit_ratio(c: FitCase, mode: str, got: dict) -> float:
    """the largest error / bound of (a) and (b) without asserting them; inf where (c), (d), (e) or the box fails"""
    try:
        return check_fit(c, mode, got, "fit", strict=False)
    except AssertionError:
        return math.inf
