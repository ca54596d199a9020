"""Cases, integer / float64 restatement and bounds of the multi-label bootstrap (aecf_amd/metrics.py: bootstrap_metrics and
bootstrap_compare; aecf_mlboot_order / _draw / _walk of the library).

The restatement, in numpy, of the three passes as include/aecf_hip.h documents them:

 order   the valid (non-NaN) rows of a class in numpy's STABLE descending argsort of the evaluation's integer order image (-0 ties
         +0), each entry row | head << 31 | pos << 30 | pred << 29.
 draw    replicate 0 all ones; replicate r >= 1: n draws from philox4x32_10 (Salmon et al. 2011, the published constants, written
         out below), key (seed lo, seed hi), counter (t >> 1 lo, t >> 1 hi, r, 0x626f6f74), value c[2 (t & 1) + 1] << 32 |
         c[2 (t & 1)], row = (value * n) >> 64.
 walk    per tie group: gall, gpos the weight sums, cum_* the sums of the groups before; S = sum gpos (cum_pos + gpos) / (cum_all +
         gall) over the groups with gpos > 0, U2 = sum (gall - gpos) (2 cum_pos + gpos), TP / FP / FN weighted.  Integers in
         int64 (exact at these sizes: 2 Wpos Wneg < 2**40), S with one float64 quotient and product per group and ``math.fsum``.

The bounds (U = 2**-53).  Every integer statistic is compared for EQUALITY.
 S / AP.  The library's lane adds, for each of the G groups of the class that hold positive weight, a product of gpos and one
   float64 quotient: 2 roundings per term, G - 1 for the sequential sum of non-negative terms, so (G + 1) U relative; the
   restatement's terms carry the same 2 and its fsum 1: 3 U.  ``s_bound(G) = (G + 4) U``, relative to S, and S <= Wpos.  AP = S /
   Wpos adds one division on either side: ``ap_bound(G) = (G + 6) U`` absolute (AP <= 1).  G is taken as the number of tie groups
   of the class that hold a positive ROW: no replicate has more groups with positive weight.
 AUROC, F1.  Exact integers (below 2**53) and one division on either side, the same quotient: they agree bit for bit; 2 U
   relative allows a division that is not correctly rounded, as tests/metrics_cases.py does.
 Macro values.  A mean over at most C values: ``macro_bound(b, C) = b + (C + 2) U`` (metrics_cases).
 Percentile limits.  Both sides interpolate linearly between the order statistics at the virtual index q (m - 1) of m defined
   replicates.  The index is at most m and is formed with up to three roundings (numpy forms m q - q, torch q (m - 1)), each at
   most m U; an index error e moves the interpolated value by at most e times the distance of two neighbouring order statistics,
   itself at most 1; the interpolation adds 3 roundings of values <= 1.  ``ci_bound(b, m) = b + (3 m + 3) U`` with b the bound of
   the replicates' values.
"""
import math

import numpy as np

from tests import metrics_cases as M

U = M.U
TAG = 0x626f6f74
HEAD, POS, PRED = 1 << 31, 1 << 30, 1 << 29
STAT_NAMES = ("wpos", "wvalid", "u2", "tp", "fp", "fn")
SCORES = ("ap", "auroc", "f1", "map", "macro_auroc", "macro_f1")
AUROC_BOUND = 2 * U
F1_BOUND = 2 * U


def s_bound(groups: int) -> float:
    return (groups + 4) * U


def ap_bound(groups: int) -> float:
    b = (groups + 6) * U
    assert b < M.CAP
    return b


def macro_bound(b: float, classes: int) -> float:
    return b + (classes + 2) * U


def ci_bound(b: float, m: int) -> float:
    return b + (3 * m + 3) * U


# ---------------------------------------------------------------------------------------------- philox and the draw

def philox4x32_10(c, k0, k1):
    """c: four uint64 arrays holding 32-bit words; returns the four output words (Salmon et al., SC'11: multipliers 0xD2511F53
    and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten rounds)"""
    m32 = np.uint64(0xffffffff)
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & m32 for x in c)
    k0, k1 = np.uint64(k0 & 0xffffffff), np.uint64(k1 & 0xffffffff)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & m32, p0 & m32, n0, n2
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def _row_of(lo, hi, n):
    """(hi << 32 | lo) * n >> 64 for 32-bit words lo, hi and n <= 2**24, in uint64 without overflow"""
    n = np.uint64(n)
    return ((hi * n + ((lo * n) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def draw_weights(n: int, replicates: int, seed: int, replicate0: int = 0, rule=None) -> np.ndarray:
    """int64 [replicates, n]: the multiplicities of replicates replicate0 .. .  ``rule="drawn_zero"`` draws replicate 0 too."""
    out = np.zeros((replicates, n), dtype=np.int64)
    pairs = np.arange((n + 1) // 2, dtype=np.uint64)
    for q in range(replicates):
        r = replicate0 + q
        if r == 0 and rule != "drawn_zero":
            out[q] = 1
            continue
        c = philox4x32_10((pairs, pairs >> np.uint64(32), np.full_like(pairs, r), np.full_like(pairs, TAG)), seed, seed >> 32)
        rows = np.concatenate([_row_of(c[0], c[1], n), _row_of(c[2], c[3], n)[:n // 2]])       # draws 2 t | draws 2 t + 1 < n
        out[q] = np.bincount(rows, minlength=n)
    return out


# ---------------------------------------------------------------------------------------------- order

def order_image(s: np.ndarray) -> np.ndarray:
    """the evaluation's integer image of float32 order as int64; NaN -> INT_MIN, -0 -> the image of +0"""
    b = np.ascontiguousarray(s, dtype=np.float32).view(np.int32).astype(np.int64)
    nan = (b & 0x7fffffff) > 0x7f800000
    b = np.where(b == -(1 << 31), 0, b)
    b = np.where(b < 0, b ^ 0x7fffffff, b)
    return np.where(nan, -(1 << 31), b)


def restate_order(logits, labels, thresholds, rule=None):
    """list over the classes of uint32 arrays [nvalid]: the entries in slot order.  ``rule="position_ties"``: every entry a head"""
    s = np.asarray(logits, dtype=np.float32)
    y = np.asarray(labels) != 0
    n, C = s.shape
    thr = order_image(np.asarray(thresholds, dtype=np.float32))
    out = []
    for c in range(C):
        img = order_image(s[:, c])
        rows = np.flatnonzero(img != -(1 << 31))
        rows = rows[np.argsort(-img[rows], kind="stable")]
        k = img[rows]
        head = np.ones(len(rows), dtype=bool)
        if rule != "position_ties":
            head[1:] = k[1:] != k[:-1]
        e = rows.astype(np.uint32) | (head * HEAD).astype(np.uint32) | (y[rows, c] * POS).astype(np.uint32) \
            | ((k > thr[c]) * PRED).astype(np.uint32)
        out.append(e)
    return out


def positive_groups(order) -> np.ndarray:
    """per class, the tie groups that hold a positive row (the G of the bounds)"""
    out = []
    for e in order:
        gid = np.cumsum((e & HEAD) != 0)
        out.append(len(np.unique(gid[(e & POS) != 0])))
    return np.array(out, dtype=np.int64)


# ---------------------------------------------------------------------------------------------- walk and closing

def restate_walk(order, weights, rule=None):
    """dict of int64 [R, C] wpos | wvalid | u2 | tp | fp | fn and float64 [R, C] s, from the entries of ``restate_order`` and
    weights int [R, n].  Rules broken on purpose: "pos_weights_only" (a negative row weighs 1), "unweighted_pred" (TP / FP / FN
    count rows), "independent_classes" (class c takes the weights of replicate (r + c) mod R: its own resample)."""
    W = np.asarray(weights, dtype=np.int64)
    R, C = W.shape[0], len(order)
    out = {k: np.zeros((R, C), dtype=np.int64) for k in STAT_NAMES}
    out["s"] = np.zeros((R, C))
    for c, e in enumerate(order):
        if len(e) == 0:
            continue
        rows = (e & 0xffffff).astype(np.int64)
        pos, pred = (e & POS) != 0, (e & PRED) != 0
        Wc = np.roll(W, -c, axis=0) if rule == "independent_classes" else W
        w = Wc[:, rows]
        if rule == "pos_weights_only":
            w = np.where(pos, w, 1)
        starts = np.flatnonzero((e & HEAD) != 0)
        gall = np.add.reduceat(w, starts, axis=1)
        gpos = np.add.reduceat(w * pos, starts, axis=1)
        cum_pos = np.cumsum(gpos, axis=1) - gpos
        ge_pos, ge_all = cum_pos + gpos, np.cumsum(gall, axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            terms = np.where(gpos > 0, gpos * (ge_pos / np.where(gpos > 0, ge_all, 1)), 0.0)
        out["s"][:, c] = [math.fsum(t) for t in terms]
        out["u2"][:, c] = ((gall - gpos) * (2 * cum_pos + gpos)).sum(1)
        out["wpos"][:, c], out["wvalid"][:, c] = gpos.sum(1), gall.sum(1)
        wp = np.ones_like(w) if rule == "unweighted_pred" else w
        out["tp"][:, c] = (wp * (pos & pred)).sum(1)
        out["fp"][:, c] = (wp * (~pos & pred)).sum(1)
        out["fn"][:, c] = (wp * (pos & ~pred)).sum(1)
    return out


def close(st):
    """ap / auroc / f1 [R, C] and map / macro_auroc / macro_f1 [R] from the statistics: ``_close``'s rules per replicate"""
    wpos, wneg = st["wpos"].astype(np.float64), (st["wvalid"] - st["wpos"]).astype(np.float64)
    tp, fp, fn = (st[k].astype(np.float64) for k in ("tp", "fp", "fn"))
    has, both = wpos > 0, (wpos > 0) & (wneg > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ap = np.where(has, st["s"] / np.where(has, wpos, 1), 0.0)
        auroc = np.where(both, st["u2"].astype(np.float64) / np.where(both, 2 * wpos * wneg, 1), np.nan)
        scored = has & (tp > 0)
        f1 = np.where(scored, 2 * tp / np.where(scored, 2 * tp + fp + fn, 1), 0.0)
    out = dict(ap=ap, auroc=auroc, f1=f1, map=np.zeros(len(ap)), macro_auroc=np.full(len(ap), np.nan), macro_f1=np.zeros(len(ap)))
    for r in range(len(ap)):
        for name, values, keep in (("map", ap[r], has[r]), ("macro_auroc", auroc[r], both[r]), ("macro_f1", f1[r], f1[r] > 0)):
            if keep.any():
                out[name][r] = math.fsum(values[keep]) / keep.sum()
    return out


def restate(logits, labels, weights, thresholds=None, rule=None):
    """everything at once: dict(order, groups, stats, scores)"""
    C = np.asarray(logits).shape[1]
    thr = np.zeros(C, dtype=np.float32) if thresholds is None else np.asarray(thresholds, dtype=np.float32)
    order = restate_order(logits, labels, thr, rule=rule)
    stats = restate_walk(order, weights, rule=rule)
    return dict(order=order, groups=positive_groups(order), stats=stats, scores=close(stats))


def score_bounds(groups, classes):
    """name -> bound of a replicate's value ([C] for ap, scalars else)"""
    b_ap = np.array([ap_bound(int(g)) for g in groups])
    return dict(ap=b_ap, auroc=AUROC_BOUND, f1=F1_BOUND, map=macro_bound(float(b_ap.max()), classes),
                macro_auroc=macro_bound(AUROC_BOUND, classes), macro_f1=macro_bound(F1_BOUND, classes))


def compare_scores(got, ref, groups, classes):
    """{name: max error / bound} over replicates and classes; NaN must sit where the restatement has NaN.  AUROC and F1 bounds
    are relative, the values at most 1"""
    ratios = {}
    for name, bound in score_bounds(groups, classes).items():
        g, r = np.asarray(got[name], dtype=np.float64), np.asarray(ref[name], dtype=np.float64)
        assert g.shape == r.shape, (name, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), name
        err = np.where(np.isnan(r), 0.0, np.abs(g - r))
        ratios[name] = float((err / bound).max()) if err.size else 0.0
    return ratios


def percentile_limits(values, confidence):
    """[2, ...] numpy.nanpercentile limits (linear interpolation) of replicate values [m, ...]; all-NaN columns give NaN"""
    import warnings
    a = 100.0 * (1.0 - confidence) / 2.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanpercentile(values, [a, 100.0 - a], axis=0)


def repeat_rows(logits, labels, w):
    """the rows physically repeated by their multiplicities"""
    idx = np.repeat(np.arange(len(w)), w)
    return np.asarray(logits)[idx], np.asarray(labels)[idx]


# ---------------------------------------------------------------------------------------------- the cases
# name -> (logits float32 [n, C] holding values of `dtype`, labels bool [n, C], dtype name, replicates R (replicate 0 included),
#          seed, float32 [C] logit thresholds)

def _make(n, c, dtype, seed, quantum=None, density=0.3):
    g = np.random.default_rng(seed)
    s = g.standard_normal((n, c)).astype(np.float32)
    if quantum:
        s = (np.round(s / quantum) * quantum).astype(np.float32)
    if dtype == "bfloat16":
        s = M.to_bf16(s)
    elif dtype == "float16":
        s = s.astype(np.float16).astype(np.float32)
    y = g.random((n, c)) < density
    return s, y, dtype


def _thresholds(c, seed, dtype="float32"):
    """per-class logit thresholds on the quarter grid: some fall on scores of the quantised cases"""
    return (np.round(np.random.default_rng(seed).standard_normal(c) * 2) / 4).astype(np.float32)


_MAKERS = {
    "n1": lambda: (*M.case("n1"), 1, 3, np.zeros(1, dtype=np.float32)),
    "n63": lambda: (*_make(63, 17, "float32", 21), 63, 5, np.zeros(17, dtype=np.float32)),
    "n64": lambda: (*_make(64, 1, "float16", 22), 64, 6, _thresholds(1, 1)),
    "n65": lambda: (*_make(65, 65, "bfloat16", 23, quantum=0.5), 65, 7, _thresholds(65, 2)),
    "n257": lambda: (*_make(257, 17, "float32", 24, quantum=0.25, density=0.1), 130, 8, _thresholds(17, 3)),
    "n1025": lambda: (*M.case("bf16"), 65, 9, np.zeros(5, dtype=np.float32)),                 # one row past the 1024-key tile
    "quantised": lambda: (*M.case("quantised"), 64, 10, _thresholds(17, 4)),                  # 2049 x 17, degenerate classes
    "specials": lambda: (*M.case("specials"), 130, 11, np.zeros(4, dtype=np.float32)),        # NaN, +-inf, +-0, denormals
}
CASE_IDS = list(_MAKERS)
_CASES, _RESTATED = {}, {}


def case(name):
    if name not in _CASES:
        s, y, dtype, R, seed, thr = _MAKERS[name]()
        for a in (s, y, thr):
            a.setflags(write=False)
        _CASES[name] = (s, y, dtype, R, seed, thr)
    return _CASES[name]


def restated(name):
    """the drawn weights and the restatement of a case, computed once and shared"""
    if name not in _RESTATED:
        s, y, _, R, seed, thr = case(name)
        w = draw_weights(s.shape[0], R, seed)
        r = restate(s, y, w, thr)
        r["weights"] = w
        _RESTATED[name] = r
    return _RESTATED[name]


def caller_weights(n, rows, seed):
    """uint8 [rows, n] multiplicities holding 0 and 255, a row of zeros on the first half (a replicate that may lose every
    positive of a class) and a row of 255s"""
    g = np.random.default_rng(seed)
    w = g.choice(np.array([0, 0, 1, 1, 2, 3, 7, 255], dtype=np.uint8), size=(rows, n))
    w[0, : n // 2] = 0
    w[1] = 255
    return w
