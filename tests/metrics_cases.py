"""Cases, float64 restatement and bounds of the multi-label evaluation (aecf_amd/metrics.py, aecf_mlmetrics_* of the library).

The restatement.  For class c the valid entries are the non-NaN logits.  For every valid positive i, over the valid entries j:
``ge_all_i = #{s_j >= s_i}``, ``gt_all_i = #{s_j > s_i}``, ``ge_pos_i`` / ``gt_pos_i`` the same over the positives.  Then

    AP    = (1 / npos) sum_i ge_pos_i / ge_all_i
    AUROC = sum_i (lt_neg_i + eq_neg_i / 2) / (npos nneg),   lt_neg_i = (nvalid - ge_all_i) - (npos - ge_pos_i),
                                                             eq_neg_i = (ge_all_i - gt_all_i) - (ge_pos_i - gt_pos_i)
    F1    = 2 TP / (2 TP + FP + FN) at logit > float32(log(t / (1 - t))), over the valid entries

``restate`` forms the counts with a sort of the keys and a binary search (an independent route to the same integers: the
library compares every pair) and sums with ``math.fsum``.

The bounds (U = 2**-53, the unit roundoff of float64; every value is at most 1, so relative and absolute bounds agree).
 AP.  The library's finalize gives lane t of 256 the rows t, t + 256, .. of a rank, so a lane adds at most ceil(n / 256)
   quotients in sequence; a tree of 8 levels adds the lanes; the all-reduce adds ``world`` shares; then one division by npos.
   Every quotient ge_pos / ge_all carries one rounding.  With the standard bound (1 + U)^k on a sum of k roundings of
   non-negative terms:  ceil(n / 256) - 1 + 8 + (world - 1) + 1 + 1  roundings.  The restatement's quotients carry one rounding,
   its fsum one, its division one: 3 more.  ``ap_bound`` is their sum times U -- 2.6e-15 at n = 2049, far under the 1e-12 cap.
 AUROC.  lt_neg + eq_neg / 2 is a half-integer and so is every partial sum, far below 2**52: the sums are exact on both sides in
   any order, npos nneg is an exact integer, and both sides round the same exact quotient once.  They agree bit for bit; the
   bound allows the one ulp of a division that is not correctly rounded, 2 U.
 F1.  The same: integers, one division.  2 U.
 Macro values.  A mean over m <= C per-class values adds at most C - 1 + 1 roundings in the library's float64 torch ops and 2 in
   the restatement: ``macro_bound(b, C) = b + (C + 2) U``.
Integer outputs (the count arrays, n_pos, n_invalid) are compared for equality.
"""
import math

import numpy as np

A = 256             # anchors per block of the counting kernel (MLM_A in aecf_amd/csrc/aecf_metrics.hip)
K = 1024            # keys per LDS tile (MLM_K)
U = 2.0 ** -53
CAP = 1e-12


def ap_bound(n_all: int, world: int = 1) -> float:
    b = ((n_all + 255) // 256 - 1 + 8 + (world - 1) + 1 + 1 + 3) * U
    assert b < CAP
    return b


AUROC_BOUND = 2 * U
F1_BOUND = 2 * U


def macro_bound(b: float, classes: int) -> float:
    return b + (classes + 2) * U


def logit_threshold(threshold: float) -> np.float32:
    return np.float32(math.log(threshold / (1.0 - threshold)))


def to_bf16(x: np.ndarray) -> np.ndarray:
    """float32 values rounded to the nearest bfloat16 (ties to even), as float32"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return b.astype(np.uint32).view(np.float32).reshape(x.shape)


# ---------------------------------------------------------------------------------------------- the cases
# name -> (logits float32 [N, C] holding values of `dtype`, labels bool [N, C], dtype name)

def _draw(seed, n, c, density=0.2):
    g = np.random.default_rng(seed)
    return g, g.standard_normal((n, c)).astype(np.float32), g.random((n, c)) < density


def _continuous(n, seed):
    _, s, y = _draw(seed, n, 3)
    return s, y, "float32"


def _n1():
    return np.array([[0.25]], dtype=np.float32), np.array([[True]]), "float32"


def _quantised():
    n = 2 * K + 1
    _, s, y = _draw(11, n, 17)
    s = (np.round(1.5 * s * 4) / 4).astype(np.float32)
    y[:, 0] = False                     # no positive
    y[:, 1] = True                      # only positives
    y[:, 2] = False
    y[1234, 2] = True                   # one positive
    y[:, 3] = True
    y[77, 3] = False                    # one negative
    return s, y, "float32"


def _low(dtype, seed):
    _, s, y = _draw(seed, 1025, 5)
    s = to_bf16(s) if dtype == "bfloat16" else s.astype(np.float16).astype(np.float32)
    return s, y, dtype


def _specials():
    g, s, y = _draw(17, 300, 4)
    s = (np.round(s * 4) / 4).astype(np.float32)
    tiny = np.float32(1e-45)            # the smallest denormal
    specials = np.array([np.inf, -np.inf, 0.0, -0.0, tiny, -tiny, 3 * tiny, np.float32(1.1e-38), np.nan, -np.nan], dtype=np.float32)
    for c in range(4):
        rows = g.permutation(300)[:80]
        s[rows, c] = np.tile(specials, 8)
        y[rows[:40], c] = True          # every special value, NaN included, on positive rows ...
        y[rows[40:], c] = False         # ... and on negative rows
    s[:, 3] = np.where(np.isnan(s[:, 3]), s[:, 3], np.where(y[:, 3], np.float32(0.0), np.float32(-0.0)))   # +0 against -0 only
    return s, y, "float32"


_MAKERS = {
    "n1": _n1,
    "a_minus": lambda: _continuous(A - 1, 1),
    "a": lambda: _continuous(A, 2),
    "a_plus": lambda: _continuous(A + 1, 3),
    "quantised": _quantised,
    "bf16": lambda: _low("bfloat16", 5),
    "f16": lambda: _low("float16", 6),
    "specials": _specials,
}
CASE_IDS = list(_MAKERS)
_CASES = {}
_RESTATED = {}


def case(name):
    if name not in _CASES:
        s, y, dtype = _MAKERS[name]()
        s.setflags(write=False)
        y.setflags(write=False)
        _CASES[name] = (s, y, dtype)
    return _CASES[name]


def restated(name):
    """the restatement of a case, computed once and shared"""
    if name not in _RESTATED:
        s, y, _ = case(name)
        _RESTATED[name] = restate(s, y)
    return _RESTATED[name]


# ---------------------------------------------------------------------------------------------- the restatement

def _above(sorted_keys, x, strict):
    """#{k in sorted_keys : k > x} (strict) or >= x, for every x"""
    return len(sorted_keys) - np.searchsorted(sorted_keys, x, side="right" if strict else "left")


def restate(logits, labels, threshold=0.5, rule=None):
    """dict: counts int64 [4, C, N] (ge_all | gt_all | ge_pos | gt_pos, 0 where the entry is not a valid positive), shares
    float64 [5, C], ap / auroc / f1 float64 [C], n_pos / n_invalid int64 [C], map / macro_auroc / macro_f1.

    ``rule`` breaks one rule on purpose (tests/test_metrics_cpu.py): "gt_for_ge" counts ge_all with >, "nan_key" keeps NaN as a
    key (above everything, where a descending sort puts it), "neg_anchors" lets every valid entry be an anchor, "no_half" drops
    the 1/2 of the tie term, "f1_invalid" counts F1 over the invalid rows too."""
    s = np.asarray(logits, dtype=np.float32)
    y = np.asarray(labels) != 0
    n, C = s.shape
    thr = logit_threshold(threshold)
    counts = np.zeros((4, C, n), dtype=np.int64)
    shares = np.zeros((5, C))
    ap, auroc, f1 = np.zeros(C), np.full(C, np.nan), np.zeros(C)
    n_pos, n_invalid = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64)
    for c in range(C):
        valid = ~np.isnan(s[:, c])
        pos = valid & y[:, c]
        anchors = valid if rule == "neg_anchors" else pos
        keys = np.sort(s[valid, c].astype(np.float64))
        pkeys = np.sort(s[pos, c].astype(np.float64))
        a = s[anchors, c].astype(np.float64)
        ge_all = _above(keys, a, strict=(rule == "gt_for_ge"))
        gt_all = _above(keys, a, strict=True)
        if rule == "nan_key":
            ge_all, gt_all = ge_all + (n - valid.sum()), gt_all + (n - valid.sum())
        ge_pos, gt_pos = _above(pkeys, a, strict=False), _above(pkeys, a, strict=True)
        npos, nvalid = int(pos.sum()), int(valid.sum()) + (int(n - valid.sum()) if rule == "nan_key" else 0)
        nneg = nvalid - npos
        n_pos[c], n_invalid[c] = npos, n - int(valid.sum())
        for k, v in enumerate((ge_all, gt_all, ge_pos, gt_pos)):
            counts[k, c, anchors] = v
        lt_neg = (nvalid - ge_all) - (npos - ge_pos)
        eq_neg = (ge_all - gt_all) - (ge_pos - gt_pos)
        shares[0, c] = math.fsum(ge_pos / np.maximum(ge_all, 1).astype(np.float64))
        shares[1, c] = math.fsum(lt_neg + (0.0 if rule == "no_half" else 0.5) * eq_neg)
        with np.errstate(invalid="ignore"):
            pred = s[:, c] > thr                        # a NaN compares false
        rows = np.ones(n, dtype=bool) if rule == "f1_invalid" else valid
        yes = y[:, c] & rows
        shares[2, c] = int((yes & pred).sum())
        shares[3, c] = int((~y[:, c] & rows & pred).sum())
        shares[4, c] = int((yes & ~pred).sum())
        if npos > 0:
            ap[c] = shares[0, c] / npos
            if nneg > 0:
                auroc[c] = shares[1, c] / (npos * nneg)
            if shares[2, c] > 0:
                f1[c] = 2 * shares[2, c] / (2 * shares[2, c] + shares[3, c] + shares[4, c])
    out = dict(counts=counts, shares=shares, ap=ap, auroc=auroc, f1=f1, n_pos=n_pos, n_invalid=n_invalid)
    out.update(macros(ap, auroc, f1, n_pos))
    return out


def macros(ap, auroc, f1, n_pos):
    has = n_pos > 0
    both = ~np.isnan(auroc)
    return dict(map=math.fsum(ap[has]) / has.sum() if has.any() else 0.0,
                macro_auroc=math.fsum(auroc[both]) / both.sum() if both.any() else float("nan"),
                macro_f1=math.fsum(f1[f1 > 0]) / (f1 > 0).sum() if (f1 > 0).any() else 0.0)


def position_tie_map(logits, labels):
    """aecf_amd.train_xray.mean_average_precision in float64 numpy: ties broken by position (a stable descending sort)"""
    s = np.asarray(logits, dtype=np.float64)
    y = (np.asarray(labels) != 0).astype(np.float64)
    order = np.argsort(-s, axis=0, kind="stable")
    hit = np.take_along_axis(y, order, 0)
    prec = np.cumsum(hit, 0) / np.arange(1, s.shape[0] + 1)[:, None]
    npos = y.sum(0)
    ap = (prec * hit).sum(0) / np.maximum(npos, 1.0)
    keep = npos > 0
    return float(ap[keep].mean()) if keep.any() else 0.0


def compare(got, ref, n_all, classes, world=1):
    """{name: error / bound} of the float outputs of a result (numpy arrays / floats) against the restatement; NaN must sit
    where the restatement has NaN.  Integer outputs are the caller's to compare for equality."""
    b_ap = ap_bound(n_all, world)
    bounds = dict(ap=b_ap, auroc=AUROC_BOUND, f1=F1_BOUND, map=macro_bound(b_ap, classes),
                  macro_auroc=macro_bound(AUROC_BOUND, classes), macro_f1=macro_bound(F1_BOUND, classes))
    ratios = {}
    for name, bound in bounds.items():
        g, r = np.asarray(got[name], dtype=np.float64), np.asarray(ref[name], dtype=np.float64)
        assert g.shape == r.shape, name
        assert np.array_equal(np.isnan(g), np.isnan(r)), name
        err = np.where(np.isnan(r), 0.0, np.abs(g - r))
        ratios[name] = float(err.max()) / bound if err.size else 0.0
    return ratios
