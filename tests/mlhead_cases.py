"""Cases, float64 reference and bounds of the fused classifier head (aecf_amd/losses.py: linear_multilabel_loss and
MultilabelHead; aecf_mlhead_* of the library).

The definition (h [n, K] and W [C, K] bfloat16 as stored, bias float32 [C] or absent, t [n, C] targets, the element l and its
derivative g = dl/dz of tests/mlloss_cases.py):

    z = h W^T + bias        loss = sum l(z, t) (/ N)        dh = scale g W        dW = scale g^T h        dbias = scale sum_i g

``reference`` states it in float64 numpy with ``mlloss_cases.closed_form`` for the element.

The bounds are derived from the operations of aecf_amd/csrc/aecf_mlhead_flash.hip, not fitted to a run.  U = 2**-24.

    z          K products of two bfloat16 values are exact in float32 (16 significant bits).  The MFMAs add them into a float32
               accumulator; the order and the rounding of the adder inside an instruction are not documented, so every one of
               the K additions is given one rounding of at most 2 U (a truncating adder's), and the bias one more addition:
               |dz| <= c(K) U (sum_k |h w| + |bias|),   c(K) = 2 (K + 1)
    element    evaluated at the kernel's z it carries mlloss_cases' own float32 bounds (loss_err, grad_err).  The error of z
               moves the loss by at most (|g| + dg) |dz| and g by dg, where dg bounds |g(z') - g(z)| over |z' - z| <= |dz|:
               without a margin dg = G2 |dz| with |g'| <= G2 = (cp + cn) (1/4 + gamma + gamma^2 / 2), gamma the larger exponent:
               for P = cp u^y L (u = 1 - s, L = -log s) P'' = -cp u^y { -y s (y s L + u) + y s u L - y s u - s u }, and with
               s L <= 1/e, s u <= 1/4, u <= 1 its size is at most cp (y^2 / e + y / e + y / 2 + 1/4); the negative side is
               the mirror image.  With a margin the negative side has a kink at s = m and, for an exponent below 2, an
               unbounded second derivative beside it, so there dg is EVALUATED: twice the larger of |g(z +- dz) - g(z)| in
               float64 (g is monotone between its few turning points and dz is of the order 1e-4 |z|; the factor 2 covers a
               turning point inside the interval), plus the margin-free bound of the positive side.
    g as the   one rounding to bfloat16 in both gradient products: 8 significant bits, round to nearest even, so half a unit in
    B operand  the last place is at most 2**-8 of the value (mlloss_cases.U16 -- 2**-9 is the AVERAGE over a binade and is
               exceeded just above every power of two: 1 + 2**-8 rounds to 1); dbias sums the unrounded float32 g.
    products   g (bfloat16) times h or W (bfloat16) is exact; an output element is a float32 accumulation over the streamed
               rows of a split (``split(...)``: per of them, copies past the end weigh 0), again 2 U per addition, then the
               splits in order (U each): (2 per + KS) U sum |g h|.
    scalar     a lane adds the losses (and g) of the rows it meets in float32: at most per / 4 + 4 of them, U each; the four
    sums       lanes of a class and the splits are joined in float64 for the loss (and in float32, 2 + KS additions, for g).
    scale      upstream * factor (U), divided by N in float64 and rounded (U), times the sum (U): 3 U; a scale or a result
               below float32's normal range is rounded to a multiple of 2**-149: TINY32 (1 + |sum|) absolute.
    output     dh rounded once to bfloat16 (2**-8) or stored as float32; weight.grad / bias.grad of bfloat16 parameters are
               the float32 results cast once (2**-8).
First order throughout; the total is multiplied by mlloss_cases.SECOND_ORDER.  Valid counts and N are integers: demanded equal.
Where every target of a row (class) is unknown every g of it is an exact 0 by select, so dh of that row (dW and dbias of that
class) is demanded to be an exact zero, and everything when nothing is valid.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

from tests import mlloss_cases as M

U = M.U
U64 = M.U64
UB = M.U16["bfloat16"]              # one rounding to bfloat16: 2**-8
TINY32 = 2.0 ** -149
WIDTHS = (128, 256, 384, 512, 768, 1024)


class Split(NamedTuple):
    rule: int
    live: int
    per: int


def split(rows: int, cols: int) -> Split:
    """flash_split of aecf_amd/csrc/aecf_flash_stream.h: the streamed range (cols) of a role whose stationary rows are ``rows``"""
    rb = (rows + 63) // 64
    ks = max(1, min((256 + rb - 1) // rb, (cols + 511) // 512, 64))
    per = ((cols + ks - 1) // ks + 31) // 32 * 32
    return Split(ks, (cols + per - 1) // per, per)


def workspace_layout(n: int, C: int, K: int) -> int:
    al = lambda v: (v + 255) // 256 * 256
    kc, kr = split(C, n).live, split(n, C).live
    rows = max(kc * C, kr * n if kr > 1 else 0)
    return al(rows * K * 4) + al(kc * C * 8) + al(kc * C * 4) + al(kc * C * 4)


# name -> (n, C, K, form, label kind, ignore plan, bias)
CASES = {
    "H1": (1, 1, 128, "bce", "float32", "none", True),
    "H2": (33, 15, 128, "bce_w", "uint8", "none", True),
    "H2_i8": (33, 15, 128, "focal", "int8", "some", False),
    "H3": (65, 17, 256, "asl", "float32", "some", True),
    "H3_row": (65, 17, 256, "bce", "int8", "row", True),
    "H4": (64, 64, 384, "bce_soft", "bfloat16", "none", False),
    "H4_all": (64, 64, 384, "focal", "float32", "all", True),
    "H5": (63, 65, 512, "focal", "float32", "class", True),
    "H6": (1100, 15, 128, "bce_w", "float32", "some", True),
    "H7": (33, 1100, 128, "asl", "int8", "some", True),
    "H8": (40, 80, 768, "bce", "bool", "none", True),
    "H9": (40, 15, 1024, "bce_soft", "bfloat16", "some", False),
    "H10": (8, 15, 128, "bce", "float32", "specials", False),
    "H10_focal": (8, 15, 128, "focal", "float32", "specials", False),
}
CASE_IDS = list(CASES)
# the splits the table of cases relies on: name -> (CLS splits over the rows, ROW splits over the classes, CLS class blocks)
EXPECTED_SPLITS = {"H1": (1, 1, 1), "H2": (1, 1, 1), "H3": (1, 1, 1), "H4": (1, 1, 1), "H5": (1, 1, 2), "H6": (3, 1, 1),
                   "H7": (1, 3, 18), "H8": (1, 1, 2), "H9": (1, 1, 1), "H10": (1, 1, 1)}
SPECIAL_Z = (0.0, -0.0, 20.0, -20.0, 88.5, -88.5, 104.0, -104.0, 9984.0, -9984.0)


class Case(NamedTuple):
    form: M.Form
    h: np.ndarray                   # float32 [n, K], bfloat16 values
    w: np.ndarray                   # float32 [C, K], bfloat16 values
    bias: Optional[np.ndarray]      # float32 [C], bfloat16 values (the module may hold it in either dtype)
    t: np.ndarray                   # float32 [n, C]; unknown: NaN or -1 (alternating)
    valid: np.ndarray
    kind: str                       # the label dtype the case is run with
    pos_weight: Optional[np.ndarray]
    class_weight: Optional[np.ndarray]
    a: np.ndarray
    b: np.ndarray


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    n, C, K, form_name, kind, plan, with_bias = CASES[name]
    form = M.FORMS[form_name]
    g = np.random.default_rng(CASE_IDS.index(name) + 4000)
    h = M.to_bf16(g.standard_normal((n, K)).astype(np.float32))
    w = M.to_bf16((3.0 / np.sqrt(K)) * g.standard_normal((C, K)).astype(np.float32))
    bias = M.to_bf16(g.standard_normal(C).astype(np.float32)) if with_bias else None
    if form.soft:
        t = (g.integers(0, 17, size=(n, C)) / 16).astype(np.float32)            # sixteenths: exact in bfloat16
    else:
        t = (g.random((n, C)) < 0.3).astype(np.float32)
    valid = np.ones((n, C), dtype=bool)
    if plan == "some":
        valid = g.random((n, C)) >= 0.3
    elif plan == "row":
        valid = g.random((n, C)) >= 0.2
        valid[n // 2] = False
        valid[n - 1] = False
    elif plan == "class":
        valid[:, C // 2] = False
        valid[:, C - 1] = False
    elif plan == "all":
        valid[:] = False
    elif plan == "specials":
        # row i is the unit vector e_i, so z[i, c] = w[c, i] exactly; class c holds targets 1 (c % 3 == 0), 0 (== 1), unknown (== 2)
        h[:] = 0
        h[np.arange(n), np.arange(n)] = 1.0
        for i in range(n):
            for c in range(C):
                w[c, i] = SPECIAL_Z[(i + c) % len(SPECIAL_Z)]
        t = np.tile((np.arange(C) % 3 == 0).astype(np.float32), (n, 1))
        valid = np.tile(np.arange(C) % 3 != 2, (n, 1))
        assert np.array_equal(M.to_bf16(w), w)
    if kind in ("bool", "uint8"):
        assert valid.all()
    unknown = np.where((np.arange(n * C).reshape(n, C) % 2) == 0, np.float32(np.nan), np.float32(-1.0))
    t = np.where(valid, t, unknown).astype(np.float32)
    pw = cw = None
    if form.weights:
        pw = (0.25 + 4.0 * g.random(C)).astype(np.float32)
        cw = (0.5 + g.random(C)).astype(np.float32)
    a, b = M.fold(form, pw, cw, C)
    return Case(form, h, w, bias, t, valid, kind, pw, cw, a, b)


def labels_of(c: Case):
    """the label matrix of the case's kind as (numpy array, torch dtype name); int8 marks unknown with -1 and positives with 3"""
    if c.kind in ("float32", "bfloat16"):
        return c.t.copy(), c.kind
    hard = np.where(c.valid, c.t, 0.0) != 0
    if c.kind == "int8":
        return np.where(c.valid, hard.astype(np.int8) * 3, np.int8(-1)).astype(np.int8), "int8"
    return (hard.astype(np.uint8) * (7 if c.kind == "uint8" else 1)).astype(np.uint8), c.kind


# ---------------------------------------------------------------------------------------------- reference and bounds

def c_of_k(K: int) -> float:
    return 2.0 * (K + 1)


class Reference(NamedTuple):
    z: np.ndarray                   # float64 [n, C]
    loss: float
    n_valid: float
    stats: np.ndarray               # [2, C] loss sums | valid counts
    per_class: np.ndarray
    dh: np.ndarray                  # for upstream * factor = 1
    dw: np.ndarray
    db: np.ndarray
    loss_bound: float
    stats_bound: np.ndarray
    per_class_bound: np.ndarray
    dh_bound: np.ndarray            # float32 results, before a rounding into bfloat16 (``rounded``)
    dw_bound: np.ndarray
    db_bound: np.ndarray
    zero_rows: np.ndarray           # bool [n]: dh demanded exactly zero
    zero_classes: np.ndarray        # bool [C]: dW, dbias demanded exactly zero
    g: np.ndarray                   # unscaled dl/dz
    scale: float


def _elements(z, c: Case):
    return M.closed_form(z, c.t, c.valid, c.a, c.b, c.form)


def reference(c: Case, reduction: str = "mean", upstream: float = 1.0, world: int = 1) -> Reference:
    h, w = c.h.astype(np.float64), c.w.astype(np.float64)
    n, K = h.shape
    C = w.shape[0]
    bias = np.zeros(C) if c.bias is None else c.bias.astype(np.float64)
    form = c.form
    with np.errstate(all="ignore"):
        z = h @ w.T + bias[None, :]
        dz = c_of_k(K) * U * (np.abs(h) @ np.abs(w).T + np.abs(bias)[None, :])
        el = _elements(z, c)
        ts = np.where(c.valid, c.t.astype(np.float64), 0.0)
        tp = ts * (1.0 - form.eps) + form.eps / 2
        cp, cn = c.a.astype(np.float64)[None, :] * tp, c.b.astype(np.float64)[None, :] * (1.0 - tp)
        if form.m == 0:
            y = max(form.gp, form.gn)
            dg = (cp + cn) * (0.25 + y + 0.5 * y * y) * dz
        else:
            up_, dn_ = _elements(z + dz, c).grad, _elements(z - dz, c).grad
            dg = 2.0 * np.maximum(np.abs(up_ - el.grad), np.abs(dn_ - el.grad)) + cp * (0.25 + form.gp + 0.5 * form.gp ** 2) * dz
        dg = np.where(c.valid, dg, 0.0)
        g = el.grad
        ag = np.abs(g)
        e_l = el.loss_err + (ag + dg) * dz * c.valid
        e_g = el.grad_err + dg
        e_gb = e_g + UB * (ag + e_g)
        sc, sr = split(C, n), split(n, C)
        chain = sc.per // 4 + 4
        # loss sums
        sums = el.loss.sum(0)
        counts = c.valid.sum(0).astype(np.float64)
        mags = np.abs(el.loss).sum(0)
        sums_b = (e_l.sum(0) + (chain * U + (8 + sc.live + world) * U64) * mags) * M.SECOND_ORDER
        N = counts.sum()
        div = N if reduction == "mean" else 1.0
        loss = sums.sum() / div if div > 0 else 0.0
        loss_b = (sums_b.sum() / max(div, 1.0) + (U + (C + 16) * U64) * abs(loss)) * M.SECOND_ORDER
        per_class = np.where(counts > 0, sums / np.maximum(counts, 1.0), 0.0)
        per_class_b = (sums_b / np.maximum(counts, 1.0) + (U + 4 * U64) * np.abs(per_class)) * M.SECOND_ORDER
        scale = upstream * ((1.0 / div) if div > 0 else 0.0)
        asc = abs(scale)
        # gradients
        gh, gw = ag.T @ np.abs(h), ag @ np.abs(w)
        dw_u, dh_u, db_u = g.T @ h, g @ w, g.sum(0)
        dw_b = (e_gb.T @ np.abs(h) + ((2 * (sc.per + 32) + sc.live) * U + 3 * U) * gh) * asc + TINY32 * (1.0 + gh)
        dh_b = (e_gb @ np.abs(w) + ((2 * (sr.per + 32) + sr.live) * U + 3 * U) * gw) * asc + TINY32 * (1.0 + gw)
        db_b = (e_g.sum(0) + ((chain + 2 + sc.live) * U + 3 * U) * ag.sum(0)) * asc + TINY32 * (1.0 + ag.sum(0))
        zero_rows, zero_classes = ~c.valid.any(1), ~c.valid.any(0)
        dh_b[zero_rows] = 0.0
        dw_b[zero_classes] = 0.0
        db_b[zero_classes] = 0.0
        if scale == 0.0:
            dh_b[:], dw_b[:], db_b[:] = 0.0, 0.0, 0.0
    return Reference(z, float(loss), float(N), np.stack((sums, counts)), per_class, dh_u * scale, dw_u * scale, db_u * scale, float(loss_b),
                     sums_b, per_class_b, dh_b * M.SECOND_ORDER, dw_b * M.SECOND_ORDER, db_b * M.SECOND_ORDER, zero_rows, zero_classes,
                     g, scale)


def rounded(bound: np.ndarray, value: np.ndarray) -> np.ndarray:
    """a float32 result's bound after one more rounding into bfloat16"""
    return np.where(bound > 0, bound + UB * (np.abs(value) + bound), 0.0)


def check_zero(got, mask, what: str) -> None:
    got = np.asarray(got)
    assert not got[mask].any(), f"{what}: exact zeros demanded where every target is unknown"


# ---------------------------------------------------------------------------------------------- emulation (and broken rules)

RULES = ("bias_dropped", "bias_per_row", "z_bf16", "ignore_by_product", "count_ignored", "padded_rows_counted",
         "scale_before_rounding", "db_from_rounded_g", "targets_transposed")
RULE_OUTPUT = {"bias_dropped": "loss", "bias_per_row": "loss", "z_bf16": "loss", "ignore_by_product": "stats",
               "count_ignored": "n_valid", "padded_rows_counted": "counts", "scale_before_rounding": "dw",
               "db_from_rounded_g": "db", "targets_transposed": "counts"}


def _chain32(x: np.ndarray) -> np.ndarray:
    """float32 sum over axis 0, one addition after the other"""
    if x.shape[0] == 0:
        return np.zeros(x.shape[1:], dtype=np.float32)
    return np.cumsum(x.astype(np.float32), axis=0, dtype=np.float32)[-1]


def emulate(c: Case, reduction: str = "mean", upstream: float = 1.0, rule: Optional[str] = None, nan_at=None):
    """The design in float32 numpy: float32 z (numpy's own summation order, inside the same bound), the element by
    mlloss_cases.emulate, bfloat16 g in the products, a lane's float32 sums over the rows it meets, splits added in order.
    ``nan_at = (i, c)``: that logit is NaN (an unknown target's, for ignore_by_product).  Returns dict(loss, n_valid, stats, dh
    (float32, before the output rounding), dw, db)."""
    f = np.float32
    n, K = c.h.shape
    C = c.w.shape[0]
    t, valid = c.t, c.valid
    if rule == "targets_transposed":                                # element (i, c) read at c * n + i of the row-major matrix
        idx = (np.arange(C)[None, :] * n + np.arange(n)[:, None])
        t = c.t.reshape(-1)[idx]
        valid = c.valid.reshape(-1)[idx]
    with np.errstate(all="ignore"):
        z = (c.h @ c.w.T).astype(f)
        if c.bias is not None and rule != "bias_dropped":
            z = z + (c.bias[np.arange(n) % C][:, None] if rule == "bias_per_row" else c.bias[None, :])
        if rule == "z_bf16":
            z = M.to_bf16(z)
        if nan_at is not None:
            z[nan_at] = np.nan
        flat = M.Case(c.form, z.reshape(1, -1), t.reshape(1, -1), valid.reshape(1, -1), None, None, np.tile(c.a, n), np.tile(c.b, n))
        em = M.emulate(flat, "sum", rule="ignore_by_product" if rule == "ignore_by_product" else None)
        l = em["per_class"].reshape(n, C).astype(f)                 # one row per "class" of the flat case: the elements themselves
        g = em["grad"].reshape(n, C).astype(f)
        if rule == "ignore_by_product":
            l = (np.where(np.isnan(z), f(np.nan), l) * valid.astype(f)).astype(f)
        sc, sr = split(C, n), split(n, C)
        sums = np.zeros(C)
        gsum = np.zeros(C, dtype=f)
        counts = np.zeros(C)
        dw = np.zeros((C, K), dtype=f)
        for s in range(sc.live):
            lo, hi = s * sc.per, min((s + 1) * sc.per, n)
            rows = np.arange(lo, hi)
            lane = ((rows - lo) % 16) // 4
            ls = [_chain32(l[rows[lane == q]]) for q in range(4)]
            gs = [_chain32(g[rows[lane == q]]) for q in range(4)]
            sums += (ls[0].astype(np.float64) + ls[1]) + (ls[2].astype(np.float64) + ls[3])
            gsum = gsum + ((gs[0] + gs[1]) + (gs[2] + gs[3]))
            counts += valid[lo:hi].sum(0)
            if rule == "padded_rows_counted" and (hi - lo) % 16:
                counts += valid[hi - 1] * (16 - (hi - lo) % 16)
            gb = g[lo:hi]
            if rule != "scale_before_rounding":
                dw = dw + (M.to_bf16(gb).T @ c.h[lo:hi]).astype(f)
        N = float(n * C) if rule == "count_ignored" else counts.sum()
        total = sums.sum()
        div = N if reduction == "mean" else 1.0
        loss = f(total / div) if div > 0 else f(0.0)
        scale = f(np.float64(f(upstream)) / div) if div > 0 else f(0.0)
        if rule == "scale_before_rounding":
            dw_out = (M.to_bf16(g * scale).T @ c.h).astype(f)
            dh_out = (M.to_bf16(g * scale) @ c.w).astype(f)
        else:
            dh = np.zeros((n, K), dtype=f)
            for s in range(sr.live):
                lo, hi = s * sr.per, min((s + 1) * sr.per, C)
                dh = dh + (M.to_bf16(g[:, lo:hi]) @ c.w[lo:hi]).astype(f)
            dw_out, dh_out = dw * scale, dh * scale
        if rule == "db_from_rounded_g":
            gsum = _chain32(M.to_bf16(g))
        db_out = gsum * scale
    return dict(loss=loss, n_valid=N, stats=np.stack((sums, counts)), dh=dh_out, dw=dw_out, db=db_out)
