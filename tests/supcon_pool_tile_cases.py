"""Cases, float64 reference, derived bounds and a CPU emulation shared by tests/test_supcon_pool_tile_cpu.py and
tests/test_supcon_pool_tile_gpu.py: the tile-GEMM form of the pooled supervised contrastive loss (aecf_supcon_pool_sym_pass1 / _loss /
_grads: the EPI_SUP and EPI_SUP_SELF logits epilogues, sup_sums_kernel, sup_pool_combine_kernel, sup_finalize_kernel, the two
sup_weights_kernel variants and the gradient products of aecf_nce_gemm.hip).  Rows, shards, twins and geometry are those of
tests/nce_tile_cases.py, cases S1 - S4, the labels the plan of tests/supcon_tile_cases.plan, both imported, not copied; "S3u" is S3
with every label -1.  The reference's formulas are the pooled ones of tests/supcon_pool_cases.reference over both anchor halves,
with supcon_pool_cases.match_matrix of the plan.  Nothing here touches a GPU; every function works on the device of its tensors.

The problem.  n rows of two views a, b (unit bf16 rows) with ONE label per pair (shared by the views), dealt over shards (emulated
ranks); shard s owns rows lo .. hi.  The 2 n rows are one pool; every row is an anchor, itself left out; its positives are the
partner (by index) and every other row of either view with its non-negative label:
  anchors of view a:  keys [b | a], partner at column i,     excluded at column n + i        (supcon_pool_cases, off = 0, self_off = n)
  anchors of view b:  keys [b | a], partner at column n + i, excluded at column i            (off = n, self_off = 0)
With Ga = Pa - Mna, Gb = Pb - Mnb [n, 2 n] (P the softmax, 0 on the excluded key; Mn = match / n_i) the three blocks carry
  G_X = Ga[:, :n] + Gb[:, n:]^T      Q_X = Pa[:, :n] + Pb[:, n:]^T      Mn_X = m_X (1 / na_i + 1 / nb_j), the partner in m_X
  G_Y = Ga[:, n:]                    Q_Y = Pa[:, n:]                    Mn_Y = m_Y / na_i            (all 0 on the diagonal)
  G_Z = Gb[:, :n]                    Q_Z = Pb[:, :n]                    Mn_Z = m_Z / nb_i            (all 0 on the diagonal)
and a shard's outputs are those of tests/ntxent_tile_cases.py over these G (loss_rows, da_loc, db_loc, the shares da_all, db_all,
dT), plus the three column statistics it hands to the all-reduce (ml = the match by LABEL, the partner / the anchor excluded):
  colsum = sum_{i in s} E_X[i, :]           + the row sums of E_Z[s] on columns lo .. hi
  colcnt = sum_{i in s} ml_X[i, :]          + the row sums of ml_Z[s] on columns lo .. hi
  colsx  = sum_{i in s} (ml_X S_X)[i, :]    + the row sums of (ml_Z S_Z)[s] on columns lo .. hi
The shares add up to the pooled gradients (``pooled_check``).  The labels are shared, so ml_X = ml_Y = ml_Z as matrices: the counts
of the X and Y blocks agree row by row (``composition`` checks it, and that the excluded key is never a positive).

Bounds.  Elementwise, derived from the roundings of the design, never from results, no further factor.  They are those of
tests/ntxent_tile_cases.py (eps_e, eps_l, eps_cs, eps_Da = eps_l + h, eps_Db, the two-product outputs with 2 (Cp + 32) / 2 (Rp + 32)
terms, dT over three products, M with ln(2 n)) with the label terms of tests/supcon_tile_cases.py (counts exact; matched sums with
dr = 22 + ceil(n_tiles / 4) additions per row element and dcs = 15 + ceil(m_tiles / 4) per column element; the mean; the matched
weight bound) -- EPI_SUP_SELF sums a row's matches in EPI_SUP's order, so dr holds for Y and Z.  What this design adds:
  ONE float32 addition on each combined statistic.
    counts: ka = nX + nY <= 2 n - 2 and kb likewise are integers below 2^24, exact in any order: bound 0.
    sa_i = fl(sX_i + sY_i): |d sa_i| <= 4 s_err ka_i + (dr + 1) h sum over both blocks of ml |S|.
    colsx on a rank's own range = fl(scX + sZ): the two bounds (column: dcs, row of Z: dr) plus h (|scX| + |sZ| + the two bounds);
      elsewhere the column bound of supcon_tile_cases.  colsum: as ntxent_tile_cases (max(eps_cs, eps_l) + h on the own range).
    sb = the float32 sum of the shards' colsx in rank order: dc = max over shards of max(dcs, dr) + 1 + shards - 1 additions.
  mean_a = (dot + sa) * (1 / na): supcon_tile_cases' (dr + 4) h A becomes (dr + 5) h Aa_i, Aa_i = (sum over X and Y of m |S|) / na_i,
      and NOTHING where ka_i = 0 (0 + 0 = 0, 1 / 1 = 1: mean = dot exactly); mean_b with (dc + 4) h Ab_g.
  loss_i = nce_row_term(Da) + nce_col_term(Db):
      |d loss_i| <= eps_Da + eps_Db + 8 s_err / T + [ka_i > 0] (dr + 5) h Aa_i / T + [kb_g > 0] (dc + 4) h Ab_g / T + 4 h xm + 12 h M
  W_X: supcon_tile_cases' three weight bounds (no match / match by label / partner) with Q_X, Mn_X, G_X, the combined counts in
      [ka_i + kb_i > 0] and eps_w = eps_e + max(eps_Da, eps_Db) + 10 h.
  W_Y, W_Z: the same no-match and match bounds at v = 0 and 1 / nc = 0 (u + 0 and rn + 0 are exact; the counts of roundings stay
      upper bounds), Q = Q_Y / Q_Z, Mn = Mn_Y / Mn_Z.  The excluded key is bf16(ct 0) = 0 exactly and Q, Mn, G are 0 there: only
      the flush term remains.
With every label -1 every Mn term is the partner's alone and the bounds are those of ntxent_tile_cases.

The label plan puts, on S2 / S3 / S4, 192 / 225 / 1685 rows with a label positive, each with at most 53 / 63 / 119 positives over both
views, the partner among them (``composition``)."""
import functools
import math

import torch

from tests import nce_tile_cases as N
from tests import ntxent_tile_cases as X
from tests import supcon_pool_cases as P
from tests import supcon_tile_cases as L
from tests.nce_stream_cases import EPS_P, FLUSH, used_temperature  # noqa: F401  (used_temperature: for the tests)

H = N.H
TEMPS = N.TEMPS
MIN_T = N.MIN_T
TILE_IDS = ("S1", "S2", "S3", "S4")
CASE_IDS = TILE_IDS + ("S3u",)
GRADS = X.GRADS
STATS = ("colsum", "colcnt", "colsx")
OUTPUTS = STATS + ("loss_rows",) + GRADS + ("dT",)


def base(cid):
    return "S3" if cid == "S3u" else cid


@functools.lru_cache(maxsize=None)
def make_case(cid):
    """nce_tile_cases.make_symmetric (a, b [n, d] bf16 unit rows on the CPU, shards, coef = 0.5 / n, twins) plus lab [n] int64: the
    plan of supcon_tile_cases, or every label -1 (S3u)"""
    assert cid in CASE_IDS
    c = dict(N.make_symmetric(base(cid)))
    n = c["a"].shape[0]
    lab = L.plan(n, c["twins"])[0] if cid != "S3u" else torch.full((n,), -1, dtype=torch.int64)
    c.update(lab=lab)
    return c


def score_error(cid):
    return X.score_error(base(cid))


def workspace_bytes_py(rows, cols, d):
    """sup_pool_carve() + 256: three E blocks, the row and column partials of three quantities, three sets of row statistics, 1/Da,
    1/na, 1/Db, 1/nb, the last two at the partner, ediag, zeros, the dT partials, the slabs of two da products, the float32 stage
    of db_all -- each rounded up to 256 bytes"""
    g = N.geometry(rows, cols, d)
    Rp, Cp = g["Rp"], g["Cp"]
    parts = [Rp * Cp * 2] * 3 + [3 * g["n_tiles"] * Rp * 4, 3 * g["m_tiles"] * Cp * 4] + [3 * Rp * 4] * 3 + \
        [Rp * 4, Rp * 4, Cp * 4, Cp * 4, Rp * 4, Rp * 4, Rp * 4, Cp * 4,
         3 * 32 * 16 * g["m_tiles"] * 4, 2 * g["splits"] * rows * d * 4, 2 * cols * d * 4]
    return sum(N.up256(p) for p in parts) + 256


def label_block(lab):
    """bool [n, n]: the same non-negative label, the diagonal (the partner in X, the anchor in Y and Z) excluded"""
    m = L.label_matrix(lab, lab)
    i = torch.arange(lab.shape[0], device=lab.device)
    m[i, i] = False
    return m


def pooled(a, b, lab, T, coef):
    """supcon_pool_cases.reference over both anchor halves of the whole problem: (ref of view a's anchors, ref of view b's anchors,
    their match matrices), keys [b | a]"""
    n = a.shape[0]
    dev = a.device
    pool = torch.cat([b, a])
    lab = lab.to(dev)
    lab_pool = torch.cat([lab, lab])
    ma, mb = P.match_matrix(lab, lab_pool, 0, n), P.match_matrix(lab, lab_pool, n, 0)
    ra = P.reference(a, pool, ma, P.excluded(n, 2 * n, n, dev), T, coef)
    rb = P.reference(b, pool, mb, P.excluded(n, 2 * n, 0, dev), T, coef)
    return ra, rb, ma, mb


def composition(cid):
    """what the plan composes to on a case: (rows with a label positive, the most positives of one anchor over both views, the
    partner among them, the excluded key is a positive somewhere, the X and Y counts agree row by row)"""
    c = make_case(cid)
    n = c["a"].shape[0]
    lab = c["lab"]
    lab_pool = torch.cat([lab, lab])
    ma, mb = P.match_matrix(lab, lab_pool, 0, n), P.match_matrix(lab, lab_pool, n, 0)
    i = torch.arange(n)
    k = ma.sum(1) - 1
    self_positive = bool(ma[i, n + i].any() or mb[i, i].any())
    ml_x = ma[:, :n].clone()
    ml_x[i, i] = False
    agree = bool(torch.equal(ml_x.sum(1), ma[:, n:].sum(1))) and bool(torch.equal(ma, torch.cat([mb[:, n:], mb[:, :n]], 1)))
    return int((k > 0).sum()), int(k.max()) + 1, self_positive, agree


def reference(a, b, lab, shards, T, coef, s_err):
    """float64 on the device of a and b [n, d].  Returns (ref, bnd): loss_rows, da_loc, db_loc [n ...] whole; colsum, colcnt, colsx,
    da_all, db_all, dT lists, one entry per shard (the shard's share); da_all_sum / db_all_sum the shares added up, with the summed
    bounds."""
    a64, b64 = a.double(), b.double()
    n, d = a64.shape
    dev = a.device
    lab = lab.to(dev)
    ct = coef / T
    ra, rb, ma, mb = pooled(a, b, lab, T, coef)
    Pa, Pb, Mna, Mnb = ra["P"], rb["P"], ra["Mn"], rb["Mn"]
    idx = torch.arange(n, device=dev)
    QX, MnX = Pa[:, :n] + Pb[:, n:].T, Mna[:, :n] + Mnb[:, n:].T
    QY, MnY = Pa[:, n:], Mna[:, n:]
    QZ, MnZ = Pb[:, :n], Mnb[:, :n]
    GX, GY, GZ = QX - MnX, QY - MnY, QZ - MnZ
    loss = ra["loss_rows"] + rb["loss_rows"]
    Ml = label_block(lab)
    Mlf = Ml.double()
    xm, S = 0.0, {}
    for x, y, name in ((a64, b64, "X"), (a64, a64, "Y"), (b64, b64, "Z")):
        S[name] = x @ y.T
        xm = max(xm, float(torch.maximum(S[name].abs(), (S[name] - 1.0).abs()).max()) / T)
    EX = torch.exp((S["X"] - 1.0) / T)
    EZ = torch.exp((S["Z"] - 1.0) / T)
    EZ[idx, idx] = 0.0
    aSX, aSY, aSZ = S["X"].abs(), S["Y"].abs(), S["Z"].abs()
    ka, kb = 2.0 * Mlf.sum(1), 2.0 * Mlf.sum(0)                 # the label positives of anchor a_i / b_g over both views
    dotabs = aSX[idx, idx]
    Aa = (dotabs + (Mlf * aSX).sum(1) + (Mlf * aSY).sum(1)) / (1.0 + ka)
    Ab = (dotabs + (Mlf * aSX).sum(0) + (Mlf * aSZ).sum(1)) / (1.0 + kb)
    aa, ab = a64.abs(), b64.abs()
    geoms = [N.geometry(hi - lo, n, d) for lo, hi in shards]
    eps_e = 4.0 * s_err / T + 6.0 * H * xm + 2.0 * H
    deep = max(max(15 + -(-g["m_tiles"] // 4), 12 + -(-g["n_tiles"] // 4)) for g in geoms)
    eps_Db = eps_e + (deep + 1 + len(shards) - 1) * H
    dc = max(max(15 + -(-g["m_tiles"] // 4), 22 + -(-g["n_tiles"] // 4)) for g in geoms) + 1 + len(shards) - 1
    M = xm + 1.0 / T + math.log(2 * n)
    flush = FLUSH * (1.0 + ct)
    ref = dict(loss_rows=loss, da_loc=torch.empty_like(a64), db_loc=torch.empty_like(a64), da_all=[], db_all=[], dT=[], colsum=[],
               colcnt=[], colsx=[])
    bnd = dict(loss_rows=torch.empty_like(loss), da_loc=torch.empty_like(a64), db_loc=torch.empty_like(a64), da_all=[], db_all=[],
               dT=[], colsum=[], colcnt=[], colsx=[])

    def weight_bound(Q, Mn, G, eps_w):
        plain = ct * ((1.0 + EPS_P) ** 2 * (1.0 + eps_w) - 1.0) * Q + flush
        matched = ct * (EPS_P * G.abs() + (1.0 + EPS_P) * (((1.0 + EPS_P) * (1.0 + eps_w) - 1.0) * Q + 5.0 * H * Mn
                                                           + 9.0 * H * G.abs())) + flush
        return torch.where(Mn > 0, matched, plain)

    for (lo, hi), g in zip(shards, geoms):
        rows = hi - lo
        sl = slice(lo, hi)
        dr, dcs = 22 + -(-g["n_tiles"] // 4), 15 + -(-g["m_tiles"] // 4)
        eps_l = eps_e + (12 + -(-g["n_tiles"] // 4)) * H
        eps_cs = eps_e + (15 + -(-g["m_tiles"] // 4)) * H
        eps_Da = eps_l + H
        eps_w = eps_e + max(eps_Da, eps_Db) + 10.0 * H
        bnd["loss_rows"][sl] = (eps_Da + eps_Db + 8.0 * s_err / T + (ka[sl] > 0) * (dr + 5) * H * Aa[sl] / T
                                + (kb[sl] > 0) * (dc + 4) * H * Ab[sl] / T + 4.0 * H * xm + 12.0 * H * M)
        ii, pos = torch.arange(rows, device=dev), idx[sl]
        BX = weight_bound(QX[sl], MnX[sl], GX[sl], eps_w)
        gd, any_k = GX[sl][ii, pos].abs(), ((ka[sl] + kb[sl]) > 0).double()
        BX[ii, pos] = ct * (EPS_P * gd + (1.0 + EPS_P) * (eps_w * QX[sl][ii, pos] + any_k * 5.0 * H * MnX[sl][ii, pos]
                                                          + 8.0 * H * gd)) + flush
        BY = weight_bound(QY[sl], MnY[sl], GY[sl], eps_w)
        BZ = weight_bound(QZ[sl], MnZ[sl], GZ[sl], eps_w)
        mX, mY, mZ = ct * GX[sl].abs() + BX, ct * GY[sl].abs() + BY, ct * GZ[sl].abs() + BZ
        nC, nR = (g["Cp"] + 32) * H, (g["Rp"] + 32) * H
        # single-product bounds (the float32 accumulators dT is taken from), then the outputs
        bX1, bY1, bZ1 = (BX + nC * mX) @ ab, (BY + nC * mY) @ aa, (BZ + nC * mZ) @ ab
        vX, vY, vZ = ct * (GX[sl] @ b64), ct * (GY[sl] @ a64), ct * (GZ[sl] @ b64)
        ref["da_loc"][sl] = vX + vY
        bnd["da_loc"][sl] = (BX + 2.0 * nC * mX) @ ab + (BY + 2.0 * nC * mY) @ aa
        ref["db_loc"][sl] = vZ
        bnd["db_loc"][sl] = bZ1
        ref["da_all"].append(ct * (GY[sl].T @ a64[sl]))
        bnd["da_all"].append((BY + nR * mY).T @ aa[sl])
        ref["db_all"].append(ct * (GX[sl].T @ a64[sl] + GZ[sl].T @ b64[sl]))
        bnd["db_all"].append((BX + 2.0 * nR * mX).T @ aa[sl] + (BZ + 2.0 * nR * mZ).T @ ab[sl])
        dT = -(1.0 / T) * float((a64[sl] * (vX + vY)).sum() + (b64[sl] * vZ).sum())
        depth = 145 + -(-(3 * g["splits"] * g["m_tiles"] * g["d_tiles"]) // 256)
        B = float((aa[sl] * (bX1 + bY1)).sum() + (ab[sl] * bZ1).sum())
        V = float((aa[sl] * (vX.abs() + vY.abs())).sum() + (ab[sl] * vZ.abs()).sum())
        ref["dT"].append(dT)
        bnd["dT"].append((B + depth * H * (V + B)) / T + 3.0 * H * abs(dT))
        # the three column statistics: block X's columns, plus block Z's rows on the shard's own range (one addition each)
        cs = EX[sl].sum(0)
        e_cs = torch.full_like(cs, eps_cs)
        cs[sl] += EZ[sl].sum(1)
        e_cs[sl] = max(eps_cs, eps_l) + H
        ref["colsum"].append(cs)
        bnd["colsum"].append(e_cs * cs)
        Mls = Mlf[sl]
        cnt = Mls.sum(0)
        cnt[sl] += Mls.sum(1)
        ref["colcnt"].append(cnt)
        bnd["colcnt"].append(torch.zeros(n, dtype=torch.float64, device=dev))
        sxc, sxz = (Mls * S["X"][sl]).sum(0), (Mls * S["Z"][sl]).sum(1)
        b_c = 4.0 * s_err * Mls.sum(0) + dcs * H * (Mls * aSX[sl]).sum(0)
        b_z = 4.0 * s_err * Mls.sum(1) + dr * H * (Mls * aSZ[sl]).sum(1)
        sx, b_sx = sxc.clone(), b_c.clone()
        sx[sl] += sxz
        b_sx[sl] = b_c[sl] + b_z + H * ((Mls * aSX[sl]).sum(0)[sl] + (Mls * aSZ[sl]).sum(1) + b_c[sl] + b_z)
        ref["colsx"].append(sx)
        bnd["colsx"].append(b_sx)
    for name in ("da_all", "db_all"):
        ref[name + "_sum"], bnd[name + "_sum"] = sum(ref[name]), sum(bnd[name])
    return ref, bnd


def pooled_check(a, b, lab, shards, T, coef):
    """largest |difference| between this module's shares, added up, and the pooled gradients of supcon_pool_cases.reference (dq of
    each half on its own rows, dk on the pool [b | a]), relative to the largest gradient or to 1: float64 rounding only"""
    n = a.shape[0]
    ref, _ = reference(a, b, lab, shards, T, coef, 0.0)
    ra, rb, _, _ = pooled(a, b, lab, T, coef)
    dk = ra["dk"] + rb["dk"]
    want_a, want_b = ra["dq"] + dk[n:], rb["dq"] + dk[:n]
    got_a, got_b = ref["da_loc"] + ref["da_all_sum"], ref["db_loc"] + ref["db_all_sum"]
    scale = max(float(torch.maximum(want_a.abs().max(), want_b.abs().max())), 1.0)
    worst = max(float((got_a - want_a).abs().max()), float((got_b - want_b).abs().max())) / scale
    dT = abs(sum(ref["dT"]) - (ra["dT"] + rb["dT"])) / max(abs(ra["dT"] + rb["dT"]), 1.0)
    return worst, dT


def ratios(got, ref, bnd):
    """largest |error| / bound per output over all shards (``got`` laid out as ``ref``; outputs it lacks are skipped).  Every
    element takes part; an error of exactly 0 counts 0 whatever the bound (the counts, and the matched sums of columns without a
    match, have the bound 0)."""
    out = {}
    for name in OUTPUTS:
        if name not in got:
            continue
        worst = 0.0
        gs, rs, bs = (got[name], ref[name], bnd[name]) if isinstance(ref[name], list) else ([got[name]], [ref[name]], [bnd[name]])
        for g, r, b in zip(gs, rs, bs):
            if name == "dT":
                worst = max(worst, abs(float(g) - r) / b)
            else:
                err = (g.double() - r).abs()
                worst = max(worst, float(torch.where(err == 0, torch.zeros_like(err), err / b).max()))
        out[name] = worst
    return out


def signal(ref, bnd):
    """largest |value| / bound per output: how many bounds the reference itself is worth"""
    nothing = {name: [v * 0 for v in ref[name]] if isinstance(ref[name], list) else ref[name] * 0 for name in bnd}
    return ratios(nothing, ref, bnd)


# ---- the design's arithmetic on the CPU ----
MUTATIONS = ("self_positive", "partner_twice", "y_counts_dropped", "z_local", "wy_minus_rnc")


def emulate(a, b, lab, shards, T, coef, mutation=None, upstream=1.0):
    """The kernels' arithmetic on the CPU: float32 scores, exponentials, sums, counts and matched sums of the three blocks, the
    excluded key 0 in the stored E, in the row sum and in the matches; row statistics = X's + Y's, col_stats = X's columns with Z's
    rows added on the shard's own range, their float32 sum over the shards; E rounded to bf16 once, the weights a second time, the
    partner's weight from the float32 ediag; float32 products, two of them added in float32 where they share an output.  Output
    laid out as ``reference`` (without the _sum entries).  mutation:
      "self_positive"     the anchor itself stays a positive by label in Y and Z (counts, sums and weights)
      "partner_twice"     the partner is not excluded from the matches by label in X: a labeled row counts it twice
      "y_counts_dropped"  na = 1 + nX: block Y's counts never reach the row statistics
      "z_local"           block Z's statistics are added at the local index i instead of off + i
      "wy_minus_rnc"      a matched weight of block Y subtracts 1 / na_i + 1 / nb_j, as block X's does"""
    assert mutation is None or mutation in MUTATIONS
    f32 = torch.float32
    inv = torch.tensor(1.0, dtype=f32) / torch.tensor(T, dtype=f32)
    log2e = torch.tensor(1.4426950408889634, dtype=f32)
    scale2 = inv * log2e
    af, bf = a.float(), b.float()
    n = a.shape[0]
    ml_all = label_block(lab)
    labeled = lab >= 0
    state, cols = [], []
    for lo, hi in shards:
        rows = hi - lo
        ii, pos = torch.arange(rows), torch.arange(lo, hi)
        ml = ml_all[lo:hi]
        st = dict(ml=ml)
        for name, x, y in (("X", af, bf), ("Y", af, af), ("Z", bf, bf)):
            S = x[lo:hi] @ y.T
            E = torch.exp2(S * scale2 - scale2)
            m = ml.clone()
            if name != "X":
                E[ii, pos] = 0.0
                if mutation == "self_positive":
                    m[ii, pos] = labeled[pos]
            elif mutation == "partner_twice":
                m[ii, pos] = labeled[pos]
            mf = m.float()
            st["E" + name], st["m" + name] = E, m
            st["l" + name], st["n" + name], st["s" + name] = E.sum(1), mf.sum(1), (mf * S).sum(1)
            if name == "X":
                st["c"], st["nc"], st["sc"] = E.sum(0), mf.sum(0), (mf * S).sum(0)
        st["Da"] = st["lX"] + st["lY"]
        st["ka"] = st["nX"] if mutation == "y_counts_dropped" else st["nX"] + st["nY"]
        st["sa"] = st["sX"] + st["sY"]
        col = [st["c"].clone(), st["nc"].clone(), st["sc"].clone()]
        own = slice(0, rows) if mutation == "z_local" else slice(lo, hi)
        for q, z in zip(col, (st["lZ"], st["nZ"], st["sZ"])):
            q[own] = q[own] + z
        cols.append(col)
        state.append(st)
    tot = [c.clone() for c in cols[0]]
    for col in cols[1:]:
        tot = [t + c for t, c in zip(tot, col)]
    Db, kb, sb = tot
    ct = torch.tensor(coef, dtype=f32) * inv * torch.tensor(upstream, dtype=f32)
    one = torch.tensor(1.0, dtype=f32)
    v, rnc = 1.0 / Db, 1.0 / (one + kb)
    out = dict(loss_rows=torch.empty(n), colsum=[c[0] for c in cols], colcnt=[c[1] for c in cols], colsx=[c[2] for c in cols],
               da_loc=torch.empty(a.shape, dtype=f32), db_loc=torch.empty(a.shape, dtype=f32), da_all=[], db_all=[], dT=[])
    for (lo, hi), st in zip(shards, state):
        rows = hi - lo
        ii, pos = torch.arange(rows), torch.arange(lo, hi)
        dot = (af[lo:hi] * bf[pos]).sum(1)
        ediag = torch.exp2((dot - 1.0) * inv * log2e)
        u, rn = 1.0 / st["Da"], 1.0 / (one + st["ka"])
        mean_r = (dot + st["sa"]) * rn
        mean_c = (dot + sb[pos]) * rnc[pos]
        out["loss_rows"][lo:hi] = (torch.log(st["Da"]) + inv - mean_r * inv) + (torch.log(Db[pos]) + inv - mean_c * inv)
        uz, rnz = v[pos], rnc[pos]
        prod = st["EX"].to(torch.bfloat16).float() * (u[:, None] + v[None, :])
        WX = torch.where(st["mX"], prod - (rn[:, None] + rnc[None, :]), prod)
        WX[ii, pos] = ediag * (u + v[pos]) - (rn + rnc[pos])
        WX = (ct * WX).to(torch.bfloat16).float()
        prod = st["EY"].to(torch.bfloat16).float() * u[:, None]
        sub = rn[:, None] + rnc[None, :] if mutation == "wy_minus_rnc" else rn[:, None].expand(rows, n)
        WY = (ct * torch.where(st["mY"], prod - sub, prod)).to(torch.bfloat16).float()
        prod = st["EZ"].to(torch.bfloat16).float() * uz[:, None]
        WZ = (ct * torch.where(st["mZ"], prod - rnz[:, None], prod)).to(torch.bfloat16).float()
        dX, dY, dZ = WX @ bf, WY @ af, WZ @ bf
        out["da_loc"][lo:hi] = dX + dY
        out["db_loc"][lo:hi] = dZ
        out["da_all"].append(WY.T @ af[lo:hi])
        out["db_all"].append(WX.T @ af[lo:hi] + WZ.T @ bf[lo:hi])
        out["dT"].append(-float(((af[lo:hi] * dX).sum() + (af[lo:hi] * dY).sum() + (bf[lo:hi] * dZ).sum()) * inv))
    return out
