"""Cases, float64 reference, derived bounds and a CPU emulation shared by tests/test_supcon_ml_pool_tile_cpu.py and
tests/test_supcon_ml_pool_tile_gpu.py: the tile-GEMM form of the pooled multi-label contrastive loss (aecf_supcon_ml_pool_sym_pass1 /
_loss / _grads: the EPI_SETS_* and EPI_SETS_*_SELF logits epilogues, sup_sums_kernel, sup_pool_combine_kernel, sup_finalize_kernel,
the two set_weights_kernel variants and the gradient products of aecf_nce_gemm.hip).  Rows, shards, twins and geometry are those of
tests/nce_tile_cases.py, cases S1 - S4; the set plan, the word arithmetic and "S3m" those of tests/supcon_ml_tile_cases.py; the pool
arrangement (keys [b | a], partner and excluded columns) and the float64 formulas those of tests/supcon_pool_cases.py, whose
``reference`` takes a float weight matrix where it took a match matrix (it divides by the row sums of whatever it is given) -- all
imported, not copied.  "S3e" is S3 with every set empty.  Nothing here touches a GPU; every function works on the device of its
tensors.

The problem.  n rows of two views a, b (unit bf16 rows), row sets sr [n] and column sets sc [n] as int64 words (bit c = class c; sr =
sc but in S3m), dealt over shards (emulated ranks); shard s owns rows lo .. hi.  With w(A, B) the overlap or Jaccard weight of
supcon_ml_tile_cases, Wl_ij = w(sr_i, sc_j) off the diagonal and 0 on it, Wf = Wl with 1 on the diagonal, the three blocks weigh
  X = a b^T: Wf (the partner 1 by index)        Y = a a^T: Wl        Z = b b^T: Wl        (the anchor's own key 0 by index)
and the 2 n rows are one pool, every row an anchor, itself left out:
  anchors of view a:  keys [b | a], weights [Wf | Wl],    excluded at column n + i        (supcon_pool_cases, off = 0, self_off = n)
  anchors of view b:  keys [b | a], weights [Wl | Wf^T],  excluded at column i            (off = n, self_off = 0)
  Wa_i = sum of row i of [Wf | Wl],  Wb_g = sum of row g of [Wl | Wf^T]
  loss_i = [lse_a_i - (sum_k w_k x_k) / Wa_i] + [lse_b_i - (sum_k w_k x_k) / Wb_i],   x = score / T
With Ga = Pa - Mna, Gb = Pb - Mnb [n, 2 n] (P the softmax, 0 on the excluded key; Mn = weight / W) the blocks carry
  G_X = Ga[:, :n] + Gb[:, n:]^T      Q_X = Pa[:, :n] + Pb[:, n:]^T      Mn_X = Wf (1 / Wa_i + 1 / Wb_j)
  G_Y = Ga[:, n:]                    Q_Y = Pa[:, n:]                    Mn_Y = Wl / Wa_i            (all 0 on the diagonal)
  G_Z = Gb[:, :n]                    Q_Z = Pb[:, :n]                    Mn_Z = Wl / Wb_i            (all 0 on the diagonal)
and a shard's outputs are those of tests/supcon_pool_tile_cases.py over these G (loss_rows, da_loc, db_loc, the shares da_all,
db_all, dT), plus the three column statistics it hands to the all-reduce:
  colsum = sum_{i in s} E_X[i, :]           + the row sums of E_Z[s] on columns lo .. hi
  colw   = sum_{i in s} Wl[i, :]            + the row sums of Wl[s] on columns lo .. hi
  colwx  = sum_{i in s} (Wl S_X)[i, :]      + the row sums of (Wl S_Z)[s] on columns lo .. hi
The shares add up to the pooled gradients and the excluded key never carries weight (``pooled_check``, ``composition``).

Bounds.  Elementwise, derived from the roundings of the design, never from results, no further factor: the composition of the
derivations in tests/supcon_pool_tile_cases.py (P) and tests/supcon_ml_tile_cases.py (M), whose symbols stand (h = 2^-24, EPS_P,
s_err, xm, eps_e, eps_l, eps_cs, eps_Da = eps_l + h, eps_Db, M with ln(2 n), f; q = 1 under "jaccard", 0 under "overlap").
  depths.  The SELF epilogues sum a row's weights in the order of EPI_SETS_* (ct-major over the lane's 16 elements, the lane
      groups, the four column waves, sup_sums_kernel), so M's row depth holds for X, Y and Z alike:
          dr = 22 + ceil(n_tiles / 4),   dcs = 15 + ceil(m_tiles / 4),   dc = max over shards of max(dcs, dr) + 1 + shards - 1   (P's dc)
  the sums of w of one block: M's -- q (dr + 1) h sum wl for a row, q (dcs + 1) h sum wl for a column; overlap sums are integers
      below 2^24, exact in any order: bound 0.
  the sums of w S of one block: M's -- 4 s_err sum wl + (dr + q + 1) h sum wl |S| for a row, dcs for a column.
  ONE more float32 addition on each combined statistic (P):
      colw, colwx on a rank's own range = fl(column of X + row of Z): the two bounds plus [q for colw] h (|column| + |row| + the two
          bounds); elsewhere the column bound alone.  colsum as in P (max(eps_cs, eps_l) + h on the own range).
      ka = fl(rwX + rwY) and the sum of the shards' colw: one and (1 + shards - 1) more additions.
  1 / W.  Wa = 1 + ka: the depth of a block's sum and its quotients (dr + 1), the combine (1), the addition of 1 (1), each q h, and
      the quotient 1 / Wa within an ulp (2 h):   eWa = (2 + q (dr + 3)) h;   Wb likewise with dc, which holds the combine and the
      all-reduce already:   eWb = (2 + q (dc + 2)) h   (M's eWc with P's dc).
  means.  mean_a = (dot + sa) (1 / Wa) with sa = fl(sX + sY): M's row bound with one more addition,
          |d mean_a_i| <= 4 s_err + ((dr + q + 2) h + 2 h + eWa) Aa_i,   Aa_i = (sum over X and Y of w |S|) / Wa_i
      and 4 s_err alone where anchor a_i has no weight by label; mean_b with dc, eWb and Ab_g (M's column bound with P's dc).
  loss_i = nce_row_term(Da) + nce_col_term(Db):
      |d loss_i| <= eps_Da + eps_Db + 8 s_err / T + [ka_i > 0] ((dr + q + 4) h + eWa) Aa_i / T + [kb_g > 0] ((dc + q + 3) h + eWb) Ab_g / T
                    + 4 h xm + 12 h M                                       (k: the number of weights by label that are not 0)
  W_X: M's three weight bounds (w = 0 / a weight / the partner) with Q_X, Mn_X, G_X, eps_w = eps_e + max(eps_Da, eps_Db) + 10 h and
          dMn_ij = w_ij (eWa / Wa_i + eWb / Wb_j) + (1 + q) h Mn_ij.
  W_Y, W_Z: the same w = 0 and weighted bounds at v = 0 and 1 / Wc = 0 (u + 0 and rn + 0 are exact; the counts of roundings stay
      upper bounds):  dMn = w eWa / Wa_i + (1 + q) h Mn_Y,  resp.  w eWb / Wb_i + (1 + q) h Mn_Z.  The excluded key is bf16(ct 0) = 0
      exactly and Q, Mn, G are 0 there: only the flush term remains.
  da_loc, db_loc, da_all, db_all, dT: P's formulas (two-product outputs with 2 (Cp + 32) / 2 (Rp + 32) terms, dT over three
      products) over these |d W| and these G.
With all sets empty every Mn term is the partner's alone and the bounds are those of tests/ntxent_tile_cases.py; with one-hot sets
q = 0 and they are P's (whose 5 h Mn covers the 2 h + 2 h + h here)."""
import functools
import math

import torch

from tests import nce_tile_cases as N
from tests import ntxent_tile_cases as X
from tests import supcon_ml_tile_cases as M
from tests import supcon_pool_cases as P
from tests.nce_stream_cases import EPS_P, FLUSH, used_temperature  # noqa: F401  (used_temperature: for the tests)
from tests.supcon_pool_tile_cases import workspace_bytes_py  # noqa: F401  (the layout is sup_pool_carve's, shared)

H = N.H
TEMPS = N.TEMPS
MIN_T = N.MIN_T
WEIGHTINGS = M.WEIGHTINGS
TILE_IDS = ("S1", "S2", "S3", "S4")
CASE_IDS = TILE_IDS + ("S3m",)
ALL_IDS = CASE_IDS + ("S3e",)
GRADS = X.GRADS
STATS = ("colsum", "colw", "colwx")
OUTPUTS = STATS + ("loss_rows",) + GRADS + ("dT",)
# the broken rules of ``emulate``
RULES = ("anchor_kept", "anchor_by_sets", "partner_by_sets", "partner_twice", "y_weights_lost", "z_at_local_index",
         "wy_subtracts_col", "union_inter")


def base(cid):
    return "S3" if cid in ("S3m", "S3e") else cid


@functools.lru_cache(maxsize=None)
def make_case(cid):
    """supcon_ml_tile_cases.make_case (a, b [n, d] bf16 unit rows on the CPU, shards, coef = 0.5 / n, twins, sr, sc [n] int64 words);
    S3e: S3's rows with every set empty"""
    assert cid in ALL_IDS
    if cid != "S3e":
        return M.make_case(cid)
    c = dict(M.make_case("S3"))
    c.update(sr=torch.zeros_like(c["sr"]), sc=torch.zeros_like(c["sc"]))
    return c


def score_error(cid):
    return X.score_error(base(cid))


def block_weights(sr, sc, weighting, rule=None, single=False):
    """(Wf, Wl) [n, n]: the weights of block X (the partner 1 on the diagonal, unless ``rule`` says otherwise) and of blocks Y and Z
    (the diagonal 0); ``rule``: a broken rule of supcon_ml_tile_cases.weights"""
    Wf = M.weights(sr, sc, weighting, rule=rule, single=single)
    Wl = Wf.clone()
    i = torch.arange(sr.shape[0], device=sr.device)
    Wl[i, i] = 0.0
    return Wf, Wl


def pooled(a, b, sr, sc, weighting, T, coef):
    """supcon_pool_cases.reference over both anchor halves of the whole problem, keys [b | a], with weight matrices where it takes
    match matrices: (ref of view a's anchors, ref of view b's anchors, their weight matrices [n, 2 n])"""
    n = a.shape[0]
    dev = a.device
    pool = torch.cat([b, a])
    Wf, Wl = block_weights(sr.to(dev), sc.to(dev), weighting)
    wa, wb = torch.cat([Wf, Wl], 1), torch.cat([Wl, Wf.T], 1)
    ra = P.reference(a, pool, wa, P.excluded(n, 2 * n, n, dev), T, coef)
    rb = P.reference(b, pool, wb, P.excluded(n, 2 * n, 0, dev), T, coef)
    return ra, rb, wa, wb


def composition(cid, weighting):
    """what the plan composes to on a case: (anchors with a weight by label, the most weights by label of one anchor over both views,
    the excluded key carries weight somewhere, the partner weighs 1 everywhere)"""
    c = make_case(cid)
    n = c["a"].shape[0]
    Wf, Wl = block_weights(c["sr"], c["sc"], weighting)
    wa, wb = torch.cat([Wf, Wl], 1), torch.cat([Wl, Wf.T], 1)
    i = torch.arange(n)
    k = torch.cat([(wa != 0).sum(1) - 1, (wb != 0).sum(1) - 1])
    excluded_weighs = bool((wa[i, n + i] != 0).any() or (wb[i, i] != 0).any())
    partner_one = bool((wa[i, i] == 1).all() and (wb[i, n + i] == 1).all())
    return int((k > 0).sum()), int(k.max()), excluded_weighs, partner_one


def reference(a, b, sr, sc, weighting, shards, T, coef, s_err):
    """float64 on the device of a and b [n, d].  Returns (ref, bnd): loss_rows, da_loc, db_loc [n ...] whole; colsum, colw, colwx,
    da_all, db_all, dT lists, one entry per shard (the shard's share); da_all_sum / db_all_sum the shares added up, with the summed
    bounds."""
    a64, b64 = a.double(), b.double()
    n, d = a64.shape
    dev = a.device
    q = 1.0 if weighting == "jaccard" else 0.0
    ct = coef / T
    ra, rb, wa, wb = pooled(a, b, sr, sc, weighting, T, coef)
    Pa, Pb, Mna, Mnb = ra["P"], rb["P"], ra["Mn"], rb["Mn"]
    Wf, Wl = wa[:, :n], wa[:, n:]
    idx = torch.arange(n, device=dev)
    QX, MnX = Pa[:, :n] + Pb[:, n:].T, Mna[:, :n] + Mnb[:, n:].T
    QY, MnY = Pa[:, n:], Mna[:, n:]
    QZ, MnZ = Pb[:, :n], Mnb[:, :n]
    GX, GY, GZ = QX - MnX, QY - MnY, QZ - MnZ
    loss = ra["loss_rows"] + rb["loss_rows"]
    xm, S = 0.0, {}
    for x, y, name in ((a64, b64, "X"), (a64, a64, "Y"), (b64, b64, "Z")):
        S[name] = x @ y.T
        xm = max(xm, float(torch.maximum(S[name].abs(), (S[name] - 1.0).abs()).max()) / T)
    EX = torch.exp((S["X"] - 1.0) / T)
    EZ = torch.exp((S["Z"] - 1.0) / T)
    EZ[idx, idx] = 0.0
    aSX, aSY, aSZ = S["X"].abs(), S["Y"].abs(), S["Z"].abs()
    Wa, Wb = wa.sum(1), wb.sum(1)
    ka, kb = (wa != 0).sum(1) - 1, (wb != 0).sum(1) - 1          # the weights by label of anchor a_i / b_g that are not 0
    Aa = (wa * torch.cat([aSX, aSY], 1)).sum(1) / Wa
    Ab = (wb * torch.cat([aSZ, aSX.T], 1)).sum(1) / Wb
    aa, ab = a64.abs(), b64.abs()
    geoms = [N.geometry(hi - lo, n, d) for lo, hi in shards]
    eps_e = 4.0 * s_err / T + 6.0 * H * xm + 2.0 * H
    deep = max(max(15 + -(-g["m_tiles"] // 4), 12 + -(-g["n_tiles"] // 4)) for g in geoms)
    eps_Db = eps_e + (deep + 1 + len(shards) - 1) * H
    dc = max(max(15 + -(-g["m_tiles"] // 4), 22 + -(-g["n_tiles"] // 4)) for g in geoms) + 1 + len(shards) - 1
    eWb = (2.0 + q * (dc + 2)) * H
    Mbig = xm + 1.0 / T + math.log(2 * n)
    flush = FLUSH * (1.0 + ct)
    ref = dict(loss_rows=loss, da_loc=torch.empty_like(a64), db_loc=torch.empty_like(a64), da_all=[], db_all=[], dT=[], colsum=[],
               colw=[], colwx=[])
    bnd = dict(loss_rows=torch.empty_like(loss), da_loc=torch.empty_like(a64), db_loc=torch.empty_like(a64), da_all=[], db_all=[],
               dT=[], colsum=[], colw=[], colwx=[])

    def weight_bound(Q, Mn, G, dMn, eps_w):
        plain = ct * ((1.0 + EPS_P) ** 2 * (1.0 + eps_w) - 1.0) * Q + flush
        weighted = ct * (EPS_P * G.abs() + (1.0 + EPS_P) * (((1.0 + EPS_P) * (1.0 + eps_w) - 1.0) * Q + dMn + 9.0 * H * G.abs())) + flush
        return torch.where(Mn > 0, weighted, plain)

    for (lo, hi), g in zip(shards, geoms):
        rows = hi - lo
        sl = slice(lo, hi)
        dr, dcs = 22 + -(-g["n_tiles"] // 4), 15 + -(-g["m_tiles"] // 4)
        eWa = (2.0 + q * (dr + 3)) * H
        eps_l = eps_e + (12 + -(-g["n_tiles"] // 4)) * H
        eps_cs = eps_e + (15 + -(-g["m_tiles"] // 4)) * H
        eps_Da = eps_l + H
        eps_w = eps_e + max(eps_Da, eps_Db) + 10.0 * H
        bnd["loss_rows"][sl] = (eps_Da + eps_Db + 8.0 * s_err / T + (ka[sl] > 0) * ((dr + q + 4) * H + eWa) * Aa[sl] / T
                                + (kb[sl] > 0) * ((dc + q + 3) * H + eWb) * Ab[sl] / T + 4.0 * H * xm + 12.0 * H * Mbig)
        ii, pos = torch.arange(rows, device=dev), idx[sl]
        dMnX = Wf[sl] * (eWa / Wa[sl, None] + eWb / Wb[None, :]) + (1.0 + q) * H * MnX[sl]
        dMnY = Wl[sl] * (eWa / Wa[sl, None]) + (1.0 + q) * H * MnY[sl]
        dMnZ = Wl[sl] * (eWb / Wb[sl, None]) + (1.0 + q) * H * MnZ[sl]
        BX = weight_bound(QX[sl], MnX[sl], GX[sl], dMnX, eps_w)
        gd, any_k = GX[sl][ii, pos].abs(), ((ka[sl] + kb[sl]) > 0).double()
        BX[ii, pos] = ct * (EPS_P * gd + (1.0 + EPS_P) * (eps_w * QX[sl][ii, pos] + any_k * dMnX[ii, pos] + 8.0 * H * gd)) + flush
        BY = weight_bound(QY[sl], MnY[sl], GY[sl], dMnY, eps_w)
        BZ = weight_bound(QZ[sl], MnZ[sl], GZ[sl], dMnZ, eps_w)
        del dMnX, dMnY, dMnZ
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
        Wls = Wl[sl]
        cw, rw = Wls.sum(0), Wls.sum(1)
        b_cw, b_rw = q * (dcs + 1) * H * cw, q * (dr + 1) * H * rw
        w_tot, b_w = cw.clone(), b_cw.clone()
        w_tot[sl] += rw
        b_w[sl] = b_cw[sl] + b_rw + q * H * (cw[sl] + rw + b_cw[sl] + b_rw)
        ref["colw"].append(w_tot)
        bnd["colw"].append(b_w)
        sxc, sxz = (Wls * S["X"][sl]).sum(0), (Wls * S["Z"][sl]).sum(1)
        axc, axz = (Wls * aSX[sl]).sum(0), (Wls * aSZ[sl]).sum(1)
        b_c = 4.0 * s_err * cw + (dcs + q + 1) * H * axc
        b_z = 4.0 * s_err * rw + (dr + q + 1) * H * axz
        sx, b_sx = sxc.clone(), b_c.clone()
        sx[sl] += sxz
        b_sx[sl] = b_c[sl] + b_z + H * (axc[sl] + axz + b_c[sl] + b_z)
        ref["colwx"].append(sx)
        bnd["colwx"].append(b_sx)
    for name in ("da_all", "db_all"):
        ref[name + "_sum"], bnd[name + "_sum"] = sum(ref[name]), sum(bnd[name])
    return ref, bnd


def pooled_check(a, b, sr, sc, weighting, shards, T, coef):
    """largest |difference| between this module's shares, added up, and the pooled gradients of supcon_pool_cases.reference (dq of
    each half on its own rows, dk on the pool [b | a]), relative to the largest gradient or to 1: float64 rounding only"""
    n = a.shape[0]
    ref, _ = reference(a, b, sr, sc, weighting, shards, T, coef, 0.0)
    ra, rb, _, _ = pooled(a, b, sr, sc, weighting, T, coef)
    dk = ra["dk"] + rb["dk"]
    want_a, want_b = ra["dq"] + dk[n:], rb["dq"] + dk[:n]
    got_a, got_b = ref["da_loc"] + ref["da_all_sum"], ref["db_loc"] + ref["db_all_sum"]
    scale = max(float(torch.maximum(want_a.abs().max(), want_b.abs().max())), 1.0)
    worst = max(float((got_a - want_a).abs().max()), float((got_b - want_b).abs().max())) / scale
    dT = abs(sum(ref["dT"]) - (ra["dT"] + rb["dT"])) / max(abs(ra["dT"] + rb["dT"]), 1.0)
    return worst, dT


def ratios(got, ref, bnd, outputs=OUTPUTS):
    """largest |error| / bound per output over all shards (``got`` laid out as ``ref``; outputs it lacks are skipped).  Every
    element takes part; an error of exactly 0 counts 0 whatever the bound (the overlap weight sums, and the weighted sums of
    columns without a weight, have the bound 0)."""
    out = {}
    for name in outputs:
        if name not in got:
            continue
        worst = 0.0
        gs, rs, bs = (got[name], ref[name], bnd[name]) if isinstance(ref[name], list) else ([got[name]], [ref[name]], [bnd[name]])
        for g, r, b in zip(gs, rs, bs):
            if name == "dT":
                e = abs(float(g) - r) / b
                worst = max(worst, e if e == e else float("inf"))
            else:
                err = (g.double() - r).abs()
                rel = torch.where(err == 0, torch.zeros_like(err), err / b)
                worst = max(worst, float(torch.nan_to_num(rel, nan=float("inf")).max()))     # an output that is no number is outside
        out[name] = worst
    return out


def signal(ref, bnd):
    """largest |value| / bound per output: how many bounds the reference itself is worth"""
    nothing = {name: [v * 0 for v in ref[name]] if isinstance(ref[name], list) else ref[name] * 0 for name in bnd}
    return ratios(nothing, ref, bnd)


# ---- the design's arithmetic on the CPU ----
def emulate(a, b, sr, sc, weighting, shards, T, coef, rule=None, upstream=1.0):
    """The kernels' arithmetic on the CPU, step for step in the kernels' order of operations: float32 scores, exponentials, weights
    (one float32 quotient), sums of E, of w and of w S of the three blocks, the excluded key 0 in the stored E, in the row sum and
    in the weights; row statistics = X's + Y's, col_stats = X's columns with Z's rows added on the shard's own range, their float32
    sum over the shards in rank order; E rounded to bf16 once, the weights a second time, the partner's weight from the float32
    ediag; float32 products, two of them added in float32 where they share an output.  (Inside one sum torch's float32 order stands
    for the kernels' fixed order: the bounds hold for every order of the documented depth.)  Output laid out as ``reference``
    (without the _sum entries).  rule:
      "anchor_kept"        the anchor's own key weighs 1 in block Y (its E stays 0)
      "anchor_by_sets"     the anchor's own key is weighted by its sets like any key, in Y and Z
      "partner_by_sets"    the partner is weighted by its sets like any key, everywhere (statistics, means and gradient weights)
      "partner_twice"      W = 2 + sum and the partner's dot added twice, for both anchors
      "y_weights_lost"     Wa = 1 + wX: block Y's weight sums never reach the row statistics
      "z_at_local_index"   block Z's statistics are added at the local index i instead of off + i
      "wy_subtracts_col"   a weighted element of block Y subtracts w (1 / Wa_i + 1 / Wb_j), as block X's does
      "union_inter"        union and intersection swapped in the weight"""
    assert rule is None or rule in RULES
    f32 = torch.float32
    inv = torch.tensor(1.0, dtype=f32) / torch.tensor(T, dtype=f32)
    log2e = torch.tensor(1.4426950408889634, dtype=f32)
    scale2 = inv * log2e
    af, bf = a.float(), b.float()
    n = a.shape[0]
    idx = torch.arange(n)
    wrule = rule if rule in ("partner_by_sets", "union_inter") else None
    Wf, Wl = block_weights(sr, sc, weighting, rule=wrule, single=True)
    by_sets = M.weights(sr, sc, weighting, rule="partner_by_sets", single=True)[idx, idx]
    pw_all = Wf[idx, idx].clone()                                # the partner's weight: 1 but under partner_by_sets
    twice = torch.tensor(2.0 if rule == "partner_twice" else 1.0, dtype=f32)
    state, cols = [], []
    for lo, hi in shards:
        rows = hi - lo
        ii, pos = torch.arange(rows), torch.arange(lo, hi)
        st = {}
        for name, x, y in (("X", af, bf), ("Y", af, af), ("Z", bf, bf)):
            S = x[lo:hi] @ y.T
            E = torch.exp2(S * scale2 - scale2)
            w = Wl[lo:hi].clone()
            if name != "X":
                E[ii, pos] = 0.0
                if rule == "anchor_by_sets":
                    w[ii, pos] = by_sets[pos]
                if rule == "anchor_kept" and name == "Y":
                    w[ii, pos] = 1.0
            st["E" + name], st["w" + name] = E, w
            st["l" + name], st["rw" + name], st["rx" + name] = E.sum(1), w.sum(1), (w * S).sum(1)
            if name == "X":
                st["c"], st["cw"], st["cx"] = E.sum(0), w.sum(0), (w * S).sum(0)
        st["Da"] = st["lX"] + st["lY"]
        st["ka"] = st["rwX"] if rule == "y_weights_lost" else st["rwX"] + st["rwY"]
        st["sa"] = st["rxX"] + st["rxY"]
        col = [st["c"].clone(), st["cw"].clone(), st["cx"].clone()]
        own = slice(0, rows) if rule == "z_at_local_index" else slice(lo, hi)
        for qv, z in zip(col, (st["lZ"], st["rwZ"], st["rxZ"])):
            qv[own] = qv[own] + z
        cols.append(col)
        state.append(st)
    tot = [c.clone() for c in cols[0]]
    for col in cols[1:]:
        tot = [t + c for t, c in zip(tot, col)]
    Db, kb, sb = tot
    ct = torch.tensor(coef, dtype=f32) * inv * torch.tensor(upstream, dtype=f32)
    v, rnc = 1.0 / Db, 1.0 / (twice * pw_all + kb)
    out = dict(loss_rows=torch.empty(n), colsum=[c[0] for c in cols], colw=[c[1] for c in cols], colwx=[c[2] for c in cols],
               da_loc=torch.empty(a.shape, dtype=f32), db_loc=torch.empty(a.shape, dtype=f32), da_all=[], db_all=[], dT=[])
    for (lo, hi), st in zip(shards, state):
        rows = hi - lo
        ii, pos = torch.arange(rows), torch.arange(lo, hi)
        pw = twice * pw_all[pos]
        dot = (af[lo:hi] * bf[pos]).sum(1)
        ediag = torch.exp2((dot - 1.0) * inv * log2e)
        u, rn = 1.0 / st["Da"], 1.0 / (pw + st["ka"])
        mean_r = (pw * dot + st["sa"]) * rn
        mean_c = (pw * dot + sb[pos]) * rnc[pos]
        out["loss_rows"][lo:hi] = (torch.log(st["Da"]) + inv - mean_r * inv) + (torch.log(Db[pos]) + inv - mean_c * inv)
        uz, rnz = v[pos], rnc[pos]
        WX = st["EX"].to(torch.bfloat16).float() * (u[:, None] + v[None, :]) - st["wX"] * (rn[:, None] + rnc[None, :])
        WX[ii, pos] = ediag * (u + v[pos]) - pw_all[pos] * (rn + rnc[pos])
        WX = (ct * WX).to(torch.bfloat16).float()
        sub = rn[:, None] + rnc[None, :] if rule == "wy_subtracts_col" else rn[:, None].expand(rows, n)
        WY = (ct * (st["EY"].to(torch.bfloat16).float() * u[:, None] - st["wY"] * sub)).to(torch.bfloat16).float()
        WZ = (ct * (st["EZ"].to(torch.bfloat16).float() * uz[:, None] - st["wZ"] * rnz[:, None])).to(torch.bfloat16).float()
        dX, dY, dZ = WX @ bf, WY @ af, WZ @ bf
        out["da_loc"][lo:hi] = dX + dY
        out["db_loc"][lo:hi] = dZ
        out["da_all"].append(WY.T @ af[lo:hi])
        out["db_all"].append(WX.T @ af[lo:hi] + WZ.T @ bf[lo:hi])
        out["dT"].append(-float(((af[lo:hi] * dX).sum() + (af[lo:hi] * dY).sum() + (bf[lo:hi] * dZ).sum()) * inv))
    return out
