"""Label plan, float64 reference, derived bounds and a CPU emulation shared by tests/test_supcon_tile_cpu.py and
tests/test_supcon_tile_gpu.py: the tile-GEMM form of the symmetric supervised contrastive loss (the EPI_SUP epilogue and the
sup_* kernels of aecf_nce_gemm.hip behind aecf_supcon_sym_pass1 / _loss / _grads).  Rows, twins, shards and geometry are those
of tests/nce_tile_cases.py, cases S1 to S4, imported, not copied; this module adds the labels.  Nothing here touches a GPU; every
function works on the device of the tensors it is given.

One block, both directions (a [n, d] against b [n, d], the rows dealt over shards = emulated ranks, labels lr of the rows and lc of
the columns; S = a b^T, x = S / T, ct = coef / T):
    m_ij = (j == i) or (lr_i >= 0 and lr_i == lc_j)         n_i = sum_j m_ij     nc_j = sum_i m_ij
    loss_i = [lse_row_i - (sum_j m_ij x_ij) / n_i] + [lse_col_i - (sum_i' m_i'i x_i'i) / nc_i]
    G = P_row + P_col - m (1 / n_i + 1 / nc_j),   da = ct G b,   db = ct G^T a (a shard's share: its rows of G),   dT = -(1/T) sum a . da
    col_stats of a shard = [ sum_i E_ij | #{i: label match, i != j} | sum over those of S_ij ],   E = exp((S - 1) / T)

The label plan (``plan``), deterministic per case:
  * row i carries class i // 3; rows with i % 4 == 3 are unlabeled, alternately -1 and -7 (two different negative labels, and two
    equal ones, must never match);
  * both rows of every twin pair (r', r) share a class, 100000 + r if row r was unlabeled: a positive by label on every boundary
    the geometry names, and across shards;
  * the large class 2^40 on every 9th row from row 5 that is no twin, 60 rows at most: one class spread over all tiles and shards;
  * distractor classes 2^40 + 2^32 (1 + i % 5) on every 11th remaining row: they differ from the large class only above bit 31.
  lr = lc = the plan.  Case "S3m" is S3 with lr[2] set to a distractor class while lc[2] keeps its own: the partner still counts,
  by index, and the counts of a row and of a column of one matched element differ (only the C ABI can express it).

Bounds.  Elementwise, derived from the roundings of the design, never from results, no further factor; they extend the derivation
in tests/nce_tile_cases.py (h = 2^-24, EPS_P = 2^-8, s_err, xm, eps_e, eps_l, eps_cs, eps_c, eps_w, M as there).  What is new:
  counts: sums of zeros and ones in float32, exact below 2^24 in any order: bound 0.
  rs_i = float32 sum of the raw accumulators of the label matches of row i (the partner excluded).  An accumulator is within
      4 s_err of the exact score; an element passes through 16 (the lane's elements of the row) + 2 (lane groups) + 2 (the
      block's 4 waves) + ceil(n_tiles / 4) + 2 (sup_sums_kernel) additions; a column's sum through 8 + 4 + 1 + ceil(m_tiles / 4) + 2,
      and shards - 1 more in the all-reduce:
          |d rs_i| <= 4 s_err k_i + dr h sum_j ml_ij |S_ij|,     dr = 22 + ceil(n_tiles / 4)          k = the number of label matches
          |d cs_j| <= 4 s_err kc_j + dcs h sum_i ml_ij |S_ij|,   dcs = 15 + ceil(m_tiles / 4)         (a shard's col_stats[2])
          the summed column statistics: dc = max over shards of dcs + shards - 1
  mean_i = (dot_i + rs_i) * (1 / n_i): the partner's own float32 dot (4 s_err), one addition (h), the quotient 1 / n within an ulp
      (2 h; n = 1 + count is exact), one product (h).  With A_i = (sum_j m_ij |S_ij|) / n_i:
          |d mean_i| <= 4 s_err + (dr + 4) h A_i             -- and NOTHING where row i has no label match: rs = 0, 1 / n = 1 and
          mean = dot exactly; the same for a column with dc and Ac_j = (sum_i m_ij |S_ij|) / nc_j
  loss_i = logf(l_i) + 1/T - mean_i / T + the same of column i: InfoNCE's bound with the mean in the partner's place,
          |d loss_i| <= eps_l + eps_c + 8 s_err / T + [k_i > 0] (dr + 4) h A_i / T + [kc_i > 0] (dc + 4) h Ac_i / T + 4 h xm + 12 h M
  W_ij without a match: bf16(ct (bf16(E32_ij) (u_i + v_j))) -- the bound it has in nce_tile_cases.
  W_ij with a match (Q = P_row + P_col, Mn = 1 / n_i + 1 / nc_j, G = Q - Mn): bf16(ct (bf16(E32) (u + v) - (rn_i + rnc_j))): the two
      quotients (2 h each) and their sum (h) stand on Mn, ONE more subtraction (h) and ct's roundings (8 h, as for the partner
      there) on the difference, and one bf16 rounding around it:
          |d W_ij| <= ct (EPS_P |G_ij| + (1 + EPS_P) (((1 + EPS_P) (1 + eps_w) - 1) Q_ij + 5 h Mn_ij + 9 h |G_ij|)) + f
  W_ii, the partner: bf16(ct (ediag_i (u_i + v_i) - (rn_i + rnc_i))):
          |d W_ii| <= ct (EPS_P |G_ii| + (1 + EPS_P) (eps_w Q_ii + [k_i + kc_i > 0] 5 h Mn_ii + 8 h |G_ii|)) + f
      (no label match in row and column i: rn + rnc = 2 exactly, the bound of nce_tile_cases).
  da, db, dT, the column sums of E: the formulas of nce_tile_cases over these |d W| and this G.
A bf16 gradient adds 2^-8 |value|; an upstream scalar multiplies ct."""
import functools
import math

import torch

from tests import nce_tile_cases as N
from tests.nce_tile_cases import EPS_P, FLUSH, H, MIN_T, TEMPS, used_temperature  # noqa: F401  (for the tests)

LARGE = 2 ** 40
CASE_IDS = list(N.SMALL_SYMMETRIC)               # S1 .. S4
ALL_IDS = CASE_IDS + ["S3m"]


def base(cid):
    return "S3" if cid == "S3m" else cid


def distractor(i):
    return LARGE + 2 ** 32 * (1 + i % 5)


def plan(n, twins):
    """int64 labels [n] of the plan above, with the rows that got the large class and the distractor classes"""
    lab = torch.empty(n, dtype=torch.int64)
    for i in range(n):
        lab[i] = (-1 if (i // 4) % 2 == 0 else -7) if i % 4 == 3 else i // 3
    for rp, r in twins:
        if int(lab[r]) < 0:
            lab[r] = 100000 + r
        lab[rp] = lab[r]
    taken = {x for pair in twins for x in pair}
    large = [i for i in range(5, n) if i not in taken][::9][:60]
    for i in large:
        lab[i] = LARGE
    rest = [i for i in range(n) if i not in taken and i not in set(large)]
    distract = rest[::11]
    for i in distract:
        lab[i] = distractor(i)
    return lab, large, distract


@functools.lru_cache(maxsize=None)
def make_case(cid):
    """the rows, shards and twins of nce_tile_cases plus lr [n], lc [n] (CPU, int64)"""
    c = dict(N.make_symmetric(base(cid)))
    n = c["a"].shape[0]
    lc, large, distract = plan(n, c["twins"])
    lr = lc.clone()
    if cid == "S3m":
        k = [i for i in distract if i != 2][0]
        lr[2] = lc[k]
    c.update(lr=lr, lc=lc, large=large, distract=distract)
    return c


def score_error(cid):
    return N.score_error(base(cid))


def label_matrix(lr, lc, compare32=False, unlabeled_class=False):
    """bool [rows, cols]: the same non-negative label -- no partner.  compare32 / unlabeled_class: what a 32-bit compare / a
    missing sign test would match (for the mutations)"""
    a, b = lr[:, None], lc[None, :]
    if compare32:
        a, b = a.to(torch.int32), b.to(torch.int32)
    m = a == b
    return m if unlabeled_class else m & (a >= 0)


def match_matrix(lr, lc, off=0):
    """bool [rows, cols]: the partner (column off + i) by index, or the same non-negative label"""
    m = label_matrix(lr, lc)
    i = torch.arange(lr.shape[0], device=lr.device)
    m[i, off + i] = True
    return m


def workspace_bytes_py(rows, cols, d):
    """sup_carve() + 256: E, the row and column partials of three quantities, the row statistics, 1/l, 1/n, 1/c, 1/nc, ediag, the da
    slabs -- each rounded up to 256 bytes"""
    g = N.geometry(rows, cols, d)
    Rp, Cp = g["Rp"], g["Cp"]
    parts = [Rp * Cp * 2, 3 * g["n_tiles"] * Rp * 4, 3 * g["m_tiles"] * Cp * 4, 3 * Rp * 4, Rp * 4, Rp * 4, Cp * 4, Cp * 4, Rp * 4,
             g["splits"] * rows * d * 4]
    return sum(N.up256(p) for p in parts) + 256


# ---- float64 reference and the bounds of the module docstring ----
def reference(a, b, lr, lc, shards, T, coef, s_err, keep=False):
    """float64 on the device of a and b (n x n, off = 0).  Returns (ref, bnd): loss_rows, da whole; db, dT and the three column
    statistics (colsum, colcnt, colsx) as lists, one entry per shard; db_sum = the shares added up, with the summed bounds."""
    a64, b64 = a.double(), b.double()
    n, d = a64.shape
    dev = a.device
    lr, lc = lr.to(dev), lc.to(dev)
    ct = coef / T
    i = torch.arange(n, device=dev)
    S = a64 @ b64.T
    aS = S.abs()
    xm = float(torch.maximum(aS, (S - 1.0).abs()).max()) / T
    x = S / T
    E = torch.exp((S - 1.0) / T)
    Ml = label_matrix(lr, lc)
    Ml[i, i] = False                                             # the matches by label, the partner excluded
    Mf = Ml.double()
    Mf[i, i] = 1.0
    k_row, k_col = Ml.sum(1), Ml.sum(0)
    n_row, n_col = Mf.sum(1), Mf.sum(0)
    lse_row, lse_col = torch.logsumexp(x, dim=1), torch.logsumexp(x, dim=0)
    loss = lse_row - (Mf * x).sum(1) / n_row + lse_col - (Mf * x).sum(0) / n_col
    P_row, P_col = torch.exp(x - lse_row[:, None]), torch.exp(x - lse_col[None, :])
    del x
    Q = P_row + P_col
    Mn = Mf * (1.0 / n_row[:, None] + 1.0 / n_col[None, :])
    G = Q - Mn
    aa, ab = a64.abs(), b64.abs()
    da = ct * (G @ b64)
    A_row, A_col = (Mf * aS).sum(1) / n_row, (Mf * aS).sum(0) / n_col

    geoms = [N.geometry(hi - lo, n, d) for lo, hi in shards]
    eps_e = 4.0 * s_err / T + 6.0 * H * xm + 2.0 * H
    eps_c = eps_e + (max(15 + -(-g["m_tiles"] // 4) for g in geoms) + len(shards) - 1) * H
    dc = max(15 + -(-g["m_tiles"] // 4) for g in geoms) + len(shards) - 1
    M = xm + 1.0 / T + math.log(n)
    flush = FLUSH * (1.0 + ct)
    ref = dict(loss_rows=loss, da=da, db=[], dT=[], colsum=[], colcnt=[], colsx=[])
    bnd = dict(loss_rows=torch.empty_like(loss), da=torch.empty_like(da), db=[], dT=[], colsum=[], colcnt=[], colsx=[])
    for (lo, hi), g in zip(shards, geoms):
        dr, dcs = 22 + -(-g["n_tiles"] // 4), 15 + -(-g["m_tiles"] // 4)
        eps_l = eps_e + (12 + -(-g["n_tiles"] // 4)) * H
        eps_cs = eps_e + (15 + -(-g["m_tiles"] // 4)) * H
        eps_w = eps_e + max(eps_l, eps_c) + 10.0 * H
        sl = slice(lo, hi)
        bnd["loss_rows"][sl] = (eps_l + eps_c + 8.0 * s_err / T + (k_row[sl] > 0) * (dr + 4) * H * A_row[sl] / T
                                + (k_col[sl] > 0) * (dc + 4) * H * A_col[sl] / T + 4.0 * H * xm + 12.0 * H * M)
        Gs, Qs, Mns, Ms = G[sl], Q[sl], Mn[sl], Mf[sl]
        ii = torch.arange(hi - lo, device=dev)
        first = ((1.0 + EPS_P) ** 2 * (1.0 + eps_w) - 1.0) * Qs
        BW = ct * first + flush                                  # no match: the bound of nce_tile_cases (G = Q there)
        matched = ct * (EPS_P * Gs.abs() + (1.0 + EPS_P) * (((1.0 + EPS_P) * (1.0 + eps_w) - 1.0) * Qs + 5.0 * H * Mns
                                                            + 9.0 * H * Gs.abs())) + flush
        BW = torch.where(Ms > 0, matched, BW)
        gd, any_k = Gs[ii, lo + ii].abs(), ((k_row[sl] + k_col[sl]) > 0).double()
        BW[ii, lo + ii] = ct * (EPS_P * gd + (1.0 + EPS_P) * (eps_w * Qs[ii, lo + ii] + any_k * 5.0 * H * Mns[ii, lo + ii]
                                                              + 8.0 * H * gd)) + flush
        del first, matched
        mag = ct * Gs.abs() + BW
        b_da = (BW + (g["Cp"] + 32) * H * mag) @ ab
        b_db = (BW + (g["Rp"] + 32) * H * mag).T @ aa[sl]
        del mag, BW
        bnd["da"][sl] = b_da
        ref["db"].append(ct * (Gs.T @ a64[sl]))
        bnd["db"].append(b_db)
        dT = -(1.0 / T) * float((a64[sl] * da[sl]).sum())
        depth = 145 + -(-(g["splits"] * g["m_tiles"] * g["d_tiles"]) // 256)
        ref["dT"].append(dT)
        bnd["dT"].append((float((aa[sl] * b_da).sum()) + depth * H * float((aa[sl] * (da[sl].abs() + b_da)).sum())) / T
                         + 3.0 * H * abs(dT))
        cs = E[sl].sum(0)
        ref["colsum"].append(cs)
        bnd["colsum"].append(eps_cs * cs)
        Mls = Ml[sl].double()
        ref["colcnt"].append(Mls.sum(0))
        bnd["colcnt"].append(torch.zeros(n, dtype=torch.float64, device=dev))
        ref["colsx"].append((Mls * S[sl]).sum(0))
        bnd["colsx"].append(4.0 * s_err * Mls.sum(0) + dcs * H * (Mls * aS[sl]).sum(0))
    ref["db_sum"], bnd["db_sum"] = sum(ref["db"]), sum(bnd["db"])
    if keep:
        ref.update(G=G, Mf=Mf)
    return ref, bnd


OUTPUTS = ("colsum", "colcnt", "colsx", "loss_rows", "da", "db", "db_sum", "dT")


def ratios(got, ref, bnd, bf16=False):
    """largest |error| / bound per output over all shards (``got`` laid out as ``ref``; outputs it lacks are skipped); an error of
    exactly 0 counts 0 whatever the bound (the counts, and the matched sums of columns without a match, have the bound 0).
    bf16: the gradients were rounded once more on the way out, 2^-8 |value| joins their bounds."""
    out = {}
    for name in OUTPUTS:
        if name not in got:
            continue
        worst = 0.0
        gs, rs, bs = (got[name], ref[name], bnd[name]) if isinstance(ref[name], list) else ([got[name]], [ref[name]], [bnd[name]])
        for g, r, b in zip(gs, rs, bs):
            if name == "dT":
                worst = max(worst, abs(float(g) - r) / b)
            elif r.numel():
                g = g.double()
                if bf16 and name in ("da", "db", "db_sum"):
                    b = b + 2.0 ** -8 * g.abs()
                err = (g - r).abs()
                q = torch.where(err == 0, torch.zeros_like(err), err / b)
                worst = max(worst, float(q.max()))
        out[name] = worst
    return out


def signal(ref, bnd):
    """largest |value| / bound per output: how many bounds the reference itself is worth"""
    nothing = {name: [v * 0 for v in ref[name]] if isinstance(ref[name], list) else ref[name] * 0 for name in bnd}
    return ratios(nothing, ref, bnd)


def two_directions(a, b, lr, lc, T, coef):
    """the same loss as the sum of two tests/supcon_cases.reference directions (one shard): a against b with the match matrix,
    b against a with its transpose"""
    from tests import supcon_cases as SC
    m = match_matrix(lr, lc)
    ab, ba = SC.reference(a, b, m, T, coef), SC.reference(b, a, m.T, T, coef)
    return dict(loss_rows=ab["loss_rows"] + ba["loss_rows"], da=ab["dq"] + ba["dk"], db=ab["dk"] + ba["dq"], dT=ab["dT"] + ba["dT"])


# ---- the design's arithmetic on the CPU ----
def emulate(a, b, lr, lc, shards, T, coef, mutation=None, state=None, upstream=1.0):
    """The kernels' arithmetic on the CPU: float32 scores, exponentials, sums, matched sums and quotients, E rounded to bf16 once,
    the weights a second time, the partner's weight from the float32 ediag.  Output laid out as ``reference`` (no db_sum).
    mutation:
      ("row_lost", i, j)  the label positive (i, j) is missing from the row statistics (count and sum) only
      ("col_lost", i, j)  ... from the column statistics only
      ("compare32",)      labels compared in their low 32 bits
      ("unlabeled",)      no sign test: equal negative labels match
      ("partner_twice",)  n = 2 + count and the partner's dot added twice, rows and columns
      ("row_count",)      the column term of a matched weight (not the partner's) takes 1 / n_i for 1 / nc_j"""
    st = state or N.emulate_pass1(a, b, shards, T)
    inv = st["inv"]
    f32 = torch.float32
    af, bf = a.float(), b.float()
    n = a.shape[0]
    kind = mutation[0] if mutation else None
    ml_all = label_matrix(lr, lc, compare32=kind == "compare32", unlabeled_class=kind == "unlabeled")
    idx = torch.arange(n)
    ml_all[idx, idx] = False
    per = []
    for (lo, hi), s in zip(shards, st["shards"]):
        S32 = af[lo:hi] @ bf.T
        ml = ml_all[lo:hi].clone()
        mr, mc = ml.float(), ml.float()
        if kind == "row_lost" and lo <= mutation[1] < hi:
            mr = mr.clone(); mr[mutation[1] - lo, mutation[2]] = 0.0
        if kind == "col_lost" and lo <= mutation[1] < hi:
            mc = mc.clone(); mc[mutation[1] - lo, mutation[2]] = 0.0
        per.append(dict(S=S32, ml=ml, rcnt=mr.sum(1), rsx=(mr * S32).sum(1), ccnt=mc.sum(0), csx=(mc * S32).sum(0)))
    c_tot, cc_tot, cx_tot = st["shards"][0]["c"], per[0]["ccnt"], per[0]["csx"]
    for s, q in zip(st["shards"][1:], per[1:]):
        c_tot, cc_tot, cx_tot = c_tot + s["c"], cc_tot + q["ccnt"], cx_tot + q["csx"]
    ct = torch.tensor(coef, dtype=f32) * inv * torch.tensor(upstream, dtype=f32)
    one = torch.tensor(2.0 if kind == "partner_twice" else 1.0, dtype=f32)
    log2e = torch.tensor(1.4426950408889634, dtype=f32)
    rnc = 1.0 / (one + cc_tot)
    v = 1.0 / c_tot
    out = dict(loss_rows=torch.empty(n), colsum=[s["c"] for s in st["shards"]], colcnt=[q["ccnt"] for q in per],
               colsx=[q["csx"] for q in per], da=torch.empty(a.shape, dtype=f32), db=[], dT=[])
    for (lo, hi), s, q in zip(shards, st["shards"], per):
        rows = hi - lo
        i = torch.arange(rows)
        pos = lo + i
        dot = (af[lo:hi] * bf[pos]).sum(1)
        ediag = torch.exp2((dot - 1.0) * inv * log2e)
        rn = 1.0 / (one + q["rcnt"])
        mean_r = (one * dot + q["rsx"]) * rn
        mean_c = (one * dot + cx_tot[pos]) * rnc[pos]
        out["loss_rows"][lo:hi] = (torch.log(s["l"]) + inv - mean_r * inv) + (torch.log(c_tot[pos]) + inv - mean_c * inv)
        u = 1.0 / s["l"]
        Eb = s["E"].to(torch.bfloat16).float()
        prod = Eb * (u[:, None] + v[None, :])
        col_term = rn[:, None].expand(rows, n) if kind == "row_count" else rnc[None, :]
        W = torch.where(q["ml"], prod - (rn[:, None] + col_term), prod)
        W[i, pos] = ediag * (u + v[pos]) - (rn + rnc[pos])
        W = (ct * W).to(torch.bfloat16).float()
        da = W @ bf
        out["da"][lo:hi] = da
        out["db"].append(W.T @ af[lo:hi])
        out["dT"].append(-float((af[lo:hi] * da).sum() * inv))
    return out
