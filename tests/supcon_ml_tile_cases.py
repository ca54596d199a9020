"""Set plan, float64 reference, derived bounds and a CPU emulation shared by tests/test_supcon_ml_tile_cpu.py and
tests/test_supcon_ml_tile_gpu.py: the tile-GEMM form of the symmetric multi-label contrastive loss (the EPI_SETS_OV / EPI_SETS_JAC
epilogues, sup_sums_kernel, sup_finalize_kernel and set_weights_kernel of aecf_nce_gemm.hip behind aecf_supcon_ml_sym_pass1 /
_loss / _grads).  Rows, twins, shards and geometry are those of tests/nce_tile_cases.py, cases S1 to S4, imported, not copied; the
word arithmetic (mask, weights, unpack) is that of tests/supcon_ml_cases.py; this module adds the class sets of the tile cases.
Nothing here touches a GPU; every function works on the device of the tensors it is given.

One block, both directions (a [n, d] against b [n, d], the rows dealt over shards = emulated ranks, sets sr of the rows and sc of
the columns as int64 words; S = a b^T, x = S / T, ct = coef / T):
    w_ij = 1 if j == i, else [A_i & B_j != 0] ("overlap") or |A_i & B_j| / |A_i | B_j| ("jaccard", 0 for an empty union)
    Wr_i = sum_j w_ij     Wc_j = sum_i w_ij
    loss_i = [lse_row_i - (sum_j w_ij x_ij) / Wr_i] + [lse_col_i - (sum_i' w_i'i x_i'i) / Wc_i]
    G = P_row + P_col - w (1 / Wr_i + 1 / Wc_j),   da = ct G b,   db = ct G^T a (a shard's share: its rows of G),   dT = -(1/T) sum a . da
    col_stats of a shard = [ sum_i E_ij | sum_{i != j} w_ij | sum_{i != j} w_ij S_ij ],   E = exp((S - 1) / T)

The set plan (``plan``), deterministic per case; {..} are classes:
  * row i carries {i % 7, 7 + i % 5}, and {40 + i % 3} too when i is even; rows with i % 4 == 3 are empty.  About a third of all
    pairs carry a weight: the positives are dense, as in the timing run, and the Jaccard weights among them are 1/5 .. 1;
  * the first row r' of every twin pair (r', r) of the geometry carries its partner row's set without that set's lowest class, plus
    class 62 (an empty row r first gets {r % 7, 7 + r % 5, 40 + r % 3}): weight 1 under "overlap" and 1/3 or 1/2 under "jaccard"
    on every tile boundary the geometry names, and across the shards;
  * the heavy set {25, 44, 63} on every 9th row from row 5 that is no twin -- where that is more than 60 rows, on 60 of them, evenly
    spaced from the first to the last: spread over all tiles and shards;
  * every 11th of the remaining rows carries {33 + i % 4, 63}: it meets the heavy set in class 63 alone, the sign bit of the word
    and a class >= 32 only (weight 1/4);
  * six further rows, the "low-word twins", carry {25, 50 + i % 5}: against the heavy set their low words are equal (weight 1/4;
    the popcounts of the low words alone would say 1).
  sr = sc = the plan.  Case "S3m" is S3 with sr[2] = {20, 45}, which no column holds, while sc[2] keeps its own: the partner
  still counts, by index, and row 2 has no other positive (only the C ABI can express it).

Bounds.  Elementwise, derived from the roundings of the design, never from results, no further factor; they extend the derivation
in tests/supcon_tile_cases.py (h = 2^-24, EPS_P = 2^-8, s_err, xm, eps_e, eps_l, eps_cs, eps_c, eps_w, M as there and in
tests/nce_tile_cases.py).  q = 1 under "jaccard" and 0 under "overlap": a Jaccard weight is ONE correctly rounded float32 quotient
of two exact integers (relative error h, the u of supcon_ml_cases), an overlap weight is 0 or 1.  The summation order is the one
the header comment of aecf_nce_gemm.hip states: an element of a ROW passes through 16 (the lane's elements of the row) + 2 (lane
groups) + 2 (the block's 4 column waves) + ceil(n_tiles / 4) + 2 (sup_sums_kernel) additions, an element of a COLUMN through 8 + 4
+ 1 + ceil(m_tiles / 4) + 2, and shards - 1 more in the all-reduce:
      dr = 22 + ceil(n_tiles / 4),   dcs = 15 + ceil(m_tiles / 4),   dc = max over shards of dcs + shards - 1
  the sums of w (the partner excluded): of zeros and ones exact below 2^24 in any order (overlap: bound 0); of Jaccard weights the
      h of every quotient and the depth of the sum:
          |d rw_i| <= q (dr + 1) h sum_j wl_ij          |d cw_j| <= q (dcs + 1) h sum_i wl_ij      (wl: w without the partner)
  the sums of w S: an accumulator is within 4 s_err of the exact score; every term carries the h of its quotient (q) and the h of
      the product w * S (the kernel fuses the product into its addition; the bound keeps it), then the depth:
          |d rx_i| <= 4 s_err sum_j wl_ij + (dr + q + 1) h sum_j wl_ij |S_ij|      (columns: dcs, the summed statistics: dc)
  1 / W: W = 1 + rw, one addition (h, and none where the sum is an exact integer), the quotient within an ulp (2 h).  The depth of
      the fixed order stands where the streaming form of supcon_ml_cases has its n: relative error
          eW = (2 + q (dr + 2)) h   for a row,     eWc = (2 + q (dc + 2)) h   for a column
  mean_i = (dot_i + rx_i) * (1 / Wr_i): the partner's own float32 dot (4 s_err), one addition (h), 1 / Wr (eW), one product (h).
      With A_i = (sum_j w_ij |S_ij|) / Wr_i (4 s_err (1 + sum wl) / Wr = 4 s_err):
          |d mean_i| <= 4 s_err + ((dr + q + 1) h + 2 h + eW) A_i     -- and 4 s_err alone where row i has no weight by label
          (rx = 0, 1 / Wr = 1 and mean = dot exactly); the same for a column with dc, eWc and Ac_j
  loss_i: InfoNCE's bound with the means in the partner's place,
          |d loss_i| <= eps_l + eps_c + 8 s_err / T + [k_i > 0] ((dr + q + 3) h + eW) A_i / T + [kc_i > 0] ((dc + q + 3) h + eWc) Ac_i / T
                        + 4 h xm + 12 h M                                          (k: the number of weights by label that are not 0)
  W_ij with w = 0: bf16(ct (bf16(E32_ij) (u_i + v_j))) -- the bound it has in nce_tile_cases.
  W_ij with a weight (Q = P_row + P_col, Mn = w (1 / Wr_i + 1 / Wc_j), G = Q - Mn): bf16(ct fma(-w, rn_i + rnc_j, bf16(E32) (u + v))).
      On Mn: the two quotients with their own errors, their sum (h), the weight (q h):
          dMn_ij = w_ij (eW / Wr_i + eWc / Wc_j) + (1 + q) h Mn_ij
      ONE rounding of the fused subtraction (h) and ct's roundings (8 h) on the difference, one bf16 rounding around it:
          |d W_ij| <= ct (EPS_P |G_ij| + (1 + EPS_P) (((1 + EPS_P) (1 + eps_w) - 1) Q_ij + dMn_ij + 9 h |G_ij|)) + f
  W_ii, the partner (w = 1, exact): bf16(ct fma(ediag_i, u_i + v_i, -(rn_i + rnc_i))):
          |d W_ii| <= ct (EPS_P |G_ii| + (1 + EPS_P) (eps_w Q_ii + [k_i + kc_i > 0] dMn_ii + 8 h |G_ii|)) + f
      (no weight by label in row and column i: rn + rnc = 2 exactly, the bound of nce_tile_cases).
  da, db, dT, the column sums of E: the formulas of nce_tile_cases over these |d W| and this G.
A bf16 gradient adds 2^-8 |value|; an upstream scalar multiplies ct.  With one-hot sets q = 0 and these are the bounds of
supcon_tile_cases (whose 5 h Mn covers the 2 h + 2 h + h here): the two forms sum in orders of the same depth."""
import functools
import math

import torch

from tests import nce_tile_cases as N
from tests import supcon_ml_cases as ML
from tests.nce_tile_cases import EPS_P, FLUSH, H, MIN_T, TEMPS, used_temperature  # noqa: F401  (for the tests)
from tests.supcon_tile_cases import OUTPUTS, base, ratios, score_error, signal, workspace_bytes_py  # noqa: F401

WEIGHTINGS = ML.WEIGHTINGS
HEAVY = ML.HEAVY
S3M_SET = ML.C9_SET
CASE_IDS = list(N.SMALL_SYMMETRIC)               # S1 .. S4
ALL_IDS = CASE_IDS + ["S3m"]
# the broken rules of ``weights`` and of ``emulate``
RULES = ("and32", "pop_lo", "partner_by_sets", "partner_twice", "row_lost", "col_lost", "row_weight_sum", "union_inter")


def plan(n, twins):
    """class lists [n] of the plan above, with the heavy rows, the rows that meet them in class 63 alone and the low-word twins"""
    sets = [ML.local_set(i) for i in range(n)]
    for rp, r in twins:
        if not sets[r]:
            sets[r] = [r % 7, 7 + r % 5, 40 + r % 3]
        sets[rp] = sorted(sets[r])[1:] + [62]
    taken = {x for pair in twins for x in pair}
    heavy = [i for i in range(5, n) if i not in taken][::9]
    if len(heavy) > 60:
        heavy = [heavy[(t * (len(heavy) - 1)) // 59] for t in range(60)]
    for i in heavy:
        sets[i] = list(HEAVY)
    rest = [i for i in range(n) if i not in taken and i not in set(heavy)]
    sign = rest[::11]
    for i in sign:
        sets[i] = [33 + i % 4, 63]
    rest = [i for i in rest if i not in set(sign)]
    low = rest[3::13][:6]
    for i in low:
        sets[i] = [25, 50 + i % 5]
    return sets, heavy, sign, low


@functools.lru_cache(maxsize=None)
def make_case(cid):
    """the rows, shards and twins of nce_tile_cases plus sr [n], sc [n] (CPU, int64 words)"""
    c = dict(N.make_symmetric(base(cid)))
    n = c["a"].shape[0]
    sets, heavy, sign, low = plan(n, c["twins"])
    sc = torch.tensor([ML.mask(s) for s in sets], dtype=torch.int64)
    sr = sc.clone()
    if cid == "S3m":
        sr[2] = ML.mask(S3M_SET)
    c.update(sr=sr, sc=sc, heavy=heavy, sign=sign, low=low)
    return c


def weights(sr, sc, weighting, rule=None, single=False):
    """The weight matrix [n, n] of one block (off = 0, the partner on the diagonal): ML.weights, whose rules and32, pop_lo and
    partner_by_sets serve as they are, plus
      union_inter   union and intersection swapped: [A | B != 0] (overlap), |A | B| / |A & B| with 0 for an empty intersection (jaccard)"""
    if rule != "union_inter":
        return ML.weights(sr, sc, 0, weighting, rule=rule if rule in ML.RULES else None, single=single)
    inter, union, _, _ = ML.counts(sr, sc)
    if weighting == "overlap":
        w = (union > 0).double()
    else:
        den = torch.where(inter > 0, inter, torch.ones_like(inter))
        w = torch.where(inter > 0, (union.float() / den.float()).double() if single else union / den, torch.zeros_like(inter))
    i = torch.arange(sr.shape[0], device=sr.device)
    w[i, i] = 1.0
    return w.float() if single else w


# ---- float64 reference and the bounds of the module docstring ----
def reference(a, b, sr, sc, weighting, shards, T, coef, s_err, keep=False):
    """float64 on the device of a and b (n x n, off = 0).  Returns (ref, bnd) laid out as supcon_tile_cases.reference: loss_rows, da
    whole; db, dT and the three column statistics (colsum, colcnt = the sums of w, colsx) as lists, one entry per shard; db_sum."""
    a64, b64 = a.double(), b.double()
    n, d = a64.shape
    dev = a.device
    q = 1.0 if weighting == "jaccard" else 0.0
    ct = coef / T
    i = torch.arange(n, device=dev)
    S = a64 @ b64.T
    aS = S.abs()
    xm = float(torch.maximum(aS, (S - 1.0).abs()).max()) / T
    x = S / T
    E = torch.exp((S - 1.0) / T)
    Wf = weights(sr.to(dev), sc.to(dev), weighting)               # the partner 1
    Wl = Wf.clone()
    Wl[i, i] = 0.0                                               # the weights by label, the partner excluded
    k_row, k_col = (Wl != 0).sum(1), (Wl != 0).sum(0)
    W_row, W_col = Wf.sum(1), Wf.sum(0)
    lse_row, lse_col = torch.logsumexp(x, dim=1), torch.logsumexp(x, dim=0)
    loss = lse_row - (Wf * x).sum(1) / W_row + lse_col - (Wf * x).sum(0) / W_col
    P_row, P_col = torch.exp(x - lse_row[:, None]), torch.exp(x - lse_col[None, :])
    del x
    Q = P_row + P_col
    Mn = Wf * (1.0 / W_row[:, None] + 1.0 / W_col[None, :])
    G = Q - Mn
    aa, ab = a64.abs(), b64.abs()
    da = ct * (G @ b64)
    A_row, A_col = (Wf * aS).sum(1) / W_row, (Wf * aS).sum(0) / W_col

    geoms = [N.geometry(hi - lo, n, d) for lo, hi in shards]
    eps_e = 4.0 * s_err / T + 6.0 * H * xm + 2.0 * H
    dc = max(15 + -(-g["m_tiles"] // 4) for g in geoms) + len(shards) - 1
    eps_c = eps_e + dc * H
    eWc = (2.0 + q * (dc + 2)) * H
    M = xm + 1.0 / T + math.log(n)
    flush = FLUSH * (1.0 + ct)
    ref = dict(loss_rows=loss, da=da, db=[], dT=[], colsum=[], colcnt=[], colsx=[])
    bnd = dict(loss_rows=torch.empty_like(loss), da=torch.empty_like(da), db=[], dT=[], colsum=[], colcnt=[], colsx=[])
    for (lo, hi), g in zip(shards, geoms):
        dr, dcs = 22 + -(-g["n_tiles"] // 4), 15 + -(-g["m_tiles"] // 4)
        eW = (2.0 + q * (dr + 2)) * H
        eps_l = eps_e + (12 + -(-g["n_tiles"] // 4)) * H
        eps_cs = eps_e + (15 + -(-g["m_tiles"] // 4)) * H
        eps_w = eps_e + max(eps_l, eps_c) + 10.0 * H
        sl = slice(lo, hi)
        bnd["loss_rows"][sl] = (eps_l + eps_c + 8.0 * s_err / T + (k_row[sl] > 0) * ((dr + q + 3) * H + eW) * A_row[sl] / T
                                + (k_col[sl] > 0) * ((dc + q + 3) * H + eWc) * A_col[sl] / T + 4.0 * H * xm + 12.0 * H * M)
        Gs, Qs, Mns, Ws = G[sl], Q[sl], Mn[sl], Wf[sl]
        ii = torch.arange(hi - lo, device=dev)
        dMn = Ws * (eW / W_row[sl, None] + eWc / W_col[None, :]) + (1.0 + q) * H * Mns
        first = ((1.0 + EPS_P) ** 2 * (1.0 + eps_w) - 1.0) * Qs
        BW = ct * first + flush                                  # w = 0: the bound of nce_tile_cases (G = Q there)
        weighted = ct * (EPS_P * Gs.abs() + (1.0 + EPS_P) * (((1.0 + EPS_P) * (1.0 + eps_w) - 1.0) * Qs + dMn
                                                             + 9.0 * H * Gs.abs())) + flush
        BW = torch.where(Ws > 0, weighted, BW)
        gd, any_k = Gs[ii, lo + ii].abs(), ((k_row[sl] + k_col[sl]) > 0).double()
        BW[ii, lo + ii] = ct * (EPS_P * gd + (1.0 + EPS_P) * (eps_w * Qs[ii, lo + ii] + any_k * dMn[ii, lo + ii]
                                                              + 8.0 * H * gd)) + flush
        del first, weighted, dMn
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
        Wls = Wl[sl]
        ref["colcnt"].append(Wls.sum(0))
        bnd["colcnt"].append(q * (dcs + 1) * H * Wls.sum(0))
        ref["colsx"].append((Wls * S[sl]).sum(0))
        bnd["colsx"].append(4.0 * s_err * Wls.sum(0) + (dcs + q + 1) * H * (Wls * aS[sl]).sum(0))
    ref["db_sum"], bnd["db_sum"] = sum(ref["db"]), sum(bnd["db"])
    if keep:
        ref.update(G=G, Wf=Wf)
    return ref, bnd


def two_directions(a, b, sr, sc, weighting, T, coef):
    """the same loss as the sum of two tests/supcon_ml_cases.reference directions (one shard): a against b with the weight matrix,
    b against a with its transpose"""
    w = weights(sr, sc, weighting)
    ab, ba = ML.reference(a, b, w, T, coef), ML.reference(b, a, w.T.contiguous(), T, coef)
    return dict(loss_rows=ab["loss_rows"] + ba["loss_rows"], da=ab["dq"] + ba["dk"], db=ab["dk"] + ba["dq"], dT=ab["dT"] + ba["dT"])


def stream_bounds(a, b, sr, sc, weighting, T, coef, ex):
    """the bounds of the two streaming directions of ``two_directions`` added up (tests/supcon_ml_cases.bounds; ex = its eps_x):
    loss_rows, da, db, dT"""
    w = weights(sr, sc, weighting)
    rab, rba = ML.reference(a, b, w, T, coef), ML.reference(b, a, w.T.contiguous(), T, coef)
    bab, bba = ML.bounds(rab, a, b, T, coef, ex), ML.bounds(rba, b, a, T, coef, ex)
    return dict(loss_rows=bab["loss_rows"] + bba["loss_rows"], da=bab["dq"] + bba["dk"], db=bab["dk"] + bba["dq"],
                dT=bab["dT"] + bba["dT"])


# ---- the design's arithmetic on the CPU ----
def emulate(a, b, sr, sc, weighting, shards, T, coef, mutation=None, state=None, upstream=1.0):
    """The kernels' arithmetic on the CPU: float32 scores, exponentials, weights (one float32 quotient), sums of w and of w S and
    quotients, E rounded to bf16 once, the weights of the gradient a second time, the partner's from the float32 ediag.  Output
    laid out as ``reference`` (no db_sum).  mutation, a tuple (rule, ...):
      ("and32",) ("pop_lo",) ("union_inter",)  the weights of that broken rule of ``weights``
      ("partner_by_sets",)   the partner weighted by its sets like any element, everywhere (statistics, means and gradient weights)
      ("partner_twice",)     W = 2 + sum and the partner's dot added twice, rows and columns
      ("row_lost", i, j)     the weighted positive (i, j) is missing from the row statistics (sum of w and of w S) only
      ("col_lost", i, j)     ... from the column statistics only
      ("row_weight_sum",)    the column term of a weighted element (not the partner's) takes 1 / Wr_i for 1 / Wc_j"""
    st = state or N.emulate_pass1(a, b, shards, T)
    inv = st["inv"]
    f32 = torch.float32
    af, bf = a.float(), b.float()
    n = a.shape[0]
    kind = mutation[0] if mutation else None
    wf = weights(sr, sc, weighting, rule=kind if kind in ("and32", "pop_lo", "union_inter", "partner_by_sets") else None, single=True)
    idx = torch.arange(n)
    pw_all = wf[idx, idx].clone()                                # the partner's weight: 1 but under partner_by_sets
    wl_all = wf.clone()
    wl_all[idx, idx] = 0.0
    per = []
    for (lo, hi), s in zip(shards, st["shards"]):
        S32 = af[lo:hi] @ bf.T
        wl = wl_all[lo:hi]
        wr, wc = wl, wl
        if kind == "row_lost" and lo <= mutation[1] < hi:
            wr = wr.clone(); wr[mutation[1] - lo, mutation[2]] = 0.0
        if kind == "col_lost" and lo <= mutation[1] < hi:
            wc = wc.clone(); wc[mutation[1] - lo, mutation[2]] = 0.0
        per.append(dict(S=S32, wl=wl, rw=wr.sum(1), rx=(wr * S32).sum(1), cw=wc.sum(0), cx=(wc * S32).sum(0)))
    c_tot, cw_tot, cx_tot = st["shards"][0]["c"], per[0]["cw"], per[0]["cx"]
    for s, q in zip(st["shards"][1:], per[1:]):
        c_tot, cw_tot, cx_tot = c_tot + s["c"], cw_tot + q["cw"], cx_tot + q["cx"]
    ct = torch.tensor(coef, dtype=f32) * inv * torch.tensor(upstream, dtype=f32)
    twice = torch.tensor(2.0 if kind == "partner_twice" else 1.0, dtype=f32)
    log2e = torch.tensor(1.4426950408889634, dtype=f32)
    rnc = 1.0 / (twice * pw_all + cw_tot)
    v = 1.0 / c_tot
    out = dict(loss_rows=torch.empty(n), colsum=[s["c"] for s in st["shards"]], colcnt=[q["cw"] for q in per],
               colsx=[q["cx"] for q in per], da=torch.empty(a.shape, dtype=f32), db=[], dT=[])
    for (lo, hi), s, q in zip(shards, st["shards"], per):
        rows = hi - lo
        i = torch.arange(rows)
        pos = lo + i
        pw = twice * pw_all[pos]
        dot = (af[lo:hi] * bf[pos]).sum(1)
        ediag = torch.exp2((dot - 1.0) * inv * log2e)
        rn = 1.0 / (pw + q["rw"])
        mean_r = (pw * dot + q["rx"]) * rn
        mean_c = (pw * dot + cx_tot[pos]) * rnc[pos]
        out["loss_rows"][lo:hi] = (torch.log(s["l"]) + inv - mean_r * inv) + (torch.log(c_tot[pos]) + inv - mean_c * inv)
        u = 1.0 / s["l"]
        Eb = s["E"].to(torch.bfloat16).float()
        prod = Eb * (u[:, None] + v[None, :])
        col_term = rn[:, None].expand(rows, n) if kind == "row_weight_sum" else rnc[None, :]
        W = prod - q["wl"] * (rn[:, None] + col_term)
        W[i, pos] = ediag * (u + v[pos]) - pw_all[pos] * (rn + rnc[pos])
        W = (ct * W).to(torch.bfloat16).float()
        da = W @ bf
        out["da"][lo:hi] = da
        out["db"].append(W.T @ af[lo:hi])
        out["dT"].append(-float((af[lo:hi] * da).sum() * inv))
    return out


def one_hot_labels(n):
    """int64 labels [n] with classes < 64 for the one-hot comparison with the single-label tile form: class i % 61, every 4th row
    unlabeled (-1)"""
    i = torch.arange(n, dtype=torch.int64)
    return torch.where(i % 4 == 3, torch.full_like(i, -1), i % 61)
