"""Cases, float64 reference, derived bounds and a CPU emulation shared by tests/test_queue_supcon_cpu.py and
tests/test_queue_supcon_gpu.py: the supervised contrastive loss with a key queue on the tile GEMMs (aecf_supcon_queue_pass1 / _loss /
_grads: the EPI_SUP and EPI_SUP_Q logits epilogues, sup_sums_kernel, sup_pool_combine_kernel, sup_finalize_kernel, the three variants
of sup_weights_kernel and the gradient products of aecf_nce_gemm.hip) and the labelled ring behind it
(aecf_key_queue_push_labeled).  Rows, shards, twins, queue plans, queue rows and the host ring are those of
tests/queue_nce_cases.py (cases S1 - S4, plans Q0 - Q4), the batch labels the plan of tests/supcon_tile_cases.py, the geometry that of
tests/nce_tile_cases.py: imported, not copied.  This module adds the ring of stored labels.  Nothing here touches a GPU; every
function works on the device of the tensors it is given.

The problem.  n rows of two views a, b (unit bf16 rows) with labels y [n] shared by the views (negative: unlabeled), dealt over
shards (emulated ranks); two key rings Qa, Qb [q_cap, d] and ONE label ring Ql [q_cap] of which slots 0 .. V - 1 count.  With
S_X = a b^T, S_U = a Qb[:V]^T, S_W = b Qa[:V]^T, E = exp((S - 1) / T), ct = coef / T:
  ml_X[i, j] = (y_i == y_j >= 0, j != i)                 ml_Q[i, s] = (y_i == Ql[s] >= 0, s < V)         all 64 bits
  Da_i = sum_j E_X[i, j] + sum_s E_U[i, s]               Db_g = sum_i E_X[i, g] + sum_s E_W[g, s]
  ka_i = sum_j ml_X[i, j] + sum_s ml_Q[i, s]             kb_g = sum_i ml_X[i, g] + sum_s ml_Q[g, s]       na = 1 + ka, nb = 1 + kb
  sa_i = sum_j ml_X S_X + sum_s ml_Q S_U                 sb_g = sum_i ml_X[i, g] S_X[i, g] + sum_s ml_Q[g, s] S_W[g, s]
  loss_rows[i] = [log Da_i + 1/T - (S_X[i, i] + sa_i) / (na_i T)] + [log Db_i + 1/T - (S_X[i, i] + sb_i) / (nb_i T)]
  G_X = E_X / Da_i + E_X / Db_j - m_X (1 / na_i + 1 / nb_j)     (m_X = ml_X with the partner, by index)
  G_U = E_U / Da_i - ml_Q / na_i                         G_W = E_W / Db_g - ml_Q / nb_g
  da_loc[s] = ct (G_X[s] b + G_U[s] Qb[:V])     db_loc[s] = ct G_W[s] Qa[:V]     db_all share = ct G_X[s]^T a[s]
  dT share = -(1/T) (sum a[s] . da_loc[s] + sum b[s] . db_loc[s])
  col_stats of a shard [3][n] = the column sums over its rows of E_X | ml_X | ml_X S_X, plus the row sums of E_W | ml_Q | ml_Q S_W
  of its rows on columns lo .. hi         (colsum | colcnt | colsx: what ranks exchange, pass 1's output)
A slot at or above V is no key and no positive by its INDEX; a stored key is nobody's partner.  The rings take no gradient.

The label ring, deterministic per plan (``slot_label``, ``make_queue``).  Valid slot k carries, in rotation: the large class 2^40 on
every 7th slot; else by k mod 3 a class of the batch ((k // 3) mod the number of batch classes), a distractor class 2^40 + 2^32 (1 +
k mod 5) -- the batch's own distractor classes: they differ from the large class only above bit 31 -- or no label, alternately -1
and -7 (they must match no unlabeled row).  Slot V - 1 (V >= 2) keeps queue_nce_cases' bit-identical twin of b[r] / a[r] and gets a
class row r does NOT carry: a legitimate negative with the partner's score, not excluded by value, not counted by value.  Where V
>= 3 slot V - 2 (an unrelated row) gets row r's label.  Slots at or above V hold queue_nce_cases' garbage rows AND labels that live
rows carry (``live_label``: the large class on the even slots, a batch row's class on the odd ones).  Q4's labels ride through the
host ring (``ring_push``) with the keys, the twin's and its neighbour's in the LAST push: slots 89 and 88 of the wrapped ring.

Bounds: the two derivations this form joins, tests/queue_nce_cases.py (three blocks, Da, Db, the products, dT) and
tests/supcon_tile_cases.py (counts, matched sums, means, the matched-weight bound), with what the join changes.  h = 2^-24, EPS_P =
2^-8, s_err (the largest |S32 - S64| over the three products), xm, eps_e, eps_lX, eps_lQ, eps_Da = max(eps_lX, eps_lQ) + h, eps_cs,
eps_Db, eps_w = eps_e + max(eps_Da, eps_Db) + 10 h, M = xm + 1/T + ln(n + V) and the flush term exactly as in queue_nce_cases.
Every count is an upper bound read off the code; no bound carries a further factor and none was fitted to results.
  counts: sums of zeros and ones in float32; an anchor's count adds two blocks' counts, at most (n - 1) + q_cap, exact below 2^24 in
      any order (cols + q_cap <= 2^24 is the served bound): bound 0, for ka, kb and every shard's colcnt.
  matched sums of one block.  X's rows and columns: supcon_tile_cases' drX = 22 + ceil(n_tiles / 4), dcs = 15 + ceil(m_tiles / 4).
      U's and W's rows (EPI_SUP_Q runs EPI_SUP's row chain: 16 elements of the lane, 2 lane groups, 2 for the block's 4 waves, the
      queue's tiles and sup_sums_kernel): drQ = 22 + ceil(q_tiles / 4).  A skipped tile and a slot at or above V add exact zeros.
  sa_i = X's + U's, ONE float32 addition (sup_pool_combine_kernel): |d sa_i| <= 4 s_err ka_i + dra h (the matched |S| of row i),
      dra = max(drX, drQ) + 1.  A shard's colsx on its own range = X's column sum + W's row sum, ONE addition: depth max(dcs, drQ) +
      1 there, dcs elsewhere; the all-reduce adds shards - 1: dcb = max over shards of (max(dcs, drQ) + 1) + shards - 1.
  means: supcon_tile_cases' chain (the partner's own float32 dot, one addition, the quotient within an ulp, one product) with dra
      and dcb: |d mean_a_i| <= 4 s_err + (dra + 4) h A_i, A_i = (|S_ii| + the matched |S| of both blocks) / na_i, and nothing beyond
      the dot's 4 s_err where the anchor has no label match in either block (0 + 0 matched sum, 1 / 1: the mean is the dot).
  loss_rows: |d loss_i| <= eps_Da + eps_Db + 8 s_err / T + [ka_i > 0] (dra + 4) h A_i / T + [kb_i > 0] (dcb + 4) h Ab_i / T + 4 h xm
      + 12 h M.
  W_X: supcon_tile_cases' three weight bounds (no match, match, partner) with Q = E_X / Da + E_X / Db, Mn = m_X (1 / na + 1 / nb), this
      eps_w, and [ka_i + kb_i > 0] in the partner's (no match in either block: rn + rnc = 2 exactly).
  W_U, W_W: v = rnc = 0 (u + 0 and rn + 0 are exact, so the counts stay upper bounds).  No match: queue_nce_cases' off-diagonal
      bound, Q = E_U / Da (E_W / Db).  Match: supcon_tile_cases' matched bound with Mn = ml_Q / na (ml_Q / nb).  No partner element.
      A slot at or above V: bf16(ct (0 (u + 0))) = 0 exactly.
  da_loc, db_loc, db_all, dT, colsum: queue_nce_cases' formulas over these |d W| and |G| (G_U and G_W may be negative now).
Other output forms: a bf16 gradient is the float32 sum rounded once: 2^-8 |value| joins its bound.  An upstream scalar multiplies
ct: reference and bounds are taken at coef * upstream."""
import functools
import math

import torch

from tests import nce_tile_cases as N
from tests import queue_nce_cases as Q
from tests import supcon_tile_cases as S
from tests.nce_tile_cases import EPS_P, FLUSH, H, MIN_T, TEMPS, used_temperature  # noqa: F401  (for the tests)

CASE_IDS = Q.CASE_IDS
PLANS = Q.PLANS
PLAN_IDS = Q.PLAN_IDS
GRADS = Q.GRADS
OUTPUTS = ("colsum", "colcnt", "colsx", "loss_rows") + GRADS + ("dT",)
LARGE = S.LARGE
_unit = Q._unit


@functools.lru_cache(maxsize=None)
def make_case(cid):
    """queue_nce_cases.make_case (a, b, shards, coef, twins) plus y [n] int64: supcon_tile_cases' label plan of the same rows"""
    c = dict(Q.make_case(cid))
    c["y"] = S.make_case(cid)["lc"]
    return c


def batch_classes(n):
    return -(-n // 3)


def slot_label(k, n):
    """the label of the k-th stored key (k: the slot, or the push order for Q4)"""
    if k % 7 == 0:
        return LARGE
    if k % 3 == 0:
        return (k // 3) % batch_classes(n)
    if k % 3 == 1:
        return S.distractor(k)
    return -1 if (k // 3) % 2 == 0 else -7


def live_label(k, y):
    """what a slot at or above V holds: a label live rows carry, the large class included"""
    if k % 2 == 0:
        return LARGE
    v = int(y[k % y.shape[0]])
    return v if v >= 0 else (k // 3) % batch_classes(y.shape[0])


def foreign_class(cid):
    """a class of the batch that row r (queue_nce_cases.twin_row) does not carry"""
    y = make_case(cid)["y"]
    return 1 if int(y[Q.twin_row(cid)]) == 0 else 0


# ---- the labelled ring on the host ----
def ring_push(qa, qb, ql, state, src_a, src_b, src_l, mutation=None):
    """aecf_key_queue_push_labeled on the host, in place: the labels go where queue_nce_cases.ring_push puts the keys, from the
    cursor the push found; src_l None writes -1.  mutation "label_order": the labels are written from slot 0 in push order while
    the keys wrap; "stale": a push without labels leaves the label slots as they were."""
    q_cap, n = ql.shape[0], src_a.shape[0]
    cur = state[0]
    for i in range(max(0, n - q_cap), n):
        slot = i % q_cap if mutation == "label_order" else (cur + i) % q_cap
        if src_l is not None:
            ql[slot] = src_l[i]
        elif mutation != "stale":
            ql[slot] = -1
    Q.ring_push(qa, qb, state, src_a, src_b)


def push_labels(cid, last_unlabeled=False):
    """the labels of Q4's three pushes: ``slot_label`` in push order; the twin (the last row of the last push) gets the class row
    r does not carry, the row in front of it row r's label.  last_unlabeled: the last push comes without labels (None)."""
    c = make_case(cid)
    n = c["y"].shape[0]
    out, k = [], 0
    for m in Q.Q4_PUSHES:
        out.append(torch.tensor([slot_label(k + i, n) for i in range(m)], dtype=torch.int64))
        k += m
    out[-1][-1] = foreign_class(cid)
    out[-1][-2] = int(c["y"][Q.twin_row(cid)])
    if last_unlabeled:
        out[-1] = None
    return out


@functools.lru_cache(maxsize=None)
def make_queue(cid, pid, mutation=None, last_unlabeled=False):
    """(Qa, Qb [q_cap, d] bf16, Ql [q_cap] int64 on the CPU, V) of a plan; the keys are queue_nce_cases.make_queue's.  mutation
    ("label_order", "stale") and last_unlabeled: plan Q4 through the broken ring / with an unlabeled last push."""
    c = make_case(cid)
    y = c["y"]
    n = y.shape[0]
    qa, qb, V = Q.make_queue(cid, pid)
    q_cap = qa.shape[0]
    if pid == "Q4":
        ka, kb = torch.zeros_like(qa), torch.zeros_like(qb)
        ql = torch.full((q_cap,), -1, dtype=torch.int64)
        state = [0, 0]
        for (sa, sb), sl in zip(Q.push_sources(cid), push_labels(cid, last_unlabeled)):
            ring_push(ka, kb, ql, state, sa, sb, sl, mutation)
        assert torch.equal(ka, qa) and torch.equal(kb, qb) and state[1] == V
        return qa, qb, ql, V
    ql = torch.tensor([slot_label(k, n) if k < V else live_label(k, y) for k in range(q_cap)], dtype=torch.int64)
    if V >= 2:
        ql[V - 1] = foreign_class(cid)
    if V >= 3:
        ql[V - 2] = int(y[Q.twin_row(cid)])
    return qa, qb, ql, V


def workspace_bytes_py(rows, cols, q_cap, d):
    """sup_que_carve() + 256: E_X, E_U, E_W, the row partials of three quantities over the wider block, X's column partials, the
    three row statistics, 1/Da, 1/na, 1/Db, 1/nb, both at the partner, ediag, zeros, the dT partials, the slabs of two da products --
    each rounded up to 256 bytes"""
    g, q = N.geometry(rows, cols, d), N.geometry(rows, q_cap, d)
    Rp, Cp, Qp = g["Rp"], g["Cp"], q["Cp"]
    Zp = max(Cp, Qp)
    parts = [Rp * Cp * 2, Rp * Qp * 2, Rp * Qp * 2, 3 * (Zp // 256) * Rp * 4, 3 * g["m_tiles"] * Cp * 4, 3 * Rp * 4, 3 * Rp * 4,
             3 * Rp * 4, Rp * 4, Rp * 4, Cp * 4, Cp * 4, Rp * 4, Rp * 4, Rp * 4, Zp * 4, 3 * 32 * 16 * g["m_tiles"] * 4,
             (g["splits"] + q["splits"]) * rows * d * 4]
    return sum(N.up256(p) for p in parts) + 256


score_error = Q.score_error


def reference(a, b, y, qa, qb, ql, V, shards, T, coef, s_err):
    """float64 on the device of a and b [n, d] over the whole batch.  Returns (ref, bnd): loss_rows, da_loc, db_loc [n ...] whole;
    colsum, colcnt, colsx, db_all, dT lists, one entry per shard (the shard's share); db_all_sum the shares added up, with the
    summed bounds."""
    a64, b64 = a.double(), b.double()
    dev = a.device
    ka, kb = qa[:V].to(dev).double(), qb[:V].to(dev).double()       # the slots at or above V are no part of the definition
    y, lq = y.to(dev), ql[:V].to(dev)
    n, d = a64.shape
    q_cap = qa.shape[0]
    ct = coef / T
    idx = torch.arange(n, device=dev)
    SX, SU, SW = a64 @ b64.T, a64 @ kb.T, b64 @ ka.T
    xm = 0.0
    for Sm in (SX, SU, SW):
        if Sm.numel():
            xm = max(xm, float(torch.maximum(Sm.abs(), (Sm - 1.0).abs()).max()) / T)
    EX, EU, EW = torch.exp((SX - 1.0) / T), torch.exp((SU - 1.0) / T), torch.exp((SW - 1.0) / T)
    Da, Db = EX.sum(1) + EU.sum(1), EX.sum(0) + EW.sum(1)
    MlX = S.label_matrix(y, y)
    MlX[idx, idx] = False                                       # the matches by label, the partner excluded
    MlQ = S.label_matrix(y, lq)                                 # [n, V]: the same for the anchors of both views (shared labels)
    fX, fQ = MlX.double(), MlQ.double()
    MfX = fX.clone()
    MfX[idx, idx] = 1.0
    ka_cnt, kb_cnt = fX.sum(1) + fQ.sum(1), fX.sum(0) + fQ.sum(1)
    na, nb = 1.0 + ka_cnt, 1.0 + kb_cnt
    sii = SX[idx, idx]
    aX, aU, aW = SX.abs(), SU.abs(), SW.abs()
    sa, sb = (fX * SX).sum(1) + (fQ * SU).sum(1), (fX * SX).sum(0) + (fQ * SW).sum(1)
    loss = (torch.log(Da) + 1.0 / T - (sii + sa) / na / T) + (torch.log(Db) + 1.0 / T - (sii + sb) / nb / T)
    A_a = (sii.abs() + (fX * aX).sum(1) + (fQ * aU).sum(1)) / na
    A_b = (sii.abs() + (fX * aX).sum(0) + (fQ * aW).sum(1)) / nb
    QX = EX / Da[:, None] + EX / Db[None, :]
    MnX = MfX * (1.0 / na[:, None] + 1.0 / nb[None, :])
    GX = QX - MnX
    QU, QW = EU / Da[:, None], EW / Db[:, None]
    MnU, MnW = fQ / na[:, None], fQ / nb[:, None]
    GU, GW = QU - MnU, QW - MnW
    aa, ab, aka, akb = a64.abs(), b64.abs(), ka.abs(), kb.abs()
    geoms = [N.geometry(hi - lo, n, d) for lo, hi in shards]
    q_tiles = N.up256(q_cap) // 256
    Qp = N.up256(q_cap)
    eps_e = 4.0 * s_err / T + 6.0 * H * xm + 2.0 * H
    eps_lQ = eps_e + (12 + -(-q_tiles // 4)) * H
    eps_Db = eps_e + (max(max(15 + -(-g["m_tiles"] // 4), 12 + -(-q_tiles // 4)) for g in geoms) + 1 + len(shards) - 1) * H
    drQ = 22 + -(-q_tiles // 4)
    dcb = max(max(15 + -(-g["m_tiles"] // 4), drQ) + 1 for g in geoms) + len(shards) - 1
    M = xm + 1.0 / T + math.log(n + V)
    flush = FLUSH * (1.0 + ct)
    lists = ("db_all", "dT", "colsum", "colcnt", "colsx")
    ref = dict(loss_rows=loss, da_loc=torch.empty_like(a64), db_loc=torch.empty_like(a64), **{k: [] for k in lists})
    bnd = dict(loss_rows=torch.empty_like(loss), da_loc=torch.empty_like(a64), db_loc=torch.empty_like(a64), **{k: [] for k in lists})
    for (lo, hi), g in zip(shards, geoms):
        rows = hi - lo
        sl = slice(lo, hi)
        q_splits = N.da_splits(g["Rp"], Qp, d)
        drX, dcs = 22 + -(-g["n_tiles"] // 4), 15 + -(-g["m_tiles"] // 4)
        dra = max(drX, drQ) + 1
        eps_lX = eps_e + (12 + -(-g["n_tiles"] // 4)) * H
        eps_cs = eps_e + (15 + -(-g["m_tiles"] // 4)) * H
        eps_Da = max(eps_lX, eps_lQ) + H
        eps_w = eps_e + max(eps_Da, eps_Db) + 10.0 * H
        bnd["loss_rows"][sl] = (eps_Da + eps_Db + 8.0 * s_err / T + (ka_cnt[sl] > 0) * (dra + 4) * H * A_a[sl] / T
                                + (kb_cnt[sl] > 0) * (dcb + 4) * H * A_b[sl] / T + 4.0 * H * xm + 12.0 * H * M)
        ii, pos = torch.arange(rows, device=dev), idx[sl]

        def weight_bound(G, Qm, Mn, matched):
            plain = ct * ((1.0 + EPS_P) ** 2 * (1.0 + eps_w) - 1.0) * Qm + flush
            hit = ct * (EPS_P * G.abs() + (1.0 + EPS_P) * (((1.0 + EPS_P) * (1.0 + eps_w) - 1.0) * Qm + 5.0 * H * Mn
                                                           + 9.0 * H * G.abs())) + flush
            return torch.where(matched, hit, plain)

        BX = weight_bound(GX[sl], QX[sl], MnX[sl], MfX[sl] > 0)
        gd, any_k = GX[sl][ii, pos].abs(), ((ka_cnt[sl] + kb_cnt[sl]) > 0).double()
        BX[ii, pos] = ct * (EPS_P * gd + (1.0 + EPS_P) * (eps_w * QX[sl][ii, pos] + any_k * 5.0 * H * MnX[sl][ii, pos]
                                                          + 8.0 * H * gd)) + flush
        BU = weight_bound(GU[sl], QU[sl], MnU[sl], MlQ[sl])
        BW = weight_bound(GW[sl], QW[sl], MnW[sl], MlQ[sl])
        mX, mU, mW = ct * GX[sl].abs() + BX, ct * GU[sl].abs() + BU, ct * GW[sl].abs() + BW
        nC, nQ, nR = (g["Cp"] + 32) * H, (Qp + 32) * H, (g["Rp"] + 32) * H
        # single-product bounds (the float32 accumulators dT is taken from), then the outputs
        bX1, bU1, bW1 = (BX + nC * mX) @ ab, (BU + nQ * mU) @ akb, (BW + nQ * mW) @ aka
        vX, vU, vW = ct * (GX[sl] @ b64), ct * (GU[sl] @ kb), ct * (GW[sl] @ ka)
        ref["da_loc"][sl] = vX + vU
        bnd["da_loc"][sl] = (BX + (nC + nQ) * mX) @ ab + (BU + (nC + nQ) * mU) @ akb
        ref["db_loc"][sl] = vW
        bnd["db_loc"][sl] = bW1
        ref["db_all"].append(ct * (GX[sl].T @ a64[sl]))
        bnd["db_all"].append((BX + nR * mX).T @ aa[sl])
        dT = -(1.0 / T) * float((a64[sl] * (vX + vU)).sum() + (b64[sl] * vW).sum())
        depth = 145 + -(-((g["splits"] + 2 * q_splits) * g["m_tiles"] * g["d_tiles"]) // 256)
        B = float((aa[sl] * (bX1 + bU1)).sum() + (ab[sl] * bW1).sum())
        Vv = float((aa[sl] * (vX.abs() + vU.abs())).sum() + (ab[sl] * vW.abs()).sum())
        ref["dT"].append(dT)
        bnd["dT"].append((B + depth * H * (Vv + B)) / T + 3.0 * H * abs(dT))
        cs = EX[sl].sum(0)
        e_cs = torch.full_like(cs, eps_cs)
        cs[sl] += EW[sl].sum(1)
        e_cs[sl] = max(eps_cs, eps_lQ) + H
        ref["colsum"].append(cs)
        bnd["colsum"].append(e_cs * cs)
        cc = fX[sl].sum(0)
        cc[sl] += fQ[sl].sum(1)
        ref["colcnt"].append(cc)
        bnd["colcnt"].append(torch.zeros_like(cc))
        cx, kx, mx = (fX[sl] * SX[sl]).sum(0), fX[sl].sum(0), (fX[sl] * aX[sl]).sum(0)
        depth_x = torch.full_like(cx, float(dcs))
        cx[sl] += (fQ[sl] * SW[sl]).sum(1)
        kx[sl] += fQ[sl].sum(1)
        mx[sl] += (fQ[sl] * aW[sl]).sum(1)
        depth_x[sl] = max(dcs, drQ) + 1
        ref["colsx"].append(cx)
        bnd["colsx"].append(4.0 * s_err * kx + depth_x * H * mx)
    ref["db_all_sum"], bnd["db_all_sum"] = sum(ref["db_all"]), sum(bnd["db_all"])
    return ref, bnd


def autograd_check(a, b, y, qa, qb, ql, V, T, coef):
    """largest |difference| between ``reference`` (one shard) and float64 autograd of the definition written with explicit sets of
    positives, relative to the largest gradient or to 1: (loss and gradients, dT) -- float64 rounding only"""
    n = a.shape[0]
    x, z = a.double().requires_grad_(True), b.double().requires_grad_(True)
    t = torch.tensor(T, dtype=torch.float64, requires_grad=True)
    ka, kb, lq = qa[:V].double(), qb[:V].double(), ql[:V]
    i = torch.arange(n)
    pos = torch.cat([(y[:, None] == y[None, :]) & (y[:, None] >= 0), (y[:, None] == lq[None, :]) & (y[:, None] >= 0)], 1)
    pos[i, i] = True
    pf = pos.double()
    la = torch.cat([x @ z.T, x @ kb.T], 1) / t
    lb = torch.cat([z @ x.T, z @ ka.T], 1) / t
    loss = coef * sum((torch.logsumexp(l, 1) - (pf * l).sum(1) / pf.sum(1)).sum() for l in (la, lb))
    loss.backward()
    ref, _ = reference(a, b, y, qa, qb, ql, V, [(0, n)], T, coef, 0.0)
    scale = max(float(x.grad.abs().max()), float(z.grad.abs().max()), 1.0)
    worst = max(float((ref["da_loc"] - x.grad).abs().max()), float((ref["db_loc"] + ref["db_all_sum"] - z.grad).abs().max())) / scale
    loss = float(loss.detach())
    worst = max(worst, abs(coef * float(ref["loss_rows"].sum()) - loss) / max(abs(loss), 1.0))
    return worst, abs(ref["dT"][0] - float(t.grad)) / max(abs(float(t.grad)), 1.0)


def ratios(got, ref, bnd, bf16=False):
    """largest |error| / bound per output over all shards (``got`` laid out as ``ref``; outputs it lacks are skipped).  Every
    element takes part; an error of exactly 0 counts 0 whatever the bound (a bound of 0 -- the counts, an empty product, a matched
    sum without a match -- asks for the exact value), an error that is no number counts as infinite.  bf16: the gradients were
    rounded once more on the way out, 2^-8 |value| joins their bounds."""
    out = {}
    for name in OUTPUTS:
        if name not in got:
            continue
        worst = 0.0
        gs, rs, bs = (got[name], ref[name], bnd[name]) if isinstance(ref[name], list) else ([got[name]], [ref[name]], [bnd[name]])
        for g, r, b in zip(gs, rs, bs):
            if name == "dT":
                e = abs(float(g) - r) / b
                worst = max(worst, e if e == e else math.inf)
            elif r.numel():
                if bf16 and name in GRADS and name != "db_all_sum":
                    b = b + EPS_P * (r.abs() + b)
                elif bf16 and name == "db_all_sum":
                    b = b + EPS_P * sum(x.abs() + z for x, z in zip(ref["db_all"], bnd["db_all"]))
                err = (g.double() - r).abs()
                e = torch.nan_to_num(torch.where(err == 0.0, err, err / b), nan=math.inf, posinf=math.inf)
                worst = max(worst, float(e.max()))
        out[name] = worst
    return out


def signal(ref, bnd):
    """largest |value| / bound per output: how many bounds the reference itself is worth"""
    nothing = {name: [v * 0 for v in ref[name]] if isinstance(ref[name], list) else ref[name] * 0 for name in bnd}
    return ratios(nothing, ref, bnd)


# ---- the design's arithmetic on the CPU ----
# mutation -> the output whose bound it must leave
MUTATIONS = {"labels_ignored": "loss_rows", "one_direction": "colsx", "count_ignored": "loss_rows", "unlabeled": "loss_rows",
             "compare32": "loss_rows", "stats_local": "colsum", "twin_by_value": "loss_rows", "label_order": "loss_rows",
             "stale": "loss_rows"}


def emulate(a, b, y, qa, qb, ql, V, shards, T, coef, mutation=None, upstream=1.0):
    """The kernels' arithmetic on the CPU: float32 scores, exponentials, sums, counts, matched sums and quotients; the slots at or
    above V 0 in E, in the sums and in the matches BY INDEX; row statistics X's + U's, column statistics X's with W's row
    statistics added on the shard's own range, their float32 sum over the shards; E rounded to bf16 once, the weights a second
    time, the partner's weight from the float32 ediag; float32 products over ALL q_cap slots.  Laid out as ``reference`` (without
    db_all_sum).  mutation:
      "labels_ignored"  the stored labels are not read: the queue holds negatives only
      "one_direction"   the stored labels serve the anchors of view a only (W has no matches)
      "count_ignored"   a slot at or above V still matches by its label (its E is left out)
      "unlabeled"       no sign test against the ring: -1 matches -1
      "compare32"       stored labels compared in their low 32 bits
      "stats_local"     W's statistics are added at the local index i instead of off + i
      "twin_by_value"   a stored key whose float32 score equals the partner's counts as a positive
    ("label_order" and "stale" are mutations of the ring, ``ring_push``: the caller hands over the label ring it leaves.)"""
    assert mutation is None or mutation in MUTATIONS
    f32 = torch.float32
    inv = torch.tensor(1.0, dtype=f32) / torch.tensor(T, dtype=f32)
    log2e = torch.tensor(1.4426950408889634, dtype=f32)
    scale2 = inv * log2e
    af, bf = a.float(), b.float()
    kU, kW = qb.float(), qa.float()                         # U's keys, W's keys: every slot
    n, q_cap = a.shape[0], qa.shape[0]
    live = torch.arange(q_cap) < V
    idx = torch.arange(n)
    mlX_all = S.label_matrix(y, y)
    mlX_all[idx, idx] = False
    mlQ_all = S.label_matrix(y, ql, compare32=mutation == "compare32", unlabeled_class=mutation == "unlabeled")
    if mutation != "count_ignored":
        mlQ_all = mlQ_all & live[None, :]
    if mutation == "labels_ignored":
        mlQ_all = torch.zeros_like(mlQ_all)
    state = []
    for lo, hi in shards:
        rows = hi - lo
        pos = torch.arange(lo, hi)
        SX = af[lo:hi] @ bf.T
        st = dict(EX=torch.exp2(SX * scale2 - scale2), mlX=mlX_all[lo:hi])
        sp = SX[torch.arange(rows), pos]
        mx = st["mlX"].float()
        st["row"] = [st["EX"].sum(1), mx.sum(1), (mx * SX).sum(1)]
        st["col"] = [st["EX"].sum(0).clone(), mx.sum(0), (mx * SX).sum(0)]
        for name, x, k in (("U", af, kU), ("W", bf, kW)):
            Sq = x[lo:hi] @ k.T
            E = torch.exp2(Sq * scale2 - scale2).masked_fill(~live[None, :].expand_as(Sq), 0.0)
            m = mlQ_all[lo:hi].clone()
            if mutation == "twin_by_value":
                m = m | ((Sq == sp[:, None]) & live[None, :])
            if mutation == "one_direction" and name == "W":
                m = torch.zeros_like(m)
            st["E" + name], st["m" + name] = E, m
            st[name] = [E.sum(1), m.float().sum(1), torch.where(m, Sq, torch.zeros_like(Sq)).sum(1)]
        st["row"] = [x + u for x, u in zip(st["row"], st["U"])]
        for q in range(3):
            if mutation == "stats_local":
                st["col"][q][0:rows] = st["col"][q][0:rows] + st["W"][q]
            else:
                st["col"][q][lo:hi] = st["col"][q][lo:hi] + st["W"][q]
        state.append(st)
    tot = [state[0]["col"][q] for q in range(3)]
    for st in state[1:]:
        tot = [t + st["col"][q] for q, t in enumerate(tot)]
    c_tot, cc_tot, cx_tot = tot
    ct = torch.tensor(coef, dtype=f32) * inv * torch.tensor(upstream, dtype=f32)
    one = torch.tensor(1.0, dtype=f32)
    v, rnc = 1.0 / c_tot, 1.0 / (one + cc_tot)
    out = dict(loss_rows=torch.empty(n), colsum=[st["col"][0] for st in state], colcnt=[st["col"][1] for st in state],
               colsx=[st["col"][2] for st in state], da_loc=torch.empty(a.shape, dtype=f32), db_loc=torch.empty(a.shape, dtype=f32),
               db_all=[], dT=[])
    for (lo, hi), st in zip(shards, state):
        rows = hi - lo
        ii, pos = torch.arange(rows), torch.arange(lo, hi)
        l, rcnt, rsx = st["row"]
        dot = (af[lo:hi] * bf[pos]).sum(1)
        ediag = torch.exp2((dot - 1.0) * inv * log2e)
        u, rn = 1.0 / l, 1.0 / (one + rcnt)
        mean_r, mean_c = (dot + rsx) * rn, (dot + cx_tot[pos]) * rnc[pos]
        out["loss_rows"][lo:hi] = (torch.log(l) + inv - mean_r * inv) + (torch.log(c_tot[pos]) + inv - mean_c * inv)
        uz, rnz = v[pos], rnc[pos]
        prod = st["EX"].to(torch.bfloat16).float() * (u[:, None] + v[None, :])
        WX = torch.where(st["mlX"], prod - (rn[:, None] + rnc[None, :]), prod)
        WX[ii, pos] = ediag * (u + v[pos]) - (rn + rnc[pos])
        WX = (ct * WX).to(torch.bfloat16).float()
        pU = st["EU"].to(torch.bfloat16).float() * u[:, None]
        WU = (ct * torch.where(st["mU"], pU - rn[:, None], pU)).to(torch.bfloat16).float()
        pW = st["EW"].to(torch.bfloat16).float() * uz[:, None]
        WW = (ct * torch.where(st["mW"], pW - rnz[:, None], pW)).to(torch.bfloat16).float()
        dX, dU, dW = WX @ bf, WU @ kU, WW @ kW
        out["da_loc"][lo:hi] = dX + dU
        out["db_loc"][lo:hi] = dW
        out["db_all"].append(WX.T @ af[lo:hi])
        out["dT"].append(-float(((af[lo:hi] * dX).sum() + (af[lo:hi] * dU).sum() + (bf[lo:hi] * dW).sum()) * inv))
    return out
