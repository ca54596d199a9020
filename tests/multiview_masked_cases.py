"""Mask plans, the float64 reference in two formulations, derived bounds and a CPU emulation shared by
tests/test_multiview_masked_cpu.py and tests/test_multiview_masked_gpu.py: multi-view InfoNCE with missing views
(aecf_nce_multi_masked_pair_coef / _pass1 / _loss / _grads, losses.multiview_info_nce(..., key_padding_mask=...)).  Nothing here
touches a GPU; every function works on the device of the tensors it is given.

Shapes, shards, inputs and twin rows are those of tests/multiview_cases.py (V2, V3, V3A, V4, V8).  ``absent`` [n, M] bool is the
padding mask over the GLOBAL rows (True: view m of row g is absent); a shard (lo, hi) reads its rows as absent[lo:hi].

Definition.  For pair p = (m, n): V_p = the rows that hold both views, n_p = |V_p|, P' = the pairs with n_p > 0,
coef_p = 0.5 / n_p / P' (0 for an empty pair).  Pair p is the symmetric problem of tests/nce_tile_cases.py restricted to V_p on both
sides; a row outside V_p has a loss row of 0, a zero row of G and a zero column of G.  ``reference`` evaluates this by masking
(-inf logits outside V_p x V_p); ``compacted_loss`` evaluates the same as the mean over the non-empty pairs of the symmetric
InfoNCE of x[V_p, m] against x[V_p, n] on gathered copies, for autograd -- the CPU suite asserts that the two agree.

Bounds: the derivation of tests/multiview_cases.py (and through it of tests/nce_tile_cases.py) at the UNCOMPACTED geometry of the
shard -- the kernels run every pair over all Rp x Cp elements, so the summation depths are those of the unmasked form -- with
these changes.  An element outside V_p x V_p is a select of an exact zero: it is 0 in the stored block, in every partial, in
every sum and in every product, and adds no rounding; the reference holds a zero there and the bound IS zero (such an element
must come out as an exact zero).  Q, G, xm and the column sums of the bound expressions are therefore those of the masked
problem.  ct_p = float32(coef_p) / T: coef_p is formed in float64 and rounded once, one h more on the float32 factor of W next to
the roundings the two-view derivation counts: eps_w = eps_e + max(eps_l, eps_c) + 11 h.  Everything else is value for value the
expression of tests/multiview_cases.reference; with every view present it differs from it by that one h alone.

The value L = sum_p coef_p sum_i loss_rows[p][i] is a float32 sum of P n <= 2^13 non-negative terms in trees of depth <= 14, a
rounding of coef_p and a product per pair: 2^-20 of the value beside the rows' own bounds (as tests/test_multiview_gpu.py takes
it for the unmasked form).

Mask plans (each named for what it catches):
  K0 all present            the unmasked form's bits
  K1 random presence        0.7 per (row, view); row 0 keeps no view, row 1 keeps view 0 alone
  K2 tile-aligned           view 1 absent on rows 0..255, present from 256 on: whole absent row tiles and column tiles beside full ones
  K3 an empty pair          the first pair's second view is present exactly where its first view is absent: n_p = 0, P' = P - 1
  K4 a pair of one row      the first pair's views overlap in one row: n_p = 1, its loss is 0 to rounding
  K5 an absent twin         of every second twin pair (r', r), and of those on a later shard's first row, the row r' lacks the second
                            view of the first pair -- and keeps its data there: a kept key moves row r's loss by about ln 2
(K6, poison in the absent slots, is a GPU test on K1.)"""
import functools
import math

import torch

from tests import multiview_cases as C
from tests import nce_tile_cases as N

H, EPS_P, FLUSH = N.H, N.EPS_P, N.FLUSH
TEMPS = N.TEMPS
MIN_T = N.MIN_T
CASES = ("V2", "V3", "V3A", "V4", "V8")
PLANS = ("K0", "K1", "K2", "K3", "K4", "K5")
SHARDED = ("V2", "V4")              # the cases whose shards put row_offset != 0 under K1, K2 and K5


@functools.lru_cache(maxsize=None)
def make_mask(cid, plan):
    """absent [n, M] bool (CPU) of a case under a plan"""
    c = C.make_case(cid)
    n, M, _ = c["x"].shape
    pr = C.pairs(M, c["anchor"])
    m0, n0 = pr[0]
    g = torch.Generator().manual_seed(7300 + 16 * CASES.index(cid) + PLANS.index(plan))
    absent = torch.zeros(n, M, dtype=torch.bool)
    if plan == "K1":
        absent = torch.rand(n, M, generator=g) > 0.7
        absent[0] = True
        absent[1] = True
        absent[1, 0] = False
    elif plan == "K2":
        absent[:256, 1] = True
    elif plan == "K3":
        gone = torch.rand(n, generator=g) < 0.3
        absent[:, m0] = gone
        absent[:, n0] = ~gone
    elif plan == "K4":
        h = n // 2
        absent[h + 1:, m0] = True
        absent[:h, n0] = True
    elif plan == "K5":
        starts = {lo for lo, _ in c["shards"] if lo > 0}
        for k, (rp, _) in enumerate(c["twins"]):
            if (k % 2 == 0 and rp != 0) or rp in starts:    # (a later shard's first row always, row 0 never: the shards differ)
                absent[rp, n0] = True
    return absent


def presence_bytes(absent):
    """[n] uint8, bit v = view v present"""
    M = absent.shape[1]
    w = (1 << torch.arange(M, device=absent.device)).to(torch.int64)
    return ((~absent).to(torch.int64) * w).sum(1).to(torch.uint8)


def pair_counts(absent, anchor):
    """(n_p of every pair, P')"""
    pres = ~absent
    cnt = [int((pres[:, m] & pres[:, n]).sum()) for m, n in C.pairs(absent.shape[1], anchor)]
    return cnt, sum(1 for v in cnt if v > 0)


def pair_coefs(absent, anchor):
    """coef_p in float64 as the definition has them"""
    cnt, live = pair_counts(absent, anchor)
    return [0.5 / v / live if v > 0 else 0.0 for v in cnt]


def reference(x, absent, shards, anchor, T, s_errs):
    """float64 on the device of x, by masking.  Laid out as multiview_cases.reference: loss_rows [P][n], dx_loc [n][M][d] whole;
    colsum, dx_all, dT as lists, one entry per shard; dx_all_sum; plus loss = sum_p coef_p sum_i loss_rows and its bound."""
    n, M, d = x.shape
    dev = x.device
    pr = C.pairs(M, anchor)
    r_da, r_db = C.roles(M, anchor)
    absent = absent.to(dev)
    pres = ~absent
    coefs = pair_coefs(absent, anchor)
    x64 = x.double()
    ax = x64.abs()
    geoms = [N.geometry(hi - lo, n, d) for lo, hi in shards]
    f64 = dict(dtype=torch.float64, device=dev)
    ref = dict(loss_rows=torch.zeros(len(pr), n, **f64), dx_loc=torch.zeros(n, M, d, **f64),
               colsum=[torch.zeros(len(pr), n, **f64) for _ in shards], dx_all=[torch.zeros(n, M, d, **f64) for _ in shards], dT=[])
    bnd = dict(loss_rows=torch.zeros(len(pr), n, **f64), dx_loc=torch.zeros(n, M, d, **f64),
               colsum=[torch.zeros(len(pr), n, **f64) for _ in shards], dx_all=[torch.zeros(n, M, d, **f64) for _ in shards], dT=[])
    i_all = torch.arange(n, device=dev)
    neg = torch.tensor(float("-inf"), **f64)
    zero = torch.zeros((), **f64)
    loss, loss_bnd = 0.0, 0.0
    for p, (m, nn) in enumerate(pr):
        V = pres[:, m] & pres[:, nn]
        if not bool(V.any()):
            continue
        coef = coefs[p]
        ct = coef / T
        flush = FLUSH * (1.0 + ct)
        VV = V[:, None] & V[None, :]
        a, b = x64[:, m], x64[:, nn]
        S = a @ b.T
        xm = float(torch.where(VV, torch.maximum(S.abs(), (S - 1.0).abs()), zero).max()) / T
        xs = torch.where(VV, S / T, neg)
        E = torch.where(VV, torch.exp((S - 1.0) / T), zero)
        del S
        lse_row = torch.where(V, torch.logsumexp(xs, dim=1), zero)
        lse_col = torch.where(V, torch.logsumexp(xs, dim=0), zero)
        xii = torch.where(V, xs.diagonal(), zero)
        Q = torch.where(VV, torch.exp(xs - lse_row[:, None]) + torch.exp(xs - lse_col[None, :]), zero)
        del xs
        G = Q.clone()
        G[i_all[V], i_all[V]] -= 2.0
        ref["loss_rows"][p] = torch.where(V, lse_row + lse_col - 2.0 * xii, zero)
        ref["dx_loc"][:, m] += ct * (G @ b)
        eps_e = 4.0 * s_errs[p] / T + 6.0 * H * xm + 2.0 * H
        eps_c = eps_e + (max(15 + -(-g["m_tiles"] // 4) for g in geoms) + len(shards) - 1) * H
        Mx = xm + 1.0 / T + math.log(n)
        s_da, s_db = len(r_da[m]), len(r_db[nn])
        for k, ((lo, hi), g) in enumerate(zip(shards, geoms)):
            eps_l = eps_e + (12 + -(-g["n_tiles"] // 4)) * H
            eps_cs = eps_e + (15 + -(-g["m_tiles"] // 4)) * H
            eps_w = eps_e + max(eps_l, eps_c) + 11.0 * H
            bnd["loss_rows"][p, lo:hi] = torch.where(V[lo:hi], torch.full((hi - lo,), eps_l + eps_c + 2.0 * (4.0 * s_errs[p] / T + 2.0 * H * xm)
                                                                          + 12.0 * H * Mx, **f64), zero)
            cs = E[lo:hi].sum(0)
            ref["colsum"][k][p], bnd["colsum"][k][p] = cs, eps_cs * cs
            Gs, Qs = G[lo:hi], Q[lo:hi]
            ref["dx_all"][k][:, nn] += ct * (Gs.T @ a[lo:hi])
            ii, pos = torch.arange(hi - lo, device=dev), i_all[lo:hi]
            inside = VV[lo:hi]
            BW = torch.where(inside, ct * ((1.0 + EPS_P) ** 2 * (1.0 + eps_w) - 1.0) * Qs + flush, zero)
            gd = Gs[ii, pos].abs()
            BW[ii, pos] = torch.where(V[lo:hi], ct * (EPS_P * gd + (1.0 + EPS_P) * (eps_w * Qs[ii, pos] + 8.0 * H * gd)) + flush, zero)
            mag = ct * Gs.abs() + BW
            bnd["dx_loc"][lo:hi, m] += (BW + (s_da * g["Cp"] + 32) * H * mag) @ ax[:, nn]
            bnd["dx_all"][k][:, nn] += (BW + (s_db * g["Rp"] + 32) * H * mag).T @ ax[lo:hi, m]
        loss += coef * float(ref["loss_rows"][p].sum())
        loss_bnd += coef * float(bnd["loss_rows"][p].sum())
    # a gradient slot of an absent (row, view) must be an exact zero: W is zero in its whole row / column of every pair
    for (lo, hi), g in zip(shards, geoms):
        dT, lin, quad = 0.0, 0.0, 0.0
        for m in r_da:
            dT += -(1.0 / T) * float((x64[lo:hi, m] * ref["dx_loc"][lo:hi, m]).sum())
            lin += float((ax[lo:hi, m] * bnd["dx_loc"][lo:hi, m]).sum())
            quad += float((ax[lo:hi, m] * (ref["dx_loc"][lo:hi, m].abs() + bnd["dx_loc"][lo:hi, m])).sum())
        depth = 145 + -(-(len(r_da) * g["splits"] * g["m_tiles"] * g["d_tiles"]) // 256)
        ref["dT"].append(dT)
        bnd["dT"].append((lin + depth * H * quad) / T + 3.0 * H * abs(dT))
    ref["dx_all_sum"], bnd["dx_all_sum"] = sum(ref["dx_all"]), sum(bnd["dx_all"])
    ref["loss"], bnd["loss"] = loss, loss_bnd + 2.0 ** -20 * abs(loss)
    return ref, bnd


def compacted_loss(x64, absent, anchor, t):
    """The second formulation, differentiable: the mean over the non-empty pairs of info_nce(x[V_p, m], x[V_p, n]) on gathered
    (index_select-ed) copies of the rows of V_p.  x64 [n, M, d] float64 unit rows, t a float64 scalar (tensor or number)."""
    pres = ~absent.to(x64.device)
    terms = []
    for m, n in C.pairs(x64.shape[1], anchor):
        idx = torch.nonzero(pres[:, m] & pres[:, n]).flatten()
        if idx.numel() == 0:
            continue
        s = x64[:, m].index_select(0, idx) @ x64[:, n].index_select(0, idx).T / t
        terms.append(0.5 * (torch.logsumexp(s, dim=1) + torch.logsumexp(s, dim=0) - 2.0 * s.diagonal()).mean())
    if not terms:
        return (x64 * 0.0).sum()
    return torch.stack(terms).mean()


def ratios(got, ref, bnd, bf16=False):
    """multiview_cases.ratios, with two additions: an output that is not finite counts as inf (a NaN must not pass a maximum),
    and the value ``loss`` is judged where ``got`` holds it"""
    for name, v in got.items():
        for t in (v if isinstance(v, list) else [v]):
            if isinstance(t, torch.Tensor) and not bool(torch.isfinite(t).all()):
                return {name: float("inf")}
            if not isinstance(t, torch.Tensor) and not math.isfinite(float(t)):
                return {name: float("inf")}
    out = C.ratios(got, ref, bnd, bf16=bf16)
    if "loss" in got:
        out["loss"] = abs(float(got["loss"]) - ref["loss"]) / bnd["loss"] if bnd["loss"] > 0 else (0.0 if float(got["loss"]) == 0.0 else float("inf"))
    return out


# ---- the design's arithmetic on the CPU ----
MUTATIONS = ("keys_kept", "rows_only", "one_over_b_all", "P_for_P_live", "row_mask_global", "partner_absent")


def emulate(x, absent, shards, anchor, T, mutation=None, bf16_out=False):
    """The kernels' arithmetic on the CPU: multiview_cases.emulate with the selects of the masked form.  x [n, M, d] bf16 keeps
    its data in the absent slots (finite: what the masked kernels are handed must exclude by the mask).  Output laid out as
    ``reference`` (with ``loss``).  mutation, one broken rule each:
      keys_kept         the row sums run over every key: absent keys stay in the row denominators
      rows_only         E is zeroed for absent rows alone: absent columns stay keys and keep column sums
      one_over_b_all    coef_p = 0.5 / b_all / P' in place of 0.5 / n_p / P'
      P_for_P_live      coef_p = 0.5 / n_p / P
      row_mask_global   a shard reads the presence of its local row i at the global index row_offset + i of its LOCAL bytes,
                        i.e. the byte of global row (2 row_offset + i) mod n
      partner_absent    the partner term -2 [j = off + i] is applied to the rows outside V_p too"""
    n, M, d = x.shape
    pr = C.pairs(M, anchor)
    r_da, r_db = C.roles(M, anchor)
    pres = ~absent
    cnt, live = pair_counts(absent, anchor)
    xf = x.float()
    f32 = torch.float32
    inv = torch.tensor(1.0, dtype=f32) / torch.tensor(T, dtype=f32)
    log2e = torch.tensor(1.4426950408889634, dtype=f32)
    scale2 = inv * log2e
    out = dict(loss_rows=torch.zeros(len(pr), n), colsum=[torch.zeros(len(pr), n) for _ in shards],
               dx_loc=torch.zeros(n, M, d), dx_all=[torch.zeros(n, M, d) for _ in shards], dT=[])
    W = {}
    loss = torch.zeros((), dtype=f32)
    for p, (m, nn) in enumerate(pr):
        V = pres[:, m] & pres[:, nn]
        if mutation == "one_over_b_all":
            coef = 0.5 / n / live if cnt[p] else 0.0
        elif mutation == "P_for_P_live":
            coef = 0.5 / cnt[p] / len(pr) if cnt[p] else 0.0
        else:
            coef = 0.5 / cnt[p] / live if cnt[p] else 0.0
        ct = torch.tensor(coef, dtype=f32) * inv
        af, bf = xf[:, m], xf[:, nn]
        colok = torch.ones_like(V) if mutation == "rows_only" else V
        st = []
        for lo, hi in shards:
            rowok = V[lo:hi]
            if mutation == "row_mask_global":
                rowok = V[(2 * lo + torch.arange(hi - lo)) % n]
            E_all = torch.exp2((af[lo:hi] @ bf.T) * scale2 - scale2)
            E = torch.where(rowok[:, None] & colok[None, :], E_all, torch.zeros(()))
            l = torch.where(rowok[:, None], E_all, torch.zeros(())).sum(1) if mutation == "keys_kept" else E.sum(1)
            st.append(dict(E=E, l=l, c=E.sum(0), rowok=rowok))
        c_tot = st[0]["c"]
        for s in st[1:]:
            c_tot = c_tot + s["c"]
        pair_rows = torch.zeros((), dtype=f32)
        for k, ((lo, hi), s) in enumerate(zip(shards, st)):
            out["colsum"][k][p] = s["c"]
            rowok = s["rowok"]
            i = torch.arange(hi - lo)
            pos = lo + i
            dot = (af[lo:hi] * bf[pos]).sum(1)
            ediag = torch.where(rowok, torch.exp2((dot - 1.0) * inv * log2e), torch.zeros(()))
            rows = (torch.log(s["l"]) + inv - dot * inv) + (torch.log(c_tot[pos]) + inv - dot * inv)
            out["loss_rows"][p, lo:hi] = torch.where(rowok, rows, torch.zeros(()))
            pair_rows = pair_rows + out["loss_rows"][p, lo:hi].sum()
            u = torch.where(rowok, 1.0 / s["l"], torch.zeros(()))
            v = torch.where(colok, 1.0 / c_tot, torch.zeros(()))
            Eb = s["E"].to(torch.bfloat16).float()
            Wp = ct * (Eb * (u[:, None] + v[None, :]))
            part = ct * (ediag * (u + v[pos]) - 2.0)
            sel = torch.ones_like(rowok) if mutation == "partner_absent" else rowok
            Wp[i[sel], pos[sel]] = part[sel]
            W[p, k] = Wp.to(torch.bfloat16).float()
        loss = loss + pair_rows * torch.tensor(coef, dtype=f32)
    out["loss"] = float(loss)

    def rnd(t):
        return t.to(torch.bfloat16).float()

    for k, (lo, hi) in enumerate(shards):
        td = torch.zeros((), dtype=f32)
        for m, segs in r_da.items():
            da = torch.cat([W[p, k] for p, _ in segs], dim=1) @ torch.cat([xf[:, nn] for _, nn in segs], dim=0)
            td = td + (xf[lo:hi, m] * da).sum()
            out["dx_loc"][lo:hi, m] = rnd(da) if bf16_out else da
        out["dT"].append(-float(td * inv))
        for nn, segs in r_db.items():
            db = torch.cat([W[p, k].T for p, _ in segs], dim=1) @ torch.cat([xf[lo:hi, m] for _, m in segs], dim=0)
            out["dx_all"][k][:, nn] = rnd(db) if bf16_out else db
    return out
