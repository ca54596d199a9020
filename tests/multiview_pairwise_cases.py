"""Cases, the float64 reference, derived bounds and a CPU emulation shared by tests/test_multiview_pairwise_cpu.py and
tests/test_multiview_pairwise_gpu.py: multi-view InfoNCE with a temperature and a weight per pair (aecf_nce_multi_pp_pair_coef /
_pass1 / _loss / _grads, losses.multiview_info_nce(x, temperature=[P], pair_weights=[P])).  Nothing here touches a GPU; every
function works on the device of the tensors it is given.

Shapes, shards, inputs and twin rows are those of tests/multiview_cases.py (V2, V3A, V4, V8); the mask plans K0 (all present) and
K2 (tile-aligned) those of tests/multiview_masked_cases.py, plus KE below, which leaves the LAST pair without a row.  ``absent``
[n, M] bool over the global rows; all False is the unmasked form.

Definition.  Pair p = (m, n) of multiview_cases.pairs runs at T_p = max(temps[p], MIN_T) over V_p = the rows that hold both
views, n_p = |V_p|.  With weights w_p >= 0 and W = the sum of w_p over the pairs with n_p > 0,
    coef_p = 0.5 / n_p * w_p / W        (0 where n_p = 0, w_p = 0 or W = 0),        L = sum_p coef_p sum_i loss_rows[p][i]
and every pair is the symmetric problem of tests/nce_tile_cases.py restricted to V_p on both sides.  With E_ij = exp((s_ij - 1) /
T_p) on V_p x V_p, l_i = sum_j E_ij and c_j = sum_i E_ij over ALL rows, a shard's share of the temperature gradient is
    dT_p = -(coef_p / T_p^2) [ A + B - 2 D ],   A = sum_(i in shard) RS_i / l_i,   B = sum_j CS_j / c_j,   D = sum_(i in shard) (s_ii - 1)
    RS_i = sum_j E_ij (s_ij - 1),   CS_j = sum_(i in shard) E_ij (s_ij - 1)
and 0 where temps[p] < MIN_T (the clamp has no slope).  tests/test_multiview_pairwise_cpu.py asserts that these expressions are
the float64 autograd of the definition.

Bounds.  loss_rows, colsum, dx_loc, dx_all: the derivation of tests/multiview_masked_cases.py (and through it of
tests/multiview_cases.py and tests/nce_tile_cases.py) pair by pair, value for value, with the pair's own T_p and coef_p in place
of T and coef: ct_p = float32(coef_p) / T_p, xm_p = max |s - 1| / T_p, eps_e, eps_l, eps_c, eps_w of the pair.  coef_p is formed on
the device in float64 and rounded once, as the masked form's: eps_w keeps its 11 h.

dT_p is new: it does not come from the gradient product but from a sweep over the float32 accumulators of the logits pass.  Per
element the kernel forms t_ij = E_ij (s_ij - 1) with E the float32 exponential (relative error eps_e, as every E) and s_ij - 1 from
the accumulator (absolute error 4 s_err, the allowance eps_e grants the MFMA sum, + h): |d t_ij| <= E_ij (|s_ij - 1| (eps_e + 2 h)
+ 4 s_err).  Then, all in float32 and in a fixed order:
  RS_i   16 terms in a lane, 2 lane-group steps, 4 waves, n_tiles partials in four strided sums and a tree of 2:
         depth_r = 16 + 1 + 2 + 3 + ceil(n_tiles / 4) + 2 additions, each <= h of the running sum of |t|
  CS_j   8 row groups in a lane, 4 steps over the 16 rows, 2 waves, m_tiles partials likewise: depth_c = 8 + 4 + 1 + ceil(m_tiles / 4) + 2
  u_i = 1 / l_i: relative eps_l + h;   v_j = 1 / c_j: relative eps_c + h   (eps_l, eps_c as above; c is the all-reduced sum)
  A      one fused multiply-add per row in 256 strided chains and a tree of 8: depth_A = ceil(rows / 256) + 8;   B likewise over cols
  D      s_ii is the finalize kernel's own float32 dot (d / 64 fused multiply-adds in a lane, 6 steps over the wave, unit rows):
         |d (s_ii - 1)| <= (d / 64 + 7) h;  the sum over the rows as A: depth_D = ceil(rows / 256) + 8
  the scalar: coef_p / (T T) (3 roundings with coef_p's own), upstream, (A + B) - 2 D (2), the product (1): 8 h of every magnitude.
With TA = sum_i (1 / l_i) sum_j E_ij |s_ij - 1|, TB the same down the columns of the shard, nV the shard's rows in V_p and
EB = sum_j (sum_(i in shard) E_ij) / c_j <= nV:
  |d A| <= TA (eps_e + 2 h + depth_r h + eps_l + h + depth_A h) + 4 s_err nV
  |d B| <= TB (eps_e + 2 h + depth_c h + eps_c + h + depth_B h) + 4 s_err EB
  |d D| <= nV (d / 64 + 7) h + depth_D h sum |s_ii - 1|
  |d dT_p| <= (coef_p / T_p^2) (|d A| + |d B| + 2 |d D| + 8 h (TA + TB + 2 sum |s_ii - 1|))
The three terms cancel heavily (A + B is close to 2 D wherever the positives dominate their rows), so the bound is absolute and is
NOT small beside dT_p at low T; the mutations of the CPU suite show what it still sees.  A pair with coef_p = 0 or a clamped T_p has
bound 0: its dT_p must be an exact zero.

Temperatures: one distinct value per pair, float32(0.025 * 20^(p / (P - 2))) for p < P - 1 -- 0.025 to 0.5 -- and 0.02, below MIN_T,
for the last pair: it runs at 0.025 and its dT is 0.  Weights: w_p = 0.5 + 0.25 p with w_0 = 0 (in V3A view 0 has pair 0 alone:
its gradient must be exact zeros).  Plan KE empties the last pair, so under it the pairs 1 .. P - 2 keep weight, rows and slope."""
import functools
import math

import torch

from tests import multiview_cases as C
from tests import multiview_masked_cases as K
from tests import nce_tile_cases as N

H, EPS_P, FLUSH = N.H, N.EPS_P, N.FLUSH
MIN_T = N.MIN_T
CASES = ("V2", "V3A", "V4", "V8")
PLANS = ("K0", "K2", "KE")
GRADS = C.GRADS


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def n_pairs(cid):
    c = C.make_case(cid)
    return len(C.pairs(c["views"], c["anchor"]))


@functools.lru_cache(maxsize=None)
def temperatures(cid):
    """the raw per-pair temperatures (float32 values as Python floats); the last entry lies below MIN_T"""
    P = n_pairs(cid)
    return tuple([f32(0.025 * 20.0 ** (p / (P - 2))) for p in range(P - 1)] + [f32(0.02)])


@functools.lru_cache(maxsize=None)
def weights(cid):
    P = n_pairs(cid)
    return tuple([0.0] + [0.5 + 0.25 * p for p in range(1, P)])


@functools.lru_cache(maxsize=None)
def make_mask(cid, plan):
    """absent [n, M] bool (CPU).  KE: the second view of the LAST pair is present exactly where its first view is absent, so that
    pair has no row and drops out of the weight normalisation (its weight is not zero)."""
    if plan in ("K0", "K2"):
        return K.make_mask(cid, plan)
    c = C.make_case(cid)
    n, M, _ = c["x"].shape
    m0, n0 = C.pairs(M, c["anchor"])[-1]
    g = torch.Generator().manual_seed(7900 + CASES.index(cid))
    absent = torch.zeros(n, M, dtype=torch.bool)
    gone = torch.rand(n, generator=g) < 0.3
    absent[:, m0] = gone
    absent[:, n0] = ~gone
    return absent


def pair_coefs(absent, anchor, w):
    """coef_p in float64 as the definition has them; w None: uniform"""
    cnt, _ = K.pair_counts(absent, anchor)
    w = [1.0] * len(cnt) if w is None else [float(v) for v in w]
    total = sum(v for v, k in zip(w, cnt) if k > 0)
    return [0.5 / k * v / total if (k > 0 and v > 0 and total > 0) else 0.0 for v, k in zip(w, cnt)]


def workspace_bytes_py(rows, cols, d, views, anchor):
    """mv_pp_carve() + 256: the unmasked form's pieces, then the partials of E (s - 1), RS, CS and s_ii - 1"""
    g = N.geometry(rows, cols, d)
    Rp, Cp, P = g["Rp"], g["Cp"], len(C.pairs(views, None if anchor < 0 else anchor))
    parts = [P * g["n_tiles"] * Rp * 4, P * g["m_tiles"] * Cp * 4, P * Rp * 4, P * cols * 4, P * Rp * 4]
    return C.workspace_bytes_py(rows, cols, d, views, anchor) + sum(N.up256(p) for p in parts)


def definition(x64, absent, anchor, temps, w, min_t=MIN_T):
    """float64, differentiable in x64 (unit rows) and temps ([P] float64 tensor): sum_p coef_p * symmetric InfoNCE sums of pair p
    over V_p at max(temps[p], min_t)."""
    pres = ~absent.to(x64.device)
    coefs = pair_coefs(absent, anchor, w)
    total = (x64 * 0.0).sum() + (temps * 0.0).sum()
    for p, (m, n) in enumerate(C.pairs(x64.shape[1], anchor)):
        idx = torch.nonzero(pres[:, m] & pres[:, n]).flatten()
        if idx.numel() == 0 or coefs[p] == 0.0:
            continue
        t = torch.clamp(temps[p], min=min_t)
        s = x64[:, m].index_select(0, idx) @ x64[:, n].index_select(0, idx).T / t
        total = total + coefs[p] * (torch.logsumexp(s, dim=1) + torch.logsumexp(s, dim=0) - 2.0 * s.diagonal()).sum()
    return total


def reference(x, absent, shards, anchor, temps, w, s_errs):
    """float64 on the device of x.  Laid out as multiview_masked_cases.reference: loss_rows [P][n], dx_loc [n][M][d] whole; colsum,
    dx_all as lists, one entry per shard; dT a list per shard of [P] float64 tensors, dT_sum their sum; dx_all_sum; loss."""
    n, M, d = x.shape
    dev = x.device
    pr = C.pairs(M, anchor)
    P = len(pr)
    r_da, r_db = C.roles(M, anchor)
    absent = absent.to(dev)
    pres = ~absent
    coefs = pair_coefs(absent, anchor, w)
    x64 = x.double()
    ax = x64.abs()
    geoms = [N.geometry(hi - lo, n, d) for lo, hi in shards]
    f64 = dict(dtype=torch.float64, device=dev)
    ref = dict(loss_rows=torch.zeros(P, n, **f64), dx_loc=torch.zeros(n, M, d, **f64), colsum=[torch.zeros(P, n, **f64) for _ in shards],
               dx_all=[torch.zeros(n, M, d, **f64) for _ in shards], dT=[torch.zeros(P, **f64) for _ in shards])
    bnd = dict(loss_rows=torch.zeros(P, n, **f64), dx_loc=torch.zeros(n, M, d, **f64), colsum=[torch.zeros(P, n, **f64) for _ in shards],
               dx_all=[torch.zeros(n, M, d, **f64) for _ in shards], dT=[torch.zeros(P, **f64) for _ in shards])
    i_all = torch.arange(n, device=dev)
    neg = torch.tensor(float("-inf"), **f64)
    zero = torch.zeros((), **f64)
    loss, loss_bnd = 0.0, 0.0
    for p, (m, nn) in enumerate(pr):
        V = pres[:, m] & pres[:, nn]
        if not bool(V.any()):
            continue
        T = max(temps[p], MIN_T)
        clamped = temps[p] < MIN_T
        coef = coefs[p]
        ct = coef / T
        flush = FLUSH * (1.0 + ct)
        VV = V[:, None] & V[None, :]
        a, b = x64[:, m], x64[:, nn]
        S = a @ b.T
        xm = float(torch.where(VV, torch.maximum(S.abs(), (S - 1.0).abs()), zero).max()) / T
        xs = torch.where(VV, S / T, neg)
        E = torch.where(VV, torch.exp((S - 1.0) / T), zero)
        Sm1 = torch.where(VV, S - 1.0, zero)
        sdiag = torch.where(V, S.diagonal() - 1.0, zero)
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
        l_all, c_all = E.sum(1), E.sum(0)
        inv_l = torch.where(V, 1.0 / l_all.clamp_min(1e-300), zero)
        inv_c = torch.where(V, 1.0 / c_all.clamp_min(1e-300), zero)
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
            if coef > 0.0:
                BW = torch.where(inside, ct * ((1.0 + EPS_P) ** 2 * (1.0 + eps_w) - 1.0) * Qs + flush, zero)
                gd = Gs[ii, pos].abs()
                BW[ii, pos] = torch.where(V[lo:hi], ct * (EPS_P * gd + (1.0 + EPS_P) * (eps_w * Qs[ii, pos] + 8.0 * H * gd)) + flush, zero)
                mag = ct * Gs.abs() + BW
                bnd["dx_loc"][lo:hi, m] += (BW + (s_da * g["Cp"] + 32) * H * mag) @ ax[:, nn]
                bnd["dx_all"][k][:, nn] += (BW + (s_db * g["Rp"] + 32) * H * mag).T @ ax[lo:hi, m]
            # dT_p of the shard and its bound (the docstring's derivation); a zero coef or a clamped T: exact zero, bound 0
            if coef > 0.0 and not clamped:
                Es, Ts = E[lo:hi], E[lo:hi] * Sm1[lo:hi]
                A = float((Ts.sum(1) * inv_l[lo:hi]).sum())
                B = float((Ts.sum(0) * inv_c).sum())
                D = float(sdiag[lo:hi].sum())
                TA = float((Ts.abs().sum(1) * inv_l[lo:hi]).sum())
                TB = float((Ts.abs().sum(0) * inv_c).sum())
                SD = float(sdiag[lo:hi].abs().sum())
                nV = int(V[lo:hi].sum())
                EB = float((Es.sum(0) * inv_c).sum())
                rows = hi - lo
                depth_r = 16 + 1 + 2 + 3 + -(-g["n_tiles"] // 4) + 2
                depth_c = 8 + 4 + 1 + -(-g["m_tiles"] // 4) + 2
                depth_A = -(-rows // 256) + 8
                depth_B = -(-n // 256) + 8
                dA = TA * (eps_e + 2.0 * H + depth_r * H + eps_l + H + depth_A * H) + 4.0 * s_errs[p] * nV
                dB = TB * (eps_e + 2.0 * H + depth_c * H + eps_c + H + depth_B * H) + 4.0 * s_errs[p] * EB
                dD = nV * (d // 64 + 7) * H + depth_A * H * SD
                gsc = coef / (T * T)
                ref["dT"][k][p] = -gsc * (A + B - 2.0 * D)
                bnd["dT"][k][p] = gsc * (dA + dB + 2.0 * dD + 8.0 * H * (TA + TB + 2.0 * SD))
        loss += coef * float(ref["loss_rows"][p].sum())
        loss_bnd += coef * float(bnd["loss_rows"][p].sum())
    ref["dx_all_sum"], bnd["dx_all_sum"] = sum(ref["dx_all"]), sum(bnd["dx_all"])
    ref["dT_sum"], bnd["dT_sum"] = sum(ref["dT"]), sum(bnd["dT"])
    ref["loss"], bnd["loss"] = loss, loss_bnd + 2.0 ** -20 * abs(loss)
    return ref, bnd


def ratios(got, ref, bnd, bf16=False):
    """multiview_masked_cases.ratios for the tensors and the loss; dT ([P] per shard) and dT_sum elementwise by the same rule: an
    element whose bound is 0 must be exactly 0 (it counts as 0 or inf)."""
    plain = {k: v for k, v in got.items() if k not in ("dT", "dT_sum")}
    out = K.ratios(plain, ref, bnd, bf16=bf16)
    for name in ("dT", "dT_sum"):
        if name not in got:
            continue
        gs, rs, bs = (got[name], ref[name], bnd[name]) if name == "dT" else ([got[name]], [ref[name]], [bnd[name]])
        worst = 0.0
        for g, r, b in zip(gs, rs, bs):
            g = torch.as_tensor(g, dtype=torch.float64, device=r.device)
            if not bool(torch.isfinite(g).all()):
                worst = float("inf")
                continue
            err = (g - r).abs()
            q = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
            worst = max(worst, float(q.max()))
        out[name] = worst
    return out


# ---- the design's arithmetic on the CPU ----
MUTATIONS = ("T_pair0", "T_by_view", "dT_per_view", "w_unnormalised", "w_norm_all", "c_local")


def emulate(x, absent, shards, anchor, temps, w, mutation=None, bf16_out=False):
    """The kernels' arithmetic on the CPU: multiview_masked_cases.emulate with the pair's own temperature and coefficient, and dT_p
    by the route the kernels take (float32 sums of E (s - 1) from the float32 scores, u, v and s_ii - 1).  Output laid out as
    ``reference``.  mutation, one broken rule each:
      T_pair0          the temperature of pair 0 serves every pair
      T_by_view        the temperature is indexed by the pair's a-role view m, not by the pair
      dT_per_view      dT is formed per VIEW from the gradient product (the one-temperature route) and dealt evenly over the view's pairs
      w_unnormalised   coef_p = 0.5 / n_p * w_p, the sum of the weights is not divided out
      w_norm_all       the weights are normalised over all pairs, the empty ones included
      c_local          the column term of dT uses 1 / (this shard's column sums), not 1 / (the all-reduced ones)"""
    n, M, d = x.shape
    pr = C.pairs(M, anchor)
    P = len(pr)
    r_da, r_db = C.roles(M, anchor)
    pres = ~absent
    cnt, _ = K.pair_counts(absent, anchor)
    wl = [1.0] * P if w is None else [float(v) for v in w]
    if mutation == "w_unnormalised":
        total = 1.0
    elif mutation == "w_norm_all":
        total = sum(wl)
    else:
        total = sum(v for v, k in zip(wl, cnt) if k > 0)
    xf = x.float()
    f = torch.float32
    log2e = torch.tensor(1.4426950408889634, dtype=f)
    zero = torch.zeros((), dtype=f)
    out = dict(loss_rows=torch.zeros(P, n), colsum=[torch.zeros(P, n) for _ in shards], dx_loc=torch.zeros(n, M, d),
               dx_all=[torch.zeros(n, M, d) for _ in shards], dT=[torch.zeros(P) for _ in shards])
    W = {}
    inv_of, coef_of = {}, {}
    loss = torch.zeros((), dtype=f)
    for p, (m, nn) in enumerate(pr):
        V = pres[:, m] & pres[:, nn]
        t_raw = temps[0] if mutation == "T_pair0" else (temps[m % P] if mutation == "T_by_view" else temps[p])
        tc = torch.tensor(max(t_raw, MIN_T), dtype=f)
        inv = torch.tensor(1.0, dtype=f) / tc
        scale2 = inv * log2e
        coef = 0.5 / cnt[p] / (total / wl[p]) if (cnt[p] > 0 and wl[p] > 0 and total > 0) else 0.0
        coef32 = torch.tensor(coef, dtype=f)
        ct = coef32 * inv
        inv_of[p], coef_of[p] = inv, coef32
        af, bf = xf[:, m], xf[:, nn]
        st = []
        for lo, hi in shards:
            rowok = V[lo:hi]
            S = af[lo:hi] @ bf.T
            ok = rowok[:, None] & V[None, :]
            E_all = torch.exp2(S * scale2 - scale2)
            E = torch.where(ok, E_all, zero)
            Tm = torch.where(ok, E_all * (S - 1.0), zero)
            st.append(dict(E=E, l=E.sum(1), c=E.sum(0), rs=Tm.sum(1), cs=Tm.sum(0), rowok=rowok))
        c_tot = st[0]["c"]
        for s in st[1:]:
            c_tot = c_tot + s["c"]
        pair_rows = torch.zeros((), dtype=f)
        for k, ((lo, hi), s) in enumerate(zip(shards, st)):
            out["colsum"][k][p] = s["c"]
            rowok = s["rowok"]
            i = torch.arange(hi - lo)
            pos = lo + i
            dot = (af[lo:hi] * bf[pos]).sum(1)
            ediag = torch.where(rowok, torch.exp2((dot - 1.0) * inv * log2e), zero)
            rows = (torch.log(s["l"]) + inv - dot * inv) + (torch.log(c_tot[pos]) + inv - dot * inv)
            out["loss_rows"][p, lo:hi] = torch.where(rowok, rows, zero)
            pair_rows = pair_rows + out["loss_rows"][p, lo:hi].sum()
            u = torch.where(rowok, 1.0 / s["l"], zero)
            v = torch.where(V, 1.0 / c_tot, zero)
            Eb = s["E"].to(torch.bfloat16).float()
            Wp = ct * (Eb * (u[:, None] + v[None, :]))
            part = ct * (ediag * (u + v[pos]) - 2.0)
            Wp[i[rowok], pos[rowok]] = part[rowok]
            W[p, k] = Wp.to(torch.bfloat16).float()
            # dT_p: the kernels' route
            v_dt = torch.where(V & (s["c"] > 0), 1.0 / s["c"], zero) if mutation == "c_local" else v
            sdiag = torch.where(rowok, dot - 1.0, zero)
            total_p = ((u * s["rs"]).sum() + (v_dt * s["cs"]).sum()) - 2.0 * sdiag.sum()
            g = coef32 / (tc * tc)
            out["dT"][k][p] = -g * total_p if (t_raw >= MIN_T and coef != 0.0) else 0.0
        loss = loss + pair_rows * coef32
    out["loss"] = float(loss)

    def rnd(t):
        return t.to(torch.bfloat16).float()

    for k, (lo, hi) in enumerate(shards):
        for m, segs in r_da.items():
            da = torch.cat([W[p, k] for p, _ in segs], dim=1) @ torch.cat([xf[:, nn] for _, nn in segs], dim=0)
            out["dx_loc"][lo:hi, m] = rnd(da) if bf16_out else da
            if mutation == "dT_per_view":
                td = (xf[lo:hi, m] * da).sum()
                for p, _ in segs:
                    out["dT"][k][p] = -float(td * inv_of[p]) / len(segs) if (temps[p] >= MIN_T and float(coef_of[p]) != 0.0) else 0.0
        for nn, segs in r_db.items():
            db = torch.cat([W[p, k].T for p, _ in segs], dim=1) @ torch.cat([xf[lo:hi, m] for _, m in segs], dim=0)
            out["dx_all"][k][:, nn] = rnd(db) if bf16_out else db
    out["dT_sum"] = sum(t.double() for t in out["dT"])
    return out
