"""Cases, inputs, the float64 reference, derived bounds and a CPU emulation shared by tests/test_multiview_cpu.py and
tests/test_multiview_gpu.py: multi-view InfoNCE (aecf_nce_multi_pass1 / _loss / _grads, losses.multiview_info_nce) on the tile
GEMMs.  Nothing here touches a GPU; every function works on the device of the tensors it is given.

x [n, M, d] holds M views.  The pairs (m, n), m < n: every pair in lexicographic order (anchor None), or (min(k, n), max(k, n))
for n != k rising (anchor k).  Every pair is the symmetric problem of tests/nce_tile_cases.py on a = x[:, m], b = x[:, n]
(off = 0, the rows dealt over shards), all pairs at one T and one coef.  Outputs, per view and role:
  loss_rows [P][n], colsum per shard [P][n]      the pair's own, as nce_tile_cases.reference(..., sym=1) gives them
  dx_loc [n][M][d]     dx_loc[:, m] = sum over the pairs (m, .) of the pair's da          (a role; 0 for a view without one)
  dx_all per shard     dx_all[:, n] = sum over the pairs (., n) of the shard's share of db (b role; 0 likewise)
  dT per shard         the sum of the pairs' dT = -(1/T) sum_m sum_i x_im . dx_loc_im

Bounds: the derivation of the docstring of tests/nce_tile_cases.py, pair by pair, with these changes.  The kernels form the
weights W_p of every pair exactly as the two-view form does, so |d W_p| <= BW_p as there (BW_p from the pair's own score error,
eps_e, eps_l, eps_c, eps_w).  A gradient element is then ONE float32 sum over ALL the partner blocks of its view: with S partner
blocks the K loop of da runs over S Cp padded keys (and the slab sum over <= 32 splits), that of db over S Rp padded rows, so
      |d dx_loc[:, m]| <= sum over the S pairs (m, n) of (BW_p + (S Cp + 32) h (ct |G_p| + BW_p)) |x[:, n]|
      |d dx_all[:, n]| <= sum over the S pairs (m, n) of (BW_p + (S Rp + 32) h (ct |G_p| + BW_p))^T |x[:, m]|
-- the BW terms add over the partner blocks, and the summation term counts the terms that land on the output, not a pair's.
dT is reduced from splits m_tiles d_tiles partials per view with the a role, all views in one nce_dtemp_kernel:
      |d dT| <= (1/T) (sum |x_m| bound_m + (145 + ceil(parts / 256)) h sum |x_m| (|dx_loc_m| + bound_m)) + 3 h |dT|,
      parts = (views with the a role) splits m_tiles d_tiles, the sums over those views.
With M = 2 there is one pair and S = 1 everywhere: every bound is the expression of nce_tile_cases.reference, value for value.

Inputs: view 0 is nce_tile_cases.make_rows' a (unit rows, the symmetric twins of the case's shards); views 1 .. M - 1 are rows at
cosine 0.8 to view 0 with independent noise; every twin row is copied in ALL views, so in every pair rows r and r' each hold
half of each other's softmax and a lost or doubled key moves a loss row by about ln 2."""
import functools

import torch

from tests import nce_tile_cases as N

H, EPS_P, FLUSH = N.H, N.EPS_P, N.FLUSH
TEMPS = N.TEMPS
MIN_T = N.MIN_T

# id: (the case of N.SYMMETRIC whose shape and shards it takes, views, anchor)
CASES = {
    "V1": ("S1", 3, None),      # 1 x 64: one row
    "V2": ("S2", 3, None),      # 257 x 128, two shards
    "V3": ("S3", 3, None),      # 300 x 192
    "V3A": ("S3", 4, 2),        # the anchor in the a role for one partner and in the b role for two
    "V4": ("S4", 3, None),      # 2305 x 256, three shards, 5 da splits
    "V8": ("S2", 8, None),      # P = 28: the edge of the pair table
}


def pairs(views, anchor=None):
    if anchor is None:
        return [(m, n) for m in range(views) for n in range(m + 1, views)]
    return [(min(anchor, n), max(anchor, n)) for n in range(views) if n != anchor]


def roles(views, anchor=None):
    """({view m: [(pair index, partner n), ...]} of the a role, {view n: [(pair index, partner m), ...]} of the b role), pair order"""
    da, db = {}, {}
    for p, (m, n) in enumerate(pairs(views, anchor)):
        da.setdefault(m, []).append((p, n))
        db.setdefault(n, []).append((p, m))
    return da, db


def workspace_bytes_py(rows, cols, d, views, anchor):
    """mv_carve() + 256: per pair E, the two partial arrays, l, u, v, ediag; then the da slabs -- each rounded up to 256 bytes"""
    g = N.geometry(rows, cols, d)
    Rp, Cp, P = g["Rp"], g["Cp"], len(pairs(views, None if anchor < 0 else anchor))
    parts = [P * Rp * Cp * 2, P * g["n_tiles"] * Rp * 4, P * g["m_tiles"] * Cp * 4, P * Rp * 4, P * Rp * 4, P * Cp * 4, P * Rp * 4,
             g["splits"] * rows * views * d * 4]
    return sum(N.up256(p) for p in parts) + 256


@functools.lru_cache(maxsize=None)
def make_case(cid):
    """x [n, M, d] bf16 (CPU), the shard bounds, the anchor and the twins of a case"""
    sid, views, anchor = CASES[cid]
    (n, d), shards, _, _ = N.SYMMETRIC[sid]
    v0, v1, twins = N.make_rows(n, d, shards, 6100 + list(CASES).index(cid))
    g = torch.Generator().manual_seed(6200 + list(CASES).index(cid))
    cols = [v0, v1]
    for _ in range(2, views):
        v = N._positives(N._unit(v0.float()), g).to(torch.bfloat16)
        for rp, r in twins:
            v[rp] = v[r]
        cols.append(v)
    return dict(x=torch.stack(cols, dim=1).contiguous(), shards=list(shards), views=views, anchor=anchor, twins=twins,
                coef=0.5 / n)


@functools.lru_cache(maxsize=None)
def score_errors(cid):
    """max |S32 - S64| of every pair, both products by torch on the CPU"""
    c = make_case(cid)
    out = []
    for m, n in pairs(c["views"], c["anchor"]):
        a, b = c["x"][:, m], c["x"][:, n]
        out.append(float(((a.float() @ b.float().T).double() - a.double() @ b.double().T).abs().max()))
    return tuple(out)


def reference(x, shards, anchor, T, coef, s_errs):
    """float64 on the device of x.  Returns (ref, bnd) with loss_rows [P][n], dx_loc [n][M][d] whole; colsum, dx_all, dT as
    lists, one entry per shard; dx_all_sum = the shares added up, with the summed bounds."""
    n, M, d = x.shape
    dev = x.device
    pr = pairs(M, anchor)
    r_da, r_db = roles(M, anchor)
    ct = coef / T
    x64 = x.double()
    ax = x64.abs()
    geoms = [N.geometry(hi - lo, n, d) for lo, hi in shards]
    f64 = dict(dtype=torch.float64, device=dev)
    ref = dict(loss_rows=torch.empty(len(pr), n, **f64), dx_loc=torch.zeros(n, M, d, **f64),
               colsum=[torch.empty(len(pr), n, **f64) for _ in shards], dx_all=[torch.zeros(n, M, d, **f64) for _ in shards], dT=[])
    bnd = dict(loss_rows=torch.empty(len(pr), n, **f64), dx_loc=torch.zeros(n, M, d, **f64),
               colsum=[torch.empty(len(pr), n, **f64) for _ in shards], dx_all=[torch.zeros(n, M, d, **f64) for _ in shards], dT=[])
    flush = FLUSH * (1.0 + ct)
    i_all = torch.arange(n, device=dev)
    for p, (m, nn) in enumerate(pr):
        a, b = x[:, m], x[:, nn]
        r, bd = N.reference(a, b, 0, shards, T, coef, 1, s_errs[p], keep=True)
        ref["loss_rows"][p], bnd["loss_rows"][p] = r["loss_rows"], bd["loss_rows"]
        ref["dx_loc"][:, m] += r["da"]
        S = a.double() @ b.double().T
        xm = float(torch.maximum(S.abs(), (S - 1.0).abs()).max()) / T
        del S
        G, Q = r["G"], r["P_row"] + r["P_col"]
        eps_e = 4.0 * s_errs[p] / T + 6.0 * H * xm + 2.0 * H
        eps_c = eps_e + (max(15 + -(-g["m_tiles"] // 4) for g in geoms) + len(shards) - 1) * H
        s_da, s_db = len(r_da[m]), len(r_db[nn])
        for k, ((lo, hi), g) in enumerate(zip(shards, geoms)):
            ref["colsum"][k][p], bnd["colsum"][k][p] = r["colsum"][k], bd["colsum"][k]
            ref["dx_all"][k][:, nn] += r["db"][k]
            eps_l = eps_e + (12 + -(-g["n_tiles"] // 4)) * H
            eps_w = eps_e + max(eps_l, eps_c) + 10.0 * H
            Gs, Qs = G[lo:hi], Q[lo:hi]
            ii, pos = torch.arange(hi - lo, device=dev), i_all[lo:hi]
            BW = ct * ((1.0 + EPS_P) ** 2 * (1.0 + eps_w) - 1.0) * Qs + flush
            gd = Gs[ii, pos].abs()
            BW[ii, pos] = ct * (EPS_P * gd + (1.0 + EPS_P) * (eps_w * Qs[ii, pos] + 8.0 * H * gd)) + flush
            mag = ct * Gs.abs() + BW
            bnd["dx_loc"][lo:hi, m] += (BW + (s_da * g["Cp"] + 32) * H * mag) @ ax[:, nn]
            bnd["dx_all"][k][:, nn] += (BW + (s_db * g["Rp"] + 32) * H * mag).T @ ax[lo:hi, m]
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
    return ref, bnd


GRADS = ("dx_loc", "dx_all", "dx_all_sum")


def ratios(got, ref, bnd, bf16=False):
    """largest |error| / bound per output over all shards (``got`` laid out as ``ref``; outputs it lacks are skipped).  bf16: the
    gradients were rounded once on the way out, 2^-8 |value| joins their bounds (as nce_tile_cases.ratios).  An element whose
    bound is 0 (a view without the role) must be exactly 0: it counts as 0 or inf."""
    out = {}
    for name in ("colsum", "loss_rows") + GRADS + ("dT",):
        if name not in got:
            continue
        worst = 0.0
        gs, rs, bs = (got[name], ref[name], bnd[name]) if isinstance(ref[name], list) else ([got[name]], [ref[name]], [bnd[name]])
        for g, r, b in zip(gs, rs, bs):
            if name == "dT":
                worst = max(worst, abs(float(g) - r) / b)
            elif r.numel():
                g = g.double()
                if bf16 and name in GRADS:
                    b = b + 2.0 ** -8 * g.abs()
                err = (g - r).abs()
                q = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
                worst = max(worst, float(q.max()))
        out[name] = worst
    return out


# ---- the design's arithmetic on the CPU ----
def emulate(x, shards, anchor, T, coef, mutation=None, bf16_out=False):
    """The kernels' arithmetic on the CPU, pair by pair as nce_tile_cases.emulate (float32 scores, exponentials and sums, E rounded
    to bf16 once, the off-diagonal weights a second time, the positive's weight from the float32 ediag), then ONE float32 product
    per view and role over the concatenated partner blocks, rounded once where bf16_out.  Output laid out as ``reference``.
    mutation: ("db_view", p) -- the db product of pair p lands on its m view; ("seg_keys", m) -- the second segment of view m's da
    product reads the first segment's keys; ("omit", p) -- pair p is left out of the gradients and its loss rows are 0;
    ("no_1_over_P",) -- the gradients carry coef * P; ("round_pairs",) -- every pair's product is rounded to bf16 and the rounded
    products are added in bf16, as autograd adds the bf16 gradients of a loop of two-view calls (("round_pairs", "f32_sum"): the
    rounded products are added in float32)."""
    n, M, d = x.shape
    pr = pairs(M, anchor)
    r_da, r_db = roles(M, anchor)
    kind = mutation[0] if mutation else None
    xf = x.float()
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(T, dtype=torch.float32)
    log2e = torch.tensor(1.4426950408889634, dtype=torch.float32)
    ct = torch.tensor(coef * (len(pr) if kind == "no_1_over_P" else 1), dtype=torch.float32) * inv
    out = dict(loss_rows=torch.zeros(len(pr), n), colsum=[torch.empty(len(pr), n) for _ in shards],
               dx_loc=torch.zeros(n, M, d), dx_all=[torch.zeros(n, M, d) for _ in shards], dT=[])
    W = {}
    for p, (m, nn) in enumerate(pr):
        af, bf = xf[:, m], xf[:, nn]
        st = N.emulate_pass1(x[:, m], x[:, nn], shards, T)
        c_tot = st["shards"][0]["c"]
        for s in st["shards"][1:]:
            c_tot = c_tot + s["c"]
        for k, ((lo, hi), s) in enumerate(zip(shards, st["shards"])):
            out["colsum"][k][p] = s["c"]
            i = torch.arange(hi - lo)
            pos = lo + i
            dot = (af[lo:hi] * bf[pos]).sum(1)
            ediag = torch.exp2((dot - 1.0) * inv * log2e)
            if not (kind == "omit" and mutation[1] == p):
                out["loss_rows"][p, lo:hi] = (torch.log(s["l"]) + inv - dot * inv) + (torch.log(c_tot[pos]) + inv - dot * inv)
            u, v = 1.0 / s["l"], 1.0 / c_tot
            Eb = s["E"].to(torch.bfloat16).float()
            Wp = ct * (Eb * (u[:, None] + v[None, :]))
            Wp[i, pos] = ct * (ediag * (u + v[pos]) - 2.0)
            W[p, k] = Wp.to(torch.bfloat16).float()

    def rnd(t):
        return t.to(torch.bfloat16).float()

    def product(blocks, operands):
        if kind == "round_pairs":
            acc = rnd(blocks[0] @ operands[0])
            for w, o in zip(blocks[1:], operands[1:]):
                acc = acc + rnd(w @ o)
                if len(mutation) < 2 or mutation[1] != "f32_sum":
                    acc = rnd(acc)                  # autograd adds bf16 gradients in bf16
            return acc
        return torch.cat(blocks, dim=1) @ torch.cat(operands, dim=0)

    for k, (lo, hi) in enumerate(shards):
        td = torch.zeros((), dtype=torch.float32)
        for m, segs in r_da.items():
            segs = [(p, nn) for p, nn in segs if not (kind == "omit" and mutation[1] == p)]
            if not segs:
                continue
            keys = [xf[:, nn] for _, nn in segs]
            if kind == "seg_keys" and mutation[1] == m and len(keys) > 1:
                keys[1] = keys[0]
            da = product([W[p, k] for p, _ in segs], keys)
            td = td + (xf[lo:hi, m] * da).sum()
            out["dx_loc"][lo:hi, m] = rnd(da) if bf16_out else da
        out["dT"].append(-float(td * inv))
        for nn, segs in r_db.items():
            segs = [(p, m) for p, m in segs if not (kind == "omit" and mutation[1] == p)]
            moved = [(p, m) for p, m in segs if kind == "db_view" and mutation[1] == p]
            segs = [s for s in segs if s not in moved]
            if segs:
                db = product([W[p, k].T for p, _ in segs], [xf[lo:hi, m] for _, m in segs])
                out["dx_all"][k][:, nn] = rnd(db) if bf16_out else db
            for p, m in moved:
                out["dx_all"][k][:, m] += W[p, k].T @ xf[lo:hi, m]
    return out
