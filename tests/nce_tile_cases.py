"""Case tables, inputs, float64 references, derived bounds and a CPU emulation shared by tests/test_nce_tile_cpu.py and
tests/test_nce_tile_gpu.py: the tile-GEMM InfoNCE (aecf_nce_gemm.hip behind aecf_nce_fwd_bwd[_dt] with the rows x cols workspace
and aecf_nce_sym_pass1 / _loss / _grads[_dt]) at its tile, patch, split and ragged edges.  Nothing here touches a GPU; every
function works on the device of the tensors it is given.

One problem, two uses.  Rows a [R, d] against keys b [C, d], the positive of row i at column off + i, x = a.b / T:
  sym = 0 (one direction)   loss_i = lse_row_i - x_ii,                G = P_row - [j = off + i]
  sym = 1 (symmetric)       loss_i = lse_row_i + lse_col_i - 2 x_ii,  G = P_row + P_col - 2 [j = off + i]
  da = ct G b,  db = ct G^T a,  dT = -(1/T) sum_i a_i . da_i,  ct = coef / T,  P_row / P_col the softmax along a row / down a
  column.  In the symmetric use the rows are dealt over shards (emulated ranks): the column log-sum-exps are global, and a shard
  owns its rows of loss and da, its SHARE of db (ct G[shard]^T a[shard]) and of dT, and its column sums
  sum_{i in shard} exp((s_ij - 1) / T) -- the one thing ranks exchange.

What the kernels round (h = 2^-24, half a float32 ulp; EPS_P = 2^-8, half a bf16 ulp; every count below is an upper bound read
off the code, first order in h, and the bounds carry no further factor):
  E32_ij = exp2(acc scale2 - shift2), scale2 = shift2 = (1/T) log2 e.
      acc against the exact score: 4 s_err, s_err = max |S32 - S64| of torch's CPU products, measured on the reference (the
      factor 4: the MFMA sums in another order) -- as in tests/nce_stream_cases.py.  scale2: the quotient 1/T within one ulp
      (2 h), the constant log2 e as a float (h), their product (h): 4 h of the exponent.  The exponent itself: one rounding when
      the compiler fuses acc scale2 - shift2, two when it does not: 2 h.  v_exp_f32: one ulp, 2 h of the value.  With
      xm = max(|S|, |S - 1|) / T (the largest exponent, on the reference):
          eps_e = 4 s_err / T + 6 h xm + 2 h                                    relative error of E32 (never subnormal: T >= 0.025)
      ediag_i (the positive's exponential, from a float32 dot of its own): the dot 4 s_err likewise; dot - 1, times 1/T (2 h + h),
      times log2 e (h + h): 6 h xm; the exponential 2 h -- the same eps_e.
  l_i = sum_j E32_ij (before E is rounded), additions an element passes through: 4 (the lane's column tiles) + 1 (e01 + e23) + 1
      (the two halves) + 2 (lane groups) + 2 (the block's 4 waves) + ceil(n_tiles / 4) + 2 (nce_sums_kernel):
          eps_l = eps_e + (12 + ceil(n_tiles / 4)) h
  c_j = sum_i E32_ij: 8 (row tiles of the lane) + 4 (16 lanes) + 1 (2 waves) + ceil(m_tiles / 4) + 2:
          eps_cs = eps_e + (15 + ceil(m_tiles / 4)) h                           a shard's own column sums (an output of pass 1)
          eps_c  = eps_e + (max over shards of the count + shards - 1) h        their float32 sum over shards (the all-reduce)
  loss_i = logf(l_i) + 1/T - dot/T [+ logf(c_pos) + 1/T - dot/T].  Per direction: the sum's relative error (eps_l or eps_c), the
      dot (4 s_err / T), 1/T within an ulp against |1 - dot| <= T xm (2 h xm), logf within an ulp (2 h) and three float32
      operations (3 h) on values no larger than M = xm + 1/T + ln C; the symmetric form adds the two directions: 2 h M more.
          |d loss_i| <= eps_l + 4 s_err / T + 2 h xm + 5 h M                                                        (sym = 0)
          |d loss_i| <= eps_l + eps_c + 2 (4 s_err / T + 2 h xm) + 12 h M                                           (sym = 1)
  W_ij = bf16(ct (bf16(E32_ij) (u_i + v_j))), u = 1/l, v = 1/c (0 when sym = 0): the float32 factor next to bf16(E) is off by
          eps_w = eps_e + max(eps_l, eps_c) + 2 h + 8 h
      (E32; the sums; the quotients 1/l, 1/c within an ulp; u + v, the two products, and ct = float(coef) (1/T) [upstream]: h, 2 h,
      h, h), and two bf16 roundings stand around it:
          |d W_ij| <= ct ((1 + EPS_P)^2 (1 + eps_w) - 1) Q_ij + f,      Q = P_row + sym P_col,  f = 2^-126 (1 + ct)
      (f: a product below the smallest normal float32, before or after the factor ct, may flush to zero).
  W_ii = bf16(ct (ediag_i (u_i + v_pos) - npos)), npos = 1 + sym: ONE bf16 rounding, of the small difference G_ii:
          |d W_ii| <= ct (EPS_P |G_ii| + (1 + EPS_P) (eps_w Q_ii + 8 h |G_ii|)) + f
  da = W b, db = W^T a: bf16 x bf16 products are exact in float32; a float32 sum of n terms in ANY order is within n h of the sum
      of their magnitudes, n <= Cp + 32 for da (the padded keys, the slab sum over <= 32 splits), Rp + 32 for db:
          |d da| <= (BW + (Cp + 32) h (ct |G| + BW)) |b|,     |d db| <= (BW + (Rp + 32) h (ct |G| + BW))^T |a|,    BW = the |d W| above
  dT = -(sum of per-block partials of acc . a) / T: the float32 accumulators of da before any store, 128 fmaf per lane, 6 + 3
      reduction steps in the block, ceil(parts / 256) + 8 in nce_dtemp_kernel (parts = splits m_tiles d_tiles), the quotient:
          |d dT| <= (1/T) (sum |a| bound_da + (145 + ceil(parts / 256)) h sum |a| (|da| + bound_da)) + 3 h |dT|
  column sums (pass 1's output):  |d cs_j| <= eps_cs cs_j
Other output forms: a bf16 gradient adds 2^-8 |value| (one rounding of the float32 sum); an upstream scalar multiplies ct, so
reference and bounds are taken at coef * upstream.

Which output carries the teeth.  A twin (below) holds half of a softmax, so a key or row lost or counted twice at a boundary
moves the loss of the twin's row by about ln 2, thousands of bounds, and da / db by more than a hundred (``signal`` prints
|value| / bound).  dT's bound is a triangle-inequality sum over rows x d elements: a wrong sign or factor shows there, a small
error does not.

Twins.  One direction: a column twin k[j] = k[off + r] on every boundary column the geometry names that is no positive's column
(63, 64, 255, 256, both sides of every da-split boundary, cols - 1, the first column of the last column tile, 2047, 2048), each
with a row r of its own, the row edges first (rows - 1, 0, 127, 128, 255, 256, 1023, 1024).  Symmetric: row twins a[r'] = a[r],
b[r'] = b[r] with r' on rows 127, 128, 255, 256, 1023, 1024, every shard's first and last row, n - 1 and the boundary columns
above (row r' is also column r'), r a row of its own off every boundary.  Rows r and r' then each hold half of row r's, row
r''s, column r's and column r''s softmax.  Unlike nce_stream_cases.make_case the positive's noise is taken orthogonal to the
query, so the cosine is 0.8 in every row (before the rounding to bf16) and no twin of a narrow case (d = 64) falls under a
quarter share by the draw.

The ediag mutation (positive's weight from bf16(E_ii) instead of the float32 ediag_i) errs by up to ct EPS_P Q_ii on W_ii, against
a bound of ct EPS_P (|G_ii| |b_pos| + 2 sum_j |G_ij| |b_j|) on da: about (1 + sym) / (3 |G_ii|) bounds at best.  It shows where the
positive dominates its row and column (Q_ii -> 1 + sym, G_ii -> 0): on a twin's row Q_ii = |G_ii| and it cannot show, and at
T = 0.07 and cosine 0.8 a row without a twin keeps |G_ii| under 3 % only among a few hundred keys (D5, S2, S3: 20 to 30 bounds in
the emulation; D4 and S4, thousands of keys: 4 to 9).  The CPU test therefore judges it on the rows without twins of D5, S2, S3.

Symmetric twins and the gradients.  Rows r and r' being one vector, G_rr = G_r'r' = -1 and G_rr' = G_r'r = +1 at low T: their
contributions to da_r and db_r cancel.  The loss (about ln 2 per lost or doubled key, thousands of bounds) and a shard's share of
db (when r and r' lie in different shards) are the detectors there; one-direction twins show in db as well."""
import functools
import math

import torch

from tests.nce_stream_cases import EPS_P, FLUSH, _unit, used_temperature  # noqa: F401  (used_temperature: for the tests)

H = 2.0 ** -24
TEMPS = (0.07, 0.025)
MIN_T = 0.025
ROW_EDGES = (127, 128, 255, 256, 1023, 1024)


# ---- the geometry of aecf_nce_gemm.hip, restated ----
def up256(v):
    return (v + 255) // 256 * 256


def da_splits(Rp, Cp, d):
    """K splits of da = W b (aecf_nce_gemm.hip: da_splits)"""
    items = (Rp // 256) * ((d + 255) // 256)
    s = (768 + items - 1) // items
    cap = Cp // 64 // 8
    s = min(s, cap)
    if 5 <= s <= 12 and cap >= 8:
        s = 8
    return max(1, min(s, 32))


def geometry(rows, cols, d):
    """everything the launchers derive from a shape: padded sizes, tiles, MAP_2D patches of the logits pass, the K split of da"""
    Rp, Cp = up256(rows), up256(cols)
    splits = da_splits(Rp, Cp, d)
    k_steps = Cp // 64
    per = -(-k_steps // splits)
    live = -(-k_steps // per)
    m_tiles, n_tiles, d_tiles = Rp // 256, Cp // 256, -(-d // 256)
    m_patches, n_patches = -(-m_tiles // 4), -(-n_tiles // 8)
    return dict(Rp=Rp, Cp=Cp, splits=splits, per=per, live=live, last=k_steps - (live - 1) * per,
                map="SPLITX" if splits == 8 else "UNITS", da_units=m_tiles * splits,
                m_tiles=m_tiles, n_tiles=n_tiles, d_tiles=d_tiles, d_last=d - 256 * (d_tiles - 1),
                m_patches=m_patches, n_patches=n_patches, logits_blocks=-(-(m_patches * n_patches) // 8) * 8 * 32,
                logits_steps=d // 64)


def workspace_bytes_py(rows, cols, d):
    """carve() + 256: E, the two partial arrays, l, u, v, ediag, c_local, the da slabs -- each rounded up to 256 bytes"""
    g = geometry(rows, cols, d)
    Rp, Cp = g["Rp"], g["Cp"]
    parts = [Rp * Cp * 2, g["n_tiles"] * Rp * 4, g["m_tiles"] * Cp * 4, Rp * 4, Rp * 4, Cp * 4, Rp * 4, Cp * 4,
             g["splits"] * rows * d * 4]
    return sum(up256(p) for p in parts) + 256


# id: ((rows, cols, off, d), the geometry claimed, what it puts on an edge)
DIRECTION = {
    "D1": ((1, 1, 0, 64), dict(splits=1, live=1, last=4, map="UNITS", m_tiles=1, n_tiles=1, d_tiles=1, m_patches=1, n_patches=1,
                               logits_steps=1), "one row, one key; one logits K-step"),
    "D2": ((33, 6700, 6667, 128), dict(splits=13, live=12, last=9, map="UNITS", m_tiles=1, n_tiles=27, d_tiles=1, m_patches=1,
                                       n_patches=4, logits_steps=2), "off + rows == cols; 13 splits, 12 live"),
    "D3": ((65, 10900, 700, 64), dict(splits=21, live=20, last=1, map="UNITS", m_tiles=1, n_tiles=43, d_tiles=1, m_patches=1,
                                      n_patches=6, logits_steps=1), "21 splits, 20 live; last live split has 1 K-step"),
    "D4": ((300, 4300, 2000, 192), dict(splits=8, live=8, last=5, per=9, map="SPLITX", m_tiles=2, n_tiles=17, d_tiles=1,
                                        d_last=192, m_patches=1, n_patches=3, logits_steps=3),
           "8 splits, MAP_SPLITX; last split 5 of 9 steps; partial d tile"),
    "D5": ((257, 513, 256, 320), dict(splits=1, live=1, last=12, map="UNITS", m_tiles=2, n_tiles=3, d_tiles=2, d_last=64,
                                      m_patches=1, n_patches=1, logits_steps=5),
           "second row tile holds one row; third column tile holds one column; 2 d tiles, the second 64 wide"),
    "D6": ((1025, 2100, 1000, 1024), dict(splits=4, live=4, last=9, map="UNITS", m_tiles=5, n_tiles=9, d_tiles=4, d_last=256,
                                          m_patches=2, n_patches=2, logits_steps=16),
           "5 row tiles (second m patch); 9 column tiles (second n patch); 4 splits"),
}

# id: ((n, d), shard bounds, the geometry claimed per shard, note)
SYMMETRIC = {
    "S1": ((1, 64), [(0, 1)], [dict(splits=1, m_tiles=1, n_tiles=1, logits_steps=1)], "one row"),
    "S2": ((257, 128), [(0, 256), (256, 257)], [dict(splits=1, m_tiles=1, n_tiles=2), dict(splits=1, m_tiles=1, n_tiles=2)],
           "one-row shard at an offset"),
    "S3": ((300, 192), [(0, 300)], [dict(splits=1, live=1, m_tiles=2, n_tiles=2, d_last=192, logits_steps=3)],
           "splits == 1: the da GEMM stores its output itself"),
    "S4": ((2305, 256), [(0, 65), (65, 1090), (1090, 2305)],
           [dict(splits=5, live=5, last=8, map="UNITS", da_units=5, m_tiles=1, n_tiles=10, n_patches=2),
            dict(splits=5, live=5, last=8, map="UNITS", da_units=25, m_tiles=5, n_tiles=10, m_patches=2, n_patches=2),
            dict(splits=5, live=5, last=8, map="UNITS", da_units=25, m_tiles=5, n_tiles=10, m_patches=2, n_patches=2)],
           "10 column tiles; 1025- and 1215-row shards with 5 row tiles"),
    "S5": ((4300, 192), [(0, 300), (300, 4300)],
           [dict(splits=8, live=8, last=5, map="SPLITX", m_tiles=2, n_tiles=17), dict(splits=8, live=8, last=5, map="SPLITX", m_tiles=16,
                                                                                     n_tiles=17, m_patches=4, n_patches=3)],
           "MAP_SPLITX in both shards; 16 row tiles"),
    "S6": ((6700, 128), [(0, 200), (200, 6700)],
           [dict(splits=13, live=12, last=9, map="UNITS", da_units=13, m_tiles=1, n_tiles=27),
            dict(splits=13, live=12, last=9, map="UNITS", da_units=338, m_tiles=26, n_tiles=27, m_patches=7, n_patches=4)],
           "13/12 splits in both shards; 26 row tiles; 338 da units, no multiple of 8"),
}
SMALL_DIRECTION = ("D1", "D2", "D3", "D4", "D5")       # the cases the CPU suite emulates (the rest: geometry only)
SMALL_SYMMETRIC = ("S1", "S2", "S3", "S4")


def boundary_columns(cols, geoms):
    """the columns the geometry names, the end of the key range first: cols - 1, the first column of the last column tile, both
    sides of every da-split boundary of every shard's split, 2048 / 2047, 256 / 255, 64 / 63"""
    wanted = [cols - 1, up256(cols) - 256]
    for g in geoms:
        for s in range(g["live"] - 1, 0, -1):
            wanted += [g["per"] * 64 * s, g["per"] * 64 * s - 1]
    wanted += [2048, 2047, 256, 255, 64, 63]
    out = []
    for j in wanted:
        if 0 <= j < cols and j not in out:
            out.append(j)
    return out


def direction_twins(rows, cols, off, d):
    """[(column j, row r_j)]: the boundary columns that are no positive's column, each with a row of its own (row edges first)"""
    columns = [j for j in boundary_columns(cols, [geometry(rows, cols, d)]) if not (off <= j < off + rows)]
    order = []
    for r in (rows - 1, 0) + ROW_EDGES + tuple(range(rows)):
        if 0 <= r < rows and r not in order:
            order.append(r)
    return list(zip(columns, order))


def symmetric_twins(n, d, shards):
    """[(row r', row r)]: r' on the row edges, every shard's first and last row, n - 1 and the boundary columns; r off all of them,
    spread over the rows, distinct for distinct twins.  As many as the free rows allow."""
    spots = set(r for r in ROW_EDGES + (n - 1,) if 0 <= r < n)
    for lo, hi in shards:
        spots |= {lo, hi - 1}
    spots |= set(boundary_columns(n, [geometry(hi - lo, n, d) for lo, hi in shards]))
    spots = sorted(spots)
    free = [r for r in range(n) if r not in set(spots)]
    spots = spots[-len(free):] if free else []
    return [(rp, free[(k * len(free)) // len(spots)]) for k, rp in enumerate(spots)]


def _positives(q, g):
    """unit rows at cosine 0.8 to the rows of q: 0.8 q + 0.6 (unit noise orthogonal to q)"""
    z = torch.randn(q.shape, generator=g)
    z = _unit(z - (z * q).sum(1, keepdim=True) * q)
    return 0.8 * q + 0.6 * z


@functools.lru_cache(maxsize=None)
def make_direction(cid):
    """bf16 unit rows q [rows, d], k [cols, d] (CPU), the offset and the twins [(column, row)] of a one-direction case"""
    (rows, cols, off, d), _, _ = DIRECTION[cid]
    g = torch.Generator().manual_seed(5000 + list(DIRECTION).index(cid))
    q = _unit(torch.randn(rows, d, generator=g))
    k = _unit(torch.randn(cols, d, generator=g))
    k[off:off + rows] = _positives(q, g)
    q, k = q.to(torch.bfloat16), k.to(torch.bfloat16)
    twins = direction_twins(rows, cols, off, d)
    for j, r in twins:
        k[j] = k[off + r]
    return dict(a=q, b=k, off=off, shards=[(0, rows)], sym=0, coef=1.0 / cols, twins=twins)


def make_rows(n, d, shards, seed):
    """bf16 unit rows a, b [n, d] (CPU) with b_i at cosine 0.8 to a_i, and the row twins [(row r', row r)] of these shards"""
    g = torch.Generator().manual_seed(seed)
    a = _unit(torch.randn(n, d, generator=g))
    b = _positives(a, g)
    a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
    twins = symmetric_twins(n, d, shards)
    for rp, r in twins:
        a[rp], b[rp] = a[r], b[r]
    return a, b, twins


@functools.lru_cache(maxsize=None)
def make_symmetric(cid):
    """the rows, the shard bounds and the twins of a symmetric case"""
    (n, d), shards, _, _ = SYMMETRIC[cid]
    a, b, twins = make_rows(n, d, shards, 5100 + list(SYMMETRIC).index(cid))
    return dict(a=a, b=b, off=0, shards=list(shards), sym=1, coef=0.5 / n, twins=twins)


def make_case(cid):
    return make_direction(cid) if cid in DIRECTION else make_symmetric(cid)


@functools.lru_cache(maxsize=None)
def score_error(cid):
    """max |S32 - S64| of a case, both products by torch on the CPU"""
    c = make_case(cid)
    s32 = c["a"].float() @ c["b"].float().T
    return float((s32.double() - c["a"].double() @ c["b"].double().T).abs().max())


# ---- float64 reference and the bounds of the module docstring ----
def reference(a, b, off, shards, T, coef, sym, s_err, keep=False):
    """float64 on the device of a and b.  a [R, d]: every row of the problem (sym: R == C, off == 0), ``shards`` its row ranges.
    Returns (ref, bnd): loss_rows, da [R ...] whole; db, dT, colsum as lists, one entry per shard (db: the shard's share);
    db_sum = the shares added up, with the summed bounds.  keep: also P_row, P_col, G (for the CPU tests)."""
    a64, b64 = a.double(), b.double()
    R, d = a64.shape
    C = b64.shape[0]
    dev = a.device
    ct = coef / T
    npos = 1.0 + sym
    i = torch.arange(R, device=dev)
    pos = off + i
    S = a64 @ b64.T
    xm = float(torch.maximum(S.abs(), (S - 1.0).abs()).max()) / T
    x = S / T
    E = torch.exp((S - 1.0) / T)
    del S
    lse_row = torch.logsumexp(x, dim=1)
    xii = x[i, pos]
    P_row = torch.exp(x - lse_row[:, None])
    loss = lse_row - xii
    Q = P_row.clone()
    P_col = None
    if sym:
        lse_col = torch.logsumexp(x, dim=0)
        P_col = torch.exp(x - lse_col[None, :])
        loss = loss + lse_col[pos] - xii
        Q += P_col
    del x
    G = Q.clone()
    G[i, pos] -= npos
    aa, ab = a64.abs(), b64.abs()
    da = ct * (G @ b64)

    geoms = [geometry(hi - lo, C, d) for lo, hi in shards]
    eps_e = 4.0 * s_err / T + 6.0 * H * xm + 2.0 * H
    eps_c = eps_e + (max(15 + -(-g["m_tiles"] // 4) for g in geoms) + len(shards) - 1) * H if sym else 0.0
    M = xm + 1.0 / T + math.log(C)
    flush = FLUSH * (1.0 + ct)
    ref = dict(loss_rows=loss, da=da, db=[], dT=[], colsum=[])
    bnd = dict(loss_rows=torch.empty_like(loss), da=torch.empty_like(da), db=[], dT=[], colsum=[])
    for (lo, hi), g in zip(shards, geoms):
        eps_l = eps_e + (12 + -(-g["n_tiles"] // 4)) * H
        eps_cs = eps_e + (15 + -(-g["m_tiles"] // 4)) * H
        eps_w = eps_e + max(eps_l, eps_c) + 10.0 * H
        if sym:
            bnd["loss_rows"][lo:hi] = eps_l + eps_c + 2.0 * (4.0 * s_err / T + 2.0 * H * xm) + 12.0 * H * M
        else:
            bnd["loss_rows"][lo:hi] = eps_l + 4.0 * s_err / T + 2.0 * H * xm + 5.0 * H * M
        Gs, Qs = G[lo:hi], Q[lo:hi]
        ii = torch.arange(hi - lo, device=dev)
        BW = ct * ((1.0 + EPS_P) ** 2 * (1.0 + eps_w) - 1.0) * Qs + flush
        gd = Gs[ii, pos[lo:hi]].abs()
        BW[ii, pos[lo:hi]] = ct * (EPS_P * gd + (1.0 + EPS_P) * (eps_w * Qs[ii, pos[lo:hi]] + 8.0 * H * gd)) + flush
        mag = ct * Gs.abs() + BW
        b_da = (BW + (g["Cp"] + 32) * H * mag) @ ab
        b_db = (BW + (g["Rp"] + 32) * H * mag).T @ aa[lo:hi]
        del mag, BW
        bnd["da"][lo:hi] = b_da
        ref["db"].append(ct * (Gs.T @ a64[lo:hi]))
        bnd["db"].append(b_db)
        dT = -(1.0 / T) * float((a64[lo:hi] * da[lo:hi]).sum())
        depth = 145 + -(-(g["splits"] * g["m_tiles"] * g["d_tiles"]) // 256)
        ref["dT"].append(dT)
        bnd["dT"].append((float((aa[lo:hi] * b_da).sum()) + depth * H * float((aa[lo:hi] * (da[lo:hi].abs() + b_da)).sum())) / T
                         + 3.0 * H * abs(dT))
        cs = E[lo:hi].sum(0)
        ref["colsum"].append(cs)
        bnd["colsum"].append(eps_cs * cs)
    ref["db_sum"], bnd["db_sum"] = sum(ref["db"]), sum(bnd["db"])
    if keep:
        ref.update(P_row=P_row, P_col=P_col, G=G)
    return ref, bnd


def ratios(got, ref, bnd, bf16=False):
    """largest |error| / bound per output over all shards (``got`` laid out as ``ref``; outputs it lacks are skipped).  bf16: the
    gradients were rounded once more on the way out, 2^-8 |value| joins their bounds."""
    out = {}
    for name in ("colsum", "loss_rows", "da", "db", "db_sum", "dT"):
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
                worst = max(worst, float(((g - r).abs() / b).max()))
        out[name] = worst
    return out


def signal(ref, bnd):
    """largest |value| / bound per output: how many bounds the reference itself is worth -- what a check can see at all"""
    nothing = {name: [v * 0 for v in ref[name]] if isinstance(ref[name], list) else ref[name] * 0 for name in bnd}
    return ratios(nothing, ref, bnd)


# ---- the design's arithmetic on the CPU ----
def emulate_pass1(a, b, shards, T):
    """float32 E (before its rounding to bf16), row sums and column sums of every shard"""
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(T, dtype=torch.float32)
    scale2 = inv * torch.tensor(1.4426950408889634, dtype=torch.float32)
    af, bf = a.float(), b.float()
    state = []
    for lo, hi in shards:
        E = torch.exp2((af[lo:hi] @ bf.T) * scale2 - scale2)
        state.append(dict(E=E, l=E.sum(1), c=E.sum(0)))
    return dict(inv=inv, scale2=scale2, shards=state)


def emulate(a, b, off, shards, T, coef, sym, mutation=None, grads=True, state=None, upstream=1.0):
    """The kernels' arithmetic on the CPU: float32 scores, exponentials and sums, E rounded to bf16 once, the off-diagonal
    weights a second time, the positive's weight from the float32 ediag.  Output laid out as ``reference`` (no db_sum).
    mutation: ("col", j, times) -- key j enters the row sums 0 times or twice; ("row", i, times) -- row i (of a) enters the column
    sums 0 times or twice; ("ediag",) -- the positive's weight is formed from the bf16 E.  grads = False: loss rows and column
    sums only (what the two sum mutations are judged on).  state: emulate_pass1 of the same inputs, to share it."""
    st = state or emulate_pass1(a, b, shards, T)
    inv, scale2 = st["inv"], st["scale2"]
    af, bf = a.float(), b.float()
    kind = mutation[0] if mutation else None
    ls, cs = [], []
    for (lo, hi), s in zip(shards, st["shards"]):
        l, c = s["l"], s["c"]
        if kind == "col":
            l = l + (mutation[2] - 1) * s["E"][:, mutation[1]]
        if kind == "row" and lo <= mutation[1] < hi:
            c = c + (mutation[2] - 1) * s["E"][mutation[1] - lo]
        ls.append(l)
        cs.append(c)
    c_tot = cs[0]
    for c in cs[1:]:
        c_tot = c_tot + c
    ct = torch.tensor(coef, dtype=torch.float32) * inv * torch.tensor(upstream, dtype=torch.float32)
    npos = 1.0 + sym
    out = dict(loss_rows=torch.empty(a.shape[0]), colsum=cs)
    if grads:
        out.update(da=torch.empty(a.shape, dtype=torch.float32), db=[], dT=[])
    for (lo, hi), s, l in zip(shards, st["shards"], ls):
        rows = hi - lo
        i = torch.arange(rows)
        pos = off + lo + i
        dot = (af[lo:hi] * bf[pos]).sum(1)
        ediag = torch.exp2((dot - 1.0) * inv * torch.tensor(1.4426950408889634, dtype=torch.float32))
        loss = torch.log(l) + inv - dot * inv
        if sym:
            loss = loss + (torch.log(c_tot[pos]) + inv - dot * inv)
        out["loss_rows"][lo:hi] = loss
        if not grads:
            continue
        u = 1.0 / l
        v = 1.0 / c_tot if sym else torch.zeros_like(c_tot)
        Eb = s["E"].to(torch.bfloat16).float()
        W = ct * (Eb * (u[:, None] + v[None, :]))
        W[i, pos] = ct * ((Eb[i, pos] if kind == "ediag" else ediag) * (u + v[pos]) - npos)
        W = W.to(torch.bfloat16).float()
        da = W @ bf
        out["da"][lo:hi] = da
        out["db"].append(W.T @ af[lo:hi])
        out["dT"].append(-float((af[lo:hi] * da).sum() * inv))
    return out
