"""Case table, inputs, float64 reference, derived bounds and a CPU emulation shared by tests/test_sig_tile_cpu.py and
tests/test_sig_tile_gpu.py: the tile-GEMM sigmoid (SigLIP) loss (aecf_sig_pass1 / aecf_sig_grads: the EPI_SIG epilogue,
sig_rows_kernel, sig_dbias_kernel and the EPI_OUT_S / EPI_OUT_TD_S gradient products of aecf_nce_gemm.hip) at its tile, patch,
split and ragged edges.  Nothing here touches a GPU; every function works on the device of the tensors it is given.

The problem.  Rows a [R, d] against keys b [C, d], the positive of row i at column off + i, Tc = max(T, min_temperature):
  l_ij = a_i.b_j / Tc + bias,  y_ij = +1 at j = off + i, else -1,  z_ij = -y_ij l_ij
  loss_i = sum_j softplus(z_ij),  g_ij = -y_ij sigmoid(z_ij) = sigmoid(l_ij) - [j = off + i],  dbias = sum_ij g_ij (what
  aecf_sig_pass1 leaves: no coef in it),  da = ct g b,  db = ct g^T a,  dT = -(1/Tc) sum_i a_i.da_i,  ct = coef upstream / Tc.
A row shard [lo, hi) is the same problem with off = lo: loss rows and da are its own, db, dbias and dT its shares.

What the kernels round (h = 2^-24, half a float32 ulp; EPS_P = 2^-8, half a bf16 ulp; every count is an upper bound read off
aecf_nce_gemm.hip, first order in h; the bounds carry no further factor).  m = |g| = sigmoid(z), sp = softplus(z) per element.
  n = acc s2 + b2 (line 578), the logit in units of ln 2.  acc against the exact score: 4 s_err, s_err = max |S32 - S64| of
      torch's CPU products measured on the reference (the factor 4: the MFMA sums in another order), as in nce_tile_cases.
      s2 = (1/Tc) log2 e (line 553): the quotient within one ulp (2 h), the constant as a float (h), the product (h): 4 h of
      |S| / Tc.  b2 = bias log2 e: the constant and the product, 2 h of |bias|.  The packed fma: one rounding, two if the compiler
      does not fuse: 2 h of |S| / Tc + |bias|.  In natural units
          dl = 4 s_err / Tc + 6 h |S| / Tc + 4 h |bias|
  sig_terms (lines 244-254), for the positive at -n (line 582):  u = v_exp(min(n, 126)) within one ulp (2 h), t = 1 + u (h),
      r = v_rcp(t) within one ulp (2 h), sigmoid = u r (h).  d sigmoid / dl = m (1 - m), and u's own error passes the same way:
          e_g = m ((1 - m) (dl + 2 h) + 4 h) + f                      f = 2^-126: u below the smallest normal may flush
      softplus = ln 2 (log2 t + (n - min(n, 126))) + corr: d softplus / dl = m (also past the clamp, where m = 1); v_log within one
      ulp (2 h), the sum inside lg2 (h), the constant ln 2 as a float (h), and corr = (u - (t - 1)) r -- which hands back what
      t = 1 + u dropped -- with its own r and product (3 h |corr|, |corr| <= min(u, h) <= sp) and, past u = 2^24 where t - 1
      rounds too, the dropped ln(1 + 1 / u) <= h <= h sp / 16: 4 h sp for corr.
          e_sp = m (dl + 2 h) + 8 h sp + f
  loss_i: additions an element passes through -- the packed adds over the lane's 4 x 2 x 2 elements (8 per component of sl and sc,
      line 592), sl[0] + sl[1] and sc[0] + sc[1] (1), the fma that joins them (1, line 598), reduce_lg (2), the four wn waves
      (2, line 615), sig_rows_kernel (ceil(n_tiles / 4) + 2, lines 1413-1421); every partial sum is below sum_j sp:
          |d loss_i| <= sum_j e_sp + (16 + ceil(n_tiles / 4)) h sum_j sp
  gsum_i = sum_j g (float32, before the rounding to bf16): 8 + 1 + 2 + 2 + ceil(n_tiles / 4) + 2 additions; dbias
      (sig_dbias_kernel, lines 1430-1437): ceil(rows / 256) additions, then the tree of 8:
          |d dbias| <= sum_ij e_g + (23 + ceil(n_tiles / 4) + ceil(rows / 256)) h sum_ij m
  g is rounded ONCE to bf16 (line 596), unscaled:
          BW = e_g + EPS_P (m + e_g)
  da = osc (gb b), db = osc (gb^T a): bf16 x bf16 products are exact in float32; a float32 sum of n terms in any order is within
      n h of the sum of their magnitudes, n <= Cp + 32 for da (the padded keys, the slab sum over <= 32 splits, line 1395),
      Rp + 32 for db; osc = float(coef) (1/Tc) [upstream] (lines 497-498: h, 2 h, h, h) times the accumulator (h, line 502): 6 h.
          |d da| <= ct (BW + (Cp + 38) h (m + BW)) |b| + f (1 + ct),   |d db| <= ct (BW + (Rp + 38) h (m + BW))^T |a| + f (1 + ct)
  dT = -(sum of per-block partials of acc . a) / Tc (lines 522-549, nce_dtemp_kernel): the scaled float32 accumulators of da
      before any store, 128 fmaf per lane, 6 + 3 reduction steps in the block, ceil(parts / 256) + 8 in nce_dtemp_kernel
      (parts = splits m_tiles d_tiles), the quotient (3 h).  The partial sums are per K split, so they are bounded by the
      magnitude sum A = ct (m + BW) |b|, not by |da|:
          |d dT| <= (1/Tc) (sum |a| bound_da + (145 + ceil(parts / 256)) h sum |a| A) + 3 h |dT|
Other output forms: a bf16 gradient adds 2^-8 |value| (one rounding of the float32 sum); an upstream scalar multiplies ct, so
reference and bounds are taken at coef * upstream.  The loss rows and dbias know neither coef nor upstream.

Which output carries the teeth.  A twin (below) is a negative with the positive's logit.  At (T, bias) = (0.1, -10) it holds
g = sigmoid(-2) = 0.12 in a row whose sum of |g| is about 1.1: some twenty bf16 roundings of the row in da and db, and
softplus(-2) = 0.127 in a loss row bounded at a few 1e-6: a key lost or counted twice moves the loss row by thousands of bounds.
At (0.07, -5) the twin's g is 0.998 but the negatives of a row sum to several (d = 128 and wider) or tens (d = 64, 10900 keys)
of |g|: da sees the weakest twin at 7 to 41 bounds, at 1.8 in G7; the loss row (softplus(6.4) against 1e-3 or less) carries
thousands and the twin's own row of db (the one large g of its column) 24 to 230.  dT's bound is a triangle-inequality sum over
rows x d elements: a wrong sign or factor shows there, a small error does not.  ``signal`` prints the twin's contribution over the
bound per output.

Twins.  A column twin b[j] = b[off + r] on every boundary column the geometry names that is no positive's column
(nce_tile_cases.boundary_columns: cols - 1, the first column of the last column tile, both sides of every da-split boundary,
2047 / 2048, 255 / 256, 63 / 64), each with a row r of its own, the row edges first (rows - 1, 0, 127, 128, 255, 256, 1023,
1024), so a lost row shows in that column's db.  The positive's noise is orthogonal to the query: cosine 0.8 in every row.

Mutations (``emulate``) and where each is judged (tests/test_sig_tile_cpu.py asserts 2 bounds on at least one output):
  drop / twice     a twin column lost from, or counted twice in, its row: every case with a twin (G1 has no second key).
  padcol           the padded column ``cols`` (the copy re-reads key cols - 1) counted as valid: every case with cols % 256 != 0.
  padrow           the padded row ``rows`` (re-reads row rows - 1, its positive at off + rows where that exists) counted in db
                   and dbias: every case with rows % 256 != 0.
  shift            the positive taken at off + i + 1: every case.
  plain            one band tile run through the plain path, its positives treated as negatives: every case.
  dbias_bf16       dbias summed from the bf16 g.  The roundings of a sum of N comparable terms grow like sqrt(N) EPS_P against a
                   bound of N (dl + 30 h).  At (0.1, -10) the positives carry the sum (|g| = 0.88 each, all at cosine 0.8: their
                   roundings add up with one sign) and the mutation stands out in every case; at (0.07, -5) the positives hold
                   1.6e-3 each and hundreds or thousands of negatives of every size carry it: no case with a second key reaches 2
                   bounds there (0.1 to 1.05 in the emulation), so the mutation is judged at (0.1, -10) only.
The block-uniform ``special`` predicate: G3, G6, G7 and G9 have ONE ragged row tile, so every tile of theirs is special (as G1's
single tile is); the plain path is reached by the cases with a full row tile -- G2, G4, G5, G8, G10, G11."""
import functools
import math

import torch

from tests.nce_stream_cases import EPS_P, FLUSH, _unit, used_temperature  # noqa: F401  (used_temperature: for the tests)
from tests.nce_tile_cases import _positives, boundary_columns, da_splits, direction_twins, geometry, up256  # noqa: F401

H = 2.0 ** -24
PARAMS = ((0.1, -10.0), (0.07, -5.0))           # (T, bias): the library's defaults, and a pair with large negatives
MIN_T = 1e-3
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453


# ---- the geometry of the sigmoid form, restated ----
def workspace_bytes_py(rows, cols, d):
    """sig_carve() + 256: g, sp_part, sg_part, gsum, tdot_part [32][16][m_tiles], the da slabs -- each rounded up to 256 bytes"""
    g = geometry(rows, cols, d)
    Rp, Cp = g["Rp"], g["Cp"]
    parts = [Rp * Cp * 2, g["n_tiles"] * Rp * 4, g["n_tiles"] * Rp * 4, Rp * 4, 32 * 16 * g["m_tiles"] * 4, g["splits"] * rows * d * 4]
    return sum(up256(p) for p in parts) + 256


def special_tile(mi, ni, rows, cols, off):
    """the block-uniform predicate of EPI_SIG: the tile takes the path with the positive and ragged-edge selects"""
    p0 = off + 256 * mi
    return 256 * (mi + 1) > rows or 256 * (ni + 1) > cols or (p0 < 256 * (ni + 1) and p0 + 256 > 256 * ni)


# id: ((rows, cols, off, d), the geometry claimed, what it puts on an edge)
CASES = {
    "G1": ((1, 1, 0, 64), dict(splits=1, live=1, m_tiles=1, n_tiles=1, d_tiles=1, m_patches=1, n_patches=1, logits_steps=1),
           "one row, one key, one K-step of the logits pass"),
    "G2": ((256, 1024, 256, 64), dict(splits=2, live=2, map="UNITS", m_tiles=1, n_tiles=4, m_patches=1, n_patches=1, logits_steps=1),
           "no ragged edge; the band exactly fills tile (0, 1), every other tile takes the plain path; 2 splits"),
    "G3": ((255, 1024, 769, 128), dict(splits=2, live=2, m_tiles=1, n_tiles=4, logits_steps=2),
           "off + rows == cols; band from one column past a boundary to the last column"),
    "G4": ((300, 1300, 511, 128), dict(splits=3, live=3, last=8, map="UNITS", m_tiles=2, n_tiles=6, da_units=6),
           "band starts one column before a boundary; 2 row tiles; 3 splits; both edges ragged"),
    "G5": ((1025, 1290, 255, 64), dict(splits=3, m_tiles=5, n_tiles=6, m_patches=2, n_patches=1, logits_steps=1),
           "5 row tiles in 2 row patches; row 1024 alone in its tile; rows 1023 / 1024"),
    "G6": ((33, 6700, 6667, 128), dict(splits=13, live=12, last=9, map="UNITS", m_tiles=1, n_tiles=27, n_patches=4),
           "13 splits, 12 live (one empty); 27 column tiles in 4 patches; off + rows == cols"),
    "G7": ((65, 10900, 700, 64), dict(splits=21, live=20, last=1, map="UNITS", m_tiles=1, n_tiles=43, n_patches=6, logits_steps=1),
           "21 splits, 20 live; the last live split has one K-step; 6 column patches"),
    "G8": ((300, 4300, 2000, 192), dict(splits=8, live=8, last=5, per=9, map="SPLITX", m_tiles=2, n_tiles=17, d_tiles=1, d_last=192,
                                        n_patches=3, logits_steps=3),
           "8 splits, the SPLITX map; d = 192: three logits K-steps, a partial d tile"),
    "G9": ((40, 2304, 2040, 320), dict(splits=4, live=4, m_tiles=1, n_tiles=9, d_tiles=2, d_last=64, n_patches=2, logits_steps=5),
           "2 d tiles, the second 64 wide; band across the 2047 / 2048 patch edge; cols a multiple of 256"),
    "G10": ((257, 2049, 1792, 64), dict(splits=4, live=4, m_tiles=2, n_tiles=9, n_patches=2, logits_steps=1),
            "one row in the second row tile; one column in the ninth column tile; band starts on a boundary"),
    "G11": ((512, 512, 0, 4096), dict(splits=1, live=1, m_tiles=2, n_tiles=2, d_tiles=16, d_last=256, logits_steps=64),
            "the width limit: 16 d tiles and 64 logits K-steps; no ragged edge"),
}
ONE_RAGGED_ROW_TILE = ("G1", "G3", "G6", "G7", "G9")       # every tile of theirs is special


@functools.lru_cache(maxsize=None)
def make_case(cid):
    """bf16 unit rows a [rows, d], b [cols, d] (CPU), the offset and the twins [(column, row)] of a case"""
    (rows, cols, off, d), _, _ = CASES[cid]
    g = torch.Generator().manual_seed(7000 + list(CASES).index(cid))
    a = _unit(torch.randn(rows, d, generator=g))
    b = _unit(torch.randn(cols, d, generator=g))
    b[off:off + rows] = _positives(a, g)
    a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
    twins = direction_twins(rows, cols, off, d)
    for j, r in twins:
        b[j] = b[off + r]
    return dict(a=a, b=b, off=off, coef=1.0 / cols, twins=twins)


SAT_T, SAT_BIAS = 0.01, 0.0
SAT_N = (125.3, 125.7, 126.3, 126.7)            # n = l log2 e on both sides of the clamp, and their negatives


@functools.lru_cache(maxsize=None)
def make_saturated():
    """48 rows against 300 keys, d = 128, off = 100, for T = 0.01 and bias 0 (n = 144.27 cosine).  Row i < 8: the positive's cosine
    puts n at +-SAT_N (the positive is evaluated at -n); row 8 + i, i < 8: a negative at column 200 + i likewise.  The rounding
    to bf16 moves n by a few tenths: the tests assert where it landed."""
    rows, cols, off, d = 48, 300, 100, 128
    g = torch.Generator().manual_seed(7100)
    a = _unit(torch.randn(rows, d, generator=g))
    b = _unit(torch.randn(cols, d, generator=g))
    b[off:off + rows] = _positives(a, g)
    targets = [s * n for s in (1.0, -1.0) for n in SAT_N]
    for i, n in enumerate(targets):
        c = n * SAT_T / LOG2E
        for row, col in ((i, off + i), (8 + i, 200 + i)):
            z = torch.randn(1, d, generator=g)
            z = _unit(z - (z * a[row:row + 1]).sum() * a[row:row + 1])
            b[col] = c * a[row] + math.sqrt(1.0 - c * c) * z[0]
    marks = [(i, off + i) for i in range(8)] + [(8 + i, 200 + i) for i in range(8)]
    return dict(a=a.to(torch.bfloat16), b=b.to(torch.bfloat16), off=off, coef=1.0 / cols, twins=[], marks=marks)


def score_error_of(a, b):
    """max |S32 - S64|, both products by torch on the CPU"""
    a, b = a.cpu(), b.cpu()
    return float(((a.float() @ b.float().T).double() - a.double() @ b.double().T).abs().max())


@functools.lru_cache(maxsize=None)
def score_error(cid):
    c = make_case(cid)
    return score_error_of(c["a"], c["b"])


# ---- float64 reference and the bounds of the module docstring ----
def reference(a, b, off, T, bias, coef, upstream, score_error, keep=False):
    """float64 autograd of the formulas above, on the device of a and b, for rows a [R, d] (a whole problem or a row shard with
    off = lo) against b [C, d]; T >= MIN_T and bias as the kernels read them (float32 values).  Returns (ref, bnd):
    loss_rows [R], dbias, dT (floats), da [R, d], db [C, d] at ct = coef upstream / Tc, and in ref the magnitude sums the bounds
    are made of (sum_sp [R], sum_m [R], mag_da = ct (m + BW) |b|, mag_db).  keep: also m, sp and g [R, C]."""
    dev = a.device
    R, d = a.shape
    C = b.shape[0]
    geo = geometry(R, C, d)
    a64 = a.double().detach().requires_grad_(True)
    b64 = b.double().detach().requires_grad_(True)
    t = torch.tensor(float(T), dtype=torch.float64, device=dev, requires_grad=True)
    bs = torch.tensor(float(bias), dtype=torch.float64, device=dev, requires_grad=True)
    tc = torch.clamp(t, min=MIN_T)
    S = a64 @ b64.T
    y = -torch.ones(R, C, dtype=torch.float64, device=dev)
    i = torch.arange(R, device=dev)
    y[i, off + i] = 1.0
    z = -y * (S / tc + bs)
    sp = -torch.nn.functional.logsigmoid(-z)                    # softplus(z), accurate at both ends
    loss_rows = sp.sum(1)
    ga, gb, gt, gbs = torch.autograd.grad(loss_rows.sum(), [a64, b64, t, bs])
    Tc = float(tc.detach())
    cu = coef * upstream
    ct = cu / Tc
    with torch.no_grad():
        sp, z, S = sp.detach(), z.detach(), S.detach()
        m = torch.sigmoid(z)
        aa, ab = a64.detach().abs(), b64.detach().abs()
        dl = 4.0 * score_error / Tc + 6.0 * H * S.abs() / Tc + 4.0 * H * abs(float(bias))
        e_g = m * ((1.0 - m) * (dl + 2.0 * H) + 4.0 * H) + FLUSH
        e_sp = m * (dl + 2.0 * H) + 8.0 * H * sp + FLUSH
        nt4 = -(-geo["n_tiles"] // 4)
        sum_sp, sum_m = sp.sum(1), m.sum(1)
        ref = dict(loss_rows=loss_rows.detach(), dbias=float(gbs), dT=cu * float(gt), da=cu * ga, db=cu * gb, sum_sp=sum_sp, sum_m=sum_m)
        bnd = dict(loss_rows=e_sp.sum(1) + (16 + nt4) * H * sum_sp)
        bnd["dbias"] = float(e_g.sum()) + (23 + nt4 + -(-R // 256)) * H * float(sum_m.sum())
        BW = e_g + EPS_P * (m + e_g)
        mag = m + BW
        flush = FLUSH * (1.0 + ct)
        ref["mag_da"], ref["mag_db"] = ct * (mag @ ab), ct * (mag.T @ aa)
        bnd["da"] = ct * (BW @ ab) + (geo["Cp"] + 38) * H * ref["mag_da"] + flush
        bnd["db"] = ct * (BW.T @ aa) + (geo["Rp"] + 38) * H * ref["mag_db"] + flush
        depth = 145 + -(-(geo["splits"] * geo["m_tiles"] * geo["d_tiles"]) // 256)
        bnd["dT"] = (float((aa * bnd["da"]).sum()) + depth * H * float((aa * ref["mag_da"]).sum())) / Tc + 3.0 * H * abs(ref["dT"])
        if keep:
            ref.update(m=m, sp=sp, g=-y * m, dl=dl)
    return ref, bnd


OUTPUTS = ("loss_rows", "dbias", "dT", "da", "db")


def ratios(got, ref, bnd, bf16=False):
    """largest |error| / bound per output (outputs ``got`` lacks are skipped).  bf16: the gradients were rounded once more on the
    way out, 2^-8 |value| joins their bounds."""
    out = {}
    for name in OUTPUTS:
        if name not in got:
            continue
        if name in ("dbias", "dT"):
            out[name] = abs(float(got[name]) - ref[name]) / bnd[name]
            continue
        g, bd = got[name].double(), bnd[name]
        if bf16 and name in ("da", "db"):
            bd = bd + 2.0 ** -8 * g.abs()
        out[name] = float(((g - ref[name]).abs() / bd).max()) if g.numel() else 0.0
    return out


def value_over_bound(ref, bnd):
    """largest |value| / bound per output: how many bounds the reference itself is worth"""
    zero = {n: (0.0 if n in ("dbias", "dT") else torch.zeros_like(ref[n])) for n in OUTPUTS}
    return ratios(zero, ref, bnd)


def signal(case, ref, bnd, coef_up, Tc, show=None):
    """per output, the smallest over the twins of (the twin's contribution) / bound: softplus(z_rj) in loss row r, g_rj b_j in da
    row r (the best of its d elements), g_rj a_r in db row j, g_rj in dbias.  ref: from reference(..., keep=True).  show: a
    label to print the line under."""
    if not case["twins"]:
        return {}
    ct = coef_up / Tc
    a, b = case["a"].double().to(ref["m"].device), case["b"].double().to(ref["m"].device)
    out = dict(loss_rows=math.inf, da=math.inf, db=math.inf, dbias=math.inf)
    for j, r in case["twins"]:
        m = float(ref["m"][r, j])
        out["loss_rows"] = min(out["loss_rows"], float(ref["sp"][r, j] / bnd["loss_rows"][r]))
        out["da"] = min(out["da"], float((ct * m * b[j].abs() / bnd["da"][r]).max()))
        out["db"] = min(out["db"], float((ct * m * a[r].abs() / bnd["db"][j]).max()))
        out["dbias"] = min(out["dbias"], m / bnd["dbias"])
    if show is not None:
        print(f"sig tile signal {show}: weakest twin / bound " + " ".join(f"{k}={v:.3g}" for k, v in out.items()))
    return out


# ---- the design's arithmetic on the CPU ----
def sig_terms32(n):
    """sig_terms of aecf_nce_gemm.hip in float32: (sigmoid, lg2, corr) with softplus = ln 2 * lg2 + corr"""
    one = torch.ones((), dtype=torch.float32)
    nc = torch.clamp(n, max=126.0)
    u = torch.exp2(nc)
    t = u + one
    r = one / t
    return u * r, torch.log2(t) + (n - nc), (u - (t - one)) * r


def emulate(case, mutation=None, T=0.1, bias=-10.0, upstream=1.0):
    """The kernels' arithmetic on the CPU: float32 scores by torch, n = S s2 + b2, sig_terms in float32 (the clamp at 126, the
    positive from -n), float32 sums, g rounded once to bf16, float32 products scaled by coef / Tc upstream afterwards.
    mutation: ("drop", j, r) / ("twice", j, r) -- key j 0 times / twice in row r; ("padcol",); ("padrow",); ("shift",);
    ("plain", mi, ni) -- the positives of that tile treated as negatives; ("dbias_bf16",)."""
    f32 = torch.float32
    a, b, off = case["a"], case["b"], case["off"]
    kind = mutation[0] if mutation else None
    af, bf = a.float(), b.float()
    R, C = af.shape[0], bf.shape[0]
    if kind == "padcol":
        bf = torch.cat([bf, bf[-1:]], 0)                        # the copy of a padded key re-reads the last one
    if kind == "padrow":
        af = torch.cat([af, af[-1:]], 0)
    inv = torch.tensor(1.0, dtype=f32) / torch.clamp(torch.tensor(T, dtype=f32), min=MIN_T)
    s2 = inv * torch.tensor(LOG2E, dtype=f32)
    b2 = torch.tensor(bias, dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    n = (af @ bf.T) * s2 + b2
    rr = torch.arange(af.shape[0])
    pcol = off + rr + (1 if kind == "shift" else 0)
    ok = pcol < bf.shape[0] if kind != "padrow" else pcol < C
    pos = torch.zeros_like(n, dtype=torch.bool)
    pos[rr[ok], pcol[ok]] = True
    if kind == "plain":
        _, mi, ni = mutation
        tile = torch.zeros_like(pos)
        tile[256 * mi:256 * (mi + 1), 256 * ni:256 * (ni + 1)] = True
        pos &= ~tile
    sig, lg2, corr = sig_terms32(n)
    sig_p, lg2_p, corr_p = sig_terms32(-n)
    g = torch.where(pos, -sig_p, sig)
    sp = torch.where(pos, lg2_p, lg2) * torch.tensor(LN2, dtype=f32) + torch.where(pos, corr_p, corr)
    if kind in ("drop", "twice"):
        _, j, r = mutation
        times = 0.0 if kind == "drop" else 2.0
        g[r, j] *= times
        sp[r, j] *= times
    loss_rows = sp.sum(1)[:R]
    gb = g.to(torch.bfloat16).float()
    dbias = (gb if kind == "dbias_bf16" else g).sum(1).sum()
    osc = torch.tensor(case["coef"], dtype=f32) * inv * torch.tensor(upstream, dtype=f32)
    da = (gb[:R] @ bf) * osc
    db = ((gb.T @ af) * osc)[:C]
    dT = -(af[:R] * da).sum() * inv
    return dict(loss_rows=loss_rows, dbias=float(dbias), dT=float(dT), da=da, db=db)
