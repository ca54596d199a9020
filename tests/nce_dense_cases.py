"""Case table, inputs, float64 reference, derived bounds and a CPU emulation shared by tests/test_nce_dense_cpu.py and
tests/test_nce_dense_gpu.py: the MATERIALISING InfoNCE (nce_generic_fwd_bwd in aecf_capi.hip over aecf_contrastive.hip and the
library's plain GEMMs) -- the only form float32 rows reach, and the form of bf16 rows whose width is no streaming width below
T = 0.025 -- and l2_normalize (l2norm_fwd_kernel / l2norm_bwd_kernel), which stands in front of every loss.  Nothing here
touches a GPU; every function works on the device of the tensors it is given.

One direction:  loss_i = logsumexp_j(q_i.k_j / T) - q_i.k_{off+i} / T,  P = softmax_j,  G = P - onehot,
                dq = ct G k,  dk = ct G^T q,  dT = -(1/T) sum_i q_i . dq_i = -(1/T) sum_ij ct G_ij S_ij,  ct = coef / T.
A device temperature is read as Tc = max(T, min_t); dT = 0 where T < min_t.

What the form does (aecf_capi.hip: nce_generic_fwd_bwd): S = q k^T by launch_gemm_nt (float32 out) into the workspace;
nce_rows_kernel, one block of 256 threads per row, three sweeps of 256 columns at a time: the maximum of s * inv_temp, the sum
of expf(s * inv_temp - mx), then g_j = (expf(s_j * inv_temp - lse) - [j == pos]) * (coef * inv_temp), stored in the rows' dtype,
with tdot_i = sum_j g_j s_j (fmaf, from the float32 g) parked in the first `rows` floats of the kT region; nce_dtemp_kernel sums
the tdot; transpose_rect overwrites the kT region with k^T; dq = G kT^T by launch_gemm_nt; dk = G^T q by launch_gemm_tn with
Ej = cols, splits = 1.

The roundings, read off that code (h = 2^-24, half a float32 ulp; EPS_P = 2^-8, half a bf16 ulp; first order in h unless a
closed form is as short; the bounds carry no further factor):
  S32_ij          float32 rows: products round, so in ANY summation order |S32 - S| <= g(d) sum_c |q_c| |k_c|, g(n) = n h / (1 - n h)
                  rounded up to (d + 1) h.  bf16 rows: products are exact in float32, the sum's error is measured on the
                  reference as 4 max |S32 - S64| of torch's CPU products (the factor 4: the MFMA sums in another order) -- the
                  convention of tests/nce_stream_cases.py.  Either is eS_ij.
  x_ij            = s * inv_temp: inv_temp = 1.0f / T within an ulp of 1 / T (2 h), the product (h; none when the compiler
                  fuses it into the subtraction that follows, which only helps):  ex_ij = eS_ij / T + 3 h |S_ij| / T
  a_ij            = x - mx (the maximum cancels in the log-sum-exp, whatever its own rounding): one rounding of |a| <= A,
                  A = max_i (max_j S_ij - min_j S_ij) / T:   e_arg_i = max_j ex_ij + h A
  sum_i           expf within an ulp (2 h of the value); the sum of `cols` positive terms: ceil(cols / 256) per thread, 6 steps of
                  the wave reduction, 2 of (red0 + red1) + (red2 + red3): n_s = ceil(cols / 256) + 8 additions at most on the
                  way of any term:   |ln(sum32 / sum)| <= e_log_i = e_arg_i - ln(1 - 2 h) - n_s ln(1 - h)
  lse_i           = mx + logf(sum): logf within an ulp of |ln sum| <= ln cols, the addition rounds |lse| <= L = max|S| / T +
                  ln cols:   e_lse_i = e_log_i + 2 h ln cols + h L
  loss_i          = lse - s[pos] * inv_temp:   |d loss_i| <= e_lse_i + ex_i,pos + h (L + max|S| / T)
  p_ij            = expf(x - lse): the exponent's error is ex_ij + e_lse_i, its rounding h (A + ln cols), expf 2 h:
                  |d p_ij| <= expm1(ex_ij + e_lse_i + h (A + ln cols) + 2 h) P_ij + f,   f = 2^-126: a weight below the smallest
                  normal float32 may flush to zero
  g_ij            = (p - [j == pos]) * scale, scale = coef * inv_temp: float(coef) (h), inv_temp (2 h), their product (h), the
                  subtraction (h, exact off the positive), the product (h):
                  bG32_ij = ct (expm1(..) P_ij + 6 h |G_ij|) + f (1 + ct)          (f ct: g itself may flush)
                  float32 rows store g as it is.  bf16 rows round it once: bG_ij = bG32_ij + EPS_P (ct |G_ij| + bG32_ij)
  dq = G k        launch_gemm_nt, K = cols; dk = G^T q: launch_gemm_tn, `rows` terms (the zero rows that pad the last 32-row
                  step add nothing).  A float32 sum of n terms in any order is within g(n) of the sum of magnitudes (products
                  included; bf16 x bf16 products are exact, which only helps):
                  |d dq| <= (bG + g(cols) (ct |G| + bG)) |k|,     |d dk| <= (bG + g(rows) (ct |G| + bG))^T |q|
  tdot_i          = sum_j g32_ij S32_ij: fmaf per thread, then the block reduction, n_t = ceil(cols / 256) + 8 roundings:
                  b_tdot_i = sum_j (bG32 |S| + (ct |G| + bG32) eS) + n_t h sum_j (ct |G| + bG32) (|S| + eS)
  dT              nce_dtemp_kernel: ceil(rows / 256) strided partials per thread and a tree of 8 levels (n_d = ceil(rows / 256)
                  + 8), the quotient by Tc within an ulp (2 h); Tc = max(T, min_t) is exact:
                  |d dT| <= (1 + 2 h) (sum_i b_tdot_i + n_d h sum_ij (ct |G| + bG32) (|S| + eS)) / T + 2 h |dT|
``e_in`` (the Python-surface test): the rows handed to the form are themselves within e_in |value| of the reference's rows
(l2_normalize's forward bound).  Then eS grows by (2 e_in + e_in^2) sum_c |q_c| |k_c| and each gradient product by e_in times
the sum of magnitudes of its terms (the operand next to G); everything above carries over.

Which output carries the teeth.  A sentinel row holds P = 1/2, 1/2 at low T (and a share >= 1/4 at T = 0.07), so a key lost or
counted twice moves loss_rows of that row by about ln 2 and dk of that column by about ct / 4, far beyond bounds of a few h / T.
A duplicate key does not move dq (p k is unchanged).  dT's bound is a triangle-inequality sum over rows x cols terms: a wrong
sign, factor or a missing row shows there in float32; in the bf16 cases (T = 0.02, saturated softmax) dq and dT are near zero and
say only that they stay so.

Sentinels.  A sentinel column j holds an exact copy of the positive key of a row r_j of its own, on a column that is no
positive's column: the boundaries the geometry names -- cols - 1, the first column of the last 128-column tile, 1023/1024,
511/512, 255/256, 127/128, 63/64, 31/32 -- where the case has them free; the rows come from the row edges first (0, rows - 1,
31/32, 63/64, 127/128).  M5 (rows == cols) has no free column and no sentinel.

l2_normalize (aecf_contrastive.hip), n_l = ceil(d / 64) + 6 (the lane's fmaf chain and the wave reduction):
  forward   ss within n_l h (positive terms), sqrtf and the quotient 1 / max(., eps) within an ulp each (2 h), the product h:
            r_inv = n_l h / 2 + 4 h (the root halves the sum's error),  |d inv_norm| <= r_inv inv_norm,
            |d zn| <= (r_inv + h) |zn|   (+ EPS_P (1 + r_inv + h) |zn| for bf16: one rounding of the product)
            A row under eps takes inv = 1 / eps whatever its sum: the same bound holds.
  backward  dot = sum dzn zn: |d dot| <= n_l h sum |dzn| |zn|;  dz = (dzn - zn dot) inv: the product, the subtraction and the
            last product round (3 h of the magnitudes of the two terms, whose difference may cancel):
            |d dz| <= inv (|zn| b_dot + 3 h (|dzn| + |zn| |dot|))   (+ EPS_P (|dz| + that) for bf16)
            judged against the float64 backward AT the stored zn and inv_norm: what the kernel is specified to compute."""
import functools
import math

import torch

from tests.nce_stream_cases import EPS_P, FLUSH, _unit, used_temperature  # noqa: F401  (used_temperature: for the tests)
from tests.nce_tile_cases import _positives

H = 2.0 ** -24
F32, BF16 = torch.float32, torch.bfloat16
F32_TEMPS = (0.07, 0.01)
BF16_TEMPS = (0.02,)
MIN_T = 0.025                                  # the library's default clamp; the ABI tests pass their own
WS_K = (128, 256, 384, 512, 768, 1024)
OUTPUTS = ("loss_rows", "dq", "dk", "dT")


# ---- geometry restated from the code ----
def up256(v):
    return (v + 255) // 256 * 256


def esize(dtype):
    return 2 if dtype == BF16 else 4


def workspace_bytes_py(rows, cols, d, dtype):
    """nce_generic_workspace_bytes: S (float32), G and kT (the rows' dtype), each rounded up to 256 bytes"""
    es = esize(dtype)
    return up256(rows * cols * 4) + up256(rows * cols * es) + up256(d * cols * es)


def ws_plain_supported(N, K, lda):
    """gemm_ws_supported for a plain product (pooled = 0): K a weight-stationary width, N a multiple of the 128 ct columns a
    block owns, two 16 x 2 x 2 K tiles within 150 KB of LDS, dense rows"""
    if K not in WS_K:
        return False
    ct = 2 if K <= 512 else 1
    if N % (128 * ct) != 0:
        return False
    if 2 * 16 * 2 * 2 * K > 150 * 1024:
        return False
    return lda == K


def gemm_nt_arm(dtype, R, N, K, lda):
    """launch_gemm_nt: 'ws' (bf16, weight-stationary), '32' (fewer than 64 block tiles of 128 x 128) or '128'"""
    if dtype == BF16 and ws_plain_supported(N, K, lda):
        return "ws"
    return "32" if ((R + 127) // 128) * ((N + 127) // 128) < 64 else "128"


def arms(dtype, rows, cols, d):
    """(the arm of S = q k^T: N = cols, K = d; the arm of dq = G k: N = d, K = cols)"""
    return gemm_nt_arm(dtype, rows, cols, d, d), gemm_nt_arm(dtype, rows, d, cols, cols)


# id: (dtype, (rows, cols, off, d), (arm of S, arm of dq), what it is there for)
CASES = {
    "M1": (F32, (1, 64, 63, 64), ("32", "32"), "smallest legal problem; positive in the last column"),
    "M2": (F32, (37, 192, 155, 192), ("32", "32"), "off + rows == cols; ragged 32-row tiles; d and cols = 1.5 x 128"),
    "M3": (F32, (65, 320, 100, 64), ("32", "32"), "one row past a 64-row wave tile; one full column sweep plus a partial one"),
    "M4": (F32, (130, 1088, 0, 320), ("32", "32"), "130 = 4 x 32 + 2 batch rows in gemm_tn; more than four sweeps; K = 1088 in dq"),
    "M5": (F32, (256, 256, 0, 128), ("32", "32"), "every tile full, rows == cols: the anchor"),
    "M6": (F32, (1000, 1088, 88, 1024), ("128", "128"), "128 x 128 tiles for both products; ragged last row tile; rows > 256 in "
                                                        "nce_dtemp_kernel"),
    "B1": (BF16, (100, 192, 50, 192), ("32", "32"), "bf16 32 x 32 tiles; rectangular gemm_tn_tr"),
    "B2": (BF16, (200, 768, 500, 640), ("32", "ws"), "dq with K = 768, N = 640 on the weight-stationary kernel, float32 out"),
    "B3": (BF16, (1000, 1088, 0, 1088), ("128", "128"), "bf16 128 x 128 tiles with out_f32 for both products"),
}
SMALL = ("M1", "M2", "M3", "M4", "M5", "B1", "B2")         # the cases the CPU suite emulates
ROW_EDGES = (31, 32, 63, 64, 127, 128)


def temps_of(cid):
    return F32_TEMPS if CASES[cid][0] == F32 else BF16_TEMPS


def boundary_columns(cols):
    """[(column, kind)]: the columns the geometry names, the end of the key range first"""
    wanted = [(cols - 1, "last column"), ((cols - 1) // 128 * 128, "first column of the last tile")]
    for b in (1024, 512, 256, 128, 64, 32):
        wanted += [(b, f"column {b}"), (b - 1, f"column {b - 1}")]
    out, seen = [], set()
    for j, kind in wanted:
        if 0 <= j < cols and j not in seen:
            seen.add(j)
            out.append((j, kind))
    return out


def sentinel_plan(rows, cols, off):
    """[(column j, row r_j, kind)]: the boundary columns that are no positive's column, each with a row of its own (the row edges
    first, then the remaining rows from the middle outwards); as many as the rows allow"""
    columns = [(j, kind) for j, kind in boundary_columns(cols) if not (off <= j < off + rows)]
    order = []
    for r in (0, rows - 1) + ROW_EDGES + tuple(range(rows // 2, rows)) + tuple(range(rows // 2)):
        if 0 <= r < rows and r not in order:
            order.append(r)
    return [(j, r, kind) for (j, kind), r in zip(columns, order)]


@functools.lru_cache(maxsize=None)
def make_case(cid):
    """unit rows q [rows, d], k [cols, d] (CPU, the case's dtype; float32 rows keep their full mantissas), the offset, coef and
    the sentinels [(column, row, kind)]"""
    dtype, (rows, cols, off, d), _, _ = CASES[cid]
    g = torch.Generator().manual_seed(8000 + list(CASES).index(cid))
    q = _unit(torch.randn(rows, d, generator=g))
    k = _unit(torch.randn(cols, d, generator=g))
    k[off:off + rows] = _positives(q, g)
    q, k = q.to(dtype), k.to(dtype)
    sentinels = sentinel_plan(rows, cols, off)
    for j, r, _ in sentinels:
        k[j] = k[off + r]
    return dict(q=q, k=k, off=off, coef=0.5 / cols, dtype=dtype, sentinels=sentinels)


def score_error_of(q, k):
    """max |S32 - S64|, both products by torch on the CPU"""
    q, k = q.cpu(), k.cpu()
    return float(((q.float() @ k.float().T).double() - q.double() @ k.double().T).abs().max())


@functools.lru_cache(maxsize=None)
def score_error(cid):
    c = make_case(cid)
    return score_error_of(c["q"], c["k"])


# ---- float64 reference and the bounds of the module docstring ----
def reference(q, k, off, T, coef, min_t=None):
    """float64 of one direction on the device of q and k, at Tc = max(T, min_t); dT = 0 where T < min_t"""
    q, k = q.double(), k.double()
    rows = q.shape[0]
    tc = T if min_t is None else max(T, min_t)
    S = q @ k.T
    x = S / tc
    lse = torch.logsumexp(x, dim=1)
    i = torch.arange(rows, device=q.device)
    loss_rows = lse - x[i, off + i]
    P = torch.exp(x - lse[:, None])
    G = P.clone()
    G[i, off + i] -= 1.0
    ct = coef / tc
    dq = ct * (G @ k)
    dk = ct * (G.T @ q)
    dT = -(1.0 / tc) * float((q * dq).sum())
    if min_t is not None and T < min_t:
        dT = 0.0
    return dict(S=S, loss_rows=loss_rows, P=P, G=G, dq=dq, dk=dk, dT=dT, T=tc)


def gamma(n):
    return n * H / (1.0 - n * H)


def bounds(ref, q, k, off, coef, s_err=None, e_in=0.0):
    """the elementwise bounds of the module docstring for the reference ``ref`` of rows q, k in the dtype the form runs in.
    s_err: max |S32 - S64| (bf16 rows; float32 rows take the a-priori bound)."""
    bf16 = q.dtype == BF16
    aq, ak = q.double().abs(), k.double().abs()
    rows, d = aq.shape
    cols = ak.shape[0]
    T = ref["T"]
    ct = coef / T
    S, P, G = ref["S"], ref["P"], ref["G"]
    aS, aG = S.abs(), G.abs()
    qk = aq @ ak.T
    eS = torch.full_like(S, 4.0 * s_err) if bf16 else (d + 1) * H * qk
    if e_in:
        eS = eS + (2.0 * e_in + e_in * e_in) * qk
    smax = float(aS.max())
    lnc = math.log(cols)
    A = float((S.max(dim=1).values - S.min(dim=1).values).max()) / T
    L = smax / T + lnc
    ex = eS / T + 3.0 * H * aS / T
    e_arg = ex.max(dim=1).values + H * A
    n_s = -(-cols // 256) + 8
    e_log = e_arg - math.log1p(-2.0 * H) - n_s * math.log1p(-H)
    e_lse = e_log + 2.0 * H * lnc + H * L
    i = torch.arange(rows, device=S.device)
    b_loss = e_lse + ex[i, off + i] + H * (L + smax / T)
    rel = torch.expm1(ex + e_lse[:, None] + H * (A + lnc) + 2.0 * H)
    bG32 = ct * (rel * P + 6.0 * H * aG) + FLUSH * (1.0 + ct)
    bG = bG32 + EPS_P * (ct * aG + bG32) if bf16 else bG32
    mag = ct * aG + bG
    b_dq = (bG + (gamma(cols) + e_in) * mag) @ ak
    b_dk = (bG + (gamma(rows) + e_in) * mag).T @ aq
    mag32 = ct * aG + bG32
    n_t = -(-cols // 256) + 8
    n_d = -(-rows // 256) + 8
    size = float((mag32 * (aS + eS)).sum())
    b_tdot = float((bG32 * aS + mag32 * eS).sum()) + n_t * H * size
    b_dT = (1.0 + 2.0 * H) * (b_tdot + n_d * H * size) / T + 2.0 * H * abs(ref["dT"])
    return dict(loss_rows=b_loss, dq=b_dq, dk=b_dk, dT=b_dT)


def ratios(got, ref, bnd):
    """largest |error| / bound per output (outputs ``got`` lacks are skipped); a bound of zero admits only the exact value"""
    out = {}
    for name in OUTPUTS:
        if name not in got:
            continue
        if name == "dT":
            err, b = abs(float(got["dT"]) - ref["dT"]), bnd["dT"]
            out[name] = err / b if b > 0 else (0.0 if err == 0 else math.inf)
        else:
            out[name] = float(((got[name].double() - ref[name]).abs() / bnd[name]).max())
    return out


def value_over_bound(ref, bnd):
    """largest |value| / bound per output: how many bounds the reference itself is worth -- what a check can see at all"""
    out = {name: float((ref[name].abs() / bnd[name]).max()) for name in ("loss_rows", "dq", "dk")}
    out["dT"] = abs(ref["dT"]) / bnd["dT"] if bnd["dT"] > 0 else 0.0
    return out


# ---- the form's arithmetic on the CPU ----
def emulate(q, k, off, T, coef, min_t=None, drop_col=None, dup_col=None, pos_shift=0, ignore_offset=False, drop_last_row_dk=False,
            drop_last_sweep=False, unscaled=False, drop_last_partial=False, keep_dt_below_clamp=False):
    """float32 scores, exponents and sums, G stored in the rows' dtype, float32 products -- and the mutations of
    tests/test_nce_dense_cpu.py: the row sum loses column ``drop_col`` / counts ``dup_col`` twice / loses the last partial sweep
    of 256 columns; the positive is taken at off + i + pos_shift (modulo cols) or at i; dk loses the last batch row; G is left
    unscaled; dT loses the last row's partial or is kept below the clamp."""
    dtype = q.dtype
    qf, kf = q.float(), k.float()
    rows, cols = qf.shape[0], kf.shape[0]
    one = torch.tensor(1.0, dtype=F32)
    t32 = torch.tensor(T, dtype=F32)
    tc = t32 if min_t is None else torch.maximum(t32, torch.tensor(min_t, dtype=F32))
    inv_t = one / tc
    S = qf @ kf.T
    x = S * inv_t
    mx = x.max(dim=1).values
    e = torch.exp(x - mx[:, None])
    if drop_col is not None:
        e[:, drop_col] = 0.0
    if drop_last_sweep:
        e[:, (cols - 1) // 256 * 256:] = 0.0
    total = e.sum(dim=1)
    if dup_col is not None:
        total = total + e[:, dup_col]
    lse = mx + torch.log(total)
    i = torch.arange(rows)
    pos = (i if ignore_offset else off + i + pos_shift) % cols
    loss_rows = lse - S[i, pos] * inv_t
    scale = one if unscaled else torch.tensor(coef, dtype=F32) * inv_t
    g32 = torch.exp(x - lse[:, None])
    g32[i, pos] -= 1.0
    g32 = g32 * scale
    g = g32.to(dtype).float()
    dq = g @ kf
    dk = (g[:-1] if drop_last_row_dk else g).T @ (qf[:-1] if drop_last_row_dk else qf)
    tdot = (g32 * S).sum(dim=1)
    if drop_last_partial:
        tdot = tdot[:-1]
    dT = float(-tdot.sum() / tc)
    if min_t is not None and T < min_t and not keep_dt_below_clamp:
        dT = 0.0
    return dict(loss_rows=loss_rows, dq=dq, dk=dk, dT=dT)


# ---- l2_normalize ----
L2_SHAPES = ((1, 1), (5, 63), (70, 65), (33, 100), (4, 4096), (257, 64))
L2_KINDS = ("zero", "tiny", "huge", "dominant")
L2_EPS = 1e-12


def l2_inputs(n, d, dtype):
    """[(z, {row: kind})]: seeded rows with the four special rows at rows 0, 1, n - 2, n - 1 where n >= 5; a shape with fewer
    rows gets one plain variant and further variants that hold the special rows n at a time."""
    g = torch.Generator().manual_seed(8100 + 7 * n + d)

    def row(kind):
        v = torch.randn(d, generator=g)
        if kind == "zero":
            return torch.zeros(d)
        if kind == "tiny":
            return (v.double() / v.double().norm() * 1e-13).float()
        if kind == "huge":
            return (v.double() / v.double().norm() * 1e15).float()
        if kind == "dominant":
            v[d // 2] = 1e4
        return v

    def variant(kinds):
        z = torch.stack([row(kinds.get(r)) for r in range(n)])
        return z.to(dtype), kinds

    if n >= 5:
        return [variant(dict(zip((0, 1, n - 2, n - 1), L2_KINDS)))]
    out = [variant({})]
    for lo in range(0, len(L2_KINDS), n):
        out.append(variant(dict(enumerate(L2_KINDS[lo:lo + n]))))
    return out


def l2_forward_reference(z, eps):
    """float64 zn, inv_norm of the stored rows z (eps: the float32 value the kernel holds) and their bounds"""
    bf16 = z.dtype == BF16
    z64 = z.double()
    d = z.shape[1]
    inv = 1.0 / z64.norm(dim=1).clamp_min(eps)
    zn = z64 * inv[:, None]
    n_l = -(-d // 64) + 6
    r_inv = n_l * H / 2.0 + 4.0 * H
    b_zn = (r_inv + H) * zn.abs()
    if bf16:
        b_zn = b_zn + EPS_P * (1.0 + r_inv + H) * zn.abs()
    return dict(zn=zn, inv_norm=inv), dict(zn=b_zn, inv_norm=r_inv * inv), r_inv


def l2_backward_reference(zn, inv, dzn):
    """float64 dz = (dzn - zn (dzn . zn)) inv at the STORED zn and inv_norm, and its bound"""
    bf16 = zn.dtype == BF16
    z64, g64, inv64 = zn.double(), dzn.double(), inv.double()[:, None]
    d = zn.shape[1]
    n_l = -(-d // 64) + 6
    dot = (g64 * z64).sum(dim=1, keepdim=True)
    b_dot = n_l * H * (g64.abs() * z64.abs()).sum(dim=1, keepdim=True)
    dz = (g64 - z64 * dot) * inv64
    b_dz = inv64 * (z64.abs() * b_dot + 3.0 * H * (g64.abs() + z64.abs() * dot.abs()))
    if bf16:
        b_dz = b_dz + EPS_P * (dz.abs() + b_dz)
    return dz, b_dz


def l2_backward_chain(zn, inv, g, b_g, e_zn, r_inv, out_bf16=False):
    """float64 dz = (g - zn (g . zn)) inv of the REFERENCE's zn, inv and g, and the bound of a kernel that was handed rows within
    e_zn |zn|, an inv_norm within r_inv inv and a gradient within b_g of them (the Python-surface test: the whole chain).  Every
    product is bilinear, so each term is bounded with the magnitudes of the perturbed operands:
        b_dot   = sum (b_g |zn'| + |g| e_zn |zn|) + n_l h sum (|g| + b_g) |zn'|,          |zn'| = (1 + e_zn) |zn|
        b_inner = b_g + |zn'| b_dot + e_zn |zn| |dot| + 3 h (|g| + b_g + |zn'| (|dot| + b_dot))
        b_dz    = (1 + r_inv) inv b_inner + r_inv |dz|      (+ EPS_P (|dz| + b_dz) for a bf16 output)"""
    d = zn.shape[1]
    n_l = -(-d // 64) + 6
    az, ag = zn.abs(), g.abs()
    azp = (1.0 + e_zn) * az
    dot = (g * zn).sum(dim=1, keepdim=True)
    b_dot = (b_g * azp + ag * e_zn * az).sum(dim=1, keepdim=True) + n_l * H * ((ag + b_g) * azp).sum(dim=1, keepdim=True)
    b_inner = b_g + azp * b_dot + e_zn * az * dot.abs() + 3.0 * H * (ag + b_g + azp * (dot.abs() + b_dot))
    dz = (g - zn * dot) * inv[:, None]
    b_dz = (1.0 + r_inv) * inv[:, None] * b_inner + r_inv * dz.abs()
    if out_bf16:
        b_dz = b_dz + EPS_P * (dz.abs() + b_dz)
    return dz, b_dz


def l2_ratio(got, ref, bnd):
    """largest |error| / bound; where the bound is zero (a zero row) only the exact value passes"""
    err = (got.double() - ref).abs()
    r = torch.where(bnd > 0, err / bnd, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    return float(r.max())
