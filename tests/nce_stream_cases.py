"""Case table, inputs, float64 reference, derived bounds and a CPU emulation shared by tests/test_nce_stream_cpu.py and
tests/test_nce_stream_gpu.py: the streaming InfoNCE (aecf_nce_flash.hip on aecf_flash_stream.h) at its split, tile and
low-temperature edges.  Nothing here touches a GPU; every function works on the device of the tensors it is given.

One direction:  loss_i = logsumexp_j(q_i.k_j / T) - q_i.k_{off+i} / T,  P = softmax_j,  G = P - onehot,
                dq = coef/T G k,  dk = coef/T G^T q,  dT = -(1/T) sum q . dq.

The bounds are elementwise and derived from the kernel's roundings, never from its results (ct = coef / T):
  eps_p = 2^-8    a weight is rounded to bf16 once (8 significant bits: the half-ulp is at most 2^-8 of the value) -- the DQ
                  role rounds exp(x - m), the DK role rounds ct (P - onehot); nothing else rounds a weight
  eps_x = 4 max|S32 - S64| / T + 2^-22 (1/T + ln cols)
                  the error of an exponent x = S/T - lse.  S32 = q.float() @ k.float().T is torch's CPU product, so the first
                  term is measured on the reference (the factor 4: the MFMA sums in another order); the second is the float32
                  rounding of x (|x| <= 2/T), of the running maximum and of the log-sum-exp (a sum of <= cols terms)
  f = 2^-126      a weight below the smallest normal float32 may flush to zero
  |d loss_i|  <= 2 eps_x                                     (lse and the positive's logit)
  |d dq[i,c]| <= ct (eps_p + 2 eps_x) (P |k|)[i,c] + ct eps_x |k[off+i,c]| + ct f sum_j |k[j,c]|
  |d dk[j,c]| <= ct (eps_p + 2 eps_x) (|G|^T |q|)[j,c] + 2 ct eps_x (P^T |q|)[j,c] + ct f sum_i |q[i,c]|
  |d dT|      <= (1/T) sum |q| bound_dq
The bounds carry no further factor.

Which output carries the teeth where.  The dT bound is a triangle-inequality sum over rows x d elements: at T = 0.07 |dT| is
between about one bound (cases B, D) and sixty (case H; none in case A, where dT = 0), so a wrong sign or factor shows there, but a small error of dT does not; at T <= 0.02 the softmax of
these inputs is saturated, dq and dT are zero to within 1e-12 of their bounds, and the lines of dq and dT say only that they
stay zero (an accumulator that missed a rescale would leave dq at ct |k|, 2^8 bounds away).  loss_rows and dk are the
detectors at every T: a sentinel row holds P = 1/2, 1/2, so |dk| on its columns is about 200 bounds and loss_rows moves by
about ln 2, hundreds of bounds, when a key is lost or doubled (``signal`` prints these figures).

Sentinels make a dropped or doubled key visible.  A sentinel column j holds an exact copy of the positive key of a row r_j
(distinct rows for distinct sentinels), so P[r_j, j] == P[r_j, off + r_j] at every T, about one half at low T: losing or
repeating column j moves loss[r_j] by about ln 2 and dk[j] by about ct / 6 and more, far beyond their bounds.  A duplicate key
does not move dq (p k is unchanged), which is why loss and dk are the detectors."""
import functools
import math

import torch

EPS_P = 2.0 ** -8
FLUSH = 2.0 ** -126
WIDTHS = (128, 256, 384, 512, 768, 1024)
TEMPS = (0.07, 0.02, 0.005)
SENTINEL_ROWS = (0, 15, 16, 63, 64)          # and rows - 1


# ---- the split rule of the DQ role, restated (aecf_amd/csrc/aecf_flash_stream.h: flash_split) ----
def flash_split_py(rows, cols):
    """(rule, live, per, last): the split count the workspace is sized by, the non-empty splits, keys per split (a multiple of
    the 32-key tile) and the keys of the last live split"""
    rb = (rows + 63) // 64
    ks = (256 + rb - 1) // rb
    ks = max(1, min(ks, (cols + 511) // 512, 64))
    per = ((cols + ks - 1) // ks + 31) // 32 * 32
    live = (cols + per - 1) // per
    return ks, live, per, cols - (live - 1) * per


def workspace_bytes_py(rows, cols, d):
    """partials (m, l, O) of `rule` splits, the log-sum-exp of every row, 1024 spare bytes"""
    rule = flash_split_py(rows, cols)[0]
    return (rule * rows * (d + 2) + rows) * 4 + 1024


# id: ((rows, cols, off, d), (rule, live, per, last), what it puts on an edge)
CASES = {
    "A": ((1, 1, 0, 128), (1, 1, 32, 1), "one row, one key"),
    "B": ((1, 513, 512, 128), (2, 2, 288, 225), "rows = 1; 2 splits 288 + 225; positive in the last column"),
    "C": ((65, 2049, 700, 256), (5, 5, 416, 385), "5 splits of 416, last 385 = 12 tiles + 1 key; second row block holds one row"),
    "D": ((63, 300, 200, 384), (1, 1, 320, 300), "one split; last tile has 12 keys, so its second sub-tile is skipped; the DK "
                                                   "role streams 32 + 31 rows"),
    "E": ((64, 7681, 31, 512), (16, 16, 512, 1), "16 splits of 512; the last holds exactly 1 key"),
    "F": ((200, 7697, 7497, 768), (16, 16, 512, 17), "last split 17 keys, so its second sub-tile holds 1; off + rows == cols; DQ "
                                                       "runs in 2 column parts"),
    "G": ((33, 7201, 0, 1024), (15, 15, 512, 33), "last split 33 keys = tile + 1; DQ in 4 column parts, DK in 2; the DK role "
                                                    "streams 32 + 1 rows"),
    "H": ((512, 16385, 0, 128), (32, 31, 544, 65), "rule 32, live 31: one empty split whose workspace slots are never written"),
}


def sentinel_plan(rows, cols, off):
    """[(column j, row r_j)]: the boundary columns of the split geometry that are no positive's column, each paired with a
    distinct row; as many as the distinct rows allow (the boundaries nearest the end of the key range first)"""
    _, live, per, _ = flash_split_py(rows, cols)
    wanted = [cols - 1, (live - 1) * per, (live - 1) * per - 1, per - 1, per, 31, 32, 0]
    columns = []
    for j in wanted:
        if 0 <= j < cols and not (off <= j < off + rows) and j not in columns:
            columns.append(j)
    picked = []
    for r in SENTINEL_ROWS + (rows - 1,):
        if 0 <= r < rows and r not in picked:
            picked.append(r)
    return list(zip(columns, picked))


def _unit(x):
    return x / x.norm(dim=1, keepdim=True)


@functools.lru_cache(maxsize=None)
def make_case(cid):
    """bf16 unit rows q [rows, d], k [cols, d] (CPU), the offset and the sentinels of a case"""
    (rows, cols, off, d), _, _ = CASES[cid]
    g = torch.Generator().manual_seed(4000 + list(CASES).index(cid))
    q = _unit(torch.randn(rows, d, generator=g))
    k = _unit(torch.randn(cols, d, generator=g))
    k[off:off + rows] = _unit(0.8 * q + 0.6 * _unit(torch.randn(rows, d, generator=g)))
    q, k = q.to(torch.bfloat16), k.to(torch.bfloat16)
    sentinels = sentinel_plan(rows, cols, off)
    for j, r in sentinels:
        k[j] = k[off + r]
    return dict(q=q, k=k, off=off, sentinels=sentinels)


def used_temperature(T):
    """the float32 value a device temperature (or a float argument of the C ABI) holds, as a Python float"""
    return float(torch.tensor(T, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def score_error(cid):
    """max |S32 - S64| of a case, both products by torch on the CPU"""
    c = make_case(cid)
    s32 = c["q"].float() @ c["k"].float().T
    s64 = c["q"].double() @ c["k"].double().T
    return float((s32.double() - s64).abs().max())


def eps_x(s_err, T, cols):
    return 4.0 * s_err / T + 2.0 ** -22 * (1.0 / T + math.log(cols))


def reference(q, k, off, T, coef):
    """float64 of one direction on the device of q and k"""
    q, k = q.double(), k.double()
    rows = q.shape[0]
    S = q @ k.T
    x = S / T
    lse = torch.logsumexp(x, dim=1)
    i = torch.arange(rows, device=q.device)
    loss_rows = lse - x[i, off + i]
    P = torch.exp(x - lse[:, None])
    G = P.clone()
    G[i, off + i] -= 1.0
    ct = coef / T
    dq = ct * (G @ k)
    dk = ct * (G.T @ q)
    dT = -(1.0 / T) * float((q * dq).sum())
    return dict(S=S, loss_rows=loss_rows, P=P, G=G, dq=dq, dk=dk, dT=dT)


def bounds(ref, q, k, off, T, coef, ex):
    """the elementwise bounds of the module docstring; ``ex`` = eps_x"""
    aq, ak = q.double().abs(), k.double().abs()
    rows = q.shape[0]
    ct = coef / T
    P, G = ref["P"], ref["G"]
    b_dq = ct * (EPS_P + 2 * ex) * (P @ ak) + ct * ex * ak[off:off + rows] + ct * FLUSH * ak.sum(0)
    b_dk = ct * (EPS_P + 2 * ex) * (G.abs().T @ aq) + 2 * ct * ex * (P.T @ aq) + ct * FLUSH * aq.sum(0)
    return dict(loss_rows=torch.full_like(ref["loss_rows"], 2 * ex), dq=b_dq, dk=b_dk, dT=float((aq * b_dq).sum()) / T)


def ratios(got, ref, bnd):
    """largest |error| / bound per output"""
    out = {}
    for name in ("loss_rows", "dq", "dk"):
        out[name] = float(((got[name].double() - ref[name]).abs() / bnd[name]).max())
    out["dT"] = abs(float(got["dT"]) - ref["dT"]) / bnd["dT"]
    return out


def signal(ref, bnd):
    """largest |value| / bound per output: how many bounds the reference itself is worth -- what a check can see at all"""
    out = {name: float((ref[name].abs() / bnd[name]).max()) for name in ("loss_rows", "dq", "dk")}
    out["dT"] = abs(ref["dT"]) / bnd["dT"]
    return out


def emulate(q, k, off, T, coef, column=None, times=1):
    """The kernel's arithmetic on the CPU: float32 scores and exponents, weights rounded to bf16 where the kernel rounds them,
    float32 sums.  ``column`` / ``times``: the DQ role streams that key 0 times (dropped) or twice -- what a wrong split or
    tile boundary does; the DK role then works from the log-sum-exp that pass left."""
    qf, kf = q.float(), k.float()
    rows = qf.shape[0]
    inv_t = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(T, dtype=torch.float32)
    x = (qf @ kf.T) * inv_t
    i = torch.arange(rows)
    seen = torch.ones(x.shape[1], dtype=torch.bool)
    if column is not None and times == 0:
        seen[column] = False
    m = x[:, seen].max(dim=1).values
    e = torch.exp(x - m[:, None]) * seen.float()
    if column is not None and times == 2:
        e = torch.cat([e, e[:, column:column + 1]], dim=1)
    l = e.sum(dim=1)
    lse = m + torch.log(l)
    loss_rows = lse - (qf * kf[off:off + rows]).sum(dim=1) * inv_t
    ct = torch.tensor(coef, dtype=torch.float32) * inv_t

    def dk_of(cols_):                                           # the DK role for the keys cols_ (a slice)
        w = torch.exp(x[:, cols_] - lse[:, None])
        hit = (off + i)[:, None] == torch.arange(x.shape[1])[cols_][None, :]
        return ((w - hit.float()) * ct).to(torch.bfloat16).float().T @ qf

    if column is not None:                                      # a mutation is judged on loss_rows and dk[column] alone
        return dict(loss_rows=loss_rows, dk_column=dk_of(slice(column, column + 1))[0])
    o = e.to(torch.bfloat16).float() @ kf
    dq = ct * (o / l[:, None] - kf[off:off + rows])
    dT = -float((qf * dq).sum(dim=1).sum() * inv_t)
    return dict(loss_rows=loss_rows, dq=dq, dk=dk_of(slice(None)), dT=dT)
