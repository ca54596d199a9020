"""Cases, float64 reference, derived bounds and a CPU emulation shared by tests/test_ntxent_tile_cpu.py and
tests/test_ntxent_tile_gpu.py: the tile-GEMM form of NT-Xent (aecf_ntxent_sym_pass1 / _loss / _grads: the EPI_EXP_DT and
EPI_EXP_SELF logits epilogues, nce_finalize_kernel, nce_weights_dt_kernel, the gradient products and the two ntx_* kernels of
aecf_nce_gemm.hip).  Rows, shards, twins and geometry are those of tests/nce_tile_cases.py, cases S1 - S4, imported, not copied;
the reference's formulas are the pooled ones of tests/supcon_pool_cases.reference with every label -1, over both anchor halves.
Nothing here touches a GPU; every function works on the device of the tensors it is given.

The problem.  n rows of two views a, b (unit bf16 rows), dealt over shards (emulated ranks); shard s owns rows lo .. hi.  The 2 n
rows are ONE pool; every row is an anchor, its positive the partner in the other view, itself left out:
  anchors of view a:  keys [b | a], partner at column i,     excluded at column n + i        (supcon_pool_cases, off = 0, self_off = n)
  anchors of view b:  keys [b | a], partner at column n + i, excluded at column i            (off = n, self_off = 0)
With Pa, Pb [n, 2 n] the two softmaxes (0 on the excluded key) the three blocks the kernels form carry
  G_X = Pa[:, :n] + Pb[:, n:]^T - 2 I       (a x b; the b x a block is its transpose)
  G_Y = Pa[:, n:]                           (a x a, 0 on the diagonal)
  G_Z = Pb[:, :n]                           (b x b, 0 on the diagonal)
and a shard's outputs are (ct = coef / T, rows s = lo .. hi)
  loss_rows[s] = both anchors of pair i            da_loc[s] = ct (G_X[s] b + G_Y[s] a)        db_loc[s] = ct G_Z[s] b
  da_all share = ct G_Y[s]^T a[s]                  db_all share = ct (G_X[s]^T a[s] + G_Z[s]^T b[s])
  dT share = -(1/T) (sum a[s] . da_loc[s] + sum b[s] . db_loc[s])
  colsum = sum_{i in s} E_X[i, :], plus the row sums of E_Z[s] on columns lo .. hi          (what ranks exchange, pass 1's output)
The shares add up to the pooled gradients (``pooled_check`` compares them with supcon_pool_cases.reference's dq and dk).

Bounds: the derivation of tests/nce_tile_cases.py (its docstring: h = 2^-24, EPS_P = 2^-8, s_err, xm, eps_e, the row-sum count
12 + ceil(n_tiles / 4), the column-sum count 15 + ceil(m_tiles / 4), eps_w = eps_e + eps_sum + 10 h, the two weight bounds, "a
float32 sum of n terms in any order is within n h of the sum of their magnitudes", dT's depth), extended by what this design adds.
Every count is an upper bound read off the code; the bounds carry no further factor and were never fitted to results.
  s_err: the largest |S32 - S64| over the three products a b^T, a a^T, b b^T.  xm likewise over the three.
  lX, lY, lZ: row sums, each eps_l = eps_e + (12 + ceil(n_tiles / 4)) h (the excluded key is a term less, no rounding more).
  Da = lX + lY: a sum of two positive numbers, the larger relative error of the two plus ONE float32 addition:
          eps_Da = eps_l + h
  col_sums[off + i] = cX + lZ_i on a rank's own range: max(eps_cs, eps_l) + h (ONE addition); elsewhere eps_cs.
  Db = the float32 sum of the shards' col_sums in rank order (shards - 1 additions):
          eps_Db = eps_e + (max over shards of max(15 + ceil(m_tiles / 4), 12 + ceil(n_tiles / 4)) + 1 + shards - 1) h
  loss_rows: nce_tile_cases' symmetric bound with l := Da, c := Db and ln(2 C) in M (a denominator holds up to 2 C - 1 keys):
          |d loss_i| <= eps_Da + eps_Db + 2 (4 s_err / T + 2 h xm) + 12 h M
      With ONE row in all (S1) both denominators hold the partner alone: the reference is 0 to float64 rounding, the kernels give
      log(E) + 1/T - s/T, which is inside this bound and not exactly 0.
  W_X: nce_tile_cases' two weight bounds with Q = Pa[:, :n] + Pb[:, n:]^T, npos = 2 and eps_w = eps_e + max(eps_Da, eps_Db) + 10 h.
  W_Y, W_Z: the off-diagonal bound at v = 0 (u + 0 is exact; the count stays an upper bound), Q = G_Y / G_Z; the excluded key
      is bf16(ct (0 (u + 0) - 0)) = 0 exactly and G is 0 there: only the flush term remains.
  da_loc = the float32 sum of TWO products: Cp terms each and the slab sum over both products' <= 32 + 32 slabs, 2 (Cp + 32) terms:
          |d da_loc| <= (BW_X + 2 (Cp + 32) h (ct |G_X| + BW_X)) |b| + (BW_Y + 2 (Cp + 32) h (ct |G_Y| + BW_Y)) |a|
      db_all's share likewise with 2 (Rp + 32) (two products of Rp terms, one addition of the two float32 stages);
      db_loc and da_all's share are single products: Cp + 32 and Rp + 32 terms.
  dT: the partials of THREE da products (parts = 3 splits m_tiles d_tiles) from their float32 accumulators, each within its own
      single-product bound (Cp + 32):
          |d dT| <= (1/T) (B + (145 + ceil(parts / 256)) h (V + B)) + 3 h |dT|,   B = sum |a| (bX + bY) + sum |b| bZ,
          V = sum |a| (|ct G_X b| + |ct G_Y a|) + sum |b| |ct G_Z b|
Other output forms: bf16 gradients are the float32 sums rounded once (round to nearest even): the GPU test asks for the bits of
the float32 output rounded by torch.  An upstream scalar multiplies ct: reference and bounds are taken at coef * upstream.

Twins (nce_tile_cases.symmetric_twins): a[r'] = a[r] and b[r'] = b[r], r' on rows 127, 128, 255, 256, 1023, 1024 and on every
shard's first and last row.  Rows r and r' of ONE view are bit-identical, so E_Y[r, r'] = exp((a_r . a_r - 1) / T) is the value of
the excluded key itself, about 1, next to a partner of exp(-0.2 / T): it holds most of Da_r and is a legitimate key.  An
exclusion by value (or by "equals the row maximum") drops it and moves loss_rows[r] by ln of a large factor; S2's twin rows 255 |
256 lie in different shards, S4's across its three."""
import functools
import math

import torch

from tests import nce_tile_cases as N
from tests import supcon_pool_cases as P
from tests.nce_stream_cases import EPS_P, FLUSH, used_temperature  # noqa: F401  (used_temperature: for the tests)

H = N.H
TEMPS = N.TEMPS
MIN_T = N.MIN_T
CASE_IDS = ("S1", "S2", "S3", "S4")
GRADS = ("da_loc", "db_loc", "da_all", "db_all", "da_all_sum", "db_all_sum")
OUTPUTS = ("colsum", "loss_rows") + GRADS + ("dT",)


def make_case(cid):
    """nce_tile_cases.make_symmetric: a, b [n, d] bf16 unit rows (CPU), the shard bounds, coef = 0.5 / n, the twins"""
    assert cid in CASE_IDS
    return N.make_symmetric(cid)


def workspace_bytes_py(rows, cols, d):
    """ntx_carve() + 256: three E blocks, the two partial arrays, Da, lY, lZ, 1/Da, 1/Db, 1/Db at the partner, ediag, zeros, the dT
    partials, the slabs of two da products, the float32 stage of db_all -- each rounded up to 256 bytes"""
    g = N.geometry(rows, cols, d)
    Rp, Cp = g["Rp"], g["Cp"]
    parts = [Rp * Cp * 2] * 3 + [g["n_tiles"] * Rp * 4, g["m_tiles"] * Cp * 4, Rp * 4, Rp * 4, Rp * 4, Rp * 4, Cp * 4, Rp * 4, Rp * 4,
                                 Cp * 4, 3 * 32 * 16 * g["m_tiles"] * 4, 2 * g["splits"] * rows * d * 4, 2 * cols * d * 4]
    return sum(N.up256(p) for p in parts) + 256


@functools.lru_cache(maxsize=None)
def score_error(cid):
    """max |S32 - S64| over the three products of a case, by torch on the CPU"""
    c = make_case(cid)
    worst = 0.0
    for x, y in ((c["a"], c["b"]), (c["a"], c["a"]), (c["b"], c["b"])):
        worst = max(worst, float(((x.float() @ y.float().T).double() - x.double() @ y.double().T).abs().max()))
    return worst


def pooled(a, b, T, coef):
    """supcon_pool_cases.reference over both anchor halves of the whole problem, every label -1: (ref of view a's anchors, ref of
    view b's anchors), keys [b | a]"""
    n = a.shape[0]
    dev = a.device
    pool = torch.cat([b, a])
    lab, lab_pool = torch.full((n,), -1, dtype=torch.int64, device=dev), torch.full((2 * n,), -1, dtype=torch.int64, device=dev)
    ra = P.reference(a, pool, P.match_matrix(lab, lab_pool, 0, n), P.excluded(n, 2 * n, n, dev), T, coef)
    rb = P.reference(b, pool, P.match_matrix(lab, lab_pool, n, 0), P.excluded(n, 2 * n, 0, dev), T, coef)
    return ra, rb


def reference(a, b, shards, T, coef, s_err):
    """float64 on the device of a and b [n, d].  Returns (ref, bnd): loss_rows, da_loc, db_loc [n ...] whole; colsum, da_all, db_all,
    dT lists, one entry per shard (the shard's share); da_all_sum / db_all_sum the shares added up, with the summed bounds."""
    a64, b64 = a.double(), b.double()
    n, d = a64.shape
    dev = a.device
    ct = coef / T
    ra, rb = pooled(a, b, T, coef)
    Pa, Pb = ra["P"], rb["P"]
    idx = torch.arange(n, device=dev)
    QX = Pa[:, :n] + Pb[:, n:].T
    GX = QX.clone()
    GX[idx, idx] -= 2.0
    GY, GZ = Pa[:, n:], Pb[:, :n]
    loss = ra["loss_rows"] + rb["loss_rows"]
    xm, EX, EZ = 0.0, None, None
    for x, y, name in ((a64, b64, "X"), (a64, a64, "Y"), (b64, b64, "Z")):
        S = x @ y.T
        xm = max(xm, float(torch.maximum(S.abs(), (S - 1.0).abs()).max()) / T)
        if name == "X":
            EX = torch.exp((S - 1.0) / T)
        if name == "Z":
            EZ = torch.exp((S - 1.0) / T)
            EZ[idx, idx] = 0.0
    aa, ab = a64.abs(), b64.abs()
    geoms = [N.geometry(hi - lo, n, d) for lo, hi in shards]
    eps_e = 4.0 * s_err / T + 6.0 * H * xm + 2.0 * H
    eps_Db = eps_e + (max(max(15 + -(-g["m_tiles"] // 4), 12 + -(-g["n_tiles"] // 4)) for g in geoms) + 1 + len(shards) - 1) * H
    M = xm + 1.0 / T + math.log(2 * n)
    flush = FLUSH * (1.0 + ct)
    ref = dict(loss_rows=loss, da_loc=torch.empty_like(a64), db_loc=torch.empty_like(a64), da_all=[], db_all=[], dT=[], colsum=[])
    bnd = dict(loss_rows=torch.empty_like(loss), da_loc=torch.empty_like(a64), db_loc=torch.empty_like(a64), da_all=[], db_all=[],
               dT=[], colsum=[])
    for (lo, hi), g in zip(shards, geoms):
        rows = hi - lo
        eps_l = eps_e + (12 + -(-g["n_tiles"] // 4)) * H
        eps_cs = eps_e + (15 + -(-g["m_tiles"] // 4)) * H
        eps_Da = eps_l + H
        eps_w = eps_e + max(eps_Da, eps_Db) + 10.0 * H
        bnd["loss_rows"][lo:hi] = eps_Da + eps_Db + 2.0 * (4.0 * s_err / T + 2.0 * H * xm) + 12.0 * H * M
        ii, pos = torch.arange(rows, device=dev), idx[lo:hi]
        off_diag = ct * ((1.0 + EPS_P) ** 2 * (1.0 + eps_w) - 1.0)
        BX = off_diag * QX[lo:hi] + flush
        gd = GX[lo:hi][ii, pos].abs()
        BX[ii, pos] = ct * (EPS_P * gd + (1.0 + EPS_P) * (eps_w * QX[lo:hi][ii, pos] + 8.0 * H * gd)) + flush
        BY = off_diag * GY[lo:hi] + flush
        BZ = off_diag * GZ[lo:hi] + flush
        mX, mY, mZ = ct * GX[lo:hi].abs() + BX, ct * GY[lo:hi] + BY, ct * GZ[lo:hi] + BZ
        nC, nR = (g["Cp"] + 32) * H, (g["Rp"] + 32) * H
        # single-product bounds (the float32 accumulators dT is taken from), then the outputs
        bX1, bY1, bZ1 = (BX + nC * mX) @ ab, (BY + nC * mY) @ aa, (BZ + nC * mZ) @ ab
        vX, vY, vZ = ct * (GX[lo:hi] @ b64), ct * (GY[lo:hi] @ a64), ct * (GZ[lo:hi] @ b64)
        ref["da_loc"][lo:hi] = vX + vY
        bnd["da_loc"][lo:hi] = (BX + 2.0 * nC * mX) @ ab + (BY + 2.0 * nC * mY) @ aa
        ref["db_loc"][lo:hi] = vZ
        bnd["db_loc"][lo:hi] = bZ1
        ref["da_all"].append(ct * (GY[lo:hi].T @ a64[lo:hi]))
        bnd["da_all"].append((BY + nR * mY).T @ aa[lo:hi])
        ref["db_all"].append(ct * (GX[lo:hi].T @ a64[lo:hi] + GZ[lo:hi].T @ b64[lo:hi]))
        bnd["db_all"].append((BX + 2.0 * nR * mX).T @ aa[lo:hi] + (BZ + 2.0 * nR * mZ).T @ ab[lo:hi])
        dT = -(1.0 / T) * float((a64[lo:hi] * (vX + vY)).sum() + (b64[lo:hi] * vZ).sum())
        depth = 145 + -(-(3 * g["splits"] * g["m_tiles"] * g["d_tiles"]) // 256)
        B = float((aa[lo:hi] * (bX1 + bY1)).sum() + (ab[lo:hi] * bZ1).sum())
        V = float((aa[lo:hi] * (vX.abs() + vY.abs())).sum() + (ab[lo:hi] * vZ.abs()).sum())
        ref["dT"].append(dT)
        bnd["dT"].append((B + depth * H * (V + B)) / T + 3.0 * H * abs(dT))
        cs = EX[lo:hi].sum(0)
        e_cs = torch.full_like(cs, eps_cs)
        cs[lo:hi] += EZ[lo:hi].sum(1)
        e_cs[lo:hi] = max(eps_cs, eps_l) + H
        ref["colsum"].append(cs)
        bnd["colsum"].append(e_cs * cs)
    for name in ("da_all", "db_all"):
        ref[name + "_sum"], bnd[name + "_sum"] = sum(ref[name]), sum(bnd[name])
    return ref, bnd


def pooled_check(a, b, shards, T, coef):
    """largest |difference| between this module's shares, added up, and the pooled gradients of supcon_pool_cases.reference
    (dq of each half on its own rows, dk on the pool [b | a]), relative to the largest gradient or to 1 (S1: every gradient is
    0): float64 rounding only"""
    n = a.shape[0]
    ref, _ = reference(a, b, shards, T, coef, 0.0)
    ra, rb = pooled(a, b, T, coef)
    dk = ra["dk"] + rb["dk"]
    want_a, want_b = ra["dq"] + dk[n:], rb["dq"] + dk[:n]
    got_a, got_b = ref["da_loc"] + ref["da_all_sum"], ref["db_loc"] + ref["db_all_sum"]
    scale = max(float(torch.maximum(want_a.abs().max(), want_b.abs().max())), 1.0)
    worst = max(float((got_a - want_a).abs().max()), float((got_b - want_b).abs().max())) / scale
    dT = abs(sum(ref["dT"]) - (ra["dT"] + rb["dT"])) / max(abs(ra["dT"] + rb["dT"]), 1.0)
    return worst, dT


def ratios(got, ref, bnd):
    """largest |error| / bound per output over all shards (``got`` laid out as ``ref``; outputs it lacks are skipped).  Every
    element takes part."""
    out = {}
    for name in OUTPUTS:
        if name not in got:
            continue
        worst = 0.0
        gs, rs, bs = (got[name], ref[name], bnd[name]) if isinstance(ref[name], list) else ([got[name]], [ref[name]], [bnd[name]])
        for g, r, b in zip(gs, rs, bs):
            if name == "dT":
                worst = max(worst, abs(float(g) - r) / b)
            else:
                worst = max(worst, float(((g.double() - r).abs() / b).max()))
        out[name] = worst
    return out


def signal(ref, bnd):
    """largest |value| / bound per output: how many bounds the reference itself is worth"""
    nothing = {name: [v * 0 for v in ref[name]] if isinstance(ref[name], list) else ref[name] * 0 for name in bnd}
    return ratios(nothing, ref, bnd)


# ---- the design's arithmetic on the CPU ----
MUTATIONS = ("self_kept", "self_in_sum", "lz_local", "by_value")


def emulate(a, b, shards, T, coef, mutation=None, upstream=1.0):
    """The kernels' arithmetic on the CPU: float32 scores, exponentials and sums, the excluded key 0 in the stored E and in the row
    sum, Da = lX + lY, col_sums = cX with lZ added on the shard's own range, their float32 sum over the shards; E rounded to bf16
    once, the weights a second time, the partner's weight from the float32 ediag; float32 products, two of them added in float32
    where they share an output.  Output laid out as ``reference`` (without the _sum entries).  mutation:
      "self_kept"    the anchor itself is not excluded (neither from the stored E nor from the row sum)
      "self_in_sum"  it is excluded from the stored E but not from the row sum
      "lz_local"     lZ is added at the local index i instead of off + i
      "by_value"     every key whose float32 score equals the anchor's own is excluded (the twins with it)"""
    assert mutation is None or mutation in MUTATIONS
    f32 = torch.float32
    inv = torch.tensor(1.0, dtype=f32) / torch.tensor(T, dtype=f32)
    scale2 = inv * torch.tensor(1.4426950408889634, dtype=f32)
    af, bf = a.float(), b.float()
    n = a.shape[0]
    state, cols = [], []
    for lo, hi in shards:
        rows = hi - lo
        ii, pos = torch.arange(rows), torch.arange(lo, hi)
        st = dict(EX=torch.exp2((af[lo:hi] @ bf.T) * scale2 - scale2))
        for name, x in (("Y", af), ("Z", bf)):
            S = x[lo:hi] @ x.T
            E = torch.exp2(S * scale2 - scale2)
            if mutation == "by_value":
                gone = S == S[ii, pos][:, None]
            else:
                gone = torch.zeros_like(S, dtype=torch.bool)
                gone[ii, pos] = True
            kept, summed = E.masked_fill(gone, 0.0), E.masked_fill(gone, 0.0)
            if mutation == "self_kept":
                kept, summed = E, E
            if mutation == "self_in_sum":
                summed = E
            st["E" + name], st["l" + name] = kept, summed.sum(1)
        st["Da"] = st["EX"].sum(1) + st["lY"]
        c = st["EX"].sum(0).clone()
        if mutation == "lz_local":
            c[0:rows] = c[0:rows] + st["lZ"]
        else:
            c[lo:hi] = c[lo:hi] + st["lZ"]
        cols.append(c)
        state.append(st)
    c_tot = cols[0]
    for c in cols[1:]:
        c_tot = c_tot + c
    ct = torch.tensor(coef, dtype=f32) * inv * torch.tensor(upstream, dtype=f32)
    out = dict(loss_rows=torch.empty(n), colsum=cols, da_loc=torch.empty(a.shape, dtype=f32), db_loc=torch.empty(a.shape, dtype=f32),
               da_all=[], db_all=[], dT=[])
    for (lo, hi), st in zip(shards, state):
        rows = hi - lo
        ii, pos = torch.arange(rows), torch.arange(lo, hi)
        dot = (af[lo:hi] * bf[pos]).sum(1)
        ediag = torch.exp2((dot - 1.0) * inv * torch.tensor(1.4426950408889634, dtype=f32))
        out["loss_rows"][lo:hi] = (torch.log(st["Da"]) + inv - dot * inv) + (torch.log(c_tot[pos]) + inv - dot * inv)
        u, v = 1.0 / st["Da"], 1.0 / c_tot
        uz = v[pos]
        Eb = st["EX"].to(torch.bfloat16).float()
        WX = ct * (Eb * (u[:, None] + v[None, :]))
        WX[ii, pos] = ct * (ediag * (u + v[pos]) - 2.0)
        WX = WX.to(torch.bfloat16).float()
        WY = (ct * (st["EY"].to(torch.bfloat16).float() * u[:, None])).to(torch.bfloat16).float()
        WZ = (ct * (st["EZ"].to(torch.bfloat16).float() * uz[:, None])).to(torch.bfloat16).float()
        dX, dY, dZ = WX @ bf, WY @ af, WZ @ bf
        out["da_loc"][lo:hi] = dX + dY
        out["db_loc"][lo:hi] = dZ
        out["da_all"].append(WY.T @ af[lo:hi])
        out["db_all"].append(WX.T @ af[lo:hi] + WZ.T @ bf[lo:hi])
        out["dT"].append(-float(((af[lo:hi] * dX).sum() + (af[lo:hi] * dY).sum() + (bf[lo:hi] * dZ).sum()) * inv))
    return out
