"""Cases, float64 reference, derived bounds and a CPU emulation shared by tests/test_queue_nce_cpu.py and
tests/test_queue_nce_gpu.py: the symmetric InfoNCE with a key queue on the tile GEMMs (aecf_nce_queue_pass1 / _loss / _grads: the
EPI_EXP_DT and EPI_EXP_Q logits epilogues, nce_finalize_kernel, nce_weights_dt_kernel, the gradient products, ntx_combine_kernel
and ntx_prep_kernel of aecf_nce_gemm.hip) and the ring buffer behind it (aecf_key_queue_push).  Rows, shards, twins and geometry
are those of tests/nce_tile_cases.py, cases S1 - S4, imported, not copied.  Nothing here touches a GPU; every function works on
the device of the tensors it is given.

The problem.  n rows of two views a, b (unit bf16 rows), dealt over shards (emulated ranks); shard s owns rows lo .. hi.  Two
queues Qa, Qb [q_cap, d] of which slots 0 .. V - 1 are keys: those of Qb are further negatives of the anchors of view a, those of
Qa of the anchors of view b.  With Pa [n, n + V] the softmax of a_i over [b | Qb[:V]] and Pb [n, n + V] that of b_g over
[a | Qa[:V]], the three blocks the kernels form carry
  G_X = Pa[:, :n] + Pb[:, :n]^T - 2 I       (a x b; the b x a block is its transpose)
  G_U = Pa[:, n:]                           (a x Qb)
  G_W = Pb[:, n:]                           (b x Qa)
and a shard's outputs are (ct = coef / T, rows s = lo .. hi)
  loss_rows[s] = both anchors of pair i          da_loc[s] = ct (G_X[s] b + G_U[s] Qb[:V])        db_loc[s] = ct G_W[s] Qa[:V]
  db_all share = ct G_X[s]^T a[s]                dT share = -(1/T) (sum a[s] . da_loc[s] + sum b[s] . db_loc[s])
  colsum = sum_{i in s} E_X[i, :], plus the row sums of E_W[s] on columns lo .. hi          (what ranks exchange, pass 1's output)
(X's column side of dT rides in G_X: sum_ij G_X_ij s_ij holds both softmaxes.)  The queues take no gradient.

Queue plans (q_cap, V): Q0 (256, 0) -- no key at all; Q1 (1, 1); Q2 (256, 255) -- the count one short of a tile; Q3 (513, 257) -- one
whole tile counts, then ONE column of the second, the third tile lies wholly above V and the capacity is ragged; Q4 (300, 300),
filled by three pushes of 130 rows through the host model of the ring (``ring_push``): wrapped, every slot a key.
Contents.  Valid slots: unit rows unrelated to the batch.  In every plan with V >= 2 slot V - 1 of Qb is a bit-identical twin of
b[r] and slot V - 1 of Qa one of a[r] (r: a row without a twin of its own): E_U[r, V - 1] is the partner's own exponential, about
half of Da_r, and a legitimate negative -- an exclusion by value drops it and moves loss_rows[r] by about ln 2.  In Q3 that slot
is the one column of the crossed tile.  Slots at or above V hold finite garbage, alternately unrelated unit rows and rows of
3e38: their scores are inf or NaN and must reach nothing; as keys of the products they meet an exact-zero weight.

Bounds: the derivation of tests/nce_tile_cases.py (its docstring: h = 2^-24, EPS_P = 2^-8, s_err, xm, eps_e, the row-sum count
12 + ceil(n_tiles / 4), the column-sum count 15 + ceil(m_tiles / 4), eps_w = eps_e + eps_sum + 10 h, the two weight bounds, "a
float32 sum of n terms in any order is within n h of the sum of their magnitudes", dT's depth) as tests/ntxent_tile_cases.py
extends it to three blocks, with what this design changes.  Every count is an upper bound read off the code; the bounds carry no
further factor and were never fitted to results.
  s_err: the largest |S32 - S64| over the three products a b^T, a Qb[:V]^T, b Qa[:V]^T.  xm likewise over the three.
  lX: eps_lX = eps_e + (12 + ceil(n_tiles / 4)) h.  lU, lW: the same chain over the queue's tiles, eps_lQ = eps_e + (12 +
      ceil(q_tiles / 4)) h (an excluded column and a skipped tile add exact zeros: terms less, no rounding more).
  Da = lX + lU: two positive numbers, the larger relative error of the two plus ONE float32 addition:
          eps_Da = max(eps_lX, eps_lQ) + h
  col_sums[off + i] = cX + lW_i on a rank's own range: max(eps_cs, eps_lQ) + h (ONE addition more); elsewhere eps_cs.
  Db = the float32 sum of the shards' col_sums in rank order (shards - 1 additions):
          eps_Db = eps_e + (max over shards of max(15 + ceil(m_tiles / 4), 12 + ceil(q_tiles / 4)) + 1 + shards - 1) h
  loss_rows: nce_tile_cases' symmetric bound with l := Da, c := Db and ln(C + V) in M (a denominator holds C + V keys):
          |d loss_i| <= eps_Da + eps_Db + 2 (4 s_err / T + 2 h xm) + 12 h M
  W_X: nce_tile_cases' two weight bounds with Q = Pa[:, :n] + Pb[:, :n]^T, npos = 2 and eps_w = eps_e + max(eps_Da, eps_Db) + 10 h.
  W_U, W_W: the off-diagonal bound at v = 0 (u + 0 is exact; the count stays an upper bound), Q = G_U / G_W.  A queue block has no
      partner element.  A slot at or above V: bf16(ct (0 (u + 0))) = 0 exactly.
  da_loc = ONE float32 sum over the slabs of two products, Cp and Qp terms and <= 32 + 32 slabs: Cp + Qp + 64 terms:
          |d da_loc| <= (BW_X + (Cp + Qp + 64) h (ct |G_X| + BW_X)) |b| + (BW_U + (Cp + Qp + 64) h (ct |G_U| + BW_U)) |Qb|
      db_loc is a single product of Qp + 32 terms, db_all's share one of Rp + 32.
  dT: the partials of THREE da-type products (parts = (splits(Cp) + 2 splits(Qp)) m_tiles d_tiles) from their float32
      accumulators, each within its own single-product bound (Cp + 32 or Qp + 32):
          |d dT| <= (1/T) (B + (145 + ceil(parts / 256)) h (V' + B)) + 3 h |dT|,   B = sum |a| (bX + bU) + sum |b| bW,
          V' = sum |a| (|ct G_X b| + |ct G_U Qb|) + sum |b| |ct G_W Qa|
Other output forms: a bf16 gradient is the float32 sum rounded once (round to nearest even): 2^-8 |value| joins its bound.  An
upstream scalar multiplies ct: reference and bounds are taken at coef * upstream."""
import functools
import math

import torch

from tests import nce_tile_cases as N
from tests.nce_stream_cases import EPS_P, FLUSH, _unit, used_temperature  # noqa: F401  (used_temperature: for the tests)

H = N.H
TEMPS = N.TEMPS
MIN_T = N.MIN_T
CASE_IDS = ("S1", "S2", "S3", "S4")
# id: (q_cap, V)
PLANS = {"Q0": (256, 0), "Q1": (1, 1), "Q2": (256, 255), "Q3": (513, 257), "Q4": (300, 300)}
PLAN_IDS = tuple(PLANS)
Q4_PUSHES = (130, 130, 130)
GRADS = ("da_loc", "db_loc", "db_all", "db_all_sum")
OUTPUTS = ("colsum", "loss_rows") + GRADS + ("dT",)
GARBAGE = 3e38


def make_case(cid):
    """nce_tile_cases.make_symmetric: a, b [n, d] bf16 unit rows (CPU), the shard bounds, coef = 0.5 / n, the twins"""
    assert cid in CASE_IDS
    return N.make_symmetric(cid)


# ---- the ring buffer on the host ----
def ring_push(qa, qb, state, src_a, src_b, mutation=None):
    """aecf_key_queue_push on the host, in place: row i of the n source rows to slot (cursor + i) mod q_cap (n > q_cap: the last
    q_cap rows alone), then cursor = (cursor + n) mod q_cap, valid = min(valid + n, q_cap).  state: [cursor, valid], a list.
    mutation "newest": the push overwrites the NEWEST rows once the ring is full (it writes backwards from the cursor)."""
    q_cap, n = qa.shape[0], src_a.shape[0]
    cur, val = state
    for i in range(max(0, n - q_cap), n):
        slot = (cur + i) % q_cap
        if mutation == "newest" and val + i >= q_cap:
            slot = (cur - 1 - (val + i - q_cap)) % q_cap
        qa[slot], qb[slot] = src_a[i], src_b[i]
    state[0], state[1] = (cur + n) % q_cap, min(val + n, q_cap)


def _garbage(rows, d, g):
    x = _unit(torch.randn(rows, d, generator=g)).to(torch.bfloat16)
    x[1::2] = GARBAGE
    return x


def twin_row(cid):
    """the row whose partner keys sit in the queues: one without a twin of its own, in the middle of the rows"""
    c = make_case(cid)
    n = c["a"].shape[0]
    taken = {r for pair in c["twins"] for r in pair}
    free = [r for r in range(n) if r not in taken] or [0]
    return free[len(free) // 2]


def push_sources(cid):
    """Q4's three pushes [(src_a, src_b)]: unit bf16 rows; the twins of a[r] / b[r] ride in the LAST push so that the wrapped
    ring holds them at slot 89 (push 3's last row)"""
    c = make_case(cid)
    d = c["a"].shape[1]
    g = torch.Generator().manual_seed(6200 + CASE_IDS.index(cid))
    out = []
    for n in Q4_PUSHES:
        out.append((_unit(torch.randn(n, d, generator=g)).to(torch.bfloat16), _unit(torch.randn(n, d, generator=g)).to(torch.bfloat16)))
    r = twin_row(cid)
    out[-1][0][-1], out[-1][1][-1] = c["a"][r], c["b"][r]
    return out


@functools.lru_cache(maxsize=None)
def make_queue(cid, pid, mutation=None):
    """(Qa, Qb [q_cap, d] bf16 on the CPU, V) of a plan; mutation "newest": Q4 filled by the broken ring"""
    c = make_case(cid)
    d = c["a"].shape[1]
    q_cap, V = PLANS[pid]
    g = torch.Generator().manual_seed(6100 + 10 * CASE_IDS.index(cid) + PLAN_IDS.index(pid))
    if pid == "Q4":
        qa, qb = torch.zeros(q_cap, d, dtype=torch.bfloat16), torch.zeros(q_cap, d, dtype=torch.bfloat16)
        state = [0, 0]
        for sa, sb in push_sources(cid):
            ring_push(qa, qb, state, sa, sb, mutation)
        assert state == [sum(Q4_PUSHES) % q_cap, q_cap]
        return qa, qb, V
    qa, qb = _garbage(q_cap, d, g), _garbage(q_cap, d, g)
    qa[:V] = _unit(torch.randn(V, d, generator=g)).to(torch.bfloat16)
    qb[:V] = _unit(torch.randn(V, d, generator=g)).to(torch.bfloat16)
    if V >= 2:
        r = twin_row(cid)
        qa[V - 1], qb[V - 1] = c["a"][r], c["b"][r]
    return qa, qb, V


def workspace_bytes_py(rows, cols, q_cap, d):
    """que_carve() + 256: E_X, E_U, E_W, the two partial arrays, Da, lU, lW, 1/Da, 1/Db, 1/Db at the partner, ediag, zeros, the dT
    partials, the slabs of two da products -- each rounded up to 256 bytes"""
    g, q = N.geometry(rows, cols, d), N.geometry(rows, q_cap, d)
    Rp, Cp, Qp = g["Rp"], g["Cp"], q["Cp"]
    Zp = max(Cp, Qp)
    parts = [Rp * Cp * 2, Rp * Qp * 2, Rp * Qp * 2, (Zp // 256) * Rp * 4, g["m_tiles"] * Cp * 4, Rp * 4, Rp * 4, Rp * 4, Rp * 4, Cp * 4,
             Rp * 4, Rp * 4, Zp * 4, 3 * 32 * 16 * g["m_tiles"] * 4, (g["splits"] + q["splits"]) * rows * d * 4]
    return sum(N.up256(p) for p in parts) + 256


def score_error(a, b, qa, qb, V):
    """max |S32 - S64| over the three products, by torch on the CPU"""
    worst = 0.0
    for x, y in ((a, b), (a, qb[:V]), (b, qa[:V])):
        if y.shape[0]:
            x, y = x.cpu(), y.cpu()
            worst = max(worst, float(((x.float() @ y.float().T).double() - x.double() @ y.double().T).abs().max()))
    return worst


def reference(a, b, qa, qb, V, shards, T, coef, s_err):
    """float64 on the device of a and b [n, d] over the whole batch.  Returns (ref, bnd): loss_rows, da_loc, db_loc [n ...] whole;
    colsum, db_all, dT lists, one entry per shard (the shard's share); db_all_sum the shares added up, with the summed bounds."""
    a64, b64 = a.double(), b.double()
    ka, kb = qa[:V].double(), qb[:V].double()           # the keys: the slots at or above V are no part of the definition
    n, d = a64.shape
    q_cap = qa.shape[0]
    dev = a.device
    ct = coef / T
    idx = torch.arange(n, device=dev)
    SX, SU, SW = a64 @ b64.T, a64 @ kb.T, b64 @ ka.T
    xm = 0.0
    for S in (SX, SU, SW):
        if S.numel():
            xm = max(xm, float(torch.maximum(S.abs(), (S - 1.0).abs()).max()) / T)
    EX, EU, EW = torch.exp((SX - 1.0) / T), torch.exp((SU - 1.0) / T), torch.exp((SW - 1.0) / T)
    Da, Db = EX.sum(1) + EU.sum(1), EX.sum(0) + EW.sum(1)
    sii = SX[idx, idx]
    loss = (torch.log(Da) + 1.0 / T - sii / T) + (torch.log(Db) + 1.0 / T - sii / T)
    QX = EX / Da[:, None] + EX / Db[None, :]
    GX = QX.clone()
    GX[idx, idx] -= 2.0
    GU, GW = EU / Da[:, None], EW / Db[:, None]
    aa, ab, aka, akb = a64.abs(), b64.abs(), ka.abs(), kb.abs()
    geoms = [N.geometry(hi - lo, n, d) for lo, hi in shards]
    q_tiles = N.up256(q_cap) // 256
    Qp = N.up256(q_cap)
    eps_e = 4.0 * s_err / T + 6.0 * H * xm + 2.0 * H
    eps_lQ = eps_e + (12 + -(-q_tiles // 4)) * H
    eps_Db = eps_e + (max(max(15 + -(-g["m_tiles"] // 4), 12 + -(-q_tiles // 4)) for g in geoms) + 1 + len(shards) - 1) * H
    M = xm + 1.0 / T + math.log(n + V)
    flush = FLUSH * (1.0 + ct)
    ref = dict(loss_rows=loss, da_loc=torch.empty_like(a64), db_loc=torch.empty_like(a64), db_all=[], dT=[], colsum=[])
    bnd = dict(loss_rows=torch.empty_like(loss), da_loc=torch.empty_like(a64), db_loc=torch.empty_like(a64), db_all=[], dT=[], colsum=[])
    for (lo, hi), g in zip(shards, geoms):
        rows = hi - lo
        q_splits = N.da_splits(g["Rp"], Qp, d)
        eps_lX = eps_e + (12 + -(-g["n_tiles"] // 4)) * H
        eps_cs = eps_e + (15 + -(-g["m_tiles"] // 4)) * H
        eps_Da = max(eps_lX, eps_lQ) + H
        eps_w = eps_e + max(eps_Da, eps_Db) + 10.0 * H
        bnd["loss_rows"][lo:hi] = eps_Da + eps_Db + 2.0 * (4.0 * s_err / T + 2.0 * H * xm) + 12.0 * H * M
        ii, pos = torch.arange(rows, device=dev), idx[lo:hi]
        off_diag = ct * ((1.0 + EPS_P) ** 2 * (1.0 + eps_w) - 1.0)
        BX = off_diag * QX[lo:hi] + flush
        gd = GX[lo:hi][ii, pos].abs()
        BX[ii, pos] = ct * (EPS_P * gd + (1.0 + EPS_P) * (eps_w * QX[lo:hi][ii, pos] + 8.0 * H * gd)) + flush
        BU = off_diag * GU[lo:hi] + flush
        BW = off_diag * GW[lo:hi] + flush
        mX, mU, mW = ct * GX[lo:hi].abs() + BX, ct * GU[lo:hi] + BU, ct * GW[lo:hi] + BW
        nC, nQ, nR = (g["Cp"] + 32) * H, (Qp + 32) * H, (g["Rp"] + 32) * H
        # single-product bounds (the float32 accumulators dT is taken from), then the outputs
        bX1, bU1, bW1 = (BX + nC * mX) @ ab, (BU + nQ * mU) @ akb, (BW + nQ * mW) @ aka
        vX, vU, vW = ct * (GX[lo:hi] @ b64), ct * (GU[lo:hi] @ kb), ct * (GW[lo:hi] @ ka)
        ref["da_loc"][lo:hi] = vX + vU
        bnd["da_loc"][lo:hi] = (BX + (nC + nQ) * mX) @ ab + (BU + (nC + nQ) * mU) @ akb
        ref["db_loc"][lo:hi] = vW
        bnd["db_loc"][lo:hi] = bW1
        ref["db_all"].append(ct * (GX[lo:hi].T @ a64[lo:hi]))
        bnd["db_all"].append((BX + nR * mX).T @ aa[lo:hi])
        dT = -(1.0 / T) * float((a64[lo:hi] * (vX + vU)).sum() + (b64[lo:hi] * vW).sum())
        depth = 145 + -(-((g["splits"] + 2 * q_splits) * g["m_tiles"] * g["d_tiles"]) // 256)
        B = float((aa[lo:hi] * (bX1 + bU1)).sum() + (ab[lo:hi] * bW1).sum())
        Vv = float((aa[lo:hi] * (vX.abs() + vU.abs())).sum() + (ab[lo:hi] * vW.abs()).sum())
        ref["dT"].append(dT)
        bnd["dT"].append((B + depth * H * (Vv + B)) / T + 3.0 * H * abs(dT))
        cs = EX[lo:hi].sum(0)
        e_cs = torch.full_like(cs, eps_cs)
        cs[lo:hi] += EW[lo:hi].sum(1)
        e_cs[lo:hi] = max(eps_cs, eps_lQ) + H
        ref["colsum"].append(cs)
        bnd["colsum"].append(e_cs * cs)
    ref["db_all_sum"], bnd["db_all_sum"] = sum(ref["db_all"]), sum(bnd["db_all"])
    return ref, bnd


def autograd_check(a, b, qa, qb, V, T, coef):
    """largest |difference| between ``reference`` (one shard) and float64 autograd of the definition, relative to the largest
    gradient or to 1: (gradients, dT) -- float64 rounding only"""
    n = a.shape[0]
    x, y = a.double().requires_grad_(True), b.double().requires_grad_(True)
    t = torch.tensor(T, dtype=torch.float64, requires_grad=True)
    ka, kb = qa[:V].double(), qb[:V].double()
    la = torch.cat([x @ y.T, x @ kb.T], 1) / t
    lb = torch.cat([y @ x.T, y @ ka.T], 1) / t
    i = torch.arange(n)
    loss = coef * ((torch.logsumexp(la, 1) - la[i, i]).sum() + (torch.logsumexp(lb, 1) - lb[i, i]).sum())
    loss.backward()
    ref, _ = reference(a, b, qa, qb, V, [(0, n)], T, coef, 0.0)
    scale = max(float(x.grad.abs().max()), float(y.grad.abs().max()), 1.0)
    worst = max(float((ref["da_loc"] - x.grad).abs().max()), float((ref["db_loc"] + ref["db_all_sum"] - y.grad).abs().max())) / scale
    loss = float(loss.detach())
    worst = max(worst, abs(coef * float(ref["loss_rows"].sum()) - loss) / max(abs(loss), 1.0))
    return worst, abs(ref["dT"][0] - float(t.grad)) / max(abs(float(t.grad)), 1.0)


def ratios(got, ref, bnd, bf16=False):
    """largest |error| / bound per output over all shards (``got`` laid out as ``ref``; outputs it lacks are skipped).  Every
    element takes part; an error that is no number counts as infinite.  bf16: the gradients were rounded once more on the way
    out, 2^-8 |value| joins their bounds."""
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
            else:
                if bf16 and name in GRADS and name != "db_all_sum":
                    b = b + EPS_P * (r.abs() + b)
                elif bf16 and name == "db_all_sum":
                    b = b + EPS_P * sum(x.abs() + y for x, y in zip(ref["db_all"], bnd["db_all"]))
                err = (g.double() - r).abs()
                # (a bound of 0 -- an empty product, plan Q0 -- asks for the exact value: 0 / 0 counts as 0, anything / 0 as infinite)
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
MUTATIONS = {"one_direction": "colsum", "swapped": "loss_rows", "v_ignored": "loss_rows", "lw_local": "colsum", "by_value": "loss_rows",
             "ring_order": "da_loc", "newest": "loss_rows"}


def emulate(a, b, qa, qb, V, shards, T, coef, mutation=None, upstream=1.0, push_order=None):
    """The kernels' arithmetic on the CPU: float32 scores, exponentials and sums, the slots at or above V 0 in the stored E and in
    the row sum BY INDEX, Da = lX + lU, col_sums = cX with lW added on the shard's own range, their float32 sum over the shards; E
    rounded to bf16 once, the weights a second time, the partner's weight from the float32 ediag; float32 products over ALL q_cap
    slots, two of them added in float32 where they share an output.  Output laid out as ``reference`` (without db_all_sum).
    mutation:
      "one_direction"  the queue serves the anchors of view a only (no W block: lW = 0, db_loc = 0)
      "swapped"        U is taken against Qa and W against Qb
      "v_ignored"      every slot counts, the garbage with them
      "lw_local"       lW is added at the local index i instead of off + i
      "by_value"       a queue key whose float32 score equals the partner's is left out (the twin with it)
      "ring_order"     the product W_U Qb runs over the keys in push order from slot 0 (``push_order``: [q_cap] slot of the k-th
                       oldest key) while E_U was formed in slot order
    ("newest" is a mutation of the ring, ``ring_push``: the caller hands over the queue it leaves.)"""
    assert mutation is None or mutation in MUTATIONS
    f32 = torch.float32
    inv = torch.tensor(1.0, dtype=f32) / torch.tensor(T, dtype=f32)
    scale2 = inv * torch.tensor(1.4426950408889634, dtype=f32)
    af, bf = a.float(), b.float()
    ua, ub = (qb.float(), qa.float()) if mutation == "swapped" else (qa.float(), qb.float())       # ub: U's keys, ua: W's
    n, q_cap = a.shape[0], qa.shape[0]
    live = torch.arange(q_cap) < (q_cap if mutation == "v_ignored" else V)
    state, cols = [], []
    for lo, hi in shards:
        rows = hi - lo
        pos = torch.arange(lo, hi)
        SX = af[lo:hi] @ bf.T
        st = dict(EX=torch.exp2(SX * scale2 - scale2))
        sp = SX[torch.arange(rows), pos]
        for name, x, k in (("U", af, ub), ("W", bf, ua)):
            S = x[lo:hi] @ k.T
            E = torch.exp2(S * scale2 - scale2)
            gone = ~live[None, :].expand_as(S)
            if mutation == "by_value":
                gone = gone | (S == sp[:, None])
            E = E.masked_fill(gone, 0.0)
            if mutation == "one_direction" and name == "W":
                E = torch.zeros_like(E)
            st["E" + name], st["l" + name] = E, E.sum(1)
        st["Da"] = st["EX"].sum(1) + st["lU"]
        c = st["EX"].sum(0).clone()
        if mutation == "lw_local":
            c[0:rows] = c[0:rows] + st["lW"]
        else:
            c[lo:hi] = c[lo:hi] + st["lW"]
        cols.append(c)
        state.append(st)
    c_tot = cols[0]
    for c in cols[1:]:
        c_tot = c_tot + c
    ct = torch.tensor(coef, dtype=f32) * inv * torch.tensor(upstream, dtype=f32)
    out = dict(loss_rows=torch.empty(n), colsum=cols, da_loc=torch.empty(a.shape, dtype=f32), db_loc=torch.empty(a.shape, dtype=f32),
               db_all=[], dT=[])
    # the products meet every slot: a weight of exactly 0 on a finite row is 0
    kU, kW = ub, ua
    if mutation == "ring_order":
        kU = ub[push_order]
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
        WU = (ct * (st["EU"].to(torch.bfloat16).float() * u[:, None])).to(torch.bfloat16).float()
        WW = (ct * (st["EW"].to(torch.bfloat16).float() * uz[:, None])).to(torch.bfloat16).float()
        dX, dU, dW = WX @ bf, WU @ kU, WW @ kW
        out["da_loc"][lo:hi] = dX + dU
        out["db_loc"][lo:hi] = dW
        out["db_all"].append(WX.T @ af[lo:hi])
        out["dT"].append(-float(((af[lo:hi] * dX).sum() + (af[lo:hi] * dU).sum() + (bf[lo:hi] * dW).sum()) * inv))
    return out
