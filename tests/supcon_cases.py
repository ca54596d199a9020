"""Label plan, float64 reference, derived bounds and a CPU emulation shared by tests/test_supcon_cpu.py and
tests/test_supcon_gpu.py: the streaming supervised contrastive loss (aecf_supcon_flash.hip on aecf_flash_stream.h).  Shapes,
split geometry, embeddings and sentinel columns are those of tests/nce_stream_cases.py (cases A-H), imported, not copied; this
module adds the labels.  Nothing here touches a GPU; every function works on the device of the tensors it is given.

One direction (ct = coef / T, Mn = match / n):
    match(i, j) = (j == off + i) or (lq[i] >= 0 and lq[i] == lk[j]),   n_i = sum_j match(i, j)
    loss_i = lse_i - (1 / n_i) sum_j match(i, j) x_ij,   G = P - Mn,   dq = ct G k,   dk = ct G^T q,   dT = -(1/T) sum q . dq

The label plan (``labels``), deterministic per case:
  * local row i carries class i // 3, rows with i % 4 == 3 are unlabeled (-1);
  * every sentinel column (a copy of the positive key of its sentinel row, sitting on a split or tile boundary) takes the class
    of that row, which first gets class 100000 + r if it was unlabeled: a positive by label on every boundary the plan names;
  * the large class 2^40 on every 9th remaining column outside the positive range (60 at most), joined by local row 1 when
    rows > 2: one row with many positives spread over the splits;
  * distractor classes 2^40 + 2^32 (1 + j % 5) on every 11th remaining outside column from the 4th: no row owns them, and they
    differ from the large class only above bit 31 -- a 32-bit compare makes them positives of row 1;
  * every other outside column is unlabeled (-1): a key no row may match by label, which "unlabeled rows are one class" would.
  lq = lk[off : off + rows].  Case "C9" is case C with lq[2] set to a distractor class while lk[off + 2] keeps its own: the
  partner still counts, by index (only the C ABI can express it).

The bounds are elementwise and derived from the roundings of the design, never from results (u = 2^-24; eps_x, EPS_P, FLUSH as in
nce_stream_cases):
  the exponent x - lse carries eps_x; lse and the mean of the matched x carry eps_x each, and the float32 sum of the matched x and
  its product with the rounded 1 / n two roundings per term; a weight ct (exp(x - lse) - match / n) is rounded to bf16 once
  (EPS_P), its exponential carries 2 eps_x (x and lse), its match / n the rounding of 1 / n and of the difference (2u); a weight
  below the smallest normal float32 may flush.
  |d loss_i|  <= 2 eps_x + 2u sum_j match(i,j) |x_ij|
  |d dq[i,c]| <= ct (EPS_P + 2 eps_x) (|G| |k|)[i,c] + 2 ct eps_x (P |k|)[i,c] + 2u ct (Mn |k|)[i,c] + ct FLUSH sum_j |k[j,c]|
  |d dk[j,c]| <= the same with G, P, Mn transposed and |q| for |k|
  |d dT|      <= (1/T) sum |q| bound_dq
The implementation rounds where the design says (aecf_supcon_flash.hip); the bounds carry no further factor."""
import functools

import torch

from tests import nce_stream_cases as C

U = 2.0 ** -24
LARGE = 2 ** 40
TEMPS = (0.07, 0.005)
CASE_IDS = list(C.CASES) + ["C9"]


def base(cid):
    """the case of nce_stream_cases a case here takes its shape and embeddings from"""
    return "C" if cid == "C9" else cid


def distractor(j):
    return LARGE + 2 ** 32 * (1 + j % 5)


def plan(rows, cols, off, sentinels):
    """int64 key labels lk [cols] of the plan above, with the columns that got the large class and the distractor classes"""
    lk = torch.full((cols,), -1, dtype=torch.int64)
    for i in range(rows):
        lk[off + i] = -1 if i % 4 == 3 else i // 3
    for j, r in sentinels:
        if int(lk[off + r]) < 0:
            lk[off + r] = 100000 + r
        lk[j] = lk[off + r]
    taken = {j for j, _ in sentinels}
    outside = [j for j in range(cols) if not (off <= j < off + rows) and j not in taken]
    large = outside[::9][:60]
    for j in large:
        lk[j] = LARGE
    if rows > 2:
        lk[off + 1] = LARGE
    rest = [j for j in outside if j not in set(large)]
    distract = rest[3::11]
    for j in distract:
        lk[j] = distractor(j)
    return lk, large, distract


@functools.lru_cache(maxsize=None)
def labels(cid):
    """dict(lq [rows], lk [cols], large, distract) of a case (CPU, int64)"""
    (rows, cols, off, _), _, _ = C.CASES[base(cid)]
    c = C.make_case(base(cid))
    lk, large, distract = plan(rows, cols, off, c["sentinels"])
    lq = lk[off:off + rows].clone()
    if cid == "C9":
        lq[2] = distractor(distract[0])
    return dict(lq=lq, lk=lk, large=large, distract=distract)


def match_matrix(lq, lk, off):
    """bool [rows, cols]: the partner by index, or the same non-negative label"""
    rows, cols = lq.shape[0], lk.shape[0]
    j = torch.arange(cols, device=lq.device)
    partner = j[None, :] == (off + torch.arange(rows, device=lq.device))[:, None]
    return partner | ((lq[:, None] >= 0) & (lq[:, None] == lk[None, :]))


def workspace_bytes_py(rows, cols, d):
    """dq partials, (m, l, count, matched-x sum) of `rule` splits, lse, 1 / n and q . dq of every row, 1024 spare bytes"""
    rule = C.flash_split_py(rows, cols)[0]
    return (rule * rows * (d + 4) + 3 * rows) * 4 + 1024


def reference(q, k, match, T, coef):
    """float64 of one direction on the device of q and k"""
    q, k = q.double(), k.double()
    x = (q @ k.T) / T
    lse = torch.logsumexp(x, dim=1)
    M = match.double()
    Mn = M / M.sum(dim=1, keepdim=True)
    loss_rows = lse - (Mn * x).sum(dim=1)
    P = torch.exp(x - lse[:, None])
    G = P - Mn
    ct = coef / T
    dq = ct * (G @ k)
    dk = ct * (G.T @ q)
    dT = -(1.0 / T) * float((q * dq).sum())
    return dict(x=x, loss_rows=loss_rows, P=P, G=G, Mn=Mn, dq=dq, dk=dk, dT=dT)


def bounds(ref, q, k, match, T, coef, ex):
    """the elementwise bounds of the module docstring; ``ex`` = eps_x"""
    aq, ak = q.double().abs(), k.double().abs()
    ct = coef / T
    P, aG, Mn = ref["P"], ref["G"].abs(), ref["Mn"]
    b_loss = 2 * ex + 2 * U * (match.double() * ref["x"].abs()).sum(dim=1)
    b_dq = ct * (C.EPS_P + 2 * ex) * (aG @ ak) + 2 * ct * ex * (P @ ak) + 2 * U * ct * (Mn @ ak) + ct * C.FLUSH * ak.sum(0)
    b_dk = ct * (C.EPS_P + 2 * ex) * (aG.T @ aq) + 2 * ct * ex * (P.T @ aq) + 2 * U * ct * (Mn.T @ aq) + ct * C.FLUSH * aq.sum(0)
    return dict(loss_rows=b_loss, dq=b_dq, dk=b_dk, dT=float((aq * b_dq).sum()) / T)


def slim(ref):
    """a reference without its rows x cols blocks (what a cached entry keeps)"""
    return {n: ref[n] for n in ("loss_rows", "dq", "dk", "dT")}


def emulate(q, k, match, T, coef):
    """The design's arithmetic on the CPU: float32 scores and exponents, float32 count / sum / 1 / n, weights
    ((exp(x - lse) - match inv_n) ct) rounded to bf16, float32 sums.  ``match``: the match matrix the kernels are to use -- a
    mutated one shows what a wrong match rule does to the outputs."""
    qf, kf = q.float(), k.float()
    inv_t = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(T, dtype=torch.float32)
    x = (qf @ kf.T) * inv_t
    m = x.max(dim=1).values
    lse = m + torch.log(torch.exp(x - m[:, None]).sum(dim=1))
    mf = match.float()
    inv_n = torch.tensor(1.0, dtype=torch.float32) / mf.sum(dim=1)
    loss_rows = lse - (x * mf).sum(dim=1) * inv_n
    ct = torch.tensor(coef, dtype=torch.float32) * inv_t
    w = ((torch.exp(x - lse[:, None]) - mf * inv_n[:, None]) * ct).to(torch.bfloat16).float()
    dq = w @ kf
    dk = w.T @ qf
    dT = -float((qf * dq).sum(dim=1).sum() * inv_t)
    return dict(loss_rows=loss_rows, dq=dq, dk=dk, dT=dT)

