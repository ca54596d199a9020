"""Case table, inputs, float64 reference, bounds and a CPU emulation shared by tests/test_supcon_pool_cpu.py and
tests/test_supcon_pool_gpu.py: the pooled contrastive losses (aecf_supcon_pool_fwd_bwd: the SELF instances of
aecf_supcon_flash.hip on aecf_flash_stream.h).  The split rule, the embeddings' construction, eps_x and the ratios are those of
tests/nce_stream_cases.py, the match rule, the reference's formulas and the bounds those of tests/supcon_cases.py, imported, not
copied; this module adds the excluded key.  Nothing here touches a GPU; every function works on the device of its tensors.

One direction (ct = coef / T, Mn = match / n), with excl(i, j) = (j == self_off + i):
    match(i, j) = not excl and ((j == off + i) or (lq[i] >= 0 and lq[i] == lk[j])),   n_i = sum_j match(i, j)
    x_ij = q_i . k_j / T, -inf where excl;   loss_i = lse_i - (1 / n_i) sum_j match(i, j) x_ij
    P = softmax_j x (0 where excl),  G = P - Mn,  dq = ct G k,  dk = ct G^T q,  dT = -(1/T) sum q . dq

Inputs (``make_case``), built as nce_stream_cases.make_case builds its own: unit bf16 rows, k[off : off + rows] at cosine 0.8 to
q, and k[self_off : self_off + rows] = q exactly -- the excluded key is the anchor, the highest score 1/T of its row.  Labels:
local row i carries class i // 3, rows with i % 4 == 3 are unlabeled (-1); both the partner and the self key of a row carry its
label (so a row's self key is a positive by label unless the exclusion comes first, and the self keys and partners of the other
rows of its class are positives from "either view"); with rows > 2, every 9th key outside both ranges (60 at most) carries class
0, the class of rows 0 .. 2: positives spread over the splits; every other key is unlabeled.

The bounds are supcon_cases.bounds unchanged, on a match matrix stripped of the excluded key and a P that is zero there: the
exclusion removes terms from every sum the bounds are sums over and adds no rounding.  The emulation of the design stays at or
below 0.96 of every bound on this table at both temperatures; an emulation that forgets the exclusion leaves the bounds by
2 10^4 (loss_rows), 7 10^2 (dq), 10^5 (dk) and 30 (dT) at least, one that counts the excluded key as a positive by 2 10^4
(loss_rows) and 2 10^4 (dk) at least (tests/test_supcon_pool_cpu.py prints the figures); the bounds carry no factor."""
import functools

import torch

from tests import nce_stream_cases as C
from tests import supcon_cases as S

TEMPS = S.TEMPS

# id: ((rows, cols, row_offset, self_offset, d), (rule, live, per, last), what it puts on an edge)
CASES = {
    "P1": ((1, 2, 0, 1, 128), (1, 1, 32, 2), "only the partner survives: the loss and every gradient exactly 0"),
    "P2": ((2, 513, 511, 0, 128), (2, 2, 288, 225), "self keys first in split 0, partners last in split 1"),
    "P3": ((65, 2200, 700, 1800, 256), (5, 5, 448, 408), "the real layout (b_all = 1100, a shard at 700); second row block holds "
                                                           "one row"),
    "P4": ((64, 7681, 31, 7617, 512), (16, 16, 512, 1), "the last split's only key is row 63's excluded key: an all -inf split"),
    "P5": ((200, 7697, 100, 7497, 768), (16, 16, 512, 17), "the last sub-tile's only key is row 199's excluded key; DQ in column "
                                                             "parts"),
    "P6": ((33, 7201, 3600, 0, 1024), (15, 15, 512, 33), "self keys in the first tiles; d = 1024 CSPLIT"),
    "P7": ((63, 300, 237, 100, 384), (1, 1, 320, 300), "one split; off + rows == cols; DK streams 32 + 31 rows"),
}
CASE_IDS = list(CASES)


@functools.lru_cache(maxsize=None)
def make_case(cid):
    """bf16 unit rows q [rows, d], k [cols, d], int64 labels lq [rows], lk [cols] (CPU) and the two offsets of a case"""
    (rows, cols, off, self_off, d), _, _ = CASES[cid]
    g = torch.Generator().manual_seed(5000 + CASE_IDS.index(cid))
    q = C._unit(torch.randn(rows, d, generator=g))
    k = C._unit(torch.randn(cols, d, generator=g))
    k[off:off + rows] = C._unit(0.8 * q + 0.6 * C._unit(torch.randn(rows, d, generator=g)))
    q, k = q.to(torch.bfloat16), k.to(torch.bfloat16)
    k[self_off:self_off + rows] = q
    lq = torch.tensor([-1 if i % 4 == 3 else i // 3 for i in range(rows)], dtype=torch.int64)
    lk = torch.full((cols,), -1, dtype=torch.int64)
    lk[off:off + rows] = lq
    lk[self_off:self_off + rows] = lq
    if rows > 2:
        outside = [j for j in range(cols) if not (off <= j < off + rows) and not (self_off <= j < self_off + rows)]
        lk[outside[::9][:60]] = 0
    return dict(q=q, k=k, lq=lq, lk=lk, off=off, self_off=self_off)


def excluded(rows, cols, self_off, device=None):
    """bool [rows, cols]: the one key of every row that takes no part"""
    j = torch.arange(cols, device=device)
    return j[None, :] == (self_off + torch.arange(rows, device=device))[:, None]


def match_matrix(lq, lk, off, self_off):
    """supcon_cases.match_matrix with the excluded key stripped: the exclusion comes before the label"""
    return S.match_matrix(lq, lk, off) & ~excluded(lq.shape[0], lk.shape[0], self_off, lq.device)


@functools.lru_cache(maxsize=None)
def score_error(cid):
    """max |S32 - S64| of a case, both products by torch on the CPU"""
    c = make_case(cid)
    s32 = c["q"].float() @ c["k"].float().T
    return float((s32.double() - c["q"].double() @ c["k"].double().T).abs().max())


def reference(q, k, match, excl, T, coef):
    """float64 of one direction on the device of q and k: supcon_cases.reference with x = -inf on the excluded key.  The ``x``
    returned holds 0 there (no match, P = 0: it enters no bound), so that supcon_cases.bounds takes the result as it is."""
    q, k = q.double(), k.double()
    x = ((q @ k.T) / T).masked_fill(excl, float("-inf"))
    lse = torch.logsumexp(x, dim=1)
    P = torch.exp(x - lse[:, None])
    x = x.masked_fill(excl, 0.0)
    M = match.double()
    Mn = M / M.sum(dim=1, keepdim=True)
    loss_rows = lse - (Mn * x).sum(dim=1)
    G = P - Mn
    ct = coef / T
    dq = ct * (G @ k)
    dk = ct * (G.T @ q)
    dT = -(1.0 / T) * float((q * dq).sum())
    return dict(x=x, loss_rows=loss_rows, P=P, G=G, Mn=Mn, dq=dq, dk=dk, dT=dT)


def bounds(ref, q, k, match, T, coef, ex):
    """supcon_cases.bounds, unchanged (``match`` without the excluded key, ``ref`` of ``reference``)"""
    return S.bounds(ref, q, k, match, T, coef, ex)


def emulate(q, k, match, excl, T, coef):
    """supcon_cases.emulate with the exclusion: float32 scores, -inf on ``excl`` for the maximum, the sum and the weights;
    float32 count / sum / 1 / n over ``match``; weights ((exp(x - lse) - match inv_n) ct) rounded to bf16, 0 on ``excl``; float32
    sums.  ``excl`` all False is a kernel that forgets the exclusion; a ``match`` that still holds the excluded key is one whose
    label match comes before it."""
    qf, kf = q.float(), k.float()
    inv_t = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(T, dtype=torch.float32)
    x = (qf @ kf.T) * inv_t
    xm = x.masked_fill(excl, float("-inf"))
    m = xm.max(dim=1).values
    lse = m + torch.log(torch.exp(xm - m[:, None]).sum(dim=1))
    mf = match.float()
    inv_n = torch.tensor(1.0, dtype=torch.float32) / mf.sum(dim=1)
    loss_rows = lse - (x * mf).sum(dim=1) * inv_n
    ct = torch.tensor(coef, dtype=torch.float32) * inv_t
    w = ((torch.exp(xm - lse[:, None]) - mf * inv_n[:, None]) * ct).to(torch.bfloat16).float()
    dq = w @ kf
    dk = w.T @ qf
    dT = -float((qf * dq).sum(dim=1).sum() * inv_t)
    return dict(loss_rows=loss_rows, dq=dq, dk=dk, dT=dT)
