"""Set plan, float64 reference, derived bounds and a CPU emulation shared by tests/test_supcon_ml_cpu.py and
tests/test_supcon_ml_gpu.py: the streaming multi-label supervised contrastive loss (aecf_supcon_ml_flash.hip on
aecf_flash_stream.h).  Shapes, split geometry, embeddings and sentinel columns are those of tests/nce_stream_cases.py (cases A-H),
imported, not copied; this module adds the class sets.  Nothing here touches a GPU; every function works on the device of the
tensors it is given.

One direction (ct = coef / T, Mn = w / W):
    w(i, j) = 1 if j == off + i, else [A_i & B_j != 0] ("overlap") or |A_i & B_j| / |A_i | B_j| ("jaccard", 0 for an empty union)
    W_i = sum_j w(i, j),   loss_i = lse_i - (1 / W_i) sum_j w(i, j) x_ij,   G = P - Mn,   dq = ct G k,   dk = ct G^T q,
    dT = -(1/T) sum q . dq
A set is one int64 word, bit c = class c (class 63 = the sign bit).

The set plan (``sets``), deterministic per case; {..} are classes:
  * local row i carries {i % 7, 7 + i % 5}, and {40 + i % 3} too when i is even; rows with i % 4 == 3 are unlabeled (empty).  Rows
    overlap partly in many ways -- the Jaccard weights among them are 1/5, 1/4, 1/3, 1/2, 2/3 and 1 -- and rows such as 0 and 6
    share class 40 and nothing else: a class >= 32 only;
  * the heavy row (row 1 where rows > 2, else row 0) carries {25, 44, 63}, classes no other local row uses;
  * every sentinel column (a copy of the positive key of its sentinel row, sitting on a split or tile boundary) carries its row's
    set without that set's lowest class, plus class 62; an unlabeled sentinel row first gets {r % 7, 7 + r % 5, 40 + r % 3}.  The
    sentinel's weight is 1 under "overlap" and 1/3 or 1/2 under "jaccard": a weighted positive on every boundary the plan names;
  * 60 (at most) of the remaining outside columns, evenly spaced from the first to the last of them and so over the splits (a
    last split that holds only a sentinel or local rows has its weighted positives already), carry {33 + j % 4, 63}: they share
    class 63 alone with the heavy row (a class >= 32 only, and the sign bit of the word), weight 1/4;
  * six further outside columns carry {25, 50 + j % 5}: against the heavy row they differ only in classes >= 32 (the low words
    are equal), weight 1/4 -- the popcounts of the low words alone would say 1;
  * of the other outside columns every 4th carries {j % 7, 7 + j % 5} (and {40 + j % 3} when j % 8 == 0) and the rest are empty.
  sq = sk[off : off + rows].  Case "C9" is case C with sq[2] = {20, 45}, which no key holds, while sk[off + 2] keeps its own:
  the partner still has weight 1, by index (only the C ABI can express it).

The bounds are elementwise and derived from the roundings of the design, to first order, never from results (u = 2^-24; eps_x,
EPS_P, FLUSH as in nce_stream_cases; n_i = the number of keys of row i with a weight that is not 0):
  a weight w is one correctly rounded float32 quotient (relative error u; 0 and 1 are exact); W is a float32 sum of n_i weights in
  some fixed order (relative error (n_i - 1) u beside the u of its terms) and 1 / W one more rounding: relative error
  (n_i + 1) u.  The float32 sum of the w x carries per term the u of w, of the product and (n_i - 1) u of the sum; its product with
  1 / W one more rounding.  lse and the x inside the mean carry eps_x each.  A weight ct (exp(x - lse) - w / W) is rounded to bf16
  once (EPS_P), its exponential carries 2 eps_x (x and lse), its w / W the u of w, the (n_i + 1) u of 1 / W, the rounding of the
  product and of the difference: (n_i + 4) u; a weight below the smallest normal float32 may flush.
  |d loss_i|  <= 2 eps_x + (2 n_i + 3) u sum_j Mn_ij |x_ij|
  |d dq[i,c]| <= ct (EPS_P + 2 eps_x) (|G| |k|)[i,c] + 2 ct eps_x (P |k|)[i,c] + ct u ((n + 4) Mn |k|)[i,c] + ct FLUSH sum_j |k[j,c]|
  |d dk[j,c]| <= the same with G, P, (n + 4) Mn transposed and |q| for |k|
  |d dT|      <= (1/T) sum |q| bound_dq
With one-hot sets (n_i = the count of supcon_cases) these are the bounds of tests/supcon_cases.py with (n_i + 4) u for its 2u and
(2 n_i + 3) u Mn for its 2u match.  The implementation rounds where the design says (aecf_supcon_ml_flash.hip); the bounds carry
no further factor."""
import functools

import torch

from tests import nce_stream_cases as C

U = 2.0 ** -24
TEMPS = (0.07, 0.005)
WEIGHTINGS = ("overlap", "jaccard")
CASE_IDS = list(C.CASES) + ["C9"]
RULES = ("and32", "pop_lo", "swap", "partner_by_sets", "empty_match")      # the broken rules of ``weights``
HEAVY = (25, 44, 63)
C9_SET = (20, 45)


def base(cid):
    """the case of nce_stream_cases a case here takes its shape and embeddings from"""
    return "C" if cid == "C9" else cid


def mask(classes):
    """the int64 word of a set of classes (class 63 = the sign bit)"""
    v = 0
    for c in classes:
        v |= 1 << c
    return v - (1 << 64) if v >= 1 << 63 else v


def classes_of(word):
    word &= (1 << 64) - 1
    return [c for c in range(64) if word >> c & 1]


def local_set(i):
    return [] if i % 4 == 3 else [i % 7, 7 + i % 5] + ([40 + i % 3] if i % 2 == 0 else [])


def plan(rows, cols, off, sentinels):
    """key sets (a list of class lists, [cols]) of the plan above, the heavy row, its class-63 columns and its low-word twins"""
    sk = [[] for _ in range(cols)]
    for i in range(rows):
        sk[off + i] = local_set(i)
    heavy = 1 if rows > 2 else 0
    sk[off + heavy] = list(HEAVY)
    for j, r in sentinels:
        if not sk[off + r]:
            sk[off + r] = [r % 7, 7 + r % 5, 40 + r % 3]
        own = sorted(sk[off + r])
        sk[j] = own[1:] + [62]
    taken = {j for j, _ in sentinels}
    outside = [j for j in range(cols) if not (off <= j < off + rows) and j not in taken]
    n_large = min(60, len(outside))
    large = sorted({outside[t * (len(outside) - 1) // max(1, n_large - 1)] for t in range(n_large)})
    for j in large:
        sk[j] = [33 + j % 4, 63]
    rest = [j for j in outside if j not in set(large)]
    twins = rest[3::11][:6]
    for j in twins:
        sk[j] = [25, 50 + j % 5]
    for j in rest:
        if j not in set(twins) and j % 4 == 0:
            sk[j] = [j % 7, 7 + j % 5] + ([40 + j % 3] if j % 8 == 0 else [])
    return sk, heavy, large, twins


@functools.lru_cache(maxsize=None)
def sets(cid):
    """dict(sq [rows], sk [cols] int64 words (CPU), heavy, large, twins) of a case"""
    (rows, cols, off, _), _, _ = C.CASES[base(cid)]
    c = C.make_case(base(cid))
    sk, heavy, large, twins = plan(rows, cols, off, c["sentinels"])
    sk = torch.tensor([mask(s) for s in sk], dtype=torch.int64)
    sq = sk[off:off + rows].clone()
    if cid == "C9":
        sq[2] = mask(C9_SET)
    return dict(sq=sq, sk=sk, heavy=heavy, large=large, twins=twins)


def unpack(words):
    """int64 words [n] -> float64 multi-hot [n, 64] (an arithmetic shift and a mask: the sign bit is class 63)"""
    return ((words[:, None] >> torch.arange(64, device=words.device)[None, :]) & 1).double()


def pack_torch(multi_hot):
    """the packing restated in torch: [b, C <= 64] of any dtype, nonzero = member -> int64 words [b]"""
    member = (multi_hot != 0).to(torch.int64)
    word = torch.zeros(multi_hot.shape[0], dtype=torch.int64, device=multi_hot.device)
    for c in range(multi_hot.shape[1]):
        word |= member[:, c] << c                                 # (1 << 63 wraps to the sign bit)
    return word


def counts(sq, sk):
    """(|A & B|, |A | B|, the same over the classes < 32 only) as float64 [rows, cols]: exact small integers"""
    mq, mk = unpack(sq), unpack(sk)
    inter = mq @ mk.T
    union = mq.sum(1)[:, None] + mk.sum(1)[None, :] - inter
    inter_lo = mq[:, :32] @ mk[:, :32].T
    union_lo = mq[:, :32].sum(1)[:, None] + mk[:, :32].sum(1)[None, :] - inter_lo
    return inter, union, inter_lo, union_lo


def weights(sq, sk, off, weighting, rule=None, single=False):
    """The weight matrix [rows, cols]: float64 with exact quotients, or (``single``) the float32 the kernels form -- the quotient
    of two float32 integers, correctly rounded.  ``rule``: one of RULES, what a wrong implementation would compute:
      and32            the and of the low 32 bits only
      pop_lo           (jaccard) both popcounts of the low 32 bits only
      swap             the other weighting
      partner_by_sets  the partner weighted by its sets like any key
      empty_match      two empty sets match with weight 1"""
    assert weighting in WEIGHTINGS and rule in (None,) + RULES
    inter, union, inter_lo, union_lo = counts(sq, sk)
    if rule == "swap":
        weighting = WEIGHTINGS[1 - WEIGHTINGS.index(weighting)]
    if rule == "and32":
        inter = inter_lo
    if rule == "pop_lo" and weighting == "jaccard":
        inter, union = inter_lo, union_lo
    if weighting == "overlap":
        w = (inter > 0).double()
    else:
        num, den = inter, torch.where(union > 0, union, torch.ones_like(union))
        w = (num.float() / den.float()).double() if single else num / den
    if rule == "empty_match":
        w = torch.where(union == 0, torch.ones_like(w), w)
    if rule != "partner_by_sets":
        rows = sq.shape[0]
        i = torch.arange(rows, device=sq.device)
        w[i, off + i] = 1.0
    return w.float() if single else w


def workspace_bytes_py(rows, cols, d):
    """dq partials, (m, l, weight sum, weighted-x sum) of `rule` splits, lse, 1 / W and q . dq of every row, 1024 spare bytes"""
    rule = C.flash_split_py(rows, cols)[0]
    return (rule * rows * (d + 4) + 3 * rows) * 4 + 1024


def reference(q, k, w, T, coef):
    """float64 of one direction on the device of q and k; ``w``: the float64 weight matrix"""
    q, k = q.double(), k.double()
    x = (q @ k.T) / T
    lse = torch.logsumexp(x, dim=1)
    Mn = w / w.sum(dim=1, keepdim=True)
    loss_rows = lse - (Mn * x).sum(dim=1)
    P = torch.exp(x - lse[:, None])
    G = P - Mn
    ct = coef / T
    dq = ct * (G @ k)
    dk = ct * (G.T @ q)
    dT = -(1.0 / T) * float((q * dq).sum())
    return dict(x=x, loss_rows=loss_rows, P=P, G=G, Mn=Mn, n=(w != 0).sum(dim=1).double(), dq=dq, dk=dk, dT=dT)


def bounds(ref, q, k, T, coef, ex):
    """the elementwise bounds of the module docstring; ``ex`` = eps_x"""
    aq, ak = q.double().abs(), k.double().abs()
    ct = coef / T
    P, aG, Mn, n = ref["P"], ref["G"].abs(), ref["Mn"], ref["n"]
    b_loss = 2 * ex + (2 * n + 3) * U * (Mn * ref["x"].abs()).sum(dim=1)
    nMn = (n + 4)[:, None] * Mn
    b_dq = ct * (C.EPS_P + 2 * ex) * (aG @ ak) + 2 * ct * ex * (P @ ak) + U * ct * (nMn @ ak) + ct * C.FLUSH * ak.sum(0)
    b_dk = ct * (C.EPS_P + 2 * ex) * (aG.T @ aq) + 2 * ct * ex * (P.T @ aq) + U * ct * (nMn.T @ aq) + ct * C.FLUSH * aq.sum(0)
    return dict(loss_rows=b_loss, dq=b_dq, dk=b_dk, dT=float((aq * b_dq).sum()) / T)


def slim(ref):
    """a reference without its rows x cols blocks (what a cached entry keeps)"""
    return {n: ref[n] for n in ("loss_rows", "dq", "dk", "dT")}


def emulate(q, k, w32, T, coef):
    """The design's arithmetic on the CPU: float32 scores and exponents, the float32 weights ``w32`` (``weights(..., single=True)``
    -- of a broken rule to see what it does to the outputs), float32 sums of w and of w x, 1 / W, weights
    ((exp(x - lse) - w inv_W) ct) rounded to bf16, float32 sums."""
    qf, kf = q.float(), k.float()
    inv_t = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(T, dtype=torch.float32)
    x = (qf @ kf.T) * inv_t
    m = x.max(dim=1).values
    lse = m + torch.log(torch.exp(x - m[:, None]).sum(dim=1))
    inv_w = torch.tensor(1.0, dtype=torch.float32) / w32.sum(dim=1)
    loss_rows = lse - (x * w32).sum(dim=1) * inv_w
    ct = torch.tensor(coef, dtype=torch.float32) * inv_t
    wgt = ((torch.exp(x - lse[:, None]) - w32 * inv_w[:, None]) * ct).to(torch.bfloat16).float()
    dq = wgt @ kf
    dk = wgt.T @ qf
    dT = -float((qf * dq).sum(dim=1).sum() * inv_t)
    return dict(loss_rows=loss_rows, dq=dq, dk=dk, dT=dT)


def outside(ratios):
    """a set of ratios leaves the bounds: some ratio above 1, or not a number (a row without any weight divides by zero)"""
    return any(not (v <= 1.0) for v in ratios.values())


def one_hot_sets(labels):
    """int64 class labels (< 64; negative = unlabeled) -> the one-hot words (0 for unlabeled)"""
    lab = labels.clamp_min(0)
    return torch.where(labels >= 0, torch.ones_like(labels) << lab, torch.zeros_like(labels))
