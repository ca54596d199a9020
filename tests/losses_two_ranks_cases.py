"""One global batch, float64 references, derived bounds and a CPU emulation of two ranks, shared by
tests/test_losses_two_ranks_cpu.py and tests/test_losses_two_ranks_gpu.py: the data-parallel paths of the label-aware and pooled
two-view losses of aecf_amd/losses.py (supervised_contrastive, nt_xent, pooled_supervised_contrastive, multilabel_contrastive,
pooled_multilabel_contrastive and fusion_objective over them).  Nothing here touches a GPU.

Inputs (``inputs``).  N = 301 rows at d = 128, bfloat16, dealt by dp.shard_bounds over two ranks: 151 and 150 rows, so rank 1's
offset (151) differs from its row count (150), the shard seam lies inside the first of two 256-wide column tiles, and d = 128 is a
width both the streaming and the tile forms serve.  Unit bf16 rows na, and nb at cosine 0.8 to its partner -- except every third
row (i % 3 == 2), whose partner lies at cosine 0.1: among 301 keys such a row's log-sum-exp is not its partner's score alone, so
ONE more key (the zero row a padded gather would leave behind) moves it by 10^-3, a hundred bounds, where a row at cosine 0.8 moves
by 10^-5, one bound -- with label sets that is the only trace an empty padding set leaves.  The views handed to the losses are
na, nb scaled row by row with powers of two (not unit-norm: the normalise backward has work to do).  T = 0.07, a learnable
one-element float32 tensor.
  labels: row i carries class i % 43 (seven rows a class, in both shards); rows with i % 4 == 3 are unlabeled, alternately -1 and
      -7; rows 5 (rank 0) and 200 (rank 1) carry class 60 and nobody else does: each one's only other member lives on the other
      rank.  Class 0 is in use (a zero-filled padding row would join it).  Every class is below 64, so the one-hot sets exist.
  sets: supcon_ml_cases.local_set(i) -- {i % 7, 7 + i % 5}, and {40 + i % 3} for even i, empty for i % 4 == 3: partial overlaps with
      Jaccard weights 1/5 .. 1 -- plus class 63 (the sign bit of the word) on rows with i % 16 == 1; as a multi-hot bool [N, 64] and
      as ready int64 words.

References (``reference``): the float64 references and elementwise bounds of the case modules, imported, on each rank's rows --
supcon_cases / supcon_pool_cases / supcon_ml_cases .reference and .bounds per rank and direction for the streaming forms,
supcon_tile_cases / ntxent_tile_cases / supcon_pool_tile_cases / supcon_ml_tile_cases / supcon_ml_pool_tile_cases .reference with
``shards`` = the two ranks for the tile forms.  Returned per view as a rank's own-row term and every rank's share of the
gathered-row term, dT per rank, the loss and its bound.

What a caller sees on two ranks, and its bound (``caller_view``, ``ratios``); half = 2^-8, every line one rounding:
  * every term a kernel hands back (an own-row gradient, a rank's share of a gathered-row gradient) has the case module's bound b
    and is rounded to bf16 once:                                   e = b + half (|v| + b)
  * where one gathered buffer collects two such terms (the pooled streaming form: its key pool is used by both directions), autograd
    adds them in bf16 BEFORE the exchange -- a rounding the single-rank tests of those forms name too:
                                                                   e = e1 + e2 + half (|v1| + |v2| + e1 + e2)
  * the reduce over ranks adds the two ranks' bf16 shares, one rounding:
                                                                   E = sum e_r + half (sum |v_r| + sum e_r)
  * autograd adds the own-row and the gathered-row contribution of a view in bf16:
                                                                   e_g = e_own + E + half (|own| + |gathered| + e_own + E)
  * the normalise backward: _after_normalise of tests/test_nce_stream_gpu.py, as
    test_supcon_gpu.py::test_supervised_contrastive_tensor_temperature_low_minimum has it;
  * the result is rounded to bf16:                                 + half |got|.
  The factor ``world`` the local term carries and the division by it are powers of two: no rounding.  The references take
  coef * world for the gradients (an upstream scalar multiplies ct, as the tile modules say) and are divided by world.
  loss: coef times the summed loss-row bounds, plus the float32 arithmetic between the rows and the returned value: the sum over a
      rank's rows (a tree: fewer than 2^4 roundings, as the single-rank tests count), the product with coef, the sum of two
      directions, the all-reduce over two ranks and the two operations of _dp_value -- fewer than 2^5 in all: 2^-19 |loss|.
  dT: the two ranks' shares added up against the summed bounds, plus 2^-23 |share| per rank for the float32 sum of a rank's two
      directions.
These bounds are derived, not fitted; they carry no factor.

Emulation (``emulate_two_ranks``): each rank's arithmetic on the CPU as the drivers arrange it -- its offset, its rows, the
gathered rows and labels or sets, float32 scores, exponentials, sums and quotients, the gradient weights rounded to bf16 (and the
stored exponentials of the tile forms), the [3, b_all] column statistics added over ranks, shares rounded to bf16, a bf16 reduce,
the bf16 sum with the own-row term, the normalise backward in float32, _dp_value.  ``mutation`` breaks one thing:
  offset_by_rank_times_rows   a rank's first row = rank x b_local (150 on rank 1, not the prefix sum 151)
  local_labels_as_keys        the labels / sets are not gathered: key j carries local row j's (none beyond b_local)
  self_and_partner_swapped    pooled forms: the two gathered views in each other's place -- the partner is excluded as the anchor
                              and the anchor's own copy counts as its partner
  stats_not_reduced           tile forms: every rank finishes with its own column statistics
  gathered_share_dropped      a rank keeps only its own share of a gathered-row gradient (no reduce)
  no_world_factor             the local term does not carry ``world``
  padding_label_zero          the zero row that pads the shorter shard to the longer one stays among the keys (index 301), as
                              class 0 / as an empty set"""
import functools

import torch

from aecf_amd import dp
from tests import nce_stream_cases as C
from tests import ntxent_tile_cases as X
from tests import supcon_cases as S
from tests import supcon_ml_cases as ML
from tests import supcon_ml_pool_tile_cases as MLP
from tests import supcon_ml_tile_cases as MLT
from tests import supcon_pool_cases as P
from tests import supcon_pool_tile_cases as PT
from tests import supcon_tile_cases as L
from tests.test_nce_stream_gpu import _after_normalise

N, D, T0, WORLD = 301, 128, 0.07, 2
SHARDS = [dp.shard_bounds(N, r, WORLD) for r in range(WORLD)]          # [(0, 151), (151, 301)]
HALF = 2.0 ** -8
F32 = torch.float32
BF16 = torch.bfloat16
PAIR_CLASS, PAIR_ROWS = 60, (5, 200)

MUTATIONS = ("offset_by_rank_times_rows", "local_labels_as_keys", "self_and_partner_swapped", "stats_not_reduced",
             "gathered_share_dropped", "no_world_factor", "padding_label_zero")

# form: (arrangement, what says which keys are positives)
FORMS = {
    "supcon_stream": ("cross_stream", "labels"),
    "supcon_tile": ("cross_tile", "labels"),
    "pool_stream": ("pool_stream", "labels"),
    "pool_tile": ("pool_tile", "labels"),
    "ntxent_stream": ("pool_stream", "none"),
    "ntxent_tile": ("pool_tile", "none"),
    "ml_stream_overlap": ("cross_stream", "overlap"),
    "ml_stream_jaccard": ("cross_stream", "jaccard"),
    "ml_tile_overlap": ("cross_tile", "overlap"),
    "ml_tile_jaccard": ("cross_tile", "jaccard"),
    "mlpool_tile_overlap": ("pool_tile", "overlap"),
    "mlpool_tile_jaccard": ("pool_tile", "jaccard"),
}

# route: (the function of aecf_amd.losses, its keyword arguments, which input says the positives, the form that serves it)
ROUTES = {
    "supcon_stream": ("supervised_contrastive", dict(low_memory=True), "labels", "supcon_stream"),
    "supcon_tile": ("supervised_contrastive", dict(low_memory=False), "labels", "supcon_tile"),
    "supcon_auto": ("supervised_contrastive", dict(low_memory=None), "labels", "supcon_tile"),
    "supcon_stream_int32": ("supervised_contrastive", dict(low_memory=True), "labels32", "supcon_stream"),
    "supcon_intra": ("supervised_contrastive", dict(intra_view=True), "labels", "pool_stream"),
    "ntxent_stream": ("nt_xent", dict(low_memory=True), None, "ntxent_stream"),
    "ntxent_tile": ("nt_xent", dict(low_memory=False), None, "ntxent_tile"),
    "pool_tile": ("pooled_supervised_contrastive", dict(low_memory=False), "labels", "pool_tile"),
    "pool_stream": ("pooled_supervised_contrastive", dict(low_memory=True), "labels", "pool_stream"),
    "ml_stream_overlap": ("multilabel_contrastive", dict(weighting="overlap", low_memory=True), "multi_hot", "ml_stream_overlap"),
    "ml_stream_jaccard": ("multilabel_contrastive", dict(weighting="jaccard", low_memory=True), "multi_hot", "ml_stream_jaccard"),
    "ml_tile_overlap": ("multilabel_contrastive", dict(weighting="overlap", low_memory=False), "words", "ml_tile_overlap"),
    "ml_tile_jaccard": ("multilabel_contrastive", dict(weighting="jaccard", low_memory=False), "words", "ml_tile_jaccard"),
    "mlpool_overlap": ("pooled_multilabel_contrastive", dict(weighting="overlap"), "words", "mlpool_tile_overlap"),
    "mlpool_jaccard": ("pooled_multilabel_contrastive", dict(weighting="jaccard"), "words", "mlpool_tile_jaccard"),
    "fusion_pool_tile": ("fusion_objective", dict(contrastive="supervised_pool", low_memory=False), "labels", "pool_tile"),
    # the pooled forms with every label -1: what nt_xent promises to have the bits of
    "pool_stream_unlabeled": ("pooled_supervised_contrastive", dict(low_memory=True), "unlabeled", "ntxent_stream"),
    "pool_tile_unlabeled": ("pooled_supervised_contrastive", dict(low_memory=False), "unlabeled", "ntxent_tile"),
}
ROUTE_IDS = list(ROUTES)
FUSION_TASK = 0.625
# (route, the route whose bits it must have)
SAME_BITS = (("supcon_auto", "supcon_tile"), ("supcon_stream_int32", "supcon_stream"), ("pool_stream", "supcon_intra"),
             ("ntxent_stream", "pool_stream_unlabeled"), ("ntxent_tile", "pool_tile_unlabeled"))


def applies(mutation, form):
    arrangement, kind = FORMS[form]
    if mutation == "self_and_partner_swapped":
        return arrangement.startswith("pool")
    if mutation == "stats_not_reduced":
        return arrangement.endswith("tile")
    if mutation == "local_labels_as_keys":
        return kind != "none"
    return True


# ---- the inputs ----
def label_plan():
    lab = torch.tensor([(-1 if (i // 4) % 2 == 0 else -7) if i % 4 == 3 else i % 43 for i in range(N)], dtype=torch.int64)
    for i in PAIR_ROWS:
        lab[i] = PAIR_CLASS
    return lab


def set_plan():
    return [ML.local_set(i) + ([63] if i % 16 == 1 else []) for i in range(N)]


@functools.lru_cache(maxsize=None)
def inputs():
    """dict(na, nb: the bf16 unit rows; za, zb: the views handed to the losses; labels int64 [N]; multi_hot bool [N, 64]; words
    int64 [N]) on the CPU"""
    g = torch.Generator().manual_seed(7301)
    a = C._unit(torch.randn(N, D, generator=g))
    noise = C._unit(torch.randn(N, D, generator=g))
    cos = torch.where(torch.arange(N) % 3 == 2, torch.tensor(0.1), torch.tensor(0.8))[:, None]
    b = C._unit(cos * a + (1.0 - cos * cos).sqrt() * noise)
    na, nb = a.to(BF16), b.to(BF16)
    scale = 2.0 ** torch.randint(-1, 3, (N, 1), generator=g).float()
    za, zb = (na.float() * scale).to(BF16), (nb.float() * scale.flip(0)).to(BF16)
    sets = set_plan()
    multi_hot = torch.zeros(N, 64, dtype=torch.bool)
    for i, s in enumerate(sets):
        multi_hot[i, s] = True
    words = torch.tensor([ML.mask(s) for s in sets], dtype=torch.int64)
    return dict(na=na, nb=nb, za=za, zb=zb, labels=label_plan(), multi_hot=multi_hot, words=words)


def meta_of(form, inp):
    """the labels / words a form reads (None: it reads none)"""
    kind = FORMS[form][1]
    if kind == "none":
        return None
    return inp["labels"] if kind == "labels" else inp["words"]


def score_errors(na, nb):
    """max |S32 - S64| of the a x b product, and of the three products of the pooled forms, by torch on the CPU"""
    err = lambda x, y: float(((x.float() @ y.float().T).double() - x.double() @ y.double().T).abs().max())
    e_ab = err(na, nb)
    return e_ab, max(e_ab, err(na, na), err(nb, nb))


# ---- float64 references, per rank ----
def _own(parts):
    """[N, d] from each rank's rows"""
    return torch.cat([v for v, _ in parts]), torch.cat([b for _, b in parts])


def reference(form, na, nb, meta, T=T0):
    """The float64 reference of the whole batch as two ranks form it.  ``na``, ``nb``: the bf16 unit rows the kernels read (CPU);
    ``meta``: the int64 labels or set words (None for NT-Xent).  Returns dict(loss, b_loss, a, b, dT, b_dT): for a view,
    ``own`` = (value, bound) [N, d] of the own-row term (None: the view's rows get none) and ``shares`` = per rank the list of
    (value, bound) [N, d] terms of its share of the gathered-row term (None: the view is not gathered); dT, b_dT per rank.
    Gradients and dT are those of ``world`` x the rank's term, divided by world."""
    arrangement, kind = FORMS[form]
    t, coef = C.used_temperature(T), 0.5 / N
    cw = coef * WORLD
    e_ab, e_pool = score_errors(na, nb)
    scale = lambda pair: (pair[0] / WORLD, pair[1] / WORLD)
    out = dict(a=dict(own=None, shares=None), b=dict(own=None, shares=None), dT=[], b_dT=[])
    if arrangement == "cross_stream":
        ex = C.eps_x(e_ab, t, N)
        rows_l, rows_b, own_a, own_b, sh_a, sh_b = [], [], [], [], [], []
        for lo, hi in SHARDS:
            if kind == "labels":
                m = S.match_matrix(meta[lo:hi], meta, lo)
                ab, ba = S.reference(na[lo:hi], nb, m, t, cw), S.reference(nb[lo:hi], na, m, t, cw)
                b_ab, b_ba = S.bounds(ab, na[lo:hi], nb, m, t, cw, ex), S.bounds(ba, nb[lo:hi], na, m, t, cw, ex)
            else:
                w = ML.weights(meta[lo:hi], meta, lo, kind)
                ab, ba = ML.reference(na[lo:hi], nb, w, t, cw), ML.reference(nb[lo:hi], na, w, t, cw)
                b_ab, b_ba = ML.bounds(ab, na[lo:hi], nb, t, cw, ex), ML.bounds(ba, nb[lo:hi], na, t, cw, ex)
            rows_l.append(ab["loss_rows"] + ba["loss_rows"])
            rows_b.append(b_ab["loss_rows"] + b_ba["loss_rows"])
            own_a.append(scale((ab["dq"], b_ab["dq"])))
            own_b.append(scale((ba["dq"], b_ba["dq"])))
            sh_a.append([scale((ba["dk"], b_ba["dk"]))])
            sh_b.append([scale((ab["dk"], b_ab["dk"]))])
            out["dT"].append((ab["dT"] + ba["dT"]) / WORLD)
            out["b_dT"].append((b_ab["dT"] + b_ba["dT"]) / WORLD)
        out["a"], out["b"] = dict(own=_own(own_a), shares=sh_a), dict(own=_own(own_b), shares=sh_b)
        loss_rows, b_rows = torch.cat(rows_l), torch.cat(rows_b)
    elif arrangement == "pool_stream":
        ex = C.eps_x(e_pool, t, 2 * N)
        lab = meta if meta is not None else torch.full((N,), -1, dtype=torch.int64)
        pool, lab_pool = torch.cat([nb, na]), torch.cat([lab, lab])
        rows_l, rows_b, own_a, own_b, sh_a, sh_b = [], [], [], [], [], []
        for lo, hi in SHARDS:
            rows = hi - lo
            ma, mb = P.match_matrix(lab[lo:hi], lab_pool, lo, N + lo), P.match_matrix(lab[lo:hi], lab_pool, N + lo, lo)
            ra = P.reference(na[lo:hi], pool, ma, P.excluded(rows, 2 * N, N + lo), t, cw)
            rb = P.reference(nb[lo:hi], pool, mb, P.excluded(rows, 2 * N, lo), t, cw)
            b_a, b_b = P.bounds(ra, na[lo:hi], pool, ma, t, cw, ex), P.bounds(rb, nb[lo:hi], pool, mb, t, cw, ex)
            rows_l.append(ra["loss_rows"] + rb["loss_rows"])
            rows_b.append(b_a["loss_rows"] + b_b["loss_rows"])
            own_a.append(scale((ra["dq"], b_a["dq"])))
            own_b.append(scale((rb["dq"], b_b["dq"])))
            # the key pool [b | a] is read by both directions: two terms per gathered view
            sh_b.append([scale((ra["dk"][:N], b_a["dk"][:N])), scale((rb["dk"][:N], b_b["dk"][:N]))])
            sh_a.append([scale((ra["dk"][N:], b_a["dk"][N:])), scale((rb["dk"][N:], b_b["dk"][N:]))])
            out["dT"].append((ra["dT"] + rb["dT"]) / WORLD)
            out["b_dT"].append((b_a["dT"] + b_b["dT"]) / WORLD)
        out["a"], out["b"] = dict(own=_own(own_a), shares=sh_a), dict(own=_own(own_b), shares=sh_b)
        loss_rows, b_rows = torch.cat(rows_l), torch.cat(rows_b)
    elif arrangement == "cross_tile":
        if kind == "labels":
            ref, bnd = L.reference(na, nb, meta, meta, SHARDS, t, cw, e_ab)
        else:
            ref, bnd = MLT.reference(na, nb, meta, meta, kind, SHARDS, t, cw, e_ab)
        out["a"] = dict(own=scale((ref["da"], bnd["da"])), shares=None)           # view a is never gathered
        out["b"] = dict(own=None, shares=[[scale((v, b))] for v, b in zip(ref["db"], bnd["db"])])
        out["dT"], out["b_dT"] = [v / WORLD for v in ref["dT"]], [v / WORLD for v in bnd["dT"]]
        loss_rows, b_rows = ref["loss_rows"], bnd["loss_rows"]
    else:
        if kind == "none":
            ref, bnd = X.reference(na, nb, SHARDS, t, cw, e_pool)
        elif kind == "labels":
            ref, bnd = PT.reference(na, nb, meta, SHARDS, t, cw, e_pool)
        else:
            ref, bnd = MLP.reference(na, nb, meta, meta, kind, SHARDS, t, cw, e_pool)
        for view, loc, gathered in (("a", "da_loc", "da_all"), ("b", "db_loc", "db_all")):
            out[view] = dict(own=scale((ref[loc], bnd[loc])), shares=[[scale((v, b))] for v, b in zip(ref[gathered], bnd[gathered])])
        out["dT"], out["b_dT"] = [v / WORLD for v in ref["dT"]], [v / WORLD for v in bnd["dT"]]
        loss_rows, b_rows = ref["loss_rows"], bnd["loss_rows"]
    out["loss"] = coef * float(loss_rows.sum())
    out["b_loss"] = coef * float(b_rows.sum()) + 2.0 ** -19 * abs(out["loss"])
    return out


def global_loss(form, na, nb, meta, T=T0):
    """the loss alone"""
    return reference(form, na, nb, meta, T)["loss"]


# ---- what a caller sees, and its bound ----
def caller_view(ref, za, zb, na, nb):
    """{"dza": (want, bound), "dzb": ...} [N, d]: the gradient on the views' rows (rank r sees its rows of it) and its bound
    before the final rounding, by the chain of the module docstring"""
    out = {}
    for name, view, z, zn in (("dza", "a", za, na), ("dzb", "b", zb, nb)):
        own, shares = ref[view]["own"], ref[view]["shares"]
        g = torch.zeros(N, D, dtype=torch.float64)
        e = torch.zeros(N, D, dtype=torch.float64)
        mag = torch.zeros(N, D, dtype=torch.float64)              # |own| + |gathered|: what the bf16 sum of the two rounds
        parts = 0
        if own is not None:
            v, b = own
            g, e, mag, parts = g + v, e + b + HALF * (v.abs() + b), mag + v.abs(), parts + 1
        if shares is not None:
            tot, e_tot, mag_tot = 0.0, 0.0, 0.0
            for terms in shares:
                v_s = sum(v for v, _ in terms)
                e_s = sum(b + HALF * (v.abs() + b) for v, b in terms)             # each term rounded to bf16 once
                if len(terms) > 1:
                    e_s = e_s + HALF * (sum(v.abs() for v, _ in terms) + e_s)     # added in bf16 before the exchange
                tot, e_tot, mag_tot = tot + v_s, e_tot + e_s, mag_tot + v_s.abs()
            e_tot = e_tot + HALF * (mag_tot + e_tot)                              # the reduce over ranks
            g, e, mag, parts = g + tot, e + e_tot, mag + tot.abs(), parts + 1
        if parts > 1:
            e = e + HALF * (mag + e)                                              # own rows + gathered rows, in bf16
        inv = 1.0 / z.double().norm(dim=1, keepdim=True)
        out[name] = _after_normalise(zn.double(), inv, g, e)
    return out


def ratios(ref, view, results):
    """largest |error| / bound per output.  ``results``: per rank dict(loss, dza [rows, d], dzb, dT) as a worker (or the
    emulation) returns them -- gradients and dT already divided by world."""
    r = dict(loss=max(abs(res["loss"] - ref["loss"]) for res in results) / ref["b_loss"])
    want_dt = sum(ref["dT"])
    b_dt = sum(ref["b_dT"]) + 2.0 ** -23 * sum(abs(v) for v in ref["dT"])
    r["dT"] = abs(sum(res["dT"] for res in results) - want_dt) / b_dt
    for name in ("dza", "dzb"):
        want, bound = view[name]
        worst = 0.0
        for (lo, hi), res in zip(SHARDS, results):
            got = res[name].double()
            q = (got - want[lo:hi]).abs() / (bound[lo:hi] + HALF * got.abs())
            worst = max(worst, float(q.max()) if bool(torch.isfinite(q).all()) else float("inf"))
        r[name] = worst
    return r


def outside(r):
    return any(not (v <= 1.0) for v in r.values())


# ---- the two ranks' arithmetic on the CPU ----
def _label_weights(kind, rmeta, kmeta, cols):
    """float32 [rows, cols]: what the labels / sets alone say (no partner, no exclusion)"""
    if kind == "none":
        return torch.zeros(rmeta, cols, dtype=F32)
    if kind == "labels":
        return ((rmeta[:, None] >= 0) & (rmeta[:, None] == kmeta[None, :])).float()
    inter, union, _, _ = ML.counts(rmeta, kmeta)
    if kind == "overlap":
        return (inter > 0).float()
    return inter.float() / torch.where(union > 0, union, torch.ones_like(union)).float()


def _direction(q, k, w, excl, inv_t, ct):
    """one streaming direction as supcon_cases.emulate / supcon_pool_cases.emulate / supcon_ml_cases.emulate form it: ``w`` the
    float32 weights with the partner's 1 in place and 0 on the excluded key"""
    x = (q @ k.T) * inv_t
    xm = x if excl is None else x.masked_fill(excl, float("-inf"))
    m = xm.max(dim=1).values
    lse = m + torch.log(torch.exp(xm - m[:, None]).sum(dim=1))
    inv_w = torch.tensor(1.0, dtype=F32) / w.sum(dim=1)
    loss_rows = lse - (x * w).sum(dim=1) * inv_w
    wgt = ((torch.exp(xm - lse[:, None]) - w * inv_w[:, None]) * ct).to(BF16).float()
    dq = wgt @ k
    return dict(loss_rows=loss_rows, dq=dq, dk=wgt.T @ q, dT=-((q * dq).sum(dim=1).sum() * inv_t))


def _rank_views(na, nb, meta, kind, mutation):
    views = []
    for r, (lo, hi) in enumerate(SHARDS):
        rows = hi - lo
        a_all, b_all = na.float(), nb.float()
        rmeta = rows if kind == "none" else meta[lo:hi]
        kmeta = None if kind == "none" else meta.clone()
        off = lo
        if mutation == "offset_by_rank_times_rows":
            off = r * rows
        if mutation == "local_labels_as_keys":
            kmeta = torch.full((N,), -1 if kind == "labels" else 0, dtype=torch.int64)
            kmeta[:rows] = meta[lo:hi]
        if mutation == "padding_label_zero":
            zero = torch.zeros(1, D, dtype=F32)
            a_all, b_all = torch.cat([a_all, zero]), torch.cat([b_all, zero])
            if kmeta is not None:
                kmeta = torch.cat([kmeta, torch.zeros(1, dtype=torch.int64)])
        swapped = mutation == "self_and_partner_swapped"
        if swapped:
            a_all, b_all = b_all, a_all
        views.append(dict(a_loc=na[lo:hi].float(), b_loc=nb[lo:hi].float(), a_all=a_all, b_all=b_all, rmeta=rmeta, kmeta=kmeta,
                          off=off, rows=rows, swapped=swapped))
    return views


def _stream_rank(v, arrangement, kind, inv_t, ct, coef):
    rows, cols, off = v["rows"], v["b_all"].shape[0], v["off"]
    i = torch.arange(rows)
    if arrangement == "cross_stream":
        w = _label_weights(kind, v["rmeta"], v["kmeta"], cols)
        w[i, off + i] = 1.0
        ab, ba = _direction(v["a_loc"], v["b_all"], w, None, inv_t, ct), _direction(v["b_loc"], v["a_all"], w, None, inv_t, ct)
        slots = dict(a_all=[ba["dk"]], b_all=[ab["dk"]])
    else:
        pool = torch.cat([v["b_all"], v["a_all"]])
        kpool = None if kind == "none" else torch.cat([v["kmeta"], v["kmeta"]])
        wl = _label_weights(kind, v["rmeta"], kpool, 2 * cols)
        wa, wb = wl.clone(), wl.clone()
        ex_a, ex_b = torch.zeros(rows, 2 * cols, dtype=torch.bool), torch.zeros(rows, 2 * cols, dtype=torch.bool)
        ex_a[i, cols + off + i], ex_b[i, off + i] = True, True
        wa[i, off + i], wb[i, cols + off + i] = 1.0, 1.0
        wa[ex_a], wb[ex_b] = 0.0, 0.0
        ab, ba = _direction(v["a_loc"], pool, wa, ex_a, inv_t, ct), _direction(v["b_loc"], pool, wb, ex_b, inv_t, ct)
        slots = dict(b_all=[ab["dk"][:cols], ba["dk"][:cols]], a_all=[ab["dk"][cols:], ba["dk"][cols:]])
    share = ab["loss_rows"].sum() * coef + ba["loss_rows"].sum() * coef
    return dict(share=share, own_a=ab["dq"], own_b=ba["dq"], slots=slots, dT=ab["dT"] + ba["dT"])


def _tile_ranks(views, pooled, kind, inv_t, ct, coef, reduce_stats):
    """the tile forms: block X = a_loc x b_all serves both directions through the column statistics ranks add up; the pooled
    forms add Y = a_loc x a_all and Z = b_loc x b_all, the anchor itself left out by index, Z's row statistics joining the
    column statistics on the rank's own range"""
    one = torch.tensor(1.0, dtype=F32)
    first = []
    for v in views:
        rows, cols, off = v["rows"], v["b_all"].shape[0], v["off"]
        i = torch.arange(rows)
        p = off + i
        blocks = {}
        for name, x, y in (("X", v["a_loc"], v["b_all"]),) + ((("Y", v["a_loc"], v["a_all"]), ("Z", v["b_loc"], v["b_all"])) if pooled else ()):
            s = x @ y.T
            e = torch.exp((s - 1.0) * inv_t)
            wl = _label_weights(kind, v["rmeta"], v["kmeta"], cols)
            wl[i, p] = 0.0                                       # the partner (X) and the anchor (Y, Z) go by index
            if name != "X":
                e[i, p] = 0.0
            blocks[name] = (s, e, wl)
        s, e, wl = blocks["X"]
        st = dict(dot=s[i, p].clone(), l=e.sum(1), rw=wl.sum(1), rwx=(wl * s).sum(1), c=e.sum(0), cw=wl.sum(0), cwx=(wl * s).sum(0))
        if pooled:
            s, e, wl = blocks["Y"]
            st["l"], st["rw"], st["rwx"] = st["l"] + e.sum(1), st["rw"] + wl.sum(1), st["rwx"] + (wl * s).sum(1)
            s, e, wl = blocks["Z"]
            st["c"][p] += e.sum(1)
            st["cw"][p] += wl.sum(1)
            st["cwx"][p] += (wl * s).sum(1)
        first.append((blocks, st, i, p))
    out = []
    for v, (blocks, st, i, p) in zip(views, first):
        c, cw, cwx = (sum(f[1][n] for f in first) for n in ("c", "cw", "cwx")) if reduce_stats else (st["c"], st["cw"], st["cwx"])
        u, vv, rn, rnc = one / st["l"], one / c, one / (one + st["rw"]), one / (one + cw)
        mean_r, mean_c = (st["dot"] + st["rwx"]) * rn, (st["dot"] + cwx[p]) * rnc[p]
        loss_rows = (torch.log(st["l"]) + inv_t - mean_r * inv_t) + (torch.log(c[p]) + inv_t - mean_c * inv_t)
        s, e, wl = blocks["X"]
        w = e.to(BF16).float() * (u[:, None] + vv[None, :]) - wl * (rn[:, None] + rnc[None, :])
        w[i, p] = e[i, p] * (u + vv[p]) - (rn + rnc[p])
        w = (ct * w).to(BF16).float()
        da, slots = w @ v["b_all"], dict(b_all=[w.T @ v["a_loc"]])
        db = None
        if pooled:
            s, e, wl = blocks["Y"]
            wy = (ct * (e.to(BF16).float() * u[:, None] - wl * rn[:, None])).to(BF16).float()
            s, e, wl = blocks["Z"]
            wz = (ct * (e.to(BF16).float() * vv[p][:, None] - wl * rnc[p][:, None])).to(BF16).float()
            da = da + wy @ v["a_all"]
            db = wz @ v["b_all"]
            slots = dict(a_all=[wy.T @ v["a_loc"]], b_all=[slots["b_all"][0] + wz.T @ v["b_loc"]])
        d_t = -((v["a_loc"] * da).sum() + ((v["b_loc"] * db).sum() if pooled else 0.0)) * inv_t
        out.append(dict(share=loss_rows.sum() * coef, own_a=da, own_b=db, slots=slots, dT=d_t))
    return out


def emulate_two_ranks(form, mutation=None, T=T0):
    """Per rank dict(loss, dza [rows, d], dzb, dT) as tests/test_losses_two_ranks_gpu.py's workers return them (gradients and dT
    divided by world), from the CPU arithmetic of the module docstring; ``mutation``: one of MUTATIONS."""
    assert form in FORMS and mutation in (None,) + MUTATIONS and (mutation is None or applies(mutation, form))
    arrangement, kind = FORMS[form]
    inp = inputs()
    na, nb, za, zb = inp["na"], inp["nb"], inp["za"], inp["zb"]
    meta = meta_of(form, inp)
    coef = torch.tensor(0.5 / N, dtype=F32)
    inv_t = torch.tensor(1.0, dtype=F32) / torch.tensor(T, dtype=F32)
    ct = coef * inv_t
    views = _rank_views(na, nb, meta, kind, mutation)
    if arrangement.endswith("stream"):
        ranks = [_stream_rank(v, arrangement, kind, inv_t, ct, coef) for v in views]
    else:
        ranks = _tile_ranks(views, arrangement == "pool_tile", kind, inv_t, ct, coef, mutation != "stats_not_reduced")
    world = 1.0 if mutation == "no_world_factor" else float(WORLD)
    bf = lambda x: x.to(BF16).float()
    # a rank's share of a gathered-row gradient goes to the view whose gathered rows stood in that slot
    target = dict(a_all="b", b_all="a") if views[0]["swapped"] else dict(a_all="a", b_all="b")
    shares = {"a": [], "b": []}
    for rk in ranks:
        got = {}
        for slot, terms in rk["slots"].items():
            g = None
            for term in terms:
                term = bf(term[:N] * world)                      # (a padding row's gradient is dropped by the gather's backward)
                g = term if g is None else bf(g + term)
            got[target[slot]] = g
        for view in ("a", "b"):
            shares[view].append(got.get(view))
    total = sum(rk["share"] for rk in ranks)                      # the all-reduce of _dp_value
    results = []
    for r, ((lo, hi), rk) in enumerate(zip(SHARDS, ranks)):
        res = {}
        scaled = rk["share"] * torch.tensor(world, dtype=F32)
        res["loss"] = float(scaled + (total - scaled))
        res["dT"] = float(rk["dT"] * world) / WORLD
        for name, view, own, z, zn in (("dza", "a", rk["own_a"], za, na), ("dzb", "b", rk["own_b"], zb, nb)):
            g = bf(own * world) if own is not None else None
            if shares[view][0] is not None:
                gathered = shares[view][r] if mutation == "gathered_share_dropped" else bf(shares[view][0] + shares[view][1])
                g = gathered[lo:hi] if g is None else bf(g + gathered[lo:hi])
            znf = zn[lo:hi].float()
            inv = 1.0 / z[lo:hi].float().norm(dim=1, keepdim=True)
            dz = bf((g - znf * (znf * g).sum(1, keepdim=True)) * inv)
            res[name] = dz / WORLD
        results.append(res)
    return results


def one_hot_words(labels):
    return ML.one_hot_sets(labels)
