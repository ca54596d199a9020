"""Case table, inputs, float64 truths, per-block bounds and a switchable float64 restatement for the score path of the
shared-query pool backward, shared by tests/test_pool_score_cpu.py and tests/test_pool_score_gpu.py.  Nothing here touches a GPU.

Why per block: every other parity test of the fused backward feeds ONE loss (y . dy + wbar . dwbar) and scores each gradient
with ``helpers.rel_err`` over the whole tensor.  dx is then dominated by its value term and dw_in / db_in by their v block, which
hold no score gradient at all; the attention-weight term d_attn_w / H and the eval-mode entropy gradient can be wrong or missing
and stay inside those bounds (test_pool_score_cpu.py puts numbers to that).  Here the three upstream gradients run apart
  * ``dy``    loss y . dy, info['attention_weights'] untouched: the kernels' d_attn_w == NULL branch
  * ``dwbar`` loss wbar . dwbar, dy absent (the layer supplies zeros)
  * ``dent``  eval mode with a CurriculumMasking attached, loss entropy . gH
and every result is cut into blocks (``blocks``), each scored against ITS OWN largest element.

Truth: oracle.aecf_oracle in float64 on the values the kernel reads.  For ``dent`` the oracle's dwbar is
``entropy_rows_backward(w_kernel, gH)`` on the float32 head-averaged weights the kernel itself returned, so that the forward's
rounding of the weights is not multiplied by the logarithm (torch's own bf16 module, forming the entropy from bf16 weights, is
1e-2 .. 5e-1 off on this upstream: no yardstick).  The CPU tests, which have no kernel, use the float32 rounding of the oracle's
weights in its place.

Bounds (``bounds``), per block and per case, never from the kernel under test:
  * bf16- / float16-stored blocks: max(2 x the error of torch.nn.MultiheadAttention run in that dtype on the CPU on the same
    values and the same upstream, 2^-8 / 2^-11), as tests/mha_edges_cases.py: bf16_bounds; for ``dent`` torch takes the
    oracle's dwbar as a d_attn_w upstream;
  * float32 activations: FP32_TOL per block, 2 x FP32_TOL for parameter gradients (tests/test_dp_routes_gpu.py: _bounds);
  * float32-stored gradients of the bf16 kernels (master weights): the BF16_F32GRAD_HILO_BOUNDS entry of the tensor, applied to
    the block's own largest element (every master-weight case here is one the hi + lo products are built for)."""
import functools
import math

import torch

from tests import mha_edges_cases as MC
from tests.helpers import BF16_BOUNDS, BF16_F32GRAD_HILO_BOUNDS, rel_err

bf16, f16, f32 = torch.bfloat16, torch.float16, torch.float32
FP32_TOL = 1e-5
FLOORS = {bf16: 2.0 ** -8, f16: 2.0 ** -11}
UPSTREAMS = ("dy", "dwbar", "dent")

# id: (activation dtype, parameter dtype, B, M, E, H, score route)
#   dsu_ws     dsu_ws_kernel (aecf_gemm_ws.hip): ds and u = ds^T x in one pass over (do, x), nothing saved by the forward
#   dsu_ws_lo  the same kernel with the do_lo tiles (AECF_HILO_GRADS: float32 master parameters)
#   dscore_v   dscore_v_kernel from the saved per-modality V
#   bwd_g      bwd_g_kernel's recompute pass (hi / lo where dsu_ws has no room for the low tiles or does not take the shape)
CASES = {
    "dsu_bf16_B1_M3_E512_H8": (bf16, bf16, 1, 3, 512, 8, "dsu_ws"),
    "dsu_bf16_B40_M3_E512_H8": (bf16, bf16, 40, 3, 512, 8, "dsu_ws"),
    "dsu_bf16_B2100_M3_E512_H8": (bf16, bf16, 2100, 3, 512, 8, "dsu_ws"),       # two 16-row steps per block and a tail
    "dsu_bf16_B4200_M4_E256_H4": (bf16, bf16, 4200, 4, 256, 4, "dsu_ws"),
    "dsu_bf16_B40_M2_E512_H16": (bf16, bf16, 40, 2, 512, 16, "dsu_ws"),
    "dsulo_master_B40_M3_E512_H8": (bf16, f32, 40, 3, 512, 8, "dsu_ws_lo"),
    "dsulo_master_B300_M4_E256_H4": (bf16, f32, 300, 4, 256, 4, "dsu_ws_lo"),
    "dsv_bf16_B37_M2_E768_H8": (bf16, bf16, 37, 2, 768, 8, "dscore_v"),
    "dsv_bf16_B37_M4_E1024_H8": (bf16, bf16, 37, 4, 1024, 8, "dscore_v"),
    "dsv_bf16_B300_M3_E128_H4": (bf16, bf16, 300, 3, 128, 4, "dscore_v"),
    "dsv_f32_B37_M3_E512_H8": (f32, f32, 37, 3, 512, 8, "dscore_v"),
    "dsv_f32_B300_M4_E128_H4": (f32, f32, 300, 4, 128, 4, "dscore_v"),
    "dsv_f16_B37_M3_E512_H8": (f16, f16, 37, 3, 512, 8, "dscore_v"),
    "bwdg_master_B37_M4_E512_H8": (bf16, f32, 37, 4, 512, 8, "bwd_g"),
    "bwdg_master_B37_M2_E768_H8": (bf16, f32, 37, 2, 768, 8, "bwd_g"),
    "bwdg_master_B37_M4_E1024_H8": (bf16, f32, 37, 4, 1024, 8, "bwd_g"),
}
# one dwbar case per route also runs with a boolean key_padding_mask (about a quarter of the keys blocked, never key 0)
KPM_CASES = ("dsu_bf16_B40_M3_E512_H8", "dsulo_master_B300_M4_E256_H4", "dsv_bf16_B300_M3_E128_H4", "bwdg_master_B37_M4_E512_H8")
# the query of the ``dent`` runs is scaled so that the head-averaged weights leave the neighbourhood of uniform (else
# log w + 1 is the same for every key and the softmax backward cancels it)
DENT_QUERY_SCALE = 16.0
# {case: (query scale, seed bump)} where 16 and the case's first seed do not spread the weights over 0.1 .. 0.5 (a single row, two
# keys, sixteen heads whose average flattens): found by search on the CPU over the float64 oracle's weights alone
DENT_SETUP = {
    "dsu_bf16_B1_M3_E512_H8": (32.0, 41),      # (a single row: also one whose key term is large enough in dx for rule 8)
    "dsu_bf16_B40_M3_E512_H8": (32.0, 0), "dsu_bf16_B40_M2_E512_H16": (32.0, 0),
    "dsv_bf16_B37_M2_E768_H8": (64.0, 0), "dsv_bf16_B37_M4_E1024_H8": (32.0, 0), "dsv_f32_B37_M3_E512_H8": (32.0, 0),
    "bwdg_master_B37_M2_E768_H8": (64.0, 0), "bwdg_master_B37_M4_E1024_H8": (32.0, 0),
}
# the spread asked of the float64 weights of the ``dent`` runs: min <= 0.1 and max >= 0.5.  Two keys under sixteen heads cannot
# get there: from scale 32 on every head has taken a side and their average stays within 0.2 .. 0.8 while torch's bf16 error
# passes 2e-2; that case is held to 0.31 .. 0.69 (log w differs by 0.8 between its keys: nothing cancels)
DENT_SPREAD = {"dsu_bf16_B40_M2_E512_H16": (0.31, 0.69)}


def dent_scale(case):
    return DENT_SETUP.get(case, (DENT_QUERY_SCALE, 0))[0]


def shape(case):
    return CASES[case][2:6]


def is_master(case):
    adt, pdt = CASES[case][:2]
    return adt != pdt


# ---- the row chunking of the kernels, restated from their launchers ----
G_SAMPLES = 128                         # aecf_bwd_g.hip: samples per block of bwd_g_kernel
DSCORE_V_ROWS = 4                       # aecf_dscore_v.hip: one wave per sample, four waves per block
DSU_LDS = 160 * 1024


def dsu_ws_smem(E, M, hd, lo):
    """aecf_gemm_ws.hip: dsu_ws_smem -- two x tiles + K-padding page + do tiles (+ do_lo) + partial dots + ds operand arrays"""
    jb = 256
    xrows = 16 * M
    zrows = 1 if 32 * ((xrows + 31) // 32) - xrows > 0 else 0
    hbl = jb // hd
    return (2 * xrows + zrows) * 2 * E + (4 if lo else 2) * 16 * 2 * jb + 8 * (16 * hbl * M) * 4 + 2 * 16 * 72 * 2


def dsu_ws_rows(B, E):
    """aecf_gemm_ws.hip: launch_dsu_t -- rows per block = ceil(B / (256 / (E / 256))) rounded up to 16"""
    chunks = max(256 // (E // 256), 1)
    rpb = (B + chunks - 1) // chunks
    return (rpb + 15) // 16 * 16


def dsu_ws_takes(M, E, H, lo=False):
    """aecf_gemm_ws.hip: dsu_ws_chunks > 0 (and dsu_ws_takes_lo)"""
    hd = E // H
    if not (1 <= M <= 4) or hd % 32 or E not in (256, 512) or 256 % hd or hd // 32 not in (1, 2, 4, 8):
        return False
    return dsu_ws_smem(E, M, hd, lo) <= DSU_LDS


def expected_route(case):
    """The score kernel aecf_capi.hip: pool_backward_on launches for the case, restated."""
    adt, pdt, B, M, E, H, _ = CASES[case]
    hilo = is_master(case) and adt == bf16
    if adt == bf16 and dsu_ws_takes(M, E, H) and (not hilo or dsu_ws_takes(M, E, H, lo=True)):
        return "dsu_ws_lo" if hilo else "dsu_ws"
    saved_v = not hilo and not (adt == bf16 and dsu_ws_takes(M, E, H))
    return "dscore_v" if saved_v else "bwd_g"


def score_chunking(case):
    """(rows per block, blocks, rows of the last block) of the score kernel the case is meant to reach"""
    B, M, E, H = shape(case)
    route = CASES[case][6]
    rows = dsu_ws_rows(B, E) if route.startswith("dsu_ws") else {"dscore_v": DSCORE_V_ROWS, "bwd_g": G_SAMPLES}[route]
    n = (B + rows - 1) // rows
    return rows, n, B - (n - 1) * rows


def tail_rows(B):
    return B % 16 or 16


# ---- inputs ----
@functools.lru_cache(maxsize=None)
def inputs(case, qscale=1.0):
    """Seeded float64 tensors the activation dtype represents exactly (bf16 values, and float16 where that is the dtype), at
    the suite's distribution (tests/test_dp_routes_gpu.py: _Case).  ``qscale`` multiplies the query.  Do not modify."""
    adt, _, B, M, E, H, _ = CASES[case]
    g = torch.Generator().manual_seed(4201 + 13 * list(CASES).index(case) + B + M + E + 1009 * DENT_SETUP.get(case, (0, 0))[1])
    r = lambda *s: torch.randn(*s, generator=g)
    rd = (lambda t_: t_.to(bf16).to(f16).double()) if adt == f16 else (lambda t_: t_.to(bf16).double())
    d = dict(B=B, T=1, S=M, E=E, H=H)
    d["x"] = rd(r(B, M, E) * torch.linspace(1.0, 2.0, M).view(1, M, 1))
    d["w_in"] = rd(r(3 * E, E) / E ** 0.5)
    d["b_in"] = rd(r(3 * E) * 0.05)
    d["w_out"] = rd(r(E, E) / E ** 0.5)
    d["b_out"] = rd(r(E) * 0.05)
    d["query"] = rd(r(1, 1, E) * (2.0 / E) ** 0.5 * qscale)
    d["dy"] = rd(r(B, 1, E))
    d["dwbar"] = rd(r(B, 1, M))
    d["gH"] = rd(r(B, 1))
    kpm = torch.rand(B, M, generator=g) < 0.25
    kpm[:, 0] = False
    d["kpm"] = kpm
    d["q"] = d["query"].expand(B, -1, -1)
    if qscale != 1.0:
        # the ``dent`` inputs: a row whose entropy lies within 2e-4 log M of a clamp is replaced by a copy of the row farthest from
        # both (rows are independent), so that float32 ``live`` and float64 ``live`` cannot disagree on any row
        from oracle import aecf_oracle as O
        w = O.mha_forward(d["q"], d["x"], d["x"], d["w_in"], d["b_in"], d["w_out"], d["b_out"], H)["wbar"].float().double()
        dist = clamp_distance(w).reshape(B)
        bad = dist < 2e-4
        if bool(bad.any()):
            d["x"] = d["x"].clone()
            d["x"][bad] = d["x"][int(dist.argmax())].clone()
    d["k"] = d["v"] = d["x"]
    return d


def clamp_distance(w):
    """per row of weights: distance of -sum xlogx from the nearer clamp (0, log M), in units of log M"""
    M = w.shape[-1]
    h = -torch.where(w == 0, torch.zeros_like(w), w * torch.log(torch.where(w == 0, torch.ones_like(w), w))).sum(-1) / math.log(M)
    return torch.minimum(h, 1.0 - h)


@functools.lru_cache(maxsize=None)
def forward(case, qscale=1.0, kpm=False):
    from oracle import aecf_oracle as O
    d = inputs(case, qscale)
    return O.mha_forward(d["q"], d["x"], d["x"], d["w_in"], d["b_in"], d["w_out"], d["b_out"], d["H"],
                         d["kpm"] if kpm else None)


def as_result(t):
    """The six results of a backward from the oracle's / torch's dictionary: dx = dkey + dvalue, dquery summed over the batch"""
    dq = t["dquery"]
    dq = dq.sum(0) if dq.dim() == 3 and dq.shape[0] > 1 else dq
    return dict(dx=t["dx"] if "dx" in t else t["dkey"] + t["dvalue"], dquery=dq.reshape(-1),
                dw_in=t["dw_in"], db_in=t["db_in"], dw_out=t["dw_out"], db_out=t["db_out"])


def blocks(t, E):
    """Cut the six results into the blocks that are scored apart: dx whole, per modality and over the ragged tail rows;
    dquery, dw_out, db_out; the q / k / v blocks of dw_in and db_in."""
    dx = t["dx"]
    B, M = dx.shape[0], dx.shape[1]
    o = {"dx": dx, "dx.tail": dx[B - tail_rows(B):]}
    for m in range(M):
        o["dx.m%d" % m] = dx[:, m]
    o.update(dquery=t["dquery"].reshape(-1), dw_out=t["dw_out"], db_out=t["db_out"])
    for i, n in enumerate("qkv"):
        o["dw_in." + n] = t["dw_in"][i * E:(i + 1) * E]
        o["db_in." + n] = t["db_in"].reshape(-1)[i * E:(i + 1) * E]
    return o


def checked_blocks(upstream, M):
    """The blocks that hold a gradient under the upstream (the others must be zero: ``zero_blocks`` and db_in.k)"""
    dx = ["dx", "dx.tail"] + ["dx.m%d" % m for m in range(M)]
    if upstream in ("dy", "both"):
        return dx + ["dquery", "dw_out", "db_out", "dw_in.q", "dw_in.k", "dw_in.v", "db_in.q", "db_in.v"]
    return dx + ["dquery", "dw_in.q", "dw_in.k", "db_in.q"]


ZERO_WITHOUT_DY = ("dw_out", "db_out", "dw_in.v", "db_in.v")        # exactly zero when dy is absent


def upstream_of(case, upstream, w_kernel=None, kpm=False):
    """(query scale, dy, dwbar) of the oracle's backward for an upstream.  ``dent``: dwbar = entropy_rows_backward on
    ``w_kernel`` ([B, 1, M] or [B, M] float32 weights of the kernel; None: the float32 rounding of the oracle's)."""
    from oracle import aecf_oracle as O
    qs = dent_scale(case) if upstream == "dent" else 1.0
    d = inputs(case, qs)
    zero = torch.zeros_like(d["dy"])
    if upstream == "dy":
        return qs, d["dy"], None
    if upstream == "dwbar":
        return qs, zero, d["dwbar"]
    if upstream == "both":
        return qs, d["dy"], d["dwbar"]
    assert upstream == "dent" and not kpm       # rows with exact zeros are not pinned by the oracle
    if w_kernel is None:
        w_kernel = forward(case, qs)["wbar"].float()
    w = w_kernel.detach().cpu().double().reshape(d["B"], 1, d["S"])
    return qs, zero, O.entropy_rows_backward(w, d["gH"])


def truth(case, upstream, w_kernel=None, kpm=False):
    """float64 blocks of the oracle's backward under one upstream ('dy', 'dwbar', 'dent', or 'both' = dy + dwbar)"""
    from oracle import aecf_oracle as O
    qs, dy, dwbar = upstream_of(case, upstream, w_kernel, kpm)
    d = inputs(case, qs)
    f = forward(case, qs, kpm)
    b = O.mha_backward(d["q"], d["x"], d["x"], d["w_in"], d["b_in"], d["w_out"], d["H"], f, dy, dwbar)
    return blocks(as_result(b), d["E"])


def torch_blocks(case, upstream, dtype, w_kernel=None, kpm=False):
    """torch.nn.MultiheadAttention in ``dtype`` on the CPU, same values, same upstream (for ``dent`` the oracle's dwbar as a
    d_attn_w upstream): its blocks in float64."""
    qs, dy, dwbar = upstream_of(case, upstream, w_kernel, kpm)
    d = dict(inputs(case, qs))
    d["dy"] = dy
    d["dwbar"] = torch.zeros_like(d["dwbar"]) if dwbar is None else dwbar
    ref = MC.torch_mha_nine(d, dict(key_padding_mask=d["kpm"]) if kpm else None, dtype)
    return blocks(as_result(ref), d["E"])


def block_errors(got, want, names):
    return {n: rel_err(got[n], want[n]) for n in names}


def bounds(case, upstream, want, w_kernel=None, kpm=False):
    """{block: bound} for the blocks checked under the upstream, and the torch errors they were made from (None: no torch run)"""
    adt, pdt, B, M, E, H, _ = CASES[case]
    names = checked_blocks(upstream, M)
    if adt == f32:
        return {n: FP32_TOL if n.startswith("dx") else 2 * FP32_TOL for n in names}, None
    ref = block_errors(torch_blocks(case, upstream, adt, w_kernel, kpm), want, names)
    out = {}
    for n in names:
        if pdt == f32 and not n.startswith("dx"):           # float32-stored gradient of the bf16 kernels
            out[n] = BF16_F32GRAD_HILO_BOUNDS[n.split(".")[0]]
        else:
            out[n] = max(2.0 * ref[n], FLOORS[adt])
    if adt == bf16 and upstream in ("dy", "both"):
        # the whole of dx where dy flows: also the project's own table (the same 4.5e-3 with or without master weights), which
        # the suite asserts under the combined loss.  2 x torch comes out near 8e-3 there, and the key term is a fifth of dx: the
        # table is the tighter of the two, and the one that still sees 5 % of the key term (rule 8)
        out["dx"] = min(out["dx"], BF16_BOUNDS["dx"])
    return out, ref


@functools.lru_cache(maxsize=None)
def reference(case, upstream, kpm=False):
    """(truth blocks, bounds, torch errors) of an upstream with nothing taken from a kernel (``dent``: the CPU stand-in for the
    kernel's weights, which the GPU tests do not use); shared, do not modify"""
    want = truth(case, upstream, kpm=kpm)
    bnd, ref = bounds(case, upstream, want, kpm=kpm)
    return want, bnd, ref


# ---- the shared-query backward restated in float64, as the kernels arrange it, with switches for broken rules ----
RULES = {
    1: "d_attn_w left out of dp",
    2: "d_attn_w not divided by H",
    3: "the softmax-backward dot formed without the d_attn_w term",
    4: "the d_attn_w term in u (dquery, dw_in) but not in the ds that dx reads",
    5: "the ragged tail rows take the last full row's d_attn_w",
    6: "entropy gradient without the + 1",
    7: "entropy gradient with live ignored",
    8: "the key term of dx scaled by 0.95",
}
RULE_UPSTREAM = {1: "dwbar", 2: "dwbar", 3: "dwbar", 4: "dwbar", 5: "dwbar", 6: "dent", 7: "dent", 8: "dy"}


def entropy_upstream(w, gH, broken=None):
    """d entropy / d wbar as the three kernels form it from their own float32 weights: live ? -(log w + 1) de : 0"""
    M = w.shape[-1]
    safe = torch.where(w == 0, torch.ones_like(w), w)
    raw = -torch.where(w == 0, torch.zeros_like(w), w * torch.log(safe)).sum(-1, keepdim=True)
    live = ((raw >= 0.0) & (raw <= math.log(M))).to(w.dtype)
    if broken == 7:
        live = torch.ones_like(live)
    return -(torch.log(w) + (0.0 if broken == 6 else 1.0)) * gH.unsqueeze(-1) * live


def restated_backward(d, f, dy, dwbar=None, w_ent=None, gH=None, broken=None):
    """do = dy W_o; da[b,h,m] = do_h . V_h[b,m]; dp = da + (dwbar + entropy gradient) / H; ds = p (dp - sum_m p dp);
    u_h = sum_{b,m} ds[b,h,m] x[b,m]; dq'_h = scale W_k,h u_h (the key bias drops out: sum_m ds = 0); dx = sum_h ds a_h + the value
    term, a_h = scale W_k,h^T q'_h.  ``d``: inputs, ``f``: oracle.mha_forward's dictionary.  Returns the six results."""
    B, M, E, H = d["B"], d["S"], d["E"], d["H"]
    hd = E // H
    scale = math.sqrt(1.0 / hd)
    x, w_in, w_out = d["x"], d["w_in"], d["w_out"]
    wq, wk, wv = w_in[:E], w_in[E:2 * E], w_in[2 * E:]
    p = f["p"].reshape(B, H, M)
    qp = f["qp"][0, 0].reshape(H, hd)                          # the shared projected query
    vp = f["vp"].reshape(B, M, H, hd)
    dy2 = dy.reshape(B, E)
    do = (dy2 @ w_out).reshape(B, H, hd)
    da = torch.einsum("bhj,bmhj->bhm", do, vp)
    dw = torch.zeros(B, M, dtype=x.dtype)
    if dwbar is not None:
        dw = dw + dwbar.reshape(B, M)
    if w_ent is not None:
        dw = dw + entropy_upstream(w_ent.reshape(B, 1, M), gH.reshape(B, 1), broken).reshape(B, M)
    if broken == 5:                                             # rows of the last 16-row step read the row before it (or padding)
        t0 = B - tail_rows(B)
        dw = dw.clone()
        dw[t0:] = dw[t0 - 1] if t0 > 0 else 0.0
    term = dw.unsqueeze(1) / (1.0 if broken == 2 else H)
    dp = da + (0.0 if broken == 1 else term)
    dot = (p * (da if broken == 3 else dp)).sum(-1, keepdim=True)
    ds = p * (dp - dot)
    ds_x = ds
    if broken == 4:
        ds_x = p * (da - (p * da).sum(-1, keepdim=True))
    u = torch.einsum("bhm,bme->he", ds, x)                      # [H, E]
    wk_h = wk.reshape(H, hd, E)
    dqp = scale * torch.einsum("hje,he->hj", wk_h, u)           # [H, hd]
    a = scale * torch.einsum("hje,hj->he", wk_h, qp)            # folded key rows [H, E]
    dkey = torch.einsum("bhm,he->bme", ds_x, a)
    if broken == 8:
        dkey = 0.95 * dkey
    dvp = torch.einsum("bhm,bhj->bmhj", p, do).reshape(B, M, E)
    dvalue = dvp @ wv
    dqp_flat = dqp.reshape(E)
    dkp_w = (scale * qp).reshape(E, 1) * u.repeat_interleave(hd, 0)          # rows of head h: scale q'_h[j] u_h
    dw_in = torch.cat([dqp_flat.reshape(E, 1) * d["query"].reshape(1, E), dkp_w, dvp.reshape(B * M, E).T @ x.reshape(B * M, E)], 0)
    db_k = (scale * qp) * ds.sum((0, 2)).reshape(H, 1)
    db_in = torch.cat([dqp_flat, db_k.reshape(E), dvp.sum((0, 1))], 0)
    return dict(dx=dkey + dvalue, dquery=dqp_flat @ wq, dw_in=dw_in, db_in=db_in, dw_out=dy2.T @ f["o"].reshape(B, E),
                db_out=dy2.sum(0))


def clamped_weights(w):
    """The weights of the case built for rule 7: rows 1, 5, 9, ... and the last row times M.  -sum xlogx of M w is
    M (H(w) - log M) < 0 for every row that is not uniform, so those rows sit on the lower clamp and carry no entropy gradient.
    (A softmax cannot produce such a row: on the device ``live`` is false only where float32 rounding lifts a uniform row's sum
    past log M, and there log w + 1 is the same for every key and cancels in the softmax backward.  The GPU cases therefore keep
    every row away from the clamps; this case exists so that the rule has something to break.)"""
    w = w.clone()
    M = w.shape[-1]
    rows = list(range(1, w.shape[0], 4)) + [w.shape[0] - 1]
    w[rows] = w[rows] * M
    return w, rows


def restated_blocks(case, upstream, broken=None, w_ent=None):
    """Blocks of the restatement under an upstream ('dy', 'dwbar', 'dent', 'both'); ``w_ent``: the weights of the entropy
    gradient (default: the float32 rounding of the oracle's)."""
    qs = dent_scale(case) if upstream == "dent" else 1.0
    d, f = inputs(case, qs), forward(case, qs)
    zero = torch.zeros_like(d["dy"])
    if upstream == "dent":
        if w_ent is None:
            w_ent = f["wbar"].float().double()
        r = restated_backward(d, f, zero, None, w_ent, d["gH"], broken)
    else:
        r = restated_backward(d, f, d["dy"] if upstream in ("dy", "both") else zero,
                              d["dwbar"] if upstream in ("dwbar", "both") else None, broken=broken)
    return blocks(r, d["E"])


OLD_TENSORS = ("dx", "dquery", "dw_in", "db_in", "dw_out", "db_out")


def old_metric_errors(case, broken):
    """What the suite asserted before: whole-tensor rel_err under the combined upstream y . dy + wbar . dwbar"""
    d, f = inputs(case), forward(case)
    want = restated_backward(d, f, d["dy"], d["dwbar"])
    got = restated_backward(d, f, d["dy"], d["dwbar"], broken=broken)
    return {n: rel_err(got[n], want[n]) for n in OLD_TENSORS}


OLD_BOUNDS = {n: BF16_BOUNDS[n] for n in OLD_TENSORS}
