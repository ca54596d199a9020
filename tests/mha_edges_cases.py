"""Case tables and CPU references shared by tests/test_mha_edges_cpu.py, tests/test_mha_edges_gpu.py and
tests/test_mha_general_gpu.py: the general attention route (aecf_mha_forward / aecf_mha_backward) at its chunk, length and
option edges.  Nothing here touches a GPU.

The truth of every comparison is oracle.aecf_oracle in float64 on the values the kernel reads.  The bf16 bounds are not set
from the kernel: ``torch_mha_nine`` runs torch.nn.MultiheadAttention (the module the reference calls) in bfloat16 on the same
values, its error against the float64 oracle is the reference's own bf16 error, and ``bf16_bounds`` turns it into the kernel's
bound, max(2 x that error, 2^-8) per tensor:
  * 2 x: the kernel stores q, k, v, o and the pre-projection gradients in bf16 once each, where torch's CPU path may keep some
    of them wide;
  * 2^-8: no bf16-stored tensor escapes one output rounding (2^-9 of its largest element), the same again for one rounded
    operand."""
import functools
import math
import warnings

import torch

NINE = ("y", "wbar", "dquery", "dkey", "dvalue", "dw_in", "db_in", "dw_out", "db_out")
BF16_FLOOR = 2.0 ** -8

# ---- the chunking of the attention core, restated (aecf_amd/csrc/aecf_mha.hip: CORE_LDS, core_rows) ----
CORE_LDS = 96 * 1024


def core_rows(T, S):
    """query rows per chunk: as many as fit CORE_LDS next to all S keys in two [rows][S + 1] float arrays, at most 64 and T"""
    tc = CORE_LDS // (2 * (S + 1) * 4)
    tc = min(tc, 64, T)
    return max(tc, 1)


def chunking(T, S):
    """(rows per chunk, number of chunks, rows of the last chunk)"""
    tc = core_rows(T, S)
    n = (T + tc - 1) // tc
    return tc, n, T - (n - 1) * tc


def core_lds_bytes(T, S):
    return 2 * core_rows(T, S) * (S + 1) * 4


# name: (B, T, S, E, H, (rows per chunk, chunks, rows of the last chunk))
GEOMETRIES = {
    "T65_S5": (6, 65, 5, 64, 4, (64, 2, 1)),            # 64 + 1 rows
    "T130_S64": (4, 130, 64, 128, 4, (64, 3, 2)),       # 64 + 64 + 2
    "T64_S191": (3, 64, 191, 64, 4, (64, 1, 64)),       # the last S with 64 rows per chunk: one chunk
    "T65_S192": (3, 65, 192, 128, 4, (63, 2, 2)),       # the first S with 63: 63 + 2
    "T40_S383": (2, 40, 383, 64, 4, (32, 2, 8)),        # 32 + 8
    "T200_S700": (2, 200, 700, 64, 4, (17, 12, 13)),    # 11 x 17 + 13
}
# length and head-geometry limits (eval mode, bool key_padding_mask): rows of test_general_path_reach
LIMITS = {
    "S4096_T5": (2, 5, 4096, 64, 4, (2, 3, 1)),         # 2 + 2 + 1; 65 552 bytes of dynamic LDS, the largest request
    "S4095_T4": (2, 4, 4095, 64, 4, (3, 2, 1)),         # 3 + 1
    "S2047_T3": (2, 3, 2047, 64, 4, (3, 1, 3)),         # one chunk, below that S's cap of 6 rows
    "T4096_S3": (2, 4096, 3, 64, 4, (64, 64, 64)),      # 64 chunks: 63 carries per dk / dv element
    "hd1024": (2, 3, 7, 1024, 1, (3, 1, 3)),            # 16 trips of the lane loop of the dots
    "hd64_H16": (2, 3, 7, 1024, 16, (3, 1, 3)),
    "hd1": (3, 3, 7, 64, 64, (3, 1, 3)),                # 63 idle lanes
    "hd2": (3, 3, 7, 64, 32, (3, 1, 3)),
    "hd96": (3, 3, 7, 192, 2, (3, 1, 3)),               # a partial second trip
}

OPTIONS = ("none", "bool2d", "bool3d", "float3d", "bool_kpm+float2d", "float_kpm+bool2d", "dropout", "dropout+bool3d+bool_kpm")
EVAL_OPTIONS = tuple(o for o in OPTIONS if not o.startswith("dropout"))
DROP_P = 0.25
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def case_seed(geometry, option, dtype_name):
    names = list(GEOMETRIES) + list(LIMITS)
    opts = list(OPTIONS) + ["bool_kpm"]
    return 10007 + 1000 * names.index(geometry) + 10 * opts.index(option) + list(DTYPES).index(dtype_name)


def make_inputs(seed, B, T, S, E, H, dtype, bias=True):
    """float32 CPU tensors that ``dtype`` represents exactly: what the kernel reads, and what the float64 oracle is given"""
    g = torch.Generator().manual_seed(seed)
    rd = lambda t_: t_.to(dtype).to(torch.float32)
    r = lambda *sh: torch.randn(*sh, generator=g)
    d = dict(B=B, T=T, S=S, E=E, H=H, g=g, rd=rd)
    d["w_in"] = rd(r(3 * E, E) / math.sqrt(E))
    d["b_in"] = rd(r(3 * E) * 0.1) if bias else None
    d["w_out"] = rd(r(E, E) / math.sqrt(E))
    d["b_out"] = rd(r(E) * 0.1) if bias else None
    d["q"], d["k"], d["v"] = rd(r(B, T, E)), rd(r(B, S, E)), rd(r(B, S, E))
    d["dy"], d["dwbar"] = rd(r(B, T, E)), rd(r(B, T, S))
    return d


def make_option(name, d):
    """Masks of one option set, drawn from the case's generator.  Key 0 is never blocked for any (sample, head, query row): no
    fully masked row, no NaN in the reference.  Float masks hold values the activation dtype represents, so that torch in
    that dtype reads the mask the kernel reads (the kernel takes it as float32).  Returns ``layer`` (keywords of the pool),
    ``oracle`` (key_padding_mask / attn_mask of oracle.mha_forward: a float key_padding_mask merged into the additive
    [B*H,T,S] mask as the layer merges it before the C call) and ``torch`` (keywords of nn.MultiheadAttention)."""
    B, T, S, H, g, rd = d["B"], d["T"], d["S"], d["H"], d["g"], d["rd"]
    ninf = float("-inf")

    def blocked(*sh, p=0.3):
        m = torch.rand(*sh, generator=g) < p
        m[..., 0] = False
        return m

    def additive(*sh):
        return rd(torch.randn(*sh, generator=g)).masked_fill(blocked(*sh, p=0.2), ninf)

    layer, oracle = {}, {}
    parts = name.split("+")
    if "bool2d" in parts:
        layer["attn_mask"] = oracle["attn_mask"] = blocked(T, S)
    if "bool3d" in parts:
        layer["attn_mask"] = oracle["attn_mask"] = blocked(B * H, T, S)
    if "float3d" in parts:
        layer["attn_mask"] = oracle["attn_mask"] = additive(B * H, T, S)
    if "float2d" in parts:
        layer["attn_mask"] = oracle["attn_mask"] = additive(T, S)
    if "bool_kpm" in parts:
        layer["key_padding_mask"] = oracle["key_padding_mask"] = blocked(B, S, p=0.25)
    tch = dict(layer)
    if "float_kpm" in parts:
        kf = additive(B, S)
        layer["key_padding_mask"] = tch["key_padding_mask"] = kf
        base = torch.zeros(T, S, dtype=torch.float64).masked_fill(layer["attn_mask"], ninf).view(1, 1, T, S)
        oracle["attn_mask"] = (base + kf.double().view(B, 1, 1, S)).expand(B, H, T, S).reshape(B * H, T, S)
    return dict(layer=layer, oracle=oracle, torch=tch, drop_p=DROP_P if "dropout" in parts else 0.0)


def oracle_nine(d, oracle_kw=None, drop_u=None, drop_p=0.0, dy=True, dwbar=True):
    """oracle.mha_forward / mha_backward in float64 on the case's values: (forward dict, the nine tensors).  ``dy`` /
    ``dwbar`` False: that upstream gradient is absent (dy = 0 / no d_attn_w)."""
    from oracle import aecf_oracle as O
    c = lambda t_: None if t_ is None else t_.double()
    kw = oracle_kw or {}
    am = kw.get("attn_mask")
    if am is not None and am.dtype != torch.bool:
        am = am.double()
    f = O.mha_forward(c(d["q"]), c(d["k"]), c(d["v"]), c(d["w_in"]), c(d["b_in"]), c(d["w_out"]), c(d["b_out"]), d["H"],
                      kw.get("key_padding_mask"), am, None if drop_u is None else drop_u.double(), drop_p)
    b = O.mha_backward(c(d["q"]), c(d["k"]), c(d["v"]), c(d["w_in"]), c(d["b_in"]), c(d["w_out"]), d["H"], f,
                       c(d["dy"]) if dy else torch.zeros_like(c(d["dy"])), c(d["dwbar"]) if dwbar else None)
    want = dict(y=f["y"], wbar=f["wbar"], **b)
    if d["b_in"] is None:
        del want["db_in"], want["db_out"]
    return f, want


def torch_mha_nine(d, torch_kw=None, dtype=torch.float64):
    """torch.nn.MultiheadAttention on the CPU in ``dtype``, eval mode, same parameters, inputs, masks and upstream
    gradients: its outputs and gradients as float64 tensors."""
    E, H = d["E"], d["H"]
    mha = torch.nn.MultiheadAttention(E, H, bias=d["b_in"] is not None, batch_first=True)
    with torch.no_grad():
        mha.in_proj_weight.copy_(d["w_in"])
        mha.out_proj.weight.copy_(d["w_out"])
        if d["b_in"] is not None:
            mha.in_proj_bias.copy_(d["b_in"])
            mha.out_proj.bias.copy_(d["b_out"])
    mha = mha.to(dtype).eval()
    q, k, v = (d[n].to(dtype).requires_grad_(True) for n in ("q", "k", "v"))
    kw = {n: (m if m.dtype == torch.bool else m.to(dtype)) for n, m in (torch_kw or {}).items()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (a bool attn_mask next to a float key_padding_mask: torch converts and warns)
        y, w = mha(q, k, v, need_weights=True, average_attn_weights=True, **kw)
    ((y.double() * d["dy"].double()).sum() + (w.double() * d["dwbar"].double()).sum()).backward()
    out = dict(y=y, wbar=w, dquery=q.grad, dkey=k.grad, dvalue=v.grad, dw_in=mha.in_proj_weight.grad,
               dw_out=mha.out_proj.weight.grad)
    if d["b_in"] is not None:
        out.update(db_in=mha.in_proj_bias.grad, db_out=mha.out_proj.bias.grad)
    return {n: t_.detach().double() for n, t_ in out.items()}


def errors(got, want):
    from tests.helpers import rel_err
    return {n: rel_err(got[n], want[n]) for n in want}


def bf16_bounds(ref_errs):
    return {n: max(2.0 * e, BF16_FLOOR) for n, e in ref_errs.items()}


def dims(name):
    return (GEOMETRIES.get(name) or LIMITS[name])[:5]


@functools.lru_cache(maxsize=None)
def eval_reference(geometry, option, dtype_name):
    """An eval-mode case of the tables above: (the float64 oracle's nine tensors, the per-tensor error of torch's module run in
    bfloat16 against them -- None for other dtypes).  Kept per case: the dropout cases in bf16, which torch's module cannot
    match draw for draw, take the largest eval-mode bound of their geometry."""
    dtype = DTYPES[dtype_name]
    d = make_inputs(case_seed(geometry, option, dtype_name), *dims(geometry), dtype)
    opt = make_option(option, d)
    _, want = oracle_nine(d, opt["oracle"])
    ref = errors(torch_mha_nine(d, opt["torch"], torch.bfloat16), want) if dtype == torch.bfloat16 else None
    return want, ref


def bf16_dropout_bounds(geometry):
    per = [bf16_bounds(eval_reference(geometry, o, "bf16")[1]) for o in EVAL_OPTIONS]
    return {n: max(p[n] for p in per) for n in NINE}
