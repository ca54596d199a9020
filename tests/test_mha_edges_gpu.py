"""The general attention route (aecf_mha_forward / aecf_mha_backward through MultimodalAttentionPool._forward_general, and the
projection-free aecf_sdpa_* kernels) against oracle.aecf_oracle in float64, where its index arithmetic has something to get
wrong: several query chunks together with the operand the chunk offset indexes (attn_mask, dropout uniforms, d_attn_w, the
float32 dk / dv carries), every option set and their combinations, all three dtypes, and the call shapes no other test makes.
Tables, references and the bf16 bound: tests/mha_edges_cases.py.  The length and head-geometry limits are rows of
tests/test_mha_general_gpu.py::test_general_path_reach.

Bounds (rel_err, max-abs over max-abs): float32 1e-5 (2e-5 at T=200, S=700: 700-term softmax sums), the route's bound;
float16 1e-3 + 2^-11, the project's; bfloat16 per tensor max(2 x torch's own bf16 error, 2^-8), see mha_edges_cases."""
import ctypes

import pytest
import torch

from tests import mha_edges_cases as C
from tests.helpers import record_errors, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16_BOUND = 1e-3 + 2.0 ** -11


def _pool(d, dtype, dropout=0.0, train=False):
    import aecf_amd
    pool = aecf_amd.MultimodalAttentionPool(d["E"], num_heads=d["H"], dropout=dropout, bias=d["b_in"] is not None)
    a = pool.attention
    with torch.no_grad():
        a.in_proj_weight.copy_(d["w_in"])
        a.out_proj.weight.copy_(d["w_out"])
        if d["b_in"] is not None:
            a.in_proj_bias.copy_(d["b_in"])
            a.out_proj.bias.copy_(d["b_out"])
    return pool.to(DEV, dtype).train(train)


def _run(d, dtype, layer_kw=None, drop_p=0.0, seed=None, info=True, use_dy=True, use_dwbar=True, value=True):
    """forward + backward of the pool on the case's values: (the tensors it produced as float64 on the CPU, the dropout
    uniforms of the call or None)"""
    pool = _pool(d, dtype, drop_p, train=drop_p > 0.0)
    q, k, v = (d[n].to(DEV, dtype).requires_grad_(True) for n in ("q", "k", "v"))
    kw = {n: m.to(DEV) for n, m in (layer_kw or {}).items()}
    U = None
    if drop_p > 0.0:
        torch.manual_seed(seed)
    out = pool(q, k, v if value else None, return_info=True, **kw) if info else (pool(q, k, v if value else None, **kw), None)
    y, inf = out
    if drop_p > 0.0:                                        # the layer's draw: torch.rand(B*H, T, S) on the device, reseeded
        torch.manual_seed(seed)
        U = torch.rand(d["B"] * d["H"], d["T"], d["S"], device=DEV).cpu().reshape(d["B"], d["H"], d["T"], d["S"])
    loss = 0.0
    if use_dy:
        loss = loss + (y.float() * d["dy"].to(DEV)).sum()
    if use_dwbar:
        loss = loss + (inf["attention_weights"].float() * d["dwbar"].to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    a = pool.attention
    got = dict(y=y, dquery=q.grad, dkey=k.grad, dw_in=a.in_proj_weight.grad, dw_out=a.out_proj.weight.grad)
    if value:
        got["dvalue"] = v.grad
    if inf is not None:
        got["wbar"] = inf["attention_weights"]
    if a.in_proj_bias is not None:
        got.update(db_in=a.in_proj_bias.grad, db_out=a.out_proj.bias.grad)
    for n, t_ in got.items():
        assert t_ is not None, n
        assert t_.dtype == dtype, (n, t_.dtype)
    return {n: t_.detach().double().cpu() for n, t_ in got.items()}, U


def _f32_bound(geometry):
    return 2e-5 if geometry == "T200_S700" else 1e-5


def _assert_finite(want):
    for n, w in want.items():
        assert bool(torch.isfinite(w).all()), ("the float64 reference is not finite", n)


# ---------------- options x chunks ----------------
@pytest.mark.parametrize("dtype_name", list(C.DTYPES))
@pytest.mark.parametrize("option", C.OPTIONS)
@pytest.mark.parametrize("geometry", list(C.GEOMETRIES))
def test_options_across_query_chunks(geometry, option, dtype_name):
    """Every option set at every chunk geometry in every dtype: all nine tensors under the loss (y*dy).sum() + (wbar*dwbar).sum()
    against the float64 oracle.  No mask blocks key 0, so no row is fully masked: asserted on the reference (finite), as is
    that the dropout cases dropped some weight of every head, before the kernel is looked at.

    float16 sits close to its bound here, by the storage format and not by the kernel's arithmetic: the largest measured error
    is wbar at T40_S383 with dropout, 1.44e-3 of 1e-3 + 2^-11 = 1.49e-3 (dkey 1.35e-3 at T64_S191).  The float64 oracle itself,
    with nothing changed but the projected q and k rounded to float16 (the kernel stores them so, as the pool's contract
    says) and wbar rounded once on output, is 1.1e-3 to 1.4e-3 off at these geometries over several dropout draws: hd = 16
    gives each score 32 rounded operands of 2^-11 each, the softmax turns that into a relative error of its largest weight,
    and rel_err is the error of that one element.  The four heads average it down; under dropout fewer heads survive at an
    element, so less averages out.  The cases are seeded and the route is deterministic.  If another seed or table trips it,
    recompute that budget (the oracle with qp, kp and wbar rounded to float16) before anything else: a wider bound is not the answer."""
    dtype = C.DTYPES[dtype_name]
    d = C.make_inputs(C.case_seed(geometry, option, dtype_name), *C.dims(geometry), dtype)
    opt = C.make_option(option, d)
    ref = None
    if opt["drop_p"] == 0.0:
        want, ref = C.eval_reference(geometry, option, dtype_name)
        _assert_finite(want)
        got, _ = _run(d, dtype, opt["layer"])
    else:
        got, U = _run(d, dtype, opt["layer"], opt["drop_p"], seed=77)
        f, want = C.oracle_nine(d, opt["oracle"], U, opt["drop_p"])
        _assert_finite(want)
        dropped = (f["keep"] == 0).reshape(d["B"], d["H"], -1)
        assert bool(dropped.any(-1).all()) and not bool(dropped.all(-1).any())
    errs = C.errors(got, want)
    assert set(errs) == set(C.NINE)
    case = f"mha_edges_{geometry}_{option}_{dtype_name}"
    record_errors(case, **errs)
    if dtype == torch.bfloat16:
        if ref is not None:
            record_errors(case + "_torch_bf16", **ref)
            bounds = C.bf16_bounds(ref)
        else:
            bounds = C.bf16_dropout_bounds(geometry)
    else:
        bounds = dict.fromkeys(C.NINE, _f32_bound(geometry) if dtype == torch.float32 else F16_BOUND)
    print(case, {n: f"{e:.2e}/{bounds[n]:.2e}" for n, e in errs.items()})
    for n, e in errs.items():
        assert e < bounds[n], (case, n, e, bounds[n])


@pytest.mark.parametrize("geometry", ["one_chunk", "T65_S5"])
def test_fully_masked_rows_are_nan_where_the_reference_is(geometry):
    """A query row whose every key is blocked is NaN in torch (softmax of a row of -inf).  The kernel's NaN pattern in y and
    wbar equals the float64 reference's; all other rows meet the bound.  One chunk, and two chunks with a masked row in each."""
    B, T, S, E, H = (3, 5, 7, 64, 4) if geometry == "one_chunk" else C.dims(geometry)
    d = C.make_inputs(4242 + T, B, T, S, E, H, torch.float32)
    opt = C.make_option("bool2d", d)
    am = opt["layer"]["attn_mask"]
    am[1, :] = True
    am[T - 1, :] = True                                            # (T = 65: the one row of the second chunk)
    f, _ = C.oracle_nine(d, dict(attn_mask=am))
    rows = torch.zeros(T, dtype=torch.bool)
    rows[1] = rows[T - 1] = True
    for n in ("y", "wbar"):
        assert torch.equal(torch.isnan(f[n]), rows.view(1, T, 1).expand_as(f[n])), n      # the reference, first
    pool = _pool(d, torch.float32)
    with torch.no_grad():
        y, info = pool(d["q"].to(DEV), d["k"].to(DEV), d["v"].to(DEV), attn_mask=am.to(DEV), return_info=True)
    got = dict(y=y.double().cpu(), wbar=info["attention_weights"].double().cpu())
    for n in ("y", "wbar"):
        nan = torch.isnan(f[n])
        assert torch.equal(torch.isnan(got[n]), nan), n
        e = rel_err(got[n][~nan], f[n][~nan])
        assert e < 1e-5, (n, e)


@pytest.mark.parametrize("dtype_name,up,down", [("bf16", 2.0 ** 5, 2.0 ** -5), ("f16", 2.0 ** 6, 2.0 ** -7)])
def test_carries_of_64_chunks_are_float32(dtype_name, up, down):
    """dk / dv are summed over the query chunks in float32 scratch and rounded once, at the last chunk.  Random rows cannot
    tell a carry kept in the narrow type from that (the roundings of 63 carries cancel like a random walk and stay inside the
    bound), so this case makes them add up: T = 4096, S = 3 (64 chunks of 64 rows), every query row of a sample the same, and
    dy / dwbar the same row times ``up`` in the first chunk and times ``down`` in the 63 others.  Every later chunk then adds
    the same term, down / up = 2^-10 (bf16) or 2^-13 (f16) of the first chunk's: below half an ulp of the narrow type
    (2^-9, 2^-12), so a narrow carry never moves, and dkey / dvalue come out 63 x 2^-10 = 6 % (63 x 2^-13 = 0.8 %) short --
    several times the bound -- while a float32 carry holds them to 2^-24.  All nine tensors, usual bounds."""
    dtype = C.DTYPES[dtype_name]
    B, T, S, E, H = C.dims("T4096_S3")
    assert C.chunking(T, S) == (64, 64, 64)
    d = C.make_inputs(6400 + int(up), B, T, S, E, H, dtype)
    row = torch.full((1, T, 1), down)
    row[:, :64] = up
    d["q"] = d["q"][:, :1].expand(B, T, E).contiguous()
    d["dy"] = d["rd"](d["dy"][:, :1] * row)
    d["dwbar"] = d["rd"](d["dwbar"][:, :1] * row)
    assert torch.equal(d["dy"][:, 64:65] * (up / down), d["dy"][:, :1])           # powers of two: the scaling is exact
    _, want = C.oracle_nine(d)
    _assert_finite(want)
    got, _ = _run(d, dtype)
    errs = C.errors(got, want)
    if dtype == torch.bfloat16:
        ref = C.errors(C.torch_mha_nine(d, None, torch.bfloat16), want)
        record_errors(f"mha_edges_carry64_{dtype_name}_torch_bf16", **ref)
        bounds = C.bf16_bounds(ref)
    else:
        bounds = dict.fromkeys(C.NINE, F16_BOUND)
    record_errors(f"mha_edges_carry64_{dtype_name}", **errs)
    print(f"mha_edges_carry64_{dtype_name}", {n: f"{e:.2e}/{bounds[n]:.2e}" for n, e in errs.items()})
    assert 63 * down / up > 2 * max(bounds["dkey"], bounds["dvalue"]), bounds          # the case can tell the two apart
    for n, e in errs.items():
        assert e < bounds[n], (n, e, bounds[n])


# ---------------- call shapes ----------------
CALL_GEOMETRY = "T65_S5"          # two chunks: the second holds one row


def test_pool_without_bias():
    """bias=False: b_in / b_out are null in the C call while db_in / db_out are still written; the seven tensors that exist."""
    d = C.make_inputs(901, *C.dims(CALL_GEOMETRY), torch.float32, bias=False)
    got, _ = _run(d, torch.float32)
    _, want = C.oracle_nine(d)
    assert len(want) == 7 and set(got) == set(want)
    for n, e in C.errors(got, want).items():
        assert e < 1e-5, (n, e)


def test_pool_without_return_info_has_no_weight_gradient():
    """pool(q, k, v): no d_attn_w reaches the backward; gradients equal the oracle's with dwbar = None."""
    d = C.make_inputs(902, *C.dims(CALL_GEOMETRY), torch.float32)
    opt = C.make_option("bool3d", d)
    got, _ = _run(d, torch.float32, opt["layer"], info=False, use_dwbar=False)
    _, want = C.oracle_nine(d, opt["oracle"], dwbar=False)
    del want["wbar"]
    assert set(got) == set(want)
    for n, e in C.errors(got, want).items():
        assert e < 1e-5, (n, e)


def test_loss_on_the_weights_alone():
    """(info['attention_weights'] * dwbar).sum() with y unused: the dy-is-None branch of _MhaFunction.backward.  dw_out and
    db_out are exactly zero, the rest equals the oracle with dy = 0."""
    d = C.make_inputs(903, *C.dims(CALL_GEOMETRY), torch.float32)
    opt = C.make_option("float3d", d)
    got, _ = _run(d, torch.float32, opt["layer"], use_dy=False)
    _, want = C.oracle_nine(d, opt["oracle"], dy=False)
    _assert_finite(want)
    assert float(got["dw_out"].abs().max()) == 0.0 and float(got["db_out"].abs().max()) == 0.0
    for n in C.NINE:
        if n not in ("dw_out", "db_out"):
            e = rel_err(got[n], want[n])
            assert e < 1e-5, (n, e)


def test_value_is_key_with_per_sample_queries():
    """value = None, per-sample queries, tgt_len 2: key.grad is the oracle's dkey + dvalue."""
    d = C.make_inputs(904, 5, 2, 5, 64, 4, torch.float32)
    d["v"] = d["k"]
    got, _ = _run(d, torch.float32, value=False)
    _, want = C.oracle_nine(d)
    want["dkey"] = want["dkey"] + want.pop("dvalue")
    assert set(got) == set(want)
    for n, e in C.errors(got, want).items():
        assert e < 1e-5, (n, e)


def test_mha_calls_stay_inside_the_callers_buffers():
    """The C entry points on buffers carved out of poisoned allocations (tests/test_abi_guards_gpu.py): a two-chunk bf16 call
    with a 3-D mask and dropout, the workspace at exactly aecf_mha_bwd_workspace_bytes.  The poison on both sides of every
    buffer survives, every payload is written, and the results are the oracle's."""
    from aecf_amd import _lib
    from aecf_amd.layer import _stream
    from tests.test_abi_guards_gpu import Guarded
    lib = _lib.load()
    dt, f32 = torch.bfloat16, torch.float32
    B, T, S, E, H = C.dims(CALL_GEOMETRY)
    d = C.make_inputs(905, B, T, S, E, H, dt)
    opt = C.make_option("float3d", d)
    g = d["g"]
    U = torch.rand(B, H, T, S, generator=g)
    desc = _lib.MhaDesc(B, T, S, E, H, _lib.AECF_BF16, C.DROP_P)
    assert lib.aecf_mha_check(ctypes.byref(desc)) == 0
    dev = torch.device(DEV)
    gd = Guarded(dev)
    nan = 0xFF
    ins = {n: d[n].to(dev, dt).contiguous() for n in ("q", "k", "v", "w_in", "b_in", "w_out", "b_out", "dy")}
    mask = opt["layer"]["attn_mask"].to(dev, f32).contiguous()
    Ud, daw = U.to(dev).contiguous(), d["dwbar"].to(dev).contiguous()
    y, attn_w = gd.tensor((B, T, E), dt, nan), gd.tensor((B, T, S), f32, nan)
    sq, so = gd.tensor((B * T, E), dt, nan), gd.tensor((B * T, E), dt, nan)
    sk, sv = gd.tensor((B * S, E), dt, nan), gd.tensor((B * S, E), dt, nan)
    probs = gd.tensor((B, H, T, S), f32, nan)
    p = lambda t_: None if t_ is None else t_.data_ptr()
    fa = _lib.MhaFwdArgs(p(ins["q"]), p(ins["k"]), p(ins["v"]), p(ins["w_in"]), p(ins["b_in"]), p(ins["w_out"]), p(ins["b_out"]),
                         p(mask), T * S, None, p(Ud), p(y), p(attn_w), p(sq), p(sk), p(sv), p(so), p(probs))
    _lib.check(lib.aecf_mha_forward(ctypes.byref(desc), ctypes.byref(fa), _stream()), "aecf_mha_forward")
    torch.cuda.synchronize()
    gd.check()
    dq, dk, dv = gd.tensor((B, T, E), dt, nan), gd.tensor((B, S, E), dt, nan), gd.tensor((B, S, E), dt, nan)
    dw_in, db_in = gd.tensor((3 * E, E), f32, nan), gd.tensor((3 * E,), f32, nan)
    dw_out, db_out = gd.tensor((E, E), f32, nan), gd.tensor((E,), f32, nan)
    ws_bytes = lib.aecf_mha_bwd_workspace_bytes(ctypes.byref(desc))
    assert ws_bytes >= 2 * B * S * E * 4                               # two chunks: the carries are in it
    ws = gd.new(ws_bytes)
    ba = _lib.MhaBwdArgs(p(ins["q"]), p(ins["k"]), p(ins["v"]), p(ins["w_in"]), p(ins["w_out"]), p(Ud), p(ins["dy"]), p(daw),
                         p(sq), p(sk), p(sv), p(so), p(probs), p(dq), p(dk), p(dv), p(dw_in), p(db_in), p(dw_out), p(db_out),
                         p(ws), ws_bytes)
    _lib.check(lib.aecf_mha_backward(ctypes.byref(desc), ctypes.byref(ba), _stream()), "aecf_mha_backward")
    torch.cuda.synchronize()
    gd.check()
    _, want = C.oracle_nine(d, opt["oracle"], U, C.DROP_P)
    _assert_finite(want)
    got = dict(y=y, wbar=attn_w, dquery=dq, dkey=dk, dvalue=dv, dw_in=dw_in, db_in=db_in, dw_out=dw_out, db_out=db_out)
    bounds = C.bf16_dropout_bounds(CALL_GEOMETRY)
    for n, t_ in got.items():
        assert bool(torch.isfinite(t_.float()).all()), n              # every payload byte was written
        e = rel_err(t_.double().cpu(), want[n])
        assert e < bounds[n], (n, e, bounds[n])
    ba.workspace_bytes = ws_bytes - 1                                 # one byte short: refused before any launch
    assert lib.aecf_mha_backward(ctypes.byref(desc), ctypes.byref(ba), _stream()) == -4


def test_lengths_beyond_4096_are_refused():
    """tgt_len = 4097 and src_len = 4097: aecf_mha_check answers AECF_ERR_UNSUPPORTED and the layer raises."""
    import aecf_amd
    from aecf_amd import _lib
    lib = _lib.load()
    pool = aecf_amd.MultimodalAttentionPool(64, num_heads=4).to(DEV)
    for T, S in ((4097, 3), (3, 4097)):
        assert lib.aecf_mha_check(ctypes.byref(_lib.MhaDesc(2, T, S, 64, 4, _lib.AECF_F32, 0.0))) == -2
        with pytest.raises(RuntimeError, match="not supported"):
            pool(torch.randn(2, T, 64, device=DEV), torch.randn(2, S, 64, device=DEV))


# ---------------- projection-free kernels ----------------
SDPA = [(64, 64, 64), (64, 1, 96), (1, 64, 32), (63, 64, 40), (17, 64, 1024)]          # (queries S, keys T, E)


def _sdpa_case(B, S, T, E, dtype, seed):
    from aecf_amd.layer import _scaled_dot_product_attention
    from oracle import aecf_oracle as O
    g = torch.Generator().manual_seed(seed)
    r = lambda *sh: torch.randn(*sh, generator=g).to(dtype).float()
    q, k, v, dout = r(B, S, E), r(B, T, E), r(B, T, E), r(B, S, E)
    qd, kd, vd = (t_.to(DEV, dtype).requires_grad_(True) for t_ in (q, k, v))
    out = _scaled_dot_product_attention(qd, kd, vd)
    (out.float() * dout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    want = O.sdpa(q.double(), k.double(), v.double())
    dq, dk, dv = O.sdpa_backward(q.double(), k.double(), v.double(), dout.double())
    assert out.dtype == dtype and qd.grad.dtype == dtype
    return dict(out=rel_err(out.detach().cpu(), want), dq=rel_err(qd.grad.cpu(), dq), dk=rel_err(kd.grad.cpu(), dk),
                dv=rel_err(vd.grad.cpu(), dv))


@pytest.mark.parametrize("dtype_name", list(C.DTYPES))
@pytest.mark.parametrize("S,T,E", SDPA)
def test_sdpa_at_the_edges_of_its_score_array(S, T, E, dtype_name):
    """aecf_sdpa_forward / _backward keep their scores in a [64][65] LDS array: the last row and column (64 x 64), one query,
    one key, E that is not a multiple of 64 (a partial trip of the lane loop), E = 1024.  bf16: these kernels read q, k, v
    and dout once and round each output once (float32 in between), so the bound is the floor of the bf16 contract, 2^-8."""
    dtype = C.DTYPES[dtype_name]
    errs = _sdpa_case(3, S, T, E, dtype, 7000 + S + T + E)
    record_errors(f"mha_edges_sdpa_S{S}_T{T}_E{E}_{dtype_name}", **errs)
    bound = {"f32": 1e-5, "f16": F16_BOUND, "bf16": C.BF16_FLOOR}[dtype_name]
    for n, e in errs.items():
        assert e < bound, (n, e, bound)


def test_sdpa_batch_beyond_65535_blocks():
    errs = _sdpa_case(70000, 2, 3, 32, torch.float32, 7)
    for n, e in errs.items():
        assert e < 1e-5, (n, e)


@pytest.mark.parametrize("S,T", [(65, 4), (4, 65)])
def test_functional_fast_path_names_its_limit_above_64(S, T):
    """The reference's functional takes any length; the projection-free kernels stop at 64 queries and 64 keys.  The C entry
    answers AECF_ERR_UNSUPPORTED, and what the caller of multimodal_attention_pool(q, k) sees is an error that names the
    limit and the lengths it got -- not a bare status, and never numbers."""
    import aecf_amd
    from aecf_amd import _lib
    from aecf_amd.layer import _stream
    q, k = torch.randn(2, S, 32, device=DEV), torch.randn(2, T, 32, device=DEV)
    out, probs = torch.empty_like(q), torch.empty(2, S, T, device=DEV)
    st = _lib.load().aecf_sdpa_forward(2, S, T, 32, _lib.AECF_F32, 32 ** -0.5, q.data_ptr(), k.data_ptr(), k.data_ptr(),
                                       out.data_ptr(), probs.data_ptr(), _stream())
    assert st == -2
    with pytest.raises(RuntimeError, match=r"at most 64 queries and 64 keys") as ei:
        aecf_amd.multimodal_attention_pool(q, k)
    assert "not supported" in str(ei.value) and str(max(S, T)) in str(ei.value)
