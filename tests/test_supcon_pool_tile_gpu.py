"""The tile-GEMM form of the pooled supervised contrastive loss (EPI_SUP and EPI_SUP_SELF, sup_pool_combine_kernel, the two
sup_weights_kernel variants and the reused kernels of aecf_nce_gemm.hip) against float64 at its tile, shard and ragged edges, with
label positives on every boundary the geometry names, through the C ABI with ctypes and through pooled_supervised_contrastive /
fusion_objective.  Cases, the float64 reference and the derived elementwise bounds are those of tests/supcon_pool_tile_cases.py
(tests/test_supcon_pool_tile_cpu.py shows that the bounds hold an emulation of the arithmetic and catch the wrong rules).

Every shard of a global n x n problem runs as a rank would: aecf_supcon_pool_sym_pass1, the shards' col_stats added in float32 on
the device (the all-reduce), aecf_supcon_pool_sym_loss, aecf_supcon_pool_sym_grads.  Every output and the workspace come from the
Guarded helper of tests/test_abi_guards_gpu.py: the workspace is exactly the documented size and filled with 0xFF (NaN as bf16 and
as float32) before pass 1, the outputs are filled alike -- a finite output was written and read nothing that was not written
first."""
import functools

import pytest
import torch

from tests import supcon_pool_tile_cases as C
from tests.helpers import record_errors
from tests.test_abi_guards_gpu import Guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
CASE_T = [(cid, T) for cid in C.CASE_IDS for T in C.TEMPS]


def _libs():
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = C.make_case(cid)
    return c["a"].to(DEV), c["b"].to(DEV), c["lab"].to(DEV)


@functools.lru_cache(maxsize=None)
def _want(cid, T, upstream=1.0):
    """(T as the kernels read it, float64 reference, bounds) at coef * upstream, computed once on the device"""
    c = C.make_case(cid)
    a, b, lab = _inputs(cid)
    t = C.used_temperature(T)
    ref, bnd = C.reference(a, b, lab, c["shards"], t, c["coef"] * upstream, C.score_error(cid))
    return t, ref, bnd


def _run(cid, T, grad_dtype=F32, upstream=None, short=False, labels=None):
    """every shard as a rank runs it; outputs laid out as C.reference.  short: hand the first call a workspace size one byte short
    and return its status with the buffers it must not have touched.  labels: in place of the case's."""
    _lib, lib, _ptr, _stream = _libs()
    c = C.make_case(cid)
    a, b, lab = _inputs(cid)
    if labels is not None:
        lab = labels
    n, d = a.shape
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    up = None if upstream is None else torch.tensor([upstream], dtype=F32, device=DEV)
    gd = Guarded(DEV)
    held, stats = [], []
    for lo, hi in c["shards"]:
        rows = hi - lo
        al, bl, ll = a[lo:hi].contiguous(), b[lo:hi].contiguous(), lab[lo:hi].contiguous()
        wsb = lib.aecf_supcon_pool_sym_workspace_bytes(rows, n, d)
        assert wsb == C.workspace_bytes_py(rows, n, d)
        ws = gd.new(wsb, 0xFF)
        cs = gd.tensor((3, n), F32, 0xFF)
        if short:
            status = lib.aecf_supcon_pool_sym_pass1(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(bl), _ptr(a), _ptr(b), _ptr(ll),
                                                    _ptr(lab), _ptr(ws), wsb - 1, _ptr(cs), _stream())
            torch.cuda.synchronize()
            gd.check()
            return status, ws, cs
        assert lib.aecf_supcon_pool_sym_pass1(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(bl), _ptr(a), _ptr(b), _ptr(ll), _ptr(lab),
                                              _ptr(ws), wsb, _ptr(cs), _stream()) == 0
        held.append((al, bl, ll, ws, wsb))
        stats.append(cs)
    total = stats[0].clone()
    for cs in stats[1:]:
        total += cs                                              # the all-reduce: float32, rank order
    gdt = _lib.AECF_BF16 if grad_dtype == BF16 else _lib.AECF_F32
    lrows = gd.tensor((n,), F32, 0xFF)
    da_loc, db_loc = gd.tensor((n, d), grad_dtype, 0xFF), gd.tensor((n, d), grad_dtype, 0xFF)
    out = dict(colsum=[s[0] for s in stats], colcnt=[s[1] for s in stats], colsx=[s[2] for s in stats], loss_rows=lrows, da_loc=da_loc,
               db_loc=db_loc, da_all=[], db_all=[], dT=[])
    for (lo, hi), (al, bl, ll, ws, wsb) in zip(c["shards"], held):
        rows = hi - lo
        lr_s = gd.tensor((rows,), F32, 0xFF)
        o1, o2 = gd.tensor((rows, d), grad_dtype, 0xFF), gd.tensor((rows, d), grad_dtype, 0xFF)
        o3, o4 = gd.tensor((n, d), grad_dtype, 0xFF), gd.tensor((n, d), grad_dtype, 0xFF)
        d_t = gd.tensor((1,), F32, 0xFF)
        assert lib.aecf_supcon_pool_sym_loss(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(b), _ptr(total), _ptr(ws), wsb, _ptr(lr_s),
                                             _stream()) == 0
        assert lib.aecf_supcon_pool_sym_grads(rows, n, lo, d, _ptr(Tt), C.MIN_T, c["coef"], _ptr(al), _ptr(bl), _ptr(a), _ptr(b), _ptr(ll),
                                              _ptr(lab), _ptr(ws), wsb, _ptr(up), gdt, _ptr(o1), _ptr(o2), _ptr(o3), _ptr(o4), _ptr(d_t),
                                              _stream()) == 0
        torch.cuda.synchronize()
        lrows[lo:hi], da_loc[lo:hi], db_loc[lo:hi] = lr_s, o1, o2
        out["da_all"].append(o3)
        out["db_all"].append(o4)
        out["dT"].append(float(d_t))
    gd.check()
    return out


@functools.lru_cache(maxsize=None)
def _measured(cid, T):
    return _run(cid, T)


def _tensors(out):
    for name, v in out.items():
        if name != "dT":
            for k, t in enumerate(v if isinstance(v, list) else [v]):
                yield f"{name}[{k}]", t


def _judge(label, cid, T, out, upstream=1.0):
    """print the line of the profile, record it, assert every output finite and every ratio <= 1 -- no element is skipped"""
    _, ref, bnd = _want(cid, T, upstream)
    got = dict(out)
    for name, t in _tensors(out):
        assert bool(torch.isfinite(t).all()), (cid, T, name)
    for name in ("da_all", "db_all"):
        got[name + "_sum"] = sum(g.double() for g in out[name])   # the shares, added in float64 for the comparison
    r = C.ratios(got, ref, bnd)
    assert set(r) == set(C.OUTPUTS)
    sig = C.signal(ref, bnd)
    print(f"supcon_pool_tile_parity case {cid} T {T}{label}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items())
          + " | value/bound " + " ".join(f"{n}={sig[n]:.3g}" for n in r))
    record_errors(f"supcon_pool_tile_parity_{cid}", T=T, **r)
    for n, v in r.items():
        assert v <= 1.0, (cid, T, label, n, v)


@pytest.mark.parametrize("cid,T", CASE_T)
def test_inside_the_derived_bounds(cid, T):
    """every shard's col_stats (sums of E, counts, matched sums), the loss rows, the four gradients (the shares of the two gathered
    ones also added up against the summed bounds) and every shard's share of dT, float32 gradients"""
    _judge(" (float32 gradients)", cid, T, _measured(cid, T))


@pytest.mark.parametrize("cid,T", [(cid, T) for cid in C.TILE_IDS for T in C.TEMPS])
def test_bf16_gradients_are_the_float32_ones_rounded_once(cid, T):
    """every gradient output in bf16 has the bits of the float32 output rounded to nearest even: where two products land on one
    output they were summed in float32 first.  The loss rows, col_stats and dT know no gradient dtype."""
    out, f32 = _run(cid, T, grad_dtype=BF16), _measured(cid, T)
    for (name, x), (_, y) in zip(_tensors(out), _tensors(f32)):
        if name.split("[")[0] in C.GRADS:
            assert x.dtype == BF16 and torch.equal(x, y.to(BF16)), (cid, T, name)
        else:
            assert torch.equal(x, y), (cid, T, name)
    assert out["dT"] == f32["dT"]


@pytest.mark.parametrize("cid", ["S2", "S3", "S4"])
def test_upstream_scalar_scales_the_gradients(cid):
    """an upstream of 0.375 in device memory: the gradients and dT within the bounds taken at coef * 0.375; the loss rows and
    col_stats have the bits of the call without it"""
    T = 0.07
    out, plain = _run(cid, T, upstream=0.375), _measured(cid, T)
    for (name, x), (_, y) in zip(_tensors(out), _tensors(plain)):
        if name.split("[")[0] in C.STATS + ("loss_rows",):
            assert torch.equal(x, y), (cid, name)
    _judge(" (upstream 0.375)", cid, T, out, upstream=0.375)
    assert not torch.equal(out["da_loc"], plain["da_loc"])


@pytest.mark.parametrize("labels", ["unlabeled", "distinct"])
@pytest.mark.parametrize("cid", ["S2", "S3", "S4"])
def test_without_a_shared_label_every_output_has_the_bits_of_nt_xent(cid, labels):
    """every label -1, and all labels distinct (non-negative, the twins too): the loss rows, the four gradients, dT and row 0 of
    col_stats are torch.equal to aecf_ntxent_sym_pass1 / _loss / _grads on the same inputs; the counts and matched sums are 0"""
    from tests import test_ntxent_tile_gpu as NT
    T = 0.07
    n = C.make_case(cid)["a"].shape[0]
    lab = torch.full((n,), -1, dtype=torch.int64, device=DEV) if labels == "unlabeled" else \
        (torch.arange(n, dtype=torch.int64, device=DEV) * 3 + 2 ** 33)
    out, want = _run(cid, T, labels=lab), NT._measured(cid, T)
    for k in range(len(out["colsum"])):
        assert torch.equal(out["colsum"][k], want["colsum"][k]), (cid, k)
        assert not bool(out["colcnt"][k].any()) and not bool(out["colsx"][k].any()), (cid, k)
        assert torch.equal(out["da_all"][k], want["da_all"][k]) and torch.equal(out["db_all"][k], want["db_all"][k]), (cid, k)
    for name in ("loss_rows", "da_loc", "db_loc"):
        assert torch.equal(out[name], want[name]), (cid, name)
    assert out["dT"] == want["dT"]


@pytest.mark.parametrize("cid", ["S2", "S4"])
def test_col_stats_of_block_x_have_the_bits_of_the_cross_view_form(cid):
    """outside a rank's own range col_stats holds the column statistics of block X alone: the bits of aecf_supcon_sym_pass1 on the
    same inputs, all three quantities; inside it block Z's sums of E were added and row 0 is larger"""
    _lib, lib, _ptr, _stream = _libs()
    c = C.make_case(cid)
    a, b, lab = _inputs(cid)
    n, d = a.shape
    T = 0.07
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    got = _measured(cid, T)
    for k, (lo, hi) in enumerate(c["shards"]):
        rows = hi - lo
        al, ll = a[lo:hi].contiguous(), lab[lo:hi].contiguous()
        wsb = lib.aecf_supcon_sym_workspace_bytes(rows, n, d)
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        cs = torch.empty(3, n, dtype=F32, device=DEV)
        assert lib.aecf_supcon_sym_pass1(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(b), _ptr(ll), _ptr(lab), _ptr(ws), wsb, _ptr(cs),
                                         _stream()) == 0
        torch.cuda.synchronize()
        outside = torch.ones(n, dtype=torch.bool, device=DEV)
        outside[lo:hi] = False
        for q, name in enumerate(C.STATS):
            assert torch.equal(got[name][k][outside], cs[q][outside]), (cid, k, name)
        assert bool((got["colsum"][k][lo:hi] > cs[0][lo:hi]).all()), (cid, k)
        assert bool((got["colcnt"][k][lo:hi] >= cs[1][lo:hi]).all()), (cid, k)


def test_workspace_one_byte_short_is_refused_with_nothing_written():
    status, ws, cs = _run("S3", 0.07, short=True)
    assert status == -4
    assert bool((ws == 0xFF).all()) and bool((cs.view(torch.uint8) == 0xFF).all())


# ---- the Python surface ----

PY_T = 0.07


@functools.lru_cache(maxsize=None)
def _views():
    """views (n = 300, d = 192: a width the streaming form refuses) whose normalised rows are case S3's unit rows, scaled by powers
    of two (exact in bf16), and S3's labels"""
    c = C.make_case("S3")
    g = torch.Generator().manual_seed(5501)
    scale = 2.0 ** torch.randint(-1, 3, (c["a"].shape[0], 1), generator=g).float()
    return (c["a"].float() * scale).to(BF16).to(DEV), (c["b"].float() * scale.flip(0)).to(BF16).to(DEV), c["lab"].to(DEV)


@functools.lru_cache(maxsize=None)
def _wide_views():
    """a d = 256 batch both forms serve, with S3's labels"""
    g = torch.Generator().manual_seed(5502)
    return (torch.randn(300, 256, generator=g).to(BF16).to(DEV), torch.randn(300, 256, generator=g).to(BF16).to(DEV),
            C.make_case("S3")["lab"].to(DEV))


def _call(low_memory=False, T=PY_T, tensor_t=True, task=None, views=None, **more):
    """(loss, dza, dzb[, dT]) of one forward + backward of pooled_supervised_contrastive (task: through fusion_objective on that
    task loss)"""
    from aecf_amd import losses
    za, zb, lab = views or _views()
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    Tt = torch.tensor(T, dtype=F32, device=DEV, requires_grad=True) if tensor_t else T
    kw = dict(more) if low_memory == "default" else dict(more, low_memory=low_memory)
    if task is not None:
        loss = losses.fusion_objective(task, None, None, a, b, temperature=Tt, contrastive="supervised_pool", labels=lab, **kw)
    else:
        loss = losses.pooled_supervised_contrastive(a, b, lab, temperature=Tt, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return (loss.detach(), a.grad, b.grad) + ((Tt.grad,) if tensor_t else ())


def _equal(one, two):
    return all(torch.equal(x, y) for x, y in zip(one, two))


def test_python_tile_form_inside_the_bounds():
    """pooled_supervised_contrastive(low_memory=False) on S3's rows and labels with a tensor temperature: the loss, the bf16
    gradients of both views and dT against the float64 three-block reference on the unit rows the kernels read, taken back
    through the documented normalise backward.  On one rank a view's gradient is the bf16 sum of two bf16 outputs (its local and
    its gathered role): each bound plus 2^-8 |value| for its rounding, 2^-8 of the absolute sum for the addition; then
    _after_normalise of tests/test_nce_stream_gpu.py and the rounding of the result.  Under torch.no_grad() the value has the same
    bits."""
    from aecf_amd import losses
    from tests.test_nce_stream_gpu import _after_normalise
    za, zb, lab = _views()
    n = za.shape[0]
    loss, dza, dzb, dT = _call(False)
    assert dza.dtype == BF16 and dzb.dtype == BF16
    with torch.no_grad():
        quiet = losses.pooled_supervised_contrastive(za, zb, lab, temperature=torch.tensor(PY_T, dtype=F32, device=DEV),
                                                     low_memory=False)
        na, nb = losses.l2_normalize(za), losses.l2_normalize(zb)
    assert torch.equal(quiet, loss) and not quiet.requires_grad
    t, coef, half = C.used_temperature(PY_T), 0.5 / n, 2.0 ** -8
    s_err = 0.0
    for x, y in ((na, nb), (na, na), (nb, nb)):
        x, y = x.cpu(), y.cpu()
        s_err = max(s_err, float(((x.float() @ y.float().T).double() - x.double() @ y.double().T).abs().max()))
    ref, bnd = C.reference(na, nb, lab, [(0, n)], t, coef, s_err)
    want_loss = coef * float(ref["loss_rows"].sum())
    # the float32 sum of the rows (a tree: fewer than 2^4 roundings) and the product with coef
    b_loss = coef * float(bnd["loss_rows"].sum()) + 2.0 ** -19 * abs(want_loss)
    r = dict(loss=abs(float(loss) - want_loss) / b_loss,
             dT=abs(float(dT) - ref["dT"][0]) / (bnd["dT"][0] + 2.0 ** -23 * abs(ref["dT"][0])))
    for name, z, zn, loc, gathered, got in (("dza", za, na, "da_loc", "da_all", dza), ("dzb", zb, nb, "db_loc", "db_all", dzb)):
        terms = [(ref[loc], bnd[loc]), (ref[gathered][0], bnd[gathered][0])]
        g_ref = sum(v for v, _ in terms)
        e_sum = sum(b_ + half * (v.abs() + b_) for v, b_ in terms)              # each output rounded to bf16 once
        e_g = e_sum + half * (sum(v.abs() for v, _ in terms) + e_sum)           # one addition in bf16
        inv = 1.0 / z.double().norm(dim=1, keepdim=True)
        want, bound = _after_normalise(zn.double(), inv, g_ref, e_g)
        assert bool(torch.isfinite(got).all())
        r[name] = float(((got.double() - want).abs() / (bound + half * got.double().abs())).max())
    print(f"supcon_pool_tile_parity pooled_supervised_contrastive(low_memory=False) S3 T {PY_T}: "
          + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    record_errors("supcon_pool_tile_python", T=PY_T, **r)
    assert all(v <= 1.0 for v in r.values()), r


def test_python_float_and_tensor_temperature_give_the_same_bits():
    with_tensor, with_float = _call(False, tensor_t=True), _call(False, tensor_t=False)
    assert _equal(with_tensor[:3], with_float)


def test_python_second_backward_raises():
    from aecf_amd import losses
    za, zb, lab = _views()
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    loss = losses.pooled_supervised_contrastive(a, b, lab, low_memory=False)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="runs once per forward"):
        loss.backward()


def test_python_tile_form_refuses_what_it_does_not_serve():
    from aecf_amd import losses
    za, zb, lab = _views()
    with pytest.raises(NotImplementedError, match="bfloat16"):
        losses.pooled_supervised_contrastive(za.float(), zb.float(), lab, low_memory=False)
    with pytest.raises(NotImplementedError, match="d % 64"):
        losses.pooled_supervised_contrastive(za[:, :96].contiguous(), zb[:, :96].contiguous(), lab, low_memory=False)
    with pytest.raises(NotImplementedError, match="min_temperature"):
        losses.pooled_supervised_contrastive(za, zb, lab, min_temperature=1e-3, low_memory=False)
    with pytest.raises(ValueError, match="low_memory"):
        losses.pooled_supervised_contrastive(za, zb, lab, low_memory="tile")
    with pytest.raises(ValueError, match="labels"):
        losses.pooled_supervised_contrastive(za, zb, lab[:-1], low_memory=False)
    for kw in (dict(), dict(low_memory=True)):
        with pytest.raises(NotImplementedError, match="d in"):   # (the streaming form does not serve d = 192, message unchanged)
            losses.pooled_supervised_contrastive(za, zb, lab, **kw)
    with pytest.raises(NotImplementedError, match="intra-view"):  # (the old argument combination keeps its answer)
        losses.supervised_contrastive(za, zb, lab, low_memory=False, intra_view=True)


def test_python_default_and_low_memory_true_are_the_streaming_form_bit_for_bit():
    """pooled_supervised_contrastive(za, zb, labels) and low_memory=True against supervised_contrastive(za, zb, labels,
    intra_view=True) on a d = 256 batch: the loss and both gradients are torch.equal; the tile form is another implementation
    and close, not equal"""
    from aecf_amd import losses
    views = _wide_views()
    a, b = views[0].clone().requires_grad_(True), views[1].clone().requires_grad_(True)
    want = losses.supervised_contrastive(a, b, views[2], temperature=PY_T, intra_view=True)
    want.backward()
    torch.cuda.synchronize()
    want = (want.detach(), a.grad, b.grad)
    assert _equal(_call("default", tensor_t=False, views=views), want)
    assert _equal(_call(True, tensor_t=False, views=views), want)
    tile = _call(False, tensor_t=False, views=views)
    assert not _equal(tile, want)
    assert abs(float(tile[0]) - float(want[0])) <= 1e-3 * abs(float(want[0]))


def test_python_none_takes_the_tile_form_where_it_runs():
    """low_memory=None: the tile form on S3's rows (d = 192; its bits) and on the d = 256 batch, the streaming form below the tile
    form's temperature bound (min_temperature = 1e-3: the bits of low_memory=True)"""
    assert _equal(_call(None), _call(False))
    views = _wide_views()
    assert _equal(_call(None, views=views), _call(False, views=views))
    assert not _equal(_call(None, views=views), _call(True, views=views))
    assert _equal(_call(None, views=views, min_temperature=1e-3), _call(True, views=views, min_temperature=1e-3))


def test_fusion_objective_hands_low_memory_to_the_pooled_form():
    """fusion_objective(..., contrastive="supervised_pool", low_memory=False) is task + pooled_supervised_contrastive(...,
    low_memory=False) bit for bit, loss and gradients; intra_view is ignored for it"""
    task = torch.tensor(0.25, dtype=F32, device=DEV)
    through, alone = _call(False, task=task), _call(False)
    assert torch.equal(through[0], task + alone[0])
    assert _equal(through[1:], alone[1:])
    assert _equal(_call(False, task=task, intra_view=True), through)


def test_captured_step_reads_temperature_and_labels_at_replay():
    """forward + backward of the tile form inside torch.cuda.graph; new values written in place into the temperature tensor and the
    labels; the replay equals an eager call on the new values bit for bit (no host read anywhere)."""
    from aecf_amd import losses
    za, zb, labels = _views()
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    T = torch.tensor(0.07, dtype=F32, device=DEV, requires_grad=True)
    lab = torch.full_like(labels, -1)

    def step():
        return losses.pooled_supervised_contrastive(a, b, lab, temperature=T, low_memory=False)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            a.grad = b.grad = T.grad = None
            step().backward()
    torch.cuda.current_stream().wait_stream(s)
    a.grad = b.grad = T.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
        loss.backward()
    with torch.no_grad():
        T.copy_(torch.tensor(0.04))
        lab.copy_(labels)
    graph.replay()
    torch.cuda.synchronize()
    got = (loss.detach().clone(), a.grad.clone(), b.grad.clone(), T.grad.clone())
    want = _call(False, T=0.04)
    plain = losses.pooled_supervised_contrastive(za, zb, torch.full_like(labels, -1), temperature=0.04, low_memory=False)
    assert not torch.equal(plain, want[0])                        # the labels matter to the value the replay must reach
    assert _equal(got, want)
