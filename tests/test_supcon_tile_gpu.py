"""The tile-GEMM form of the symmetric supervised contrastive loss (EPI_SUP and the sup_* kernels of aecf_nce_gemm.hip) against
float64 at its tile, patch, shard and ragged edges, through the C ABI with ctypes and once through supervised_contrastive.
Cases, labels, the float64 reference and the derived elementwise bounds are those of tests/supcon_tile_cases.py
(tests/test_supcon_tile_cpu.py shows that the bounds hold an emulation of the arithmetic and catch the wrong match rules).

Every shard of a global n x n problem runs as a rank would: aecf_supcon_sym_pass1, the shards' column statistics added in float32
on the device (the all-reduce), aecf_supcon_sym_loss, aecf_supcon_sym_grads.  Every output and the workspace come from the Guarded
helper of tests/test_abi_guards_gpu.py: the workspace is exactly the documented size and filled with 0xFF (NaN as bf16 and as
float32) before pass 1, the outputs are filled alike -- a finite output was written and read nothing that was not written
first."""
import functools

import pytest
import torch

from tests import nce_tile_cases as N
from tests import supcon_tile_cases as C
from tests.helpers import record_errors
from tests.test_abi_guards_gpu import Guarded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
CASE_T = [(cid, T) for cid in C.ALL_IDS for T in C.TEMPS]


def _libs():
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    return _lib, _lib.load(), _ptr, _stream


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = C.make_case(cid)
    return c["a"].to(DEV), c["b"].to(DEV), c["lr"].to(DEV), c["lc"].to(DEV)


@functools.lru_cache(maxsize=None)
def _want(cid, T, upstream=1.0):
    """(T as the kernels read it, float64 reference, bounds) at coef * upstream, computed once on the device"""
    c = C.make_case(cid)
    a, b, lr, lc = _inputs(cid)
    t = C.used_temperature(T)
    ref, bnd = C.reference(a, b, lr, lc, c["shards"], t, c["coef"] * upstream, C.score_error(cid))
    return t, ref, bnd


def _run(cid, T, grad_dtype=F32, upstream=None, poison=0xFF, labels=None, short=False):
    """every shard as a rank runs it; outputs laid out as C.reference.  labels: (lr, lc) in place of the case's.  short: hand the
    first call a workspace size one byte short and return its status with the buffers it must not have touched."""
    _lib, lib, _ptr, _stream = _libs()
    c = C.make_case(cid)
    a, b, lr, lc = _inputs(cid)
    if labels is not None:
        lr, lc = labels
    n, d = a.shape
    Tt = torch.tensor([T], dtype=F32, device=DEV)
    up = None if upstream is None else torch.tensor([upstream], dtype=F32, device=DEV)
    gd = Guarded(DEV)
    held, stats = [], []
    for lo, hi in c["shards"]:
        rows = hi - lo
        al, ll = a[lo:hi].contiguous(), lr[lo:hi].contiguous()
        wsb = lib.aecf_supcon_sym_workspace_bytes(rows, n, d)
        assert wsb == C.workspace_bytes_py(rows, n, d)
        ws = gd.new(wsb, poison)
        cs = gd.tensor((3, n), F32, 0xFF)
        if short:
            status = lib.aecf_supcon_sym_pass1(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(b), _ptr(ll), _ptr(lc), _ptr(ws), wsb - 1,
                                               _ptr(cs), _stream())
            torch.cuda.synchronize()
            gd.check()
            return status, ws, cs
        assert lib.aecf_supcon_sym_pass1(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(b), _ptr(ll), _ptr(lc), _ptr(ws), wsb,
                                         _ptr(cs), _stream()) == 0
        held.append((al, ll, ws, wsb))
        stats.append(cs)
    total = stats[0].clone()
    for cs in stats[1:]:
        total += cs                                              # the all-reduce: float32, rank order
    gdt = _lib.AECF_BF16 if grad_dtype == BF16 else _lib.AECF_F32
    lrows, da = gd.tensor((n,), F32, 0xFF), gd.tensor((n, d), grad_dtype, 0xFF)
    out = dict(colsum=[s[0] for s in stats], colcnt=[s[1] for s in stats], colsx=[s[2] for s in stats], loss_rows=lrows, da=da,
               db=[], dT=[])
    for (lo, hi), (al, ll, ws, wsb) in zip(c["shards"], held):
        rows = hi - lo
        lr_s, da_s, db_s = gd.tensor((rows,), F32, 0xFF), gd.tensor((rows, d), grad_dtype, 0xFF), gd.tensor((n, d), grad_dtype, 0xFF)
        d_t = gd.tensor((1,), F32, 0xFF)
        assert lib.aecf_supcon_sym_loss(rows, n, lo, d, _ptr(Tt), C.MIN_T, _ptr(al), _ptr(b), _ptr(total), _ptr(ws), wsb, _ptr(lr_s),
                                        _stream()) == 0
        assert lib.aecf_supcon_sym_grads(rows, n, lo, d, _ptr(Tt), C.MIN_T, c["coef"], _ptr(al), _ptr(b), _ptr(ll), _ptr(lc), _ptr(ws),
                                         wsb, _ptr(up), gdt, _ptr(da_s), _ptr(db_s), _ptr(d_t), _stream()) == 0
        torch.cuda.synchronize()
        lrows[lo:hi], da[lo:hi] = lr_s, da_s
        out["db"].append(db_s)
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


def _same_bits(one, two, what, names=None):
    for (name, x), (_, y) in zip(_tensors(one), _tensors(two)):
        if names is None or name.split("[")[0] in names:
            assert torch.equal(x, y), (what, name)
    if names is None or "dT" in names:
        assert one["dT"] == two["dT"], (what, one["dT"], two["dT"])


def _judge(label, cid, T, out, bf16=False, upstream=1.0):
    """print the line of the profile, record it, assert every ratio <= 1 and every output finite"""
    _, ref, bnd = _want(cid, T, upstream)
    got = dict(out)
    for name, t in _tensors(out):
        assert bool(torch.isfinite(t).all()), (cid, T, name)
    if not bf16:
        got["db_sum"] = sum(g.double() for g in out["db"])
    r = C.ratios(got, ref, bnd, bf16=bf16)
    if bf16:
        # a sum of shares rounded to bf16 one by one: every share's rounding joins the summed bounds
        total = sum(g.double() for g in out["db"])
        r["db_sum"] = float(((total - ref["db_sum"]).abs() / (bnd["db_sum"] + 2.0 ** -8 * sum(g.double().abs() for g in out["db"]))).max())
    sig = C.signal(ref, bnd)
    print(f"supcon_tile_parity case {cid} T {T}{label}: " + " ".join(f"{n}={v:.3f}" for n, v in r.items())
          + " | value/bound " + " ".join(f"{n}={sig[n]:.3g}" for n in r))
    record_errors(f"supcon_tile_parity_{cid}", T=T, **r)
    for n, v in r.items():
        assert v <= 1.0, (cid, T, label, n, v)


@pytest.mark.parametrize("cid,T", CASE_T)
def test_inside_the_derived_bounds(cid, T):
    """the three column statistics of every shard, loss rows, da, every shard's share of db and of dT, and the shares of db added
    up against the summed bounds, float32 gradients"""
    _judge(" (float32 gradients)", cid, T, _measured(cid, T))


@pytest.mark.parametrize("cid,T", CASE_T)
def test_bf16_gradients_inside_the_derived_bounds(cid, T):
    """bf16 gradient outputs and an upstream of 0.375 in device memory: the bounds at coef * 0.375 plus 2^-8 |value|; the loss
    rows and column statistics know no upstream"""
    out = _run(cid, T, grad_dtype=BF16, upstream=0.375)
    assert out["da"].dtype == BF16
    _same_bits(out, _measured(cid, T), (cid, T), names=("colsum", "colcnt", "colsx", "loss_rows"))
    _judge(" (bf16 gradients, upstream 0.375)", cid, T, out, bf16=True, upstream=0.375)


@pytest.mark.parametrize("cid", ["S2", "S4"])
def test_zero_filled_workspace_gives_the_same_bits(cid):
    """nothing of the workspace is read before it is written: zeros in place of NaNs cannot move a bit"""
    _same_bits(_measured(cid, 0.07), _run(cid, 0.07, poison=0x00), cid)


def test_workspace_one_byte_short_is_refused_with_nothing_written():
    status, ws, cs = _run("S3", 0.07, short=True)
    assert status == -4
    assert bool((ws == 0xFF).all()) and bool((cs.view(torch.uint8) == 0xFF).all())


@pytest.mark.parametrize("cid", ["S2", "S3"])
def test_temperature_below_the_minimum_is_clamped(cid):
    """*T = 0.01 < min_temperature = 0.025: dT is exactly 0, every other output has the bits of *T = 0.025"""
    low, at = _run(cid, 0.01), _run(cid, C.MIN_T)
    assert all(v == 0.0 for v in low["dT"]) and any(v != 0.0 for v in at["dT"])
    _same_bits(low, at, cid, names=("colsum", "colcnt", "colsx", "loss_rows", "da", "db"))


@pytest.mark.parametrize("labels", ["all_unlabeled", "all_distinct"])
@pytest.mark.parametrize("cid", ["S2", "S3", "S4"])
def test_without_shared_labels_it_is_symmetric_info_nce_bit_for_bit(cid, labels):
    """every label -1, or all labels distinct: the column sums of E, loss rows, da, db and dT have the bits of aecf_nce_sym_pass1_dt /
    _loss_dt / _grads_dt on the same inputs; no column has a match"""
    from tests.test_nce_tile_gpu import _run_symmetric
    n = _inputs(cid)[0].shape[0]
    lab = torch.full((n,), -1, dtype=torch.int64, device=DEV) if labels == "all_unlabeled" else \
        (torch.arange(n, dtype=torch.int64, device=DEV) * 3 + 2 ** 33)
    for T in C.TEMPS:
        got, want = _run(cid, T, labels=(lab, lab)), _run_symmetric(cid, T, dt=True)
        for k in range(len(want["colsum"])):
            assert torch.equal(got["colsum"][k], want["colsum"][k]), (cid, T, k)
            assert not bool(got["colcnt"][k].any()) and not bool(got["colsx"][k].any())
            assert torch.equal(got["db"][k], want["db"][k]), (cid, T, k)
        assert torch.equal(got["loss_rows"], want["loss_rows"]) and torch.equal(got["da"], want["da"]), (cid, T)
        assert got["dT"] == want["dT"], (cid, T)


# ---- the Python surface ----

PY_T = 0.07


@functools.lru_cache(maxsize=None)
def _views(cid="S3"):
    """views whose normalised rows are a case's unit rows, scaled by powers of two (exact in bf16), and the case's labels.  S3
    (d = 192) is served by the tile form alone; S2 (d = 128) by both forms."""
    c = C.make_case(cid)
    g = torch.Generator().manual_seed(5301)
    scale = 2.0 ** torch.randint(-1, 3, (c["a"].shape[0], 1), generator=g).float()
    return (c["a"].float() * scale).to(BF16).to(DEV), (c["b"].float() * scale.flip(0)).to(BF16).to(DEV), c["lc"].to(DEV)


def _call(low_memory="default", min_temperature=C.MIN_T, T=PY_T, through_objective=False, cid="S3"):
    """(loss, dza, dzb, dT) of one forward + backward of supervised_contrastive on the views of a case"""
    from aecf_amd import losses
    za, zb, lab = _views(cid)
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    Tt = torch.tensor(T, dtype=F32, device=DEV, requires_grad=True)
    kw = {} if low_memory == "default" else dict(low_memory=low_memory)
    if through_objective:
        loss = losses.fusion_objective(torch.zeros((), dtype=F32, device=DEV), None, None, a, b, temperature=Tt,
                                       min_temperature=min_temperature, contrastive="supervised", labels=lab, **kw)
    else:
        loss = losses.supervised_contrastive(a, b, lab, temperature=Tt, min_temperature=min_temperature, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), a.grad, b.grad, Tt.grad


def test_python_tile_form_inside_the_bounds():
    """supervised_contrastive(low_memory=False) on case S3 with a tensor temperature: the loss, the bf16 gradients of both views
    and dT against the float64 one-block reference on the unit rows the kernels read, taken back through the documented normalise
    backward.  Bounds: the da / db bounds at coef = 0.5 / n plus 2^-8 |value| for each bf16 output, _after_normalise of
    tests/test_nce_stream_gpu.py, the rounding of the result.  na and nb are the library's own l2_normalize outputs."""
    from aecf_amd import losses
    from tests.test_nce_stream_gpu import _after_normalise
    za, zb, lab = _views()
    n = za.shape[0]
    loss, dza, dzb, dT = _call(False)
    assert dza.dtype == BF16 and dzb.dtype == BF16
    with torch.no_grad():
        na, nb = losses.l2_normalize(za), losses.l2_normalize(zb)
    t, coef, half = C.used_temperature(PY_T), 0.5 / n, 2.0 ** -8
    s_err = float((na.cpu().float() @ nb.cpu().float().T - na.cpu().double() @ nb.cpu().double().T).abs().max())
    ref, bnd = C.reference(na, nb, lab, lab, [(0, n)], t, coef, s_err)
    want_loss = coef * float(ref["loss_rows"].sum())
    # the float32 sum of the rows (a tree: fewer than 2^4 roundings) and the product with coef
    b_loss = coef * float(bnd["loss_rows"].sum()) + 2.0 ** -19 * abs(want_loss)
    r = dict(loss=abs(float(loss) - want_loss) / b_loss,
             dT=abs(float(dT) - ref["dT"][0]) / (bnd["dT"][0] + 2.0 ** -23 * abs(ref["dT"][0])))
    for name, z, zn, g_ref, b_g, got in (("dza", za, na, ref["da"], bnd["da"], dza), ("dzb", zb, nb, ref["db"][0], bnd["db"][0], dzb)):
        e_g = b_g + half * (g_ref.abs() + b_g)
        inv = 1.0 / z.double().norm(dim=1, keepdim=True)
        want, bound = _after_normalise(zn.double(), inv, g_ref, e_g)
        assert bool(torch.isfinite(got).all())
        r[name] = float(((got.double() - want).abs() / (bound + half * got.double().abs())).max())
    print(f"supcon_tile_parity supervised_contrastive(low_memory=False) S3 T {PY_T}: " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    record_errors("supcon_tile_python", T=PY_T, **r)
    assert all(v <= 1.0 for v in r.values()), r


def _equal(one, two):
    return all(torch.equal(x, y) for x, y in zip(one, two))


def test_python_forms_are_chosen_as_documented():
    """None takes the tile form where it runs and the streaming form below the tile form's temperature bound; the default is the
    streaming form; fusion_objective hands low_memory on.  On S3 (d = 192, no streaming kernel) and on S2 (d = 128, both forms)."""
    from aecf_amd import losses
    tile3 = _call(False)
    assert _equal(_call(None), tile3)
    assert _equal(_call(False, through_objective=True), tile3)
    za, zb, lab = _views()
    for kw in (dict(), dict(low_memory=True), dict(low_memory=None, min_temperature=1e-3)):
        with pytest.raises(NotImplementedError, match="d in"):   # (the streaming form does not serve d = 192)
            losses.supervised_contrastive(za, zb, lab, **kw)
    tile, stream = _call(False, cid="S2"), _call(True, cid="S2")
    assert not _equal(tile, stream)                              # (two implementations: the bits differ)
    assert _equal(_call(None, cid="S2"), tile)
    assert _equal(_call("default", cid="S2"), stream)
    assert _equal(_call(None, min_temperature=1e-3, cid="S2"), _call(True, min_temperature=1e-3, cid="S2"))
    assert _equal(_call(False, through_objective=True, cid="S2"), tile)
    assert _equal(_call("default", through_objective=True, cid="S2"), stream)


def test_python_tile_form_refuses_what_it_does_not_serve():
    from aecf_amd import losses
    za, zb, lab = _views()
    with pytest.raises(NotImplementedError, match="bfloat16"):
        losses.supervised_contrastive(za.float(), zb.float(), lab, low_memory=False)
    with pytest.raises(NotImplementedError, match="d % 64"):
        losses.supervised_contrastive(za[:, :96].contiguous(), zb[:, :96].contiguous(), lab, low_memory=False)
    with pytest.raises(NotImplementedError, match="min_temperature"):
        losses.supervised_contrastive(za, zb, lab, min_temperature=1e-3, low_memory=False)


def test_python_second_backward_raises():
    from aecf_amd import losses
    za, zb, lab = _views()
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    loss = losses.supervised_contrastive(a, b, lab, low_memory=False)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="runs once per forward"):
        loss.backward()


def test_captured_step_reads_temperature_and_labels_at_replay():
    """forward + backward of the tile form inside torch.cuda.graph; new values written in place into the temperature tensor and the
    labels; the replay equals an eager call on the new values bit for bit (no host read anywhere)."""
    from aecf_amd import losses
    za, zb, labels = _views()
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    T = torch.tensor(0.07, dtype=F32, device=DEV, requires_grad=True)
    lab = torch.full_like(labels, -1)

    def step():
        return losses.supervised_contrastive(a, b, lab, temperature=T, low_memory=False)

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
    plain = losses.supervised_contrastive(za, zb, torch.full_like(labels, -1), temperature=0.04, low_memory=False)
    assert not torch.equal(plain, want[0])                        # the labels matter to the value the replay must reach
    assert _equal(got, want)
