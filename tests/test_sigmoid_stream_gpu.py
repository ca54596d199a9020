"""The streaming form of the pairwise sigmoid (SigLIP) loss: aecf_sig_stream_fwd_bwd and losses.sigmoid_contrastive(...,
low_memory=...), which never hold the rows x cols block of g.

The yardstick is the one of tests/test_sigmoid_loss_gpu.py, restated here: float64 autograd of the header's formulas on the same
bf16-rounded unit-norm rows the kernels read,

    Tc = max(T, min_temperature);  l_ij = a_i . b_j / Tc + bias;  L = 1/C sum_ij softplus(-y_ij l_ij),  y = +1 on j == off + i, else -1

and so are the bounds: loss 2e-3, loss rows 1e-3, dT and dbias 5e-3, da / db rel_err 1.5e-2 (g is rounded once to bf16).

Shapes that tests/test_sigmoid_loss_gpu.py does not have were admitted by its criterion: the float64 conditioning
|sum terms| / sum |terms| of dT and of dbias, computed once on the CPU from the same generator, is at least 0.45 --
    (70, 130, off 37), seed 3, (T, bias) = (0.1, -10): dT 0.998 / 0.999 / 0.999 / 0.999 / 1.000 / 1.000 at d = 128 .. 1024, dbias 0.980 .. 0.986
    (70, 1100, off 500), d = 256, seed 3, (0.1, -10):  dT 0.992, dbias 0.871
    (320, 320, off 0), d = 256, seed 3, (0.1, -10):    dT 0.998, dbias 0.961
((0.1, -2) fails it at (70, 130) from d = 512 up: dT 0.46 .. 0.31.)"""
import math

import pytest
import torch

from tests.helpers import record_errors, rel_err

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LOSS, SCALAR_GRAD, ROW_GRAD, LOSS_ROWS = 2e-3, 5e-3, 1.5e-2, 1e-3
SHAPES = [(333, 256), (1000, 512)]
WIDTHS = (128, 256, 384, 512, 768, 1024)


def _views(n, d, dtype=torch.bfloat16, seed=3):
    g = torch.Generator().manual_seed(seed)
    za = torch.randn(n, d, generator=g)
    zb = 0.8 * za + 0.6 * torch.randn(n, d, generator=g)
    return za.to(dtype).to(DEV), zb.to(dtype).to(DEV)


def _normed(za, zb):
    from aecf_amd import losses
    return losses.l2_normalize(za).detach(), losses.l2_normalize(zb).detach()


def _rel(got, want):
    got, want = (float(x.detach()) if isinstance(x, torch.Tensor) else float(x) for x in (got, want))
    return abs(got - want) / abs(want)


def _ref(a, b, T, bias, off=0, min_t=1e-3, coef=None):
    """float64 autograd of the objective for rows a [R, d] (positives at column off + i) against b [C, d]; a and b may carry a
    graph.  Returns loss, loss rows (without coef) and the gradients on a, b, T and the bias."""
    a = a.double() if a.requires_grad else a.detach().double().requires_grad_(True)
    b = b.double() if b.requires_grad else b.detach().double().requires_grad_(True)
    t = torch.tensor(float(T), dtype=torch.float64, device=a.device, requires_grad=True)
    bs = torch.tensor(float(bias), dtype=torch.float64, device=a.device, requires_grad=True)
    l = a @ b.T / torch.clamp(t, min=min_t) + bs
    y = -torch.ones_like(l)
    i = torch.arange(a.shape[0], device=a.device)
    y[i, off + i] = 1.0
    terms = torch.nn.functional.softplus(-y * l)
    coef = 1.0 / b.shape[0] if coef is None else coef
    loss = coef * terms.sum()
    ga, gb, gt, gbs = torch.autograd.grad(loss, [a, b, t, bs], retain_graph=True)
    return dict(loss=loss.item(), rows=terms.sum(1).detach(), da=ga, db=gb, dT=gt.item(), dbias=gbs.item(), graph=(loss, a, b))


def _scalars(T, bias):
    return torch.tensor([T], device=DEV), torch.tensor([bias], device=DEV)


def _stream_call(a, b, off, T, bias, min_t=1e-3, coef=None, guard=0, loss_only=False):
    """aecf_sig_stream_fwd_bwd through the C ABI on a workspace of exactly aecf_sig_stream_workspace_bytes (+ guard bytes)."""
    from aecf_amd import _lib
    from aecf_amd.layer import _ptr, _stream
    lib = _lib.load()
    rows, d = a.shape
    cols = b.shape[0]
    coef = 1.0 / cols if coef is None else coef
    f32 = dict(dtype=torch.float32, device=DEV)
    wsb = lib.aecf_sig_stream_workspace_bytes(rows, cols, d)
    assert wsb > 0
    ws = torch.full((wsb + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    lr = torch.empty(rows, **f32)
    if loss_only:
        dbias = dT = da = db = None
    else:
        dbias, dT = torch.empty(1, **f32), torch.empty(1, **f32)
        da, db = torch.empty(rows, d, **f32), torch.empty(cols, d, **f32)
    _lib.check(lib.aecf_sig_stream_fwd_bwd(rows, cols, off, d, _ptr(T), min_t, _ptr(bias), coef, _ptr(a), _ptr(b), _ptr(lr), _ptr(dbias),
                                           _ptr(dT), _ptr(da), _ptr(db), _ptr(ws), wsb, _stream()), "aecf_sig_stream_fwd_bwd")
    torch.cuda.synchronize()
    out = dict(rows=lr, loss=float(lr.double().sum()) * coef, ws=ws, wsb=wsb)
    if not loss_only:
        out.update(dbias=float(dbias) * coef, dT=float(dT), da=da, db=db, raw=(lr, dbias, dT, da, db))
    return out


def _all_errs(got, want):
    return dict(rows=rel_err(got["rows"], want["rows"]), loss=_rel(got["loss"], want["loss"]), dbias=_rel(got["dbias"], want["dbias"]),
                dT=_rel(got["dT"], want["dT"]), da=rel_err(got["da"], want["da"]), db=rel_err(got["db"], want["db"]))


def _check_all(tag, errs, **where):
    print(f"{tag} {where}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    record_errors(tag, **where, **errs)
    assert errs["rows"] < LOSS_ROWS and errs["loss"] < LOSS
    assert errs["dbias"] < SCALAR_GRAD and errs["dT"] < SCALAR_GRAD
    assert errs["da"] < ROW_GRAD and errs["db"] < ROW_GRAD


# measured on the MI355X (maxima over the five cases): loss rows 4.2e-7, loss 4.2e-7, dbias 5.1e-7, dT 3.2e-4, da 1.4e-3, db 1.7e-3
@pytest.mark.parametrize("rows,cols,off", [(1, 1, 0), (65, 257, 100), (63, 300, 200), (257, 300, 43), (256, 512, 256)])
def test_ragged_shapes_offsets_and_guard_band(rows, cols, off):
    """Row and column counts that fill no tile, positives at an offset: every output against float64 (a padded row or column that
    entered a sum would add softplus(bias) or a sigmoid to it), and the 4096 bytes after the workspace stay as they were."""
    d = 128
    za, zb = _views(cols, d, seed=11)
    na, nb = _normed(za, zb)
    a = na[off:off + rows].contiguous()
    T, bs = _scalars(0.1, -2.0)
    got = _stream_call(a, nb, off, T, bs, guard=4096)
    want = _ref(a, nb, 0.1, -2.0, off=off)
    assert got["ws"].numel() == got["wsb"] + 4096 and bool((got["ws"][got["wsb"]:] == 0xA5).all())
    assert all(bool(torch.isfinite(x).all()) for x in got["raw"])
    _check_all("sigmoid_stream_edges", _all_errs(got, want), n_rows=rows, n_cols=cols, off=off)


# measured on the MI355X (maxima over the six widths): loss rows 1.3e-6, loss 2.5e-7, dbias 5.8e-8, dT 2.5e-4, da 2.1e-3, db 2.0e-3
@pytest.mark.parametrize("d", WIDTHS)
def test_every_served_width(d):
    """Each width once (d = 768 and 1024 produce their output columns in two launches per role), at a shape that fills no tile."""
    rows, cols, off = 70, 130, 37
    za, zb = _views(cols, d)
    na, nb = _normed(za, zb)
    a = na[off:off + rows].contiguous()
    T, bs = _scalars(0.1, -10.0)
    got = _stream_call(a, nb, off, T, bs)
    want = _ref(a, nb, 0.1, -10.0, off=off)
    _check_all("sigmoid_stream_widths", _all_errs(got, want), d=d)


# measured on the MI355X: loss rows 6.2e-7, loss 3.2e-8, dbias 2.9e-8, dT 9.9e-5, da 1.8e-3, db 2.0e-3
def test_split_column_range_is_reproducible():
    """(70, 1100): the split rule (InfoNCE's flash rule: at least 512 columns per split, split length rounded up to 32) gives
    three splits of 384, 384 and a ragged 332 columns.  The rule then counts the splits from that length (ceil(cols / length)),
    so it cannot yield an empty split.  Fixed-order sums: two runs give identical bits on all five outputs."""
    rows, cols, off, d = 70, 1100, 500, 256
    za, zb = _views(cols, d)
    na, nb = _normed(za, zb)
    a = na[off:off + rows].contiguous()
    T, bs = _scalars(0.1, -10.0)
    got = _stream_call(a, nb, off, T, bs)
    # three splits: [3, rows, d + 2] partials + the two per-row sums
    assert got["wsb"] == (3 * rows * (d + 2) + 2 * rows) * 4 + 1024
    want = _ref(a, nb, 0.1, -10.0, off=off)
    _check_all("sigmoid_stream_split", _all_errs(got, want), n_rows=rows, n_cols=cols)
    again = _stream_call(a, nb, off, T, bs)
    assert all(torch.equal(x, y) for x, y in zip(got["raw"], again["raw"]))


def test_saturated_logits_stay_finite():
    """1 / T = 1000 (logits far past the float32 exponent range of exp) and a bias of -30 (sigmoid ~ e^-30): no NaN, and the
    loss and the row gradients keep their accuracy."""
    za, zb = _views(300, 128, seed=5)
    na, nb = _normed(za, zb)
    for T, bias in [(1e-3, 0.0), (1.0, -30.0)]:
        Tt, bs = _scalars(T, bias)
        got = _stream_call(na, nb, 0, Tt, bs)
        want = _ref(na, nb, T, bias)
        assert all(bool(torch.isfinite(x).all()) for x in got["raw"])
        errs = dict(loss=_rel(got["loss"], want["loss"]), da=rel_err(got["da"], want["da"]), db=rel_err(got["db"], want["db"]))
        print(f"sigmoid stream saturation (T {T}, bias {bias}): " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
        record_errors("sigmoid_stream_saturation", T=T, bias=bias, **errs)
        assert errs["loss"] < LOSS
        assert errs["da"] < ROW_GRAD and errs["db"] < ROW_GRAD


def test_emulated_ranks_sum_to_the_global_values():
    """Two emulated ranks (rows [0, n/3) and [n/3, n) of (333, 256) against all columns): nothing is exchanged, the shares of loss,
    dbias, dT and db add up to the global float64 values and da concatenates to them."""
    n, d = 333, 256
    za, zb = _views(n, d)
    na, nb = _normed(za, zb)
    T, bs = _scalars(0.1, -10.0)
    want = _ref(na, nb, 0.1, -10.0)
    cut = n // 3
    parts = [_stream_call(na[lo:hi].contiguous(), nb, lo, T, bs) for lo, hi in [(0, cut), (cut, n)]]
    errs = dict(loss=_rel(sum(p["loss"] for p in parts), want["loss"]), dbias=_rel(sum(p["dbias"] for p in parts), want["dbias"]),
                dT=_rel(sum(p["dT"] for p in parts), want["dT"]), rows=rel_err(torch.cat([p["rows"] for p in parts]), want["rows"]),
                da=rel_err(torch.cat([p["da"] for p in parts]), want["da"]), db=rel_err(parts[0]["db"] + parts[1]["db"], want["db"]))
    _check_all("sigmoid_stream_shards", errs, n=n, d=d)


def test_loss_only_mode_gives_the_same_loss_bits():
    """da = db = NULL (d_bias and d_temperature NULL too): loss_rows alone, the bits of the full call -- at a one-split shape,
    at the three-split shape and at a width with two column launches; and through Python, the value under no_grad is the
    training call's value bit for bit."""
    from aecf_amd import losses
    for rows, cols, off, d in [(65, 257, 100, 128), (70, 1100, 500, 256), (70, 130, 37, 768)]:
        za, zb = _views(cols, d)
        na, nb = _normed(za, zb)
        a = na[off:off + rows].contiguous()
        T, bs = _scalars(0.1, -10.0)
        full = _stream_call(a, nb, off, T, bs)
        only = _stream_call(a, nb, off, T, bs, loss_only=True, guard=4096)
        assert torch.equal(only["rows"], full["rows"])
        assert bool((only["ws"][only["wsb"]:] == 0xA5).all())
    za, zb = _views(333, 256)
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    T = torch.tensor(0.1, device=DEV, requires_grad=True)
    train = losses.sigmoid_contrastive(a, b, temperature=T, bias=-10.0, low_memory=True)
    assert train.requires_grad
    with torch.no_grad():
        evaluated = losses.sigmoid_contrastive(a, b, temperature=T, bias=-10.0, low_memory=True)
    assert not evaluated.requires_grad and torch.equal(evaluated, train.detach())
    plain = losses.sigmoid_contrastive(za, zb, temperature=0.1, bias=-10.0, low_memory=True)      # nothing requires grad
    assert torch.equal(plain, train.detach())


def _grads(fn, za, zb):
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    loss = fn(a, b)
    loss.backward()
    return loss.detach(), a.grad, b.grad


# measured on the MI355X ((333, 256) / (1000, 512)): loss 3.8e-8 / 2.2e-8, logit_scale.grad 5.4e-5 / 1.1e-5, bias.grad 1.9e-8 / 3.8e-8,
# za.grad 5.7e-3 / 7.2e-3, zb.grad 7.4e-3 / 7.4e-3 (the last two carry the bf16 rounding of g and of the normalise backward)
@pytest.mark.parametrize("n,d", SHAPES)
def test_python_surface_matches_float64(n, d):
    """sigmoid_contrastive(low_memory=True) with tensor temperature 1 / logit_scale.exp() and tensor bias, gradients on za, zb,
    logit_scale and the bias; the float64 reference reads the bf16 unit rows the kernels read and differentiates through a
    float64 normalise (the scheme of test_sigmoid_contrastive_matches_float64)."""
    from aecf_amd import losses
    T, bias = 0.1, -10.0
    za, zb = _views(n, d)
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    ls = torch.tensor(math.log(1.0 / T), device=DEV, requires_grad=True)
    bs = torch.tensor(bias, device=DEV, requires_grad=True)
    loss = losses.sigmoid_contrastive(a, b, temperature=1 / ls.exp(), bias=bs, low_memory=True)
    loss.backward()
    t_used = float(1 / ls.detach().exp())

    def through_norm(z, unit):                      # value: the bf16 unit rows; gradient: through the float64 normalise
        z64 = z.detach().double().requires_grad_(True)
        u = z64 / z64.norm(dim=1, keepdim=True)
        return z64, u + (unit.double() - u).detach()

    na, nb = _normed(za, zb)
    a64, ua = through_norm(za, na)
    b64, ub = through_norm(zb, nb)
    want = _ref(ua, ub, t_used, bias)
    wa, wb = torch.autograd.grad(want["graph"][0], [a64, b64])
    errs = dict(loss=_rel(loss, want["loss"]), dT=_rel(ls.grad, want["dT"] * (-t_used)), dbias=_rel(bs.grad, want["dbias"]),
                da=rel_err(a.grad, wa), db=rel_err(b.grad, wb))
    print(f"sigmoid stream parity ({n}, {d}): " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    record_errors("sigmoid_stream_parity", n=n, d=d, **errs)
    assert errs["loss"] < LOSS
    assert errs["dT"] < SCALAR_GRAD and errs["dbias"] < SCALAR_GRAD
    assert errs["da"] < ROW_GRAD and errs["db"] < ROW_GRAD


@pytest.mark.parametrize("n,d", SHAPES)
def test_python_surface_forms_and_routing(n, d):
    from aecf_amd import losses
    za, zb = _views(n, d)
    # a float temperature and bias give the bits of one-element tensors holding them
    got = _grads(lambda a, b: losses.sigmoid_contrastive(a, b, temperature=0.07, bias=-5.0, low_memory=True), za, zb)
    T, bs = torch.tensor(0.07, device=DEV), torch.tensor([-5.0], device=DEV)
    want = _grads(lambda a, b: losses.sigmoid_contrastive(a, b, temperature=T, bias=bs, low_memory=True), za, zb)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    # fusion_objective passes the flag on
    fused = _grads(lambda a, b: losses.fusion_objective(torch.zeros((), device=DEV), None, None, a, b, temperature=0.07,
                                                        min_temperature=1e-3, contrastive="sigmoid", bias=-5.0, low_memory=True),
                   za, zb)
    for x, y in zip(fused, want):
        assert torch.equal(x, y)
    # None takes the tile form where it fits: the bits of low_memory=False
    auto = _grads(lambda a, b: losses.sigmoid_contrastive(a, b, temperature=0.07, bias=-5.0), za, zb)
    tile = _grads(lambda a, b: losses.sigmoid_contrastive(a, b, temperature=0.07, bias=-5.0, low_memory=False), za, zb)
    for x, y in zip(auto, tile):
        assert torch.equal(x, y)
    assert auto[1].dtype == torch.bfloat16


def test_automatic_fallback_when_the_block_does_not_fit(monkeypatch):
    """With 1 MiB reported free, the default call runs the streaming form instead of raising; low_memory=False still raises;
    and low_memory=True names the served widths where there is no streaming form."""
    from aecf_amd import losses
    total = torch.cuda.mem_get_info(DEV)[1]
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *args, **kw: (1 << 20, total))
    za, zb = _views(320, 256)
    a, b = za.clone().requires_grad_(True), zb.clone().requires_grad_(True)
    T = torch.tensor(0.1, device=DEV, requires_grad=True)
    bs = torch.tensor(-10.0, device=DEV, requires_grad=True)
    loss = losses.sigmoid_contrastive(a, b, temperature=T, bias=bs)
    loss.backward()
    defaults = losses.sigmoid_contrastive(za, zb)                     # T = 0.1, bias = -10 are the defaults
    assert torch.equal(defaults, loss.detach())

    def through_norm(z, unit):
        z64 = z.detach().double().requires_grad_(True)
        u = z64 / z64.norm(dim=1, keepdim=True)
        return z64, u + (unit.double() - u).detach()

    na, nb = _normed(za, zb)
    a64, ua = through_norm(za, na)
    b64, ub = through_norm(zb, nb)
    want = _ref(ua, ub, 0.1, -10.0)
    wa, wb = torch.autograd.grad(want["graph"][0], [a64, b64])
    errs = dict(loss=_rel(loss, want["loss"]), dT=_rel(T.grad, want["dT"]), dbias=_rel(bs.grad, want["dbias"]),
                da=rel_err(a.grad, wa), db=rel_err(b.grad, wb))
    print("sigmoid stream fallback: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    record_errors("sigmoid_stream_fallback", **errs)
    assert errs["loss"] < LOSS
    assert errs["dT"] < SCALAR_GRAD and errs["dbias"] < SCALAR_GRAD
    assert errs["da"] < ROW_GRAD and errs["db"] < ROW_GRAD
    with pytest.raises(NotImplementedError, match="0.6 of the free device memory"):
        losses.sigmoid_contrastive(za, zb, low_memory=False)
    z192 = _views(64, 192)
    with pytest.raises(NotImplementedError, match=r"128, 256, 384, 512, 768, 1024"):
        losses.sigmoid_contrastive(*z192, low_memory=True)


def test_captured_step_reads_temperature_and_bias_at_replay():
    from aecf_amd import losses
    za, zb = _views(512, 256)
    a = za.clone().requires_grad_(True)
    T = torch.tensor(0.1, device=DEV, requires_grad=True)
    bs = torch.tensor(-10.0, device=DEV, requires_grad=True)

    def step():
        return losses.sigmoid_contrastive(a, zb, temperature=T, bias=bs, low_memory=True)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            a.grad = T.grad = bs.grad = None
            step().backward()
    torch.cuda.current_stream().wait_stream(s)
    a.grad = T.grad = bs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
        loss.backward()
    with torch.no_grad():
        T.copy_(torch.tensor(0.07))
        bs.copy_(torch.tensor(-5.0))
    graph.replay()
    torch.cuda.synchronize()
    got = (loss.detach().clone(), a.grad.clone(), T.grad.clone(), bs.grad.clone())
    a2 = za.clone().requires_grad_(True)
    T2 = torch.tensor(0.07, device=DEV, requires_grad=True)
    b2 = torch.tensor(-5.0, device=DEV, requires_grad=True)
    want = losses.sigmoid_contrastive(a2, zb, temperature=T2, bias=b2, low_memory=True)
    want.backward()
    assert torch.equal(got[0], want.detach())
    assert torch.equal(got[1], a2.grad)
    assert torch.equal(got[2], T2.grad) and torch.equal(got[3], b2.grad)


def test_larger_block_against_float64_on_a_subset():
    """4096 local rows (row_offset 4096) against 16384 columns, d = 768 (several row blocks per split, two column launches per
    role).  float64 on a fixed subset: the loss rows and da of 64 rows (every column enters them), db of 64 columns (every local
    row enters them), half of them positives' columns.  Measured on the MI355X: loss rows 1.9e-6, da 1.8e-3, db 1.8e-3."""
    rows, cols, d, off = 4096, 16384, 768, 4096
    za, zb = _views(cols, d, seed=5)
    na, nb = _normed(za, zb)
    del za, zb
    a = na[off:off + rows].contiguous()
    T, bs = _scalars(0.1, -10.0)
    got = _stream_call(a, nb, off, T, bs)
    g = torch.Generator().manual_seed(1)
    ri = torch.randperm(rows, generator=g)[:64].sort().values.to(DEV)
    ci = torch.cat([off + ri[:32], torch.randperm(cols, generator=g)[:32].to(DEV)])
    a64, b64 = a.double(), nb.double()

    def g_of(l, r_idx, c_idx):                      # coef / Tc * (sigmoid(l) - [positive]) for rows r_idx x columns c_idx
        pos = (off + r_idx)[:, None] == c_idx[None, :]
        return (torch.sigmoid(l) - pos.double()) / cols / 0.1, pos

    l_r = a64[ri] @ b64.T / 0.1 - 10.0                                 # [64, cols]
    w_r, pos_r = g_of(l_r, ri, torch.arange(cols, device=DEV))
    want_rows = torch.nn.functional.softplus(torch.where(pos_r, -l_r, l_r)).sum(1)
    want_da = w_r @ b64
    l_c = a64 @ b64[ci].T / 0.1 - 10.0                                 # [rows, 64]
    w_c, _ = g_of(l_c, torch.arange(rows, device=DEV), ci)
    want_db = w_c.T @ a64
    errs = dict(rows=rel_err(got["rows"][ri], want_rows), da=rel_err(got["da"][ri], want_da), db=rel_err(got["db"][ci], want_db))
    print("sigmoid stream larger block: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    record_errors("sigmoid_stream_block", **errs)
    assert all(bool(torch.isfinite(x).all()) for x in got["raw"])
    assert errs["rows"] < LOSS_ROWS and errs["da"] < ROW_GRAD and errs["db"] < ROW_GRAD
