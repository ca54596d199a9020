"""The multi-label bootstrap on the device against the numpy restatement of tests/bootstrap_cases.py: every case through the C
ABI (order entries, drawn weights and the six integer statistics EQUAL, S and the scores inside the derived bounds), replicate
0 against multilabel_metrics, caller-supplied weights with 0 and 255 and clipped wider counts, NaN payloads and repeats that
move no bit, the percentile limits against numpy.nanpercentile, replicate chunks, a captured call replayed with new inputs, the
paired comparison, two ranks over one process group with uneven and with empty shards, and the trainer's --bootstrap."""
import datetime
import os
import socket
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from aecf_amd import _lib
from tests import bootstrap_cases as B
from tests import metrics_cases as M

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda:0")
TORCH_DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
ABI_DTYPES = {"float32": _lib.AECF_F32, "bfloat16": _lib.AECF_BF16, "float16": _lib.AECF_F16}
POISON_ENTRY = 0x60000000           # an order entry nobody wrote: row 0, pos and pred set -- consumed, it would move the counts


def _device_case(name, dev=DEV):
    s, y, dtype, R, seed, thr = B.case(name)
    x = torch.from_numpy(s.copy()).to(TORCH_DTYPES[dtype])
    assert np.array_equal(x.float().numpy(), s, equal_nan=True)            # the case's values exist in its dtype
    return x.to(dev), torch.from_numpy(y.copy()).to(dev), dtype, R, seed, torch.from_numpy(thr.copy()).to(dev)


def _numpy(result):
    return {k: v.detach().cpu().numpy() for k, v in result.items() if isinstance(v, torch.Tensor)}


def _capi(x, y, dtype, thr, R, seed, replicate0=0, counts=None):
    """order, draw (or pack ``counts`` int32 [n, Rp]) and walk with poisoned outputs: class_counts [3, C], order [C, Np], weights
    [n, Rp], stats int64 [R, 7, C] and n_saturated as numpy"""
    from aecf_amd.layer import _ptr, _stream
    lib = _lib.load()
    n, C = x.shape
    Np, Rp = (n + 63) // 64 * 64, (R + 63) // 64 * 64
    y8 = y.to(torch.uint8).contiguous()
    wsb, dwsb = lib.aecf_mlboot_workspace_bytes(n, C), lib.aecf_mlboot_draw_workspace_bytes(n, R)
    assert wsb > 0 and dwsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    dws = torch.full((dwsb,), 0x55, dtype=torch.uint8, device=x.device)    # the draw zeroes its scratch itself
    cc = torch.full((3, C), -7, dtype=torch.int32, device=x.device)
    order = torch.full((C, Np), POISON_ENTRY, dtype=torch.int32, device=x.device)
    w = torch.full((n, Rp), 0xee, dtype=torch.uint8, device=x.device)
    sat = torch.zeros(1, dtype=torch.int32, device=x.device)
    stats = torch.full((R, 7, C), -7, dtype=torch.int64, device=x.device)
    st = _stream()
    _lib.check(lib.aecf_mlboot_order(n, C, ABI_DTYPES[dtype], _ptr(x), _ptr(y8), _ptr(thr), _ptr(cc), _ptr(order), _ptr(ws), wsb, st),
               "aecf_mlboot_order")
    if counts is None:
        _lib.check(lib.aecf_mlboot_draw(n, R, replicate0, seed, None, _ptr(w), _ptr(sat), _ptr(dws), dwsb, st), "aecf_mlboot_draw")
    else:
        _lib.check(lib.aecf_mlboot_draw(n, R, replicate0, seed, _ptr(counts), _ptr(w), _ptr(sat), None, 0, st), "aecf_mlboot_draw")
    _lib.check(lib.aecf_mlboot_walk(n, C, R, _ptr(cc), _ptr(order), _ptr(w), _ptr(stats), st), "aecf_mlboot_walk")
    torch.cuda.synchronize()
    return cc.cpu().numpy(), order.cpu().numpy(), w.cpu().numpy(), stats.cpu().numpy(), int(sat.item())


def _check_stats(stats, ref, what):
    """the six integers equal; S within s_bound(G) of the restatement's, relative to S (both are at most Wpos)"""
    for k, name in enumerate(B.STAT_NAMES):
        assert np.array_equal(stats[:, k], ref["stats"][name]), (what, name)
    s = stats[:, 6].copy().view(np.float64)
    bound = np.array([B.s_bound(int(g)) for g in ref["groups"]]) * ref["stats"]["s"]
    err = np.abs(s - ref["stats"]["s"])
    assert not err[bound == 0].any(), what                      # S = 0: no positive weight, an exact zero on both sides
    ratio = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"bootstrap {what}: S error / bound {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)


def _check_scores(got, ref, C, what):
    ratios = B.compare_scores(got, ref["scores"], ref["groups"], C)
    print(f"bootstrap {what}: error / bound " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)


def _check_order(order, ref_order, what):
    for c, e in enumerate(ref_order):
        assert np.array_equal(order[c, :len(e)].view(np.uint32), e), (what, c)
        assert (order[c, len(e):] == POISON_ENTRY).all(), (what, c)        # slots past nvalid are not written


@pytest.mark.parametrize("name", B.CASE_IDS)
def test_case_through_the_c_abi(name):
    """the order array is numpy's stable descending argsort with the flags; the drawn weights are the restatement's, their
    replicates sum to n_all, replicate 0 is ones and the padding columns are zero; the six integer statistics are equal, S and
    the closed scores inside the bounds"""
    from aecf_amd import metrics
    x, y, dtype, R, seed, thr = _device_case(name)
    n, C = x.shape
    ref = B.restated(name)
    cc, order, w, stats, sat = _capi(x, y, dtype, thr, R, seed)
    _check_order(order, ref["order"], name)
    assert np.array_equal(cc[1], [len(e) for e in ref["order"]])
    assert np.array_equal(w[:, :R].T, ref["weights"]) and not w[:, R:].any() and sat == 0
    assert np.array_equal(w[:, :R].astype(np.int64).sum(0), np.full(R, n)) and (w[:, 0] == 1).all()
    _check_stats(stats, ref, f"case {name} ({n} x {C} {dtype}, {R} replicates)")
    got = _numpy(metrics._close_replicates(torch.from_numpy(stats).to(DEV)))
    _check_scores(got, ref, C, f"case {name}")


def test_replicate_offset_and_repeats_are_bit_equal():
    """replicates 3 .. 66 drawn on their own are columns 3 .. 66 of the full draw, statistics included; the same call twice gives
    the same bits (integer atomics commute)"""
    x, y, dtype, R, seed, thr = _device_case("n257")
    _, order, w, stats, _ = _capi(x, y, dtype, thr, R, seed)
    _, order2, w2, stats2, _ = _capi(x, y, dtype, thr, R, seed)
    assert np.array_equal(order, order2) and np.array_equal(w, w2) and np.array_equal(stats, stats2)
    _, _, w3, stats3, _ = _capi(x, y, dtype, thr, 64, seed, replicate0=3)
    assert np.array_equal(w3[:, :64], w[:, 3:67]) and np.array_equal(stats3, stats[3:67])


def test_replicate_zero_is_multilabel_metrics():
    """the point estimate against multilabel_metrics on the same inputs: counts equal, AP within the sum of both bounds, AUROC
    and F1 within theirs -- the specials and the degenerate classes included"""
    from aecf_amd import metrics
    for name in ("specials", "quantised", "n1025"):
        x, y, _, _, seed, _ = _device_case(name)
        n, C = x.shape
        ref = B.restated(name)
        one = _numpy(metrics.multilabel_metrics(x, y))
        out = metrics.bootstrap_metrics(x, y, n_boot=3, seed=seed, return_replicates=True)
        got = _numpy(out)
        b_ap = M.ap_bound(n) + np.array([B.ap_bound(int(g)) for g in ref["groups"]])
        assert np.array_equal(np.isnan(got["auroc"]), np.isnan(one["auroc"]))
        assert (np.abs(got["ap"] - one["ap"]) <= b_ap).all()
        assert np.nanmax(np.abs(got["auroc"] - one["auroc"]), initial=0.0) <= M.AUROC_BOUND + B.AUROC_BOUND
        assert np.abs(got["f1"] - one["f1"]).max() <= M.F1_BOUND + B.F1_BOUND
        assert abs(got["map"] - one["map"]) <= B.macro_bound(float(b_ap.max()), C)
        assert abs(got["macro_f1"] - one["macro_f1"]) <= B.macro_bound(M.F1_BOUND + B.F1_BOUND, C)
        assert np.array_equal(out["replicates"]["ap"][0].cpu().numpy(), got["ap"])


def test_caller_weights_with_0_and_255_and_clipped_counts():
    """uint8 weights holding 0 and 255 (a replicate that loses positives, one at the uint8 limit) against the restatement, with
    replicate 0 still the point estimate; int32 counts beyond 0 .. 255 are clipped and counted in n_saturated"""
    from aecf_amd import metrics
    x, y, dtype, _, seed, thr = _device_case("n257")
    s, yy, *_ = B.case("n257")
    n, C = x.shape
    w = B.caller_weights(n, 66, seed)
    full = np.concatenate([np.ones((1, n), dtype=np.uint8), w])
    ref = B.restate(s, yy, full, thr.cpu().numpy())
    out = metrics.bootstrap_metrics(x, y, threshold=thr, weights=torch.from_numpy(w).to(DEV), return_replicates=True, return_weights=True)
    assert np.array_equal(out["weights"].cpu().numpy(), full) and int(out["n_saturated"]) == 0
    _check_scores(_numpy(out["replicates"]), ref, C, "caller weights")
    wide = w.astype(np.int32)
    wide[5, :7], wide[6, 3] = 300, -2
    out2 = metrics.bootstrap_metrics(x, y, threshold=thr, weights=torch.from_numpy(wide).to(DEV), return_replicates=True, return_weights=True)
    clipped = np.concatenate([np.ones((1, n), dtype=np.int32), np.clip(wide, 0, 255)])
    assert np.array_equal(out2["weights"].cpu().numpy(), clipped) and int(out2["n_saturated"]) == 8
    _check_scores(_numpy(out2["replicates"]), B.restate(s, yy, clipped, thr.cpu().numpy()), C, "clipped counts")


def test_nan_payloads_move_no_bit():
    """other NaN bit patterns (sign, payload) in place of the specials' NaNs: order, weights and statistics keep every bit"""
    x, y, dtype, R, seed, thr = _device_case("specials")
    base = _capi(x, y, dtype, thr, R, seed)
    bits = x.view(torch.int32).clone()
    nan = torch.isnan(x)
    garbage = torch.randint(1, 1 << 22, x.shape, generator=torch.Generator().manual_seed(5), dtype=torch.int32).to(DEV)
    bits[nan] = (bits[nan] & -0x00400000) ^ garbage[nan] ^ (garbage[nan] << 31)
    x2 = bits.view(torch.float32)
    assert torch.isnan(x2).eq(nan).all() and not torch.equal(bits, x.view(torch.int32))
    other = _capi(x2, y, dtype, thr, R, seed)
    for a, b in zip(base, other):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["n257", "specials"])
def test_python_surface_and_percentile_limits(name):
    """keys, shapes and dtypes; the replicates against the restatement; <name>_ci against numpy.nanpercentile of the RESTATED
    replicates 1 .. R within ci_bound; n_defined; a per-class threshold tensor; replicate chunks give the bits of one chunk"""
    from aecf_amd import metrics
    x, y, _, R, seed, thr = _device_case(name)
    n, C = x.shape
    ref = B.restated(name)
    conf = 0.9
    out = metrics.bootstrap_metrics(x, y, n_boot=R - 1, confidence=conf, threshold=thr, seed=seed, return_replicates=True,
                                    return_weights=True)
    assert set(out) == {f"{k}{s}" for k in B.SCORES for s in ("", "_ci", "_se")} | {"n_defined", "n_saturated", "replicates", "weights"}
    assert np.array_equal(out["weights"].cpu().numpy(), ref["weights"]) and out["weights"].dtype == torch.uint8
    reps = _numpy(out["replicates"])
    _check_scores(reps, ref, C, f"python surface {name}")
    bounds = B.score_bounds(ref["groups"], C)
    for k in B.SCORES:
        shape = (C,) if k in ("ap", "auroc", "f1") else ()
        assert out[k].shape == shape and out[k + "_ci"].shape == (2,) + shape and out[k + "_se"].shape == shape
        assert out[k].dtype == torch.float64 and out[k].device == x.device
        assert np.array_equal(out[k].cpu().numpy(), reps[k][0], equal_nan=True)
        rr = ref["scores"][k][1:]
        defined = (~np.isnan(rr)).sum(0)
        assert np.array_equal(out["n_defined"][k].cpu().numpy(), defined)
        want, got = B.percentile_limits(rr, conf), out[k + "_ci"].cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)), k
        err = np.where(np.isnan(want), 0.0, np.abs(got - want))
        assert (err <= B.ci_bound(np.max(bounds[k]), R - 1)).all(), (k, err.max())
        with np.errstate(invalid="ignore"):
            se = np.where(defined > 1, np.nanstd(np.where(defined > 1, rr, 0.0), axis=0, ddof=1), np.nan)
        assert np.allclose(out[k + "_se"].cpu().numpy(), se, rtol=1e-9, atol=1e-15, equal_nan=True), k
    # 129 replicates in chunks of 64: the same bits
    old = metrics._BOOT_CHUNK_ELEMS
    try:
        metrics._BOOT_CHUNK_ELEMS = 64 * n
        assert metrics._boot_chunk(n) == 64
        chunked = metrics.bootstrap_metrics(x, y, n_boot=R - 1, confidence=conf, threshold=thr, seed=seed, return_replicates=True,
                                            return_weights=True)
    finally:
        metrics._BOOT_CHUNK_ELEMS = old
    assert torch.equal(chunked["weights"], out["weights"])
    for k in B.SCORES:
        assert np.array_equal(_numpy(chunked["replicates"])[k], reps[k], equal_nan=True)
        assert np.array_equal(chunked[k + "_ci"].cpu().numpy(), out[k + "_ci"].cpu().numpy(), equal_nan=True)


def test_python_refusals_and_label_kinds():
    from aecf_amd import metrics
    x, y, _, _, seed, _ = _device_case("n63")
    a = metrics.bootstrap_metrics(x, y, n_boot=5, seed=seed)
    b = metrics.bootstrap_metrics(x, y.float() * 0.25, n_boot=5, seed=seed)
    assert all(torch.equal(a[k + "_ci"], b[k + "_ci"]) for k in ("ap", "map", "macro_f1"))
    with pytest.raises(ValueError, match="threshold"):
        metrics.bootstrap_metrics(x, y, threshold=1.0)
    with pytest.raises(ValueError, match="threshold"):
        metrics.bootstrap_metrics(x, y, threshold=torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match="n_boot"):
        metrics.bootstrap_metrics(x, y, n_boot=0)
    with pytest.raises(ValueError, match="one shape"):
        metrics.bootstrap_metrics(x, y[:-1])
    with pytest.raises(TypeError, match="logits"):
        metrics.bootstrap_metrics(x.double(), y)
    with pytest.raises(ValueError, match="weights"):
        metrics.bootstrap_metrics(x, y, weights=torch.ones(4, 5, dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError, match="weights"):
        metrics.bootstrap_metrics(x, y, weights=torch.ones(4, 63, device=DEV))


def test_paired_comparison():
    """a model against itself differs by exactly zero in every replicate; two models: the difference's point, limits and the
    shares at or below / above zero are those of the restated replicate differences"""
    from aecf_amd import metrics
    x, y, _, R, seed, thr = _device_case("n257")
    s, yy, *_ = B.case("n257")
    n, C = x.shape
    same = metrics.bootstrap_compare(x, x, y, n_boot=R - 1, seed=seed, threshold=thr, return_replicates=True)
    for k in B.SCORES:
        d = same["replicates"][k]
        assert not torch.nan_to_num(d).any() and not torch.nan_to_num(same[k + "_ci"]).any()
    s_b = np.roll(s, 1, axis=0).copy()
    x_b = torch.from_numpy(s_b).to(DEV)
    ref_a, ref_b = B.restated("n257"), B.restate(s_b, yy, B.restated("n257")["weights"], thr.cpu().numpy())
    out = metrics.bootstrap_compare(x, x_b, y, n_boot=R - 1, seed=seed, threshold=thr, confidence=0.9)
    bounds_a, bounds_b = B.score_bounds(ref_a["groups"], C), B.score_bounds(ref_b["groups"], C)
    for k in B.SCORES:
        d = ref_a["scores"][k] - ref_b["scores"][k]
        b = np.max(bounds_a[k]) + np.max(bounds_b[k])
        got = out[k].cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(d[0])) and np.nanmax(np.abs(got - d[0]), initial=0.0) <= b, k
        want = B.percentile_limits(d[1:], 0.9)
        ci = out[k + "_ci"].cpu().numpy()
        assert np.array_equal(np.isnan(ci), np.isnan(want)) and np.nanmax(np.abs(ci - want), initial=0.0) <= B.ci_bound(b, R - 1), k
    # the shares on the macro F1 difference, whose replicates are far from zero compared with the bound, or exactly zero
    d = (ref_a["scores"]["macro_f1"] - ref_b["scores"]["macro_f1"])[1:]
    assert (np.abs(d[d != 0]) > 1e-9).all()
    assert abs(float(out["macro_f1_p_le0"]) - (d <= 0).mean()) <= 1e-15 and abs(float(out["macro_f1_p_ge0"]) - (d >= 0).mean()) <= 1e-15


def test_captured_call_replays_with_new_inputs():
    """one rank reads nothing on the host: the call captures, and three replays with logits and labels changed in place give the
    three restatements"""
    from aecf_amd import metrics
    s, y0, _, R, seed, thr = B.case("n257")
    sets = [(s, y0), (np.roll(s, 3, axis=0).copy(), y0), (s, ~y0)]
    n, C = s.shape
    x = torch.zeros(n, C, device=DEV)
    y = torch.zeros(n, C, dtype=torch.bool, device=DEV)
    t = torch.from_numpy(thr.copy()).to(DEV)
    kw = dict(n_boot=R - 1, threshold=t, seed=seed, confidence=0.9, return_replicates=True)
    metrics.bootstrap_metrics(x, y, **kw)                     # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = metrics.bootstrap_metrics(x, y, **kw)
    w = B.restated("n257")["weights"]
    for i, (si, yi) in enumerate(sets):
        x.copy_(torch.from_numpy(si.copy()))
        y.copy_(torch.from_numpy(yi.copy()))
        graph.replay()
        torch.cuda.synchronize()
        ref = B.restate(si, yi, w, thr)
        _check_scores(_numpy(out["replicates"]), ref, C, f"replay {i}")
        want = B.percentile_limits(ref["scores"]["map"][1:], 0.9)
        assert np.abs(out["map_ci"].cpu().numpy() - want).max() <= B.ci_bound(B.score_bounds(ref["groups"], C)["map"], R - 1)
        assert int(out["n_saturated"]) == 0


# ---------------------------------------------------------------------------------------------- two ranks

TWO_RANK_CASE = "n257"
SPLITS = {"uneven": None, "empty": (1.0, 0.0)}             # None: dp.shard_bounds (129 and 128 of 257 rows); rank 1 holds no row
FLAT = [k + s for k in B.SCORES for s in ("", "_ci", "_se")]


def _flat(out):
    got = {k: out[k].cpu().numpy() for k in FLAT}
    got.update({"rep_" + k: v.cpu().numpy() for k, v in out["replicates"].items()})
    got.update({"def_" + k: v.cpu().numpy() for k, v in out["n_defined"].items()})
    got["weights"] = out["weights"].cpu().numpy()
    return got


def _two_ranks_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from aecf_amd import dp, metrics
    dev = torch.device("cuda", 0)                   # both ranks on one GPU, joined over gloo
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=90))
    done, error = {}, None
    try:
        x, y, _, R, seed, thr = _device_case(TWO_RANK_CASE, dev)
        n = x.shape[0]
        for split, how in SPLITS.items():
            lo, hi = dp.shard_bounds(n, rank, world) if how is None else ((0, n) if rank == 0 else (n, n))
            out = metrics.bootstrap_metrics(x[lo:hi], y[lo:hi], n_boot=R - 1, threshold=thr, seed=seed, group=dist.group.WORLD,
                                            return_replicates=True, return_weights=True)
            done[split] = _flat(out)
            done[split]["rows"] = hi - lo
    except Exception:
        error = f"rank {rank}:\n{traceback.format_exc()}"
    finally:
        q.put((rank, done, error))
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks():
    world = 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_two_ranks_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = []
    try:
        got = sorted([q.get(timeout=240) for _ in range(world)], key=lambda r: r[0])
        for p in procs:
            p.join(60)
    finally:
        alive = [p for p in procs if p.is_alive()]
        for p in alive:
            p.kill()
        for p in alive:
            p.join(30)
    errors = [e for _, _, e in got if e is not None]
    assert not errors, "\n".join(errors)
    assert not alive and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return [done for _, done, _ in got]


@pytest.mark.parametrize("split", list(SPLITS))
def test_two_ranks_equal_one_rank(two_ranks, split):
    """each rank walks its slice of the replicates and one all-reduce joins them: both ranks hold the bits of the one-rank call --
    replicates, limits, standard errors and weights"""
    from aecf_amd import metrics
    x, y, _, R, seed, thr = _device_case(TWO_RANK_CASE)
    one = _flat(metrics.bootstrap_metrics(x, y, n_boot=R - 1, threshold=thr, seed=seed, return_replicates=True, return_weights=True))
    r0, r1 = (dict(r[split]) for r in two_ranks)
    assert r0.pop("rows") + r1.pop("rows") == x.shape[0]
    for k in one:
        assert np.array_equal(r0[k], one[k], equal_nan=True), k
        assert np.array_equal(r1[k], one[k], equal_nan=True), k


# ---------------------------------------------------------------------------------------------- the trainer

def test_trainer_bootstrap_flag():
    """train_xray.main --bootstrap for one tiny epoch: a last row with the three plans' values inside their intervals and the
    paired differences; without the flag no such row"""
    from aecf_amd import train_xray
    argv = ["--epochs", "1", "--switch-epoch", "1", "--samples", "128", "--val-samples", "130", "--batch", "64", "--classes", "5"]
    rows = train_xray.main(argv + ["--bootstrap", "40", "--bootstrap-seed", "3"])
    assert len(rows) == 2 and rows[1]["bootstrap"] == 40 and rows[1]["bootstrap_seed"] == 3
    row = rows[1]
    for short in ("map", "auroc", "macro_f1"):
        for sfx in ("", "_no_images", "_no_texts"):
            lo, hi = row[f"val_{short}{sfx}_ci"]
            assert 0.0 <= lo <= hi <= 1.0 and isinstance(row[f"val_{short}{sfx}"], float)
        for sfx in ("_no_images", "_no_texts"):
            lo, hi = row[f"val_{short}_minus{sfx}_ci"]
            assert -1.0 <= lo <= hi <= 1.0 and 0.0 <= row[f"val_{short}_minus{sfx}_p_le0"] <= 1.0
            assert abs(row[f"val_{short}_minus{sfx}"] - (row[f"val_{short}"] - row[f"val_{short}{sfx}"])) <= 1e-12
    assert abs(row["val_map"] - rows[0]["val_map"]) < 0.05          # (today's val_map breaks ties by position)
    assert len(train_xray.main(argv)) == 1
