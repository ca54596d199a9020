"""The calibration statistics and the scaling fit on the device against the restatement and bounds of
tests/calibration_cases.py: every case and logits dtype through the C ABI and through multilabel_calibration (integer statistics
equal, float statistics and closing values inside the derived bounds, bit-equal repeats, garbage under unknown targets and in
place of NaN logits changing no bit), the label dtypes, the forms of scale and bias, the error paths, the fit's conditions
(a) - (e), captures replayed with new inputs, two ranks over one process group, and the trainer's flags."""
import datetime
import math
import os
import socket
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from aecf_amd import _lib
from tests import calibration_cases as K

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda:0")
TORCH_DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
ABI_DTYPES = {"float32": _lib.AECF_F32, "bfloat16": _lib.AECF_BF16, "float16": _lib.AECF_F16}
WORST = {}                                                          # the largest error / bound seen, by group of tests


def _note(group, ratio):
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    print(f"calibration {group}: error / bound {ratio:.3g} (largest so far {WORST[group]:.3g})")


def _logits(x, dtype, dev=DEV):
    t = torch.from_numpy(x.copy()).to(TORCH_DTYPES[dtype])
    assert np.array_equal(t.float().numpy(), x, equal_nan=True)                # the case's values exist in its dtype
    return t.to(dev)


def _vec(v, dev=DEV):
    return None if v is None else torch.from_numpy(v.copy()).to(dev)


def _capi(c, dtype):
    """aecf_mlcal_stats with poisoned outputs and workspace: the float64 block [3 B + 5, C] as numpy"""
    import ctypes
    from aecf_amd.layer import _ptr, _stream
    lib = _lib.load()
    x, y = _logits(c.x, dtype), torch.from_numpy(c.t.copy()).to(DEV)
    n, C = x.shape
    wsb = lib.aecf_mlcal_workspace_bytes(n, C, c.B)
    assert wsb == K.workspace_layout(n, C, c.B)
    ws = torch.full((wsb,), 0xA5, dtype=torch.uint8, device=DEV)
    stats = torch.full((3 * c.B + 5, C), float("nan"), dtype=torch.float64, device=DEV)
    e = K.edges(c.B)
    edges = (ctypes.c_float * max(e.size, 1))(*e.tolist())
    sc, bi = _vec(c.scale), _vec(c.bias)
    _lib.check(lib.aecf_mlcal_stats(n, C, ABI_DTYPES[dtype], _lib.AECF_F32, _ptr(x), _ptr(y), _ptr(sc), _ptr(bi), c.B, edges,
                                    _ptr(stats), _ptr(ws), wsb, _stream()), "aecf_mlcal_stats")
    torch.cuda.synchronize()
    return stats.cpu().numpy()


def _block_as_dict(block, B):
    i = lambda v: v.astype(np.int64)
    assert np.array_equal(block[:2 * B], np.round(block[:2 * B])) and np.array_equal(block[3 * B + 2:], np.round(block[3 * B + 2:]))
    return dict(bin_count=i(block[:B].T), bin_pos=i(block[B:2 * B].T), bin_conf=block[2 * B:3 * B].T, brier_sum=block[3 * B],
                nll_sum=block[3 * B + 1], n_invalid=i(block[3 * B + 2]), n_valid=i(block[3 * B + 3]), n_pos=i(block[3 * B + 4]))


def _python(c, dtype, labels=None, dev=DEV, rows=None, **kw):
    from aecf_amd import metrics
    x = _logits(c.x, dtype, dev)
    y = torch.from_numpy(c.t.copy()).to(dev) if labels is None else labels
    if rows is not None:
        x, y = x[rows[0]:rows[1]].clone(), y[rows[0]:rows[1]].clone()
    kw.setdefault("scale", _vec(c.scale, dev))
    kw.setdefault("bias", _vec(c.bias, dev))
    m = metrics.multilabel_calibration(x, y, n_bins=c.B, **kw)
    C = c.x.shape[1]
    assert m["bin_count"].shape == (C, c.B) and m["bin_count"].dtype == torch.int64 and m["bin_conf"].dtype == torch.float64
    assert m["ece"].dim() == 0 and m["ece_per_class"].shape == (C,) and m["n_valid"].dtype == torch.int64
    assert all(v.device == x.device for v in m.values())
    return {k: v.cpu().numpy() for k, v in m.items()}


@pytest.mark.parametrize("dtype", K.DTYPES)
@pytest.mark.parametrize("name", K.CASE_IDS)
def test_case_through_the_c_abi_and_python(name, dtype):
    """integer statistics EQUAL the restatement's, float statistics and closing values inside the bounds, infinities and NaN
    where the restatement has them; a second run and a run with other garbage where nothing may be read give the same bits"""
    c = K.case(name, dtype)
    ref = K.reference(c)
    block = _capi(c, dtype)
    _note("statistics", K.check_stats(_block_as_dict(block, c.B), ref, f"{name} {dtype} C ABI"))
    assert block.tobytes() == _capi(c, dtype).tobytes(), "two runs differ"
    assert block.tobytes() == _capi(K.garbage(c), dtype).tobytes(), "an unknown target's logit or a NaN logit reached an output"
    got = _python(c, dtype)
    _note("closing values", K.check_stats(got, ref, f"{name} {dtype} multilabel_calibration"))
    assert np.array_equal(got["bin_conf"], _block_as_dict(block, c.B)["bin_conf"])


@pytest.mark.parametrize("name", ("255x15_b15", "64x80_b15", "257x1_b32"))
def test_no_scaling_against_the_identity_scaling(name):
    """scale=None, bias=None and scale=1, bias=0 take different paths (no multiply against a multiply by 1): both inside the
    bounds of the same reference, their integers equal"""
    c = K.case(name)._replace(scale=None, bias=None)
    ref = K.reference(c)
    C = c.x.shape[1]
    plain = _python(c, "float32")
    for form in (dict(scale=1.0, bias=0.0), dict(scale=1, bias=None), dict(scale=None, bias=torch.zeros(C, device=DEV)),
                 dict(scale=torch.ones(C, device=DEV, dtype=torch.float64), bias=0.0)):
        got = _python(c, "float32", **form)
        _note("identity scaling", K.check_stats(got, ref, f"{name} {form}"))
        assert np.array_equal(got["bin_count"], plain["bin_count"])
    K.check_stats(plain, ref, name)


@pytest.mark.parametrize("label_dtype", ("int8", "uint8", "bool", "bfloat16", "float16"))
def test_label_dtypes(label_dtype):
    c = K.case("255x15_b15")
    kn = K.known(c.t)
    if label_dtype == "int8":
        y = torch.from_numpy(np.where(kn, c.t * 3, -2).astype(np.int8)).to(DEV)          # a positive is any non-zero value
    elif label_dtype in ("uint8", "bool"):                          # no unknown value: the unknown targets become negatives
        c = c._replace(t=np.where(kn, c.t, np.float32(0.0)).astype(np.float32))
        y = torch.from_numpy(c.t.copy()).to(DEV).to(torch.uint8 if label_dtype == "uint8" else torch.bool)
    else:
        y = torch.from_numpy(c.t.copy()).to(DEV).to(TORCH_DTYPES[label_dtype])
    K.check_stats(_python(c, "float32", labels=y), K.reference(c), f"labels {label_dtype}")


def test_error_paths():
    from aecf_amd import metrics
    x, y = torch.zeros(4, 3, device=DEV), torch.zeros(4, 3, device=DEV)
    for fn in (metrics.multilabel_calibration, metrics.fit_calibration):
        with pytest.raises(ValueError, match="one shape"):
            fn(x, y[:-1])
        with pytest.raises(TypeError, match="float32, bfloat16 or float16 logits"):
            fn(x.double(), y)
        with pytest.raises(TypeError, match="labels, got torch.int64"):
            fn(x, y.long())
        with pytest.raises(NotImplementedError, match="C <= 4096"):
            fn(torch.zeros(2, 4097, device=DEV), torch.zeros(2, 4097, device=DEV))
        with pytest.raises(RuntimeError, match="must be on a ROCm device"):
            fn(x.cpu(), y.cpu())
    for bad in (0, 33, 2.0, True):
        with pytest.raises(ValueError, match=r"n_bins in 1 \.\. 32"):
            metrics.multilabel_calibration(x, y, n_bins=bad)
    with pytest.raises(ValueError, match=r"scale must hold one value per class, \[3\]"):
        metrics.multilabel_calibration(x, y, scale=torch.ones(4, device=DEV))
    with pytest.raises(TypeError, match="bias must be None, a Python number or a"):
        metrics.multilabel_calibration(x, y, bias="0")
    with pytest.raises(ValueError, match="'temperature', 'class_temperature' or 'platt'"):
        metrics.fit_calibration(x, y, mode="vector")
    with pytest.raises(ValueError, match="max_iter >= 1"):
        metrics.fit_calibration(x, y, max_iter=0)
    lib = _lib.load()
    assert lib.aecf_mlcal_workspace_bytes(1 << 20, 4096, 15) == 0 and lib.aecf_mlcal_workspace_bytes(4, 3, 0) == 0
    assert lib.aecf_mlcal_fit_update(3, 3, None, None, None, None, None, None, None) == -1
    assert lib.aecf_mlcal_fit_update(3, 0, None, None, None, None, None, None, None) == -3


# ---------------------------------------------------------------------------------------------- the fit

def _fit(c, dtype, mode, dev=DEV, rows=None, **kw):
    from aecf_amd import metrics
    x, y = _logits(c.x, dtype, dev), torch.from_numpy(c.t.copy()).to(dev)
    if rows is not None:
        x, y = x[rows[0]:rows[1]].clone(), y[rows[0]:rows[1]].clone()
    r = metrics.fit_calibration(x, y, mode=mode, **kw)
    C, P = c.x.shape[1], (1 if mode == "temperature" else c.x.shape[1])
    assert r["scale"].shape == (C,) and r["scale"].dtype == torch.float32 and r["bias"].shape == (C,)
    assert r["fitted"].shape == (P,) and r["fitted"].dtype == torch.bool and r["nll_after"].shape == (P,)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _per_problem(r, mode):
    """scale and bias of every problem: one for the shared temperature (the same value in every class), else per class"""
    if mode == "temperature":
        assert (r["scale"] == r["scale"][0]).all() and (r["bias"] == 0).all()
        return dict(r, scale=r["scale"][:1], bias=r["bias"][:1])
    return r


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", K.FIT_CASE_IDS)
def test_fit_meets_its_conditions(name, mode):
    """(a) the float64 gradient at the returned parameters inside eps_g + tau, (b) the parameters inside the bound around the
    float64 optimum, (c) the NLL not above the first, (d) degenerate classes untouched or inside the box, (e) converged"""
    c = K.fit_case(name)
    r = _fit(c, "float32", mode)
    _note("fit", K.check_fit(c, mode, _per_problem(r, mode), f"{name} {mode}"))
    use = K.used(c)
    assert np.array_equal(r["n_used"], use.sum(0)) and np.array_equal(r["n_skipped"], (K.known(c.t) & np.isinf(c.x)).sum(0))
    again = _fit(c, "float32", mode)
    assert all(np.array_equal(r[k], again[k], equal_nan=True) for k in r), "two fits differ"
    # what is fitted is what the statistics apply: the NLL of the fitted scaling, pooled over the used elements
    sc = K.Case(np.where(np.isfinite(c.x), c.x, np.float32(np.nan)), c.t, 15, r["scale"], r["bias"])
    m = _python(sc, "float32")
    K.check_close(m["nll"] * m["n_valid"].sum(), r["nll_after"].sum(), 2.0 ** -13 * r["nll_after"].sum(), "the statistics' NLL")


@pytest.mark.parametrize("dtype", ("bfloat16", "float16"))
def test_fit_on_16_bit_logits(dtype):
    c = K.fit_case("fit_2049x17", dtype)
    for mode in ("temperature", "platt"):
        _note("fit", K.check_fit(c, mode, _per_problem(_fit(c, dtype, mode), mode), f"fit_2049x17 {dtype} {mode}"))


# ---------------------------------------------------------------------------------------------- captures

def test_captured_statistics_and_fit_replay_with_new_inputs():
    """no host read: one call of each captures, and the replays follow logits and labels changed in place"""
    from aecf_amd import metrics
    first = K.fit_case("fit_257x5")
    sets = [first, first._replace(x=np.ascontiguousarray(first.x[::-1, ::-1]), t=np.ascontiguousarray(first.t[::-1, ::-1]))]
    x = torch.zeros(257, 5, device=DEV)
    y = torch.zeros(257, 5, device=DEV)
    scale = torch.ones(5, device=DEV)
    metrics.multilabel_calibration(x, y, scale=scale, bias=0.25)    # warm-up outside the capture
    metrics.fit_calibration(x, y, mode="platt", max_iter=2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m = metrics.multilabel_calibration(x, y, scale=scale, bias=0.25)
        f = metrics.fit_calibration(x, y, mode="platt")
    seen = []
    for i, c in enumerate(sets):
        with torch.no_grad():
            x.copy_(torch.from_numpy(c.x.copy()))
            y.copy_(torch.from_numpy(c.t.copy()))
        graph.replay()
        torch.cuda.synchronize()
        sc = K.Case(c.x, c.t, 15, np.ones(5, dtype=np.float32), np.full(5, 0.25, dtype=np.float32))
        K.check_stats({k: v.cpu().numpy() for k, v in m.items()}, K.reference(sc), f"replay {i}")
        K.check_fit(c, "platt", {k: v.cpu().numpy() for k, v in f.items()}, f"replay {i}")
        seen.append(f["scale"].cpu().numpy().copy())
    # the second set is the first with rows and classes reversed: the replay followed it
    assert np.allclose(seen[0], seen[1][::-1], rtol=1e-4) and not np.allclose(seen[0], seen[1], rtol=1e-2)


# ---------------------------------------------------------------------------------------------- two ranks

CUT = 700                                                           # rank 0 holds rows [0, 700), rank 1 the other 1349
SPLITS = ("uneven", "empty")
TWO_RANK_STATS = "2049x17_b15"
TWO_RANK_FIT = "fit_2049x17"


def _rows(split, rank, n):
    if split == "empty":
        return (0, n) if rank == 0 else (n, n)
    return (0, CUT) if rank == 0 else (CUT, n)


def _two_ranks_worker(rank, world, port, backend, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    limit = datetime.timedelta(seconds=90)          # a collective without its partner raises here instead of hanging
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=limit)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=limit)
    done, error = {}, None
    try:
        for split in SPLITS:
            c, fc = K.case(TWO_RANK_STATS), K.fit_case(TWO_RANK_FIT)
            n = c.x.shape[0]
            done[split] = dict(stats=_python(c, "float32", dev=dev, rows=_rows(split, rank, n), group=dist.group.WORLD),
                               fit={mode: _fit(fc, "float32", mode, dev=dev, rows=_rows(split, rank, n), group=dist.group.WORLD)
                                    for mode in ("temperature", "platt")})
    except Exception:
        error = f"rank {rank}:\n{traceback.format_exc()}"
    finally:
        q.put((rank, done, error))
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks():
    world = 2
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_two_ranks_worker, args=(r, world, port, backend, q)) for r in range(world)]
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


@pytest.mark.parametrize("split", SPLITS)
def test_two_ranks_equal_one_rank(two_ranks, split):
    """uneven shards and an empty shard: both ranks hold the same bits; the integer statistics equal the one-rank call's, the
    float ones lie inside the bounds with the ranks' sums added; the fitted parameters meet the fit's conditions"""
    c, fc = K.case(TWO_RANK_STATS), K.fit_case(TWO_RANK_FIT)
    r0, r1 = (r[split] for r in two_ranks)
    for k in r0["stats"]:
        assert np.array_equal(r0["stats"][k], r1["stats"][k], equal_nan=True), k
    one = _python(c, "float32")
    for k in ("bin_count", "bin_pos", "n_valid", "n_pos", "n_invalid"):
        assert np.array_equal(r0["stats"][k], one[k]), k
    _note("two ranks", K.check_stats(r0["stats"], K.reference(c, world=2), f"two ranks, {split} shards"))
    for mode in ("temperature", "platt"):
        for k in r0["fit"][mode]:
            assert np.array_equal(r0["fit"][mode][k], r1["fit"][mode][k], equal_nan=True), (mode, k)
        _note("two ranks", K.check_fit(fc, mode, _per_problem(r0["fit"][mode], mode), f"two ranks {split} {mode}", world=2))


# ---------------------------------------------------------------------------------------------- the trainer

def test_trainer_with_the_calibration_flags():
    """train_xray.main --calibration --calibrate temperature for two tiny epochs: the three plans' ECE, Brier and NLL in every
    row, and a last row with the fit -- whose NLL with all modalities present is not above the uncalibrated one.  Without the
    flags the rows carry the usual keys only."""
    from aecf_amd import train_xray
    argv = ["--epochs", "2", "--switch-epoch", "1", "--samples", "320", "--val-samples", "128", "--batch", "64", "--classes", "5"]
    history = train_xray.main(argv + ["--calibration", "--calibrate", "temperature"])
    assert len(history) == 3
    plans = ("", "_no_images", "_no_texts")
    for row in history[:2]:
        for s in plans:
            assert 0.0 <= row["val_ece" + s] <= 1.0 and 0.0 <= row["val_brier" + s] <= 1.0 and row["val_nll" + s] > 0
    last = history[2]
    assert last["calibrate"] == "temperature" and len(last["temperature"]) == 5 and last["fitted"] == [True]
    assert 1.0 / 64 <= last["temperature"][0] <= 64.0 and last["val_nll_calibrated"] <= last["val_nll"] * (1 + 1e-6)
    assert all(math.isfinite(last[k + t + s]) for k in ("val_ece", "val_nll") for t in ("", "_calibrated") for s in plans)
    assert abs(last["val_ece"] - history[1]["val_ece"]) <= 1e-12
    plain = train_xray.main(argv)
    keys = {"epoch", "curriculum", "train_loss", "gate_entropy", "sec", "val_map", "val_map_no_images", "val_map_no_texts"}
    assert len(plain) == 2 and all(set(row) == keys for row in plain)
    assert [r["val_map"] for r in plain] == [r["val_map"] for r in history[:2]]
