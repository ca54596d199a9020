"""The multi-label evaluation on the device against the float64 restatement of tests/metrics_cases.py: every case through the
C ABI (counts and class numbers equal, float outputs inside the derived bounds), row shards that reproduce the one-shard count
arrays bit for bit, the Python surface with every label dtype, a captured call replayed with new inputs, two ranks over one
process group with uneven and with empty shards, and the trainer's --full-metrics."""
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
from tests import metrics_cases as M

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda:0")
TORCH_DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
ABI_DTYPES = {"float32": _lib.AECF_F32, "bfloat16": _lib.AECF_BF16, "float16": _lib.AECF_F16}
FLOATS = ("ap", "auroc", "f1", "map", "macro_auroc", "macro_f1")


def _device_case(name, dev=DEV):
    s, y, dtype = M.case(name)
    x = torch.from_numpy(s.copy()).to(TORCH_DTYPES[dtype])
    assert np.array_equal(x.float().numpy(), s, equal_nan=True)            # the case's values exist in its dtype
    return x.to(dev), torch.from_numpy(y.copy()).to(dev), dtype


def _numpy(result):
    return {k: v.detach().cpu().numpy() for k, v in result.items()}


def _capi(x, y, dtype, shards, threshold=0.5):
    """prepare once, then counts and finalize per row shard.  Returns (class_counts [3, C], [counts [4, C, rows] per shard],
    [shares [5, C] per shard]) as numpy; every output buffer is poisoned first: the calls write, they do not accumulate."""
    from aecf_amd.layer import _ptr, _stream
    lib = _lib.load()
    n, C = x.shape
    y8 = y.to(torch.uint8).contiguous()
    wsb = lib.aecf_mlmetrics_workspace_bytes(n, C)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    cc = torch.full((3, C), -7, dtype=torch.int32, device=x.device)
    _lib.check(lib.aecf_mlmetrics_prepare(n, C, ABI_DTYPES[dtype], _ptr(x), _ptr(y8), _ptr(cc), _ptr(ws), wsb, _stream()), "prepare")
    counts, shares = [], []
    thr = float(M.logit_threshold(threshold))
    for off, rows in shards:
        cn = torch.full((4, C, rows), -7, dtype=torch.int32, device=x.device)
        sh = torch.full((5, C), float("nan"), dtype=torch.float64, device=x.device)
        _lib.check(lib.aecf_mlmetrics_counts(n, C, off, rows, _ptr(cc), _ptr(cn) if rows else None, _ptr(ws), wsb, _stream()), "counts")
        _lib.check(lib.aecf_mlmetrics_finalize(n, C, off, rows, thr, _ptr(cc), _ptr(cn) if rows else None, _ptr(sh), _ptr(ws), wsb,
                                               _stream()), "finalize")
        counts.append(cn)
        shares.append(sh)
    torch.cuda.synchronize()
    return cc.cpu().numpy(), [c.cpu().numpy() for c in counts], [s.cpu().numpy() for s in shares]


def _check_floats(got, ref, n_all, classes, what, world=1):
    ratios = M.compare(got, ref, n_all, classes, world)
    print(f"metrics {what}: error / bound " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)


@pytest.mark.parametrize("name", M.CASE_IDS)
def test_case_through_the_c_abi(name):
    """one shard: the four count arrays, npos / nvalid / ninvalid and the integer shares equal the restatement's; the closing
    arithmetic of aecf_amd.metrics on the shares is inside the bounds"""
    from aecf_amd import metrics
    x, y, dtype = _device_case(name)
    n, C = x.shape
    ref = M.restated(name)
    cc, (cn,), (sh,) = _capi(x, y, dtype, [(0, n)])
    assert np.array_equal(cn, ref["counts"])
    assert np.array_equal(cc[0], ref["n_pos"]) and np.array_equal(cc[2], ref["n_invalid"]) and np.array_equal(cc[1], n - ref["n_invalid"])
    assert np.array_equal(sh[1:], ref["shares"][1:])                        # half-integer and integer sums: exact
    got = _numpy(metrics._close(torch.from_numpy(sh).to(DEV), torch.from_numpy(cc).to(DEV)))
    assert np.array_equal(got["n_pos"], ref["n_pos"]) and np.array_equal(got["n_invalid"], ref["n_invalid"])
    _check_floats(got, ref, n, C, f"case {name} ({n} x {C} {dtype})")


def test_row_shards_reproduce_the_one_shard_counts():
    """shards of 0, 1, 300 and the remaining rows through the C ABI: the concatenated count arrays are the one-shard arrays bit
    for bit, an empty shard's shares are zero, and the shares add up to the one-shard values (the integer ones exactly)"""
    x, y, dtype = _device_case("quantised")
    n, C = x.shape
    shards = [(0, 0), (0, 1), (1, 300), (301, n - 301)]
    cc, (one,), (one_sh,) = _capi(x, y, dtype, [(0, n)])
    cc2, parts, shares = _capi(x, y, dtype, shards)
    assert np.array_equal(cc, cc2)
    assert np.array_equal(np.concatenate(parts, axis=2), one)
    assert np.array_equal(one, M.restated("quantised")["counts"])
    assert not shares[0].any()
    total = shares[0] + shares[1] + shares[2] + shares[3]
    assert np.array_equal(total[1:], one_sh[1:])
    assert np.abs(total[0] - one_sh[0]).max() <= M.ap_bound(n, world=4) * np.maximum(one_sh[0], 1.0).max()


@pytest.mark.parametrize("label_dtype", [torch.bool, torch.uint8, torch.float32, torch.float16, torch.bfloat16, torch.float64])
def test_python_surface_with_every_label_dtype(label_dtype):
    from aecf_amd import metrics
    x, y, dtype = _device_case("bf16")
    n, C = x.shape
    labels = y.to(label_dtype)
    if label_dtype.is_floating_point:
        labels = labels * 0.25                              # positive iff non-zero, not iff one
    out = metrics.multilabel_metrics(x, labels)
    assert set(out) == {"ap", "auroc", "f1", "n_pos", "n_invalid", "map", "macro_auroc", "macro_f1"}
    assert all(out[k].dtype == torch.float64 and out[k].device == x.device for k in FLOATS)
    assert all(out[k].shape == (C,) for k in ("ap", "auroc", "f1", "n_pos", "n_invalid")) and out["map"].dim() == 0
    assert out["n_pos"].dtype == torch.int64 and out["n_invalid"].dtype == torch.int64
    got, ref = _numpy(out), M.restated("bf16")
    assert np.array_equal(got["n_pos"], ref["n_pos"]) and np.array_equal(got["n_invalid"], ref["n_invalid"])
    _check_floats(got, ref, n, C, f"python surface, labels {label_dtype}")


def test_python_surface_edges_and_threshold():
    """the specials and the degenerate classes through multilabel_metrics; another threshold; refusals"""
    from aecf_amd import metrics
    for name in ("specials", "quantised", "n1"):
        x, y, _ = _device_case(name)
        got, ref = _numpy(metrics.multilabel_metrics(x, y)), M.restated(name)
        assert np.array_equal(got["n_pos"], ref["n_pos"]) and np.array_equal(got["n_invalid"], ref["n_invalid"])
        _check_floats(got, ref, x.shape[0], x.shape[1], f"python surface, case {name}")
    x, y, _ = _device_case("quantised")
    s, yy, _ = M.case("quantised")
    _check_floats(_numpy(metrics.multilabel_metrics(x, y, threshold=0.8)), M.restate(s, yy, threshold=0.8), x.shape[0], x.shape[1],
                  "python surface, threshold 0.8")
    with pytest.raises(ValueError, match="threshold"):
        metrics.multilabel_metrics(x, y, threshold=1.0)
    with pytest.raises(ValueError, match="one shape"):
        metrics.multilabel_metrics(x, y[:-1])
    with pytest.raises(TypeError, match="labels"):
        metrics.multilabel_metrics(x, y.to(torch.int64))
    with pytest.raises(TypeError, match="logits"):
        metrics.multilabel_metrics(x.double(), y)


def test_captured_call_replays_with_new_inputs():
    """one rank reads nothing on the host: the call captures, and three replays with logits and labels changed in place give
    the three restatements"""
    from aecf_amd import metrics
    sets = []
    for name in ("bf16", "f16"):
        s, y, _ = M.case(name)
        sets.append((s, y, M.restated(name)))
    s2, y2 = sets[0][0], ~sets[1][1]
    sets.append((s2, y2, M.restate(s2, y2)))
    n, C = sets[0][0].shape
    x = torch.zeros(n, C, device=DEV)
    y = torch.zeros(n, C, dtype=torch.bool, device=DEV)
    metrics.multilabel_metrics(x, y)                        # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = metrics.multilabel_metrics(x, y)
    for i, (s, lab, ref) in enumerate(sets):
        x.copy_(torch.from_numpy(s.copy()))
        y.copy_(torch.from_numpy(lab.copy()))
        graph.replay()
        torch.cuda.synchronize()
        got = _numpy(out)
        assert np.array_equal(got["n_pos"], ref["n_pos"]) and np.array_equal(got["n_invalid"], ref["n_invalid"])
        _check_floats(got, ref, n, C, f"replay {i}")


# ---------------------------------------------------------------------------------------------- two ranks

TWO_RANK_CASE = "bf16"
SPLITS = {"uneven": None, "empty": (1.0, 0.0)}             # None: dp.shard_bounds (513 and 512 of 1025 rows); rank 1 holds no row


def _two_ranks_worker(rank, world, port, backend, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from aecf_amd import dp, metrics
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    limit = datetime.timedelta(seconds=90)          # a collective without its partner raises here instead of hanging
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=limit)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=limit)
    done, error = {}, None
    try:
        x, y, _ = _device_case(TWO_RANK_CASE, dev)
        n = x.shape[0]
        for split, how in SPLITS.items():
            lo, hi = dp.shard_bounds(n, rank, world) if how is None else ((0, n) if rank == 0 else (n, n))
            done[split] = _numpy(metrics.multilabel_metrics(x[lo:hi], y[lo:hi], group=dist.group.WORLD))
            done[split]["rows"] = hi - lo
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


@pytest.mark.parametrize("split", list(SPLITS))
def test_two_ranks_equal_one_rank(two_ranks, split):
    """both ranks return the global values -- the same bits on both -- inside the bound of the restatement of all rows, and
    within it of the one-rank result"""
    from aecf_amd import metrics
    ref = M.restated(TWO_RANK_CASE)
    x, y, _ = _device_case(TWO_RANK_CASE)
    n, C = x.shape
    one = _numpy(metrics.multilabel_metrics(x, y))
    r0, r1 = (dict(r[split]) for r in two_ranks)
    assert r0.pop("rows") + r1.pop("rows") == n
    for k in r0:
        assert np.array_equal(r0[k], r1[k], equal_nan=True), k
    assert np.array_equal(r0["n_pos"], ref["n_pos"]) and np.array_equal(r0["n_invalid"], ref["n_invalid"])
    _check_floats(r0, ref, n, C, f"two ranks, {split} shards", world=2)
    _check_floats(r0, one, n, C, f"two ranks against one, {split} shards", world=2)


# ---------------------------------------------------------------------------------------------- the trainer

def test_trainer_full_metrics(monkeypatch):
    """train_xray.main --full-metrics --ema-decay for one tiny epoch: the epoch row's val_map_exact, val_auroc and val_macro_f1
    (and their _no_images / _no_texts / ema_ forms) are the restatement on the logits the trainer scored; without the flag the
    evaluation is not called and the row has today's keys."""
    from aecf_amd import train_xray
    seen = []
    real = train_xray.multilabel_metrics

    def spy(logits, labels, **kw):
        seen.append((logits.float().cpu().numpy(), labels.cpu().numpy()))
        return real(logits, labels, **kw)

    monkeypatch.setattr(train_xray, "multilabel_metrics", spy)
    argv = ["--epochs", "1", "--switch-epoch", "1", "--samples", "128", "--val-samples", "130", "--batch", "64", "--classes", "5"]
    (row,) = train_xray.main(argv + ["--full-metrics", "--ema-decay", "0.99"])
    assert len(seen) == 6                                   # the model, then the averaged weights: none, no images, no texts
    names = [prefix + "val_{}" + suffix for prefix in ("", "ema_") for suffix in ("", "_no_images", "_no_texts")]
    for (s, y), name in zip(seen, names):
        assert s.shape == (130, 5)
        ref = M.restate(s, y)
        b = M.ap_bound(130)
        assert abs(row[name.format("map_exact")] - ref["map"]) <= M.macro_bound(b, 5)
        assert abs(row[name.format("auroc")] - ref["macro_auroc"]) <= M.macro_bound(M.AUROC_BOUND, 5)
        assert abs(row[name.format("macro_f1")] - ref["macro_f1"]) <= M.macro_bound(M.F1_BOUND, 5)
    (plain,) = train_xray.main(argv + ["--ema-decay", "0.99"])
    assert len(seen) == 6                                   # the flag is off: the evaluation is not called
    assert set(plain) == {"epoch", "curriculum", "train_loss", "gate_entropy", "sec", "val_map", "val_map_no_images", "val_map_no_texts",
                          "ema_val_map", "ema_val_map_no_images", "ema_val_map_no_texts"}
    assert set(row) == set(plain) | {n.format(m) for n in names for m in ("map_exact", "auroc", "macro_f1")}
