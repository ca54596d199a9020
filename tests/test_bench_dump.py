"""`bench.py --dump-outputs DIR`: what the timed path computed in its last timed step, as float32 / float64 .npy files of at most
64 MB, from inputs that are the same every run -- so that two builds can be compared output for output."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import ROOT

DUMP_LIMIT = 64 * 10 ** 6


def _bench_module(monkeypatch):
    # bench.py sets HIP_FORCE_DEV_KERNARG when it is imported: keep this process's environment as it was
    monkeypatch.setenv("HIP_FORCE_DEV_KERNARG", os.environ.get("HIP_FORCE_DEV_KERNARG", "1"))
    import bench
    return bench


def _load_dir(d):
    return {os.path.basename(p)[:-4]: np.load(p, allow_pickle=False) for p in sorted(glob.glob(os.path.join(d, "*.npy")))}


def _dir_bytes(d):
    return sum(os.path.getsize(p) for p in glob.glob(os.path.join(d, "*")))


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    """A batch too large for the budget: every batch-major array keeps the same seeded, sorted sample of rows (rows.npy), the
    same in every call; other arrays are written whole; bf16 is widened to float32 exactly, float64 stays float64."""
    bench = _bench_module(monkeypatch)
    g = torch.Generator().manual_seed(3)
    B = 40000
    per_row = {"out": torch.randn(B, 1, 512, generator=g).to(torch.bfloat16), "grad.x": torch.randn(B, 3, 128, generator=g)}
    whole = {"loss": torch.tensor(0.25, dtype=torch.float64), "grad.w": torch.randn(384, 128, generator=g)}
    runs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        summary = bench.dump_outputs(d, B, per_row, whole)
        got = _load_dir(d)
        assert _dir_bytes(d) <= DUMP_LIMIT and summary["bytes"] <= DUMP_LIMIT
        assert sorted(got) == ["grad.w", "grad.x", "loss", "out", "rows"]
        assert all(a.dtype in (np.float32, np.float64) for a in got.values())
        assert got["loss"].dtype == np.float64 and float(got["loss"]) == 0.25
        rows = got["rows"].astype(np.int64)
        assert summary["rows"] == len(rows) and 1000 < len(rows) < B
        assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < B
        np.testing.assert_array_equal(got["out"], per_row["out"].float().numpy()[rows])
        np.testing.assert_array_equal(got["grad.x"], per_row["grad.x"].numpy()[rows])
        np.testing.assert_array_equal(got["grad.w"], whole["grad.w"].numpy())
        runs.append(got)
    np.testing.assert_array_equal(runs[0]["rows"], runs[1]["rows"])


def test_dump_outputs_small_batch_is_written_whole(tmp_path, monkeypatch):
    bench = _bench_module(monkeypatch)
    per_row = {"out": torch.randn(64, 1, 32)}
    summary = bench.dump_outputs(str(tmp_path), 64, per_row, {"loss": torch.tensor(1.0)})
    got = _load_dir(str(tmp_path))
    assert sorted(got) == ["loss", "out"] and summary["rows"] == 64
    np.testing.assert_array_equal(got["out"], per_row["out"].numpy())


def _run_bench(args, timeout=280):
    env = dict(os.environ, AECF_BENCH_DUMP_STEPS="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return line, r.stderr


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_bit_for_bit(tmp_path):
    """Two runs with the same arguments: exactly --steps timed steps, ms_per_step in the line, and the same outputs bit for bit
    (the library has no float atomics; the mask draws of the dumped step do not depend on how long the process settled).
    d256 at 16384 rows: a shape whose settle would otherwise run by the clock, with more rows than the dump holds."""
    dumps = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        line, err = _run_bench(["--config", "d256", "--rows", "16384", "--steps", "3", "--warmup", "2", "--no-cpu-baseline",
                                "--dump-outputs", d])
        step_ms = [l for l in err.splitlines() if l.startswith("step_ms")]
        assert len(step_ms) == 1 and len(json.loads(step_ms[0][len("step_ms"):])) == 3
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        assert line["dump_outputs"]["dir"] == d and _dir_bytes(d) <= DUMP_LIMIT
        got = _load_dir(d)
        for k in ("out", "loss", "grad.x", "grad.query", "grad.attention.in_proj_weight", "grad.attention.out_proj.weight",
                  "info.attention_weights", "info.masked_attention_weights", "info.entropy", "rows"):
            assert k in got, (k, sorted(got))
        assert all(a.dtype in (np.float32, np.float64) for a in got.values())
        assert all(np.isfinite(a).all() for a in got.values())
        assert got["out"].shape == (len(got["rows"]), 1, 256) and got["grad.x"].shape == (len(got["rows"]), 3, 256)
        dumps.append(got)
    assert sorted(dumps[0]) == sorted(dumps[1])
    for k in dumps[0]:
        np.testing.assert_array_equal(dumps[0][k], dumps[1][k], err_msg=k)


@pytest.mark.gpu
def test_bench_example_model_dump_outputs(tmp_path):
    """--config c4: the step's loss and info, the updated parameters and their gradients."""
    d = str(tmp_path / "c4")
    line, _ = _run_bench(["--config", "c4", "--batch", "64", "--steps", "2", "--warmup", "1", "--dump-outputs", d])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["dump_outputs"]["rows"] == 64
    got = _load_dir(d)
    assert "loss" in got and "info.attention_weights" in got and "rows" not in got
    assert "param.attention_pool.attention.in_proj_weight" in got and "grad.classifier.3.weight" in got
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
