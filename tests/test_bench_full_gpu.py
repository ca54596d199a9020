"""`bench.py` with and without `--full`: a plain run measures the headline figure and nothing more; `--full` adds the passes of
their own after the timed steps (per-stage HIP-event times, roofline, CPU baseline) to the same line."""
import json
import os
import subprocess
import sys

import pytest

from tests.helpers import ROOT

pytestmark = pytest.mark.gpu

EXTRAS = ("stage_ms", "stage_pass", "roofline", "cpu_baseline", "collective_ms", "strong_scaling")


def _run_bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "tiny", "--steps", "5", "--warmup", "2",
                        "--settle-seconds", "0"] + args, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.timeout(300)
def test_plain_run_reports_the_headline_only():
    line = _run_bench([])
    assert line["full"] is False and line["steps"] == 5 and line["warmup"] == 2
    assert line["metric"] == "fused samples/sec (fwd+bwd)" and line["unit"] == "samples/s" and line["dtype"] == "bf16"
    assert line["higher_is_better"] is True and line["value"] > 0 and line["ms_per_step"] > 0
    for k in EXTRAS:
        assert line[k] is None, (k, line[k])


@pytest.mark.timeout(300)
def test_full_run_adds_stage_times_roofline_and_cpu_baseline():
    line = _run_bench(["--full", "--cpu-baseline-seconds", "5"])
    assert line["full"] is True and line["steps"] == 5 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["stage_ms"] and all(v >= 0 for v in line["stage_ms"].values())
    assert line["stage_pass"]["steps"] > 0 and line["stage_pass"]["sum_ms"] > 0
    assert line["roofline"]["kernel"] in line["stage_ms"] and line["roofline"]["frac"] > 0
    cb = line["cpu_baseline"]
    assert cb["value"] > 0 and cb["unit"] == "samples/s" and cb["threads"] >= 1
