"""bench.py on one GPU: a plain run prints the headline and nothing behind it; --full adds the checks of the stream and
the CPU baseline; both compute the same stream (their --dump-outputs arrays are equal) and --full finds it equal to the
oracle's golden."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--mib-per-gpu", "64", "--hang-timeout", "240"]


def _bench(extra_args, dump_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra_args + ["--dump-outputs", str(dump_dir)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _dumped(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_bench_plain_and_full_runs(tmp_path):
    plain = _bench([], tmp_path / "plain")
    assert plain["metric"].startswith("BZip2 level-9 encode MB/s") and plain["unit"] == "MB/s"
    assert plain["higher_is_better"] is True and plain["dtype"] == "u8/u32"
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["steps"] == 2 and plain["warmup"] == 1
    assert plain["step_ms"]["n"] == 2 and plain["roofline"]["frac"] > 0
    for k in ("checks", "stream_sha256", "cpu_baseline", "cpu_baseline_all_cores", "end_to_end", "extra", "t2_stress"):
        assert k not in plain, k

    full = _bench(["--full", "--no-extras", "--cpu-sample-mib", "8"], tmp_path / "full")
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["cores"] == 1
    checks = full["checks"]
    for k in ("head_decodes_to_input", "stream_sha_equals_oracle_golden", "gpu_equals_oracle_on_cpu_sample"):
        assert checks.get(k) is True, (k, checks)
    assert full["config"]["out_bytes"] == plain["config"]["out_bytes"]

    a, b = _dumped(tmp_path / "plain"), _dumped(tmp_path / "full")
    assert sorted(a) == sorted(b) and "stream_length.npy" in a
    assert int(a["stream_length.npy"][0]) == plain["config"]["out_bytes"]
    for f in a:
        assert np.array_equal(a[f], b[f]), f
