"""bench.py's command line: a plain run prints the headline alone (everything else is behind --full), and --dump-outputs writes what the
last timed step returned, identically from run to run with the same arguments (two builds are compared output for output that way)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_bench_dumps_identical_outputs(tmp_path):
    def run(tag):
        out = tmp_path / tag
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16", "--patch", "32",
               "--dump-outputs", str(out)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=420)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        files = sorted(os.listdir(out))
        return d, files, {f: np.load(out / f) for f in files}, sum(os.path.getsize(out / f) for f in files)

    d1, files1, a1, size1 = run("a")
    d2, files2, a2, _ = run("b")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d1, k
    assert d1["steps"] == 3 and d1["ms_per_step"] > 0 and d1["value"] > 0
    # the legs of --full are not run
    for k in ("roofline", "parity", "eval", "alt_geometry", "alt_model", "cpu_baseline"):
        assert k not in d1, k
    assert files1 == files2 == ["loss.npy", "weights_sample.npy"]
    assert size1 <= 64 << 20
    for f in files1:
        assert a1[f].dtype in (np.float32, np.float64), (f, a1[f].dtype)
        assert np.isfinite(a1[f]).all(), f
        assert np.array_equal(a1[f], a2[f]), f"{f} differs between two runs with the same arguments"
    assert abs(float(a1["loss.npy"][0]) - d1["loss"]) < 1e-4
    assert a1["weights_sample.npy"].size > 100_000
