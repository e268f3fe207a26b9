"""bench.py --dump-outputs on the GPU: two runs with the same arguments write
equal files, in the headline's lock-free update mode (whose dump holds the
scanned last batch and the serial probe of the train kernel) and in the
exact mode (whose dump holds the timed steps' model)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = {"run_shape.npy", "step_samples.npy", "samples_trained.npy", "label_counts.npy", "rows.npy",
          "last_batch_row_ptr.npy", "last_batch_labels.npy", "last_batch_fidx.npy", "last_batch_fval.npy"}
MODEL = ("W.npy", "P.npy", "samples_updated.npy", "heldout_scores.npy")


@pytest.mark.parametrize("mode", ["atomic", "exact"])
def test_two_runs_dump_equal_files(mode, tmp_path):
    # 3 steps x 2 batches of 64 requests x 32 samples; the two runs share the GPU
    runs = []
    for i in range(2):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
               "--requests", "64", "--per-request", "32", "--hash-bits", "16", "--batches-per-step", "2",
               "--update-mode", mode, "--dump-outputs", str(tmp_path / f"d{i}")]
        runs.append(subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    dumps = []
    for i, p in enumerate(runs):
        out, err = p.communicate(timeout=200)
        assert p.returncode == 0, err[-3000:]
        line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 3 and line["full"] is False and line["config"]["concurrent_update"] == mode
        d = tmp_path / f"d{i}"
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = dumps
    prefix = "" if mode == "exact" else "serial_"
    assert set(a) == COMMON | {prefix + f for f in MODEL}
    n = 64 * 32
    assert a["run_shape.npy"].tolist() == [2, 3] and a["step_samples.npy"].tolist() == [n, n]
    assert a["samples_trained.npy"].tolist() == [3 * 2 * n]
    # the whole last batch: 8 string + 8 numeric features a sample
    assert a["last_batch_row_ptr.npy"].tolist() == list(range(0, 16 * n + 1, 16))
    assert a["last_batch_fidx.npy"].shape == (16 * n,) and a["last_batch_fidx.npy"].min() >= 0
    assert a[prefix + "W.npy"].shape == a[prefix + "P.npy"].shape == (1 << 16, 16)
    assert np.any(a[prefix + "W.npy"] != 0) and 0 < a[prefix + "samples_updated.npy"][0] <= 3 * 2 * n
    assert a[prefix + "heldout_scores.npy"].shape == (2048, 16)
    for f in a:
        assert a[f].dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)
