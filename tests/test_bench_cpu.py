"""bench.py contract rehearsed on the CPU: 2 ranks over gloo through
torch.distributed.run (127.0.0.1 rendezvous), one JSON line from rank 0 with
the fields the driver reads; the overlapped and synchronous MIX both run."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("mode", ["overlap", "sync"])
def test_bench_two_ranks_cpu(mode):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--device", "cpu", "--requests", "8",
           "--per-request", "16", "--hash-bits", "12", "--latency-iters", "5", "--mix-mode", mode,
           "--batches-per-step", "2", "--dist-engines", "none"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in out
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["config"]["parallelism"] == "dp2"
    assert out["config"]["global_batch"] == 2 * 2 * 8 * 16 and mode in out["config"]["mix"]
    assert out["config"]["world_size_observed"] == 2
    assert out["timed_samples_per_rank"] == 2 * 2 * 8 * 16
    assert 0.0 < out["update_fraction"] <= 1.0


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    """a plain run measures the headline alone (the secondary records are
    null without --full); --dump-outputs writes what the last timed step
    computed as float .npy files - on the host engine, whose update order is
    defined, the model too - and a second run with the same arguments trains
    on the same bytes: the dumps are equal"""
    import numpy as np
    dumps = []
    for i in range(2):
        d = tmp_path / f"dump{i}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
               "--device", "cpu", "--requests", "8", "--per-request", "16", "--hash-bits", "12",
               "--batches-per-step", "2", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd="/tmp")
        assert r.returncode == 0, r.stderr[-3000:]
        out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["full"] is False
        assert out["timed_samples_per_rank"] == 3 * 2 * 8 * 16
        for k in ("heldout_accuracy", "classify_latency_us_p50", "exact_mode", "served", "engines"):
            assert out[k] is None
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = dumps
    assert set(a) == {"run_shape.npy", "step_samples.npy", "samples_trained.npy", "label_counts.npy", "W.npy",
                      "P.npy", "rows.npy", "samples_updated.npy", "heldout_scores.npy"}
    assert a["run_shape.npy"].tolist() == [2, 3]
    assert a["W.npy"].shape == a["P.npy"].shape == (1 << 12, 16)
    assert a["step_samples.npy"].tolist() == [8 * 16, 8 * 16]
    assert a["samples_trained.npy"][0] == 3 * 2 * 8 * 16 and np.any(a["W.npy"] != 0)
    assert sum(x.nbytes for x in a.values()) <= 64_000_000
    for f in a:
        assert a[f].dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a[f], b[f])


def test_dump_samples_fixed_rows_of_a_large_table(tmp_path, monkeypatch):
    """tables above the dump's size limit: a seeded sample of the rows, the
    same rows in every run, their numbers in rows.npy"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_TABLE_BYTES", 64 * 16 * 4)
    W = np.arange(1000 * 16, dtype=np.float32).reshape(1000, 16)

    class Model:
        def _host_tables(self):
            return W, None

        def get_labels(self):
            return {"b": 2, "a": 1}

    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), Model(), [2, 7], [5, 5], {}, 10,
                           bench._model_arrays(Model(), 3, [[0.5, -0.5]]))
    # the serial probe's model goes beside the run's own records under its prefix
    bench.dump_outputs(str(tmp_path / "z"), Model(), [2, 7], [5, 5], {"last_batch_fidx": np.zeros(3, np.float32)}, 10,
                       bench._model_arrays(Model(), 3, [[0.5, -0.5]], "serial_"))
    assert sorted(os.listdir(tmp_path / "z")) == [
        "label_counts.npy", "last_batch_fidx.npy", "rows.npy", "run_shape.npy", "samples_trained.npy",
        "serial_W.npy", "serial_heldout_scores.npy", "serial_samples_updated.npy", "step_samples.npy"]
    assert np.load(tmp_path / "x" / "run_shape.npy").tolist() == [2.0, 7.0]
    rows = np.load(tmp_path / "x" / "rows.npy")
    assert rows.shape == (64,) and np.all(np.diff(rows) > 0) and rows.dtype == np.float64
    np.testing.assert_array_equal(rows, np.load(tmp_path / "y" / "rows.npy"))
    np.testing.assert_array_equal(np.load(tmp_path / "x" / "W.npy"), W[rows.astype(np.int64)])
    assert not (tmp_path / "x" / "P.npy").exists()
    assert np.load(tmp_path / "x" / "label_counts.npy").tolist() == [1.0, 2.0]
    assert np.load(tmp_path / "x" / "samples_trained.npy").tolist() == [10.0]
    assert np.load(tmp_path / "x" / "samples_updated.npy").tolist() == [3.0]


def test_bench_spawns_ranks_without_torchrun():
    """--gpus N without WORLD_SIZE: bench.py launches the N ranks itself"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1",
           "--warmup", "1", "--device", "cpu", "--requests", "4", "--per-request", "8",
           "--hash-bits", "10", "--latency-iters", "2", "--batches-per-step", "1", "--dist-engines", "none"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd="/tmp", env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert out["n_gpus"] == 2 and out["config"]["world_size_observed"] == 2
