"""Train throughput of a converter config with a num filter, against the same
config without it: an AROW classifier and PA regression over 16 numeric
features, normalised with gaussian_normalization (one filter rule, key `*`:
two num rule rows, so twice the slots of the filter-free config).

* driver   LinearClassifier.train / PARegression.train in this process, in
           chunks of --driver-batch samples
* served   the native jubaclassifier / jubaregression over RPC, driven by
           jubaloadgen (pre-encoded train requests of --batch samples,
           --conns connections, --depth requests in flight each)

Where the fixed-slot path serves filters the filter config converts on the
GPU (request scan + fv_hash.hip); where it does not (a tree before that
change) the same run converts on the host, so running this file in both
trees with the same arguments compares the two on the same stream. Each case
runs for --seconds after a warm-up; one JSON line per case, then one line
with all of them.

Usage: python tools/bench_fv_num_filters.py [--batch 64] [--driver-batch 1024]
       [--seconds 4] [--conns 8] [--depth 4] [--skip-served] [--out FILE.json]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import msgpack
import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
NATIVE_BIN = os.path.join(ROOT, "jubatus_amd", "native_bin")

DIM = 16
PLAIN = {"num_rules": [{"key": "*", "type": "num"}], "hash_max_size": 1 << 20}
FILTER = {"num_filter_types": {"z": {"method": "gaussian_normalization", "average": 1.0,
                                     "standard_deviation": 2.0}},
          "num_filter_rules": [{"key": "*", "type": "z", "suffix": "_z"}],
          "num_rules": [{"key": "*", "type": "num"}], "hash_max_size": 1 << 20}
ENGINES = {"classifier": ("AROW", {"regularization_weight": 1.0}),
           "regression": ("PA", {"sensitivity": 0.1, "regularization_weight": 1.0})}


def stream(engine, n, seed=0):
    """n samples: [label or target, {f0..f15: float}]"""
    rng = np.random.default_rng(seed)
    y = rng.integers(4, size=n)
    X = rng.normal(1.0 + 0.5 * y[:, None], 2.0, size=(n, DIM))
    keys = [f"f{j}" for j in range(DIM)]
    first = (lambda i: f"L{y[i]}") if engine == "classifier" else (lambda i: float(X[i].sum()))
    return [[first(i), dict(zip(keys, map(float, X[i])))] for i in range(n)]


def driver_case(engine, conv_cfg, batch, seconds):
    import torch
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.fv_converter.gpu_path import gpu_eligible
    dev = torch.device("cuda", 0)
    method, param = ENGINES[engine]
    conv = DatumToFvConverter(conv_cfg)
    if engine == "classifier":
        from jubatus_amd.models.classifier import LinearClassifier
        m = LinearClassifier(method, param, conv, device=dev)
        sync = m.synchronize
    else:
        from jubatus_amd.models.regression import PARegression
        m = PARegression(method, param, conv, dev)
        sync = torch.cuda.synchronize
    chunks = [stream(engine, batch, seed=s) for s in range(8)]
    m.train(chunks[0])
    sync()
    done, k, t0 = 0, 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        done += m.train(chunks[k % len(chunks)])
        k += 1
    sync()
    dt = time.perf_counter() - t0
    return {"samples_per_s": round(done / dt, 1), "samples": done, "seconds": round(dt, 3),
            "gpu_conversion": bool(gpu_eligible(conv))}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def served_case(engine, conv_cfg, batch, seconds, conns, depth, tmp):
    from jubatus_amd.common.mprpc import RpcClient, RpcIOError, RpcTimeoutError
    from jubatus_amd.fv_converter.datum import Datum
    exe = os.path.join(NATIVE_BIN, "juba" + engine)
    gen = os.path.join(NATIVE_BIN, "jubaloadgen")
    if not (os.path.exists(exe) and os.path.exists(gen)):
        return {"skipped": "native server / jubaloadgen not built"}
    method, param = ENGINES[engine]
    cfg = os.path.join(tmp, f"{engine}.json")
    with open(cfg, "w") as f:
        json.dump({"method": method, "parameter": param, "converter": conv_cfg}, f)
    params = os.path.join(tmp, f"{engine}.bin")
    with open(params, "wb") as f:
        for s in range(2 * conns):
            f.write(msgpack.packb(["", [[y, Datum(d).to_msgpack()] for y, d in stream(engine, batch, seed=s)]],
                                  use_bin_type=False))
    port = _free_port()
    p = subprocess.Popen([exe, "-p", str(port), "-b", "127.0.0.1", "-f", cfg, "-d", tmp, "-c", "16"],
                         stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    try:
        deadline = time.time() + 60
        while True:
            try:
                with RpcClient("127.0.0.1", port, 5.0) as c:
                    c.call("get_config", "")
                break
            except (OSError, RpcIOError, RpcTimeoutError):
                if p.poll() is not None or time.time() > deadline:
                    return {"error": "server did not start"}
                time.sleep(0.1)

        def load(t):
            r = subprocess.run([gen, "-p", str(port), "-m", "train", "-f", params, "-c", str(conns),
                                "-d", str(depth), "-t", str(t)], capture_output=True, text=True,
                               timeout=t + 120)
            if r.returncode != 0:
                raise RuntimeError((r.stderr or r.stdout)[-300:])
            return json.loads(r.stdout.strip().splitlines()[-1])
        load(1.0)                                  # labels, buffers, first-launch costs
        r = load(seconds)
        with RpcClient("127.0.0.1", port, 10.0) as c:
            (st,) = c.call("get_status", "").values()
        st = {(k.decode() if isinstance(k, bytes) else k): (v.decode() if isinstance(v, bytes) else v)
              for k, v in st.items()}
        return {"samples_per_s": round(r["requests_per_s"] * batch, 1), "requests_per_s": r["requests_per_s"],
                "p50_us": r["p50_us"], "p99_us": r["p99_us"], "seconds": r["seconds"],
                "train_scan.gpu": st.get("train_scan.gpu"), "train_scan.host": st.get("train_scan.host"),
                "server_runtime": st.get("server_runtime")}
    finally:
        p.terminate()
        try:
            p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            p.kill()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64,
                    help="samples per served train request (about 16 KB: the device scan takes it)")
    ap.add_argument("--driver-batch", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--conns", type=int, default=8)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--skip-served", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_fv_num_filters: no GPU (a CPU run gives no timing)\n")
        return 2
    res = {"batch": a.batch, "driver_batch": a.driver_batch, "features": DIM,
           "device": torch.cuda.get_device_name(0), "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for engine in ENGINES:
            for name, cfg in (("filter", FILTER), ("plain", PLAIN)):
                r = driver_case(engine, cfg, a.driver_batch, a.seconds)
                res["cases"][f"driver/{engine}/{name}"] = r
                print(json.dumps({f"driver/{engine}/{name}": r}), flush=True)
                if not a.skip_served:
                    r = served_case(engine, cfg, a.batch, a.seconds, a.conns, a.depth, tmp)
                    res["cases"][f"served/{engine}/{name}"] = r
                    print(json.dumps({f"served/{engine}/{name}": r}), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
