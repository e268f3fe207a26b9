"""Nearest-neighbour regression, time of one estimate batch on the GPU, two
paths over the same table (models/nn_regression.py, NN / euclid_lsh):

* fused    NNRegression.estimate: the batch converted at once, one device
           top-k, csrc/hip/nn_reduce.hip, one copy of nq floats
* unfused  what the NN classifier does today: engine.query_datum per datum
           (every (row id, distance) pair to the host), a dictionary lookup per
           pair and a host loop

Each path is warmed up, then timed --repeat times with a host clock between
two device synchronisations; the medians and the spread are printed as one
JSON line and written as a table to --out.

Usage: python tools/bench_nn_regression.py [--rows 100000] [--batch 256]
       [--k 128] [--hash-num 64] [--dim 16] [--weight distance] [--warmup 3]
       [--repeat 20] [--out profiles/nn_regression_estimate.md]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CONVERTER = {"num_rules": [{"key": "*", "type": "num"}]}


def unfused(drv, ds):
    """the NN classifier's scheme (models/nn_classifier.py classify / _score)
    with targets in place of labels"""
    out = []
    for d in ds:
        nb = drv.engine.query_datum(d, drv.k, False)
        dmin = min((v for _, v in nb), default=0.0)
        sw = swt = 0.0
        for rid, v in nb:
            t = drv.row_target.get(rid)
            if t is None:
                continue
            w = math.exp(-drv.alpha * (v - dmin)) if drv.mode == 1 else 1.0
            sw += w
            swt += w * t
        out.append(swt / sw if sw > 0 else 0.0)
    return out


def timed(fn, warmup, repeat):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--hash-num", type=int, default=64)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--weight", choices=("uniform", "distance"), default="distance")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_nn_regression: no GPU (a CPU run gives no timing)\n")
        return 2
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.fv_converter.datum import as_datum
    from jubatus_amd.models.nn_regression import NNRegression

    dev = torch.device("cuda", 0)
    drv = NNRegression("NN", {"method": "euclid_lsh", "parameter": {"hash_num": a.hash_num},
                              "nearest_neighbor_num": a.k, "weight": a.weight,
                              "local_sensitivity": 1.0}, DatumToFvConverter(CONVERTER), device=dev)
    rng = np.random.default_rng(0)
    coef = rng.normal(size=a.dim)
    keys = [f"n{j}" for j in range(a.dim)]
    t0 = time.perf_counter()
    for b0 in range(0, a.rows, 10000):
        X = rng.normal(size=(min(10000, a.rows - b0), a.dim))
        y = X @ coef
        drv.train([[float(t), dict(zip(keys, map(float, x)))] for x, t in zip(X, y)])
    torch.cuda.synchronize()
    fill_s = time.perf_counter() - t0
    Q = rng.normal(size=(a.batch, a.dim))
    ds = [as_datum(dict(zip(keys, map(float, q)))) for q in Q]

    fused = drv.estimate(ds)
    slow = unfused(drv, ds)
    dev_max = float(np.abs(np.asarray(fused) - np.asarray(slow)).max())
    # alternate the two paths, so that both see the same machine
    tf, tu = [], []
    timed(lambda: drv.estimate(ds), a.warmup, 0)
    timed(lambda: unfused(drv, ds), a.warmup, 0)
    for _ in range(a.repeat):
        tf += timed(lambda: drv.estimate(ds), 0, 1)
        tu += timed(lambda: unfused(drv, ds), 0, 1)
    res = {"rows": a.rows, "batch": a.batch, "k": a.k, "hash_num": a.hash_num, "dim": a.dim,
           "weight": a.weight, "repeat": a.repeat, "fill_s": round(fill_s, 2),
           "fused_ms_median": round(statistics.median(tf), 3),
           "fused_ms_min": round(min(tf), 3), "fused_ms_max": round(max(tf), 3),
           "unfused_ms_median": round(statistics.median(tu), 3),
           "unfused_ms_min": round(min(tu), 3), "unfused_ms_max": round(max(tu), 3),
           "max_abs_difference": dev_max, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if a.out:
        names = {"fused": f"fused (batch conversion, device top-k, nn_reduce, one copy of {a.batch} floats)",
                 "unfused": "unfused (query_datum per datum, host lookups and loop)"}
        rows_md = "\n".join(
            f"| {names[p]} | {res[p + '_ms_median']} | {res[p + '_ms_min']} | {res[p + '_ms_max']} | "
            f"{res[p + '_ms_median'] * 1e3 / a.batch:.1f} |" for p in ("fused", "unfused"))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"""# Nearest-neighbour regression: one estimate batch, fused against unfused

`python tools/bench_nn_regression.py --rows {a.rows} --batch {a.batch} --k {a.k} --hash-num {a.hash_num}
--dim {a.dim} --weight {a.weight} --warmup {a.warmup} --repeat {a.repeat}` on {res["device"]}.

Table: {a.rows} rows, NN / euclid_lsh, hash_num {a.hash_num}, {a.dim} numeric features per datum,
k = {a.k}, weight {a.weight}. One call estimates {a.batch} datums. Host clock between two device
synchronisations, {a.warmup} warm-up calls per path, then {a.repeat} timed calls per path,
alternating. Whole-call times (conversion, top-k, reduction, copies), not kernel times.

| path | median ms | min ms | max ms | per datum, us (median) |
|---|---|---|---|---|
{rows_md}

Largest difference between the two paths' estimates: {dev_max:.3g} (float64 host loop against
the fp32 kernel). Filling the table took {res["fill_s"]} s.
""")
    return 0


if __name__ == "__main__":
    sys.exit(main())
