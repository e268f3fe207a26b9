"""Nearest-neighbour classifiers, time of one classify call on the GPU, two
paths over the same table (models/nn_classifier.py), for config/classifier/
nn.json (NN / euclid_lsh) and cosine.json (inverted index):

* fused      NNClassifier._classify_fused: the batch converted at once, one
             device top-k, csrc/hip/nn_vote.hip, one copy of [nq, labels]
* per datum  NNClassifier._classify_each: engine.query_datum per datum (every
             (row id, distance) pair to the host), a dictionary lookup per
             pair and a host loop; the classify path before the vote kernel

Per batch size each path is warmed up, then timed --repeat times with a host
clock between two device synchronisations, the two paths alternating; the
medians and the spread are printed as one JSON line per configuration and
written as a table to --out.

Usage: python tools/bench_nn_classifier.py [--rows 100000] [--labels 16]
       [--batches 1,8,64,256] [--dim 16] [--warmup 3] [--repeat 15]
       [--commit ID] [--out profiles/nn_classifier_classify.md]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

CONFIGS = ("nn.json", "cosine.json")


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


def commit_id():
    try:
        r = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                           text=True, timeout=10)
        return r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else "unknown"
    except OSError:
        return "unknown"


def stats(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3),
            "max": round(max(ts), 3)}


def run(cfg_name, a, dev):
    import torch
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.fv_converter.datum import as_datum
    from jubatus_amd.models.nn_classifier import NNClassifier

    cfg = json.load(open(os.path.join(ROOT, "config", "classifier", cfg_name)))
    drv = NNClassifier(cfg["method"], cfg["parameter"], DatumToFvConverter(cfg["converter"]),
                       device=dev)
    rng = np.random.default_rng(0)
    centres = rng.normal(size=(a.labels, a.dim)) * 2.0
    keys = [f"n{j}" for j in range(a.dim)]
    t0 = time.perf_counter()
    for b0 in range(0, a.rows, 10000):
        n = min(10000, a.rows - b0)
        lab = rng.integers(0, a.labels, n)
        X = centres[lab] + rng.normal(size=(n, a.dim))
        drv.train([(f"L{int(c)}", dict(zip(keys, map(float, x)))) for x, c in zip(X, lab)])
    torch.cuda.synchronize()
    fill_s = time.perf_counter() - t0
    res = {"config": cfg_name, "method": cfg["method"], "k": drv.k, "rows": a.rows,
           "labels": a.labels, "dim": a.dim, "repeat": a.repeat, "warmup": a.warmup,
           "fill_s": round(fill_s, 2), "batches": {}}
    for nq in a.batches:
        lab = rng.integers(0, a.labels, nq)
        Q = centres[lab] + rng.normal(size=(nq, a.dim))
        ds = [as_datum(dict(zip(keys, map(float, q)))) for q in Q]
        fused = drv._classify_fused(ds)
        each = drv._classify_each(ds)
        assert [[lab for lab, _ in r] for r in fused] == [[lab for lab, _ in r] for r in each]
        diff = max(abs(x - y) for rf, re in zip(fused, each) for (_, x), (_, y) in zip(rf, re))
        # alternate the two paths, so that both see the same machine
        tf, te = [], []
        timed(lambda: drv._classify_fused(ds), a.warmup, 0)
        timed(lambda: drv._classify_each(ds), a.warmup, 0)
        for _ in range(a.repeat):
            tf += timed(lambda: drv._classify_fused(ds), 0, 1)
            te += timed(lambda: drv._classify_each(ds), 0, 1)
        res["batches"][str(nq)] = {"fused_ms": stats(tf), "per_datum_ms": stats(te),
                                   "max_abs_difference": diff}
    return res


def table(res):
    lines = ["| datums | fused median ms | fused min .. max | per datum median ms | "
             "per datum min .. max | per datum / fused |", "|---|---|---|---|---|---|"]
    for nq, r in res["batches"].items():
        f, e = r["fused_ms"], r["per_datum_ms"]
        lines.append(f"| {nq} | {f['median']} | {f['min']} .. {f['max']} | {e['median']} | "
                     f"{e['min']} .. {e['max']} | {e['median'] / f['median']:.2f} |")
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--labels", type=int, default=16)
    ap.add_argument("--batches", type=lambda s: [int(x) for x in s.split(",")],
                    default=[1, 8, 64, 256])
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=15)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_nn_classifier: no GPU (a CPU run gives no timing)\n")
        return 2
    dev = torch.device("cuda", 0)
    commit = a.commit or commit_id()
    results = []
    for cfg_name in CONFIGS:
        res = run(cfg_name, a, dev)
        res["commit"] = commit
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        parts = [f"""# Nearest-neighbour classifiers: one classify call, fused against per datum

`python tools/bench_nn_classifier.py --rows {a.rows} --labels {a.labels} --batches
{",".join(map(str, a.batches))} --dim {a.dim} --warmup {a.warmup} --repeat {a.repeat}` on
{results[0]["device"]}, commit {commit}.

Tables of {a.rows} rows under {a.labels} labels, {a.dim} numeric features per datum. fused:
`_classify_fused` (batch conversion, device top-k, nn_vote, one copy of [datums, labels]); per
datum: `_classify_each` (query_datum per datum, host lookups and loop), the classify path before
the vote kernel. Both in one process: host clock between two device synchronisations,
{a.warmup} warm-up calls per path and batch size, then {a.repeat} timed calls per path,
alternating. Whole-call times (conversion, top-k, vote, copies), not kernel times; min .. max is
the spread over the {a.repeat} calls.
"""]
        for res in results:
            worst = max(r["max_abs_difference"] for r in res["batches"].values())
            parts.append(f"""## config/classifier/{res["config"]} ({res["method"]}, k = {res["k"]})

{table(res)}

Largest difference between the two paths' scores: {worst:.3g} (float64 host loop against the
fp32 kernel). Filling the table took {res["fill_s"]} s.
""")
        with open(a.out, "w") as f:
            f.write("\n".join(parts))
    return 0


if __name__ == "__main__":
    sys.exit(main())
