"""Exact sparse index, time of one InvertedIndex.query_device call on the GPU
(host preparation, scan, top-k), two paths over the same row pool
(models/similarity.py):

* 8-query   JUBATUS_POOL_WIDE=0: the batch cut into groups of 8, each
            normalised, staged and scanned by csrc/hip/sparse_pool.hip
* wide      JUBATUS_POOL_WIDE=1: the pass planner, up to 64 queries per pass
            on csrc/hip/sparse_pool_wide.hip

Two data shapes: "shared" (every row and query holds the same --dim numeric
features, as config/classifier/cosine.json makes of numeric datums) and
"distinct" (60 features per row drawn from 100000, so the queries of a pass
share few). Per table size, shape and batch size both paths are warmed up,
then timed --repeat times with a host clock between two device
synchronisations, alternating; the medians and the spread are printed as one
JSON line per table and written as tables to --out (a generated file of its
own: profiles/pool_wide_scan.md, which reads the tables, is written by hand).

Usage: python tools/bench_pool_wide.py [--rows 100000,1000000]
       [--batches 9,16,32,64,256] [--dim 16] [--k 16] [--warmup 3]
       [--repeat 15] [--commit ID] [--out profiles/pool_wide_scan_tables.md]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_nn_classifier import commit_id, stats, timed  # noqa: E402

SHAPES = ("shared", "distinct")


def make_csr(shape, n, dim, rng):
    """host CSR of n rows of the shape -> (row_ptr, idx, val)"""
    width = dim if shape == "shared" else 60
    if shape == "shared":
        idx = np.tile(np.arange(dim, dtype=np.int64) * 7919 + 13, n)
    else:
        idx = rng.integers(0, 100000, n * width).astype(np.int64)
    return (np.arange(n + 1, dtype=np.int64) * width, idx,
            rng.normal(size=n * width).astype(np.float32))


def run(shape, rows, a, dev):
    import torch
    from jubatus_amd.models.similarity import InvertedIndex
    rng = np.random.default_rng(0)
    ix = InvertedIndex(False, dev)
    for b0 in range(0, rows, 100000):
        n = min(100000, rows - b0)
        ix.set_rows_csr(np.arange(b0, b0 + n, dtype=np.int64), *make_csr(shape, n, a.dim, rng))
    torch.cuda.synchronize()
    res = {"shape": shape, "rows": rows, "k": a.k, "repeat": a.repeat, "warmup": a.warmup, "batches": {}}
    for nq in a.batches:
        rp, idx, val = make_csr(shape, nq, a.dim, rng)
        qs = [(idx[rp[i]:rp[i + 1]], val[rp[i]:rp[i + 1]]) for i in range(nq)]

        def call(knob):
            os.environ["JUBATUS_POOL_WIDE"] = knob
            return ix.query_device(qs, rows, a.k)
        d0, d1 = call("0")[0], call("1")[0]
        diff = float((d0 - d1).abs().max())
        t0, t1 = [], []
        for knob in ("0", "1"):
            timed(lambda: call(knob), a.warmup, 0)
        for _ in range(a.repeat):                 # alternate: both see the same machine
            t0 += timed(lambda: call("0"), 0, 1)
            t1 += timed(lambda: call("1"), 0, 1)
        res["batches"][str(nq)] = {"narrow_ms": stats(t0), "wide_ms": stats(t1), "max_abs_difference": diff}
    os.environ.pop("JUBATUS_POOL_WIDE", None)
    return res


def table(res):
    lines = ["| queries | 8-query median ms | 8-query min .. max | wide median ms | wide min .. max | "
             "8-query / wide |", "|---|---|---|---|---|---|"]
    for nq, r in res["batches"].items():
        n, w = r["narrow_ms"], r["wide_ms"]
        lines.append(f"| {nq} | {n['median']} | {n['min']} .. {n['max']} | {w['median']} | "
                     f"{w['min']} .. {w['max']} | {n['median'] / w['median']:.2f} |")
    return "\n".join(lines)


def main() -> int:
    ints = lambda s: [int(x) for x in s.split(",")]         # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=ints, default=[100000, 1000000])
    ap.add_argument("--batches", type=ints, default=[9, 16, 32, 64, 256])
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=15)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_pool_wide: no GPU (a CPU run gives no timing)\n")
        return 2
    dev = torch.device("cuda", 0)
    commit = a.commit or commit_id()
    parts = [f"""# Exact sparse index: one query_device call, 8-query passes against the wide scan

`python tools/bench_pool_wide.py --rows {",".join(map(str, a.rows))} --batches
{",".join(map(str, a.batches))} --dim {a.dim} --k {a.k} --warmup {a.warmup} --repeat {a.repeat}` on
{torch.cuda.get_device_name(0)}, commit {commit}.

Cosine index, k = {a.k}. 8-query: `JUBATUS_POOL_WIDE=0`, the path of the parent commit; wide:
`JUBATUS_POOL_WIDE=1`, the pass planner on sparse_pool_wide.hip. Both in one process: host clock
between two device synchronisations, {a.warmup} warm-up calls per path and batch size, then
{a.repeat} timed calls per path, alternating. Whole-call times (normalisation, H2D, scan, top-k),
not kernel times; min .. max is the spread over the {a.repeat} calls.
"""]
    for rows in a.rows:
        for shape in SHAPES:
            res = run(shape, rows, a, dev)
            res["commit"] = commit
            print(json.dumps(res), flush=True)
            worst = max(r["max_abs_difference"] for r in res["batches"].values())
            width = f"{a.dim} shared" if shape == "shared" else "60 mostly distinct"
            parts.append(f"## {rows} rows, {width} features per row and query\n\n{table(res)}\n\n"
                         f"Largest difference between the two paths' distances: {worst:.3g}.\n")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(parts))
    return 0


if __name__ == "__main__":
    sys.exit(main())
