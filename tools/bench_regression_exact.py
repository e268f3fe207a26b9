"""Regression training of a batch of requests, time of one launch on the GPU,
three paths over the same input (100 requests of 1000 samples by default):

* ordered  jb_regression_train_ordered (csrc/hip/regression_ordered.hip): the
           requests back to back, applied in order by one workgroup from LDS
           windows; the serial-equivalent result
* single   jb_regression_train_m with one stream over the same concatenated
           input: what serial order costs without the ordered entry
* atomic   jb_regression_train_m with one concurrent stream per request: the
           default of a batch of requests, not serial-equivalent

Shapes: 16 slots and 130 slots a sample on random rows of H = 2^20, and 16
slots a sample all on the same 16 rows (numeric datums share their rows).
Values N(0,1)/sqrt(width), targets w_true.x + noise, sensitivity 0.1, C = 1.0.
Protocol of docs/PERFORMANCE.md "Regression kernels, one stream": the tables
are reset before every launch, one untimed launch first, device events around
the launch, median of --repeat launches with min .. max. One JSON line is
printed and a table is written to --out.

Usage: python tools/bench_regression_exact.py [--samples 100000]
       [--requests 100] [--methods PA,AROW] [--repeat 5]
       [--out profiles/regression_exact.md]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

H = 1 << 20
SHAPES = (("16 slots, random rows", 16, None), ("130 slots, random rows", 130, None),
          ("16 slots, the same 16 rows", 16, 16))
PATHS = ("ordered", "single", "atomic")


def make_input(n, width, pool, seed):
    """-> host CSR arrays and the initial w"""
    rng = np.random.default_rng(seed)
    if pool is None:
        fidx = rng.integers(0, H, size=(n, width), dtype=np.int64).astype(np.int32)
    else:
        fidx = np.tile(np.arange(pool, dtype=np.int32), (n, 1))
    fval = (rng.standard_normal((n, width)) / np.sqrt(width)).astype(np.float32)
    used = np.unique(fidx)
    wt = np.zeros(H)
    wt[used] = rng.standard_normal(len(used))
    w0 = np.zeros(H, np.float32)
    w0[used] = (wt[used] + 0.12 * rng.standard_normal(len(used))).astype(np.float32)
    y = ((fval.astype(np.float64) * wt[fidx]).sum(1) + 0.12 * rng.standard_normal(n)).astype(np.float32)
    row_ptr = np.arange(0, (n + 1) * width, width, dtype=np.int64)
    return row_ptr, fidx.reshape(-1), fval.reshape(-1), y, w0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--requests", type=int, default=100)
    ap.add_argument("--methods", default="PA,AROW")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_regression_exact: no GPU (a CPU run gives no timing)\n")
        return 2
    from jubatus_amd.models.linear_oracle import METHOD_IDS, USES_COVARIANCE
    from jubatus_amd.ops import hip

    dev = torch.device("cuda", 0)
    n, R = a.samples, a.requests
    sp_req = torch.from_numpy(np.linspace(0, n, R + 1).astype(np.int64)).to(dev)
    sp_one = torch.tensor([0, n], dtype=torch.int64, device=dev)
    res = {"samples": n, "requests": R, "repeat": a.repeat, "device": torch.cuda.get_device_name(0), "ms": {}}
    lines = []
    for method in a.methods.split(","):
        cov = METHOD_IDS[method] in USES_COVARIANCE
        for k, (shape, width, pool) in enumerate(SHAPES):
            row_ptr, fidx, fval, y, w0 = (torch.from_numpy(x).to(dev) for x in make_input(n, width, pool, 10 + k))
            W, P, stats = torch.empty_like(w0), torch.empty_like(w0), torch.empty(3, device=dev)
            scratch = torch.empty_like(fval) if cov else None
            status = torch.zeros(2, dtype=torch.int32, device=dev)

            def launch(path):
                W.copy_(w0)
                P.fill_(1.0)
                stats.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if path == "ordered":
                    hip.regression_train_ordered(row_ptr, fidx, fval, y, n, W, stats, 1.0, 0.1, method=method,
                                                 P=P if cov else None, slot_scratch=scratch, status=status)
                else:
                    conc = path == "atomic"
                    hip.regression_train(row_ptr, fidx, fval, y, sp_req if conc else sp_one, R if conc else 1, W,
                                         stats, 1.0, 0.1, concurrent=conc, method=method, P=P if cov else None,
                                         slot_scratch=scratch)
                e1.record()
                e1.synchronize()
                if path == "ordered":
                    hip.regression_ordered_check(status)
                return e0.elapsed_time(e1)

            row, tabs = {}, {}
            for path in PATHS:
                launch(path)                                   # untimed
                ts = [launch(path) for _ in range(a.repeat)]
                row[path] = [round(statistics.median(ts), 2), round(min(ts), 2), round(max(ts), 2)]
                tabs[path] = W.clone()
            # the ordered entry and the single stream compute the same thing
            scale = float(tabs["single"].abs().max())
            row["ordered_vs_single_max_dw"] = float((tabs["ordered"] - tabs["single"]).abs().max()) / scale
            res["ms"][f"{method} / {shape}"] = row
            lines.append(f"| {method} | {shape} | " + " | ".join(
                "%.2f (%.2f .. %.2f)" % tuple(row[p]) for p in PATHS) +
                " | %.2f | %.1e |" % (row["single"][0] / row["ordered"][0], row["ordered_vs_single_max_dw"]))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"""# Regression: serial-equivalent training of a batch of requests

`python tools/bench_regression_exact.py --samples {n} --requests {R} --methods {a.methods}
--repeat {a.repeat}` on {res["device"]}.

{n} samples as {R} requests, H = 2^20 rows, values N(0,1)/sqrt(width), sensitivity 0.1, C = 1.0.
The tables are reset before every launch; one untimed launch, then device events around each of
{a.repeat} launches: median (min .. max), in ms. `ordered` is `jb_regression_train_ordered`
(one workgroup, LDS windows of 4096 slots), `single` is `jb_regression_train_m` with one stream
over the same concatenated input (serial order without the ordered entry), `atomic` is
`jb_regression_train_m` with one concurrent stream per request (not serial-equivalent). The last
columns: single / ordered (medians), and the largest difference between the W of the ordered and
of the single-stream launch over max|W|.

| method | shape | ordered | single | atomic | single / ordered | max dW |
|---|---|---|---|---|---|---|
""" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
