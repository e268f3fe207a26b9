"""DBSCAN of one coreset-sized point set, the GPU launch chain against the
driver's host path on the same points (models/clustering.py):

* gpu   ops.hip.dbscan: csrc/hip/dbscan.hip (adjacency bitmap on the matrix
        cores, masses, lock-free union, flatten, border) and the read-back of
        the status word; the points are in HBM already
* host  dbscan_host: the same five rules in NumPy float64, what a server
        without a device runs

The points are blobs plus uniform noise with coordinates on a 1/64 grid
inside [-4, 4], so every fp32 distance is exact and the two paths must give
the same labels: that is checked before anything is timed. Each path is
warmed up, then timed with a host clock (the GPU path between two device
synchronisations); medians and the spread are printed as one JSON line and
written as a table to --out.

Usage: python tools/bench_dbscan.py [--n 4096] [--dim 32] [--blobs 8]
       [--noise 0.05] [--eps 2.0] [--min-core-point 20] [--warmup 3]
       [--repeat 20] [--host-repeat 3] [--out profiles/dbscan.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def points(n: int, dim: int, blobs: int, noise: float, seed: int = 0):
    rng = np.random.default_rng(seed)
    m = int(n * noise)
    centers = rng.uniform(-3.0, 3.0, (blobs, dim))
    X = centers[rng.integers(0, blobs, n - m)] + 0.25 * rng.standard_normal((n - m, dim))
    X = np.concatenate([X, rng.uniform(-4.0, 4.0, (m, dim))])
    X = np.clip(np.round(X * 64.0) / 64.0, -4.0, 4.0)
    X = X[rng.permutation(n)]
    w = rng.integers(1, 9, n) * 0.25
    return X.astype(np.float32), w.astype(np.float32)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--blobs", type=int, default=8)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--eps", type=float, default=2.0)
    ap.add_argument("--min-core-point", type=float, default=20.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--host-repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_dbscan: no GPU (a CPU run gives no timing)\n")
        return 2
    from jubatus_amd.models.clustering import dbscan_host
    from jubatus_amd.ops import hip

    X, w = points(a.n, a.dim, a.blobs, a.noise)
    dev = torch.device("cuda", 0)
    Xd, wd = torch.from_numpy(X).to(dev), torch.from_numpy(w).to(dev)

    def gpu():
        return hip.dbscan(Xd, wd, a.eps, a.min_core_point)

    def host():
        return dbscan_host(X, w, a.eps, a.min_core_point)

    label_g = gpu()[0].cpu().numpy().astype(np.int64)
    label_h = host()[0]
    if not (label_g == label_h).all():
        sys.stderr.write(f"bench_dbscan: the paths disagree on {(label_g != label_h).sum()} labels\n")
        return 1
    n_clusters = int(np.unique(label_h[label_h >= 0]).size)
    n_noise = int((label_h < 0).sum())

    for _ in range(a.warmup):
        gpu()
    tg, th = [], []
    for _ in range(a.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gpu()
        torch.cuda.synchronize()
        tg.append((time.perf_counter() - t0) * 1e3)
    for _ in range(a.host_repeat):
        t0 = time.perf_counter()
        host()
        th.append((time.perf_counter() - t0) * 1e3)
    res = {"n": a.n, "dim": a.dim, "blobs": a.blobs, "noise_share": a.noise, "eps": a.eps,
           "min_core_point": a.min_core_point, "clusters": n_clusters, "noise_points": n_noise,
           "labels_agree": True, "repeat": a.repeat, "host_repeat": a.host_repeat,
           "gpu_ms_median": round(statistics.median(tg), 3), "gpu_ms_min": round(min(tg), 3),
           "gpu_ms_max": round(max(tg), 3), "host_ms_median": round(statistics.median(th), 1),
           "host_ms_min": round(min(th), 1), "host_ms_max": round(max(th), 1),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if a.out:
        names = {"gpu": "gpu: `ops.hip.dbscan`, points in HBM, host clock between two device synchronisations",
                 "host": "host: `dbscan_host`, NumPy float64"}
        rows_md = "\n".join(
            f"| {names[p]} | {res[p + '_ms_median']} | {res[p + '_ms_min']} | {res[p + '_ms_max']} | {k} |"
            for p, k in (("gpu", a.repeat), ("host", a.host_repeat)))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"""# DBSCAN: the GPU launch chain against the host path

`python tools/bench_dbscan.py --n {a.n} --dim {a.dim} --blobs {a.blobs} --noise {a.noise} --eps {a.eps}
--min-core-point {a.min_core_point} --warmup {a.warmup} --repeat {a.repeat} --host-repeat {a.host_repeat}`
on {res["device"]}.

Shape: {a.n} points, {a.dim} dims, {a.blobs} blobs (sigma 0.25) plus {a.noise:.0%} uniform noise,
coordinates on a 1/64 grid, weights 0.25 .. 2; eps {a.eps}, min_core_point {a.min_core_point}:
{n_clusters} clusters, {n_noise} noise points. The labels of the two paths agree on every point
(checked before timing). No parent implementation exists, so the host path of the same commit
is the comparison; no threshold is set.

| path | median ms | min ms | max ms | timed calls |
|---|---|---|---|---|
{rows_md}

Whole-call times: the GPU figure includes the norms, the scratch allocations, the six
launches and the read-back of the status word, not the upload of the points. Kernel times
were not measured.
""")
    return 0


if __name__ == "__main__":
    sys.exit(main())
