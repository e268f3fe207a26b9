"""Lloyd to convergence on the GPU (100 iterations at most, allclose 1e-6 /
1e-5: what models/clustering.py _recluster asks for), the paths of
_recluster against each other on the same seeded inputs:

* wide    ops/hip.py lloyd_wide (csrc/hip/kmeans_wide.hip: two launches an
          iteration over the whole GPU, scores and update sums on the matrix
          cores)
* torch   the torch loop of _recluster (what a shape past one workgroup's LDS
          ran before the wide kernels: sqdist, argmin, two index_add_, where
          and an allclose with a host synchronisation every iteration)
* fused   ops/hip.py lloyd (csrc/hip/clustering.hip lloyd_kernel, one
          workgroup), where the shape fits it

Three shapes: k 64, d 128, n 10 000 and k 512, d 64, n 20 000 (past the
one-workgroup limit: wide against torch) and k 5, d 17, n 1000 (fits both
kernels: fused against wide). Each path is warmed up, then timed --repeat
times with a host clock between two device synchronisations, the paths
alternating; medians and spread go to stdout as one JSON line per shape and
as a table to --out.

Usage: python tools/bench_lloyd.py [--spread 1.0] [--warmup 3] [--repeat 15]
       [--commit ID] [--out profiles/lloyd_wide.md]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_nn_classifier import commit_id, stats, timed  # noqa: E402

SHAPES = ((10000, 64, 128, ("wide", "torch")), (20000, 512, 64, ("wide", "torch")), (1000, 5, 17, ("fused", "wide")))
ITERS, ATOL, RTOL = 100, 1e-6, 1e-5


def run(n, k, d, paths, a, dev):
    import torch
    from jubatus_amd.ops import hip
    g = torch.Generator().manual_seed(n + k + d)
    centers = torch.randn(k, d, generator=g) * a.spread
    X = (centers[torch.arange(n) % k] + torch.randn(n, d, generator=g)).to(dev)
    w = (torch.rand(n, generator=g) + 0.5).to(dev)
    C0 = X[:k].clone()
    out, iters = {}, {}

    def kernel(fn, name):
        def call():
            C = C0.clone()
            res = fn(X, w, C, ITERS, ATOL, RTOL)
            if res is None:
                raise RuntimeError(f"{fn.__name__} declined n {n} k {k} d {d}")
            out[name] = C
            iters[name] = res[1] if name == "wide" else None   # (lloyd_kernel leaves `iters` there)
        return call

    def torch_loop():
        # _recluster's loop as it runs when both kernels decline
        C, done = C0.clone(), 0
        for _ in range(ITERS):
            am = hip.sqdist(X, C).argmin(1)
            wsum = torch.zeros(k, dtype=torch.float32, device=dev).index_add_(0, am, w)
            S = torch.zeros_like(C).index_add_(0, am, X * w[:, None])
            newC = torch.where(wsum[:, None] > 0, S / wsum.clamp_min(1e-12)[:, None], C)
            stop = bool(torch.allclose(newC, C, atol=ATOL))
            C, done = newC, done + 1
            if stop:
                break
        out["torch"], iters["torch"] = C, done

    fns = {"wide": kernel(hip.lloyd_wide, "wide"), "fused": kernel(hip.lloyd, "fused"), "torch": torch_loop}
    for p in paths:
        timed(fns[p], a.warmup, 0)
    ts = {p: [] for p in paths}
    for _ in range(a.repeat):      # alternate the paths, so that both see the same machine
        for p in paths:
            ts[p] += timed(fns[p], 0, 1)
    diff = float((out[paths[0]] - out[paths[1]]).abs().max())
    return {"n": n, "k": k, "d": d, "paths": list(paths), "ms": {p: stats(ts[p]) for p in paths},
            "iterations": {p: iters[p] for p in paths}, "max_abs_difference": diff}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--spread", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=15)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_lloyd: no GPU (a CPU run gives no timing)\n")
        return 2
    dev = torch.device("cuda", 0)
    commit = a.commit or commit_id()
    device = torch.cuda.get_device_name(0)
    results = []
    for n, k, d, paths in SHAPES:
        res = run(n, k, d, paths, a, dev)
        res.update(commit=commit, device=device)
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        lines = [f"""# Lloyd to convergence: the paths of `Clustering._recluster` against each other

`python tools/bench_lloyd.py --spread {a.spread} --warmup {a.warmup} --repeat {a.repeat}` on {device},
commit {commit}.

wide: `hip.lloyd_wide` (csrc/hip/kmeans_wide.hip); fused: `hip.lloyd` (one workgroup,
csrc/hip/clustering.hip); torch: the torch loop of `_recluster`, which is what a shape past the
one-workgroup limit ran before the wide kernels (the loop's code is unchanged by them). Inputs:
k centres times {a.spread} plus unit noise, weights in [0.5, 1.5], C0 the first k points; at most
{ITERS} iterations, allclose {ATOL} / {RTOL}. One process: host clock between two device
synchronisations, {a.warmup} warm-up calls per path, then {a.repeat} timed calls per path,
alternating. Whole-call times to convergence, with the final assignment (the kernels) or without
it (the torch loop, which assigns in a later call); min .. max is the spread over the {a.repeat}
calls. Iterations: the update iterations a path ran (the one-workgroup kernel does not report
them).

| n | k | d | path | iterations | median ms | min .. max | first / second |
|---|---|---|---|---|---|---|---|"""]
        for r in results:
            p0, p1 = r["paths"]
            for p in (p0, p1):
                m = r["ms"][p]
                ratio = f"{r['ms'][p0]['median'] / r['ms'][p1]['median']:.2f}" if p == p0 else ""
                its = r["iterations"][p] if r["iterations"][p] is not None else "-"
                lines.append(f"| {r['n']} | {r['k']} | {r['d']} | {p} | {its} | {m['median']} | "
                             f"{m['min']} .. {m['max']} | {ratio} |")
        lines.append("")
        for r in results:
            lines.append(f"n {r['n']}, k {r['k']}, d {r['d']}: largest difference between the two paths' C: "
                         f"{r['max_abs_difference']:.3g}.")
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
