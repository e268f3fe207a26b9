"""GMM EM, time of 50 iterations on the GPU, the paths of models/clustering.py
_em against each other on the same seeded inputs:

* wide    ops/hip.py gmm_em_wide (csrc/hip/gmm_wide.hip: a launch chain per
          iteration over the whole GPU, the M-step sums on the matrix cores)
* torch   the torch loop of _em (what a shape past one workgroup's LDS ran
          before the wide kernels: [n, k, d] materialised every iteration)
* fused   ops/hip.py gmm_em (csrc/hip/clustering.hip gmm_em_kernel, one
          workgroup), where the shape fits it

Two shapes: k 64, d 128, n 10 000 (past the one-workgroup limit: wide against
torch) and k 5, d 17, n 1000 (fits both kernels: fused against wide). Each
path is warmed up, then timed --repeat times with a host clock between two
device synchronisations, the paths alternating; medians and spread go to
stdout as one JSON line per shape and as a table to --out.

Usage: python tools/bench_gmm_em.py [--iters 50] [--warmup 3] [--repeat 15]
       [--commit ID] [--out profiles/gmm_em_wide.md]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_nn_classifier import commit_id, stats, timed  # noqa: E402

SHAPES = ((10000, 64, 128, ("wide", "torch")), (1000, 5, 17, ("fused", "wide")))


def run(n, k, d, paths, a, dev):
    import torch
    from jubatus_amd.models.clustering import Clustering
    from jubatus_amd.ops import hip
    g = torch.Generator().manual_seed(n + k + d)
    centers = torch.randn(k, d, generator=g) * 6
    X = (centers[torch.arange(n) % k] + torch.randn(n, d, generator=g)).to(dev)
    w = (torch.rand(n, generator=g) + 0.5).to(dev)
    C0 = X[:k].clone()
    out = {}

    def kernel(fn):
        def call():
            C, var = C0.clone(), torch.ones(k, d, device=dev)
            pi = torch.full((k,), 1.0 / k, device=dev)
            assign = torch.empty(n, dtype=torch.int32, device=dev)
            if not fn(X, w, C, var, pi, a.iters, assign):
                raise RuntimeError(f"{fn.__name__} declined n {n} k {k} d {d}")
            out[fn.__name__] = (C, var, pi)
        return call

    def torch_loop():
        # _em's loop as it runs when both kernels decline (a host engine's code on device tensors)
        eng = Clustering.__new__(Clustering)
        real = hip.gmm_em, hip.gmm_em_wide
        hip.gmm_em = hip.gmm_em_wide = lambda *args: False
        try:
            out["torch"] = eng._em(X, w, C0.clone(), a.iters)
        finally:
            hip.gmm_em, hip.gmm_em_wide = real

    fns = {"wide": kernel(hip.gmm_em_wide), "fused": kernel(hip.gmm_em), "torch": torch_loop}
    for p in paths:
        timed(fns[p], a.warmup, 0)
    ts = {p: [] for p in paths}
    for _ in range(a.repeat):      # alternate the paths, so that both see the same machine
        for p in paths:
            ts[p] += timed(fns[p], 0, 1)
    keys = {"wide": "gmm_em_wide", "fused": "gmm_em", "torch": "torch"}
    ra, rb = out[keys[paths[0]]], out[keys[paths[1]]]
    diff = max(float((x - y).abs().max()) for x, y in zip(ra, rb))
    return {"n": n, "k": k, "d": d, "iters": a.iters, "paths": list(paths),
            "ms": {p: stats(ts[p]) for p in paths}, "max_abs_difference": diff}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=15)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.stderr.write("bench_gmm_em: no GPU (a CPU run gives no timing)\n")
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
        lines = [f"""# GMM EM: {a.iters} iterations, the paths of `Clustering._em` against each other

`python tools/bench_gmm_em.py --iters {a.iters} --warmup {a.warmup} --repeat {a.repeat}` on {device},
commit {commit}.

wide: `hip.gmm_em_wide` (csrc/hip/gmm_wide.hip); fused: `hip.gmm_em` (one workgroup,
csrc/hip/clustering.hip); torch: the torch loop of `_em`, which is what a shape past the
one-workgroup limit ran before the wide kernels (the loop's code is unchanged by them). One
process: host clock between two device synchronisations, {a.warmup} warm-up calls per path, then
{a.repeat} timed calls per path, alternating. Whole-call times of {a.iters} iterations plus the
final assignment (the kernels) or without it (the torch loop, which assigns in a later call);
min .. max is the spread over the {a.repeat} calls.

| n | k | d | path | median ms | min .. max | first / second |
|---|---|---|---|---|---|---|"""]
        for r in results:
            p0, p1 = r["paths"]
            for p in (p0, p1):
                m = r["ms"][p]
                ratio = f"{r['ms'][p0]['median'] / r['ms'][p1]['median']:.2f}" if p == p0 else ""
                lines.append(f"| {r['n']} | {r['k']} | {r['d']} | {p} | {m['median']} | {m['min']} .. {m['max']} | "
                             f"{ratio} |")
        lines.append("")
        for r in results:
            lines.append(f"n {r['n']}, k {r['k']}, d {r['d']}: largest difference between the two paths' C, var "
                         f"and pi: {r['max_abs_difference']:.3g}.")
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
