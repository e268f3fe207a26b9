"""Micro-benchmark of the similarity scan kernels (1 GPU): full hamming_scan
(distance matrix) vs fused scan + top-k (topk.hip) at various N, k, nq.
``--wide``: lists of 256 to 4096 entries (topk_wide.hip) against scan + torch.topk."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jubatus_amd.ops import hip  # noqa: E402


def timeit(fn, iters=30):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / iters, 2)


def wide(nqs=(1, 8), ks=(256, 1024, 4096), iters=20):
    """k past TOPK_MAX_K (csrc/hip/topk_wide.hip) against the path such a call
    took before: hamming_scan + torch.topk, or torch.topk on the score matrix.
    One JSON line per shape, microseconds per call (median of 5 timed loops).
    ``--wide NQ,NQ.. K,K..`` picks other query and list sizes."""
    d = torch.device("cuda", 0)
    g = torch.Generator(device=d).manual_seed(0)

    def med(fn):
        return sorted(timeit(fn, iters) for _ in range(5))[2]

    for nrows in (1_000_000, 10_000_000):
        tb = torch.randint(-2**62, 2**62, (nrows, 1), device=d, dtype=torch.int64, generator=g)
        tn = torch.rand(nrows, device=d, generator=g) + 0.5
        valid = torch.ones(nrows, dtype=torch.uint8, device=d)
        for nq in nqs:
            qb, qn = tb[:nq].clone(), tn[:nq].clone()
            full = torch.empty((nq, nrows), dtype=torch.float32, device=d)
            sc = torch.rand((nq, nrows), device=d, generator=g)
            for k in ks:
                for name, metric in (("lsh", 0), ("euclid_lsh", 1)):
                    def old():
                        hip.hamming_scan(qb, qn, nq, tb, tn, valid, nrows, 64, metric, full)
                        return torch.topk(full, k, dim=1, largest=False, sorted=True)
                    new = lambda: hip.topk_hamming(qb, qn, nq, tb, tn, valid, nrows, 64, metric, k)  # noqa: E731
                    print(json.dumps({"src": name, "N": nrows, "nq": nq, "k": k, "scan_torch_topk_us": med(old),
                                      "topk_wide_us": med(new)}), flush=True)
                old = lambda: torch.topk((1.0 - sc).nan_to_num(posinf=float("inf")), k, dim=1,  # noqa: E731
                                         largest=False, sorted=True)
                new = lambda: hip.topk_scores(sc, nq, nrows, k, True)  # noqa: E731
                print(json.dumps({"src": "scores", "N": nrows, "nq": nq, "k": k, "torch_topk_us": med(old),
                                  "topk_wide_us": med(new)}), flush=True)


def main():
    if "--wide" in sys.argv[1:]:
        lists = [tuple(int(x) for x in a.split(",")) for a in sys.argv[sys.argv.index("--wide") + 1:]]
        return wide(*lists)
    d = torch.device("cuda", 0)
    g = torch.Generator(device=d).manual_seed(0)
    out = {}
    for nrows in (100_000, 1_000_000, 10_000_000):
        tb = torch.randint(-2**62, 2**62, (nrows, 1), device=d, dtype=torch.int64, generator=g)
        tn = torch.rand(nrows, device=d, generator=g)
        valid = torch.ones(nrows, dtype=torch.uint8, device=d)
        for nq in (1, 8):
            qb = tb[:nq].clone()
            qn = tn[:nq].clone()
            full = torch.empty((nq, nrows), dtype=torch.float32, device=d)
            out[f"scan_full_N{nrows}_q{nq}_us"] = timeit(
                lambda: hip.hamming_scan(qb, qn, nq, tb, tn, valid, nrows, 64, 1, full))
            for k in (1, 10, 100):
                out[f"topk_N{nrows}_q{nq}_k{k}_us"] = timeit(
                    lambda: hip.topk_hamming(qb, qn, nq, tb, tn, valid, nrows, 64, 1, k))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
