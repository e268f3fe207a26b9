"""k-means++ kernel timing per call (csrc/hip/clustering.hip through ops/hip.kmeanspp): n points x d dims, m draws.
Usage: python tools/kpp_bench.py (JB_KMEANSPP_WAVE=1 / JB_KMEANSPP_BLOCK=1 for the other kernels)
       python tools/kpp_bench.py --wide [--lloyd]
--wide: A/B of hip.kmeanspp against hip.kmeanspp_wide (csrc/hip/kmeanspp_wide.hip) per call, the two alternating,
over n in {3000, 20000, 100000} x d in {4, 64, 1024} x m in {8, 128, 1024}; a case whose first narrow call runs
past a minute is skipped. A markdown table on stdout, with jb_kmeanspp_wide_pays' answer per shape.
--lloyd: one recluster's seeding (both kernels) against its hip.lloyd_wide, at n 2500, d 128, k 64."""
import os, sys, time, torch, numpy as np
sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", "/root/repo"))
from jubatus_amd.ops import hip
d = torch.device("cuda", 0)
def operands(n, dd, m):
    rng = np.random.default_rng(0)
    X = torch.from_numpy((rng.standard_normal((n, dd)) * 3).astype(np.float32)).to(d)
    w = torch.from_numpy((rng.random(n) + 0.25).astype(np.float32)).to(d)
    return X, w, list(rng.random(m))
def timed(fn, it):
    """us per call by device events (every call ends in a read-back of its picks)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / it
def run(n, dd, m, it=50):
    X, w, u = operands(n, dd, m)
    for _ in range(3): hip.kmeanspp(X, w, u, m)
    torch.cuda.synchronize()
    return timed(lambda: hip.kmeanspp(X, w, u, m), it)
def ab(n, dd, m, est=0.0):
    """(narrow us, wide us) per call: warm-up, then rounds of both, the medians. est: seconds a narrow call is
    expected to take, from the same shape at fewer draws (it is linear in m); None for a case over a minute"""
    if est > 60.0: return None
    X, w, u = operands(n, dd, m)
    t0 = time.perf_counter()
    hip.kmeanspp(X, w, u, m); hip.kmeanspp_wide(X, w, u, m)
    torch.cuda.synchronize()
    once = time.perf_counter() - t0
    it = max(1, min(20, int(0.2 / once)))
    a, b = [], []
    for _ in range(5 if once < 0.2 else 3 if once < 2.0 else 1):
        a.append(timed(lambda: hip.kmeanspp(X, w, u, m), it))
        b.append(timed(lambda: hip.kmeanspp_wide(X, w, u, m), it))
    return float(np.median(a)), float(np.median(b))
if "--wide" in sys.argv:
    print("| n | d | m | kmeanspp us | kmeanspp_wide us | narrow / wide | pays |\n|---|---|---|---|---|---|---|")
    for n in (3000, 20000, 100000):
        for dd in (4, 64, 1024):
            est = 0.0
            for m in (8, 128, 1024):
                r = ab(n, dd, m, est)
                est = est * 8 if r is None else r[0] * 1e-6 * 8    # the next m is 8 or 16 times this one
                cells = "skipped (over a minute) | | " if r is None else f"{r[0]:.1f} | {r[1]:.1f} | {r[0] / r[1]:.2f}"
                print(f"| {n} | {dd} | {m} | {cells} | {int(hip.kmeanspp_wide_pays(n, dd, m))} |", flush=True)
    if "--lloyd" in sys.argv:
        n, dd, k = 2500, 128, 64
        X, w, u = operands(n, dd, k)
        a, b = ab(n, dd, k)
        C0 = X[hip.kmeanspp_wide(X, w, u, k)[0]].contiguous()
        hip.lloyd_wide(X, w, C0.clone(), 100, 1e-6, 1e-5)
        iters = []
        t = timed(lambda: iters.append(hip.lloyd_wide(X, w, C0.clone(), 100, 1e-6, 1e-5)[1]), 10)
        print(f"\nrecluster at n {n}, d {dd}, k {k}: seeding {a:.1f} us (kmeanspp), {b:.1f} us (kmeanspp_wide); "
              f"lloyd_wide {t:.1f} us ({iters[-1]} iterations)", flush=True)
    sys.exit(0)
for n, dd in ((1000, 10), (200, 10), (1000, 1), (1000, 32)):
    for m in (1, 10, 100):
        print(os.environ.get("JB_KMEANSPP_WAVE", "blk"), n, dd, m, round(run(n, dd, m), 1), "us", flush=True)
