#!/usr/bin/env python3
"""Throughput of the label-chunked linear kernels (csrc/hip/linear_chunked.hip)
by label capacity: exact mode (one stream) for each waves-per-stream value,
atomic mode with 256 streams, and the batched classify of 64 samples. The
row at LC = 1024 is the LC-templated kernel of linear.hip, for scale.

H = 2^16 rows, 16 features per sample, AROW, uniform random labels and rows
(every sample reads 16 rows of LC * 4 bytes for its scores). Each figure is
the median of --reps timed launches after one warm-up launch, timed with
device events around the launch; train launches start from freshly reset
tables every time (the reset is outside the timed region). The spread table
gives min / max of the same launches. Prints two Markdown tables and one
JSON line.

    python tools/bench_many_labels.py [--reps 5] [--caps 1024,2048,...]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H = 1 << 16
NF = 16
AROW = 5


def _timed(fn, reps, prep=None):
    """-> (median, min, max) seconds of ``reps`` launches after one warm-up;
    prep runs before every launch, outside the timed region"""
    import torch
    out = []
    for i in range(reps + 1):
        if prep is not None:
            prep()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:
            out.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(out), min(out), max(out)


def _stream(n, LC, nstreams, seed, dev):
    import torch
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(a).to(dev)
    rp = t(np.arange(n + 1, dtype=np.int64) * NF)
    fi = t(rng.integers(0, H, n * NF).astype(np.int32))
    fv = t(rng.normal(size=n * NF).astype(np.float32))
    lab = t(rng.integers(0, LC, n).astype(np.int32))
    sp = t((np.arange(nstreams + 1, dtype=np.int64) * (n // nstreams)))
    return rp, fi, fv, lab, sp


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--caps", default="1024,2048,4096,8192,16384")
    ap.add_argument("--exact-samples", type=int, default=2048)
    ap.add_argument("--atomic-streams", type=int, default=256)
    ap.add_argument("--atomic-per-stream", type=int, default=64)
    a = ap.parse_args()
    import torch
    from jubatus_amd.ops import hip
    dev = torch.device("cuda", 0)
    rows = []
    for LC in [int(x) for x in a.caps.split(",")]:
        W = torch.zeros((H, LC), device=dev)
        P = torch.ones((H, LC), device=dev)
        act = torch.ones(LC, dtype=torch.int32, device=dev)
        stats = torch.zeros(2, dtype=torch.int64, device=dev)
        per_sample = NF * LC * 4

        def reset():
            W.zero_()
            P.fill_(1.0)

        def train(rp, fi, fv, lab, sp, ns, mode, waves):
            if LC <= hip.TEMPLATE_MAX_LC:
                hip.linear_train(rp, fi, fv, lab, sp, ns, W, P, act, AROW, 1.0, mode, stats=stats)
            else:
                hip.linear_train_chunked(rp, fi, fv, lab, sp, ns, W, P, act, AROW, 1.0, mode, waves,
                                         stats)
        row = {"LC": LC, "kernel": "template" if LC <= hip.TEMPLATE_MAX_LC else "chunked"}
        n = a.exact_samples
        ex = _stream(n, LC, 1, 1, dev)
        for waves in ((0,) if LC <= hip.TEMPLATE_MAX_LC else (1, 4, 16)):
            s, lo, hi = _timed(lambda: train(*ex, 1, hip.UPDATE_EXACT, waves), a.reps, reset)
            row[f"exact_w{waves}_samples_per_s"] = round(n / s)
            row[f"exact_w{waves}_min_max"] = [round(n / hi), round(n / lo)]
            row[f"exact_w{waves}_read_GBps"] = round(n * per_sample / s / 1e9, 1)
        n = a.atomic_streams * a.atomic_per_stream
        at = _stream(n, LC, a.atomic_streams, 2, dev)
        for waves in ((0,) if LC <= hip.TEMPLATE_MAX_LC else (1, 4, 16)):
            s, lo, hi = _timed(lambda: train(*at, a.atomic_streams, hip.UPDATE_ATOMIC, waves), a.reps,
                               reset)
            row[f"atomic_w{waves}_samples_per_s"] = round(n / s)
            row[f"atomic_w{waves}_min_max"] = [round(n / hi), round(n / lo)]
            row[f"atomic_w{waves}_read_GBps"] = round(n * per_sample / s / 1e9, 1)
        cl = _stream(64, LC, 1, 3, dev)
        out = torch.zeros((64, LC), device=dev)
        s, lo, hi = _timed(lambda: hip.linear_classify(cl[0], cl[1], cl[2], 64, W, out), max(a.reps, 20))
        row["classify64_us"] = round(s * 1e6, 1)
        row["classify64_us_min_max"] = [round(lo * 1e6, 1), round(hi * 1e6, 1)]
        row["classify64_read_GBps"] = round(64 * per_sample / s / 1e9, 1)
        rows.append(row)
        del W, P
        torch.cuda.empty_cache()
    print("| LC | kernel | exact samples/s (waves 1 / 4 / 16) | exact GB/s read | "
          "atomic 256 streams samples/s (1 / 4 / 16) | atomic GB/s read | classify 64 us | classify GB/s |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        ws = (0,) if r["kernel"] == "template" else (1, 4, 16)
        print(f"| {r['LC']} | {r['kernel']} | "
              + " / ".join(str(r[f'exact_w{w}_samples_per_s']) for w in ws) + " | "
              + " / ".join(str(r[f'exact_w{w}_read_GBps']) for w in ws) + " | "
              + " / ".join(str(r[f'atomic_w{w}_samples_per_s']) for w in ws) + " | "
              + " / ".join(str(r[f'atomic_w{w}_read_GBps']) for w in ws) + " | "
              + f"{r['classify64_us']} | {r['classify64_read_GBps']} |")
    print()
    print("| LC | exact samples/s min-max (waves 1 / 4 / 16) | atomic samples/s min-max (1 / 4 / 16) | "
          "classify 64 us min-max |")
    print("|---|---|---|---|")
    for r in rows:
        ws = (0,) if r["kernel"] == "template" else (1, 4, 16)
        mm = lambda k: " / ".join("{}-{}".format(*r[f"{k}_w{w}_min_max"]) for w in ws)
        print(f"| {r['LC']} | {mm('exact')} | {mm('atomic')} | "
              + "{}-{} |".format(*r["classify64_us_min_max"]))
    print(json.dumps({"bench": "many_labels", "H": H, "features": NF, "method": "AROW", "rows": rows}))


if __name__ == "__main__":
    main()
