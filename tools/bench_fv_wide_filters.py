"""Train throughput of a wide-rule config with a num filter through the Python
GPU driver: config/classifier/arow_combinational_feature.json (every pair of
features multiplied) with the numbers normalised first by a
gaussian_normalization filter, key `*`. Each sample has two string and two num
values: 2 + 2 + 2 derived = 6 base features and 15 pairs.

Where the wide rule set serves num filters the config converts on the device
(fv_path gpu-wide, csrc/hip/fv_wide.hip); in a tree before that change the
same run goes through the per-datum Python converter, so running this file
against both trees (--root) compares the two on the same stream. One JSON
line: the path taken and samples/s over --seconds after a warm-up batch.

--no-filter runs the config without the filter (the device wide path in either
tree: what the filter-free path costs before and after).

Usage: python tools/bench_fv_wide_filters.py [--batch 4096] [--seconds 4]
       [--no-filter] [--root DIR_OF_ANOTHER_CHECKOUT]
"""
import argparse
import json
import os
import random
import sys
import time

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def converter(filtered=True):
    with open(os.path.join(HERE, "config", "classifier", "arow_combinational_feature.json")) as f:
        conv = json.load(f)["converter"]
    conv["hash_max_size"] = 1 << 18
    if not filtered:
        return conv
    conv["num_filter_types"] = {"g": {"method": "gaussian_normalization", "average": 0.5,
                                      "standard_deviation": 2.0}}
    conv["num_filter_rules"] = [{"key": "*", "type": "g", "suffix": "_g"}]
    return conv


def stream(n, seed):
    r = random.Random(seed)
    out = []
    for _ in range(n):
        y = r.randrange(3)
        out.append((f"L{y}", {"a": f"w{y}{r.randrange(4)}x", "b": f"v{r.randrange(9)}",
                              "x": y + r.gauss(0, 0.3), "z": r.gauss(0, 1)}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--no-filter", action="store_true",
                    help="the config as it is in config/: the wide path in either tree")
    ap.add_argument("--root", default=HERE, help="the checkout whose jubatus_amd package runs")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.models.classifier import LinearClassifier
    m = LinearClassifier("AROW", {"regularization_weight": 1.0}, DatumToFvConverter(converter(not a.no_filter)),
                         device=torch.device("cuda", 0))
    chunks = [stream(a.batch, seed=s) for s in range(4)]
    m.train(chunks[0])
    m.synchronize()
    done, k, t0 = 0, 0, time.perf_counter()
    while time.perf_counter() - t0 < a.seconds:
        done += m.train(chunks[k % len(chunks)])
        k += 1
    m.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"root": os.path.abspath(a.root), "filter": not a.no_filter,
                      "fv_path": m.get_status()["fv_path"],
                      "batch": a.batch, "batches": k, "samples_per_s": round(done / dt, 1)}))


if __name__ == "__main__":
    main()
