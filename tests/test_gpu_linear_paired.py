"""Paired-lane atomic update of the linear train kernels (csrc/hip/linear.hip
step 3 / step 5, jb_linear.hpp general_sample and addw_pair): lanes 2j / 2j+1
carry the y / lstar elements of feature j. Everything is compared with the
host oracle (LinearClassifier(device=None)) at the bars of test_gpu_linear.py;
the data uses noise string values so that most samples update."""
import random

import msgpack
import numpy as np
import pytest

from jubatus_amd.fv_converter.converter import DatumToFvConverter

pytestmark = pytest.mark.gpu

# one slot per key: a sample's width is its key count
CONV1 = {
    "string_rules": [{"key": "*", "type": "str", "sample_weight": "bin", "global_weight": "bin"}],
    "num_rules": [{"key": "*", "type": "num"}],
    "hash_max_size": 1 << 18,
}
# two rules per key: the rule a key does not match leaves an invalid (-1) slot
CONV2 = {
    "string_rules": [{"key": "*", "type": "str", "sample_weight": "bin", "global_weight": "bin"},
                     {"key": "s1*", "type": "str", "sample_weight": "log_tf", "global_weight": "bin"}],
    "num_rules": [{"key": "*", "type": "num"}, {"key": "*1", "type": "log"}],
    "hash_max_size": 1 << 18,
}
# staged-window edges (32 features, 16 at capacity 64) and the direct path
WIDTHS = [1, 2, 15, 16, 17, 31, 32, 33, 45]


def _device():
    import torch
    return torch.device("cuda", 0)


def _pair(method, conv, param=None, **kw):
    """(GPU model forced to the atomic kernel without the hot-row replica, host oracle)"""
    from jubatus_amd.models.classifier import LinearClassifier
    from jubatus_amd.ops import hip

    param = param or {"regularization_weight": 0.5}
    g = LinearClassifier(method, param, DatumToFvConverter(conv), device=_device(),
                         concurrent_update="atomic", **kw)
    c = LinearClassifier(method, param, DatumToFvConverter(conv), device=None)
    g._mode = lambda n: hip.UPDATE_MODES["atomic"]
    g.hot_rows = False
    return g, c


def _assert_tables(g, c):
    g.synchronize()
    g.pipe.check_errors()
    scale = float(np.abs(c.W).max()) or 1.0
    np.testing.assert_allclose(g.W.float().cpu().numpy()[:, :c.LC], c.W, rtol=2e-3, atol=2e-3 * scale)
    if c.P is not None:
        np.testing.assert_allclose(g.P.cpu().numpy()[:, :c.LC], c.P, rtol=2e-3,
                                   atol=2e-3 * float(c.P.max()))


def _noise(rng):
    return f"z{rng.getrandbits(40)}"


def _width_stream(n, nlabels, seed, prefix=""):
    """key 0 is a numeric key every sample carries (a shared row, forwarded
    from sample to sample); the others are string keys with noise values,
    some from a small vocabulary so that rows recur"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        y = rng.randrange(nlabels)
        w = rng.choice(WIDTHS)
        d = {f"{prefix}n0": (y - nlabels / 2) * 0.3 + rng.gauss(0.0, 1.0)}
        for j in range(1, w):
            d[f"{prefix}k{j}"] = _noise(rng) if rng.random() < 0.7 else f"v{(y + j) % 5}"
        out.append((f"L{y}", d))
    return out


@pytest.mark.parametrize("method", ["PA1", "CW", "AROW", "NHERD"])
@pytest.mark.parametrize("nlabels", [1, 2, 12, 20, 40])
def test_paired_atomic_stream_matches_oracle(nlabels, method):
    """one atomic stream over every sample width and label capacities 8, 16,
    32 and 64; one label: never a wrong label, every odd lane off"""
    g, c = _pair(method, CONV1)
    data = _width_stream(200, nlabels, seed=100 + nlabels)
    for i in range(0, len(data), 100):
        g.train(data[i:i + 100])
        c.train(data[i:i + 100])
    assert g.LC == {1: 8, 2: 8, 12: 16, 20: 32, 40: 64}[nlabels]
    _assert_tables(g, c)
    assert g.train_stats()["updated"] == c.train_stats()["updated"] > 80


def test_paired_atomic_repeated_key_and_invalid_slots():
    """a numeric key repeated inside the datum (both increments of its row
    land, each with the gathered confidence) and rules that leave -1 slots"""
    rng = random.Random(9)
    data = []
    for _ in range(200):
        y = rng.randrange(4)
        sv = [[f"s{j}", _noise(rng) if rng.random() < 0.7 else f"v{y}"] for j in range(4)]
        nv = [[f"n{j}", (y - 2) * 0.3 + rng.gauss(0, 1)] for j in range(3)] + [["bias", 1.0]]
        nv.append(["n0", 0.5 + rng.random()])
        data.append((f"L{y}", [sv, nv, []]))
    g, c = _pair("AROW", CONV2, {"regularization_weight": 1.0})
    idx, _ = c.conv.hashed(c.conv.convert(data[0][1]))
    assert len(set(idx)) < len(idx)                 # the repeated row
    g.train(data)
    c.train(data)
    _assert_tables(g, c)
    # the repeated row's precision grew by both increments of every update
    r = max(set(idx), key=idx.count)
    assert float(c.P[r].max()) > 1.0
    assert g.train_stats()["updated"] == c.train_stats()["updated"] > 80


def test_paired_atomic_concurrent_streams_on_disjoint_rows():
    """eight concurrent streams (two blocks of four waves) whose key names
    carry the stream number: no two streams share a row, so the lock-free
    result is the oracle's on the concatenation"""
    from jubatus_amd.fv_converter.datum import Datum

    conv = dict(CONV1, hash_max_size=1 << 22)
    g, c = _pair("AROW", conv)
    streams = []
    for q in range(8):
        rng = random.Random(4100 + q)
        items = []
        for _ in range(20):
            y = rng.randrange(3)
            w = rng.choice([2, 5, 9, 33])
            d = {f"q{q}_n0": (y - 1) * 0.3 + rng.gauss(0.0, 1.0)}
            for j in range(1, w):
                d[f"q{q}_k{j}"] = _noise(rng) if rng.random() < 0.7 else f"v{(y + j) % 5}"
            items.append((f"L{y}", d))
        streams.append(items)
    rows = [set() for _ in streams]
    for q, items in enumerate(streams):
        for _, d in items:
            rows[q].update(c.conv.hashed(c.conv.convert(d))[0])
    for a in range(8):
        for b in range(a + 1, 8):
            assert not (rows[a] & rows[b]), (a, b)
    bodies = [msgpack.packb([[l, Datum(d).to_msgpack()] for l, d in items], use_bin_type=False)
              for items in streams]
    assert g.train_requests(bodies) == 160
    for items in streams:
        c.train(items)
    _assert_tables(g, c)
    assert g.train_stats()["updated"] == c.train_stats()["updated"]


def _vocab_stream(n, nlabels, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        y = rng.randrange(nlabels)
        w = rng.choice([3, 16, 33, 40])
        out.append((f"L{y}", {f"k{j}": f"v{rng.randrange(6)}" for j in range(w)}))
    return out


@pytest.mark.parametrize("nlabels", [2, 5])
def test_paired_atomic_bf16_perceptron_is_exact(nlabels):
    """bf16 table, one atomic stream, perceptron on bin features: every
    increment is +-1 and the weights are small integers, so stochastic
    rounding is exact and the table equals the fp32 oracle's. Two labels:
    y and lstar are the two halves of one word in every update (one
    compare-and-swap for both)."""
    g, c = _pair("perceptron", CONV1, {}, weight_dtype="bf16")
    assert g.W.dtype.itemsize == 2
    data = _vocab_stream(180, nlabels, seed=30 + nlabels)
    g.train(data)
    c.train(data)
    g.synchronize()
    g.pipe.check_errors()
    assert g.train_stats()["updated"] == c.train_stats()["updated"] > 50
    assert float(np.abs(c.W).max()) <= 128.0        # integers bf16 holds exactly
    assert np.array_equal(g.W.float().cpu().numpy()[:, :c.LC], c.W)


def test_paired_atomic_bf16_arow_two_labels_tracks_oracle():
    """AROW over a bf16 table with two labels (both halves of a word in one
    compare-and-swap, real-valued steps): the weight distance to the fp32
    oracle stays under the exact-mode bar of test_gpu_bf16.py"""
    g, c = _pair("AROW", CONV1, {"regularization_weight": 1.0}, weight_dtype="bf16")
    data = _width_stream(200, 2, seed=77)
    g.train(data)
    c.train(data)
    g.synchronize()
    g.pipe.check_errors()
    Wg = g.W.float().cpu().numpy()[:, :c.LC]
    rel = float(np.linalg.norm(Wg - c.W) / np.linalg.norm(c.W))
    print(f"bf16 AROW atomic, 2 labels: rel W diff {rel:.4f}")
    assert rel <= 0.3, rel
    assert g.train_stats()["trained"] == len(data)
