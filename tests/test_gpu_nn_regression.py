"""Nearest-neighbour regression on the device: csrc/hip/nn_reduce.hip against
the float64 reduce of tests/test_nn_regression.py on synthetic top-k lists,
and the GPU driver (models/nn_regression.py: device top-k + nn_reduce)
against the brute force and against the unfused path (the GPU engine's
query_datum lists, reduced in float64).

Kernel bound: |out - ref| <= (k + 8) 2^-23 (sum w|t| / sum w): the fp32
summation bound of the two sums for any order (k 2^-24 each, relative to
sum w|t| and sum w), plus a few ulps for exp, 1 - d and the division. out_n
is exact; a list without a kept entry gives out == 0 and out_n == 0.

The driver is compared with the float64 reduce of the fp32 distances that
the same engine's query_datum reports for the same query (the fused path
against the tested unfused path, same bound), and its neighbour set with the
brute force's (k-th and (k+1)-th oracle distances more than 1e-4 relative
apart, asserted by the oracle; lsh uses k = rows).
"""
import json
import os

import numpy as np
import pytest

from helpers import ROOT
from test_nn_regression import (CONVERTER, datum, driver, make_data, oracle, params, reduce64,
                                ref_nn_reduce, scored, check_invariant)

pytestmark = pytest.mark.gpu

NROWS = 1000
NN_CFG = os.path.join(ROOT, "config", "regression", "nn.json")
INT_MAX = 2 ** 31 - 1
EPS = 2.0 ** -23


def dev():
    import torch
    return torch.device("cuda", 0)


def lists(nq, k, seed, lo=0.0, hi=1.5):
    """[nq, k] ascending distances in [lo, hi) and rows in [0, NROWS). By
    query q % 4: 0 nothing padded, 1 a padded tail, 2 all padded, 3 a padded
    tail plus entries whose row is >= NROWS or negative (finite distance)"""
    rng = np.random.default_rng(seed)
    dist = np.sort(rng.uniform(lo, hi, (nq, k)).astype(np.float32), axis=1)
    row = rng.integers(0, NROWS, (nq, k)).astype(np.int32)
    for q in range(nq):
        kind = q % 4
        keep = k if kind == 0 else 0 if kind == 2 else int(rng.integers(0, k + 1))
        dist[q, keep:] = np.inf
        row[q, keep:] = INT_MAX
        if kind == 3 and keep:
            row[q, int(rng.integers(keep))] = NROWS + int(rng.integers(0, 5))
            row[q, int(rng.integers(keep))] = -1 - int(rng.integers(0, 5))
    targets = rng.normal(size=NROWS).astype(np.float32)          # mixed sign
    return dist, row, targets


def launch(dist, row, targets, mode, alpha, nrows=NROWS):
    import torch
    from jubatus_amd.ops import hip
    d = torch.from_numpy(dist).to(dev())
    r = torch.from_numpy(row).to(dev())
    t = torch.from_numpy(targets).to(dev())
    out, n = hip.nn_reduce(d, r, dist.shape[0], dist.shape[1], t, nrows, mode, alpha)
    torch.cuda.synchronize()
    return out, n


def check(dist, row, targets, mode, alpha, tag):
    out, n = launch(dist, row, targets, mode, alpha)
    out, n = out.cpu().numpy(), n.cpu().numpy()
    ref, cnt, scale = ref_nn_reduce(dist, row, targets, NROWS, mode, alpha)
    k = dist.shape[1]
    err = np.abs(out.astype(np.float64) - ref)
    bound = (k + 8) * EPS * scale
    worst = int(np.argmax(err - bound))
    print(f"{tag}: max err {err.max():.3g}; worst query {worst}: err {err[worst]:.3g}, "
          f"bound {bound[worst]:.3g}")
    assert np.array_equal(n, cnt)
    assert np.all(err <= bound)
    assert np.all(out[cnt == 0] == 0)
    return out, ref


@pytest.mark.parametrize("nq", [1, 5, 257])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 128, 200])
def test_kernel_matches_the_float64_reduce(k, nq):
    dist, row, targets = lists(nq, k, 1000 * k + nq)
    for mode, alpha in ((0, 1.0), (1, 0.5), (1, 0.0), (2, 1.0)):
        out, ref = check(dist, row, targets, mode, alpha, f"k={k} nq={nq} mode={mode} alpha={alpha}")
        if nq > 1:
            assert np.abs(ref).max() > 0


def test_shifted_exponent_survives_a_large_alpha_times_distance():
    dist, row, targets = lists(5, 64, 7, lo=100.0, hi=200.0)
    # exp(-50 d) underflows to zero for every entry; the shifted exponent does not
    assert np.all(np.exp(-50.0 * dist[np.isfinite(dist)].astype(np.float64)) == 0)
    out, ref = check(dist, row, targets, 1, 50.0, "alpha d in [5000, 10000]")
    has = np.isfinite(dist).any(axis=1) & (np.abs(ref) > 0)
    assert has.sum() >= 2 and np.all(out[has] != 0)


def test_two_launches_give_the_same_bits():
    import torch
    dist, row, targets = lists(257, 200, 9)
    for mode in (0, 1, 2):
        a, na = launch(dist, row, targets, mode, 0.5)
        b, nb = launch(dist, row, targets, mode, 0.5)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(na, nb)


def test_binding_checks_its_operands():
    import torch
    from jubatus_amd.ops import hip
    dist, row, targets = lists(2, 4, 3)
    d, r, t = (torch.from_numpy(x).to(dev()) for x in (dist, row, targets))
    with pytest.raises(TypeError):
        hip.nn_reduce(d, r.to(torch.int64), 2, 4, t, NROWS, 0, 1.0)
    with pytest.raises(TypeError):
        hip.nn_reduce(d.cpu(), r, 2, 4, t, NROWS, 0, 1.0)
    with pytest.raises(ValueError):
        hip.nn_reduce(d, r, 3, 4, t, NROWS, 0, 1.0)
    with pytest.raises(ValueError):
        hip.nn_reduce(d, r, 2, 4, t, NROWS + 1, 0, 1.0)
    with pytest.raises(ValueError):
        hip.nn_reduce(d, r, 2, 4, t, NROWS, 3, 1.0)
    with pytest.raises(ValueError):
        hip.nn_reduce(d, r, 2, 4, t, NROWS, 1, -1.0)
    out, n = hip.nn_reduce(d, r, 0, 4, t, NROWS, 0, 1.0)
    assert out.numel() == 0 and n.numel() == 0


# ------------------------------------------------------------------ driver
DRIVER_CASES = [("NN", "euclid_lsh", 10, 62), ("NN", "lsh", 300, 62), ("cosine", None, 10, 63),
                ("euclidean", None, 10, 64)]


@pytest.mark.parametrize("weight", ["uniform", "distance"])
@pytest.mark.parametrize("method,inner,k,seed", DRIVER_CASES)
def test_gpu_driver_fused_against_unfused(method, inner, k, seed, weight):
    X, y, Q = make_data(300, 12, seed)
    p = params(method, inner, k, weight, 1.0)
    g = driver(method, p, device=dev())
    assert g.train(scored(X[:150], y[:150])) == 150
    assert g.train(scored(X[150:], y[150:])) == 150
    check_invariant(g)
    assert g.targets.is_cuda and g.get_status()["nn.storage"] == "hbm"
    _, sets = oracle(method, inner, X, y, Q, k, weight, 1.0)
    qs = [datum(q) for q in Q]
    got = g.estimate(qs)
    assert len(got) == 12 and all(isinstance(v, float) for v in got)
    index_of = {f"{g.prefix}-{i}": i for i in range(300)}
    for q, est, want in zip(qs, got, sets):
        nb = g.engine.query_datum(q, k, False)          # the unfused path: [(row id, fp32 distance)]
        assert sorted(index_of[rid] for rid, _ in nb) == want
        ref, scale = reduce64(np.asarray([d for _, d in nb], np.float32),
                              [np.float32(g.row_target[rid]) for rid, _ in nb], g.mode, 1.0)
        bound = (len(nb) + 8) * EPS * scale
        print(f"{method}/{inner} {weight}: fused {est!r} unfused {ref!r} bound {bound:.3g}")
        assert abs(est - ref) <= bound
    # the CPU driver on the same data (its bound: tests/test_nn_regression.py)
    c = driver(method, p)
    c.train(scored(X, y))
    diff = np.abs(np.asarray(got) - np.asarray(c.estimate(qs))).max()
    print(f"{method}/{inner} {weight}: GPU driver - CPU driver {diff:.3g}")
    assert diff <= 2e-4 * np.abs(y).max()


def test_slot_reuse_on_the_gpu():
    g = driver("NN", params("NN", "euclid_lsh", 16, "uniform", unlearner="lru",
                            unlearner_parameter={"max_size": 4}), device=dev())
    X, _, Q = make_data(8, 5, 71)
    g.train(scored(X[:4], [1.0] * 4))
    assert g.estimate([datum(q) for q in Q]) == [1.0] * 5
    g.train(scored(X[4:], [-1.0] * 4))
    assert len(g.row_target) == 4 and g.engine.rows.nslots < 8
    assert g.estimate([datum(q) for q in Q]) == [-1.0] * 5
    check_invariant(g)
    g.clear()
    assert g.estimate([datum(q) for q in Q]) == [0.0] * 5


def test_targets_grow_with_the_engine_and_survive_unpack():
    X, y, Q = make_data(1500, 4, 72)                   # past the first 1024 slots
    p = params("euclidean", None, 5, "distance")
    g = driver("euclidean", p, device=dev())
    g.train(scored(X[:1000], y[:1000]))
    g.train(scored(X[1000:], y[1000:]))
    assert g.targets.numel() >= 1500
    check_invariant(g)
    h = driver("euclidean", p, device=dev())
    h.unpack(g.pack())
    check_invariant(h)
    qs = [datum(q) for q in Q]
    assert h.estimate(qs) == g.estimate(qs)


@pytest.fixture
def gpu_server(tmp_path):
    from jubatus_amd.framework.server_helper import ServerHelper
    from jubatus_amd.framework.server_util import ServerArgv
    from jubatus_amd.server import get_serv
    a = ServerArgv.parse(["-p", "9199", "-b", "127.0.0.1", "-f", NN_CFG, "-d", str(tmp_path),
                          "-c", "4", "--gpu", "0"], "regression")
    a.port = 0
    h = ServerHelper(get_serv("regression"), a, install_signals=False)
    h.start(block=False)
    yield h
    h.stop()


def test_python_gpu_server(gpu_server):
    from jubatus_amd.client import Datum, Regression
    cfg = json.load(open(NN_CFG))
    assert cfg["converter"] == CONVERTER
    X, y, Q = make_data(64, 8, 73)
    with Regression("127.0.0.1", gpu_server.argv.port, "", timeout=60) as c:
        assert c.train([[float(t), Datum(datum(x))] for x, t in zip(X, y)]) == 64
        q = [Datum(datum(x)) for x in Q]
        got = c.estimate(q)
        # k = 128 >= 64 rows, uniform weights: the mean of all targets
        assert np.abs(np.asarray(got) - y.astype(np.float32).astype(np.float64).mean()).max() \
            <= (64 + 8) * EPS * np.abs(y).mean()
        st = list(c.get_status().values())[0]
        assert st["method"] == "NN" and st["nn.storage"] == "hbm" and st["nn.num_rows"] == "64"
        c.save("m")
        assert c.clear() is True
        assert c.estimate(q) == [0.0] * 8
        assert c.load("m") is True
        again = c.estimate(q)
        # the same rows in the same slots: the same lists, the same sums
        assert np.abs(np.asarray(again) - np.asarray(got)).max() <= (64 + 8) * EPS * np.abs(y).mean()

