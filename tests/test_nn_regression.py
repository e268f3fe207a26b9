"""Nearest-neighbour regression (NN, cosine, euclidean;
models/nn_regression.py) on the host: the driver against a float64 brute force
written here; configuration and argument errors; the unlearner; model files;
MIX; the Python server on the CPU; the native server's configuration check.

The three methods are this project's own (the reference, Jubatus 0.9.2, ships
PA regression only). The brute force below is the oracle; parity with later
Jubatus releases is unpinned.

This module also holds the data, the brute force and the float64 reduce that
tests/test_gpu_nn_regression.py runs against the device.

Oracle: exact cosine / euclid from the raw vectors in float64 for cosine /
euclidean; for NN the signatures of models/similarity.py signature_host and
the distance formulas (hamming fraction; euclid_lsh sqrt(a^2 + b^2 -
2 a b cos(pi fraction))) in float64. The k nearest by (distance, insertion
order), then sum w t / sum w.

Ties at the k-th neighbour make the answer ambiguous, so lsh and minhash
cases use k >= the number of rows, and the cases with k < rows (euclidean,
cosine, NN / euclid_lsh on Gaussian data) assert that the oracle's k-th and
(k+1)-th distances differ by more than 1e-4 relative, for every query; the
seeds were chosen with the oracle alone.

Bound of the driver against the oracle: |estimate - oracle| <= 1e-4 max|t|.
The engines hold fp32 distances: relative error about 1e-6, up to about 1e-5
absolute after the cancellation in |q|^2 + |x|^2 - 2 q.x at these norms (< 5)
and distances (> 0.2). A weight exp(-alpha (d - d_min)) with alpha <= 2 is
then off by at most 4e-5 relative, 1 - d by 1e-5, and the fp32 sums add
k 2^-23; the weighted mean of targets moves by less than 1e-4 of max|t|.
"""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, config_path, start_standalone

REG_BIN = os.path.join(ROOT, "jubatus_amd", "native_bin", "jubaregression")
CONVERTER = json.load(open(config_path("regression/pa.json")))["converter"]
DIM = 6
HASH_NUM = 64
LSH_SEED = 1091              # models/row_engine.py make_index default
TIE_GAP = 1e-4
DRIVER_TOL = 1e-4            # of max|t| (module docstring)


# -------------------------------------------------------------------- data
def make_data(n, nq, seed):
    """n rows and nq queries, N(0,1)^DIM; targets linear + noise, mixed sign"""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, DIM))
    Q = rng.normal(size=(nq, DIM))
    coef = rng.normal(size=DIM)
    y = X @ coef + 0.1 * rng.normal(size=n)
    return X, y, Q


def datum(x):
    return {f"n{j}": float(v) for j, v in enumerate(x)}


def scored(X, y):
    return [[float(t), datum(x)] for x, t in zip(X, y)]


def converter():
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    return DatumToFvConverter(CONVERTER)


def driver(method, parameter, device=None):
    from jubatus_amd.models.nn_regression import NNRegression
    return NNRegression(method, parameter, converter(), device=device)


def params(method, inner, k, weight, alpha=1.0, **extra):
    p = {"nearest_neighbor_num": k, "weight": weight, "local_sensitivity": alpha, **extra}
    if method == "NN":
        p.update({"method": inner, "parameter": {"hash_num": HASH_NUM}})
    return p


# ------------------------------------------------------------------ oracle
def _fv(conv, x):
    from jubatus_amd.fv_converter.datum import as_datum
    idx, val = conv.hashed(conv.convert(as_datum(datum(x))))
    assert len(set(idx)) == DIM          # no hash collision among the DIM features
    return idx, val


def _popcount(a):
    return sum(bin(int(w)).count("1") for w in a)


def distances(method, inner, X, Q):
    """float64 distance matrix [nq, n] in the view the top-k reports"""
    X = np.asarray(X, np.float64)
    Q = np.asarray(Q, np.float64)
    if method == "euclidean":
        return np.sqrt(((Q[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    if method == "cosine":
        den = np.linalg.norm(Q, axis=1)[:, None] * np.linalg.norm(X, axis=1)[None, :]
        return 1.0 - (Q @ X.T) / den
    from jubatus_amd.models.similarity import signature_host
    conv = converter()
    mode = 1 if inner == "minhash" else 0
    sx = [signature_host(*_fv(conv, x), HASH_NUM, LSH_SEED, mode) for x in X]
    sq = [signature_host(*_fv(conv, q), HASH_NUM, LSH_SEED, mode) for q in Q]
    D = np.empty((len(Q), len(X)))
    for i, (qb, qn) in enumerate(sq):
        for j, (xb, xn) in enumerate(sx):
            frac = _popcount(qb ^ xb) / HASH_NUM
            if inner == "euclid_lsh":
                D[i, j] = math.sqrt(max(0.0, qn * qn + xn * xn - 2 * qn * xn * math.cos(math.pi * frac)))
            else:
                D[i, j] = frac
    return D


def weights64(d, mode, alpha):
    d = np.asarray(d, np.float64)
    if mode == 1:
        return np.exp(-float(alpha) * (d - d.min())) if d.size else d
    if mode == 2:
        return np.maximum(0.0, 1.0 - d)
    return np.ones_like(d)


def reduce64(d, t, mode, alpha):
    """float64 weighted mean -> (estimate, sum w|t| / sum w); (0, 0) without
    a neighbour or when sum w == 0"""
    w = weights64(d, mode, alpha)
    t = np.asarray(t, np.float64)
    sw = w.sum()
    if not sw > 0:
        return 0.0, 0.0
    return float((w * t).sum() / sw), float((w * np.abs(t)).sum() / sw)


def ref_nn_reduce(dist, row, targets, nrows, mode, alpha):
    """the float64 oracle of csrc/hip/nn_reduce.hip on [nq, k] lists ->
    (out, out_n, scale): entries with a non-finite d or a row outside
    [0, nrows) are skipped"""
    out, cnt, scale = [], [], []
    for d, r in zip(np.asarray(dist), np.asarray(row)):
        keep = np.isfinite(d) & (r >= 0) & (r < nrows)
        e, s = reduce64(d[keep].astype(np.float64), np.asarray(targets, np.float64)[r[keep]],
                        mode, alpha)
        out.append(e)
        scale.append(s)
        cnt.append(int(keep.sum()))
    return np.asarray(out), np.asarray(cnt), np.asarray(scale)


def oracle(method, inner, X, y, Q, k, weight, alpha, live=None):
    """-> (estimates float64 [nq], neighbour index lists); asserts the tie
    guard when k < rows. ``live``: indices of the rows that exist."""
    live = np.arange(len(X)) if live is None else np.asarray(live)
    D = distances(method, inner, np.asarray(X)[live], Q)
    mode = 0 if weight == "uniform" else (2 if method == "cosine" else 1)
    est, sets = [], []
    for d in D:
        order = np.argsort(d, kind="stable")
        if k < len(d):
            a, b = d[order[k - 1]], d[order[k]]
            assert b - a > TIE_GAP * abs(b), ("tie at the k-th neighbour", a, b)
        nb = order[:k]
        est.append(reduce64(d[nb], np.asarray(y)[live][nb], mode, alpha)[0])
        sets.append(sorted(int(live[j]) for j in nb))
    return np.asarray(est), sets


def check_invariant(drv):
    """targets[slot_of[rid]] == row_target[rid] for every live row"""
    slot_of = drv.engine.rows.slot_of
    assert set(drv.row_target) == set(slot_of)
    t = drv.targets.cpu().numpy() if hasattr(drv.targets, "cpu") else drv.targets
    assert len(t) >= drv.engine.rows.nslots
    for rid, s in slot_of.items():
        assert t[s] == np.float32(drv.row_target[rid]), rid


# (method, inner, k, rows, seed): lsh / minhash with k >= rows, the others k < rows
CASES = [("NN", "lsh", 128, 60, 11), ("NN", "minhash", 128, 60, 12), ("NN", "euclid_lsh", 7, 80, 13),
         ("cosine", None, 7, 80, 14), ("euclidean", None, 7, 80, 15), ("euclidean", None, 1, 80, 16)]


# ------------------------------------------------------------------- tests
@pytest.mark.parametrize("weight,alpha", [("uniform", 1.0), ("distance", 1.0), ("distance", 2.0),
                                          ("distance", 0.0)])
@pytest.mark.parametrize("method,inner,k,n,seed", CASES)
def test_driver_matches_the_brute_force(method, inner, k, n, seed, weight, alpha):
    X, y, Q = make_data(n, 9, seed)
    d = driver(method, params(method, inner, k, weight, alpha))
    assert d.train(scored(X[:n // 2], y[:n // 2])) == n // 2
    assert d.train(scored(X[n // 2:], y[n // 2:])) == n - n // 2
    ref, _ = oracle(method, inner, X, y, Q, k, weight, alpha)
    got = d.estimate([datum(q) for q in Q])
    assert all(isinstance(g, float) for g in got)
    err = np.abs(np.asarray(got) - ref).max()
    print(f"{method}/{inner} k={k} {weight} alpha={alpha}: max |err| {err:.3g}, "
          f"bound {DRIVER_TOL * np.abs(y).max():.3g}")
    assert err <= DRIVER_TOL * np.abs(y).max()
    check_invariant(d)


def test_host_reduce_matches_the_float64_reduce():
    from jubatus_amd.models.nn_regression import reduce_host
    rng = np.random.default_rng(5)
    for k in (1, 7, 64, 200):
        d = np.sort(rng.uniform(0, 1.5, k)).astype(np.float32)
        t = rng.normal(size=k).astype(np.float32)
        for mode, alpha in ((0, 1.0), (1, 0.5), (1, 0.0), (2, 1.0)):
            ref, scale = reduce64(d, t, mode, alpha)
            assert abs(reduce_host(d, t, mode, alpha) - ref) <= (k + 8) * 2.0 ** -23 * scale
    # the shifted exponent: the nearest row weighs 1 however large alpha * d is
    d = np.sort(rng.uniform(100, 200, 32)).astype(np.float32)
    t = rng.normal(size=32).astype(np.float32)
    ref, scale = reduce64(d, t, 1, 50.0)
    got = reduce_host(d, t, 1, 50.0)
    assert got != 0.0 and abs(got - ref) <= 40 * 2.0 ** -23 * scale
    assert reduce_host(np.zeros(0, np.float32), np.zeros(0, np.float32), 1, 1.0) == 0.0
    assert reduce_host(np.asarray([1.5, 2.0], np.float32), np.ones(2, np.float32), 2, 1.0) == 0.0
    assert reduce_host(np.asarray([0.5, np.inf], np.float32), np.asarray([3.0, 9.0], np.float32), 0,
                       1.0) == 3.0


def test_empty_model_and_zero_datums():
    for method, inner in (("NN", "lsh"), ("cosine", None), ("euclidean", None)):
        d = driver(method, params(method, inner, 4, "distance"))
        assert d.estimate([]) == []
        assert d.estimate([datum(np.ones(DIM)), datum(np.zeros(DIM))]) == [0.0, 0.0]
        assert d.train([]) == 0
        X, y, Q = make_data(10, 2, 1)
        d.train(scored(X, y))
        assert d.estimate([]) == []
        d.clear()
        assert d.seq == 0 and d.row_target == {} and d.engine.rows.nslots == 0
        assert d.estimate([datum(q) for q in Q]) == [0.0, 0.0]
        check_invariant(d)


def test_argument_errors():
    from jubatus_amd.common.exceptions import ArgumentError
    d = driver("euclidean", {})
    for bad in ([[1.0]], [["a", datum(np.ones(DIM))]], [[True, datum(np.ones(DIM))]], [1.0],
                [[None, datum(np.ones(DIM))]]):
        with pytest.raises(ArgumentError):
            d.train(bad)
    with pytest.raises(ArgumentError):
        d.train([[1.0, {"x": object()}]])
    assert d.train([[1, datum(np.ones(DIM))]]) == 1       # an int score is a number


def test_configuration_errors():
    from jubatus_amd.models.regression import Regression, RegressionConfigError
    from jubatus_amd.server.regression_serv import build_regression
    for method in ("NN", "cosine", "euclidean"):
        for p, msg in (({"weight": "gaussian"}, "weight"), ({"weight": None}, "weight"),
                       ({"nearest_neighbor_num": 0}, "nearest_neighbor_num"),
                       ({"nearest_neighbor_num": -3}, "nearest_neighbor_num"),
                       ({"nearest_neighbor_num": 2.5}, "nearest_neighbor_num"),
                       ({"local_sensitivity": -0.1}, "local_sensitivity"),
                       ({"unlearner": "fifo"}, "unlearner"),
                       ({"unlearner": "lru"}, "max_size")):
            with pytest.raises(RegressionConfigError, match=msg):
                driver(method, p)
            with pytest.raises(RegressionConfigError, match=msg):
                build_regression({"method": method, "parameter": p, "converter": CONVERTER}, None)
    with pytest.raises(RegressionConfigError, match="nearest neighbor method"):
        driver("NN", {"method": "inverted_index"})
    with pytest.raises(RegressionConfigError, match="hash_num"):
        driver("NN", {"method": "lsh", "parameter": {"hash_num": 0}})
    with pytest.raises(RegressionConfigError, match="unsupported regression method"):
        driver("SVR", {})
    # the linear driver keeps its message, directly and through the server's builder
    with pytest.raises(RegressionConfigError, match="unsupported regression method"):
        Regression("SVR", {}, converter())
    with pytest.raises(RegressionConfigError, match="unsupported regression method"):
        Regression("NN", {}, converter())
    with pytest.raises(RegressionConfigError, match="unsupported regression method"):
        build_regression({"method": "SVR", "converter": CONVERTER}, None)
    d = driver("NN", None)
    assert (d.k, d.weight, d.alpha, d.engine.method) == (128, "uniform", 1.0, "lsh")
    assert driver("cosine", {}).engine.method == "inverted_index"
    assert driver("euclidean", {}).engine.method == "inverted_index_euclid"
    st = driver("NN", params("NN", "euclid_lsh", 5, "distance", 0.5)).get_status()
    assert st["method"] == "NN" and st["nearest_neighbor_num"] == "5" and st["weight"] == "distance"
    assert st["local_sensitivity"] == "0.5" and st["nn.method"] == "euclid_lsh"
    assert type(build_regression({"method": "PA", "converter": CONVERTER}, None)) is Regression


@pytest.mark.parametrize("method,inner,k", [("euclidean", None, 3), ("NN", "lsh", 128)])
def test_unlearner_keeps_the_survivors_targets(method, inner, k):
    X, y, Q = make_data(20, 6, 21)
    d = driver(method, params(method, inner, k, "distance", 1.0, unlearner="lru",
                              unlearner_parameter={"max_size": 8}))
    assert d.train(scored(X[:5], y[:5])) == 5
    assert d.train(scored(X[5:], y[5:])) == 15
    assert len(d.row_target) == 8 and len(d.engine.rows.slot_of) == 8
    check_invariant(d)
    ref, _ = oracle(method, inner, X, y, Q, k, "distance", 1.0, live=range(12, 20))
    got = np.asarray(d.estimate([datum(q) for q in Q]))
    assert np.abs(got - ref).max() <= DRIVER_TOL * np.abs(y).max()


def test_slot_reuse_yields_the_new_target():
    d = driver("euclidean", params("euclidean", None, 128, "uniform", unlearner="lru",
                                   unlearner_parameter={"max_size": 4}))
    X, _, Q = make_data(8, 3, 22)
    d.train(scored(X[:4], [1.0] * 4))
    assert d.estimate([datum(q) for q in Q]) == [1.0] * 3
    d.train(scored(X[4:], [-1.0] * 4))
    assert d.engine.rows.nslots < 8                    # slots were reused
    assert d.estimate([datum(q) for q in Q]) == [-1.0] * 3
    check_invariant(d)


@pytest.mark.parametrize("method,inner,k,seed", [("NN", "euclid_lsh", 5, 31), ("cosine", None, 5, 32),
                                                  ("euclidean", None, 5, 33)])
def test_pack_unpack(method, inner, k, seed):
    import msgpack
    X, y, Q = make_data(40, 6, seed)
    p = params(method, inner, k, "distance")
    a = driver(method, p)
    a.train(scored(X, y))
    obj = a.pack()
    assert set(obj) == {"method", "engine", "row_target", "seq"}
    assert obj["method"] == method and obj["seq"] == 40 and len(obj["row_target"]) == 40
    b = driver(method, p)
    b.unpack(msgpack.unpackb(msgpack.packb(obj), strict_map_key=False))
    qs = [datum(q) for q in Q]
    assert b.estimate(qs) == a.estimate(qs)
    assert b.seq == 40 and b.row_target == a.row_target
    check_invariant(b)
    b.train(scored(X[:1], y[:1]))                       # the sequence goes on: no id is reused
    assert len(b.row_target) == 41
    other = driver("euclidean" if method != "euclidean" else "cosine", {})
    with pytest.raises(ValueError, match="method"):
        other.unpack(obj)
    from jubatus_amd.models.regression import Regression
    with pytest.raises(ValueError, match="method"):
        a.unpack(Regression("PA", {}, converter()).pack())


def test_mix_diffs_leave_both_with_the_union():
    from jubatus_amd.models.nn_regression import NNRegression
    X, y, Q = make_data(60, 6, 41)
    p = params("euclidean", None, 5, "distance")
    a, b = driver("euclidean", p), driver("euclidean", p)
    a.train(scored(X[:25], y[:25]))
    b.train(scored(X[25:], y[25:]))
    da, db = a.get_diff(), b.get_diff()
    assert set(da) == {"rows", "targets"} and set(da["targets"]) == set(a.row_target)
    mixed = NNRegression.mix_diff(da, db)
    assert a.put_diff(mixed) is True and b.put_diff(mixed) is True
    assert set(a.row_target) == set(b.row_target) and len(a.row_target) == 60
    check_invariant(a)
    check_invariant(b)
    ref, _ = oracle("euclidean", None, X, y, Q, 5, "distance", 1.0)
    qs = [datum(q) for q in Q]
    for drv in (a, b):
        assert np.abs(np.asarray(drv.estimate(qs)) - ref).max() <= DRIVER_TOL * np.abs(y).max()
    assert a.get_diff()["rows"]["rows"] == {}           # nothing changed since the MIX
    # a removed row loses its target everywhere
    gone = f"{a.prefix}-0"
    a.engine.clear_row(gone)
    mixed = NNRegression.mix_diff(a.get_diff(), b.get_diff())
    assert gone in mixed["rows"]["removed"]
    a.put_diff(mixed)
    b.put_diff(mixed)
    assert gone not in a.row_target and gone not in b.row_target and len(b.row_target) == 59
    check_invariant(a)
    check_invariant(b)
    ref, _ = oracle("euclidean", None, X, y, Q, 5, "distance", 1.0, live=range(1, 60))
    assert np.abs(np.asarray(b.estimate(qs)) - ref).max() <= DRIVER_TOL * np.abs(y).max()


@pytest.mark.parametrize("method,inner,k", [("NN", "euclid_lsh", 5), ("cosine", None, 5),
                                            ("euclidean", None, 5)])
def test_python_server_cpu(tmp_path, method, inner, k):
    from jubatus_amd.client import Datum, Regression
    from jubatus_amd.cmd.jubadump import dump
    X, y, Q = make_data(50, 8, 51)
    p = params(method, inner, k, "distance")
    cfg = json.dumps({"method": method, "parameter": p, "converter": CONVERTER})
    h = start_standalone("regression", cfg, tmp_path)
    try:
        ref, _ = oracle(method, inner, X, y, Q, k, "distance", 1.0)
        with Regression("127.0.0.1", h.argv.port, "") as c:
            assert c.train([[float(t), Datum(datum(x))] for x, t in zip(X, y)]) == 50
            q = [Datum(datum(x)) for x in Q]
            got = c.estimate(q)
            assert np.abs(np.asarray(got) - ref).max() <= DRIVER_TOL * np.abs(y).max()
            assert any(abs(g) > 0.1 for g in got)
            st = list(c.get_status().values())[0]
            assert st["method"] == method and st["weight"] == "distance" and st["nn.num_rows"] == "50"
            assert c.estimate([]) == []
            c.save("m")
            assert c.clear() is True
            assert c.estimate(q) == [0.0] * 8
            assert c.load("m") is True
            assert c.estimate(q) == got
        (model,) = [f for f in os.listdir(tmp_path) if f.endswith(".jubatus")]
        body = dump(os.path.join(tmp_path, model))["model"]
        assert body["method"] == method and len(body["row_target"]) == 50 and body["seq"] == 50
    finally:
        h.stop()


@pytest.mark.parametrize("name,method", [("nn", "NN"), ("cosine", "cosine"), ("euclidean", "euclidean")])
def test_configs_and_native_check(name, method):
    path = config_path(f"regression/{name}.json")
    cfg = json.load(open(path))
    assert cfg["method"] == method and cfg["converter"] == CONVERTER
    if name == "nn":
        clf = json.load(open(config_path("classifier/nn.json")))["parameter"]
        assert cfg["parameter"]["method"] == clf["method"]
        assert cfg["parameter"]["parameter"] == clf["parameter"]
    from jubatus_amd.server.regression_serv import build_regression
    assert build_regression(cfg, None).method == method
    # the native server hands these methods to the Python server before any GPU call
    r = subprocess.run([REG_BIN, "--native-check", "-f", path], capture_output=True, text=True,
                       timeout=30)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("python:"), r.stdout
