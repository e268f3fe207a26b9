"""The regression methods besides PA (PA1, PA2, perceptron, CW, AROW, NHERD):
models/regression.py train_one (the host oracle and the --cpu backend) against
a float64 sequential reference written here, independent of
models/regression.py; configuration errors; model files; the Python server on
the CPU; the native server's configuration check.

The rules are this project's own (the reference, Jubatus 0.9.2, ships PA
regression only): the classifier's formulas with one label, no rival label
and 1 - margin replaced by loss. The float64 reference below is the oracle;
parity with later Jubatus releases is unpinned.

This module also holds the reference and the sample streams that
tests/test_gpu_regression_methods.py runs on the device. Inputs as in
tests/test_gpu_regression.py: H = 512, values N(0,1)/sqrt(width), targets
w_true.x + noise, initial w = w_true + 0.12 N(0,1), sensitivity 0.1.

Bounds: W at rtol 1e-3, atol 1e-4 * max|W_ref| (the project's regression
bound); statistics at rtol 1e-4; P at rtol 1e-4.

Perceptron, AROW and NHERD are discontinuous at loss = 0 (the step, or the P
increment, jumps there), so every stream's seed is chosen such that the
float64 reference's min |loss| over all samples is at least 1e-4 (about 300
times the fp32 deviation below), for every C the tests use; check_guard
asserts it on the reference. CW is continuous and needs no guard. The seeds
were searched with the reference alone.

Measured on the host with train_one (NumPy fp32) against the float64
reference, max|dW| / max|W_ref| (bound 1e-4), max relative P deviation (bound
1e-4) and max relative statistics deviation (bound 1e-4), over the six
methods and C = 1.0 / 0.05 (perceptron: rate 1.0 / 0.05):
    widths          W 3.7e-7, P 1.2e-5 (NHERD at C = 1, where P reaches 85)
    boundary        W 4.9e-7, P 8.8e-7
    skipped slots   W 3.0e-7, P 1.1e-6
    repeated index  W 4.2e-7, P 7.6e-7
    row reuse       W 2.7e-7, P 7.8e-7
(the host statistics are float64 and equal the reference's; the device's
fp32 sums are bounded by the statistics bound)
"""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, config_path, start_standalone
from test_gpu_regression import H, WIDTHS, Stream, _model, _slots, _targets

REG_BIN = os.path.join(ROOT, "jubatus_amd", "native_bin", "jubaregression")
METHODS = ["PA1", "PA2", "perceptron", "CW", "AROW", "NHERD"]
COV = ("CW", "AROW", "NHERD")
GUARDED = ("perceptron", "AROW", "NHERD")
C_VALUES = [1.0, 0.05]
EPS = 0.1
MIN_LOSS = 1e-4


# --------------------------------------------------------------- reference
def ref_train(method, w, P, stats, st, C, eps):
    """the rules of models/regression.py's docstring in float64, one sample
    after the other, on the fp32-rounded inputs; w, P (float64[H]) and stats
    (float64[3]) in place. -> (updating samples, min |loss| over all samples)"""
    C = float(np.float32(C))
    eps = float(np.float32(eps))
    updates, min_loss = 0, math.inf
    for s in range(st.n):
        a, b = int(st.row_ptr[s]), int(st.row_ptr[s + 1])
        idx = st.fidx[a:b].astype(np.int64)
        x = st.fval[a:b].astype(np.float64)
        keep = idx >= 0
        idx, x = idx[keep], x[keep]
        dot = float(np.dot(x, w[idx]))          # a repeated index: once per occurrence
        nrm = float(np.dot(x, x))
        S = 1.0 / P[idx]                        # the pre-sample variances, per occurrence
        v = float(np.dot(x * x, S))
        y = float(st.targets[s])
        stats += (y, y * y, 1.0)
        avg = stats[0] / stats[2]
        sd = math.sqrt(max(0.0, stats[1] / stats[2] - avg * avg))
        err = y - dot
        sgn = 1.0 if err > 0 else -1.0
        loss = sgn * err - eps * sd
        min_loss = min(min_loss, abs(loss))
        if method == "CW":
            if not v > 0:
                continue
            m, phi = -loss, C
            bb = 1.0 + 2.0 * phi * m
            gamma = (-bb + math.sqrt(max(0.0, bb * bb - 8.0 * phi * (m - phi * v)))) / (4.0 * phi * v)
            if not gamma > 0:
                continue
            np.add.at(w, idx, sgn * gamma * S * x)
            np.add.at(P, idx, 2.0 * gamma * phi * x * x)
            updates += 1
            continue
        if not (loss > 0 and nrm > 0):
            continue
        updates += 1
        if method in ("PA1", "PA2", "perceptron"):
            tau = {"PA1": min(C, loss / nrm), "PA2": loss / (nrm + 1.0 / (2.0 * C)), "perceptron": C}[method]
            np.add.at(w, idx, sgn * tau * x)
            continue
        if method == "AROW":
            beta = 1.0 / (v + 1.0 / C)
            alpha = loss * beta
        else:
            assert method == "NHERD"
            alpha = loss / (v + 1.0 / C)
            beta = (C * C * v + 2.0 * C) / (1.0 + C * v) ** 2
        np.add.at(w, idx, sgn * alpha * S * x)
        np.add.at(P, idx, beta * x * x / (1.0 - beta * S * x * x))
    return updates, min_loss


_REF_CACHE = {}


def reference(key, st, w0, method, C, eps=EPS, stats0=None):
    """-> (w, P, stats, updates, min |loss|); computed once per key and shared
    (the callers do not modify it)"""
    k = (key, method, C, eps)
    if k not in _REF_CACHE:
        w = w0.astype(np.float64)
        P = np.ones(len(w0))
        stats = np.zeros(3) if stats0 is None else stats0.astype(np.float64)
        upd, ml = ref_train(method, w, P, stats, st, C, eps)
        _REF_CACHE[k] = (w, P, stats, upd, ml)
    return _REF_CACHE[k]


def check_guard(method, st, updates, min_loss):
    """the stream exercises the rule (a fifth of the samples update, at
    least) and stays clear of the discontinuity at loss = 0"""
    assert 5 * updates >= st.n, (updates, st.n)
    if method in GUARDED:
        assert min_loss >= MIN_LOSS, min_loss


def assert_tables(got_w, got_P, got_s, w_ref, P_ref, stats_ref, cov):
    scale = float(np.abs(w_ref).max())
    print("max|dW|/max|W_ref| = %.3g, max rel P = %.3g, max rel stats = %.3g"
          % (np.abs(got_w - w_ref).max() / scale, np.abs(got_P / P_ref - 1.0).max() if cov else 0.0,
             np.abs(got_s / stats_ref - 1.0).max()))
    np.testing.assert_allclose(got_w, w_ref, rtol=1e-3, atol=1e-4 * scale)
    np.testing.assert_allclose(got_s, stats_ref, rtol=1e-4)
    if cov:
        np.testing.assert_allclose(got_P, P_ref, rtol=1e-4)


# ------------------------------------------------------------------ inputs
# seeds: see the module docstring (min |loss| >= 1e-4 on the float64 reference)
SEEDS = {"widths": 4, "boundary": 1, "skipped": 2, "repeated": 1, "row_reuse": 3}


def case_widths():
    rng = np.random.default_rng(SEEDS["widths"])
    wt, w0 = _model(rng, H)
    samples = [_slots(rng, WIDTHS[s % len(WIDTHS)], H) for s in range(400)]
    return Stream(samples, _targets(rng, samples, wt)), w0


BOUNDARY_WIDTHS = [255, 256, 257, 300, 600]


def case_boundary():
    """around the 256 slots the kernel keeps in registers; 600 slots over 512
    rows repeat indices freely"""
    rng = np.random.default_rng(SEEDS["boundary"])
    wt, w0 = _model(rng, H)
    samples = [_slots(rng, BOUNDARY_WIDTHS[s % 5], H, distinct=BOUNDARY_WIDTHS[s % 5] <= H) for s in range(100)]
    return Stream(samples, _targets(rng, samples, wt)), w0


def case_skipped():
    """idx = -1 slots carrying large values: one in chunk 0 of every sample;
    samples of 65+ slots also at slot 64 and at their last slot"""
    rng = np.random.default_rng(SEEDS["skipped"])
    wt, w0 = _model(rng, H)
    samples = []
    for s in range(120):
        width = [2, 5, 65, 100, 130, 300][s % 6]
        idx, val = _slots(rng, width, H)
        skip = [int(rng.integers(0, min(width, 64)))]
        if width >= 65:
            skip += [64, width - 1]
        idx[skip] = -1
        val[skip] = 3.0
        samples.append((idx, val))
    return Stream(samples, _targets(rng, samples, wt)), w0


REPEATED_WIDTHS = [2, 5, 65, 130, 200, 257, 300, 600]


def case_repeated():
    """the last slot repeats the first slot's index (widths 2, 5: both in
    chunk 0; the others: in different chunks, from 257 on past the register
    slots); the two slots carry 0.7 and -0.5 whatever the width, so a P
    re-read after the sample's own add shows in P (2e-3 .. 5.5e-3 relative at
    C = 1.0 against a bound of 1e-4)"""
    rng = np.random.default_rng(SEEDS["repeated"])
    wt, w0 = _model(rng, H)
    samples = []
    for s in range(160):
        width = REPEATED_WIDTHS[s % 8]
        idx, val = _slots(rng, width, H, distinct=width <= H)
        idx[-1] = idx[0]
        val[0], val[-1] = 0.7, -0.5
        samples.append((idx, val))
    return Stream(samples, _targets(rng, samples, wt)), w0


def case_row_reuse():
    """back-to-back samples on the same 8 rows"""
    rng = np.random.default_rng(SEEDS["row_reuse"])
    wt, w0 = _model(rng, 8)
    samples = [_slots(rng, 5, 8) for _ in range(200)]
    return Stream(samples, _targets(rng, samples, wt)), w0


CASES = {"widths": case_widths, "boundary": case_boundary, "skipped": case_skipped,
         "repeated": case_repeated, "row_reuse": case_row_reuse}
_CASE_CACHE = {}


def case(name):
    if name not in _CASE_CACHE:
        _CASE_CACHE[name] = CASES[name]()
    return _CASE_CACHE[name]


def host_train(method, st, w0, C, eps=EPS):
    """models/regression.py train_one over the stream -> (w, P, stats)"""
    from jubatus_amd.models.regression import train_one
    w = w0.copy()
    P = np.ones(len(w0), np.float32) if method in COV else None
    stats = np.zeros(3, np.float64)
    for s in range(st.n):
        a, b = int(st.row_ptr[s]), int(st.row_ptr[s + 1])
        train_one(w, stats, st.fidx[a:b], st.fval[a:b], float(st.targets[s]), C, eps, method=method, P=P)
    return w, P, stats


# ------------------------------------------------------------------- tests
@pytest.mark.parametrize("C", C_VALUES)
@pytest.mark.parametrize("name", ["widths", "repeated"])
@pytest.mark.parametrize("method", METHODS)
def test_train_one_matches_float64_reference(method, name, C):
    st, w0 = case(name)
    w_ref, P_ref, stats_ref, upd, ml = reference(name, st, w0, method, C)
    check_guard(method, st, upd, ml)
    w, P, stats = host_train(method, st, w0, C)
    assert_tables(w, P, stats, w_ref, P_ref, stats_ref, method in COV)


def test_train_one_default_is_pa():
    """the positional call of before: PA"""
    from jubatus_amd.models.regression import train_one
    st, w0 = case("row_reuse")
    a, b = w0.copy(), w0.copy()
    sa, sb = np.zeros(3), np.zeros(3)
    for s in range(20):
        i, j = int(st.row_ptr[s]), int(st.row_ptr[s + 1])
        train_one(a, sa, st.fidx[i:j], st.fval[i:j], float(st.targets[s]), 0.05, 0.1)
        train_one(b, sb, st.fidx[i:j], st.fval[i:j], float(st.targets[s]), 0.05, 0.1, method="PA")
    assert np.array_equal(a, b) and np.array_equal(sa, sb) and not np.array_equal(a, w0)


CONV = {"num_rules": [{"key": "*", "type": "num"}], "hash_max_size": 1024}


def _driver(method, parameter, device=None):
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.models.regression import Regression
    return Regression(method, parameter, DatumToFvConverter(CONV), device)


def test_config_errors():
    from jubatus_amd.models.regression import PARegression, Regression, RegressionConfigError
    assert PARegression is Regression
    with pytest.raises(RegressionConfigError, match="unsupported regression method"):
        _driver("SVR", {})
    for m in COV:
        with pytest.raises(RegressionConfigError, match="regularization_weight"):
            _driver(m, {"sensitivity": 0.1})
        with pytest.raises(RegressionConfigError, match="regularization_weight"):
            _driver(m, {"regularization_weight": 0.0})
    for lr in (0.0, -1.0):
        with pytest.raises(RegressionConfigError, match="learning_rate"):
            _driver("perceptron", {"learning_rate": lr})
    for m in ["PA"] + METHODS:
        with pytest.raises(RegressionConfigError, match="sensitivity"):
            _driver(m, {"sensitivity": -0.5, "regularization_weight": 1.0})
    d = _driver("perceptron", {})
    assert d.C == 1.0 and d.eps == 0.1 and d.P is None
    assert _driver("PA2", None).C == pytest.approx(3.40282e38)
    for m in ["PA"] + METHODS:
        assert _driver(m, {"regularization_weight": 1.0}).get_status()["method"] == m


def _data(n, seed=3):
    import random
    rng = random.Random(seed)
    coef = [rng.gauss(0, 1) for _ in range(6)]
    out = []
    for _ in range(n):
        xs = [rng.gauss(0, 1) for _ in range(6)]
        out.append([sum(c * x for c, x in zip(coef, xs)) + rng.gauss(0, 0.1),
                    [[], [[f"n{j}", x] for j, x in enumerate(xs)], []]])
    return out


def test_pack_unpack():
    data = _data(80)
    a = _driver("AROW", {"regularization_weight": 1.0})
    a.train(data)
    assert np.any(a.P != 1) and np.any(a.w != 0)
    obj = a.pack()
    assert set(obj) == {"method", "H", "rows", "w", "stats", "weights", "P"}
    rows = np.frombuffer(obj["rows"], np.int64)
    assert np.array_equal(rows, np.flatnonzero((a.w != 0) | (a.P != 1)))
    assert len(obj["P"]) == 4 * len(rows)
    b = _driver("AROW", {"regularization_weight": 1.0})
    b.unpack(obj)
    assert np.array_equal(a.P, b.P) and np.array_equal(a.w, b.w)
    q = [d for _, d in data[:10]]
    assert a.estimate(q) == b.estimate(q)
    # an absent "P": the initial precision
    del obj["P"]
    b.unpack(obj)
    assert np.all(b.P == 1) and np.array_equal(a.w, b.w)
    # PA writes exactly the keys it wrote before P existed
    p = _driver("PA", {"regularization_weight": 1.0})
    p.train(data)
    pobj = p.pack()
    assert list(pobj) == ["method", "H", "rows", "w", "stats", "weights"]
    assert np.array_equal(np.frombuffer(pobj["rows"], np.int64), np.flatnonzero(p.w))
    for m in ("PA1", "PA2", "perceptron"):
        assert list(_driver(m, {}).pack()) == list(pobj)
    with pytest.raises(ValueError, match="method"):
        a.unpack(pobj)
    with pytest.raises(ValueError, match="method"):
        p.unpack(a.pack())


def test_mix_tables_include_precision():
    a = _driver("NHERD", {"regularization_weight": 1.0})
    ts = a._tables()
    assert len(ts) == 3 and ts[1].data_ptr() == a.P.ctypes.data
    assert len(_driver("PA1", {})._tables()) == 2


def test_python_server_cpu_arow(tmp_path):
    from jubatus_amd.client import Datum, Regression
    cfg = json.load(open(config_path("regression/arow.json")))
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.models.regression import Regression as Driver
    h = start_standalone("regression", config_path("regression/arow.json"), tmp_path)
    try:
        ora = Driver(cfg["method"], cfg["parameter"], DatumToFvConverter(cfg["converter"]))
        data = _data(60)
        with Regression("127.0.0.1", h.argv.port, "") as c:
            assert c.train([[s, Datum(dict(d[1]))] for s, d in data]) == len(data)
            ora.train(data)
            q = [Datum(dict(d[1])) for _, d in data[:10]]
            got = c.estimate(q)
            np.testing.assert_allclose(got, ora.estimate([d for _, d in data[:10]]), rtol=1e-6, atol=1e-6)
            assert any(abs(g) > 0.1 for g in got)
            assert list(c.get_status().values())[0]["method"] == "AROW"
            c.save("m")
            assert c.clear() is True
            assert c.estimate(q) == [0.0] * 10
            assert c.load("m") is True
            assert c.estimate(q) == got
    finally:
        h.stop()


def _check(cfg_file):
    r = subprocess.run([REG_BIN, "--native-check", "-f", cfg_file], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip()


@pytest.mark.parametrize("name", ["pa1", "pa2", "perceptron", "cw", "arow", "nherd"])
def test_native_check_accepts_the_new_configs(name):
    assert _check(config_path(f"regression/{name}.json")) == "native"
    cfg = json.load(open(config_path(f"regression/{name}.json")))
    assert cfg["converter"] == json.load(open(config_path("regression/pa.json")))["converter"]


def test_native_check_parameter_errors(tmp_path):
    p = tmp_path / "r.json"
    conv = {"num_rules": [{"key": "*", "type": "num"}]}
    for m in COV:
        p.write_text(json.dumps({"method": m, "parameter": {"sensitivity": 0.1}, "converter": conv}))
        assert "regularization_weight" in _check(str(p))
        p.write_text(json.dumps({"method": m, "converter": conv}))
        assert "regularization_weight" in _check(str(p))
    p.write_text(json.dumps({"method": "perceptron", "parameter": {"learning_rate": 0}, "converter": conv}))
    assert "learning_rate" in _check(str(p))
    p.write_text(json.dumps({"method": "SVR", "converter": conv}))
    out = _check(str(p))
    assert "is not PA" in out and "NHERD" in out
