"""csrc/hip/regression.hip, the methods besides PA (jb_regression_train_m: PA1,
PA2, perceptron, CW, AROW, NHERD) against the float64 sequential reference of
tests/test_regression_methods.py (independent of models/regression.py), the
Python driver and the native server against the host oracle, and the native
MIX of the precision table.

The rules are this project's own (the reference ships PA regression only);
see tests/test_regression_methods.py for the inputs, the bounds (W rtol 1e-3,
atol 1e-4 * max|W_ref|; statistics rtol 1e-4; P rtol 1e-4), the guard against
the discontinuity at loss = 0 and the fp32 emulation's deviation on the
streams shared with it. The streams of this file alone, same emulation
(train_one in NumPy fp32 against float64, every method, the C of the test):
    disjoint, 2 / 5 / 9 streams   W at most 3.8e-7, P at most 7.3e-7
Every exact-mode and disjoint-stream case compares W, P and the statistics;
P is the table that shows a P read after the sample's own add (the repeated
stream: 2e-3 .. 5.5e-3 relative at C = 1.0), a w step without S, a missing
drain and a last-wins store.
"""
import json
import os
import random
import subprocess
import time

import numpy as np
import pytest

from helpers import ROOT, config_path
from test_gpu_regression import STATS0, Stream, _driver_data, _model, _slots, _targets, H
from test_regression_methods import (C_VALUES, COV, EPS, METHODS, assert_tables, case, check_guard,
                                     ref_train, reference)

pytestmark = pytest.mark.gpu

NB = os.path.join(ROOT, "jubatus_amd", "native_bin")


def dev():
    import torch
    return torch.device("cuda", 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def gpu_train(method, st, W, P, stats, C, eps, stream_ptr=None, concurrent=False):
    import torch
    from jubatus_amd.ops import hip
    assert st.fidx.size == 0 or (int(st.fidx.max()) < W.numel() and int(st.row_ptr[-1]) == st.fidx.size)
    sp = np.asarray([0, st.n], np.int64) if stream_ptr is None else stream_ptr
    assert int(sp[-1]) == st.n and np.all(np.diff(sp) >= 0)
    fval = _t(st.fval)
    scratch = torch.empty_like(fval) if method in COV else None
    hip.regression_train(_t(st.row_ptr), _t(st.fidx), fval, _t(st.targets), _t(sp), len(sp) - 1,
                         W, stats, C, eps, concurrent=concurrent, method=method,
                         P=P if method in COV else None, slot_scratch=scratch)


def tables(w0, stats0=None):
    import torch
    W = _t(w0)
    P = torch.ones_like(W)
    stats = torch.zeros(3, dtype=torch.float32, device=dev()) if stats0 is None else _t(stats0)
    return W, P, stats


def assert_device(method, W, P, stats, w_ref, P_ref, stats_ref):
    got_P = P.cpu().numpy()
    if method not in COV:
        assert np.all(got_P == 1.0)             # the kernel leaves a table it does not use alone
    assert_tables(W.cpu().numpy(), got_P, stats.cpu().numpy(), w_ref, P_ref, stats_ref, method in COV)


# -------------------------------------------------------------- exact mode
@pytest.mark.parametrize("C", C_VALUES)
@pytest.mark.parametrize("name", ["widths", "boundary", "skipped", "repeated", "row_reuse"])
@pytest.mark.parametrize("method", METHODS)
def test_exact_stream_matches_float64_reference(method, name, C):
    """widths 1 .. 200, the register boundary (255 .. 600 slots), skipped
    slots, an index repeated across chunks with fixed values, back-to-back
    row reuse (the exact-mode drain of w and P)"""
    st, w0 = case(name)
    w_ref, P_ref, stats_ref, upd, ml = reference(name, st, w0, method, C)
    check_guard(method, st, upd, ml)
    W, P, stats = tables(w0)
    gpu_train(method, st, W, P, stats, C, EPS)
    assert_device(method, W, P, stats, w_ref, P_ref, stats_ref)


@pytest.mark.parametrize("method", METHODS)
def test_tables_and_statistics_carry_over_launches(method):
    """the widths stream in three launches == the one-launch reference"""
    st, w0 = case("widths")
    w_ref, P_ref, stats_ref, _, _ = reference("widths", st, w0, method, 1.0)
    W, P, stats = tables(w0)
    for a, b in ((0, 70), (70, 201), (201, st.n)):
        gpu_train(method, st.part(a, b), W, P, stats, 1.0, EPS)
    assert_device(method, W, P, stats, w_ref, P_ref, stats_ref)


# --------------------------------------------------------- concurrent mode
EMPTY_STREAMS = {2: (), 5: (2, 4), 9: (4, 8)}
DISJOINT_SEEDS = {2: 1, 5: 1, 9: 1}


def case_disjoint(nstreams):
    """stream k draws from rows [k * H // nstreams, (k + 1) * H // nstreams);
    unequal lengths, empty streams (a middle one and the last one), widths 3 /
    64 / 65 / 130 / 300, every third sample repeats its first index in its
    last slot, and samples wider than the slice repeat indices freely.
    -> (stream, stream_ptr, initial w)"""
    rng = np.random.default_rng(100 * DISJOINT_SEEDS[nstreams] + nstreams)
    wt, w0 = _model(rng, H, delta=0.04)
    samples, sp = [], [0]
    for k in range(nstreams):
        pool = np.arange(k * H // nstreams, (k + 1) * H // nstreams)
        n = 0 if k in EMPTY_STREAMS[nstreams] else 9 + 7 * ((3 * k) % 5) + k
        for j in range(n):
            width = [3, 64, 65, 130, 300][(j + k) % 5]
            idx, val = _slots(rng, width, pool, distinct=width <= len(pool))
            if j % 3 == 0:
                idx[-1] = idx[0]
            samples.append((idx, val))
        sp.append(len(samples))
    return Stream(samples, _targets(rng, samples, wt, noise=0.04)), np.asarray(sp, np.int64), w0


_DISJOINT = {}


@pytest.mark.parametrize("nstreams", sorted(EMPTY_STREAMS))
@pytest.mark.parametrize("method", METHODS)
def test_concurrent_disjoint_streams_match_sequential_reference(method, nstreams):
    """streams on disjoint rows with sensitivity 0 do not interact, so the
    tables are every stream's own sequential result (the float64 reference
    over the streams one after the other is exactly that) and the statistics
    take every sample once"""
    if nstreams not in _DISJOINT:
        _DISJOINT[nstreams] = case_disjoint(nstreams)
    st, sp, w0 = _DISJOINT[nstreams]
    assert len(sp) == nstreams + 1 and st.n <= 400
    w_ref, P_ref, stats_ref, upd, ml = reference(("disjoint", nstreams), st, w0, method, 1.0, 0.0, STATS0)
    check_guard(method, st, upd, ml)
    W, P, stats = tables(w0, STATS0)
    gpu_train(method, st, W, P, stats, 1.0, 0.0, stream_ptr=sp, concurrent=True)
    assert_device(method, W, P, stats, w_ref, P_ref, stats_ref)


@pytest.mark.parametrize("method", METHODS)
def test_concurrent_shared_rows_properties(method):
    """8 streams x 10 samples on 32 shared rows of 64: the result depends on
    timing, so properties only"""
    rng = np.random.default_rng(50)
    wt, w0 = _model(rng, 64)
    samples = [_slots(rng, [3, 64, 65, 130, 300][s % 5], 32, distinct=False) for s in range(80)]
    st = Stream(samples, _targets(rng, samples, wt))
    W, P, stats = tables(w0)
    gpu_train(method, st, W, P, stats, 1.0, EPS, stream_ptr=np.arange(0, 81, 10, dtype=np.int64), concurrent=True)
    w, p, s = W.cpu().numpy(), P.cpu().numpy(), stats.cpu().numpy()
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(p)) and np.all(np.isfinite(s))
    assert np.all(p >= 1.0)
    assert np.array_equal(w[32:], w0[32:]) and np.all(p[32:] == 1.0)
    assert not np.array_equal(w[:32], w0[:32])
    if method in COV:
        assert np.all(p[:32] > 1.0)
    assert s[2] == st.n


# ------------------------------------------------------------------ wrapper
def test_wrapper_operand_checks():
    import torch
    st, w0 = case("boundary")
    W, P, stats = tables(w0)
    from jubatus_amd.ops import hip
    args = (_t(st.row_ptr), _t(st.fidx), _t(st.fval), _t(st.targets), _t(np.asarray([0, st.n], np.int64)), 1,
            W, stats, 1.0, EPS)
    with pytest.raises(ValueError, match="unknown method"):
        hip.regression_train(*args, concurrent=False, method="SVR")
    with pytest.raises(ValueError, match="precision table"):
        hip.regression_train(*args, concurrent=False, method="AROW")
    with pytest.raises(ValueError, match="slot_scratch"):       # 600-slot samples need it
        hip.regression_train(*args, concurrent=False, method="AROW", P=P)
    with pytest.raises(ValueError, match="slot_scratch"):
        hip.regression_train(*args, concurrent=False, method="AROW", P=P,
                             slot_scratch=torch.empty(3, dtype=torch.float32, device=dev()))
    assert torch.equal(W, _t(w0)) and torch.all(P == 1) and torch.all(stats == 0)


# ------------------------------------------------------------------ drivers
PARAMS = {"perceptron": {"sensitivity": 0.1, "learning_rate": 0.05}}


def _params(method):
    return PARAMS.get(method, {"sensitivity": 0.1, "regularization_weight": 1.0})


@pytest.mark.parametrize("method", METHODS)
def test_driver_matches_host_oracle(method):
    """the Python driver on the device == on the host (train_one) for wide
    datums and repeated keys; the device's pack() loads into a host driver"""
    from test_gpu_engines import CONV
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.models.regression import Regression
    g = Regression(method, _params(method), DatumToFvConverter(CONV), dev())
    c = Regression(method, _params(method), DatumToFvConverter(CONV))
    data = _driver_data("wide", 60) + _driver_data("dup", 60)
    for i in range(0, len(data), 20):
        assert g.train(data[i:i + 20]) == c.train(data[i:i + 20]) == 20
    q = [d for _, d in data[:20]] + [d for _, d in data[-20:]]
    want = c.estimate(q)
    np.testing.assert_allclose(g.estimate(q), want, rtol=1e-4, atol=1e-4)
    obj = g.pack()
    assert ("P" in obj) == (method in COV)
    h = Regression(method, _params(method), DatumToFvConverter(CONV))
    h.unpack(obj)
    np.testing.assert_allclose(h.estimate(q), want, rtol=1e-4, atol=1e-4)
    if method in COV:
        np.testing.assert_allclose(h.P, c.P, rtol=1e-4)
        assert np.any(h.P > 1.0)


# ------------------------------------------------------------ native server
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _native_data(rng, n):
    """datums of 300 num keys, datums that repeat a num key, and small ones"""
    from jubatus_amd.client import Datum
    coef = [random.Random(5).gauss(0, 1) for _ in range(300)]
    out = []
    for i in range(n):
        d = Datum()
        if i % 3 == 0:
            xs = [rng.gauss(0, 0.06) for _ in range(300)]
            for j, x in enumerate(xs):
                d.add(f"n{j}", x)
            y = sum(c * x for c, x in zip(coef, xs))
        else:
            xs = [rng.gauss(0, 1) for _ in range(3)]
            for j, x in enumerate(xs):
                d.add(f"n{j}", x)
            d.add("bias", 1.0)
            y = sum(c * x for c, x in zip(coef, xs)) + 1.0
            if i % 3 == 1:
                x0 = 0.5 + rng.random()
                d.add("n0", x0)                      # the key of the first slot again
                y += coef[0] * x0
        out.append((y + rng.gauss(0, 0.1), d))
    return out


@pytest.mark.parametrize("name", ["arow", "pa2", "perceptron"])
def test_native_server_matches_oracle_and_shares_files(tmp_path, name):
    """native jubaregression, request after request: estimates as the host
    oracle, model files in both directions with the Python driver (P
    included), status method"""
    from jubatus_amd.client import Regression
    from jubatus_amd.common.mprpc import RpcClient, RpcIOError, RpcTimeoutError
    from jubatus_amd.framework import save_load
    from jubatus_amd.fv_converter.converter import DatumToFvConverter, device_hash_max_size
    from jubatus_amd.models.regression import Regression as Driver
    cfg_file = config_path(f"regression/{name}.json")
    cfg = json.load(open(cfg_file))

    def oracle():
        return Driver(cfg["method"], cfg.get("parameter"),
                      DatumToFvConverter(cfg["converter"], default_hash_max_size=device_hash_max_size()),
                      device=None)

    port = _free_port()
    p = subprocess.Popen([os.path.join(NB, "jubaregression"), "-p", str(port), "-b", "127.0.0.1", "-f", cfg_file,
                          "-d", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    try:
        deadline = time.time() + 60
        while True:
            try:
                with RpcClient("127.0.0.1", port, 5.0) as rc:
                    rc.call("get_config", "")
                break
            except (OSError, RpcIOError, RpcTimeoutError):
                assert p.poll() is None and time.time() < deadline, p.stdout.read()
                time.sleep(0.2)
        c = Regression("127.0.0.1", port, "", timeout=60)
        ora = oracle()
        data = _native_data(random.Random(9), 90)
        for i in range(0, 60, 6):
            assert c.train(data[i:i + 6]) == 6
            ora.train([(s, d) for s, d in data[i:i + 6]])
        test = [d for _, d in data[60:]]
        got, want = c.estimate(test), ora.estimate(test)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)
        assert max(abs(x) for x in want) > 0.1
        (ident, st), = c.get_status().items()
        assert st["server_runtime"] == "native" and st["method"] == cfg["method"]
        # native file -> Python driver
        (_, path), = c.save("n1").items()
        with open(path, "rb") as f:
            _, pack = save_load.load_server(f, "regression", open(cfg_file).read(), 1, False)
        assert pack["method"] == cfg["method"] and ("P" in pack) == (cfg["method"] in COV)
        ora2 = oracle()
        ora2.unpack(pack)
        np.testing.assert_allclose(ora2.estimate(test), got, rtol=1e-6, atol=1e-6)
        if cfg["method"] in COV:
            np.testing.assert_allclose(ora2.P, ora.P, rtol=1e-4)
            assert np.any(ora2.P > 1.0)
        assert c.clear() is True
        assert all(v == 0.0 for v in c.estimate(test))
        assert c.load("n1") is True
        np.testing.assert_allclose(c.estimate(test), got, rtol=1e-6, atol=1e-6)
        # Python file -> native; training goes on from the loaded w and P
        p2 = os.path.join(str(tmp_path), f"{ident}_regression_py.jubatus")
        with open(p2, "wb") as f:
            save_load.save_server(f, "regression", "py", open(cfg_file).read(), 1, ora.pack())
        assert c.load("py") is True
        np.testing.assert_allclose(c.estimate(test), want, rtol=1e-4, atol=1e-4)
        assert c.train(data[60:66]) == 6
        ora.train([(s, d) for s, d in data[60:66]])
        np.testing.assert_allclose(c.estimate(test), ora.estimate(test), rtol=1e-4, atol=1e-4)
        (_, path), = c.save("n2").items()
        with open(path, "rb") as f:
            _, pack = save_load.load_server(f, "regression", open(cfg_file).read(), 1, False)
        if cfg["method"] in COV:
            ora2.unpack(pack)
            np.testing.assert_allclose(ora2.P, ora.P, rtol=1e-4)
        c.close()
    finally:
        p.terminate()
        try:
            p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            p.kill()


def test_native_distributed_mix_carries_precision(tmp_path):
    """two native servers on arow.json train different features; one MIX
    averages w, P and the statistics: both estimate alike and their saved
    files hold equal P (the mean of 1 and the trained precision on the
    trained rows)"""
    from test_native_dist_gpu import free_port, spawn, status, stop, wait_actives, wait_group
    from jubatus_amd.client import Datum, Regression
    from jubatus_amd.common import config as zkconfig
    from jubatus_amd.common.coordinator import NativeCoordinator
    from jubatus_amd.common.lock_service import CoordinatorClient
    from jubatus_amd.common.mprpc import wait_server
    from jubatus_amd.framework import save_load
    coord = NativeCoordinator(0, "127.0.0.1")
    ls = CoordinatorClient(f"127.0.0.1:{coord.port}", timeout=5.0)
    name = "nregm"
    text = open(config_path("regression/arow.json")).read()
    zkconfig.config_tozk(ls, "regression", name, text)
    ports = [free_port(), free_port()]
    procs = [spawn(coord.port, name, p, extra=("-d", str(tmp_path)), exe="jubaregression") for p in ports]
    try:
        for p in ports:
            assert wait_server("127.0.0.1", p, 90)
        assert wait_actives(ls, name, 2, engine="regression")
        a = Regression("127.0.0.1", ports[0], name, timeout=60.0)
        b = Regression("127.0.0.1", ports[1], name, timeout=60.0)
        assert wait_group(a, b, 2)
        assert a.train([(4.0, Datum({"x": 1.0}))] * 8) == 8
        assert b.train([(-2.0, Datum({"z": 1.0}))] * 8) == 8
        assert (a.estimate([Datum({"z": 1.0})])[0], b.estimate([Datum({"x": 1.0})])[0]) == (0.0, 0.0)
        assert a.do_mix() is True
        deadline = time.time() + 30
        while time.time() < deadline and status(b).get("mix.applied_count") in (None, "0"):
            time.sleep(0.1)
        for st in (status(a), status(b)):
            assert st["method"] == "AROW" and st["mix.last_applied"] == "1", st
        probe = [Datum({"x": 1.0}), Datum({"z": 1.0})]
        ea, eb = a.estimate(probe), b.estimate(probe)
        assert ea == pytest.approx(eb, abs=1e-5), (ea, eb)
        assert ea[0] > 0.5 and ea[1] < -0.2, ea
        packs = []
        for c in (a, b):
            (_, path), = c.save("mixed").items()
            with open(path, "rb") as f:
                packs.append(save_load.load_server(f, "regression", text, 1, False)[1])
        Pa, Pb = (np.frombuffer(p["P"], np.float32) for p in packs)
        assert packs[0]["rows"] == packs[1]["rows"] and len(Pa) == 2
        np.testing.assert_allclose(Pa, Pb, rtol=1e-6)
        assert np.all(Pa > 1.0)
        a.close()
        b.close()
    finally:
        stop(procs)
        ls.close()
        coord.stop()
