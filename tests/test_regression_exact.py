"""The regression driver's ``concurrent_update`` argument (atomic | exact), its
status key, the Python server's JUBATUS_REGRESSION_UPDATE_MODE on the host
backend (sequential in either mode: same estimates) and the ctypes entry of
csrc/hip/regression_ordered.hip. The device side is
tests/test_gpu_regression_exact.py."""
import ctypes

import numpy as np
import pytest

from helpers import config_path, start_standalone
from test_regression_methods import CONV, _data

ENV = "JUBATUS_REGRESSION_UPDATE_MODE"


def _driver(method="PA", parameter=None, **kw):
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.models.regression import Regression
    return Regression(method, parameter or {"regularization_weight": 1.0}, DatumToFvConverter(CONV), None, **kw)


def test_concurrent_update_values():
    from jubatus_amd.models.regression import UPDATE_MODES, RegressionConfigError
    assert UPDATE_MODES == ("atomic", "exact")
    assert _driver().concurrent_update == "atomic"
    for mode in UPDATE_MODES:
        assert _driver(concurrent_update=mode).concurrent_update == mode
    for bad in ("hogwild", "serial", "", "Exact", None):
        with pytest.raises(RegressionConfigError, match="concurrent_update"):
            _driver(concurrent_update=bad)


@pytest.mark.parametrize("method", ["PA", "AROW"])
def test_status_key_and_host_backend_is_sequential_in_both_modes(method):
    import msgpack
    data = _data(60)
    a, e = _driver(method), _driver(method, concurrent_update="exact")
    assert a.get_status()["train.update_mode"] == "atomic"
    assert e.get_status()["train.update_mode"] == "exact"
    assert {k: v for k, v in a.get_status().items() if k != "train.update_mode"} == \
        {"num_features": "1024", "method": method, "storage": "host"}
    bodies = [msgpack.packb(data[i:i + 15], use_bin_type=False) for i in range(0, 60, 15)]
    assert a.train(data) == e.train_requests(bodies) == 60
    assert np.array_equal(a.w, e.w) and np.array_equal(a.stats, e.stats) and np.any(a.w != 0)
    q = [d for _, d in data[:10]]
    assert a.estimate(q) == e.estimate(q)


def _serve(tmp_path, sub, data, q):
    from jubatus_amd.client import Datum, Regression
    (tmp_path / sub).mkdir()
    h = start_standalone("regression", config_path("regression/arow.json"), tmp_path / sub)
    try:
        with Regression("127.0.0.1", h.argv.port, "") as c:
            for i in range(0, len(data), 10):
                assert c.train([[s, Datum(dict(d[1]))] for s, d in data[i:i + 10]]) == 10
            status = list(c.get_status().values())[0]
            return c.estimate([Datum(dict(d[1])) for d in q]), status
    finally:
        h.stop()


def test_python_server_cpu_reads_the_variable(tmp_path, monkeypatch):
    """exact, atomic, unset and an unknown value: the host backend returns the
    same estimates; the status shows the mode (unset / unknown: atomic)"""
    data = _data(40)
    q = [d for _, d in data[:10]]
    monkeypatch.delenv(ENV, raising=False)
    base, st = _serve(tmp_path, "unset", data, q)
    assert st["train.update_mode"] == "atomic" and any(abs(x) > 0.1 for x in base)
    for value, want in (("exact", "exact"), ("atomic", "atomic"), ("serial", "atomic")):
        monkeypatch.setenv(ENV, value)
        got, st = _serve(tmp_path, value, data, q)
        assert st["train.update_mode"] == want
        assert got == base


def test_ordered_entry_is_in_the_ctypes_table():
    from jubatus_amd.ops import hip
    assert callable(hip.regression_train_ordered) and callable(hip.regression_ordered_check)
    ret, args = hip._SIGS["jb_regression_train_ordered"]
    assert ret is ctypes.c_int32 and len(args) == 15
    assert args[4] is ctypes.c_int64 and args[12] is ctypes.c_int32      # n_samples, win_slots
    assert hasattr(hip.hip_lib(), "jb_regression_train_ordered")


def test_home_function_of_the_lds_table():
    """ops/hip.py regression_ordered_home mirrors the kernel's header:
    ((uint32)idx * 0x9E3779B1) >> (32 - bits), a table of at least 64 and at
    least 2 * win_slots entries"""
    from jubatus_amd.ops import hip
    assert hip.REGRESSION_ORDERED_WIN_SLOTS == 4096
    assert [hip.regression_ordered_table_bits(w) for w in (0, 4096, 2049, 2048, 64, 33, 32, 16, 1)] == \
        [13, 13, 13, 12, 7, 7, 6, 6, 6]
    for idx in (0, 1, 12345, (1 << 20) - 1, (1 << 31) - 1):
        for win in (0, 64, 16):
            bits = hip.regression_ordered_table_bits(win)
            want = int((np.uint32(idx) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> (32 - bits)
            assert hip.regression_ordered_home(idx, win) == want < (1 << bits)
