"""csrc/hip/regression_ordered.hip (jb_regression_train_ordered): the
serial-equivalent training of a batch of requests, against the float64
sequential references of tests/test_regression_methods.py (the six methods
besides PA) and tests/test_gpu_regression.py (PA), which are independent of
models/regression.py; the Python driver and the native server in exact mode
against the host oracle.

Streams, seeds, loss guards and bounds are the existing ones: W at rtol 1e-3,
atol 1e-4 * max|W_ref|; statistics at rtol 1e-4; P at rtol 1e-4
(test_regression_methods.assert_tables); estimates at rtol 1e-4, atol 1e-4.
PA runs the streams of tests/test_gpu_regression.py (`boundary`: the stream of
tests/test_regression_methods.py; the PA update is continuous in the state,
so it needs no seed search). The streams this file adds (table edges) run PA1
and CW only, the two rules that are continuous at loss = 0 and need no guard.

The entry takes one CSR batch and no request boundaries: the requests of a
batch lie back to back in request order, so `requests` cuts a stream into
uneven parts (empty ones among them) and `batch` lays them out again as the
callers do.
"""
import json
import os
import socket
import subprocess
import time

import msgpack
import numpy as np
import pytest

import test_gpu_regression as pa
from helpers import ROOT, config_path
from test_gpu_regression import Stream, _driver_data, _model, _slots, _targets
from test_regression_methods import COV, EPS, METHODS, assert_tables, case, check_guard, ref_train, reference

pytestmark = pytest.mark.gpu

NB = os.path.join(ROOT, "jubatus_amd", "native_bin")
ALL_METHODS = ["PA"] + METHODS
CASE_NAMES = ["widths", "boundary", "skipped", "repeated", "row_reuse"]
C_OF = {"PA": 0.05}                 # PA: part of the updating samples clip; the others 1.0
# uneven cuts into 2 .. 9 requests, as fractions of the stream; equal neighbours are empty requests
CUTS = {"widths": [0.0, 0.31, 1.0], "boundary": [0.0, 0.0, 0.07, 0.5, 0.5, 0.93, 1.0],
        "skipped": [0.0, 0.2, 0.2, 0.21, 0.6, 1.0, 1.0],
        "repeated": [0.0, 0.01, 0.13, 0.13, 0.4, 0.41, 0.77, 0.9, 1.0, 1.0],
        "row_reuse": [0.0, 0.5, 0.505, 1.0]}


def dev():
    import torch
    return torch.device("cuda", 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


# ------------------------------------------------------------------ inputs
_PA_CASES = {}


def stream_of(method, name):
    """-> (stream, initial w, w_ref, P_ref, stats_ref), the reference shared and unchanged"""
    C = C_OF.get(method, 1.0)
    if method == "PA":
        if name not in _PA_CASES:
            st, w0 = pa.EXACT_CASES[name]() if name in pa.EXACT_CASES else case(name)
            w_ref, stats_ref, log = pa.reference(st, w0, C, EPS)
            pa.check_clip_balance(log, C)
            _PA_CASES[name] = (st, w0, w_ref, np.ones(len(w0)), stats_ref)
        return _PA_CASES[name]
    st, w0 = case(name)
    w_ref, P_ref, stats_ref, upd, ml = reference(name, st, w0, method, C)
    check_guard(method, st, upd, ml)
    return st, w0, w_ref, P_ref, stats_ref


def requests(st, fractions):
    bounds = [int(round(f * st.n)) for f in fractions]
    assert bounds[0] == 0 and bounds[-1] == st.n and 2 <= len(bounds) - 1 <= 9
    return [st.part(a, b) for a, b in zip(bounds[:-1], bounds[1:])]


def batch(parts):
    """the requests back to back in request order, as one CSR batch"""
    s = Stream.__new__(Stream)
    s.n = sum(p.n for p in parts)
    s.fidx = np.concatenate([p.fidx for p in parts])
    s.fval = np.concatenate([p.fval for p in parts])
    s.targets = np.concatenate([p.targets for p in parts])
    s.row_ptr = np.zeros(s.n + 1, np.int64)
    at, base = 0, 0
    for p in parts:
        s.row_ptr[at + 1:at + p.n + 1] = base + p.row_ptr[1:]
        at, base = at + p.n, base + int(p.row_ptr[-1])
    return s


def tables(w0, stats0=None):
    import torch
    W = _t(w0)
    P = torch.ones_like(W)
    stats = torch.zeros(3, dtype=torch.float32, device=dev()) if stats0 is None else _t(stats0)
    return W, P, stats


def ordered(method, st, W, P, stats, win_slots=0, C=None, scratch=True):
    """one launch of the ordered entry; -> its status word on the host"""
    import torch
    from jubatus_amd.ops import hip
    assert st.fidx.size == 0 or (int(st.fidx.max()) < W.numel() and int(st.row_ptr[-1]) == st.fidx.size)
    fval = _t(st.fval)
    status = torch.full((2,), -1, dtype=torch.int32, device=dev())
    out = hip.regression_train_ordered(
        _t(st.row_ptr), _t(st.fidx), fval, _t(st.targets), st.n, W, stats, C_OF.get(method, 1.0) if C is None else C,
        EPS, method=method, P=P if method in COV else None,
        slot_scratch=torch.empty_like(fval) if method in COV and scratch else None, win_slots=win_slots,
        status=status)
    assert out is status
    return status.cpu().numpy()


def assert_device(method, W, P, stats, w_ref, P_ref, stats_ref):
    got_P = P.cpu().numpy()
    if method not in COV:
        assert np.all(got_P == 1.0)             # the kernel leaves a table it does not use alone
    assert_tables(W.cpu().numpy(), got_P, stats.cpu().numpy(), w_ref, P_ref, stats_ref, method in COV)


# ------------------------------------------- 1, 2: the cases, three windows
@pytest.mark.parametrize("win_slots", [0, 16, 64])
@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("method", ALL_METHODS)
def test_requests_in_order_match_float64_reference(method, name, win_slots):
    """the default window holds whole cases; at 16 and 64 slots row_reuse has
    3 and 12 samples a window (a stale read behind a write-back, or a lost
    write-back, shows), widths and skipped mix windowed samples with samples on
    the global path, boundary and repeated put most samples there"""
    st, w0, w_ref, P_ref, stats_ref = stream_of(method, name)
    parts = requests(st, CUTS[name])
    assert any(p.n == 0 for p in parts) or name in ("widths", "row_reuse")
    b = batch(parts)
    assert np.array_equal(b.row_ptr, st.row_ptr) and np.array_equal(b.fidx, st.fidx)
    W, P, stats = tables(w0)
    status = ordered(method, b, W, P, stats, win_slots)
    assert status.tolist() == [0, 0]
    assert_device(method, W, P, stats, w_ref, P_ref, stats_ref)


# ------------------------------------------------------------ 3: table edges
BIG_H = 1 << 20
EDGE_METHODS = ["PA1", "CW"]        # continuous at loss = 0: no guard, no seed search
_EDGE = {}


def _edge_stream(kind, win_slots):
    """full: samples of 64 (4 at the 64-slot window) slots on distinct rows, the first window holding exactly
    `win` distinct rows of H = 2^20, then a second pass over the same rows.
    home: every row of the first window has the same home position in the LDS
    table (one probe chain as long as the window), then the same rows again"""
    from jubatus_amd.ops import hip
    key = (kind, win_slots)
    if key not in _EDGE:
        win = win_slots or hip.REGRESSION_ORDERED_WIN_SLOTS
        rng = np.random.default_rng(77)
        if kind == "full":
            rows = rng.choice(BIG_H, size=win, replace=False).astype(np.int32)
            width = 64 if win > 64 else 4
        else:
            bits = hip.regression_ordered_table_bits(win_slots)
            cand = np.arange(BIG_H, dtype=np.uint64)
            home = ((cand * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)
            same = np.flatnonzero(home == home[12345])
            assert all(hip.regression_ordered_home(int(r), win_slots) == int(home[12345]) for r in same[:8])
            rows = same[:min(win, 64)].astype(np.int32)
            assert len(rows) == min(win, 64)
            width = 4
        assert len(rows) % width == 0 and len(set(rows.tolist())) == len(rows)
        wt = np.zeros(BIG_H)
        w0 = np.zeros(BIG_H, np.float32)
        wt[rows] = rng.standard_normal(len(rows))
        w0[rows] = (wt[rows] + 0.12 * rng.standard_normal(len(rows))).astype(np.float32)
        samples = []
        for _ in range(2):
            order = rng.permutation(rows)
            for k in range(0, len(rows), width):
                val = (rng.standard_normal(width) / np.sqrt(width)).astype(np.float32)
                samples.append((order[k:k + width].copy(), val))
        st = Stream(samples, _targets(rng, samples, wt))
        if kind == "full":
            assert int(st.row_ptr[len(samples) // 2]) == win       # the first window is exactly full
        _EDGE[key] = (st, w0, rows, {})
    return _EDGE[key]


def _edge_reference(st, w0, rows, refs, method):
    """the float64 reference over H = 2^20, once per stream and method; only the
    stream's own rows are kept (no other row can change)"""
    if method not in refs:
        w, P, stats = w0.astype(np.float64), np.ones(BIG_H), np.zeros(3)
        upd, ml = ref_train(method, w, P, stats, st, 1.0, EPS)
        check_guard(method, st, upd, ml)
        refs[method] = (w[rows], P[rows], stats)
    return refs[method]


@pytest.mark.parametrize("win_slots", [0, 64])
@pytest.mark.parametrize("kind", ["full", "home"])
@pytest.mark.parametrize("method", EDGE_METHODS)
def test_table_edges(method, kind, win_slots):
    st, w0, rows, refs = _edge_stream(kind, win_slots)
    w_ref, P_ref, stats_ref = _edge_reference(st, w0, rows, refs, method)
    W, P, stats = tables(w0)
    status = ordered(method, st, W, P, stats, win_slots)
    assert status.tolist() == [0, 0]
    got_w, got_P = W.cpu().numpy(), P.cpu().numpy()
    rest = np.ones(BIG_H, bool)
    rest[rows] = False
    assert np.all(got_w[rest] == 0.0) and np.all(got_P[rest] == 1.0)      # no other row is written
    assert_tables(got_w[rows], got_P[rows], stats.cpu().numpy(), w_ref, P_ref, stats_ref, method in COV)


# --------------------------------------------- 4: samples that never update
@pytest.mark.parametrize("method", ["PA", "perceptron", "CW", "AROW"])
def test_samples_without_slots_change_the_statistics_only(method):
    """every slot idx = -1 (1, 70 and 300 slots, the last one wider than the
    64-slot window of the second launch) or no slot at all: W and P keep every
    bit, the statistics take every target"""
    rng = np.random.default_rng(8)
    w0 = rng.standard_normal(64).astype(np.float32)
    samples = []
    for k in range(23):
        width = [0, 1, 70, 0, 300][k % 5]
        samples.append((np.full(width, -1, np.int32), rng.standard_normal(width).astype(np.float32)))
    ys = 2.0 + 0.3 * rng.standard_normal(len(samples))
    st = Stream(samples, ys)
    y64 = st.targets.astype(np.float64)
    for win_slots in (0, 64):
        W, P, stats = tables(w0, pa.STATS0)
        p0 = (1.0 + rng.random(64)).astype(np.float32)
        P.copy_(_t(p0))
        status = ordered(method, st, W, P, stats, win_slots)
        assert status.tolist() == [0, 0]
        np.testing.assert_array_equal(W.cpu().numpy(), w0)
        np.testing.assert_array_equal(P.cpu().numpy(), p0)
        want = pa.STATS0.astype(np.float64) + (y64.sum(), (y64 * y64).sum(), len(samples))
        np.testing.assert_allclose(stats.cpu().numpy(), want, rtol=1e-4)


# ------------------------------------------------------------ 5: carry-over
@pytest.mark.parametrize("win_slots", [0, 64])
@pytest.mark.parametrize("method", ALL_METHODS)
def test_tables_and_statistics_carry_over_launches(method, win_slots):
    """the widths stream in two launches == the one-launch reference"""
    st, w0, w_ref, P_ref, stats_ref = stream_of(method, "widths")
    W, P, stats = tables(w0)
    for a, b in ((0, 131), (131, st.n)):
        assert ordered(method, st.part(a, b), W, P, stats, win_slots).tolist() == [0, 0]
    assert_device(method, W, P, stats, w_ref, P_ref, stats_ref)


# ----------------------------------------------------------- 6: determinism
@pytest.mark.parametrize("name", ["widths", "row_reuse"])
@pytest.mark.parametrize("method", ["PA", "PA2", "AROW", "NHERD"])
def test_two_launches_give_the_same_bits(method, name):
    """indices are unique inside each sample of these streams, so no two adds
    of a sample meet in one LDS word and the order of the float adds is fixed"""
    st, w0, *_ = stream_of(method, name)
    for s in range(st.n):
        idx = st.fidx[st.row_ptr[s]:st.row_ptr[s + 1]]
        assert len(set(idx.tolist())) == len(idx)
    got = []
    for _ in range(2):
        W, P, stats = tables(w0)
        assert ordered(method, st, W, P, stats, 64 if name == "widths" else 0).tolist() == [0, 0]
        got.append((W.cpu().numpy(), P.cpu().numpy(), stats.cpu().numpy()))
    for a, b in zip(*got):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------- 7: against the single-stream launch
@pytest.mark.parametrize("name", ["widths", "repeated"])
@pytest.mark.parametrize("method", ALL_METHODS)
def test_against_the_single_stream_launch(method, name):
    """one concatenated stream through jb_regression_train_m (one stream) and
    through the ordered entry: within the bounds of each other; whether the
    bits are equal is printed, not asserted (repeated indices add in another
    order)"""
    import torch
    from jubatus_amd.ops import hip
    st, w0, *_ = stream_of(method, name)
    C = C_OF.get(method, 1.0)
    W1, P1, s1 = tables(w0)
    fval = _t(st.fval)
    hip.regression_train(_t(st.row_ptr), _t(st.fidx), fval, _t(st.targets), _t(np.asarray([0, st.n], np.int64)), 1,
                         W1, s1, C, EPS, concurrent=False, method=method, P=P1 if method in COV else None,
                         slot_scratch=torch.empty_like(fval) if method in COV else None)
    W2, P2, s2 = tables(w0)
    assert ordered(method, st, W2, P2, s2).tolist() == [0, 0]
    print("bit-identical to the single-stream launch: W %s, P %s, statistics %s"
          % (torch.equal(W1, W2), torch.equal(P1, P2), torch.equal(s1, s2)))
    assert_device(method, W2, P2, s2, W1.cpu().numpy().astype(np.float64), P1.cpu().numpy().astype(np.float64),
                  s1.cpu().numpy().astype(np.float64))


# -------------------------------------------------------- 8: argument errors
def test_argument_errors_leave_the_tables_alone():
    import torch
    from jubatus_amd.ops import hip
    from jubatus_amd.ops.hip import _fn, _p, _stream
    st, w0 = case("boundary")
    W, P, stats = tables(w0)
    args = (_t(st.row_ptr), _t(st.fidx), _t(st.fval), _t(st.targets), st.n, W, stats, 1.0, EPS)
    with pytest.raises(ValueError, match="win_slots"):
        hip.regression_train_ordered(*args, method="PA1", win_slots=hip.REGRESSION_ORDERED_WIN_SLOTS + 1)
    with pytest.raises(ValueError, match="precision table"):
        hip.regression_train_ordered(*args, method="AROW")
    with pytest.raises(ValueError, match="slot_scratch"):       # 600-slot samples need it
        hip.regression_train_ordered(*args, method="AROW", P=P)
    with pytest.raises(ValueError, match="unknown method"):
        hip.regression_train_ordered(*args, method="SVR")
    # the library itself: invalid value (hipErrorInvalidValue == 1), nothing launched
    status = torch.full((2,), -1, dtype=torch.int32, device=dev())
    scratch = torch.empty_like(args[2])
    raw = _fn("jb_regression_train_ordered")

    def call(P_, method_id, win, n=st.n, status_=status):
        return raw(_p(args[0]), _p(args[1]), _p(args[2]), _p(args[3]), n, _p(W), _p(P_), _p(stats), _p(scratch),
                   method_id, 1.0, EPS, win, _p(status_), _stream())

    assert call(P, 5, hip.REGRESSION_ORDERED_WIN_SLOTS + 1) == 1
    assert call(P, 5, -1) == 1
    assert call(None, 5, 0) == 1            # AROW without P
    assert call(P, 7, 0) == 1 and call(P, -1, 0) == 1
    assert call(P, 5, 0, status_=None) == 1
    assert call(P, 5, 0, n=0) == 0          # no samples: nothing to do
    torch.cuda.synchronize()
    assert torch.equal(W, _t(w0)) and torch.all(P == 1) and torch.all(stats == 0)
    assert status.tolist() == [-1, -1]
    assert hip.regression_train_ordered(args[0], args[1], args[2], args[3], 0, W, stats, 1.0, EPS,
                                        method="AROW", P=P).tolist() == [0, 0]
    assert torch.equal(W, _t(w0)) and torch.all(P == 1) and torch.all(stats == 0)


def test_wide_sample_without_scratch_reports_the_first_sample_not_applied():
    """status code 3: CW on the global path (64-slot windows), a 300-slot
    sample, no slot_scratch (the wrapper's width check is bypassed with a
    scratch tensor handed to it and a null pointer handed to the library).
    The samples before it are applied, it and its successors are not"""
    import torch
    from jubatus_amd.ops.hip import _fn, _p, _stream
    st, w0 = case("skipped")                  # widths 2, 5, 65, 100, 130, 300, ...
    first = 5
    assert int(np.diff(st.row_ptr)[first]) == 300 and np.all(np.diff(st.row_ptr)[:first] <= 256)
    w_ref, P_ref, stats_ref, _, _ = reference(("skipped", first), st.part(0, first), w0, "CW", 1.0)
    W, P, stats = tables(w0)
    status = torch.full((2,), -1, dtype=torch.int32, device=dev())
    ops = [_t(st.row_ptr), _t(st.fidx), _t(st.fval), _t(st.targets)]      # alive until the launch has run
    rc = _fn("jb_regression_train_ordered")(*[_p(t) for t in ops], st.n, _p(W), _p(P), _p(stats), None, 4, 1.0,
                                            EPS, 64, _p(status), _stream())
    assert rc == 0
    assert status.tolist() == [3, first]
    assert_device("CW", W, P, stats, w_ref, P_ref, stats_ref)
    from jubatus_amd.ops import hip
    with pytest.raises(RuntimeError, match=f"stopped at sample {first}"):
        hip.regression_ordered_check(status)


# ---------------------------------------------------------------- 9: driver
PARAMS = {"perceptron": {"sensitivity": 0.1, "learning_rate": 0.05}}


def _params(method):
    return PARAMS.get(method, {"sensitivity": 0.1, "regularization_weight": 1.0})


@pytest.mark.parametrize("method", ALL_METHODS)
def test_driver_exact_mode_matches_host_oracle(method):
    """8 requests submitted together in exact mode == the host driver trained
    on their concatenation (wide datums and repeated keys)"""
    from test_gpu_engines import CONV
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.models.regression import Regression
    g = Regression(method, _params(method), DatumToFvConverter(CONV), dev(), concurrent_update="exact")
    c = Regression(method, _params(method), DatumToFvConverter(CONV))
    assert g.pipe.fast and g.get_status()["train.update_mode"] == "exact"
    data = _driver_data("wide", 60) + _driver_data("dup", 60)
    cuts = [0, 3, 20, 21, 50, 64, 90, 117, 120]
    bodies = [msgpack.packb(data[a:b], use_bin_type=False) for a, b in zip(cuts[:-1], cuts[1:])]
    assert len(bodies) == 8
    assert g.train_requests(bodies) == c.train(data) == 120
    assert len(g._pending) == 1                 # the ordered launch, its status word not read yet
    q = [d for _, d in data[:20]] + [d for _, d in data[-20:]]
    want = c.estimate(q)
    np.testing.assert_allclose(g.estimate(q), want, rtol=1e-4, atol=1e-4)
    assert g._pending == [] and max(abs(x) for x in want) > 0.1
    if method in COV:
        np.testing.assert_allclose(g.P.cpu().numpy(), c.P, rtol=1e-4)
    # one request keeps the single-stream launch
    g.train_requests(bodies[:1])
    assert g._pending == []


def test_driver_default_mode_is_atomic():
    from test_gpu_engines import CONV
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.models.regression import Regression
    g = Regression("PA", _params("PA"), DatumToFvConverter(CONV), dev())
    assert g.get_status()["train.update_mode"] == "atomic"
    data = _driver_data("dup", 16)
    g.train_requests([msgpack.packb(data[:8], use_bin_type=False), msgpack.packb(data[8:], use_bin_type=False)])
    assert g._pending == []                     # the atomic launch of before


def test_driver_raises_on_the_next_synchronising_call():
    """a nonzero status word of an ordered launch raises on the driver's next
    synchronising call"""
    import torch
    from test_gpu_engines import CONV
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.models.regression import Regression
    g = Regression("PA", _params("PA"), DatumToFvConverter(CONV), dev(), concurrent_update="exact")
    g._pending.append(torch.tensor([1, 7], dtype=torch.int32, device=dev()))
    with pytest.raises(RuntimeError, match="stopped at sample 7"):
        g.estimate([[[], [["n0", 1.0]], []]])
    assert g._pending == []


# --------------------------------------------------------- 10: native server
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _pipelined_trains(port, frames):
    """every train written before any answer is read (one sendall): the
    server's batch thread takes them in arrival order, several per batch"""
    s = socket.create_connection(("127.0.0.1", port))
    s.sendall(b"".join(msgpack.packb([0, i, "train", ["", f]], use_bin_type=False) for i, f in enumerate(frames)))
    up = msgpack.Unpacker(raw=False)
    got = {}
    while len(got) < len(frames):
        chunk = s.recv(1 << 16)
        assert chunk
        up.feed(chunk)
        for msg in up:
            assert msg[2] is None, msg
            got[msg[1]] = msg[3]
    s.close()
    return [got[i] for i in range(len(frames))]


@pytest.mark.parametrize("name", ["pa", "arow"])
def test_native_server_exact_mode_matches_oracle_in_send_order(tmp_path, name):
    from jubatus_amd.common.mprpc import RpcClient, RpcIOError, RpcTimeoutError
    from jubatus_amd.fv_converter.converter import DatumToFvConverter, device_hash_max_size
    from jubatus_amd.models.regression import Regression as Driver
    cfg_file = config_path(f"regression/{name}.json")
    cfg = json.load(open(cfg_file))
    ora = Driver(cfg["method"], cfg.get("parameter"),
                 DatumToFvConverter(cfg["converter"], default_hash_max_size=device_hash_max_size()), device=None)
    data = _driver_data("wide", 96) + _driver_data("dup", 96)
    frames = [data[i:i + 6] for i in range(0, len(data), 6)]
    assert len(frames) == 32
    port = _free_port()
    env = dict(os.environ, JUBATUS_REGRESSION_UPDATE_MODE="exact")
    p = subprocess.Popen([os.path.join(NB, "jubaregression"), "-p", str(port), "-b", "127.0.0.1", "-f", cfg_file,
                          "-d", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
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
        assert _pipelined_trains(port, frames) == [6] * 32
        for f in frames:                      # the send order
            ora.train(f)
        q = [d for _, d in data[:20]] + [d for _, d in data[-20:]]
        want = ora.estimate(q)
        with RpcClient("127.0.0.1", port, 60.0) as rc:
            got = rc.call("estimate", "", q)
            (_, st), = rc.call("get_status", "").items()
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)
        assert max(abs(x) for x in want) > 0.1
        assert st["train.update_mode"] == "exact" and st["train.samples_trained"] == str(len(data))
        # a batch of several requests formed, so the ordered entry ran
        assert int(st["batching.train.calls"]) == 32
        assert int(st["batching.train.launches"]) < int(st["batching.train.calls"]), st
    finally:
        p.terminate()
        try:
            p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            p.kill()


def test_native_server_default_mode_is_atomic(tmp_path):
    from jubatus_amd.common.mprpc import RpcClient, RpcIOError, RpcTimeoutError
    cfg_file = config_path("regression/pa.json")
    port = _free_port()
    env = {k: v for k, v in os.environ.items() if k != "JUBATUS_REGRESSION_UPDATE_MODE"}
    p = subprocess.Popen([os.path.join(NB, "jubaregression"), "-p", str(port), "-b", "127.0.0.1", "-f", cfg_file,
                          "-d", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
    try:
        deadline = time.time() + 60
        while True:
            try:
                with RpcClient("127.0.0.1", port, 5.0) as rc:
                    (_, st), = rc.call("get_status", "").items()
                break
            except (OSError, RpcIOError, RpcTimeoutError):
                assert p.poll() is None and time.time() < deadline, p.stdout.read()
                time.sleep(0.2)
        assert st["train.update_mode"] == "atomic"
    finally:
        p.terminate()
        try:
            p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            p.kill()
