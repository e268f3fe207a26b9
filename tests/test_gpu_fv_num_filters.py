"""Num filters on the GPU fixed-slot path: fv_hash.hip (csrc/hip/jb_fv.hpp
emit_datum) through FeaturePipeline, in a batch the host scanner takes
(from_requests) and one the device scan takes (from_arena_gpu), against the
Python converter and slot by slot against HostFvHasher; then end to end
through the classifier, the regression driver, a recommender row engine and
the native jubaclassifier. Cases and tolerances: tests/fv_filter_cases.py."""
import json
import os
import random
import socket
import subprocess
import time

import msgpack
import numpy as np
import pytest

import fv_filter_cases as fc
import scan_cases as sc
from helpers import ROOT, start_standalone
from jubatus_amd.fv_converter import gpu_path
from jubatus_amd.fv_converter.converter import DatumToFvConverter

pytestmark = pytest.mark.gpu


def dev():
    import torch
    return torch.device("cuda", 0)


# ------------------------------------------------------------ feature rows
def _wide_datums():
    """9, 33, 40 and 129 num values: with 2 rows per value 33 -> 66 and 129 ->
    258 slots, with 8 rows 9 -> 72 and 40 -> 320: the derived rows carry the
    sample across the 64- and 256-slot widths of the training kernels"""
    rng = random.Random(4)
    return [sc.datum([], [sc.npair(b"k%d" % (j % 7), round(rng.uniform(-9, 9), 3), "f64")
                          for j in range(n)], nvf="auto") for n in (9, 33, 40, 129)]


def _requests(datums):
    """labeled requests: one of a single sample, then groups of 7"""
    ss = [sc.sample(b"", d) for d in datums]
    return [sc.body(ss[:1])] + [sc.body(ss[i:i + 7]) for i in range(1, len(ss), 7)]


def _table():
    from jubatus_amd._native import native
    t = native().LabelTable()
    t.get_or_add("")
    return t


def _rows(b, n_want):
    import torch
    torch.cuda.synchronize()
    assert b.n == n_want
    rp = b.row_ptr[:b.n + 1].cpu().numpy()
    idx = b.fidx[:rp[-1]].cpu().numpy()
    val = b.fval[:rp[-1]].cpu().numpy()
    return [(idx[rp[s]:rp[s + 1]], val[rp[s]:rp[s + 1]]) for s in range(b.n)]


def _device_rows(cfg, datums, shape):
    from jubatus_amd.ops.feature_pipeline import FeaturePipeline, ScanCheck
    pipe = FeaturePipeline(DatumToFvConverter(cfg), dev())
    assert pipe.fast
    bodies = _requests(datums)
    if shape == "host_scan":
        rows = _rows(pipe.from_requests(bodies, True, _table()), len(datums))
    else:
        arena, offs, lens = sc.build_arena(bodies, [(5 * k) % 16 for k in range(len(bodies))])
        chk = ScanCheck(128)
        b = pipe.from_arena_gpu(arena, offs, lens, _table(), chk)
        assert b is not None                    # the device scan took the batch
        rows = _rows(b, len(datums))
        assert int(chk.err[0]) == 0
    pipe.check_errors()
    return pipe, rows


def _check(cfg, datums, shape):
    pipe, rows = _device_rows(cfg, datums, shape)
    conv = pipe.conv
    worst = fc.compare(conv, datums, rows)
    # slot by slot against the host twin: the same sequence, -1 slots included;
    # values bit-equal but 3 ulp under `log` (two logf) and 1 ulp on the rows
    # whose chain holds a sigmoid (two exp)
    rt = pipe.rules
    is_log, has_sig = fc.row_kinds(rt)
    for d, (di, dv), (hi, hv) in zip(datums, rows, sc.native_rows(conv, datums)):
        np.testing.assert_array_equal(di, hi)
        obj = msgpack.unpackb(d, raw=True)
        ns, nn = len(obj[0]), len(obj[1])
        assert di.size == ns * rt.n_srules + nn * rt.n_nrules
        if di.size == 0:
            continue
        pad = np.zeros(ns * rt.n_srules, bool)
        log = np.concatenate([pad, np.tile(is_log, nn)])
        sig = np.concatenate([pad, np.tile(has_sig, nn)])
        np.testing.assert_array_equal(np.isnan(dv), np.isnan(hv))
        loose = (log | sig) & np.isfinite(hv) & np.isfinite(dv)
        exact = ~loose & ~np.isnan(hv)           # infinities included
        np.testing.assert_array_equal(dv[exact].view(np.uint32), hv[exact].view(np.uint32))
        if loose.any():
            assert (sc.ulp_diff(dv[loose], hv[loose]) <= np.where(log[loose], 3, 1)).all()
    print("largest distance from the Python converter [ulp]:", worst)


CASES = fc.method_cases()


@pytest.mark.parametrize("shape", ["host_scan", "device_scan"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_pipeline_equals_python_converter_and_host_twin(name, shape):
    cfg, sigmoid = CASES[name]
    values = [v for v in fc.VALUES if abs(v[0]) <= 500] if sigmoid else fc.VALUES
    datums = fc.datums(values) + fc.datums(fc.SPECIAL, keys=[b"height", b"t"], per=2) + _wide_datums()
    if name == "four_star":      # the rule blob is past kBlobCap: the kernel's global-memory blob path
        assert gpu_path.GpuRuleTable(DatumToFvConverter(cfg)).blob.size > 1024
    _check(cfg, datums, shape)


@pytest.mark.parametrize("shape", ["host_scan", "device_scan"])
def test_pipeline_matcher_boundaries_first_step(shape):
    _check(fc.boundary_step1(), fc.boundary_datums(), shape)


STEP2 = fc.boundary_step2()


@pytest.mark.parametrize("shape", ["host_scan", "device_scan"])
@pytest.mark.parametrize("k", range(len(STEP2)))
def test_pipeline_matcher_boundaries_second_step(k, shape):
    """every boundary matcher on the second step of a chain, where the step's
    ext_len is shorter than the row's whole extension"""
    _check(STEP2[k], fc.boundary_datums(), shape)


def test_sigmoid_saturates_on_the_device():
    """finite -g(x - b) above ~709.78 (the Python converter raises
    OverflowError there): 0.0 and 1.0, the closed form, as on the host twin"""
    cfg = fc.cfg([("*", "sig", "_n")], rules=[{"key": "*_n", "type": "num"}])
    d = sc.datum([], [sc.npair(b"k", -2000.0, "f64"), sc.npair(b"k", 2000.0, "f64")])
    _, ((idx, val),) = _device_rows(cfg, [d], "host_scan")
    np.testing.assert_array_equal(val[idx >= 0], np.float32([0.0, 1.0]))


# -------------------------------------------------------------- end to end
E2E = {
    "string_rules": [{"key": "*", "type": "str", "sample_weight": "bin", "global_weight": "bin"}],
    "num_filter_types": {
        "z": {"method": "gaussian_normalization", "average": 0.5, "standard_deviation": 2.0},
        "l": {"method": "linear_normalization", "min": 0, "max": 1048576},
        "s": {"method": "sigmoid_normalization", "gain": 0.05, "bias": -100}},
    "num_filter_rules": [{"key": "n*", "type": "z", "suffix": "_z"},
                         {"key": "big", "type": "l", "suffix": "_l"},
                         {"key": "neg", "type": "s", "suffix": "_s"}],
    "num_rules": [{"key": "*_z", "type": "num"}, {"key": "*_l", "type": "num"},
                  {"key": "*_s", "type": "num"}, {"key": "n1", "type": "log"}],
    "hash_max_size": 1 << 18,
}


def _data(n, nlabels=5, seed=0):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        y = rng.randrange(nlabels)
        d = {f"s{j}": f"v{(y * 7 + rng.randrange(4)) if rng.random() < 0.7 else rng.randrange(500)}"
             for j in range(3)}
        for j in range(3):
            d[f"n{j}"] = (y - 2) * 0.5 + rng.gauss(0, 1)
        d["big"] = rng.randrange(1 << 20)
        d["neg"] = -rng.randrange(200)
        out.append((f"L{y}", d))
    return out


def test_classifier_arow_matches_host():
    """AROW, exact mode, 400 samples of a filter config: the GPU model (device
    fv_hash with derived rows: 3 string + 5 x 16 num slots per sample) against
    device=None, at the bound of test_single_stream_train_matches_oracle"""
    from jubatus_amd.models.classifier import LinearClassifier
    param = {"regularization_weight": 0.7}
    g = LinearClassifier("AROW", param, DatumToFvConverter(E2E), device=dev())
    c = LinearClassifier("AROW", param, DatumToFvConverter(E2E), device=None)
    assert g._devfv and g.pipe.fast and g.pipe.rules.n_nrules == 16
    data = _data(400, seed=3)
    for i in range(0, len(data), 100):
        g.train(data[i:i + 100])
        c.train(data[i:i + 100])
    g.synchronize()
    Wg = g.W.cpu().numpy()
    scale = float(np.abs(c.W).max()) or 1.0
    np.testing.assert_allclose(Wg[:, :c.LC], c.W, rtol=2e-3, atol=2e-3 * scale)
    pscale = float(np.abs(c.P).max())
    np.testing.assert_allclose(g.P.cpu().numpy()[:, :c.LC], c.P, rtol=2e-3, atol=2e-3 * pscale)
    q = [d for _, d in data[:64]]
    for direct in (True, False):                 # classify_direct (host twin), batch (device)
        g.direct = direct
        for a, b in zip(g.classify(q[:3] if direct else q), c.classify(q[:3] if direct else q)):
            assert [x[0] for x in a] == [x[0] for x in b]
            np.testing.assert_allclose([x[1] for x in a], [x[1] for x in b], rtol=2e-3, atol=2e-3)
    assert g.get_labels() == c.get_labels()


def test_regression_matches_host():
    """the bound of test_gpu_engines.test_regression_single_stream_matches_oracle"""
    from jubatus_amd.models.regression import PARegression
    conv = {"num_filter_types": E2E["num_filter_types"],
            "num_filter_rules": [{"key": "x", "type": "z", "suffix": "_z"}],
            "string_rules": E2E["string_rules"],
            "num_rules": [{"key": "*_z", "type": "num"}, {"key": "x", "type": "num"}],
            "hash_max_size": 1 << 18}
    p = {"sensitivity": 0.1, "regularization_weight": 2.0}
    g = PARegression("PA", p, DatumToFvConverter(conv), dev())
    c = PARegression("PA", p, DatumToFvConverter(conv))
    r = random.Random(1)
    data = [[3.0 * x + 1.0 + r.gauss(0, 0.1), {"x": x, "t": f"k{int(x * 3) % 5}"}]
            for x in (r.random() for _ in range(300))]
    for i in range(0, 300, 50):
        g.train(data[i:i + 50])
        c.train(data[i:i + 50])
    np.testing.assert_allclose(g.w.cpu().numpy(), c.w, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(g.stats.cpu().numpy(), c.stats, rtol=1e-4)
    q = [d for _, d in data[:20]]
    np.testing.assert_allclose(g.estimate(q), c.estimate(q), rtol=1e-4, atol=1e-4)


def test_recommender_euclid_lsh_same_neighbours():
    from jubatus_amd.models.recommender import Recommender
    conv = {"num_filter_types": E2E["num_filter_types"],
            "num_filter_rules": [{"key": "*", "type": "z", "suffix": "_z"}],
            "num_rules": [{"key": "*_z", "type": "num"}], "hash_max_size": 1 << 18}
    g = Recommender("euclid_lsh", {"hash_num": 64}, DatumToFvConverter(conv), dev())
    c = Recommender("euclid_lsh", {"hash_num": 64}, DatumToFvConverter(conv))
    assert g._hasher() is not None               # the fixed-slot host twin, not the Python converter
    rng = random.Random(6)
    rows = [(f"r{i}", {"a": 4.0 * (i % 8) + rng.random(), "b": 5.0 * (i // 8) + rng.random()})
            for i in range(48)]
    g.set_rows(rows)
    c.set_rows(rows)
    for q in ({"a": 9.0, "b": 11.0}, {"a": 30.0, "b": 0.5}, {"a": 17.0}):
        rg, rc = g.similar_row_from_datum(q, 4), c.similar_row_from_datum(q, 4)
        assert [r for r, _ in rg] == [r for r, _ in rc]


BIN = os.path.join(ROOT, "jubatus_amd", "native_bin", "jubaclassifier")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_native_jubaclassifier_against_the_python_cpu_server(tmp_path):
    """train, classify and a one-datum classify (classify_direct: the host
    twin) over RPC on the native server, against the Python server on the
    host converter (--cpu)"""
    from jubatus_amd.client import Classifier, Datum
    from jubatus_amd.common.mprpc import RpcClient, RpcIOError, RpcTimeoutError
    text = json.dumps({"method": "AROW", "parameter": {"regularization_weight": 1.0}, "converter": E2E})
    cfg = tmp_path / "filters.json"
    cfg.write_text(text)
    (tmp_path / "py").mkdir()
    h = start_standalone("classifier", text, tmp_path / "py")
    port = _free_port()
    p = subprocess.Popen([BIN, "-p", str(port), "-b", "127.0.0.1", "-f", str(cfg), "-d", str(tmp_path),
                          "-c", "4"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    try:
        deadline = time.time() + 60
        while True:
            try:
                with RpcClient("127.0.0.1", port, 5.0) as rc:
                    rc.call("get_config", "")
                break
            except (OSError, RpcIOError, RpcTimeoutError):
                assert p.poll() is None and time.time() < deadline, "native server did not start"
                time.sleep(0.1)
        n = Classifier("127.0.0.1", port, "", timeout=60)
        y = Classifier("127.0.0.1", h.argv.port, "", timeout=60)
        data = [(lab, Datum(d)) for lab, d in _data(300, seed=8)]
        for i in range(0, 300, 50):
            assert n.train(data[i:i + 50]) == 50 and y.train(data[i:i + 50]) == 50
        (_, st), = n.get_status().items()
        assert st["server_runtime"] == "native" and int(st["train_scan.gpu"]) >= 1
        test = [d for _, d in data[:40]]
        for query in (test, test[:1]):
            got = [{e.label: e.score for e in r} for r in n.classify(query)]
            want = [{e.label: e.score for e in r} for r in y.classify(query)]
            assert len(got) == len(query)
            for a, b in zip(got, want):
                assert set(a) == set(b)
                for k in b:
                    assert abs(a[k] - b[k]) <= 1e-4 * max(1.0, abs(b[k])), (k, a[k], b[k])
        n.close()
        y.close()
    finally:
        h.stop()
        p.terminate()
        try:
            p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            p.kill()
