"""Num filters on the GPU wide rule set: csrc/hip/fv_wide.hip through
ops/fv_wide.py WideDevice against the Python converter and against the host
twin HostFvWide, feature by feature in order (the combination pairs hang on
it), in batches that cross a wave and a 256-thread block; the base-slot limit;
then end to end through the classifier and a recommender. Cases and
tolerances: tests/fv_wide_filter_cases.py."""
import json
import os
import random

import numpy as np
import pytest

import fv_filter_cases as fc
import fv_wide_filter_cases as wc
import scan_cases as sc
from helpers import ROOT
from jubatus_amd.fv_converter.converter import DatumToFvConverter
from jubatus_amd.fv_converter.gpu_path import WideRuleTable, fast_eligible, wide_eligible

pytestmark = pytest.mark.gpu

BATCHES = (1, 65, 257)          # one lane, past a wave, past a 256-thread block


def dev():
    import torch
    return torch.device("cuda", 0)


def device_rows(wd, blobs, update):
    """WideDevice.convert on encoded datums (the helper shape of
    test_fv_wide.py _device_convert) -> per datum (idx, val), idx < 0 dropped"""
    import torch
    d = wd.device
    offs = np.zeros(len(blobs), np.int64)
    np.cumsum([len(b) for b in blobs[:-1]], out=offs[1:])
    buf = b"".join(blobs) + b"\0" * 16
    d_buf = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(d)
    d_off = torch.from_numpy(offs).to(d)
    d_len = torch.tensor([len(b) for b in blobs], dtype=torch.int32, device=d)
    rp, idx, val, total = wd.convert(d_buf, len(buf) - 16, d_off, d_len, len(blobs), update)
    rp, idx, val = rp.cpu().numpy(), idx[:total].cpu().numpy(), val[:total].cpu().numpy()
    assert int(wd.err.item()) == 0
    out = []
    for i in range(len(blobs)):
        a, b = rp[i], rp[i + 1]
        keep = idx[a:b] >= 0
        out.append((idx[a:b][keep], val[a:b][keep]))
    return out


def _device_check(cfg, datums, batches=BATCHES):
    from jubatus_amd.ops.fv_wide import WideDevice
    cpy, chost, cdev = (DatumToFvConverter(cfg) for _ in range(3))
    assert wide_eligible(cdev) and not fast_eligible(cdev)
    wd = WideDevice(cdev, dev())
    exp = [wc.Expected(cpy, d) for d in datums]             # once, shared by every batch
    host = wc.host_rows(wc.host_wide(chost), datums)
    for n in batches:
        batch = [datums[i % len(datums)] for i in range(n)]
        for update in (True, False):
            rows = device_rows(wd, batch, update)
            assert len(rows) == n
            for i, (idx, val) in enumerate(rows):
                j = i % len(datums)
                wc.check_row(exp[j], idx, val, wc.DEVICE_TOL)
                np.testing.assert_array_equal(idx, host[j][0])
                np.testing.assert_allclose(val, host[j][1], rtol=wc.DEVICE_TOL[0], atol=wc.DEVICE_TOL[1])
    return exp


CASES = wc.method_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_wide_equals_python_converter_and_host_twin(name):
    """fails on the parent (WideRuleTable raised ValueError)"""
    cfg, sigmoid = CASES[name]
    _device_check(cfg, wc.datums(sigmoid))


BOUNDARY = wc.boundary_cases()


@pytest.mark.parametrize("k", range(len(BOUNDARY)))
def test_device_wide_matcher_boundaries(k):
    """the derived names through name_matches at every matcher boundary (the
    num rules) and through the `*` x `*` pair loop"""
    _device_check(BOUNDARY[k], fc.boundary_datums())


FOUR_STAR = [("*", "add", f"_{i}") for i in range(4)]       # 15 chains, all of them fire


def test_fifteen_chains_with_a_mul_combination():
    """three values per datum: 3 x 16 = 48 base slots and 48 x 47 / 2 = 1128 pairs"""
    cfg = fc.cfg(FOUR_STAR, combination_rules=wc.STAR_MUL)
    assert WideRuleTable(DatumToFvConverter(cfg)).n_chains == 15
    datums = [sc.datum([], [sc.npair(b"k%d" % j, 0.25 * (i + 1) * (j - 1.5), "f64") for j in range(3)])
              for i in range(5)]
    exp = _device_check(cfg, datums)
    assert all(e.n_num == 48 and len(e.idx) == 48 + 1128 for e in exp)


def _max_base_datum(n):
    return sc.datum([], [sc.npair(b"k%d" % j, 0.5 * j - 7, "f64") for j in range(n)], nvf="auto")


def test_base_slot_limit_counts_derived_rows():
    """kWideMaxBase = 4096 base slots per datum, derived rows included: with 16
    blocks 256 values fill it exactly, 257 values are refused"""
    from jubatus_amd._native import native
    from jubatus_amd.ops.feature_pipeline import FeaturePipeline
    from jubatus_amd.ops.fv_wide import WideDevice
    cfg = fc.cfg(FOUR_STAR, string_rules=[wc.SPACE])
    exp = _device_check(cfg, [_max_base_datum(256)], batches=(1,))
    assert exp[0].n_num == 4096
    wd = WideDevice(DatumToFvConverter(cfg), dev())
    with pytest.raises(AssertionError):                     # device_rows asserts wd.err == 0
        device_rows(wd, [_max_base_datum(257)], False)
    assert int(wd.err.item()) == 2
    pipe = FeaturePipeline(DatumToFvConverter(cfg), dev())
    assert pipe.wide and not pipe.fast
    table = native().LabelTable()
    table.get_or_add("")
    with pytest.raises(TypeError, match="device wide converter"):
        pipe.from_requests([sc.body([sc.sample(b"", _max_base_datum(257))])], True, table)
    b = pipe.from_requests([sc.body([sc.sample(b"", _max_base_datum(256))])], True, table)
    assert b.n == 1 and int(b.row_ptr[1].item()) == 4096


def test_sigmoid_saturates_on_the_device():
    """inputs -2000 and 2000 (the Python converter's math.exp overflows):
    exactly 0.0 and 1.0, as on the fixed-slot path and the host twin"""
    from jubatus_amd.ops.fv_wide import WideDevice
    cfg = fc.cfg([("*", "sig", "_n")], rules=[{"key": "*_n", "type": "num"}],
                 combination_rules=wc.STAR_ADD)
    d = sc.datum([], [sc.npair(b"k", -2000.0, "f64"), sc.npair(b"k", 2000.0, "f64")])
    (idx, val), = device_rows(WideDevice(DatumToFvConverter(cfg), dev()), [d], False)
    np.testing.assert_array_equal(val, np.float32([0.0, 1.0, 1.0]))
    (hidx, hval), = wc.host_rows(wc.host_wide(DatumToFvConverter(cfg)), [d])
    np.testing.assert_array_equal(idx, hidx)
    np.testing.assert_array_equal(val, hval)


# -------------------------------------------------------------- end to end
def _e2e_converter():
    """config/classifier/arow_combinational_feature.json's converter (every
    pair of features multiplied) with the numbers normalised first"""
    with open(os.path.join(ROOT, "config", "classifier", "arow_combinational_feature.json")) as f:
        conv = json.load(f)["converter"]
    conv["num_filter_types"] = {"g": {"method": "gaussian_normalization", "average": 0.5,
                                      "standard_deviation": 2.0}}
    conv["num_filter_rules"] = [{"key": "*", "type": "g", "suffix": "_g"}]
    conv["hash_max_size"] = 1 << 16
    return conv


def test_classifier_trains_on_the_device_wide_path():
    """AROW on the combination config plus a gaussian filter: converted on the
    device (fails on the parent: fv_path is the host converter's) and, trained
    as three batches, equal to the host driver at the tolerance of
    test_fv_wide.py test_classifier_trains_on_device_wide_converter"""
    from jubatus_amd.models.classifier import LinearClassifier
    conv = _e2e_converter()
    r = random.Random(3)
    data = []
    for _ in range(300):
        y = r.randrange(3)
        data.append((f"L{y}", {"a": f"w{y}{r.randrange(4)}x", "b": f"v{r.randrange(9)}",
                               "x": y + r.gauss(0, 0.3), "z": r.gauss(0, 1)}))
    param = {"regularization_weight": 1.0}
    g = LinearClassifier("AROW", param, DatumToFvConverter(conv), device=dev())
    h = LinearClassifier("AROW", param, DatumToFvConverter(conv))
    assert g.get_status()["fv_path"] == "gpu-wide"
    for i in range(0, 300, 100):
        g.train(data[i:i + 100])
        h.train(data[i:i + 100])
    G = g.W.cpu().numpy()[:, :g.labels.size()]
    Hm = h.W[:, :h.labels.size()]
    assert np.abs(Hm).max() > 0
    np.testing.assert_allclose(G, Hm, rtol=1e-3, atol=1e-4)
    test = [d for _, d in data[:50]]
    pg = [max(x, key=lambda e: e[1])[0] for x in g.classify(test)]
    ph = [max(x, key=lambda e: e[1])[0] for x in h.classify(test)]
    assert pg == ph


def test_recommender_inverted_index_same_neighbours():
    from jubatus_amd.models.recommender import Recommender
    g = Recommender("inverted_index", {}, DatumToFvConverter(wc.DRIVER), dev())
    c = Recommender("inverted_index", {}, DatumToFvConverter(wc.DRIVER))
    assert type(g._hasher()).__name__ == "HostFvWide"
    c._host_hasher = False                       # the per-datum Python converter
    rows = wc.driver_rows()
    g.set_rows(rows)
    c.set_rows(rows)
    for q in ({"a": 9.0, "b": 11.0}, {"a": 30.0, "b": 0.5, "t": "w1"}, {"a": 17.0}):
        rg, rc = g.similar_row_from_datum(q, 4), c.similar_row_from_datum(q, 4)
        assert [r for r, _ in rg] == [r for r, _ in rc]
