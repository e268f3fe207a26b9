"""Num filters on the fixed-slot path, host side: eligibility and the rule
tables (fv_converter/gpu_path.py), the host hasher HostFvHasher
(csrc/native/jb_hostfv.hpp) against the Python converter on every method,
chain and matcher boundary of tests/fv_filter_cases.py, and the native
servers' config check. CPU."""
import json
import math
import os
import re
import struct
import subprocess

import msgpack
import numpy as np
import pytest

import fv_filter_cases as fc
import scan_cases as sc
from jubatus_amd.fv_converter.converter import DatumToFvConverter
from jubatus_amd.fv_converter import gpu_path
from jubatus_amd.fv_converter.datum import Datum
from jubatus_amd.fv_converter.gpu_path import GpuRuleTable, fast_eligible, gpu_eligible

PKG = os.path.dirname(os.path.abspath(gpu_path.__file__))
NATIVE_BIN = os.path.join(os.path.dirname(PKG), "native_bin")


# ------------------------------------------------------------- eligibility
@pytest.mark.parametrize("t", sorted(fc.TYPES))
def test_each_method_is_eligible_and_packs(t):
    """fails on the parent: GpuRuleTable raised ValueError on any filter"""
    conv = DatumToFvConverter(fc.cfg([("*", t, "_n")]))
    assert fast_eligible(conv) and gpu_eligible(conv)
    rt = GpuRuleTable(conv)
    assert (rt.n_srules, rt.n_nrules) == (0, 2)
    base, derived = (gpu_path._RULE.unpack_from(rt.nrules, 32 * i) for i in range(2))
    assert base[5] == 0 and base[7] == 0
    assert derived[5] == gpu_path._DERIVED_ROW and derived[7] % 8 == 0
    blob = bytes(rt.blob)
    assert blob[derived[3]:derived[3] + derived[4]] == b"_n@num"
    n_steps, ext = struct.unpack_from("<ii", blob, derived[7])
    assert (n_steps, ext) == (1, 2)
    step = gpu_path._STEP.unpack_from(blob, derived[7] + 8)
    assert step[:4] == (0, step[1], 0, 0) and step[4] == gpu_path._METHOD[fc.TYPES[t]["method"]]


def _parent_tables(conv):
    """the packing of GpuRuleTable before filters were served, literally"""
    RULE = struct.Struct("<iiiiiifi")
    KIND = {"all": 0, "prefix": 1, "suffix": 2, "exact": 3}
    blob = bytearray()

    def put(b):
        off = len(blob)
        blob.extend(b)
        return off, len(b)

    srows, nrows = [], []
    for r in conv.string_rules:
        mo, ml = put(r.matcher.arg.encode())
        so, sl = put(r.suffix.encode())
        w = {"bin": 1.0, "tf": 1.0, "log_tf": math.log(2.0)}[r.sw]
        srows.append(RULE.pack(KIND[r.matcher.kind], mo, ml, so, sl, 0, w, 0))
    for r in conv.num_rules:
        mo, ml = put(r.matcher.arg.encode())
        so, sl = put(f"@{r.type_name}".encode())
        nrows.append(RULE.pack(KIND[r.matcher.kind], mo, ml, so, sl,
                               1 if r.type_name == "log" else 0, 0.0, 0))
    return (b"".join(srows) or b"\0" * 32, b"".join(nrows) or b"\0" * 32, bytes(blob) or b"\0",
            len(srows), len(nrows))


@pytest.mark.parametrize("cfg", [sc.CONV, sc.CONV_FV, sc.CONV_SLOT,
                                 {"num_rules": [{"key": "*", "type": "num"}]}, {}],
                         ids=["scan", "fv", "slot", "num_only", "empty"])
def test_tables_without_filters_are_unchanged(cfg):
    conv = DatumToFvConverter(cfg)
    rt = GpuRuleTable(conv)
    s, n, blob, ns, nn = _parent_tables(conv)
    assert (bytes(rt.srules), bytes(rt.nrules), bytes(rt.blob)) == (s, n, blob)
    assert (rt.n_srules, rt.n_nrules) == (ns, nn)


def test_what_stays_with_the_host_converter(tmp_path):
    star = [{"key": "*", "type": "num"}]
    # a regex filter key
    assert not fast_eligible(DatumToFvConverter(fc.cfg([("/^h/", "add", "_n")])))
    # a string filter
    c = fc.cfg([("*", "add", "_n")])
    c["string_filter_types"] = {"detag": {"method": "regexp", "pattern": "<[^>]*>", "replace": ""}}
    c["string_filter_rules"] = [{"key": "*", "type": "detag", "suffix": "-d"}]
    assert not fast_eligible(DatumToFvConverter(c))
    # a plug-in filter: the loader is asked for it, the tables refuse it
    c = {"num_filter_types": {"p": {"method": "dynamic", "path": "x.so", "function": "create"}},
         "num_filter_rules": [{"key": "*", "type": "p", "suffix": "_p"}], "num_rules": star}

    class Loader:
        def create(self, kind, params):
            return lambda x: x
    conv = DatumToFvConverter(c, plugin_loader=Loader())
    assert not fast_eligible(conv) and not gpu_eligible(conv)
    with pytest.raises(ValueError):
        GpuRuleTable(conv)
    # the chain cap: three `*` filters make 7 chains, four 15, five 31
    for n, ok in ((3, True), (4, True), (5, False)):
        conv = DatumToFvConverter(fc.cfg([("*", "add", f"_{i}") for i in range(n)]))
        assert fast_eligible(conv) == ok, n
        if ok:
            assert GpuRuleTable(conv).n_nrules == 2 ** n
    # chains that cannot fire are pruned: 16 exact-key filters are 16 chains
    keys = [f"k{i}" for i in range(16)]
    conv = DatumToFvConverter(fc.cfg([(k, "gauss", "_z") for k in keys]))
    assert fast_eligible(conv) and GpuRuleTable(conv).n_nrules == 17
    assert not fast_eligible(DatumToFvConverter(fc.cfg([(k, "gauss", "_z") for k in keys + ["k16"]])))
    # ... but a later exact filter on a derived key keeps its chain: (0), (1)
    # on an original key `a_1`, (0, 1), (2); (0, 2), (1, 2), (0, 1, 2) cannot fire
    conv = DatumToFvConverter(fc.cfg([("a", "add", "_1"), ("a_1", "gauss", "_2"), ("b_1", "add", "_3")]))
    assert GpuRuleTable(conv).n_nrules == 1 + 4


def test_cap_constant_is_shared_with_the_native_header():
    src = open(os.path.join(PKG, "..", "csrc", "native", "jb_fv_layout.hpp")).read()
    assert int(re.search(r"kMaxFilterChains = (\d+);", src).group(1)) == gpu_path.MAX_FILTER_CHAINS


# ---------------------------------------- host twin against the Python converter
def _host(cfg, datums):
    conv = DatumToFvConverter(cfg)
    rows = sc.native_rows(conv, datums)
    rt = GpuRuleTable(conv)
    for d, (idx, _) in zip(datums, rows):       # one slot per (value, row), string rules first
        obj = msgpack.unpackb(d, raw=True)
        assert idx.size == len(obj[0]) * rt.n_srules + len(obj[1]) * rt.n_nrules
    return fc.compare(conv, datums, rows)


CASES = fc.method_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_hasher_equals_python_converter(name):
    cfg, tol = CASES[name]
    values = [v for v in fc.VALUES if abs(v[0]) <= 500] if tol else fc.VALUES
    _host(cfg, fc.datums(values))
    _host(cfg, fc.datums(fc.SPECIAL, keys=[b"height", b"t"], per=2))


def test_truncate_clamps_and_nan_becomes_zero():
    """closed form: linear_normalization of [-3, 7] with truncate"""
    conv = DatumToFvConverter(fc.cfg([("*", "lin", "_n")], rules=[{"key": "*_n", "type": "num"}]))
    xs = [-10.5, -3, 2, 7, 7.5, math.nan, math.inf, -math.inf]
    d = sc.datum([], [sc.npair(b"k", x, "f64") for x in xs])
    (idx, val), = sc.native_rows(conv, [d])
    np.testing.assert_array_equal(val[idx >= 0], np.float32([0, 0, 0.5, 1, 1, 0, 1, 0]))


def test_sigmoid_saturates_where_python_overflows():
    """finite -g(x - b) above ~709.78: math.exp raises in the Python
    converter; the native hasher gives 0.0 (exp = inf), and 1.0 at the other
    end, as the reference's C++ does"""
    cfg = fc.cfg([("*", "sig", "_n")], rules=[{"key": "*_n", "type": "num"}])
    conv = DatumToFvConverter(cfg)
    d = sc.datum([], [sc.npair(b"k", -2000.0, "f64"), sc.npair(b"k", 2000.0, "f64")])
    with pytest.raises(OverflowError):
        conv.convert(Datum.from_msgpack(msgpack.unpackb(d, raw=True)))
    (idx, val), = sc.native_rows(conv, [d])
    np.testing.assert_array_equal(val[idx >= 0], np.float32([0.0, 1.0]))


def test_sigmoid_saturation_equals_the_native_wide_twin(tmp_path):
    """the same datum through native jubaconv (csrc/cmd/jubaconv.cpp: the wide
    converter with WideExt's filters): the *_n values it prints equal the
    fixed-slot host hasher's, 0.0 and 1.0"""
    exe = os.path.join(NATIVE_BIN, "jubaconv")
    assert os.path.exists(exe), "native tools not built"
    conv_cfg = fc.cfg([("*", "sig", "_n")], rules=[{"key": "*_n", "type": "num"}])
    p = tmp_path / "c.json"
    p.write_text(json.dumps({"converter": conv_cfg}))
    env = dict(os.environ, PATH="/nonexistent")      # no Python twin to hand the config to
    r = subprocess.run([exe, "-i", "json", "-o", "fv", "-c", str(p)], input='{"a": -2000.0, "b": 2000.0}',
                       capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stderr
    wide = dict(line.rsplit(": ", 1) for line in r.stdout.splitlines())
    assert set(wide) == {"/a_n@num", "/b_n@num"}
    conv = DatumToFvConverter(conv_cfg)
    d = sc.datum([], [sc.npair(b"/a", -2000.0, "f64"), sc.npair(b"/b", 2000.0, "f64")])
    (idx, val), = sc.native_rows(conv, [d])
    from jubatus_amd.fv_converter.hashing import feature_index
    fast = dict(zip(idx[idx >= 0].tolist(), val[idx >= 0].tolist()))
    for name, want in (("/a_n@num", 0.0), ("/b_n@num", 1.0)):
        assert float(wide[name]) == fast[feature_index(name, conv.hash_max_size)] == want


def test_matcher_boundaries_first_step():
    _host(fc.boundary_step1(), fc.boundary_datums())


@pytest.mark.parametrize("k", range(len(fc.boundary_step2())))
def test_matcher_boundaries_second_step(k):
    _host(fc.boundary_step2()[k], fc.boundary_datums())


def test_boundary_cases_do_match_something():
    """the boundary configs are not vacuous: each matching matcher of the
    first-step table fires on the key `height`, each mismatch does not"""
    conv = DatumToFvConverter(fc.boundary_step1())
    (idx, _), = sc.native_rows(conv, [sc.datum([], [sc.npair(fc.K.encode(), 1.0)])])
    n = len(fc._boundary_specs(fc.K, fc.S))
    base, derived = idx[:n] >= 0, idx[n:] >= 0
    #         prefix                              suffix                            exact
    want_d = [1, 1, 1, 1, 0, 0, 0, 0,             1, 1, 1, 1, 0, 0, 0, 0,           1, 0, 0, 0, 0]
    want_b = [1, 1, 0, 0, 0, 0, 0, 0,             0, 0, 0, 0, 0, 0, 0, 0,           0, 1, 0, 0, 0]
    assert derived.tolist() == [bool(x) for x in want_d]
    assert base.tolist() == [bool(x) for x in want_b]


# ----------------------------------------------------------- native servers
TRUNC_BOOL = fc.cfg([("*", "lin_b", "_n")], types={"lin_b": {"method": "linear_normalization", "min": 0,
                                                            "max": 10, "truncate": False}})
PACKED = dict({k: v[0] for k, v in CASES.items()}, boundary=fc.boundary_step1(),
              boundary_step2=fc.boundary_step2()[10], truncate_json_false=TRUNC_BOOL,
              no_filters=dict(sc.CONV_FV), four_star=fc.cfg([("*", "add", f"_{i}") for i in range(4)]))
ENGINES = {"classifier": {"method": "AROW", "parameter": {"regularization_weight": 1.0}},
           "regression": {"method": "PA", "parameter": {"sensitivity": 0.1, "regularization_weight": 1.0}},
           "recommender": {"method": "euclid_lsh", "parameter": {"hash_num": 64}}}


def _native_check(engine, conv, tmp_path):
    """--native-check with the rule dump -> (verdict line, rules line)"""
    exe = os.path.join(NATIVE_BIN, "juba" + engine)
    assert os.path.exists(exe), "native servers not built"
    p = tmp_path / "c.json"
    p.write_text(json.dumps(dict(ENGINES[engine], converter=conv)))
    r = subprocess.run([exe, "--native-check", "-f", str(p)], capture_output=True, text=True, timeout=30,
                       env=dict(os.environ, JUBATUS_NATIVE_CHECK_RULES="1"))
    assert r.returncode == 0, r.stderr
    verdict, rules = r.stdout.strip().splitlines()
    return verdict, rules


@pytest.mark.parametrize("name", sorted(PACKED))
def test_native_packer_equals_python_packer(name, tmp_path):
    """csrc/server/jb_server_common.hpp build_rules against
    gpu_path.GpuRuleTable on the same config: string rows, num rows and blob
    byte for byte (fails on the parent, which prints no such line and refuses
    filter configs there)"""
    conv = DatumToFvConverter(PACKED[name])
    rt = GpuRuleTable(conv)
    verdict, rules = _native_check("classifier", PACKED[name], tmp_path)
    assert verdict == "native"
    head, H, s, n, blob = rules.rsplit(" ", 4)
    assert head == "fixed-slot rules:" and int(H) == rt.H
    unhex = lambda x: b"" if x == "-" else bytes.fromhex(x)     # noqa: E731
    assert unhex(s) == bytes(rt.srules)[:32 * rt.n_srules]
    assert unhex(n) == bytes(rt.nrules)[:32 * rt.n_nrules]
    assert unhex(blob) == (bytes(rt.blob) if rt.n_srules + rt.n_nrules else b"")


@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_native_servers_take_filter_configs_on_the_fixed_slot_path(engine, tmp_path):
    """jubaclassifier, jubaregression (jb_linear_conv.hpp) and a row engine
    server (jb_row_engine.hpp) try build_rules first: it accepts the filter
    configs (the parent answered "num_filter_rules need the host converter"
    there and fell back to the wide converter) and still refuses what the
    fixed-slot path does not serve. --native-check prints what it prints for
    a filter-free config."""
    plain, _ = _native_check(engine, {"num_rules": [{"key": "*", "type": "num"}], "hash_max_size": fc.H},
                             tmp_path)
    assert plain == "native"
    for name in ("gauss", "chain3", "with_strings"):
        verdict, rules = _native_check(engine, CASES[name][0], tmp_path)
        assert verdict == plain and "host converter" not in verdict
        assert rules.startswith("fixed-slot rules: ") and not rules.startswith("fixed-slot rules: no")
        n_rows = len(rules.rsplit(" ", 2)[1]) // 64
        assert n_rows == GpuRuleTable(DatumToFvConverter(CASES[name][0])).n_nrules
    five = fc.cfg([("*", "add", f"_{i}") for i in range(5)])
    _, rules = _native_check(engine, five, tmp_path)
    assert rules.startswith("fixed-slot rules: no: ") and "filter chains" in rules
    bad = fc.cfg([("*", "g", "_n")], types={"g": {"method": "gaussian_normalization", "average": 0,
                                                  "standard_deviation": 0}})
    verdict, rules = _native_check(engine, bad, tmp_path)
    assert "standard_deviation must be > 0" in rules
