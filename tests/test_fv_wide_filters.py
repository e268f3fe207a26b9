"""Num filters on the wide rule set, host side: eligibility and the rule
tables (fv_converter/gpu_path.py wide_eligible / WideRuleTable), the native
host converter HostFvWide (csrc/native/jb_hostfv_wide.hpp) built from a table
with derived rows against the Python converter as a sequence, the document
statistics next to filters, and the CPU drivers that pick the path up. Cases
and tolerances: tests/fv_wide_filter_cases.py. CPU."""
import os
import struct
import subprocess

import msgpack
import numpy as np
import pytest

import fv_filter_cases as fc
import fv_wide_filter_cases as wc
import scan_cases as sc
import test_fv_wide as tw
from jubatus_amd.fv_converter import gpu_path
from jubatus_amd.fv_converter.converter import DatumToFvConverter
from jubatus_amd.fv_converter.datum import Datum
from jubatus_amd.fv_converter.gpu_path import (WideRuleTable, fast_eligible, gpu_eligible,
                                               wide_eligible)

GAUSS = [("height", "gauss", "_z")]
NGRAM = {"string_types": {"bi": {"method": "ngram", "char_num": "2"}},
         "string_rules": [{"key": "*", "type": "bi", "sample_weight": "tf", "global_weight": "bin"}]}
IDF = {"string_rules": [{"key": "*", "type": "space", "sample_weight": "tf", "global_weight": "idf"}]}
COMB = {"combination_rules": [{"key_left": "*", "key_right": "*_z@num", "type": "mul"}]}


# ------------------------------------------------------------- eligibility
@pytest.mark.parametrize("extra", [NGRAM, IDF, COMB], ids=["ngram", "idf", "combination"])
def test_builtin_filter_with_a_wide_rule_is_eligible(extra):
    """fails on the parent: wide_eligible refused every num filter"""
    conv = DatumToFvConverter(fc.cfg(GAUSS, **extra))
    assert not fast_eligible(conv)
    assert wide_eligible(conv) and gpu_eligible(conv)
    rt = WideRuleTable(conv)
    assert (rt.n_base, rt.n_chains, rt.n_nrules) == (1, 1, 2)
    base, derived = (gpu_path._RULE.unpack_from(rt.nrules, 32 * i) for i in range(2))
    assert base[5] == 0 and base[7] == 0
    assert derived[5] == gpu_path._DERIVED_ROW and derived[7] % 8 == 0
    blob = bytes(rt.blob)
    assert blob[derived[3]:derived[3] + derived[4]] == b"_z@num"
    assert struct.unpack_from("<ii", blob, derived[7]) == (1, 2)


def test_what_the_wide_path_still_refuses():
    star = [{"key": "*", "type": "num"}]
    # a string filter
    c = fc.cfg(GAUSS, **COMB)
    c["string_filter_types"] = {"detag": {"method": "regexp", "pattern": "<[^>]*>", "replace": ""}}
    c["string_filter_rules"] = [{"key": "*", "type": "detag", "suffix": "-d"}]
    assert not wide_eligible(DatumToFvConverter(c))
    # a plug-in filter
    c = dict({"num_filter_types": {"p": {"method": "dynamic", "path": "x.so", "function": "create"}},
              "num_filter_rules": [{"key": "*", "type": "p", "suffix": "_p"}], "num_rules": star}, **COMB)

    class Loader:
        def create(self, kind, params):
            return lambda x: x
    conv = DatumToFvConverter(c, plugin_loader=Loader())
    assert not wide_eligible(conv) and not gpu_eligible(conv)
    with pytest.raises(ValueError):
        WideRuleTable(conv)
    # a regex filter key
    assert not wide_eligible(DatumToFvConverter(fc.cfg([("/^h/", "add", "_n")], **COMB)))
    # the chain cap: five `*` filters make 31 chains, four make 15
    five = DatumToFvConverter(fc.cfg([("*", "add", f"_{i}") for i in range(5)], **COMB))
    assert not wide_eligible(five) and not gpu_eligible(five)
    rules = [{"key": "*", "type": "num"}, {"key": "h*", "type": "log"}]
    four = DatumToFvConverter(fc.cfg([("*", "add", f"_{i}") for i in range(4)], rules=rules, **COMB))
    assert wide_eligible(four)
    rt = WideRuleTable(four)
    assert rt.n_nrules == 16 * len(four.num_rules) and (rt.n_base, rt.n_chains) == (2, 15)


def test_both_tables_pack_the_same_num_rows():
    """one packing helper: a config both paths take packs the same num rule
    rows and blob in GpuRuleTable and WideRuleTable"""
    for name in ("chain3", "four_star", "exact_chain", "log"):
        conv = DatumToFvConverter(fc.method_cases()[name][0])
        g, w = gpu_path.GpuRuleTable(conv), WideRuleTable(conv)
        assert bytes(g.nrules) == bytes(w.nrules) and bytes(g.blob) == bytes(w.blob)
        assert (g.n_base, g.n_chains) == (w.n_base, w.n_chains)


# --------------------------------------------------- filter-free configs
def _parent_wide_tables(conv):
    """the packing of WideRuleTable before filters were served, literally"""
    RULE = struct.Struct("<iiiiiifi")
    KIND = {"all": 0, "prefix": 1, "suffix": 2, "exact": 3}
    SPLIT = {"str": 0, "ngram": 1, "space": 2}
    SW = {"bin": 0, "tf": 1, "log_tf": 2}
    GW = {"bin": 0, "idf": 1, "bm25": 2}
    blob = bytearray()

    def put(b):
        off = len(blob)
        blob.extend(b)
        return off, len(b)

    srows, nrows, crows = [], [], []
    for r in conv.string_rules:
        mo, ml = put(r.matcher.arg.encode())
        so, sl = put(r.suffix.encode())
        vk = SPLIT[r.split_kind] | SW[r.sw] << 4 | GW[r.gw] << 8
        srows.append(RULE.pack(KIND[r.matcher.kind], mo, ml, so, sl, vk, 0.0, r.split_n))
    for r in conv.num_rules:
        mo, ml = put(r.matcher.arg.encode())
        so, sl = put(f"@{r.type_name}".encode())
        nrows.append(RULE.pack(KIND[r.matcher.kind], mo, ml, so, sl, 1 if r.kind == "log" else 0, 0.0, 0))
    for ml_, mr_, tname, _ in conv.combination_rules:
        lo, ll = put(ml_.arg.encode())
        so, sl = put(f"/{tname}".encode())
        ro, rl = put(mr_.arg.encode())
        crows.append(RULE.pack(KIND[ml_.kind], lo, ll, so, sl,
                               {"add": 0, "mul": 1}[conv.combination_methods[tname]], 0.0, 0))
        crows.append(RULE.pack(KIND[mr_.kind], ro, rl, 0, 0, 0, 0.0, 0))
    return tuple(b"".join(x) or b"\0" * 32 for x in (srows, nrows, crows)) + (bytes(blob) or b"\0",)


@pytest.mark.parametrize("name", tw.CONFIGS + ["extra"])
def test_filter_free_tables_and_converter_are_unchanged(name):
    conv = tw._conv(name)
    rt = WideRuleTable(conv)
    assert (bytes(rt.srules), bytes(rt.nrules), bytes(rt.crules), bytes(rt.blob)) == \
        _parent_wide_tables(conv)
    assert rt.n_nrules == rt.n_base == len(conv.num_rules) and rt.n_chains == 0
    for r in range(rt.n_nrules):
        assert not gpu_path._RULE.unpack_from(rt.nrules, 32 * r)[5] & gpu_path._DERIVED_ROW
    ds = tw.datums(30, seed=5)
    cpy, cnat = tw._conv(name), tw._conv(name)
    h = tw.native_wide(cnat)
    for update in (True, False):
        for (ia, va), (ib, vb) in zip(tw.run_python(cpy, ds, update), tw.run_native(h, ds, update)):
            np.testing.assert_array_equal(ia, ib)
            np.testing.assert_allclose(va, vb, rtol=1e-6, atol=1e-7)


# ------------------------------- HostFvWide against the Python converter
def _host_check(cfg, datums):
    conv = DatumToFvConverter(cfg)
    assert wide_eligible(conv) and not fast_eligible(conv)
    rows = wc.host_rows(wc.host_wide(conv), datums)
    n_num = n_comb = 0
    for d, (idx, val) in zip(datums, rows):
        exp = wc.Expected(conv, d)
        assert (idx >= 0).all()                  # the host twin emits hits only
        wc.check_row(exp, idx, val, wc.HOST_TOL)
        n_num += exp.n_num
        n_comb += len(exp.idx) - exp.n_str - exp.n_num
    return n_num, n_comb


CASES = wc.method_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_wide_equals_python_converter_in_order(name):
    """fails on the parent (WideRuleTable raised ValueError)"""
    cfg, sigmoid = CASES[name]
    n_num, n_comb = _host_check(cfg, wc.datums(sigmoid))
    assert n_num > 0
    if name in ("chain2", "four_star", "exact_chain", "gauss", "add", "with_strings"):
        assert n_comb > 0                        # `*_g@num`, `height_n@num`, `*_a@num` fire


BOUNDARY = wc.boundary_cases()


@pytest.mark.parametrize("k", range(len(BOUNDARY)))
def test_host_wide_matcher_boundaries(k):
    n_num, n_comb = _host_check(BOUNDARY[k], fc.boundary_datums())
    assert n_num > 0 and n_comb > 0


def test_order_is_chain_block_then_value_then_rule():
    """pinned by hand: two `*` filters, values a and b, rule `*`"""
    cfg = fc.cfg([("*", "add", "_0"), ("*", "gauss", "_1")], combination_rules=wc.STAR_MUL)
    conv = DatumToFvConverter(cfg)
    d = sc.datum([], [sc.npair(b"a", 1.0), sc.npair(b"b", 2.0)])
    names = [f"{n}@num" for n in ("a", "b", "a_0", "b_0", "a_1", "b_1", "a_0_1", "b_0_1")]
    want = names + [f"{names[i]}&{names[j]}/mul" for i in range(8) for j in range(i + 1, 8)]
    from jubatus_amd.fv_converter.hashing import feature_index
    (idx, val), = wc.host_rows(wc.host_wide(conv), [d])
    assert idx.tolist() == [feature_index(n, conv.hash_max_size) for n in want]
    assert wc.Expected(conv, d).names == want    # and the definition agrees
    g = lambda x: (x - 1.25) / 3.1               # noqa: E731
    base = [1.0, 2.0, 3.5, 4.5, g(1.0), g(2.0), g(3.5), g(4.5)]
    np.testing.assert_array_equal(val[:8], np.float32(base))


def test_sigmoid_saturates_where_python_overflows():
    cfg = fc.cfg([("*", "sig", "_n")], rules=[{"key": "*_n", "type": "num"}],
                 combination_rules=wc.STAR_ADD)
    conv = DatumToFvConverter(cfg)
    d = sc.datum([], [sc.npair(b"k", -2000.0, "f64"), sc.npair(b"k", 2000.0, "f64")])
    (idx, val), = wc.host_rows(wc.host_wide(conv), [d])
    np.testing.assert_array_equal(val, np.float32([0.0, 1.0, 1.0]))


# ---------------------------------------------------- document statistics
def test_filters_leave_the_document_statistics_alone():
    """a bm25 string rule beside filters: only string features carry a global
    weight and count toward the document length"""
    cfg = fc.cfg([("n*", "gauss", "_g"), ("*", "add", "_a")],
                 rules=[{"key": "*", "type": "num"}, {"key": "*_g", "type": "log"}],
                 string_rules=[{"key": "t*", "type": "space", "sample_weight": "log_tf",
                                "global_weight": "bm25"}],
                 combination_rules=[{"key_left": "t*", "key_right": "*_g@log", "type": "mul"}],
                 hash_max_size=1 << 16)
    cpy, cnat = DatumToFvConverter(cfg), DatumToFvConverter(cfg)
    assert wide_eligible(cnat) and cnat.uses_global_weight
    h = tw.native_wide(cnat)
    ds = tw.datums(60, seed=11)
    for update in (True, False):
        for (ia, va), (ib, vb) in zip(tw.run_python(cpy, ds, update), tw.run_native(h, ds, update)):
            np.testing.assert_array_equal(ia, ib)
            np.testing.assert_allclose(va, vb, rtol=1e-6, atol=1e-7)
    assert cpy.weights.doc_count == cnat.weights.doc_count == 60
    assert cpy.weights.total_len == cnat.weights.total_len > 0
    np.testing.assert_array_equal(cpy.weights.df, cnat.weights.df)
    np.testing.assert_array_equal(cpy.weights.diff, cnat.weights.diff)


# ------------------------------------------------------------ CPU drivers
def test_recommender_takes_the_host_wide_converter():
    """inverted_index rows through HostFvWide == a twin forced onto the Python
    converter; on the parent _hasher() is None for this config"""
    from jubatus_amd.models.recommender import Recommender
    a = Recommender("inverted_index", {}, DatumToFvConverter(wc.DRIVER))
    b = Recommender("inverted_index", {}, DatumToFvConverter(wc.DRIVER))
    assert type(a._hasher()).__name__ == "HostFvWide"
    b._host_hasher = False                       # the per-datum Python converter
    assert b._hasher() is None
    rows = wc.driver_rows()
    a.set_rows(rows)
    b.set_rows(rows)
    for rid, _ in rows:
        (ia, va), (ib, vb) = a.rows.fv[a.rows.slot(rid)], b.rows.fv[b.rows.slot(rid)]
        assert list(ia) == list(ib) and len(ia) >= 2 + 2 + 1     # a b a_z b_z a_z&b_z + tokens
        np.testing.assert_allclose(va, vb, rtol=1e-6, atol=1e-7)
    for q in ({"a": 9.0, "b": 11.0}, {"a": 30.0, "b": 0.5, "t": "w1"}, {"a": 17.0}):
        ra, rb = a.similar_row_from_datum(q, 4), b.similar_row_from_datum(q, 4)
        assert [r for r, _ in ra] == [r for r, _ in rb]
        np.testing.assert_allclose([s for _, s in ra], [s for _, s in rb], rtol=1e-5)


def test_clustering_takes_the_host_wide_converter():
    from jubatus_amd.models.clustering import Clustering
    a = Clustering("kmeans", {"k": 2, "bucket_size": 1000}, DatumToFvConverter(wc.DRIVER))
    b = Clustering("kmeans", {"k": 2, "bucket_size": 1000}, DatumToFvConverter(wc.DRIVER))
    assert type(a._native).__name__ == "HostFvWide"
    b._native = None                             # the per-datum Python converter
    pts = [Datum(d) for _, d in wc.driver_rows(24)]
    assert a.push(pts) and b.push(pts)
    pa, pb = a.pending, b.pending
    assert len(pa) == len(pb) == 24
    np.testing.assert_array_equal(pa.rp, pb.rp)
    np.testing.assert_array_equal(pa.key, pb.key)
    np.testing.assert_allclose(pa.val, pb.val, rtol=1e-6, atol=1e-7)
    names = {a._names[int(k)] for k in pa.key}
    assert {"a_z@num", "b_z@num", "a_z@num&b_z@num/mul"} <= names
    assert names == {b._names[int(k)] for k in pb.key}


# ---------------------------------------------------- instrumented host twin
def test_host_wide_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/tools/jb_hostfv_wide_check.cpp (HostFvWide in a program of its own)
    built with -fsanitize=address,undefined over tables with derived rows, a
    bm25 rule and combinations: no report, and the features it prints are the
    Python converter's, name by name"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(gpu_path.__file__)), "..", "csrc")
    exe = str(tmp_path / "jb_hostfv_wide_check")
    r = subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-std=c++17", "-pthread", "-Wall",
                        f"-I{os.path.join(csrc, 'native')}",
                        os.path.join(csrc, "tools", "jb_hostfv_wide_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:exitcode=66",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    bm25 = {"key": "s*", "type": "space", "sample_weight": "log_tf", "global_weight": "bm25"}
    runs = [(wc.widen(fc.method_cases()[name][0]), wc.datums(sig), False)
            for name, sig in (("four_star", 0), ("chain3", 1), ("exact_chain", 0), ("log", 0))]
    runs.append((wc.widen(dict(fc.boundary_step2()[10], string_rules=[bm25]), wc.STAR_ADD),
                 fc.boundary_datums() + wc.datums(0), True))
    for cfg, datums, update in runs:
        conv = DatumToFvConverter(cfg)
        rt = WideRuleTable(conv)
        tables = struct.pack("<Qiiii", rt.H, rt.n_srules, rt.n_nrules, rt.n_crules, rt.blob.size) + \
            bytes(rt.srules)[:32 * rt.n_srules] + bytes(rt.nrules)[:32 * rt.n_nrules] + \
            bytes(rt.crules)[:64 * rt.n_crules] + bytes(rt.blob)
        (tmp_path / "tables").write_bytes(tables)
        (tmp_path / "body").write_bytes(wc.body(datums))
        r = subprocess.run([exe, str(tmp_path / "tables"), str(tmp_path / "body")] + ["update"] * update,
                           capture_output=True, timeout=120, env=env)
        err = r.stderr.decode("utf-8", "replace")
        assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
        got = r.stdout.split(b"--\n")
        assert len(got) == len(datums) + 1
        for d, lines in zip(datums, got):
            dat = Datum.from_msgpack(msgpack.unpackb(d, raw=True))
            fv = conv.convert_and_update_weight(dat) if update else conv.convert(dat)
            names = [ln.split(b" ", 2)[2] for ln in lines.splitlines()]
            assert names == [n.encode() for n, _ in fv]
            vals = np.array([int(ln.split(b" ", 2)[1], 16) for ln in lines.splitlines()],
                            np.uint32).view(np.float32)
            with np.errstate(over="ignore"):
                want = np.asarray([v for _, v in fv], np.float64).astype(np.float32)
            np.testing.assert_allclose(vals, want, rtol=1e-6, atol=1e-7)
        if update:
            assert got[-1].split() == [b"counts", str(conv.weights.doc_count).encode(),
                                       str(conv.weights.total_len).encode()]
