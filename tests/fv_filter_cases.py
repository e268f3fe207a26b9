"""Num filter configs, datums and the comparison with the Python converter,
shared by test_fv_num_filters.py (CPU: HostFvHasher) and
test_gpu_fv_num_filters.py (GPU: fv_hash.hip). No GPU use.

The definition is fv_converter/converter.py `_filtered` + the num rules; a
row set (idx, val, -1 slots included) of one datum is compared with it as a
sorted multiset of (index, float32 value):

* `num` over add / linear_normalization / gaussian_normalization: bit-equal
  (the same fp64 operations, one rounding to fp32);
* `num` over a chain that holds a sigmoid_normalization: 1 fp32 ulp (two `exp`
  implementations, each within a few fp64 ulp, move the rounding at a tie);
  the other chains of the same config stay bit-equal;
* `log`: 3 ulp of float32(log(max(1, float64(float32(y))))), the limit of
  test_gpu_scan_edges.py, y the Python converter's filtered value.
"""
import math
import struct

import msgpack
import numpy as np

import scan_cases as sc
from jubatus_amd.fv_converter.datum import Datum
from jubatus_amd.fv_converter.hashing import feature_index

H = 1 << 18

TYPES = {
    "add": {"method": "add", "value": "2.5"},
    "lin": {"method": "linear_normalization", "min": -3, "max": 7},
    "lin_raw": {"method": "linear_normalization", "min": "-3", "max": "7", "truncate": "false"},
    "gauss": {"method": "gaussian_normalization", "average": 1.25, "standard_deviation": 3.1},
    "sig": {"method": "sigmoid_normalization", "gain": 0.7, "bias": 1.5},
    "sig_neg": {"method": "sigmoid_normalization", "gain": -1.3, "bias": -0.25},
}


def cfg(filters, rules=({"key": "*", "type": "num"},), types=TYPES, **kw):
    """filters: [(key, type, suffix)]"""
    c = {"num_filter_types": {t: types[t] for _, t, _ in filters},
         "num_filter_rules": [{"key": k, "type": t, "suffix": s} for k, t, s in filters],
         "num_rules": list(rules), "hash_max_size": H}
    c.update(kw)
    return c


# values below, inside and above [min, max] = [-3, 7] of `lin`, every number
# form; |gain * (x - bias)| stays far below 700 for the Python converter
VALUES = [(-10.5, "f64"), (-3, "i8"), (-3.0000001, "f64"), (0, "posfix"), (2.25, "f32"),
          (6.999, "f64"), (7, "u8"), (7.5, "f32"), (400, "u16"), (-200, "i16"), (1e-3, "f64"),
          (12345.678, "f64"), (-31, "negfix"), (70000, "u32"), (-5000000000, "i64"), (2**40, "u64")]
SPECIAL = [(math.nan, "f32"), (math.nan, "f64"), (math.inf, "f32"), (-math.inf, "f64"),
           (math.inf, "f64"), (-0.0, "f64")]
KEYS = [b"height", b"heigh", b"xheight", b"height_nrm", b"", b"t", b"height_a", "高さ".encode()]


def datums(values=VALUES, keys=KEYS, per=3):
    """encoded datums: `per` num values each, keys and values cycling; one
    with no num values, one with a string value besides"""
    out, j = [], 0
    for i in range(0, len(values), per):
        nps = []
        for x, form in values[i:i + per]:
            nps.append(sc.npair(keys[j % len(keys)], x, form))
            j += 1
        out.append(sc.datum([], nps, top=2 + (i // per) % 2))
    out.append(sc.datum([], []))
    out.append(sc.datum([sc.spair(b"s", b"v")], [sc.npair(keys[0], 1.5)]))
    return out


def filtered_with_sigmoid(conv, d):
    """the num values of converter.py `_filtered`, each with a flag: a
    sigmoid_normalization produced it or one of the values it derives from"""
    types = conv.config.get("num_filter_types") or {}
    methods = [types[r["type"]]["method"] for r in conv.config.get("num_filter_rules") or []]
    nv = [(k, x, False) for k, x in d.num_values]
    for (m, f, suffix), method in zip(conv.num_filters, methods):
        for k, v, sig in list(nv):
            if m.match(k):
                nv.append((k + suffix, float(f(v)), sig or method == "sigmoid_normalization"))
    want = conv._filtered(d)[1]          # the definition: same keys, same bits
    assert [(k, struct.pack("<d", y)) for k, y, _ in nv] == [(k, struct.pack("<d", y)) for k, y in want]
    return nv


def expected(conv, dobj):
    """[(idx, float32 value, tolerance in ulps)] of one datum object, from the
    Python converter: 3 ulp under `log`, 1 ulp where a sigmoid is in the
    value's chain, bit-equal everywhere else"""
    d = Datum.from_msgpack(dobj)
    fv = conv.convert(d)
    idx, val = conv.hashed(fv)
    sv, _ = conv._filtered(d)
    nv = filtered_with_sigmoid(conv, d)
    n_str = len(conv._string_features(sv))
    seq = [(k, y, sig, r) for k, y, sig in nv for r in conv.num_rules if r.matcher.match(k)]
    assert len(seq) == len(fv) - n_str
    out = [(i, np.float32(v), 0) for i, v in zip(idx[:n_str], val[:n_str])]
    with np.errstate(over="ignore"):
        for (k, y, sig, r), (name, _), i in zip(seq, fv[n_str:], idx[n_str:]):
            assert name == f"{k}@{r.type_name}" and i == feature_index(name, conv.hash_max_size)
            if r.type_name == "log":
                out.append((i, sc.log_reference(np.asarray([y], np.float64))[0], 3))
            else:
                out.append((i, np.float32(y), 1 if sig else 0))
    return out


def _key(t):
    i, v = int(t[0]), float(t[1])
    return (i, v != v, 0.0 if v != v else v)


def compare(conv, datum_bytes, rows):
    """rows: per datum (idx, val) slots -> the largest distance met, in ulps"""
    worst = 0
    assert len(rows) == len(datum_bytes)
    for n, (b, (idx, val)) in enumerate(zip(datum_bytes, rows)):
        want = sorted(expected(conv, msgpack.unpackb(b, raw=True)), key=_key)
        m = idx >= 0
        assert (val[~m] == 0).all()
        got = sorted(zip(idx[m].tolist(), val[m].tolist()), key=_key)
        assert [g[0] for g in got] == [w[0] for w in want], n
        for (gi, gv), (wi, wv, tol) in zip(got, want):
            gv, wv = np.float32(gv), np.float32(wv)
            if wv != wv or gv != gv:
                assert wv != wv and gv != gv, (n, gi, gv, wv)
            elif tol == 0 or np.isinf(gv) or np.isinf(wv):
                assert gv.view(np.uint32) == wv.view(np.uint32), (n, gi, gv, wv)
            else:
                dist = int(sc.ulp_diff(np.asarray([gv]), np.asarray([wv]))[0])
                assert dist <= tol, (n, gi, gv, wv, dist)
                worst = max(worst, dist)
    return worst


def row_kinds(rt):
    """per row of a GpuRuleTable's num rule table: (a `log` row, a row whose
    chain programme holds a sigmoid_normalization step)"""
    from jubatus_amd.fv_converter import gpu_path
    blob = bytes(rt.blob)
    is_log, has_sig = [], []
    for r in range(rt.n_nrules):
        row = gpu_path._RULE.unpack_from(rt.nrules, gpu_path._RULE.size * r)
        is_log.append(bool(row[5] & 1))
        sig = False
        if row[5] & gpu_path._DERIVED_ROW:
            n_steps, _ = struct.unpack_from("<ii", blob, row[7])
            sig = any(gpu_path._STEP.unpack_from(blob, row[7] + 8 + gpu_path._STEP.size * j)[4] ==
                      gpu_path._METHOD["sigmoid_normalization"] for j in range(n_steps))
        has_sig.append(sig)
    return np.array(is_log, bool), np.array(has_sig, bool)


# ---- configs: name -> (config, 1 where a sigmoid is among the filters: |x| stays small there)
def method_cases():
    out = {}
    for t in TYPES:
        out[t] = (cfg([("*", t, "_n")]), 1 if t.startswith("sig") else 0)
    # every chain of length 1..3 fires: 7 derived values per value
    out["chain2"] = (cfg([("*", "add", "_a"), ("*", "gauss", "_g")]), 0)
    out["chain3"] = (cfg([("*", "add", "_a"), ("*", "lin_raw", "_l"), ("*", "sig", "_s")]), 1)
    # the same feature twice (empty suffix), thrice with two of them
    out["empty_suffix"] = (cfg([("*", "add", "")]), 0)
    out["empty_suffix2"] = (cfg([("*", "add", ""), ("*", "gauss", "")]), 0)
    out["log"] = (cfg([("*", "add", "_a"), ("*", "lin_raw", "_l")],
                      rules=[{"key": "*", "type": "log"}, {"key": "*_l", "type": "num"}]), 0)
    out["log_big"] = (cfg([("*", "gauss", "_g")], rules=[{"key": "*", "type": "log"}],
                          types={"gauss": {"method": "gaussian_normalization", "average": -7.0,
                                           "standard_deviation": 1e-3}}), 0)
    # a rule that sees only derived keys, one that sees only an original
    out["derived_only"] = (cfg([("*", "gauss", "_n")], rules=[{"key": "*_n", "type": "num"}]), 0)
    out["original_only"] = (cfg([("*", "gauss", "_n")], rules=[{"key": "height", "type": "num"},
                                                               {"key": "t", "type": "log"}]), 0)
    # 15 chains: a blob above fv_hash.hip's kBlobCap = 1024 bytes, read from
    # global memory instead of LDS
    out["four_star"] = (cfg([("*", "add", "_a"), ("*", "lin_raw", "_l"), ("*", "gauss", "_g"),
                             ("*_g", "add", "_2")]), 0)
    # exact filter keys: chains pruned at pack time, (0, 1) kept
    out["exact_chain"] = (cfg([("height", "add", "_a"), ("height_a", "gauss", "_g"),
                               ("t", "lin", "_x"), ("*_a", "add", "")]), 0)
    out["with_strings"] =(cfg([("height*", "lin", "_n")],
                               string_rules=[{"key": "*", "type": "str", "sample_weight": "bin",
                                              "global_weight": "bin"}]), 0)
    return out


K, S = "height", "_nrm"          # the key and suffix of the matcher boundary cases


def _boundary_specs(k, s):
    """matchers at the boundaries of key || suffix, with a mismatch next to
    each; k the key, s what was appended to it"""
    ks = k + s
    return [
        # prefix of |k| - 1, |k|, |k| + 1, |k| + |s|, one more, and mismatches
        k[:-1] + "*", k + "*", ks[:len(k) + 1] + "*", ks + "*", ks + "x*",
        k[:-1] + "x*", k + "x*", "x" + ks[1:] + "*",
        # suffix of |s| - 1, |s|, |s| + 1 (straddling), |k| + |s|, one more
        "*" + s[1:], "*" + s, "*" + ks[len(k) - 1:], "*" + ks, "*x" + ks,
        "*x" + s, "*x" + ks[1:], "*" + ks[:-1] + "x",
        # exact: the derived key, the original key, one byte short, one more
        ks, k, ks[:-1], ks + "x", "x" + ks[1:],
    ]


def boundary_step1():
    """one filter `*` + S; every boundary matcher as a num rule"""
    rules = [{"key": m, "type": "num"} for m in _boundary_specs(K, S)]
    return cfg([("*", "gauss", S)], rules=rules)


def boundary_step2():
    """-> [config]: filter 0 appends `_a`; filter 1 carries each boundary
    matcher over key || `_a` and appends `_b`; the rules match through both
    extensions (the row's suffix goes on with `_b`)"""
    rules = [{"key": "*", "type": "num"}, {"key": "*a_b", "type": "num"},
             {"key": K + "_a_*", "type": "log"}, {"key": K + "_a_b", "type": "num"},
             {"key": "*" + K[-1] + "_a", "type": "num"}]
    return [cfg([("*", "add", "_a"), (m, "lin", "_b")], rules=rules)
            for m in _boundary_specs(K, "_a")]


def boundary_datums():
    keys = [K.encode(), K[:-1].encode(), b"x" + K.encode(), (K + S).encode(), b"", b"t",
            (K + "_a").encode(), K[1:].encode(), S.encode(), S[1:].encode(), b"_a", b"a"]
    return [sc.datum([], [sc.npair(k, 0.5 + i, "f64")]) for i, k in enumerate(keys)] + \
           [sc.datum([], [sc.npair(k, 2 + i, "u8") for i, k in enumerate(keys)])]


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]
