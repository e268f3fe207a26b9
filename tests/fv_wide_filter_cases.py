"""Num filters on the wide rule set: configs, datums and the comparison with
the Python converter, shared by test_fv_wide_filters.py (CPU: HostFvWide,
csrc/native/jb_hostfv_wide.hpp) and test_gpu_fv_wide_filters.py (GPU:
csrc/hip/fv_wide.hip). No GPU use.

The configs are those of tests/fv_filter_cases.py, each with a `space` string
rule and combination rules added, which is what takes them off the fixed-slot
path. The definition is fv_converter/converter.py `_convert`; a datum's
features are compared with it as a SEQUENCE (the combination pairs i < j hang
on the order), value by value:

* `num` rows without a sigmoid in the chain: bit-equal fp32 (the same fp64
  operations, one rounding);
* `num` rows with a sigmoid_normalization in the chain: 1 fp32 ulp (two `exp`
  implementations, fv_filter_cases.py);
* `log` rows, string features and combination values: the rtol / atol
  tests/test_fv_wide.py applies to the same code (host 1e-6 / 1e-7, device
  2e-6 / 1e-7).
"""
import random

import msgpack
import numpy as np

import fv_filter_cases as fc
import scan_cases as sc
from jubatus_amd.fv_converter.datum import Datum

HOST_TOL = (1e-6, 1e-7)       # test_fv_wide.py test_native_wide_equals_python_converter
DEVICE_TOL = (2e-6, 1e-7)     # test_fv_wide.py test_device_wide_converter_equals_host

SPACE = {"key": "*", "type": "space", "sample_weight": "tf", "global_weight": "bin"}
# a right key that only derived names match, an exact derived name on the
# left, a string feature against derived values
COMBS = [{"key_left": "*", "key_right": "*_g@num", "type": "mul"},
         {"key_left": "height_n@num", "key_right": "*", "type": "add"},
         {"key_left": "s$*", "key_right": "*_a@num", "type": "add"}]
STAR_ADD = [{"key_left": "*", "key_right": "*", "type": "add"}]
STAR_MUL = [{"key_left": "*", "key_right": "*", "type": "mul"}]


def widen(cfg, combs=COMBS):
    """the config with a `space` string rule and combination rules (what
    fc.cfg(..., string_rules=..., combination_rules=...) builds)"""
    c = dict(cfg)
    c["string_rules"] = list(cfg.get("string_rules") or []) + [SPACE]
    c["combination_rules"] = list(combs)
    return c


def method_cases():
    """name -> (wide config, 1 where a sigmoid is among the filters)"""
    return {name: (widen(cfg), sig) for name, (cfg, sig) in fc.method_cases().items()}


def datums(sigmoid):
    """fc.datums() (|x| kept small where the Python converter's math.exp would
    overflow), a datum that repeats a key, one without num values, and the
    non-finite values"""
    values = [v for v in fc.VALUES if abs(v[0]) <= 500] if sigmoid else fc.VALUES
    out = fc.datums(values)
    out.append(sc.datum([sc.spair(b"s", b"x y x")],
                        [sc.npair(b"height", 1.5), sc.npair(b"height", -2.0, "f32"),
                         sc.npair(b"t", 3, "u8"), sc.npair(b"height", 1.5)]))
    out.append(sc.datum([sc.spair(b"s", b"a b"), sc.spair(b"u", b"")], []))
    out += fc.datums(fc.SPECIAL, keys=[b"height", b"t"], per=2)
    return out


def body(datum_bytes):
    return sc.enc_arr(len(datum_bytes), "auto") + b"".join(datum_bytes)


def host_wide(conv, H=None):
    """HostFvWide over the converter's WideRuleTable, no WideExt"""
    from jubatus_amd._native import native
    from jubatus_amd.fv_converter.gpu_path import WideRuleTable
    rt = WideRuleTable(conv)
    h = native().HostFvWide(rt.srules, rt.n_srules, rt.nrules, rt.n_nrules, rt.crules,
                            rt.n_crules, rt.blob, H or rt.H)
    if h.needs_weights():
        df, diff, counts = conv.weights.arrays()
        h.set_weights(df.ctypes.data, diff.ctypes.data, counts.ctypes.data)
    return h


def host_rows(h, datum_bytes, update=False):
    """HostFvWide on a list of encoded datums -> per datum (idx, val), in order"""
    n = len(datum_bytes)
    cap = 1 << 16
    while True:
        idx = np.empty(cap, np.int32)
        val = np.empty(cap, np.float32)
        rp = np.zeros(n + 1, np.int64)
        got, slots, err = h.hash([body(datum_bytes)], idx.ctypes.data, val.ctypes.data,
                                 rp.ctypes.data, n, cap, update)
        if err == 2:
            cap *= 4
            continue
        assert err == 0 and got == n, (err, got)
        return [(idx[rp[i]:rp[i + 1]].copy(), val[rp[i]:rp[i + 1]].copy()) for i in range(n)]


class Expected:
    """one datum through the Python converter: indices and float32 values in
    order, and per position how close a native value has to be"""
    EXACT, ULP1, CLOSE = 0, 1, 2

    def __init__(self, conv, datum_bytes):
        d = Datum.from_msgpack(msgpack.unpackb(datum_bytes, raw=True))
        fv = conv.convert(d)
        idx, val = conv.hashed(fv)
        self.names = [n for n, _ in fv]
        self.idx = np.asarray(idx, np.int32)
        with np.errstate(over="ignore"):
            self.val = np.asarray(val, np.float64).astype(np.float32)
        sv, _ = conv._filtered(d)
        n_str = len(conv._string_features(sv))
        nv = fc.filtered_with_sigmoid(conv, d)
        seq = [(k, sig, r) for k, _, sig in nv for r in conv.num_rules if r.matcher.match(k)]
        kind = np.full(len(fv), self.CLOSE, np.int8)
        for p, (k, sig, r) in enumerate(seq, start=n_str):
            assert self.names[p] == f"{k}@{r.type_name}"     # block order: chain, value, rule
            if r.kind == "num":
                kind[p] = self.ULP1 if sig else self.EXACT
        self.n_str, self.n_num = n_str, len(seq)
        self.kind = kind


def check_row(exp, idx, val, tol):
    """one datum's native features (idx < 0 slots already dropped) against the
    Python converter's, position by position"""
    np.testing.assert_array_equal(idx, exp.idx)
    val = np.asarray(val, np.float32)
    want = exp.val
    np.testing.assert_array_equal(np.isnan(val), np.isnan(want))
    ok = ~np.isnan(want)
    fin = ok & np.isfinite(want) & np.isfinite(val)
    exact = ok & ((exp.kind == Expected.EXACT) | ~fin)        # infinities are exact everywhere
    np.testing.assert_array_equal(val[exact].view(np.uint32), want[exact].view(np.uint32))
    ulp = fin & (exp.kind == Expected.ULP1)
    if ulp.any():
        assert (sc.ulp_diff(val[ulp], want[ulp]) <= 1).all()
    close = fin & (exp.kind == Expected.CLOSE)
    np.testing.assert_allclose(val[close], want[close], rtol=tol[0], atol=tol[1])


def boundary_cases():
    """fc.boundary_step1() and every fc.boundary_step2() config with an added
    `*` x `*` add combination: every derived name goes through the name
    matchers' neighbours, and through the pair loop"""
    return [widen(c, STAR_ADD) for c in [fc.boundary_step1()] + fc.boundary_step2()]


# ---- a driver config: every number normalised, the normalised values multiplied
DRIVER = {"num_filter_types": {"z": {"method": "gaussian_normalization", "average": 0.5,
                                     "standard_deviation": 2.0}},
          "num_filter_rules": [{"key": "*", "type": "z", "suffix": "_z"}],
          "string_rules": [{"key": "*", "type": "space", "sample_weight": "tf", "global_weight": "bin"}],
          "num_rules": [{"key": "*", "type": "num"}],
          "combination_rules": [{"key_left": "*_z@num", "key_right": "*_z@num", "type": "mul"}],
          "hash_max_size": 1 << 18}


def driver_rows(n=48, seed=6):
    rng = random.Random(seed)
    return [(f"r{i}", {"a": 4.0 * (i % 8) + rng.random(), "b": 5.0 * (i // 8) + rng.random(),
                       "t": f"w{i % 5} w{rng.randrange(3)}"}) for i in range(n)]
