"""Request bodies for the scanner / hasher edge tests, with an independent
oracle. No GPU use.

* hand-written msgpack encoders (`enc_raw`, `enc_num`, `enc_arr`): the test
  chooses every encoding, non-minimal ones included;
* `oracle`: what a train request holds, from `msgpack.Unpacker(raw=True)`
  and the Python converter;
* `chain_max_ext`: steps 1-3 of csrc/hip/scan.hip in Python - which bodies the
  device scan must accept (`kExtMax`);
* `build_arena`: a RequestArena with bodies at offsets chosen by hand and
  gaps that are not zero;
* the case groups shared by test_scan_edges_host.py (CPU) and
  test_gpu_scan_edges.py (GPU).
"""
import functools
import math
import random
import struct

import msgpack
import numpy as np

from jubatus_amd.fv_converter.datum import Datum

K_THREADS = 256            # csrc/hip/scan.hip kThreads: chunks per request
K_SCAN_BYTES = 27 * 1024   # kScanBytes
K_MAX_SAMPLES = 768        # kMaxSamples
K_EXT_MAX = 512            # kExtMax

RAW_FORMS = ("fix", "str8", "raw16", "raw32", "bin8", "bin16", "bin32")
ARR_FORMS = ("fix", "a16", "a32")
INT_FORMS = ("posfix", "negfix", "u8", "u16", "u32", "u64", "i8", "i16", "i32", "i64")
NUM_FORMS = INT_FORMS + ("f32", "f64")

# string rules '*' and a prefix, num rules '*' and a suffix (log): the rule
# set of tests/test_gpu_scan.py
CONV = {
    "string_rules": [{"key": "*", "type": "str", "sample_weight": "bin", "global_weight": "bin"},
                     {"key": "s1*", "type": "str", "sample_weight": "log_tf", "global_weight": "bin"}],
    "num_rules": [{"key": "*", "type": "num"}, {"key": "*1", "type": "log"}],
    "hash_max_size": 1 << 18,
}
# every key matcher kind (csrc/hip/jb_fv.hpp match_kind 0..3), num and log
CONV_FV = {
    "string_rules": [{"key": "*", "type": "str", "sample_weight": "bin", "global_weight": "bin"},
                     {"key": "ab*", "type": "str", "sample_weight": "log_tf", "global_weight": "bin"},
                     {"key": "*ab", "type": "str", "sample_weight": "tf", "global_weight": "bin"},
                     {"key": "ab", "type": "str", "sample_weight": "bin", "global_weight": "bin"}],
    "num_rules": [{"key": "*", "type": "num"}, {"key": "*", "type": "log"},
                  {"key": "ab*", "type": "log"}, {"key": "*ab", "type": "num"},
                  {"key": "ab", "type": "log"}],
    "hash_max_size": 1 << 18,
}
# two string rules that match every key: the slot bound
CONV_SLOT = {
    "string_rules": [{"key": "*", "type": "str", "sample_weight": "bin", "global_weight": "bin"},
                     {"key": "*", "type": "str", "sample_weight": "log_tf", "global_weight": "bin"}],
    "num_rules": [{"key": "*", "type": "num"}],
    "hash_max_size": 1 << 18,
}


# ------------------------------------------------------------------ encoders
def enc_raw(b: bytes, form: str = "auto") -> bytes:
    n = len(b)
    if form == "auto":           # what an old-spec client sends
        form = "fix" if n < 32 else "raw16" if n < 65536 else "raw32"
    if form == "fix":
        assert n < 32
        return bytes([0xA0 | n]) + b
    code, fmt = {"str8": (0xD9, ">B"), "raw16": (0xDA, ">H"), "raw32": (0xDB, ">I"),
                 "bin8": (0xC4, ">B"), "bin16": (0xC5, ">H"), "bin32": (0xC6, ">I")}[form]
    return bytes([code]) + struct.pack(fmt, n) + b


def enc_num(x, form: str) -> bytes:
    if form == "posfix":
        assert 0 <= x <= 127
        return bytes([int(x)])
    if form == "negfix":
        assert -32 <= x <= -1
        return bytes([int(x) & 0xFF])
    code, fmt = {"u8": (0xCC, ">B"), "u16": (0xCD, ">H"), "u32": (0xCE, ">I"), "u64": (0xCF, ">Q"),
                 "i8": (0xD0, ">b"), "i16": (0xD1, ">h"), "i32": (0xD2, ">i"), "i64": (0xD3, ">q"),
                 "f32": (0xCA, ">f"), "f64": (0xCB, ">d")}[form]
    return bytes([code]) + struct.pack(fmt, x if form in ("f32", "f64") else int(x))


def enc_arr(n: int, form: str = "fix") -> bytes:
    if form == "auto":
        form = "fix" if n < 16 else "a16" if n < 65536 else "a32"
    if form == "fix":
        assert n < 16
        return bytes([0x90 | n])
    return bytes([0xDC]) + struct.pack(">H", n) if form == "a16" else bytes([0xDD]) + struct.pack(">I", n)


_INT_RANGE = {"posfix": (0, 127), "negfix": (-32, -1), "u8": (0, 255), "u16": (0, 65535),
              "u32": (0, 2**32 - 1), "u64": (0, 2**64 - 1), "i8": (-128, 127),
              "i16": (-2**15, 2**15 - 1), "i32": (-2**31, 2**31 - 1), "i64": (-2**63, 2**63 - 1)}


def forms_for(x) -> list:
    """every encoding that holds x exactly (the wider ones are non-minimal)"""
    out = []
    if isinstance(x, int):
        out += [f for f in INT_FORMS if _INT_RANGE[f][0] <= x <= _INT_RANGE[f][1]]
        if float(x) == x:        # an exact double
            out.append("f64")
            if abs(x) < 2**128 and struct.unpack(">f", struct.pack(">f", float(x)))[0] == x:
                out.append("f32")
        return out
    out.append("f64")
    if x != x or math.isinf(x):
        out.append("f32")
    else:
        try:
            if struct.unpack(">f", struct.pack(">f", x))[0] == x:
                out.append("f32")
        except OverflowError:
            pass
    return out


def spair(k: bytes, v: bytes, af="fix", kf="auto", vf="auto") -> bytes:
    return enc_arr(2, af) + enc_raw(k, kf) + enc_raw(v, vf)


def npair(k: bytes, x, nf="f64", af="fix", kf="auto") -> bytes:
    return enc_arr(2, af) + enc_raw(k, kf) + enc_num(x, nf)


def datum(spairs=(), npairs=(), top=3, topf="fix", svf="auto", nvf="auto", third=b"\x90") -> bytes:
    """[sv, nv] (top 2) or [sv, nv, third] from encoded pairs"""
    return (enc_arr(top, topf) + enc_arr(len(spairs), svf) + b"".join(spairs)
            + enc_arr(len(npairs), nvf) + b"".join(npairs) + (third if top >= 3 else b""))


def sample(label: bytes, dat: bytes, af="fix", lf="auto") -> bytes:
    return enc_arr(2, af) + enc_raw(label, lf) + dat


def body(samples, af="auto") -> bytes:
    return enc_arr(len(samples), af) + b"".join(samples)


# -------------------------------------------------------------------- oracle
@functools.lru_cache(maxsize=4096)
def oracle(b: bytes):
    """-> [(label bytes, datum offset, datum length, ns, nn, datum object)]
    of a train request; ValueError if it is not one"""
    u = msgpack.Unpacker(raw=True, strict_map_key=False, max_buffer_size=1 << 30)
    u.feed(b)
    out = []
    try:
        n = u.read_array_header()
        for _ in range(n):
            if u.read_array_header() != 2:
                raise ValueError("sample is not a pair")
            lab = u.unpack()
            if not isinstance(lab, bytes):
                raise ValueError("label is not a raw")
            off = u.tell()
            d = u.unpack()
            if not isinstance(d, list) or len(d) < 2:
                raise ValueError("datum is not an array of 2 or more")
            out.append((lab, off, u.tell() - off, len(d[0]), len(d[1]), d))
    except (msgpack.exceptions.OutOfData, msgpack.exceptions.UnpackException) as e:
        raise ValueError(str(e)) from e
    if u.tell() != len(b):
        raise ValueError("trailing bytes")
    return out


def oracle_rows(conv, b: bytes):
    """per sample (idx int32, val float64) of the Python converter: the
    matching (value, rule) slots in the order the native hashers emit them"""
    rows = []
    for _, _, _, _, _, d in oracle(b):
        i, v = conv.hashed(conv.convert(Datum.from_msgpack(d)))
        rows.append((np.asarray(i, np.int32), np.asarray(v, np.float64)))
    return rows


_hashers = {}


def _hasher(conv):
    """the HostFvHasher of a converter, built once (the entry keeps conv alive)"""
    from jubatus_amd._native import native
    from jubatus_amd.fv_converter.gpu_path import GpuRuleTable
    if id(conv) not in _hashers:
        rt = GpuRuleTable(conv)
        h = native().HostFvHasher(rt.srules, rt.n_srules, rt.nrules, rt.n_nrules, rt.blob, rt.H)
        _hashers[id(conv)] = (conv, h, max(rt.n_srules, rt.n_nrules, 1))
    return _hashers[id(conv)][1:]


def native_rows(conv, datums: list):
    """HostFvHasher on a list of encoded datums -> per datum (idx, val) slots"""
    h, per = _hasher(conv)
    cap = sum(len(d) for d in datums) * per + 16
    idx = np.empty(cap, np.int32)
    val = np.empty(cap, np.float32)
    rp = np.zeros(len(datums) + 2, np.int64)
    n, slots, err = h.hash([body(datums)], idx.ctypes.data, val.ctypes.data, rp.ctypes.data,
                           len(datums) + 1, cap, False)
    assert err == 0 and n == len(datums)
    return [(idx[rp[i]:rp[i + 1]], val[rp[i]:rp[i + 1]]) for i in range(n)]


def native_csr(conv, bodies):
    """(row_ptr, idx, val) of HostFvHasher over the samples of bodies, in order"""
    rp, fi, fv = [0], [np.zeros(0, np.int32)], [np.zeros(0, np.float32)]
    for b in bodies:
        want = oracle(b)
        if want:
            for i, v in native_rows(conv, [b[o:o + n] for _, o, n, _, _, _ in want]):
                fi.append(i)
                fv.append(v)
                rp.append(rp[-1] + i.size)
    return np.asarray(rp, np.int64), np.concatenate(fi), np.concatenate(fv)


# ----------------------------------------- scan.hip steps 1-3, in plain Python
_FIXED = {0xCA: 5, 0xCE: 5, 0xD2: 5, 0xDD: 5, 0xDF: 5, 0xCB: 9, 0xCF: 9, 0xD3: 9,
          0xCC: 2, 0xD0: 2, 0xD4: 3, 0xCD: 3, 0xD1: 3, 0xDC: 3, 0xDE: 3,
          0xD5: 4, 0xD6: 6, 0xD7: 10, 0xD8: 18}


def token_size(b: bytes, p: int) -> int:
    """size of the token at p, containers header only (MessagePack spec;
    b is padded so that a header may be read past the body)"""
    t = b[p]
    if t <= 0x9F or t >= 0xE0:
        return 1
    if t <= 0xBF:
        return 1 + (t & 0x1F)
    if t in (0xC4, 0xD9):
        return 2 + b[p + 1]
    if t == 0xC7:
        return 3 + b[p + 1]
    if t in (0xC5, 0xDA):
        return 3 + ((b[p + 1] << 8) | b[p + 2])
    if t == 0xC8:
        return 4 + ((b[p + 1] << 8) | b[p + 2])
    if t in (0xC6, 0xDB, 0xC9):
        return (6 if t == 0xC9 else 5) + min(int.from_bytes(b[p + 1:p + 5], "big"), 0x3FFFFFFF)
    return _FIXED.get(t, 1)


def chain_walk(b: bytes):
    """Steps 1-3 of scan_train_kernel: every chunk walks from its first byte
    and marks what it visits, then goes on past its end until it meets a
    mark of a later chunk; the true walk is the chain of chunk 0.
    -> (the longest extension on that chain in tokens, the token starts the
    kernel keeps: each chain chunk's marks from its entry point on, and the
    chain's extensions). The kernel gives up (malformed) above kExtMax."""
    n = len(b)
    if n == 0:
        return 0, []
    pad = b + bytes(8)
    C = (n + K_THREADS - 1) // K_THREADS
    marked = bytearray(n)
    exits = []
    for t in range(K_THREADS):
        p = min(t * C, n)
        ce = min(p + C, n)
        while p < ce:
            marked[p] = 1
            p += token_size(pad, p)
        exits.append(min(p, n))
    t, entry, longest, starts = 0, 0, 0, []
    while t < K_THREADS:
        starts += [p for p in range(entry, min(min(t * C, n) + C, n)) if marked[p]]
        p, steps, nxt = exits[t], 0, K_THREADS
        while p < n:
            if marked[p]:
                nxt = p // C
                break
            starts.append(p)
            p += token_size(pad, p)
            steps += 1
        longest = max(longest, steps)
        t, entry = nxt, min(p, n)
    return longest, starts


def chain_max_ext(b: bytes) -> int:
    return chain_walk(b)[0]


def token_starts(b: bytes) -> list:
    """one walk from byte 0 with the model's own token_size table (a check
    of the chain logic, not of the table: see msgpack_token_starts)"""
    pad, p, out = b + bytes(8), 0, []
    while p < len(b):
        out.append(p)
        p += token_size(pad, p)
    return out


def msgpack_token_starts(b: bytes) -> list:
    """the token starts of one msgpack object as the msgpack library sees
    them: only the container type is read off the first byte, every size
    comes from Unpacker.tell() - independent of token_size"""
    u = msgpack.Unpacker(raw=True, strict_map_key=False, max_buffer_size=1 << 30)
    u.feed(b)
    out = []

    def walk():
        p = u.tell()
        out.append(p)
        t = b[p]
        if 0x90 <= t <= 0x9F or t in (0xDC, 0xDD):
            for _ in range(u.read_array_header()):
                walk()
        elif 0x80 <= t <= 0x8F or t in (0xDE, 0xDF):
            for _ in range(2 * u.read_map_header()):
                walk()
        else:
            u.skip()
    walk()
    assert u.tell() == len(b)
    return out


def device_takes(b: bytes) -> bool:
    return chain_max_ext(b) <= K_EXT_MAX


# --------------------------------------------------------------------- arena
def build_arena(bodies, rels=None, gap=0):
    """RequestArena.over a buffer with body k at an offset with
    (offset & 15) == rels[k] (default: packed back to back, any alignment),
    at least `gap` bytes apart. Gaps, the head and the tail (64 bytes) read
    0xdb 0xff 0xff ...: a raw32 header of 4 GB, not zeros.
    -> (arena, offs, lens)"""
    import torch
    from jubatus_amd.ops.feature_pipeline import RequestArena

    offs, cur = [], 0
    for k, b in enumerate(bodies):
        o = cur + gap if k else cur
        if rels is not None:
            o += (rels[k] - o) & 15
        offs.append(o)
        cur = o + len(b)
    buf = torch.empty(cur + 64, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    a = buf.numpy()
    a[:] = 0xFF
    a[0] = 0xDB
    for o, b in zip(offs, bodies):
        a[o:o + len(b)] = np.frombuffer(b, np.uint8)
        a[o + len(b)] = 0xDB
    lens = [len(b) for b in bodies]
    arena = RequestArena.over(buf, offs, lens)
    return arena, np.asarray(offs, np.int64), np.asarray(lens, np.int64)


# --------------------------------------------------------------- case groups
LABELS = ["", "L0", "L1", "L10", "L2", "ラベル", "L3"]        # the default table, in id order


def _ascii(rng, n):
    return bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789 _-") for _ in range(n))


def plain_sample(rng, label=None, ns=None, nn=None):
    ns = rng.randrange(0, 5) if ns is None else ns
    nn = rng.randrange(0, 4) if nn is None else nn
    label = rng.choice(LABELS).encode() if label is None else label
    sp = [spair(b"s%d" % rng.randrange(3), _ascii(rng, rng.randrange(0, 40))) for _ in range(ns)]
    nps = [npair(b"n%d" % rng.randrange(3), rng.gauss(0, 3)) for _ in range(nn)]
    return sample(label, datum(sp, nps, top=rng.choice((2, 3))))


def encoding_cases():
    """one request per (position, form): the three copies of the encoding
    table in scan.hip (token_size, token, token_d) and Reader"""
    rng = random.Random(11)

    def req(root="fix", pair="fix", lab="fix", top=3, topf="fix", third="fix", svf="fix",
            nvf="fix", spf="fix", npf="fix", skf="fix", nkf="fix", vf="fix", num=("f64", 1.5)):
        ss = []
        for m in range(3):
            sp = [spair(b"s1k", b"val%d" % m, spf, skf, vf), spair(b"k", b"", spf, skf, vf)]
            nps = [npair(b"n1", num[1], num[0], npf, nkf), npair(b"x", 2.0 + m, "f64", npf, nkf)]
            ss.append(sample(b"L1", datum(sp, nps, top, topf, svf, nvf, enc_arr(0, third)), pair, lab))
        return body(ss, root)

    out = [("plain", req())]
    for f in ARR_FORMS:
        out += [(f"root/{f}", req(root=f)), (f"sample/{f}", req(pair=f)),
                (f"top2/{f}", req(top=2, topf=f)), (f"top3/{f}", req(top=3, topf=f)),
                (f"third/{f}", req(third=f)), (f"sv/{f}", req(svf=f)), (f"nv/{f}", req(nvf=f)),
                (f"spair/{f}", req(spf=f)), (f"npair/{f}", req(npf=f))]
    for f in RAW_FORMS:
        out += [(f"label/{f}", req(lab=f)), (f"skey/{f}", req(skf=f)), (f"nkey/{f}", req(nkf=f)),
                (f"sval/{f}", req(vf=f))]
    for f, x in (("posfix", 100), ("negfix", -7), ("u8", 200), ("u16", 40000), ("u32", 3000000000),
                 ("u64", 2**63 + 2**40), ("i8", -100), ("i16", -30000), ("i32", -2000000000),
                 ("i64", -2**62), ("f32", 0.375), ("f64", 1e-3)):
        out.append((f"num/{f}", req(num=(f, x))))
    for m in range(6):           # every form at once
        c = rng.choice
        out.append((f"mix{m}", req(c(ARR_FORMS), c(ARR_FORMS), c(RAW_FORMS), c((2, 3)), c(ARR_FORMS),
                                   c(ARR_FORMS), c(ARR_FORMS), c(ARR_FORMS), c(ARR_FORMS),
                                   c(ARR_FORMS), c(RAW_FORMS), c(RAW_FORMS), c(RAW_FORMS),
                                   c((("u16", 513), ("i64", -5), ("f32", 2.5), ("u64", 7))))))
    return out


def body_of_len(L: int, rng) -> bytes:
    """a valid request of exactly L bytes (L = 1, 3, 5 or >= 6; no valid
    request has 2 or 4 bytes: an empty list takes 1, 3 or 5, a sample 5)"""
    if L in (1, 3, 5):
        return enc_arr(0, {1: "fix", 3: "a16", 5: "a32"}[L])
    small = {6: body([b"\x92\xa0\x92\x90\x90"]), 7: body([b"\x92\xa0\x93\x90\x90\x90"]),
             8: body([b"\x92\xa0\x92\x90\x90"], "a16"), 9: body([b"\x92\xa0\x93\x90\x90\x90"], "a16"),
             10: body([b"\x92\xa0\x92\x90\x90"], "a32"), 11: body([b"\x92\xa0\x92\x90\x90"] * 2)}
    if L in small:
        return small[L]
    ss, size = [], 3
    while len(ss) < K_MAX_SAMPLES - 1 and size + 200 < L:
        ss.append(plain_sample(rng))
        size += len(ss[-1])

    def make(padlen, vf):
        v = bytes(rng.choice(b"xyz01") for _ in range(padlen))
        return body(ss + [sample(b"L2", datum([spair(b"p", v, vf=vf)], [], top=2))])

    r = L - len(make(0, "fix"))
    assert r >= 0, L
    b = make(r, "fix") if r < 32 else make(r - 2, "raw16")   # a raw16 header: 2 bytes more
    assert len(b) == L, (L, len(b))
    return b


SMALL_LENS = [1, 3] + list(range(5, 18))
LARGE_LENS = [255, 256, 257, 511, 512, 513, 4 * 256 - 1, 4 * 256 + 1, 13 * 256 - 1, 13 * 256 + 1,
              40 * 256 - 1, 40 * 256 + 1, 107 * 256 - 1, 107 * 256 + 1]


def length_cases(which: str):
    """-> (bodies, rels): every length class at every rel = offset & 15;
    'large' ends with the bodies whose len + rel is 27 KB exactly"""
    rng = random.Random(5)
    bodies, rels = [], []
    for L in (SMALL_LENS if which == "small" else LARGE_LENS):
        for rel in range(16):
            bodies.append(body_of_len(L, rng))
            rels.append(rel)
    if which == "large":
        for rel in range(16):
            bodies.append(body_of_len(K_SCAN_BYTES - rel, rng))
            rels.append(rel)
    return bodies, rels


SAMPLE_COUNTS = [0, 1, 15, 16, 255, 256, 257, 767, 768]


def count_body(n: int, varied: bool) -> bytes:
    """n samples: minimal 6-byte ones, or pair counts that change from
    sample to sample (the in-request slot scan takes 3 samples per thread)"""
    if not varied:
        return body([b"\x92\xa0\x93\x90\x90\x90"] * n)
    ss = []
    for m in range(n):
        sp = [spair(b"s%d" % (j % 3), b"v%d" % (m % 7)) for j in range(m % 4)]
        nps = [npair(b"n%d" % j, m + j, "u16") for j in range((m * 5 + 1) % 3)]
        ss.append(sample(LABELS[m % len(LABELS)].encode(), datum(sp, nps, top=2 + m % 2)))
    return body(ss)


def straddle_cases():
    """whole chunks inside one raw16, and token headers on both sides of a
    chunk boundary (the chunk size C = ceil(len / 256))"""
    rng = random.Random(7)
    out = []
    for n in (300, 1000, 5000):
        for fill in (b"x", b"7", b"\xe3\x81\x82"):
            big = (fill * n)[:n]
            ss = [plain_sample(rng) for _ in range(4)]
            ss.insert(2, sample(b"L1", datum([spair(b"s1", big, vf="raw16"), spair(b"k", b"v")],
                                             [npair(b"n1", 4.0)])))
            out.append((f"inside/{n}/{fill[:1].hex()}", body(ss)))
    for total in (1500, 6000):
        C = (total + K_THREADS - 1) // K_THREADS
        head = [plain_sample(rng) for _ in range(3)]
        for j in range(C + 1):
            # pad key of j bytes, then a raw16 header, float64s and array16
            # headers: j moves all of them across the chunk boundaries
            mid = sample(b"L0", datum([spair(b"p" * j, b"v"),
                                       spair(b"s1", b"w" * 40, vf="raw16", kf="raw16")],
                                      [npair(b"n1", 1234.5678, "f64"), npair(b"n", 3.0, "f64")],
                                      top=3, svf="a16", nvf="a16", third=enc_arr(0, "a16")))

            def tail(padlen):
                return sample(b"L2", datum([spair(b"t", b"z" * padlen, vf="raw16")], [], top=2))
            b = body(head + [mid, tail(total - len(body(head + [mid, tail(0)])))])
            assert len(b) == total
            out.append((f"boundary/{total}/{j}", b))
    return out


_CJK = "機械学習の特徴量変換を試験する東京都渋谷区".encode()
_ARCYR = "مرحبا بالعالم Привет мир данные".encode()


def _hostile(rng, kind: str, n: int) -> bytes:
    if kind == "cjk":
        s = _CJK
    elif kind == "arcyr":
        s = _ARCYR
    elif kind == "containers":      # fixmap / fixarray and array16..map32 header bytes
        return bytes(rng.choice((rng.randrange(0x80, 0xA0), rng.randrange(0xDC, 0xE0)))
                     for _ in range(n))
    elif kind == "longraw":         # bin32 / raw32 headers of 4 GB
        return (bytes([rng.choice((0xC6, 0xDB))]) + b"\xff" * rng.randrange(4, 12)) * (n // 5 + 1)
    else:
        return bytes(rng.getrandbits(8) for _ in range(n))
    o = rng.randrange(len(s))
    return (s[o:] + s * (n // len(s) + 1))


PAYLOAD_KINDS = ("cjk", "arcyr", "containers", "longraw", "random")


def payload_cases(per_kind: int = 24):
    """keys and values whose bytes read as multi-byte tokens, containers or
    long raws when a chunk walk starts inside them -> [(name, body)]"""
    rng = random.Random(13)
    out = []
    for kind in PAYLOAD_KINDS:
        for r in range(per_kind):
            ss = []
            for _ in range(rng.randrange(1, 60 if r % 3 else 12)):
                sp = [spair(_hostile(rng, kind, 64)[:rng.randrange(0, 40)],
                            _hostile(rng, kind, 600)[:rng.choice((0, 3, 17, 31, 32, 90, 255, 256, 520))])
                      for _ in range(rng.randrange(0, 5))]
                nps = [npair(_hostile(rng, kind, 64)[:rng.randrange(0, 31)], rng.gauss(0, 100))
                       for _ in range(rng.randrange(0, 4))]
                ss.append(sample(rng.choice(LABELS).encode(), datum(sp, nps, top=rng.choice((2, 3)))))
                if sum(map(len, ss)) > 22000:
                    break
            b = body(ss)
            if len(b) <= K_SCAN_BYTES - 16:
                out.append((f"{kind}/{r}", b))
    return out


def fast_slack_cases():
    """the last string pair / num pair of a datum starting 79, 80 and 81
    bytes before the end of the body (jb_pack.hpp kFastSlack = 80: where the
    unchecked fast paths switch off)"""
    out = []
    for slack in (79, 80, 81):
        for kind in ("str", "num"):
            if kind == "str":
                last = spair(b"s1", b"last")
                d = enc_arr(3) + enc_arr(2) + spair(b"s0", b"first") + last + enc_arr(0) + b"\x90"
            else:
                last = npair(b"n1", 7, "posfix")
                d = (enc_arr(3) + enc_arr(1) + spair(b"s0", b"first") + enc_arr(2)
                     + npair(b"n0", 1.0) + last + b"\x90")

            def make(padlen):
                tail = sample(b"L2", datum([spair(b"t", b"z" * padlen, vf="str8")], [], top=2))
                return body([sample(b"L1", d), tail])
            b0 = make(0)
            b = make(slack - (len(b0) - b0.index(last)))
            assert len(b) - b.index(last) == slack
            out.append((f"slack{slack}/{kind}", b))
    return out


# ---- fv_hash
FV_KEYS = [b"", b"a", b"ab", b"abab", b"xab", b"abx", "日本ab".encode(), "abキー".encode(),
           "キ".encode()]
_F32_SUB = struct.unpack(">f", bytes.fromhex("00000001"))[0]
_F32_MAX = struct.unpack(">f", bytes.fromhex("7f7fffff"))[0]
FV_NUMBERS = [0, -0.0, 127, 128, -32, -33, 255, 256, 65535, 65536, 2**32 - 1, 2**32, 2**53 + 1,
              2**64 - 1, -2**63, _F32_SUB, _F32_MAX, 1e300, math.inf, -math.inf,
              1.0, 2.718281828459045, 3, 10.5, 1e-3, 12345.678, 1e10, 3.0000001]


def fv_samples():
    """-> encoded samples (label ''), every key under every rule, every
    number in every encoding that holds it"""
    out = []
    for i, k in enumerate(FV_KEYS):
        sp = [spair(k, b"v%d" % i), spair(k, "値".encode())]
        out.append(sample(b"", datum(sp, [npair(k, 1.5 + i)])))
    keys = [b"ab", b"x", b"abab"]
    n = 0
    for x in FV_NUMBERS:
        for f in forms_for(x):
            out.append(sample(b"", datum([], [npair(keys[n % 3], x, f)], top=2 + n % 2)))
            n += 1
    return out


def fv_nan_sample():
    nan32 = b"\xca\x7f\xc0\x00\x00"
    nan64 = b"\xcb\x7f\xf8\x00\x00\x00\x00\x00\x00"
    nps = [enc_arr(2) + enc_raw(b"ab") + nan32, enc_arr(2) + enc_raw(b"x") + nan64]
    return sample(b"", datum([], nps))


def fv_bodies(n: int):
    """n samples over requests of at most 50, cycling through fv_samples()"""
    ss = fv_samples()
    picked = [ss[i % len(ss)] for i in range(n)]
    return [body(picked[i:i + 50]) for i in range(0, n, 50)]


def window_body(span: int, lo_rel: int = 3):
    """one request of 64 samples whose datums, first byte to last, make the
    wave's 16-byte aligned window exactly `span` bytes when the first datum
    starts at an offset with (offset & 15) == lo_rel: the last datum ends 7
    bytes short of a 16-byte boundary -> (body, rel of the body)"""
    rng = random.Random(span)
    ss = [sample(b"", datum([spair(b"ab", _ascii(rng, 200), vf="raw16")], [npair(b"x", float(m))]))
          for m in range(63)]
    first = 3 + 1 + 1                     # a16 root header, the pair header, the label ''

    def make(padlen):
        last = sample(b"", datum([spair(b"abab", b"q" * padlen, vf="raw16")], [npair(b"ab", 2.0)]))
        return body(ss + [last], "a16")
    # datums span [lo_rel, hi) relative to a 16-byte boundary; hi = span - 7
    b = make(span - 7 - lo_rel + first - len(make(0)))
    hi = lo_rel + len(b) - first
    assert ((hi + 15) & ~15) == span and hi & 15 == 9
    return b, (lo_rel - first) & 15


def big_datum_body(nbytes: int = 20000) -> bytes:
    rng = random.Random(3)
    sp = [spair(b"ab%d" % j, _ascii(rng, 180), vf="raw16") for j in range(nbytes // 190)]
    return body([sample(b"", datum(sp, [npair(b"ab", 9.0)]))])


def slot_bound_body(npairs: int = 9000) -> bytes:
    """one datum of minimal 3-byte string pairs 92 a0 a0"""
    return body([sample(b"", datum([b"\x92\xa0\xa0"] * npairs, [], top=2))])


def log_reference(x64: np.ndarray) -> np.ndarray:
    """float32(log(max(1, float64(float32(x))))) in fp64"""
    with np.errstate(over="ignore", invalid="ignore"):
        x = x64.astype(np.float32).astype(np.float64)
        return np.log(np.where(x > 1.0, x, 1.0)).astype(np.float32)


def ulp_diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """distance in float32 ulps (same-sign finite values; equal infinities 0)"""
    ai = a.astype(np.float32).view(np.int32).astype(np.int64)
    bi = b.astype(np.float32).view(np.int32).astype(np.int64)
    return np.abs(ai - bi)


# ---- comparison of a CSR with the native hasher and the Python converter
def _same(a, b):
    if not np.array_equal(a, b):         # the full report only when they differ
        np.testing.assert_array_equal(a, b)


def check_fv(conv, cfg, bodies, row_ptr, fidx, fval) -> int:
    """rows [row_ptr, fidx, fval] of the samples of `bodies`, in order:
    every index equals the native hasher's (-1 slots included) and, where it
    matched, the Python converter's; `num` values are bit-equal to both
    (NaN: NaN in all three); `log` values are measured against
    float32(log(max(1, float64(float32(x))))) -> the largest distance in ulps"""
    sps, spn = len(cfg["string_rules"]), len(cfg["num_rules"])
    kinds = np.array([r["type"] == "log" for r in cfg["num_rules"]], bool)
    s, worst = 0, 0
    for b in bodies:
        want = oracle(b)
        if not want:
            continue
        nat = native_rows(conv, [b[o:o + n] for _, o, n, _, _, _ in want])
        for (nidx, nval), (pidx, pval), (_, _, _, ns, nn, d) in zip(nat, oracle_rows(conv, b), want):
            idx = fidx[row_ptr[s]:row_ptr[s + 1]]
            val = fval[row_ptr[s]:row_ptr[s + 1]]
            s += 1
            _same(idx, nidx)
            if idx.size == 0:
                assert pidx.size == 0
                continue
            m = idx >= 0
            _same(idx[m], pidx)
            is_log = np.zeros(idx.size, bool)
            is_log[ns * sps:] = np.tile(kinds, nn)
            with np.errstate(over="ignore"):
                p32 = pval.astype(np.float32)
            nan = np.isnan(nval)
            _same(np.isnan(val), nan)
            _same(np.isnan(p32), nan[m])
            bits, nbits = val.view(np.uint32), nval.view(np.uint32)
            exact = ~is_log & ~nan
            _same(bits[exact], nbits[exact])
            _same(bits[m][exact[m]], p32.view(np.uint32)[exact[m]])
            if nn:
                x = np.repeat(np.array([float(v) for _, v in d[1]], np.float64), spn)
                sel = is_log[ns * sps:] & m[ns * sps:]
                if sel.any():
                    ref = log_reference(x)[sel]
                    got = val[ns * sps:][sel]
                    _same(np.isinf(got), np.isinf(ref))
                    worst = max(worst, int(ulp_diff(got, ref).max()))
    assert s == len(row_ptr) - 1
    return worst


def log_sweep_body(count: int = 1024) -> bytes:
    """inputs of the `log` rules across the float32 range (and below 1),
    64 num pairs per sample under the key 'ab', which every rule matches"""
    rng = random.Random(17)
    xs = [1.0, 1.0000001, 1.5, 2.0, math.e, 10.0, 0.5, -3.0, 0.0, 3.4e38, 1e-40]
    while len(xs) < count:
        xs.append(math.exp(rng.uniform(0.0, 88.7)) if rng.random() < 0.8 else 1.0 + rng.random() * 1e-3)
    xs = [struct.unpack(">f", struct.pack(">f", min(x, _F32_MAX)))[0] for x in xs]   # float32 values
    ss = []
    for i in range(0, count, 64):
        nps = [npair(b"ab", x, "f64" if j % 2 else "f32") for j, x in enumerate(xs[i:i + 64])]
        ss.append(sample(b"", datum([], nps, svf="a16", nvf="a16")))
    return body(ss)


# ---- label tables
def colliding_labels(cap: int = 16):
    """two labels with the same home slot fnv1a64 & (cap - 1)"""
    from jubatus_amd.ops.feature_pipeline import fnv1a64
    seen = {}
    for i in range(1000):
        name = f"c{i}"
        slot = fnv1a64(name.encode()) & (cap - 1)
        if slot in seen:
            return seen[slot], name
        seen[slot] = name
    raise AssertionError


def label_cases():
    """name -> (labels of the table in id order, nhist)"""
    a, b = colliding_labels(16)
    return {
        "lds16": ([f"A{i}" for i in range(16)], 128),          # cap 32 = kLabCap: the LDS table
        "global17": ([f"A{i}" for i in range(17)], 128),       # cap 64: the global table
        "blob600": (["x" * 200, "y" * 200, "x" * 199 + "z"], 128),   # cap 16, blob > kLabBlob
        "ids70_nhist66": ([f"B{i}" for i in range(70)], 66),
        "ids70_nhist128": ([f"B{i}" for i in range(70)], 128),
        "ids70_nhist16": ([f"B{i}" for i in range(70)], 16),
        "special": (["", "ラベル", "L1", "L10", "L", "L100"], 128),
        "collide": ([a, b, "other"], 128),
    }


def label_bodies(labels):
    """every label of the table, several times, in a few requests"""
    rng = random.Random(len(labels))
    picks = [labels[i % len(labels)] for i in range(3 * len(labels))]
    rng.shuffle(picks)
    ss = [plain_sample(rng, lab.encode()) for lab in picks]
    return [body(ss[i:i + 23]) for i in range(0, len(ss), 23)]


def two_table_cases():
    """two tables with the same version (two additions each) and different
    labels -> [(labels, body)]"""
    rng = random.Random(1)
    return [(names, body([plain_sample(rng, n.encode()) for n in names]))
            for names in (["p", "q"], ["r", "s"])]


# ---- requests the device scan hands to the host
ERR_MALFORMED, ERR_LABEL = 1, 2           # csrc/hip/scan.hip kErrMalformed, kErrLabel


def good_request() -> bytes:
    rng = random.Random(2)
    return body([plain_sample(rng, lab, 2, 2) for lab in (b"L1", b"", b"L10")])


def rejection_cases():
    """-> [(name, body, error bits)]; labels come from LABELS, 'L3' has been
    deleted from the table"""
    big = b"v" * 40
    pieces = [("root", enc_arr(2))]
    for m in (0, 1):
        pieces += [(f"s{m}.pair", enc_arr(2)), (f"s{m}.label", enc_raw(b"L1")),
                   (f"s{m}.top", enc_arr(3)), (f"s{m}.sv", enc_arr(2)),
                   (f"s{m}.p1", enc_arr(2) + enc_raw(b"s1")), (f"s{m}.rawhdr", b"\xda\x00\x28"),
                   (f"s{m}.payload", big), (f"s{m}.p2", spair(b"k", b"v")), (f"s{m}.nv", enc_arr(1)),
                   (f"s{m}.np", enc_arr(2) + enc_raw(b"n1")), (f"s{m}.f64", enc_num(2.5, "f64")),
                   (f"s{m}.third", b"\x90")]
    full = b"".join(p for _, p in pieces)
    assert len(oracle(full)) == 2
    at = {}
    pos = 0
    for name, p in pieces:
        at[name] = pos
        pos += len(p)
    cuts = {"after_root": 1,
            "rawhdr+1": at["s1.rawhdr"] + 1, "rawhdr+2": at["s1.rawhdr"] + 2,
            "payload+1": at["s1.payload"] + 1, "payload-1": at["s1.payload"] + 39,
            "f64+1": at["s1.f64"] + 1, "f64+5": at["s1.f64"] + 5, "f64+8": at["s1.f64"] + 8,
            "between_pairs": at["s1.p2"], "before_nv": at["s1.nv"], "after_label": at["s1.top"],
            "before_last_sample": at["s1.pair"], "s0_rawhdr+1": at["s0.rawhdr"] + 1,
            "last_byte": len(full) - 1}
    out = [("trunc/" + k, full[:c], ERR_MALFORMED) for k, c in cuts.items()]
    one = sample(b"L1", datum([spair(b"s1", b"v")], [npair(b"n1", 1.0)]))
    out += [
        ("unknown_label", body([one, sample(b"new", datum())]), ERR_LABEL),
        ("deleted_label", body([one, sample(b"L3", datum())]), ERR_LABEL),
        ("binary_values", body([one, sample(b"L1", datum(third=enc_arr(1) + spair(b"b", b"\x00\x01", vf="bin8")))]),
         ERR_MALFORMED),
        ("datum_of_4", body([one, sample(b"L1", datum(top=4, third=b"\x90\x90"))]), ERR_MALFORMED),
        ("trailing_byte", full + b"\x00", ERR_MALFORMED),
        ("root_too_large", enc_arr(3) + full[1:], ERR_MALFORMED),
        ("root_too_small", enc_arr(1) + full[1:], ERR_MALFORMED),
        # one header claiming 2^30 elements (one only: the depth sum stays small)
        ("array32_2^30", body([one, sample(b"L1", enc_arr(3) + b"\xdd\x40\x00\x00\x00"
                                           + spair(b"k", b"v") + b"\x90\x90")]), ERR_MALFORMED),
        # no valid request has 2 or 4 bytes (see body_of_len)
        ("len2", b"\x91\x90", ERR_MALFORMED),
        ("len4", b"\x91\x92\xa0\x90", ERR_MALFORMED),
    ]
    return out


# ---- every body the GPU tests require the device to accept
def accepted_groups():
    """name -> (bodies, labels of the table in id order, labels deleted from
    it, converter config): what test_gpu_scan_edges.py scans with err == 0,
    group by group, for the host-side tests"""
    g = {
        "encodings": ([b for _, b in encoding_cases()], LABELS, [], CONV),
        "small": (length_cases("small")[0], LABELS, [], CONV),
        "large": (length_cases("large")[0], LABELS, [], CONV),
        "counts": ([count_body(n, v) for n in SAMPLE_COUNTS for v in (False, True)], LABELS, [], CONV),
        "straddles": ([b for _, b in straddle_cases()], LABELS, [], CONV),
        "payload": ([b for _, b in payload_cases()], LABELS, [], CONV),
        "fast_slack": ([b for _, b in fast_slack_cases()], LABELS, [], CONV),
        "good_request": ([good_request()], LABELS, ["L3"], CONV),
        "two_tables_0": ([two_table_cases()[0][1]], two_table_cases()[0][0], [], CONV),
        "two_tables_1": ([two_table_cases()[1][1]], two_table_cases()[1][0], [], CONV),
        "fv_log_sweep": ([log_sweep_body()], [""], [], CONV_FV),
        "fv_nan": ([body([fv_nan_sample(), fv_samples()[0]])], [""], [], CONV_FV),
        "fv_window": ([window_body(16384)[0], window_body(16400)[0]], [""], [], CONV_FV),
        "fv_large_datum": ([fv_bodies(5)[0], big_datum_body(), fv_bodies(3)[0]], [""], [], CONV_FV),
        "fv_slot_bound": ([slot_bound_body(9000)], [""], [], CONV_SLOT),
    }
    for n in (1, 63, 64, 65, 255, 256, 257):
        g[f"fv_n{n}"] = (fv_bodies(n), [""], [], CONV_FV)
    for name, (labels, _) in label_cases().items():
        g["labels_" + name] = (label_bodies(labels), labels, [], CONV)
    return g
