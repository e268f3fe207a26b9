"""GPU request scan (csrc/hip/scan.hip) and feature hashing (fv_hash.hip,
jb_fv.hpp, the Reader of jb_device.hpp) at their edges: bodies at every
offset & 15 with non-zero gaps, every msgpack encoding at every position,
the chunk-size, sample-count, label-table and window thresholds, payload
bytes that read as tokens, and the requests the device must hand back to the
host. The device result is compared with the host scanner on the same arena
(tests/test_scan_edges_host.py checks that one against a Python oracle on
the same cases); feature rows also with the host hasher and the Python
converter. Cases: tests/scan_cases.py."""
import numpy as np
import pytest

import scan_cases as sc
from jubatus_amd.fv_converter.converter import DatumToFvConverter

pytestmark = pytest.mark.gpu

FIELDS = ("row_ptr", "labels", "stream_ptr", "fidx", "fval")

# The `log` rule: the device's logf against float32(log(max(1, float64(float32(x)))))
# over every input of this file (test_fv_log_ulp: 1024 values across the
# float32 range, and each test that calls check_fv). ROCm ships no document
# with an error bound for the device logf, so the limit is the measured
# maximum plus 1 ulp for the final rounding. Measured on an MI355X: 2 ulp
# (test_fv_log_ulp and test_fv_window; 0 or 1 in the other tests).
LOG_ULP_MEASURED = 2
LOG_ULP_LIMIT = LOG_ULP_MEASURED + 1


def _pipe(cfg):
    import torch
    from jubatus_amd.ops.feature_pipeline import FeaturePipeline
    return FeaturePipeline(DatumToFvConverter(cfg), torch.device("cuda", 0))


@pytest.fixture(scope="module")
def pipe():
    return _pipe(sc.CONV)


@pytest.fixture(scope="module")
def pipe_fv():
    return _pipe(sc.CONV_FV)


_checks = {}


def _check(nhist):
    from jubatus_amd.ops.feature_pipeline import ScanCheck
    if nhist not in _checks:
        _checks[nhist] = ScanCheck(nhist)
    return _checks[nhist]


def _table(labels=sc.LABELS):
    from jubatus_amd._native import native
    t = native().LabelTable()
    for name in labels:
        t.get_or_add(name)
    return t


def _arrays(b):
    n = b.n
    rp = b.row_ptr[:n + 1].cpu().numpy()
    return (n, rp, b.labels[:n].cpu().numpy(), b.stream_ptr[:b.nstreams + 1].cpu().numpy(),
            b.fidx[:rp[-1]].cpu().numpy(), b.fval[:rp[-1]].cpu().numpy())


def _gpu_scan(pipe, arena, offs, lens, table, nhist=128):
    """-> (batch arrays, error word, label counts, slot capacity)"""
    import torch
    chk = _check(nhist)
    b = pipe.from_arena_gpu(arena, offs, lens, table, chk)
    assert b is not None
    torch.cuda.synchronize()
    pipe.check_errors()
    return _arrays(b), int(chk.err[0]), chk.hist[:nhist].copy(), b.nnz


def scan_both(pipe, bodies, rels=None, table=None, nhist=128):
    """one arena, the host scanner and the device scanner on it: err == 0
    and n, row_ptr, labels, stream_ptr, fidx, fval (bit patterns) and the
    label counts identical -> the device arrays"""
    import torch
    table = table or _table()
    arena, offs, lens = sc.build_arena(bodies, rels)
    host = _arrays(pipe.from_arena(arena, offs, lens, True, table))
    torch.cuda.synchronize()
    pipe.check_errors()
    dev, err, hist, _ = _gpu_scan(pipe, arena, offs, lens, table, nhist)
    assert err == 0
    assert dev[0] == host[0]
    for h, d, name in zip(host[1:], dev[1:], FIELDS):
        if name == "fval":
            h, d = h.view(np.uint32), d.view(np.uint32)
        np.testing.assert_array_equal(h, d, err_msg=name)
    np.testing.assert_array_equal(hist, np.bincount(host[2], minlength=nhist)[:nhist])
    return dev


def check_rows(pipe, cfg, bodies, dev):
    """feature rows against the host hasher and the Python converter"""
    worst = sc.check_fv(pipe.conv, cfg, bodies, dev[1], dev[4], dev[5])
    print("largest log ulp error:", worst)
    assert worst <= LOG_ULP_LIMIT       # measured 2, limit 3: see LOG_ULP_LIMIT above


def test_encodings(pipe):
    """One request per (position, form): root, sample pair, label, datum of
    2 and of 3 with an empty third, sv / nv arrays, pairs, keys, string
    values (fix, str8, raw16, raw32, bin8/16/32), numbers (fixints, u8..u64,
    i8..i64, f32, f64), array16 / array32 where a fixarray would do, and
    mixes. Guards the four copies of the encoding table: token_size, token
    and token_d of scan.hip and Reader of jb_device.hpp; bodies sit at every
    `rel` = offset & 15."""
    cases = sc.encoding_cases()
    bodies = [b for _, b in cases]
    dev = scan_both(pipe, bodies, [k % 16 for k in range(len(bodies))])
    assert dev[0] == 3 * len(bodies)
    check_rows(pipe, sc.CONV, bodies, dev)


@pytest.mark.parametrize("which", ["small", "large"])
def test_offsets_and_lengths(pipe, which):
    """Every length class at every `rel` = offset & 15 (scan_train_kernel
    `rel`, the `lo16` slack of fv_hash_kernel), gaps filled with 0xdb 0xff
    so that a read past a body's end shows. small: 1 (0x90), 3, 5...17 bytes
    - the chunk size `C == 1` with empty trailing chunks (2 and 4 bytes hold
    no valid request: see test_rejected_batch len2 / len4). large: 255, 256,
    257 (C 1 -> 2), 511..513, k*256 +- 1 for k = 4, 13, 40, 107 (a body that
    is no multiple of the chunk count, and one byte more than one), and
    len + rel == kScanBytes = 27 KB exactly at every rel."""
    bodies, rels = sc.length_cases(which)
    dev = scan_both(pipe, bodies, rels)
    if which == "large":
        assert [len(b) + r for b, r in zip(bodies[-16:], rels[-16:])] == [sc.K_SCAN_BYTES] * 16
    else:
        check_rows(pipe, sc.CONV, bodies, dev)


def test_sample_counts(pipe):
    """0, 1, 15, 16, 255, 256, 257, 767 and 768 samples per request, as
    minimal 6-byte samples and with pair counts that change from sample to
    sample: the one-thread-per-sample loop over 256 threads, the in-request
    slot scan (3 samples per thread) and the slot overlay on the bitmap,
    full at `kMaxSamples` = 768. 769 samples: the host takes the batch
    before any launch."""
    bodies = [sc.count_body(n, v) for n in sc.SAMPLE_COUNTS for v in (False, True)]
    dev = scan_both(pipe, bodies, [(5 * k) % 16 for k in range(len(bodies))])
    assert dev[0] == 2 * sum(sc.SAMPLE_COUNTS)
    arena, offs, lens = sc.build_arena([sc.count_body(3, True), sc.count_body(769, False)])
    assert pipe.scan_batch_args(arena, offs, lens, _table(), _check(128)) is None


def test_straddles(pipe):
    """A raw16 of 300, 1000 and 5000 bytes (whole chunks inside one token:
    their walks are dropped, the chain jumps over them), and a pad key swept
    over 0..C so that every byte of a raw16 header, a float64 and an array16
    header falls on each side of a chunk boundary (C = ceil(len / 256) = 6
    and 24)."""
    bodies = [b for _, b in sc.straddle_cases()]
    dev = scan_both(pipe, bodies, [(3 * k) % 16 for k in range(len(bodies))])
    check_rows(pipe, sc.CONV, bodies, dev)


def test_payload_bytes(pipe):
    """Keys and values of CJK, Arabic and Cyrillic UTF-8, runs of 0x80-0x9f
    and 0xdc-0xdf (container headers), 0xc6 / 0xdb 0xff... (4 GB raws) and
    seeded random bytes: a chunk walk that starts inside them does not see
    1-byte fixints, the case the re-synchronisation argument of scan.hip
    leans on. Only bodies whose longest true-chain extension exceeds
    `kExtMax` = 512 in the CPU model may be left out, at most 10 %; as
    generated, none is (test_scan_edges_host.py asserts the model's
    figures), so no rejected-for-extension batch exists to test."""
    cases = sc.payload_cases()
    kept = [b for _, b in cases if sc.device_takes(b)]
    assert len(kept) >= 0.9 * len(cases)
    dev = scan_both(pipe, kept, [(7 * k) % 16 for k in range(len(kept))])
    check_rows(pipe, sc.CONV, kept, dev)


@pytest.mark.parametrize("case", sorted(sc.label_cases()))
def test_label_tables(pipe, case):
    """The label table of scan_train_kernel: 16 live labels (capacity 32 =
    `kLabCap`, staged in LDS) and 17 (capacity 64, read from global memory);
    3 labels of 200 bytes (capacity 16 but a blob over `kLabBlob` = 512:
    global); ids up to 69 with nhist 16, 66 and 128 (ids >= kHist = 64 are
    counted with global atomics, ids >= nhist not at all); the empty label,
    a UTF-8 label and labels that are prefixes of each other; two labels
    with the same home slot (linear probing)."""
    from jubatus_amd.ops.feature_pipeline import fnv1a64, label_table_arrays
    labels, nhist = sc.label_cases()[case]
    table = _table(labels)
    th, tm, blob = label_table_arrays(table.names(), table.alive())
    want_lds = {"lds16": True, "global17": False, "blob600": False}.get(case)
    if want_lds is not None:
        assert (th.size <= 32 and blob.size <= 512) == want_lds
        assert th.size == {"lds16": 32, "global17": 64, "blob600": 16}[case]
    if case == "collide":
        a, b = labels[:2]
        home = fnv1a64(b.encode()) & (th.size - 1)
        assert home == fnv1a64(a.encode()) & (th.size - 1) and tm[3 * home + 2] == 0
    bodies = sc.label_bodies(labels)
    dev = scan_both(pipe, bodies, [(11 * k + 1) % 16 for k in range(len(bodies))], table, nhist)
    assert sorted(set(dev[2].tolist())) == list(range(len(labels)))


def test_two_label_tables_one_pipeline(pipe):
    """FeaturePipeline.label_table caches the device table: two tables with
    the same version (number of changes) and different labels must not share
    the cached copy (found by test_label_tables: the second table's labels
    were reported unknown, error bit 2)"""
    for names, b in sc.two_table_cases():
        table = _table(names)
        assert table.version() == 2
        dev = scan_both(pipe, [b], None, table)
        assert dev[2].tolist() == [0, 1]


REJECTIONS = sc.rejection_cases()


@pytest.mark.parametrize("k", range(len(REJECTIONS)), ids=[r[0] for r in REJECTIONS])
def test_rejected_batch(pipe, k):
    """A good request and one the device scan does not take: an unknown and
    a deleted label set kErrLabel (2) only; non-empty binary values, a datum
    of 4, truncations (inside a raw header, its payload, a float64, between
    tokens, before the last sample), a trailing byte, a root count one too
    large / too small, an array32 header claiming 2^30 elements (clamped in
    token_d) and the 2- and 4-byte bodies set kErrMalformed (1) only. Every
    sample of the batch becomes a no-op, and the next batch on the same
    pipeline scans clean."""
    name, bad, bits = REJECTIONS[k]
    table = _table()
    assert table.remove("L3")
    good = sc.good_request()
    arena, offs, lens = sc.build_arena([good, bad], [9, 6])
    (n, rp, labels, sp, _, _), err, _, _ = _gpu_scan(pipe, arena, offs, lens, table)
    assert err == bits
    assert n >= 3 and (labels == -1).all() and (rp == 0).all()
    dev = scan_both(pipe, [good], [9], table)
    assert dev[0] == 3 and (dev[2] >= 0).all()


def _fv_scan(pipe_fv, bodies, rels=None):
    dev = scan_both(pipe_fv, bodies, rels, _table([""]))
    check_rows(pipe_fv, sc.CONV_FV, bodies, dev)
    return dev


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_fv_rules_numbers_batch_sizes(pipe_fv, n):
    """fv_hash_kernel with n datums (one lane each; the last wave and the
    last block partly idle): rules '*', 'ab*', '*ab' and 'ab' (`match_kind`
    0..3) on the keys '', a, ab, abab, xab, abx and UTF-8 keys - shorter
    than, equal to and longer than the matcher; 0, -0.0, the fixint / 8 / 16
    / 32 / 64-bit borders, 2^53 + 1, 2^64 - 1, -2^63, a float32 subnormal,
    float32 max, 1e300 and +-inf in every encoding that holds them. Indices
    and num values bit-equal to the host hasher and the Python converter."""
    dev = _fv_scan(pipe_fv, sc.fv_bodies(n), None)
    assert dev[0] == n


def test_fv_log_ulp(pipe_fv):
    """logf(fmaxf(1, x)) of emit_datum over 1024 float32 inputs from below 1
    to float32 max, as f32 and f64: the largest error against the fp64
    reference stays within LOG_ULP_LIMIT"""
    _fv_scan(pipe_fv, [sc.log_sweep_body()], [5])


def test_fv_nan(pipe_fv):
    """NaN as float32 and float64: NaN under `num`, 0 under `log`
    (fmaxf(1, NaN) = 1) on the device, in the host hasher and in the Python
    converter (max(1.0, nan) keeps 1.0)"""
    b = sc.body([sc.fv_nan_sample(), sc.fv_samples()[0]])
    dev = _fv_scan(pipe_fv, [b], [2])
    row = dev[5][dev[1][0]:dev[1][1]]
    # key 'ab' under all five num rules, then key 'x' under '*' num and '*' log
    np.testing.assert_array_equal(np.isnan(row), [True, False, False, True, False,
                                                  True, False, False, False, False])
    assert (row[[1, 2, 4, 6]] == 0).all()


@pytest.mark.parametrize("span", [16384, 16400])
def test_fv_window(pipe_fv, span):
    """One wave of 64 datums whose 16-byte aligned window is exactly `kWin`
    = 16384 bytes (first datum at offset & 15 == 3, last one ending 7 bytes
    short of a boundary: staged in LDS) and 16400 bytes (parsed from global
    memory)"""
    b, rel = sc.window_body(span)
    arena, offs, lens = sc.build_arena([b], [rel])
    want = sc.oracle(b)
    lo = int(offs[0]) + want[0][1]
    hi = int(offs[0]) + want[-1][1] + want[-1][2]
    assert len(want) == 64 and ((hi + 15) & ~15) - (lo & ~15) == span and lo & 15 == 3
    _fv_scan(pipe_fv, [b], [rel])


def test_fv_one_large_datum(pipe_fv):
    """a single datum of about 20 KB, more than `kWin`: the global path with
    one live lane, between two requests of small datums"""
    b = sc.big_datum_body()
    assert 16384 + 16 < len(b) < sc.K_SCAN_BYTES
    _fv_scan(pipe_fv, [sc.fv_bodies(5)[0], b, sc.fv_bodies(3)[0]], [1, 13, 4])


def test_fv_slot_bound():
    """One datum of 9000 minimal string pairs (92 a0 a0, 3 bytes each) under
    two rules that match: 18000 slots against
    slot_cap = (used // 3 + 1) * max(sps, spn) of scan_batch_args"""
    pipe = _pipe(sc.CONV_SLOT)
    b = sc.slot_bound_body(9000)
    assert len(b) <= sc.K_SCAN_BYTES - 16
    table = _table([""])
    arena, offs, lens = sc.build_arena([b], [7])
    (n, rp, labels, _, fidx, fval), err, _, slot_cap = _gpu_scan(pipe, arena, offs, lens, table)
    assert err == 0 and n == 1 and labels[0] == 0
    assert rp[-1] == 18000 <= slot_cap
    assert slot_cap == ((int(offs[0]) + len(b)) // 3 + 1) * 2
    sc.check_fv(pipe.conv, sc.CONV_SLOT, [b], rp, fidx, fval)
    scan_both(pipe, [b], [7], table)
