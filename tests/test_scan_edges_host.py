"""The host scanner (csrc/native/jb_pack.{hpp,cpp}), the host hasher
(jb_hostfv.hpp) and the Python oracle of tests/scan_cases.py on every body
that tests/test_gpu_scan_edges.py requires the device to accept
(scan_cases.accepted_groups, each group with its own label table and
converter): the reference the device is compared with accepts each of them
and agrees with an independent decoder. CPU."""
import numpy as np
import pytest

import scan_cases as sc
from jubatus_amd.fv_converter.converter import DatumToFvConverter


def _table(labels=sc.LABELS):
    from jubatus_amd._native import native
    t = native().LabelTable()
    for name in labels:
        t.get_or_add(name)
    return t


def native_scan(bodies, offs, buf, table, sps, spn):
    """pack_spans on bodies laid out in buf at offs -> dict of arrays"""
    from jubatus_amd._native import native
    R = len(bodies)
    n_max = sum(len(sc.oracle(b)) for b in bodies) + 1
    offs = np.ascontiguousarray(offs, np.int64)
    lens = np.asarray([len(b) for b in bodies], np.int64)
    doff = np.zeros(n_max, np.int64)
    dlen = np.zeros(n_max, np.int32)
    lab = np.zeros(n_max, np.int32)
    rp = np.zeros(n_max + 1, np.int64)
    sp = np.zeros(R + 1, np.int64)
    n, nbytes, nslots, err, err_req = native().pack_spans(
        buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, R, True, sps, spn, table,
        doff.ctypes.data, dlen.ctypes.data, lab.ctypes.data, rp.ctypes.data, sp.ctypes.data, n_max, 2)
    assert err == 0, (err, err_req)
    out = {"n": n, "nslots": nslots, "datum_off": doff[:n].copy(), "datum_len": dlen[:n].copy(),
           "labels": lab[:n].copy(), "row_ptr": rp[:n + 1].copy(), "stream_ptr": sp.copy()}
    # pack_requests (the copying variant: bodies 16-byte aligned in its staging
    # buffer) gives the same descriptors
    staging = np.zeros(sum(len(b) + 16 for b in bodies) + 16, np.uint8)
    n2, nbytes2, nslots2, err2, _ = native().pack_requests(
        list(bodies), True, sps, spn, table, staging.ctypes.data, staging.size,
        doff.ctypes.data, dlen.ctypes.data, lab.ctypes.data, rp.ctypes.data, sp.ctypes.data, n_max, 2)
    assert (err2, n2, nslots2) == (0, n, nslots)
    base = np.cumsum([0] + [(len(b) + 15) & ~15 for b in bodies])[:R]
    per = np.diff(sp)
    np.testing.assert_array_equal(doff[:n] - np.repeat(base, per),
                                  out["datum_off"] - np.repeat(offs, per))
    for name, a in (("datum_len", dlen[:n]), ("labels", lab[:n]), ("row_ptr", rp[:n + 1]),
                    ("stream_ptr", sp)):
        np.testing.assert_array_equal(a, out[name], err_msg=name)
    for k, b in enumerate(bodies):
        assert bytes(staging[base[k]:base[k] + len(b)]) == b
    return out


GROUPS = sc.accepted_groups()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_host_scanner_and_hasher_equal_oracle(group):
    """pack_spans / pack_requests, HostFvHasher and the Python oracle on one
    group of the GPU file, with that group's label table and converter:
    sample count, labels, datum offsets / lengths, row_ptr and stream_ptr
    identical; feature indices identical, `num` values bit-equal, `log`
    values within 1 ulp (glibc logf) of the fp64 formula. Bodies sit at every
    rel = offset & 15 with non-zero gaps. `fast_slack` has the last pair 79,
    80 and 81 bytes before the end and `fv_slot_bound` 9000 fast-path pairs
    (kFastSlack)."""
    bodies, labels, deleted, cfg = GROUPS[group]
    conv = DatumToFvConverter(cfg)
    arena, offs, lens = sc.build_arena(bodies, [k % 16 for k in range(len(bodies))])
    table = _table(labels)
    for name in deleted:
        assert table.remove(name)
    sps, spn = len(cfg["string_rules"]), len(cfg["num_rules"])
    got = native_scan(bodies, offs, arena.np, table, sps, spn)
    assert table.alive() == [n not in deleted for n in labels]     # nothing was revived
    s = slot = 0
    for k, b in enumerate(bodies):
        assert got["stream_ptr"][k] == s
        for lab, doff, dlen, ns, nn, _ in sc.oracle(b):
            assert labels[got["labels"][s]].encode() == lab
            assert got["datum_off"][s] == offs[k] + doff and got["datum_len"][s] == dlen
            assert got["row_ptr"][s] == slot
            slot += ns * sps + nn * spn
            s += 1
    assert got["n"] == s and got["stream_ptr"][len(bodies)] == s
    assert got["row_ptr"][s] == slot == got["nslots"]
    rp, fidx, fval = sc.native_csr(conv, bodies)
    np.testing.assert_array_equal(rp, got["row_ptr"])
    assert sc.check_fv(conv, cfg, bodies, rp, fidx, fval) <= 1


def test_host_hasher_nan():
    """NaN as float32 and float64: NaN under num, 0 under log in the host
    hasher, as in the Python converter (checked by the fv_nan group)"""
    conv = DatumToFvConverter(sc.CONV_FV)
    b = sc.body([sc.fv_nan_sample()])
    (idx, val), = sc.native_rows(conv, [b[sc.oracle(b)[0][1]:]])
    np.testing.assert_array_equal(np.isnan(val), [True, False, False, True, False,
                                                  True, False, False, False, False])
    assert (val[[1, 2, 4, 6]] == 0).all()


def test_model_accepts_the_generated_bodies():
    """the Python model of scan.hip steps 1-3 on every body of every group
    of the GPU file: the chain of chunk walks and extensions keeps exactly
    the token starts that the msgpack library finds (its sizes, not the
    model's token_size table), and the longest extension on it stays within
    kExtMax = 512 - the device must take every body, the GPU tests drop
    none. (No generated body exceeds kExtMax; the longest extension is
    asserted to be a real one, not 0.)"""
    worst = 0
    for bodies, _, _, _ in GROUPS.values():
        for b in bodies:
            longest, starts = sc.chain_walk(b)
            assert starts == sc.msgpack_token_starts(b)
            worst = max(worst, longest)
    assert 16 < worst <= sc.K_EXT_MAX


def test_model_token_sizes_equal_msgpack():
    """token_size of the model on every msgpack type (nil, bool, every int
    and float form, str / bin / ext of every width, maps): the same token
    starts as the msgpack library's"""
    import msgpack
    obj = [None, True, False, 0, 127, -1, -32, 200, 40000, 3000000000, 2**63, -100, -30000,
           -2000000000, -2**62, 1.5, "s", "x" * 40, "y" * 300, "z" * 70000, b"b", b"c" * 300,
           b"d" * 70000, {"k": [1, {"m": None}]}, {i: i for i in range(20)}, list(range(20)),
           [msgpack.ExtType(5, b"e" * n) for n in (1, 2, 4, 8, 16, 3, 300, 70000)]]
    for kw in ({"use_bin_type": True}, {"use_bin_type": False}):
        b = msgpack.packb(obj, **kw) + b""
        assert sc.token_starts(b) == sc.msgpack_token_starts(b)
    b = b"\x93" + sc.enc_num(1.5, "f32") + sc.enc_arr(1, "a32") + b"\xdf\x00\x00\x00\x01\x01\x02" \
        + sc.enc_arr(0, "a16")
    assert sc.token_starts(b) == sc.msgpack_token_starts(b)
    b = b"\x91\xde\x00\x01\xa1k" + sc.enc_raw(b"v", "str8")
    assert sc.token_starts(b) == sc.msgpack_token_starts(b)


def test_oracle_rejects_what_is_not_a_request():
    """the oracle is strict where the device scan is: the whole body, no more"""
    import random
    good = sc.body([sc.plain_sample(random.Random(1), b"L1", 2, 2)])
    assert len(sc.oracle(good)) == 1
    # truncated, a trailing byte, a root count one too small / too large
    for bad in (good[:-1], good + b"\x00", b"\x90" + good[1:], b"\x92" + good[1:]):
        with pytest.raises(ValueError):
            sc.oracle(bad)
