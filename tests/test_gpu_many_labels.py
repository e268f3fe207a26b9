"""Label capacities above 1024 on the GPU: the run-time-LC kernels of
csrc/hip/linear_chunked.hip against models/linear_oracle.py and, at LC = 1024,
against the LC-templated kernels of linear.hip; their dispatch from
jb_linear_train / jb_linear_classify; the Python GPU driver and the native
GPU server with more than 1024 labels.

Tolerance: the project's own for online updates (tests/test_gpu_linear.py):
rtol 2e-3, atol 2e-3 * max|oracle table| on W and on P, with equal update
counts. Tables have at most 1024 rows, so LC = 16384 is 64 MiB per table."""
import functools
import json
import os
import random
import socket
import subprocess
import time

import msgpack
import numpy as np
import pytest

from jubatus_amd.fv_converter.converter import DatumToFvConverter
from jubatus_amd.models import classifier as clf_mod
from jubatus_amd.models import linear_oracle as lo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "jubatus_amd", "native_bin", "jubaclassifier")
H = 512
METHODS = {"PA": lo.PA, "PA2": lo.PA2, "AROW": lo.AROW, "NHERD": lo.NHERD}
C = 0.7


def _device():
    import torch
    return torch.device("cuda", 0)


# ----------------------------------------------------------------- streams
def _pool(LC):
    """labels that get samples: chunk 0 (0, 1, 3, 200, 255: y and l* share a
    chunk), the chunks of other waves (256, 300, 700, ..), the last label"""
    return [0, 1, 3, 200, 255, 256, 300, 700, LC // 2 + 5, LC - 257, LC - 2, LC - 1]


def _active(LC):
    a = np.zeros(LC, np.int32)
    a[_pool(LC)] = 1
    a[np.arange(2, LC, 37)] = 1          # registered labels that never get a sample
    return a


@functools.lru_cache(maxsize=None)
def _edge_stream(LC, n=200, seed=0):
    """samples (y, idx, val): widths 1, 5, 64, 65, 70 and 300, a repeated
    index, idx = -1 slots, a sample without features, labels outside [0, LC)"""
    rng = np.random.default_rng(seed)
    pool = _pool(LC)
    vocab = rng.choice(H, 48, replace=False)
    widths = [1, 5, 64, 65, 70, 300, 8, 16, 3, 12]
    out = []
    for s in range(n):
        y = pool[int(rng.integers(len(pool)))]
        w = widths[s % len(widths)]
        if s == 0:
            y = 0                        # the first update of an all-zero model
        elif s == 1:
            y = LC - 1
        elif s == 20:
            w = 0
        elif s == 40:
            y = -1
        elif s == 41:
            y = LC
        idx = rng.choice(vocab if w <= 48 else H, w, replace=False).astype(np.int32)
        val = rng.normal(size=w).astype(np.float32)
        if s % 17 == 4 and w >= 2:
            idx[-1] = idx[0]             # a row twice in one sample
        if s % 13 == 6 and w >= 3:
            idx[w // 2] = -1
        out.append((y, idx, val))
    return tuple(out)


def _csr(samples, bounds=None):
    """device CSR of a stream; bounds: sample offsets of the update streams"""
    import torch
    dev = _device()
    rp = np.zeros(len(samples) + 1, np.int64)
    for i, (_, idx, _) in enumerate(samples):
        rp[i + 1] = rp[i] + len(idx)
    fi = np.concatenate([s[1] for s in samples] + [np.zeros(1, np.int32)]).astype(np.int32)
    fv = np.concatenate([s[2] for s in samples] + [np.zeros(1, np.float32)]).astype(np.float32)
    lab = np.asarray([s[0] for s in samples] + [0], np.int32)
    sp = np.asarray(bounds if bounds is not None else [0, len(samples)], np.int64)
    t = lambda a: torch.from_numpy(a).to(dev)
    return t(rp), t(fi), t(fv), t(lab), t(sp), len(sp) - 1


def _run_oracle(samples, LC, mid, active, W=None, P=None, rows=H):
    W = np.zeros((rows, LC), np.float32) if W is None else W.copy()
    P = np.ones((rows, LC), np.float32) if P is None else P.copy()
    upd = valid = 0
    for y, idx, val in samples:
        if not 0 <= y < LC:
            continue
        valid += 1
        upd += lo.train_one(W, P, idx.astype(np.int64), val, y, active, mid, C)
    return W, P, upd, valid


@functools.lru_cache(maxsize=None)
def _edge_oracle(LC, method):
    return _run_oracle(_edge_stream(LC), LC, METHODS[method], _active(LC))


def _tables(LC, mid, dtype=None, W0=None, P0=None, rows=H):
    import torch
    dev = _device()
    W = torch.zeros((rows, LC), dtype=dtype or torch.float32, device=dev) if W0 is None else \
        torch.from_numpy(W0).to(dev).to(dtype or torch.float32)
    P = None
    if mid in lo.USES_COVARIANCE:
        P = torch.ones((rows, LC), dtype=torch.float32, device=dev) if P0 is None else \
            torch.from_numpy(P0).to(dev)
    return W, P, torch.zeros(2, dtype=torch.int64, device=dev)


def _chunked(samples, LC, mid, active, waves, mode=None, bounds=None, dtype=None, W0=None, P0=None,
             rows=H):
    import torch
    from jubatus_amd.ops import hip
    rp, fi, fv, lab, sp, ns = _csr(samples, bounds)
    W, P, stats = _tables(LC, mid, dtype, W0, P0, rows)
    touched = torch.zeros(rows, dtype=torch.uint8, device=_device())
    hip.linear_train_chunked(rp, fi, fv, lab, sp, ns, W, P, torch.from_numpy(active).to(_device()),
                             mid, C, hip.UPDATE_EXACT if mode is None else mode, waves, stats,
                             touched)
    torch.cuda.synchronize()
    return (W.float().cpu().numpy(), P.cpu().numpy() if P is not None else None,
            stats.cpu().tolist(), touched.cpu().numpy())


def _close(W, P, oW, oP, mid):
    np.testing.assert_allclose(W, oW, rtol=2e-3, atol=2e-3 * (float(np.abs(oW).max()) or 1.0))
    if mid in lo.USES_COVARIANCE:
        np.testing.assert_allclose(P, oP, rtol=2e-3, atol=2e-3 * float(np.abs(oP).max()))


# ------------------------------------------------- kernel against the oracle
@pytest.mark.parametrize("waves", [1, 4, 16])
@pytest.mark.parametrize("method", ["PA", "PA2", "AROW", "NHERD"])
@pytest.mark.parametrize("LC", [2048, 16384])
def test_chunked_train_matches_oracle(LC, method, waves):
    mid = METHODS[method]
    samples = _edge_stream(LC)
    oW, oP, upd, valid = _edge_oracle(LC, method)
    assert valid == len(samples) - 2 and upd > valid // 2
    assert {s[0] for s in samples} >= {0, LC - 1, 256, -1, LC}
    W, P, stats, touched = _chunked(samples, LC, mid, _active(LC), waves)
    print(f"LC {LC} {method} waves {waves}: updates {stats} oracle {[upd, valid]}, "
          f"max|W - oracle| {np.abs(W - oW).max():.3e} of {np.abs(oW).max():.3e}")
    assert stats == [upd, valid]
    _close(W, P, oW, oP, mid)
    rows = np.flatnonzero(np.any(oW != 0, axis=1))
    assert set(rows) <= set(np.flatnonzero(touched))
    # the same launch again from the same start: bit-identical tables
    W2, P2, stats2, _ = _chunked(samples, LC, mid, _active(LC), waves)
    assert stats2 == stats
    assert np.array_equal(W, W2)
    if P is not None:
        assert np.array_equal(P, P2)


# ------------------------------------- samples wider than the kernel's stage
STAGE = 512            # csrc/hip/linear_chunked.hip kStage
WIDE_ROWS = 2048


@functools.lru_cache(maxsize=None)
def _wide_stream(LC, lo_row=0, seed=21, n=36):
    """samples at and past the stage of 512 slots: widths 512, 513, 700 and
    1200 between narrow ones, distinct rows drawn from WIDE_ROWS rows starting
    at lo_row, then: a staged row repeated past the stage (slot 3 again at slot
    512 or 600, slot 100 again at the last slot), a row repeated inside the
    stage with its second occurrence in the last staged slot (511), idx = -1
    on both sides of the boundary. No row repeats only among the slots past
    the stage (the kernel applies those in the order their atomics land)."""
    rng = np.random.default_rng(seed)
    pool = _pool(LC)
    widths = [512, 513, 1200, 16, 700, 5]
    out = []
    for s in range(n):
        w = widths[s % len(widths)]
        y = pool[int(rng.integers(len(pool)))]
        idx = (lo_row + rng.choice(WIDE_ROWS, w, replace=False)).astype(np.int32)
        val = rng.normal(size=w).astype(np.float32)
        if w >= STAGE:
            idx[STAGE - 1] = idx[0]
            if s % 12 >= 6:
                idx[7] = -1
        if w > STAGE:
            idx[STAGE if w < 600 else 600] = idx[3]
            if w > 600:
                idx[-1] = idx[100]
                idx[STAGE + 1] = -1
        out.append((y, idx, val))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _wide_oracle(LC, method):
    return _run_oracle(_wide_stream(LC), LC, METHODS[method], _active(LC), rows=WIDE_ROWS)


@pytest.mark.parametrize("waves", [1, 4, 16])
@pytest.mark.parametrize("method", ["PA", "AROW", "NHERD"])
def test_chunked_train_wide_samples_match_oracle(method, waves):
    """widths 512, 513, 700 and 1200 with rows repeated across the stage
    boundary: the slots past the stage are scored, weighed and applied from
    global memory, and a row that is also staged is applied against the state
    before the sample, as the oracle applies it"""
    LC, mid = 2048, METHODS[method]
    samples = _wide_stream(LC)
    assert {len(s[1]) for s in samples} == {512, 513, 1200, 16, 700, 5}
    oW, oP, upd, valid = _wide_oracle(LC, method)
    assert valid == len(samples) and upd > valid // 2
    W, P, stats, touched = _chunked(samples, LC, mid, _active(LC), waves, rows=WIDE_ROWS)
    print(f"wide {method} waves {waves}: updates {stats} oracle {[upd, valid]}, "
          f"max|W - oracle| {np.abs(W - oW).max():.3e} of {np.abs(oW).max():.3e}")
    assert stats == [upd, valid]
    _close(W, P, oW, oP, mid)
    assert set(np.flatnonzero(np.any(oW != 0, axis=1))) <= set(np.flatnonzero(touched))
    W2, P2, stats2, _ = _chunked(samples, LC, mid, _active(LC), waves, rows=WIDE_ROWS)
    assert stats2 == stats and np.array_equal(W, W2)
    if P is not None:
        assert np.array_equal(P, P2)


@pytest.mark.parametrize("waves", [1, 16])
def test_atomic_streams_with_wide_samples(waves):
    """two atomic streams on disjoint halves of the table, each with samples of
    512, 513, 700 and 1200 slots: the requests applied one after the other"""
    from jubatus_amd.ops import hip
    LC, mid = 2048, lo.AROW
    a = _wide_stream(LC, 0, 31, 12)
    b = _wide_stream(LC, WIDE_ROWS, 32, 12)
    samples = list(a) + list(b)
    act = _active(LC)
    oW, oP, upd, valid = _run_oracle(samples, LC, mid, act, rows=2 * WIDE_ROWS)
    W, P, stats, _ = _chunked(samples, LC, mid, act, waves, mode=hip.UPDATE_ATOMIC,
                              bounds=[0, len(a), len(samples)], rows=2 * WIDE_ROWS)
    assert stats == [upd, valid] and upd > valid // 2
    _close(W, P, oW, oP, mid)


def test_chunked_entry_points_refuse_other_capacities():
    import torch
    from jubatus_amd.ops import hip
    dev = _device()
    rp, fi, fv, lab, sp, ns = _csr([(0, np.asarray([1], np.int32), np.asarray([1.0], np.float32))])
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    for LC in (128, 384 + 64, 16384 + 256):
        W = torch.zeros((8, LC), device=dev)
        act = torch.ones(LC, dtype=torch.int32, device=dev)
        rc = hip._fn("jb_linear_train_chunked")(rp.data_ptr(), fi.data_ptr(), fv.data_ptr(),
                                                lab.data_ptr(), sp.data_ptr(), 1, W.data_ptr(), 0, None,
                                                act.data_ptr(), LC, lo.PA, 1.0, 0, 4, stats.data_ptr(),
                                                None, None)
        assert rc != 0
        out = torch.zeros(LC, device=dev)
        rc = hip._fn("jb_linear_classify_chunked")(rp.data_ptr(), fi.data_ptr(), fv.data_ptr(), 1,
                                                   W.data_ptr(), 0, LC, out.data_ptr(), None)
        assert rc != 0
        with pytest.raises(ValueError):
            hip.linear_train_chunked(rp, fi, fv, lab, sp, 1, W, None, act, lo.PA, 1.0, 0, 4)
    W = torch.zeros((8, 2048), device=dev)
    act = torch.ones(2048, dtype=torch.int32, device=dev)
    rc = hip._fn("jb_linear_train_chunked")(rp.data_ptr(), fi.data_ptr(), fv.data_ptr(),
                                            lab.data_ptr(), sp.data_ptr(), 1, W.data_ptr(), 0, None,
                                            act.data_ptr(), 2048, lo.PA, 1.0, 0, 8, stats.data_ptr(),
                                            None, None)
    assert rc != 0                                   # waves is 1, 4 or 16
    torch.cuda.synchronize()
    assert float(W.abs().max()) == 0.0 and stats.cpu().tolist() == [0, 0]


# --------------------------------------------------------------------- ties
def _changed_cols(W, W0=None):
    d = W if W0 is None else W - W0
    return set(np.flatnonzero(np.any(d != 0, axis=0)).tolist())


@pytest.mark.parametrize("waves", [1, 4, 16])
def test_ties_go_to_the_lowest_label(waves):
    LC = 2048
    one = [(0, np.asarray([3, 7], np.int32), np.asarray([1.0, -2.0], np.float32))]
    act = np.ones(LC, np.int32)
    W, _, stats, _ = _chunked(one, LC, lo.PA, act, waves)
    assert stats == [1, 1] and _changed_cols(W) == {0, 1}
    act[1] = act[2] = 0                      # the next active index is 3
    W, _, _, _ = _chunked(one, LC, lo.PA, act, waves)
    assert _changed_cols(W) == {0, 3}
    # y itself is the lowest index: l* of y = 5 on a zero model is label 0
    W, _, _, _ = _chunked([(5, one[0][1], one[0][2])], LC, lo.PA, np.ones(LC, np.int32), waves)
    assert _changed_cols(W) == {0, 5}
    # two wrong labels with exactly equal columns in chunks of different waves
    # (waves = 4: chunk 3 is wave 3's, chunk 4 wave 0's, which reports first)
    for a, b in ((256 * 3 + 5, 256 * 4 + 7), (256 + 9, 256 * 6 + 1), (70, 256 * 7 + 70)):
        W0 = np.zeros((H, LC), np.float32)
        W0[3, a] = W0[3, b] = 0.75
        W0[7, a] = W0[7, b] = -0.5
        W, _, stats, _ = _chunked(one, LC, lo.PA, np.ones(LC, np.int32), waves, W0=W0)
        assert stats == [1, 1] and _changed_cols(W, W0) == {0, a}, (a, b)


@pytest.mark.parametrize("waves", [1, 16])
def test_inactive_labels_are_never_chosen(waves):
    LC = 2048
    act = _active(LC)
    loud = [5, 1500]                         # inactive, with the largest scores by far
    assert not act[loud].any()
    W0 = np.zeros((H, LC), np.float32)
    W0[:, loud] = 50.0
    samples = [(y, idx, np.abs(val)) for y, idx, val in _edge_stream(LC, 40, 5) if len(idx) <= 70]
    oW, oP, upd, valid = _run_oracle(samples, LC, lo.AROW, act, W0)
    W, P, stats, _ = _chunked(samples, LC, lo.AROW, act, waves, W0=W0)
    assert stats == [upd, valid] and upd > 10
    assert np.array_equal(W[:, loud], W0[:, loud])
    assert np.array_equal(P[:, loud], np.ones((H, 2), np.float32))
    _close(W, P, oW, oP, lo.AROW)


# ------------------------------------------- the templated kernels at 1024
@pytest.mark.parametrize("waves", [1, 4, 16])
@pytest.mark.parametrize("wdt", ["fp32", "bf16"])
@pytest.mark.parametrize("method", ["PA", "AROW"])
def test_chunked_equals_template_kernels_at_1024(method, wdt, waves):
    import torch
    from jubatus_amd.ops import hip
    LC, mid = 1024, METHODS[method]
    dt = torch.bfloat16 if wdt == "bf16" else torch.float32
    samples = _edge_stream(LC)
    act = _active(LC)
    rp, fi, fv, lab, sp, ns = _csr(samples)
    W, P, stats = _tables(LC, mid, dt)
    hip.linear_train(rp, fi, fv, lab, sp, 1, W, P, torch.from_numpy(act).to(_device()), mid, C,
                     hip.UPDATE_EXACT, stats=stats)
    torch.cuda.synchronize()
    tW = W.float().cpu().numpy()
    tP = P.cpu().numpy() if P is not None else None
    cW, cP, cstats, _ = _chunked(samples, LC, mid, act, waves, dtype=dt)
    print(f"{method} {wdt} waves {waves}: updates {cstats} template {stats.cpu().tolist()}, "
          f"max|dW| {np.abs(cW - tW).max():.3e} of {np.abs(tW).max():.3e}")
    assert cstats == stats.cpu().tolist() and cstats[0] > 50
    _close(cW, cP, tW, tP, mid)
    # classify over the trained table: every column, both kernels
    out_t = torch.zeros((len(samples), LC), device=_device())
    out_c = torch.full((len(samples), LC), 7.0, device=_device())
    hip.linear_classify(rp, fi, fv, len(samples), W, out_t)
    hip.linear_classify_chunked(rp, fi, fv, len(samples), W, out_c)
    torch.cuda.synchronize()
    st = out_t.cpu().numpy()
    np.testing.assert_allclose(out_c.cpu().numpy(), st, rtol=2e-3, atol=2e-3 * float(np.abs(st).max()))


# -------------------------------------------------------------------- modes
def test_atomic_streams_on_disjoint_rows_equal_the_serial_order():
    from jubatus_amd.ops import hip
    LC, mid = 2048, lo.AROW
    rng = np.random.default_rng(11)
    pool = _pool(LC)
    samples, bounds = [], [0]
    for k in range(8):                       # stream k owns rows 64 k .. 64 k + 63
        for _ in range(20):
            w = int(rng.integers(1, 17))
            idx = (64 * k + rng.choice(64, w, replace=False)).astype(np.int32)
            samples.append((pool[int(rng.integers(len(pool)))], idx,
                            rng.normal(size=w).astype(np.float32)))
        bounds.append(len(samples))
    act = _active(LC)
    oW, oP, upd, valid = _run_oracle(samples, LC, mid, act)
    for waves in (1, 4, 16):
        W, P, stats, _ = _chunked(samples, LC, mid, act, waves, mode=hip.UPDATE_ATOMIC, bounds=bounds)
        assert stats == [upd, valid]
        _close(W, P, oW, oP, mid)


@pytest.mark.parametrize("wdt", ["fp32", "bf16"])
def test_serial_mode_through_jb_linear_train(wdt):
    """mode kSerial at LC = 2048: 5 streams that share rows give the requests
    applied one after the other (fp32: within the tolerance; bf16: the bar of
    tests/test_gpu_bf16.py for the exact mode, relative distance <= 0.3)"""
    import torch
    from jubatus_amd.ops import hip
    LC, mid = 2048, lo.AROW
    samples = [s for s in _edge_stream(LC, 100, 9)]
    bounds = [0, 20, 40, 60, 80, 100]
    act = _active(LC)
    oW, oP, upd, valid = _run_oracle(samples, LC, mid, act)
    rp, fi, fv, lab, sp, ns = _csr(samples, bounds)
    W, P, stats = _tables(LC, mid, torch.bfloat16 if wdt == "bf16" else torch.float32)
    scratch = hip.SerialScratch(_device())
    hip.linear_train(rp, fi, fv, lab, sp, ns, W, P, torch.from_numpy(act).to(_device()), mid, C,
                     hip.UPDATE_SERIAL, stats=stats, n_max=len(samples), scratch=scratch)
    torch.cuda.synchronize()
    assert scratch.last_batch() == {}        # no committer ran: nothing to report
    gW = W.float().cpu().numpy()
    if wdt == "fp32":
        assert stats.cpu().tolist() == [upd, valid]
        _close(gW, P.cpu().numpy(), oW, oP, mid)
    else:
        assert stats.cpu().tolist()[1] == valid
        assert np.linalg.norm(gW - oW) / np.linalg.norm(oW) <= 0.3


# ----------------------------------------------------------------- classify
@pytest.mark.parametrize("n", [1, 3, 70])
@pytest.mark.parametrize("LC", [2048, 16384])
def test_chunked_classify_every_column(LC, n):
    """fp32: against a float64 dot at 1e-5 relative to sum |x_i W_i| (at most
    70 terms: the worst-case fp32 bound is 70 * 2^-24 = 4.2e-6 of that sum; a
    bound relative to a cancelling sum itself holds for no fp32 summation).
    bf16: the bar of tests/test_gpu_bf16.py for the batched classify."""
    import torch
    from jubatus_amd.ops import hip
    rng = np.random.default_rng(LC + n)
    Wh = rng.normal(size=(H, LC)).astype(np.float32)
    samples = []
    for s in range(n):
        w = [70, 0, 1, 33][s % 4] if n > 1 else 70
        idx = rng.choice(H, w, replace=False).astype(np.int32)
        if w > 4:
            idx[2] = -1
        samples.append((0, idx, rng.normal(size=w).astype(np.float32)))
    rp, fi, fv, _, _, _ = _csr(samples)
    for dt in (torch.float32, torch.bfloat16):
        W = torch.from_numpy(Wh).to(_device()).to(dt)
        Wd = W.float().cpu().numpy().astype(np.float64)
        out = torch.full((n, LC), 7.0, device=_device())
        hip.linear_classify(rp, fi, fv, n, W, out)        # dispatches to the chunked kernel
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for s, (_, idx, val) in enumerate(samples):
            m = idx >= 0
            ref = val[m].astype(np.float64) @ Wd[idx[m]]
            mag = np.abs(val[m].astype(np.float64)) @ np.abs(Wd[idx[m]])
            if not m.any():
                assert not got[s].any()                    # a sample without features: zeros
            elif dt == torch.float32:
                assert np.all(np.abs(got[s] - ref) <= 1e-5 * mag), (s, np.abs(got[s] - ref).max())
                # 1e-5 relative to the float64 result itself wherever the terms do
                # not cancel: for |ref| >= mag / 2 the worst case above is
                # 2 * 4.2e-6 |ref|
                plain = np.abs(ref) >= 0.5 * mag
                assert np.all(np.abs(got[s] - ref)[plain] <= 1e-5 * np.abs(ref)[plain]), s
            else:
                assert np.all(np.abs(got[s] - ref) <= 1e-4 * (1 + np.abs(ref))), s


# ------------------------------------------------------------------- driver
CONV = {
    "string_rules": [{"key": "*", "type": "str", "sample_weight": "bin", "global_weight": "bin"}],
    "num_rules": [{"key": "*", "type": "num"}],
    "hash_max_size": 1024,
}


def _payload(nlabels, method="AROW"):
    return {"method": method, "H": 1024, "labels": [f"L{i}" for i in range(nlabels)],
            "counts": [0] * nlabels, "rows": b"", "W": b"", "P": b"", "weights": None}


def _data(n, labels, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        y = rng.choice(labels)
        out.append((f"L{y}", {"w": f"t{y % 53}", "u": f"n{rng.randrange(40)}",
                              "x": (y % 7 - 3) * 0.5 + rng.gauss(0, 1)}))
    return out


def _pair(wdt="fp32"):
    from jubatus_amd.models.classifier import LinearClassifier
    param = {"regularization_weight": 1.0}
    g = LinearClassifier("AROW", param, DatumToFvConverter(CONV), device=_device(), weight_dtype=wdt)
    c = LinearClassifier("AROW", param, DatumToFvConverter(CONV))
    return g, c


def _same_model(g, c):
    g.synchronize()
    assert g.LC == c.LC and g.get_labels() == c.get_labels()
    assert g.train_stats()["updated"] == c.train_stats()["updated"]
    _close(g.W.float().cpu().numpy(), g.P.cpu().numpy(), c.W, c.P, lo.AROW)


def test_driver_1500_labels_through_the_gpu_scan():
    """1500 registered labels: the request scan looks labels up in the global
    label table (past kLabCap = 32 of scan.hip), kSerial goes to the chunked
    kernel as one stream"""
    from jubatus_amd.fv_converter.datum import Datum
    from jubatus_amd.ops.feature_pipeline import RequestArena
    g, c = _pair()
    for m in (g, c):
        m.unpack(_payload(1500))
    assert g.LC == 2048 and g.W.shape == (1024, 2048)
    data = _data(320, [0, 1, 31, 32, 33, 700, 1023, 1024, 1025, 1499], seed=2)
    reqs = [data[i:i + 40] for i in range(0, len(data), 40)]
    bodies = [msgpack.packb([[l, Datum(d).to_msgpack()] for l, d in r], use_bin_type=False) for r in reqs]
    arena = RequestArena(sum(len(b) for b in bodies) + 16 * len(bodies) + 64)
    for b in bodies:
        arena.append(b)
    g.train_arena(arena, np.asarray(arena.offs, np.int64), np.asarray(arena.lens, np.int64))
    g.synchronize()
    g.pipe.check_errors()
    assert g.get_status()["train_scan.gpu"] == "1", g.get_status()
    for r in reqs:
        c.train(r)
    assert g.train_stats()["trained"] == len(data)
    _same_model(g, c)
    q = [d for _, d in data[:8]]
    for direct in (True, False):             # the direct path hands over to the batch path
        g.direct = direct
        for a, b in zip(g.classify(q), c.classify(q)):
            assert [x[0] for x in a] == [x[0] for x in b] and len(a) == 1500
            np.testing.assert_allclose([x[1] for x in a], [x[1] for x in b], rtol=2e-3, atol=2e-3)


def test_driver_grows_1024_to_2048_in_mid_stream():
    g, c = _pair()
    for m in (g, c):
        m.unpack(_payload(1000))
    first = _data(150, list(range(0, 1000, 9)), seed=3)
    cross = [(f"L{y}", {"w": f"t{y % 53}", "x": 0.5}) for y in range(1000, 1100)]
    last = _data(150, [3, 999, 1000, 1023, 1024, 1025, 1099], seed=4)
    for part in (first, cross, last):
        g.train(part)
        c.train(part)
        if part is first:
            assert g.LC == 1024 and g.W.shape[1] == 1024
    assert g.LC == 2048 and g.W.shape == (1024, 2048) and len(g.get_labels()) == 1100
    _same_model(g, c)


def test_driver_bf16_weights_at_2048():
    """bf16 W at label capacity 2048 under the bars of tests/test_gpu_bf16.py:
    relative distance to the fp32 oracle <= 0.3 in the exact mode, classify
    equal to the fp32 dot with the upcast table at 1e-4 (1 + |ref|)"""
    g, c = _pair("bf16")
    for m in (g, c):
        m.unpack(_payload(1100))
    data = _data(300, [0, 5, 600, 1023, 1024, 1099], seed=6)
    for i in range(0, len(data), 50):
        g.train(data[i:i + 50])
        c.train(data[i:i + 50])
    g.synchronize()
    assert g.LC == 2048 and g.W.dtype.itemsize == 2
    assert g.train_stats()["trained"] == len(data)
    Wg = g.W.float().cpu().numpy()
    rel = float(np.linalg.norm(Wg - c.W) / np.linalg.norm(c.W))
    print(f"bf16 at 2048: rel W diff {rel:.4f}")
    assert rel <= 0.3
    names = g.labels.names()
    test = [d for _, d in data[:30]]
    for d, r in zip(test, g.classify(test)):
        idx, val = g.conv.hashed(g.conv.convert(d))
        ref = np.asarray(val, np.float32) @ Wg[np.asarray(idx, np.int64)]
        got = dict(r)
        for i, n in enumerate(names):
            assert abs(got[n] - ref[i]) <= 1e-4 * (1 + abs(ref[i])), (n, got[n], ref[i])


def test_driver_refuses_growth_without_room(monkeypatch):
    import torch
    from jubatus_amd.models.classifier import ClassifierConfigError
    g, _ = _pair()
    g.unpack(_payload(1024))
    g.train(_data(60, [0, 500, 1023], seed=7))
    g.synchronize()
    W, P = g.W.clone(), g.P.clone()
    free = clf_mod.device_free_bytes(_device())
    assert free == torch.cuda.mem_get_info(_device())[0] and free > (1 << 30)
    monkeypatch.setattr(clf_mod, "device_free_bytes", lambda device: 1 << 20)
    need = g.table_bytes(2048)
    assert need == 1024 * 2048 * 8 + 4 * 2048
    with pytest.raises(ClassifierConfigError) as e:
        g.train([("label 1025", {"w": "a", "x": 1.0})])
    for part in ("1025 labels", "label capacity 2048", "hash_max_size 1024", f"{need} bytes",
                 f"{1 << 20} bytes are free"):
        assert part in str(e.value), (part, str(e.value))
    g.synchronize()
    assert g.LC == 1024 and g.W.shape == (1024, 1024) and len(g.get_labels()) == 1024
    assert torch.equal(g.W, W) and torch.equal(g.P, P)
    assert g.train(_data(10, [0, 500], seed=8)) == 10            # still serves
    g.synchronize()
    W = g.W.clone()
    monkeypatch.undo()
    assert g.set_label("label 1025") is True and g.LC == 2048
    assert torch.equal(g.W[:, :1024], W)


# ------------------------------------------------------- native GPU server
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_native_gpu_server_1100_labels(tmp_path):
    from jubatus_amd.common.mprpc import RpcClient, RpcIOError, RpcTimeoutError
    from jubatus_amd.framework.save_load import read_model_file
    from jubatus_amd.models.classifier import LinearClassifier

    conv = dict(CONV, string_filter_types={}, string_filter_rules=[], num_filter_types={},
                num_filter_rules=[], string_types={}, num_types={})
    cfg = {"converter": conv, "method": "AROW", "parameter": {"regularization_weight": 1.0}}
    cfg_file = tmp_path / "many.json"
    cfg_file.write_text(json.dumps(cfg))
    rng = random.Random(5)
    ys = list(range(1100)) + [rng.randrange(1100) for _ in range(100)]
    data = [[f"L{y}", [[["w", f"t{y % 53}"], ["u", f"n{rng.randrange(40)}"]],
                       [["x", (y % 7 - 3) * 0.5 + rng.gauss(0, 1)]], []]] for y in ys]
    q = [d for _, d in data[:10]]
    g = LinearClassifier("AROW", cfg["parameter"], DatumToFvConverter(cfg["converter"]),
                         device=_device())
    for i in range(0, len(data), 100):
        g.train([(l, d) for l, d in data[i:i + 100]])
    want = [dict(r) for r in g.classify(q)]
    port = _free_port()
    p = subprocess.Popen([BIN, "-p", str(port), "-b", "127.0.0.1", "-f", str(cfg_file), "-d",
                          str(tmp_path), "-c", "4"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    c = None
    try:
        deadline = time.time() + 60
        while c is None and time.time() < deadline:
            try:
                c = RpcClient("127.0.0.1", port, 60.0)
                c.call("get_config", "")
            except (OSError, RpcIOError, RpcTimeoutError):
                c = None
                assert p.poll() is None, p.stdout.read().decode(errors="replace")
                time.sleep(0.2)
        assert c is not None
        for i in range(0, len(data), 100):
            assert c.call("train", "", data[i:i + 100]) == 100
        got = [{(k.decode() if isinstance(k, bytes) else k): v for k, v in r}
               for r in c.call("classify", "", q)]
        (_, st), = c.call("get_status", "").items()
        st = {(k.decode() if isinstance(k, bytes) else k): (v.decode() if isinstance(v, bytes) else v)
              for k, v in st.items()}
        assert st["storage"] == "hbm" and st["label_capacity"] == "2048", st
        assert int(st["train.samples_updated"]) == g.train_stats()["updated"]
        scale = max(abs(v) for w in want for v in w.values())
        for a, b in zip(got, want):
            assert sorted(a) == sorted(b) and len(a) == 1100
            for k in b:
                assert abs(a[k] - b[k]) <= 2e-3 * abs(b[k]) + 2e-3 * scale, (k, a[k], b[k])
        (_, path), = c.call("save", "", "many").items()
        path = path.decode() if isinstance(path, bytes) else path
    finally:
        if c is not None:
            c.close()
        p.terminate()
        try:
            p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            p.kill()
    # the server's model file into the Python GPU driver
    g2 = LinearClassifier("AROW", cfg["parameter"], DatumToFvConverter(cfg["converter"]),
                          device=_device())
    with open(path, "rb") as f:
        _, userobj = read_model_file(f)
    g2.unpack(userobj[1])
    assert g2.LC == 2048 and len(g2.get_labels()) == 1100
    for a, b in zip([dict(r) for r in g2.classify(q)], got):
        assert sorted(a) == sorted(b)
        for k in b:
            assert abs(a[k] - b[k]) <= 1e-5 * max(1.0, abs(b[k])), (k, a[k], b[k])
