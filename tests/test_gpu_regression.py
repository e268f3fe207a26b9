"""csrc/hip/regression.hip (K5) against a float64 sequential reference written
here, independent of models/regression.py: sample widths past one 64-lane
chunk, skipped (idx == -1) slots, an index repeated inside a sample (every
occurrence counts, in w.x, in ||x||^2 and in the update), degenerate samples,
back-to-back row reuse, statistics carried over launches, the concurrent
kernel (wave -> stream mapping, empty streams, atomics on shared rows), the
estimate kernel, and the Python driver against the host oracle.

The tests call ops/hip.py regression_train / regression_estimate on CSR
tensors they build. Inputs: values N(0,1)/sqrt(width) (so ||x||^2 ~ 1 at every
width), targets mean + w_true.x + noise (spread ~ 1), initial w = w_true + a
perturbation, so with C = 0.05 part of the updating samples clip and part do
not (asserted on the reference).

Bound (the project's regression bound, tests/test_gpu_engines.py): W at
rtol 1e-3, atol 1e-4 * max|W_ref|; statistics at rtol 1e-4; estimates at
rtol 1e-4, atol 1e-4. The PA update is continuous in the state, so a float64
reference stays close to any correct fp32 kernel. Measured on the host with
an fp32 NumPy emulation of the kernel's rule on these generators, deviation
from the float64 reference as max|dW| / max|W_ref| (bound 1e-4: every case is
below a tenth of it) and max relative statistics deviation (bound 1e-4), for
C = 3.40282e38 / C = 0.05:
    widths          W 2.4e-7 / 5.1e-7, statistics 4.4e-7
    skipped slots   W 1.3e-7 / 1.2e-7, statistics 5.8e-7
    repeated index  W 1.3e-7 / 8.9e-8, statistics 1.7e-7
    degenerate      W 1.6e-7 / 2.5e-7, statistics 1.3e-7
    row reuse       W 7.8e-8 / 2.4e-7, statistics 1.8e-7
    non-zero mean   W 1.8e-6 / 2.3e-6, statistics 3.6e-7
    disjoint, 2..9  W at most 3.6e-7 / 2.5e-7, statistics at most 9.7e-7
    shared rows     W 1.1e-6 (C = 1e-3), statistics exact
    estimate        at most 5.4e-6 absolute over n = 1..130 (bound 1e-4 absolute)
The same emulation with a last-wins store deviates on the repeated-index
stream by 0.11 / 0.041 of max|W_ref|.
"""
import math
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = 512
FLT_MAX = 3.40282e38
C_VALUES = [FLT_MAX, 0.05]
WIDTHS = [1, 2, 63, 64, 65, 127, 128, 129, 200]


def dev():
    import torch
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ inputs
class Stream:
    """samples as host CSR arrays, in the dtypes the kernels take"""

    def __init__(self, samples, targets):
        self.n = len(samples)
        self.row_ptr = np.zeros(self.n + 1, np.int64)
        self.row_ptr[1:] = np.cumsum([len(i) for i, _ in samples])
        self.fidx = np.concatenate([np.asarray(i, np.int32) for i, _ in samples] + [np.zeros(0, np.int32)])
        self.fval = np.concatenate([np.asarray(v, np.float32) for _, v in samples] + [np.zeros(0, np.float32)])
        self.targets = np.asarray(targets, np.float32)

    def part(self, a, b):
        s = Stream.__new__(Stream)
        s.n = b - a
        s.row_ptr = self.row_ptr[a:b + 1] - self.row_ptr[a]
        s.fidx = self.fidx[self.row_ptr[a]:self.row_ptr[b]]
        s.fval = self.fval[self.row_ptr[a]:self.row_ptr[b]]
        s.targets = self.targets[a:b]
        return s


def _slots(rng, width, pool, distinct=True):
    idx = rng.choice(pool, size=width, replace=not distinct).astype(np.int32)
    val = (rng.standard_normal(width) / math.sqrt(max(width, 1))).astype(np.float32)
    return idx, val


def _model(rng, h, delta=0.12):
    """(w_true, initial w): the initial error of a sample is ~ N(0, delta^2)"""
    wt = rng.standard_normal(h)
    return wt, (wt + delta * rng.standard_normal(h)).astype(np.float32)


def _targets(rng, samples, wt, mean=0.0, noise=0.12):
    ys = []
    for idx, val in samples:
        m = idx >= 0
        ys.append(mean + float(np.dot(val[m].astype(np.float64), wt[idx[m]])) + noise * rng.standard_normal())
    return ys


def case_widths():
    rng = np.random.default_rng(1)
    wt, w0 = _model(rng, H)
    samples = [_slots(rng, WIDTHS[s % len(WIDTHS)], H) for s in range(400)]
    return Stream(samples, _targets(rng, samples, wt)), w0


def case_skipped():
    """every sample has a -1 slot in chunk 0; samples of 65+ slots also at
    position 64 and at their last position. Skipped slots carry large values."""
    rng = np.random.default_rng(2)
    wt, w0 = _model(rng, H)
    samples = []
    for s in range(120):
        width = [2, 5, 65, 100, 130, 200][s % 6]
        idx, val = _slots(rng, width, H)
        skip = [int(rng.integers(0, min(width, 64)))]
        if width >= 65:
            skip += [64, width - 1]
        idx[skip] = -1
        val[skip] = 3.0
        samples.append((idx, val))
    return Stream(samples, _targets(rng, samples, wt)), w0


def case_repeated():
    """the last slot repeats the first slot's index (widths 2, 5: both in
    chunk 0; 65, 130: in different chunks); every fifth sample carries one
    index three times"""
    rng = np.random.default_rng(3)
    wt, w0 = _model(rng, H)
    samples = []
    for s in range(100):
        k = s % 5
        if k < 4:
            idx, val = _slots(rng, [2, 5, 65, 130][k], H)
            idx[-1] = idx[0]
        else:
            idx, val = _slots(rng, 7, H)
            idx[3] = idx[6] = idx[0]
        samples.append((idx, val))
    return Stream(samples, _targets(rng, samples, wt)), w0


DEGENERATE_H = 64


def _degenerate(rng, kind):
    if kind == "empty":
        return np.zeros(0, np.int32), np.zeros(0, np.float32)
    if kind.startswith("skip"):
        width = int(kind[4:])
        return np.full(width, -1, np.int32), _slots(rng, width, DEGENERATE_H, distinct=False)[1]
    width = int(kind[4:])                      # "zero<width>"
    return _slots(rng, width, DEGENERATE_H, distinct=False)[0], np.zeros(width, np.float32)


DEGENERATE_KINDS = ["empty", "skip3", "skip70", "zero5", "zero66"]


def case_degenerate():
    """ordinary samples with an empty sample, all-skipped samples and all-zero
    samples among them, one first and one last; their targets are ~2, so the
    loss is positive and only the ||x||^2 > 0 guard keeps them from updating"""
    rng = np.random.default_rng(4)
    wt, w0 = _model(rng, DEGENERATE_H)
    plan = ["empty", 12, "skip3", 9, "skip70", "zero5", 9, "empty", "zero66", 12, "skip3", 8, "zero5"]
    samples, degenerate = [], []
    for p in plan:
        if isinstance(p, int):
            samples += [_slots(rng, [3, 20, 64, 65, 40][j % 5], DEGENERATE_H, distinct=False) for j in range(p)]
        else:
            degenerate.append(len(samples))
            samples.append(_degenerate(rng, p))
    ys = _targets(rng, samples, wt)
    for s in degenerate:
        ys[s] = 2.0 + 0.3 * rng.standard_normal()
    return Stream(samples, ys), w0


def case_row_reuse():
    rng = np.random.default_rng(5)
    wt, w0 = _model(rng, 8)
    samples = [_slots(rng, 5, 8) for _ in range(200)]
    return Stream(samples, _targets(rng, samples, wt)), w0


def case_nonzero_mean():
    """targets 50 + unit spread; the last slot of every sample is a bias
    feature (row H - 1, value 1) whose initial weight is ~50, so the errors
    stay of order 0.1 and the stddev comes from sum2/n - mean^2 near 2500"""
    rng = np.random.default_rng(6)
    wt, w0 = _model(rng, H)
    wt[H - 1] = 0.0
    w0[H - 1] = np.float32(50.0 + 0.12 * rng.standard_normal())
    samples = []
    for s in range(400):
        idx, val = _slots(rng, WIDTHS[s % len(WIDTHS)] - 1, H - 1)
        samples.append((np.append(idx, np.int32(H - 1)), np.append(val, np.float32(1.0))))
    return Stream(samples, _targets(rng, samples, wt, mean=50.0)), w0


STATS0 = np.array([12.5, 40.0, 10.0], np.float32)
EMPTY_STREAMS = {2: (), 3: (1,), 4: (3,), 5: (2, 4), 9: (4, 8)}


def case_disjoint(nstreams):
    """stream k draws from rows [k * H // nstreams, (k + 1) * H // nstreams);
    unequal lengths, empty streams as EMPTY_STREAMS (a middle one, the last
    one, or both), widths 3 / 64 / 65 / 130, every third sample repeats its
    first index in its last slot, and samples wider than the slice repeat
    indices freely. -> (stream, stream_ptr, initial w)"""
    rng = np.random.default_rng(10 + nstreams)
    wt, w0 = _model(rng, H, delta=0.04)       # sensitivity 0: every sample updates, C clips past 0.05
    samples, sp = [], [0]
    for k in range(nstreams):
        pool = np.arange(k * H // nstreams, (k + 1) * H // nstreams)
        n = 0 if k in EMPTY_STREAMS[nstreams] else 2 * (9 + 7 * ((3 * k) % 5) + k)
        for j in range(n):
            width = [3, 64, 65, 130][(j + k) % 4]
            idx, val = _slots(rng, width, pool, distinct=width <= len(pool))
            if j % 3 == 0:
                idx[-1] = idx[0]
            samples.append((idx, val))
        sp.append(len(samples))
    return Stream(samples, _targets(rng, samples, wt, noise=0.04)), np.asarray(sp, np.int64), w0


SHARED_C = 1e-3


def case_shared():
    """9 streams x 8 samples over 16 rows, indices drawn with replacement;
    every target is +100"""
    rng = np.random.default_rng(20)
    w0 = (0.01 * rng.standard_normal(16)).astype(np.float32)
    samples = [_slots(rng, [3, 64, 65, 130][s % 4], 16, distinct=False) for s in range(72)]
    return Stream(samples, [100.0] * 72), np.arange(0, 73, 8, dtype=np.int64), w0


ESTIMATE_H = 64


def case_estimate(n):
    """widths 64, 65, 200, 0, 1, ... over 64 rows with replacement (repeated
    indices); -1 slots with non-zero values at position 1 and at position 64"""
    rng = np.random.default_rng(30 + n)
    w = rng.standard_normal(ESTIMATE_H).astype(np.float32)
    samples = []
    for s in range(n):
        width = [0, 1, 64, 65, 200][(s + 2) % 5]
        idx, val = _slots(rng, width, ESTIMATE_H, distinct=False)
        val *= math.sqrt(max(width, 1))
        for pos in (1, 64):
            if pos < width:
                idx[pos] = -1
                val[pos] = 3.0
        samples.append((idx, val))
    return Stream(samples, np.zeros(n)), w


# --------------------------------------------------------------- reference
def ref_train(w, stats, st, C, eps, log=None):
    """the PA regression rule in float64, one sample after the other, on the
    fp32-rounded inputs; w (float64[H]) and stats (float64[3]) in place.
    log: per updating sample (clipped, |w.x|) is appended"""
    C = float(np.float32(C))
    eps = float(np.float32(eps))
    for s in range(st.n):
        a, b = int(st.row_ptr[s]), int(st.row_ptr[s + 1])
        idx = st.fidx[a:b].astype(np.int64)
        x = st.fval[a:b].astype(np.float64)
        keep = idx >= 0
        idx, x = idx[keep], x[keep]
        dot = float(np.dot(x, w[idx]))          # a repeated index: once per occurrence
        nrm = float(np.dot(x, x))
        y = float(st.targets[s])
        stats += (y, y * y, 1.0)
        avg = stats[0] / stats[2]
        sd = math.sqrt(max(0.0, stats[1] / stats[2] - avg * avg))
        err = y - dot
        loss = abs(err) - eps * sd
        if loss > 0 and nrm > 0:
            np.add.at(w, idx, (1.0 if err > 0 else -1.0) * min(C, loss) / nrm * x)
            if log is not None:
                log.append((loss > C, abs(dot)))


def reference(st, w0, C, eps, stats0=None):
    w = w0.astype(np.float64)
    stats = np.zeros(3) if stats0 is None else stats0.astype(np.float64)
    log = []
    ref_train(w, stats, st, C, eps, log)
    return w, stats, log


def check_clip_balance(log, C):
    """with the clipping C at least a quarter of the updating samples clip and
    at least a quarter do not; with C = FLT_MAX none can"""
    clipped = sum(1 for c, _ in log if c)
    assert len(log) >= 20, len(log)
    if C == FLT_MAX:
        assert clipped == 0
    else:
        assert 4 * clipped >= len(log) and 4 * (len(log) - clipped) >= len(log), (clipped, len(log))


# ------------------------------------------------------------------ device
def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def gpu_train(st, W, stats, C, eps, stream_ptr=None, concurrent=False):
    from jubatus_amd.ops import hip
    assert st.fidx.size == 0 or (int(st.fidx.max()) < W.numel() and int(st.row_ptr[-1]) == st.fidx.size)
    sp = np.asarray([0, st.n], np.int64) if stream_ptr is None else stream_ptr
    assert int(sp[-1]) == st.n and np.all(np.diff(sp) >= 0)
    hip.regression_train(_t(st.row_ptr), _t(st.fidx), _t(st.fval), _t(st.targets), _t(sp), len(sp) - 1,
                         W, stats, C, eps, concurrent=concurrent)


def assert_state(W, stats, w_ref, stats_ref):
    got_w, got_s = W.cpu().numpy(), stats.cpu().numpy()
    scale = float(np.abs(w_ref).max())
    print("max|dW|/max|W_ref| = %.3g, max rel stats = %.3g"
          % (np.abs(got_w - w_ref).max() / scale, np.abs(got_s / stats_ref - 1.0).max()))
    np.testing.assert_allclose(got_w, w_ref, rtol=1e-3, atol=1e-4 * scale)
    np.testing.assert_allclose(got_s, stats_ref, rtol=1e-4)


# -------------------------------------------------------------- exact mode
EXACT_CASES = {"widths": case_widths, "skipped": case_skipped, "repeated": case_repeated,
               "degenerate": case_degenerate, "row_reuse": case_row_reuse, "nonzero_mean": case_nonzero_mean}


@pytest.mark.parametrize("C", C_VALUES)
@pytest.mark.parametrize("case", list(EXACT_CASES))
def test_exact_stream_matches_float64_reference(case, C):
    import torch
    st, w0 = EXACT_CASES[case]()
    w_ref, stats_ref, log = reference(st, w0, C, 0.1)
    check_clip_balance(log, C)
    W, stats = _t(w0), torch.zeros(3, dtype=torch.float32, device=dev())
    gpu_train(st, W, stats, C, 0.1)
    assert_state(W, stats, w_ref, stats_ref)


@pytest.mark.parametrize("C", C_VALUES)
@pytest.mark.parametrize("kind", DEGENERATE_KINDS)
def test_degenerate_sample_changes_statistics_only(kind, C):
    """one launch of one empty / all-skipped / all-zero sample on a trained
    model: W keeps every bit, the statistics take the target"""
    rng = np.random.default_rng(7)
    w0 = rng.standard_normal(DEGENERATE_H).astype(np.float32)
    st = Stream([_degenerate(rng, kind)], [2.5])
    W, stats = _t(w0), _t(STATS0)
    gpu_train(st, W, stats, C, 0.1)
    np.testing.assert_array_equal(W.cpu().numpy(), w0)
    np.testing.assert_allclose(stats.cpu().numpy(), STATS0.astype(np.float64) + (2.5, 6.25, 1.0), rtol=1e-4)


@pytest.mark.parametrize("C", C_VALUES)
def test_statistics_and_w_carry_over_launches(C):
    """the widths stream in launches of 1, 7, 50 samples and the rest == the
    one-launch reference; a launch without streams changes nothing"""
    import torch
    st, w0 = case_widths()
    w_ref, stats_ref, _ = reference(st, w0, C, 0.1)
    W, stats = _t(w0), torch.zeros(3, dtype=torch.float32, device=dev())
    for a, b in ((0, 1), (1, 8), (8, 58)):
        gpu_train(st.part(a, b), W, stats, C, 0.1)
    before = (W.clone(), stats.clone())
    gpu_train(st.part(58, 58), W, stats, C, 0.1, stream_ptr=np.zeros(1, np.int64))
    assert torch.equal(W, before[0]) and torch.equal(stats, before[1])
    gpu_train(st.part(58, st.n), W, stats, C, 0.1)
    assert_state(W, stats, w_ref, stats_ref)


# --------------------------------------------------------- concurrent mode
@pytest.mark.parametrize("C", C_VALUES)
@pytest.mark.parametrize("nstreams", sorted(EMPTY_STREAMS))
def test_concurrent_disjoint_streams_match_per_stream_reference(nstreams, C):
    """streams on disjoint rows with sensitivity 0 do not interact: W is each
    stream's sequential result and the statistics take every sample once.
    (With sensitivity > 0 a wave's stddev depends on which other waves had
    already added their deltas when it started: timing-dependent by design.)"""
    st, sp, w0 = case_disjoint(nstreams)
    assert len(sp) == nstreams + 1 and st.n <= 400
    assert len(set(np.diff(sp)[np.diff(sp) > 0])) == np.count_nonzero(np.diff(sp))   # unequal lengths
    w_ref, stats_ref, log = reference(st, w0, C, 0.0, STATS0)
    check_clip_balance(log, C)
    W, stats = _t(w0), _t(STATS0)
    gpu_train(st, W, stats, C, 0.0, stream_ptr=sp, concurrent=True)
    assert_state(W, stats, w_ref, stats_ref)


def test_concurrent_shared_rows_clipped_updates_commute():
    """every target is +100 and C is 1e-3, so every sample has err > 0 and
    clips whatever the streams' interleaving: its increment is C / ||x||^2 * x,
    and W = W0 + the sum of them over every occurrence, in any order"""
    st, sp, w0 = case_shared()
    C = float(np.float32(SHARED_C))
    w_ref = w0.astype(np.float64)
    grow, reach = float(np.abs(w0).max()), 0.0
    for s in range(st.n):
        a, b = int(st.row_ptr[s]), int(st.row_ptr[s + 1])
        x = st.fval[a:b].astype(np.float64)
        np.add.at(w_ref, st.fidx[a:b].astype(np.int64), C / np.dot(x, x) * x)
        grow += C / np.dot(x, x) * np.abs(x).max()
        reach = max(reach, np.abs(x).sum())
    assert grow * reach < 50.0            # |w.x| < 50 under any interleaving: err > 0, loss > C
    w_seq, stats_ref, log = reference(st, w0, SHARED_C, 0.0, STATS0)
    assert len(log) == st.n and all(c and d < 1.0 for c, d in log)
    np.testing.assert_allclose(w_seq, w_ref, rtol=1e-12)
    W, stats = _t(w0), _t(STATS0)
    gpu_train(st, W, stats, SHARED_C, 0.0, stream_ptr=sp, concurrent=True)
    assert_state(W, stats, w_ref, stats_ref)


# ----------------------------------------------------------------- estimate
@pytest.mark.parametrize("n", [1, 3, 4, 5, 130])
def test_estimate_matches_float64_dot(n):
    import torch
    from jubatus_amd.ops import hip
    st, w = case_estimate(n)
    ref = np.zeros(n)
    for s in range(n):
        a, b = int(st.row_ptr[s]), int(st.row_ptr[s + 1])
        idx = st.fidx[a:b].astype(np.int64)
        ref[s] = np.dot(st.fval[a:b][idx >= 0].astype(np.float64), w[idx[idx >= 0]].astype(np.float64))
    out = torch.full((n + 3,), -777.0, dtype=torch.float32, device=dev())
    hip.regression_estimate(_t(st.row_ptr), _t(st.fidx), _t(st.fval), n, _t(w), out)
    got = out.cpu().numpy()
    print("max |d estimate| = %.3g" % np.abs(got[:n] - ref).max())
    np.testing.assert_allclose(got[:n], ref, rtol=1e-4, atol=1e-4)
    assert np.all(got[n:] == -777.0)
    empty = np.flatnonzero(np.diff(st.row_ptr) == 0)
    assert (len(empty) > 0) == (n >= 4)
    assert np.all(got[empty] == 0.0)


# ------------------------------------------------------------------ drivers
def _driver_data(kind, n):
    """wide: 100 num keys per datum. dup: a num key repeated inside the datum
    (two slots with one hashed index), as test_gpu_linear.py _shared_data"""
    rng = random.Random(41)
    coef = [rng.gauss(0, 1) for _ in range(100)]
    out = []
    for _ in range(n):
        if kind == "wide":
            nv = [[f"n{j}", rng.gauss(0, 0.1)] for j in range(100)]
            y = sum(c * v for c, (_, v) in zip(coef, nv))
        else:
            nv = [[f"n{j}", rng.gauss(0, 1)] for j in range(3)] + [["bias", 1.0], ["n0", 0.5 + rng.random()]]
            y = sum(c * v for c, (_, v) in zip(coef, nv[:3])) + 1.0 + coef[0] * nv[4][1]
        out.append([y + rng.gauss(0, 0.1), [[], nv, []]])
    return out


@pytest.mark.parametrize("batch", [1, 50])
@pytest.mark.parametrize("kind", ["wide", "dup"])
def test_driver_matches_host_oracle(kind, batch):
    """PARegression on the device == on the host (models/regression.py
    train_one, per occurrence) for wide datums and repeated keys"""
    from test_gpu_engines import CONV
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.models.regression import PARegression
    p = {"sensitivity": 0.1, "regularization_weight": 2.0}
    g = PARegression("PA", p, DatumToFvConverter(CONV), dev())
    c = PARegression("PA", p, DatumToFvConverter(CONV))
    data = _driver_data(kind, 100)
    for i in range(0, len(data), batch):
        assert g.train(data[i:i + batch]) == c.train(data[i:i + batch]) == len(data[i:i + batch])
    assert_state(g.w, g.stats, c.w.astype(np.float64), c.stats)
    q = [d for _, d in data[:20]]
    np.testing.assert_allclose(g.estimate(q), c.estimate(q), rtol=1e-4, atol=1e-4)
