"""The nearest-neighbour classifiers on the device: csrc/hip/nn_vote.hip against
the float64 vote of tests/test_nn_vote.py on synthetic top-k lists, the GPU
driver's fused classify (models/nn_classifier.py: device top-k + nn_vote)
against its per-datum path on the same model, the ``row_lab`` invariant on the
device tensor, and the Python server with a GPU against a CPU driver.

Kernel bound, per (query, label) with n kept entries of that label:
|out - ref| <= (n + 8) 2^-23 sum|w|: the fp32 summation bound for any order
(n 2^-24 relative to sum|w|) plus a few ulps for expf / 1 - d. Distances are
below 1.5 where alpha > 0 is 1 or less, so the rounding of alpha * d moves
exp by less than 2 ulps. Columns without a kept entry are exactly 0.0, and
the words around ``out`` keep their sentinel.

The fused classify is compared with the float64 vote over the fp32 values the
same engine's query_datum reports for the same query (the per-datum path,
``_classify_each``), under the same bound; the cases have a gap at the k-th
neighbour (asserted on the CPU driver by tests/test_nn_vote.py, and again
here), so both paths keep the same rows.
"""
import json
import os

import numpy as np
import pytest

from helpers import ROOT
from test_nn_regression import datum, make_data
from test_nn_vote import (DRIVER_CASES, GROWTH_CASE, NQ, check_row_lab, driver, kth_gap_holds,
                          labelled, make_labelled, neighbour_stats, params, vote64)

pytestmark = pytest.mark.gpu

NROWS = 1000
NN_CFG = os.path.join(ROOT, "config", "classifier", "nn.json")
INT_MAX = 2 ** 31 - 1
EPS = 2.0 ** -23
SENTINEL = -777.25
GUARD = 64


def dev():
    import torch
    return torch.device("cuda", 0)


def lists(nq, k, nlabels, seed, lo=0.0, hi=1.5):
    """[nq, k] ascending distances in [lo, hi), rows in [0, NROWS) and a label
    table. By query q % 4: 0 nothing padded, 1 a padded tail, 2 all padded
    (nq > 2), 3 a padded tail plus entries whose row is >= NROWS or negative
    (finite distance); a NaN distance in every query with k > 2. The label
    table holds ids in [0, nlabels) and, about one slot in ten each, -1,
    nlabels, INT_MAX and a negative id."""
    rng = np.random.default_rng(seed)
    dist = np.sort(rng.uniform(lo, hi, (nq, k)).astype(np.float32), axis=1)
    row = rng.integers(0, NROWS, (nq, k)).astype(np.int32)
    for q in range(nq):
        kind = q % 4
        keep = k if kind == 0 else 0 if kind == 2 else int(rng.integers(0, k + 1))
        dist[q, keep:] = np.inf
        row[q, keep:] = INT_MAX
        if kind == 3 and keep:
            row[q, int(rng.integers(keep))] = NROWS + int(rng.integers(0, 5))
            row[q, int(rng.integers(keep))] = -1 - int(rng.integers(0, 5))
        if k > 2:
            dist[q, int(rng.integers(k))] = np.nan
    row_lab = rng.integers(0, nlabels, NROWS).astype(np.int32)
    kind = rng.integers(0, 10, NROWS)
    row_lab[kind == 0] = -1
    row_lab[kind == 1] = nlabels
    row_lab[kind == 2] = INT_MAX
    row_lab[kind == 3] = -7
    return dist, row, row_lab


def launch(dist, row, row_lab, nlabels, mode, alpha, nrows=NROWS):
    """-> (out [nq, nlabels], the guard words in front of and behind it); out
    is a view into a buffer filled with SENTINEL before the call"""
    import torch
    from jubatus_amd.ops import hip
    nq, k = dist.shape
    d = torch.from_numpy(dist).to(dev())
    r = torch.from_numpy(row).to(dev())
    t = torch.from_numpy(row_lab).to(dev())
    buf = torch.full((2 * GUARD + nq * nlabels,), SENTINEL, dtype=torch.float32, device=dev())
    out = buf[GUARD:GUARD + nq * nlabels]
    got = hip.nn_vote(d, r, nq, k, t, nrows, nlabels, mode, alpha, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    return out.view(nq, nlabels), torch.cat([buf[:GUARD], buf[GUARD + nq * nlabels:]])


def check(dist, row, row_lab, nlabels, mode, alpha, tag, nrows=NROWS):
    out, guard = launch(dist, row, row_lab, nlabels, mode, alpha, nrows)
    out, guard = out.cpu().numpy(), guard.cpu().numpy()
    ref, n, scale = vote64(dist, row, row_lab, nrows, nlabels, mode, alpha)
    err = np.abs(out.astype(np.float64) - ref)
    bound = (n + 8) * EPS * scale
    worst = np.unravel_index(int(np.argmax(err - bound)), err.shape)
    print(f"{tag}: max err {err.max():.3g}; worst (q, label) {worst}: err {err[worst]:.3g}, "
          f"bound {bound[worst]:.3g}, kept {int(n.sum())}")
    assert np.all(guard == np.float32(SENTINEL))
    assert np.all(out != np.float32(SENTINEL))               # every element written
    assert np.all(err <= bound)
    assert np.all(out[n == 0] == 0.0)
    return out, ref, n


@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("nlabels", [1, 2, 64, 65, 300])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 128, 129, 200])
def test_kernel_matches_the_float64_vote(k, nlabels, nq):
    dist, row, row_lab = lists(nq, k, nlabels, 100000 * k + 100 * nlabels + nq)
    kept = 0
    for mode, alpha in ((0, 1.0), (0, 0.5), (0, 0.0), (1, 0.0)):
        _, _, n = check(dist, row, row_lab, nlabels, mode, alpha,
                        f"k={k} L={nlabels} nq={nq} mode={mode} alpha={alpha}")
        kept += int(n.sum())
    if k > 2:
        assert kept > 0


@pytest.mark.parametrize("k", [1, 64, 65, 200])
def test_every_neighbour_on_one_label(k):
    rng = np.random.default_rng(k)
    dist = np.sort(rng.uniform(0, 1.5, (5, k)).astype(np.float32), axis=1)
    row = rng.integers(0, NROWS, (5, k)).astype(np.int32)
    row_lab = np.full(NROWS, 70, np.int32)
    for mode in (0, 1):
        out, _, n = check(dist, row, row_lab, 72, mode, 1.0, f"one label k={k} mode={mode}")
        assert np.all(n[:, 70] == k) and n.sum() == 5 * k
        assert np.all(out[:, :70] == 0) and np.all(out[:, 71] == 0) and np.all(out[:, 70] != 0)


@pytest.mark.parametrize("k", [2, 64, 65, 129, 200])
def test_every_neighbour_on_a_distinct_label(k):
    rng = np.random.default_rng(1000 + k)
    dist = np.sort(rng.uniform(0, 1.5, (5, k)).astype(np.float32), axis=1)
    row = np.stack([rng.permutation(NROWS)[:k] for _ in range(5)]).astype(np.int32)
    for nlabels in (k, 300 if k <= 300 else k):
        row_lab = (rng.permutation(NROWS) % nlabels).astype(np.int32)
        row_lab[row[0]] = rng.permutation(nlabels)[:k]      # query 0: k distinct ids
        for mode in (0, 1):
            _, _, n = check(dist, row, row_lab, nlabels, mode, 0.5,
                            f"distinct labels k={k} L={nlabels} mode={mode}")
            assert n[0].max() == 1 and n[0].sum() == k


def test_alpha_zero_counts_the_neighbours():
    dist, row, row_lab = lists(5, 129, 65, 5)
    out, _, n = check(dist, row, row_lab, 65, 0, 0.0, "alpha 0")
    assert np.array_equal(out, n.astype(np.float32))        # every weight is exactly 1


def test_expf_underflow_gives_zero_votes():
    dist, row, row_lab = lists(5, 128, 7, 6, lo=100.0, hi=200.0)
    finite = dist[np.isfinite(dist)].astype(np.float64)
    assert finite.size and np.all(np.exp(-50.0 * finite) == 0)      # in float64 too
    out, _, n = check(dist, row, row_lab, 7, 0, 50.0, "alpha d in [5000, 10000]")
    assert n.sum() > 0 and np.all(out == 0)


def test_cosine_mode_sums_negative_votes():
    dist, row, row_lab = lists(5, 200, 3, 7, lo=1.0, hi=2.0)          # cosine in (-1, 0]
    out, ref, n = check(dist, row, row_lab, 3, 1, 1.0, "mode 1, d in [1, 2)")
    assert np.all(out[n > 0] < 0) and ref.min() < -10                 # no clamp at 0


def test_out_of_range_labels_and_rows_vote_for_nothing():
    rng = np.random.default_rng(8)
    dist = np.sort(rng.uniform(0, 1.5, (5, 65)).astype(np.float32), axis=1)
    row = rng.integers(0, NROWS, (5, 65)).astype(np.int32)
    for bad in (-1, 4, INT_MAX, -INT_MAX - 1, 1 << 20):
        out, _, n = check(dist, row, np.full(NROWS, bad, np.int32), 4, 0, 1.0, f"row_lab {bad}")
        assert n.sum() == 0 and np.all(out == 0)
    row_lab = np.zeros(NROWS, np.int32)
    for bad in (-1, NROWS, INT_MAX, -INT_MAX - 1):
        out, _, n = check(dist, np.full_like(row, bad), row_lab, 4, 0, 1.0, f"row {bad}")
        assert n.sum() == 0 and np.all(out == 0)
    out, _, n = check(dist, row, row_lab, 4, 0, 1.0, "nrows 0", nrows=0)
    assert n.sum() == 0 and np.all(out == 0)
    out, _, _ = check(dist[:, :0], row[:, :0], row_lab, 4, 0, 1.0, "k 0")
    assert out.shape == (5, 4) and np.all(out == 0)


def test_two_launches_give_the_same_bits():
    import torch
    for nlabels in (2, 65, 300):
        dist, row, row_lab = lists(5, 200, nlabels, 9)
        for mode in (0, 1):
            a, _ = launch(dist, row, row_lab, nlabels, mode, 0.5)
            b, _ = launch(dist, row, row_lab, nlabels, mode, 0.5)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_bad_arguments_return_minus_two_without_a_launch():
    import torch
    from jubatus_amd.ops import hip
    dist, row, row_lab = lists(2, 4, 3, 3)
    d, r, t = (torch.from_numpy(x).to(dev()) for x in (dist, row, row_lab))
    out = torch.full((2, 3), SENTINEL, dtype=torch.float32, device=dev())
    fn = hip._fn("jb_nn_vote")
    stream = torch.cuda.current_stream().cuda_stream
    P = lambda x: x.data_ptr()                                        # noqa: E731
    good = [P(d), P(r), 2, 4, P(t), NROWS, 3, 0, 1.0, P(out), stream]
    for pos, bad in ((3, -1), (5, -1), (6, 0), (6, -3), (7, 2), (7, -1), (8, -1.0),
                     (8, float("inf")), (8, float("nan")), (9, None), (0, None), (1, None),
                     (4, None)):
        args = list(good)
        args[pos] = bad
        assert fn(*args) == -2, (pos, bad)
    args = list(good)
    args[2] = 0
    args[6] = 0                                                       # nq <= 0 comes first
    assert fn(*args) == 0
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)                                 # nothing was launched
    assert fn(*good) == 0
    torch.cuda.synchronize()
    assert torch.all(out != SENTINEL)
    # the wrapper's operand checks
    with pytest.raises(TypeError):
        hip.nn_vote(d, r.to(torch.int64), 2, 4, t, NROWS, 3, 0, 1.0)
    with pytest.raises(TypeError):
        hip.nn_vote(d, r, 2, 4, t.to(torch.int64), NROWS, 3, 0, 1.0)
    with pytest.raises(TypeError):
        hip.nn_vote(d.cpu(), r, 2, 4, t, NROWS, 3, 0, 1.0)
    with pytest.raises(ValueError):
        hip.nn_vote(d, r, 3, 4, t, NROWS, 3, 0, 1.0)
    with pytest.raises(ValueError):
        hip.nn_vote(d, r, 2, 4, t, NROWS + 1, 3, 0, 1.0)
    with pytest.raises(ValueError):
        hip.nn_vote(d, r, 2, 4, t, NROWS, 0, 0, 1.0)
    with pytest.raises(ValueError):
        hip.nn_vote(d, r, 2, 4, t, NROWS, 3, 2, 1.0)
    with pytest.raises(ValueError):
        hip.nn_vote(d, r, 2, 4, t, NROWS, 3, 0, -1.0)
    with pytest.raises(ValueError):
        hip.nn_vote(d, r, 2, 4, t, NROWS, 3, 0, 1.0, out=out[:1])
    assert hip.nn_vote(d, r, 0, 4, t, NROWS, 3, 0, 1.0).shape == (0, 3)


# ------------------------------------------------------------------ driver
def compare_paths(g, qs, tag, lists_of=None):
    """fused classify against the per-datum path of the same GPU driver (or
    of ``lists_of``, a driver that holds the same rows): the same labels in
    the same order, scores within the kernel's bound of the float64 vote over
    the per-datum lists -> the fused answer"""
    from jubatus_amd.fv_converter.datum import as_datum
    fused = g._classify_fused([as_datum(q) for q in qs])
    # classify takes the fused path, but for one datum on an LSH index
    one_lsh = len(qs) == 1 and g._each_for_one
    assert g.classify(qs) == (g._classify_each(qs) if one_lsh else fused)
    g = lists_of or g
    each = g._classify_each(qs)
    assert len(fused) == len(each) == len(qs)
    worst = 0.0
    for q, f, e in zip(qs, fused, each):
        assert [lab for lab, _ in f] == [lab for lab, _ in e] == list(g.labels)
        assert all(isinstance(v, float) for _, v in f)
        st = neighbour_stats(g, g.engine.query_datum(q, g.k, g.similar))
        for (lab, fv), (_, ev) in zip(f, e):
            ref, n, scale = st.get(lab, (0.0, 0, 0.0))
            bound = (n + 8) * EPS * scale
            worst = max(worst, abs(fv - ref) - bound)
            assert abs(fv - ref) <= bound, (tag, lab, fv, ref, n, bound)
            assert abs(ev - ref) <= bound, (tag, lab, ev, ref, n, bound)
            if n == 0:
                assert fv == 0.0
    print(f"{tag}: {len(qs)} queries, largest err - bound {worst:.3g}")
    return fused


@pytest.mark.parametrize("method,inner,k,n,seed", DRIVER_CASES)
def test_gpu_driver_fused_against_per_datum(method, inner, k, n, seed):
    X, labs, Q = make_labelled(n, NQ, seed)
    assert kth_gap_holds(method, inner, X, labs, Q, k)
    g = driver(method, params(method, inner, k, 0.5), device=dev())
    assert g.train(labelled(X[:n // 2], labs[:n // 2])) == n // 2
    assert g.train(labelled(X[n // 2:], labs[n // 2:])) == n - n // 2
    assert g.row_lab.is_cuda and g.get_status()["nn.storage"] == "hbm"
    check_row_lab(g)
    qs = [datum(q) for q in Q]
    fused = compare_paths(g, qs, f"{method}/{inner} k={k}")
    assert any(v != 0 for r in fused for _, v in r)
    assert g.classify([]) == []
    one = compare_paths(g, qs[:1], f"{method}/{inner} k={k}, one datum")
    assert [lab for lab, _ in one[0]] == [lab for lab, _ in fused[0]]


@pytest.mark.parametrize("method,inner", [("NN", "euclid_lsh"), ("cosine", None),
                                          ("euclidean", None)])
def test_gpu_driver_operation_sequence(method, inner):
    """every live row is a neighbour (k = 128 over at most 60 rows), so the
    two paths see the same rows whatever the ties"""
    from jubatus_amd.models.nn_classifier import NNClassifier
    X, labs, Q = make_labelled(90, 6, 96)
    qs = [datum(q) for q in Q]
    p = params(method, inner, 128, 0.5)
    g = driver(method, p, device=dev())
    # an empty table: every known label at 0.0
    assert g.classify(qs) == [[]] * 6
    assert g.set_label("spare") is True
    assert g.classify(qs) == [[("spare", 0.0)]] * 6
    g.train(labelled(X[:40], labs[:40]))
    check_row_lab(g)
    res = compare_paths(g, qs, f"{method} set_label")
    assert all(r[0] == ("spare", 0.0) for r in res)
    # delete_label, then classify: the label is gone, its id stays retired
    victim = labs[0]
    vid = g.label_id[victim]
    assert g.delete_label(victim) is True
    check_row_lab(g)
    res = compare_paths(g, qs, f"{method} delete_label")
    assert all(victim not in dict(r) for r in res)
    g.train([("late", datum(X[40]))])                      # takes a freed slot, a new id
    assert g.label_id["late"] > vid and g.label_id[victim] == vid
    check_row_lab(g)
    compare_paths(g, qs, f"{method} slot reuse after delete_label")
    # put_diff from a second driver, with a row that has no tag and a removed row
    h = driver(method, p, device=dev())
    h.train(labelled(X[41:60], [f"H{lab}" for lab in labs[41:60]]))
    h.engine.set_row("untagged-0", datum(X[60]))
    gone = next(iter(g.engine.rows.slot_of))
    g.engine.clear_row(gone)
    mixed = NNClassifier.mix_diff(g.get_diff(), h.get_diff())
    assert gone in mixed["rows"]["removed"] and mixed["tags"]["untagged-0"] is None
    assert g.put_diff(mixed) is True and h.put_diff(mixed) is True
    for drv, name in ((g, "g"), (h, "h")):
        assert gone not in drv.row_label and "untagged-0" in drv.engine.rows.slot_of
        check_row_lab(drv)
        assert int(drv.row_lab[drv.engine.rows.slot_of["untagged-0"]]) == -1
        compare_paths(drv, qs, f"{method} put_diff {name}")
    # pack -> unpack into a fresh driver answers the same
    f = driver(method, p, device=dev())
    f.unpack(g.pack())
    check_row_lab(f)
    assert f._stray is False
    assert list(f.labels) == list(g.labels) and f.row_label == g.row_label
    compare_paths(f, qs, f"{method} unpack")
    compare_paths(f, qs, f"{method} unpack, against the packed driver's lists", lists_of=g)
    # clear
    g.clear()
    check_row_lab(g)
    assert g.next_id == 0 and int(g.row_lab.max()) == -1 and g.classify(qs) == [[]] * 6


def test_gpu_driver_eviction_and_slot_reuse():
    g = driver("NN", params("NN", "euclid_lsh", 16, unlearner="lru",
                            unlearner_parameter={"max_size": 4}), device=dev())
    X, _, Q = make_data(8, 5, 71)
    qs = [datum(q) for q in Q]
    g.train([("old", datum(x)) for x in X[:4]])
    # fewer rows than k: the device lists hold the four rows, then padding
    from jubatus_amd.fv_converter.datum import as_datum
    dist, row = g.engine.index.query_device(g.engine.fvs_of([as_datum(q) for q in qs]), 4, 16)
    dist, row = dist.cpu().numpy(), row.cpu().numpy()
    assert dist.shape == (5, 16) and np.all(np.isfinite(dist[:, :4]))
    assert np.all(np.sort(row[:, :4], axis=1) == np.arange(4))
    assert np.all(np.isposinf(dist[:, 4:])) and np.all(row[:, 4:] == INT_MAX)
    res = compare_paths(g, qs, "before eviction")
    assert all(dict(r)["old"] > 0 for r in res)
    g.train([("new", datum(x)) for x in X[4:]])             # evicts the four old rows
    assert len(g.row_label) == 4 and g.engine.rows.nslots < 8
    check_row_lab(g)
    res = compare_paths(g, qs, "after eviction")
    assert all(dict(r)["old"] == 0.0 and dict(r)["new"] > 0 for r in res)


def test_row_lab_grows_past_1024_slots():
    method, inner, k, n, seed = GROWTH_CASE
    X, labs, Q = make_labelled(n, 6, seed)
    assert kth_gap_holds(method, inner, X, labs, Q[:6], k)
    g = driver(method, params(method, inner, k), device=dev())
    g.train(labelled(X[:1000], labs[:1000]))
    assert g.row_lab.numel() == 1024
    g.train(labelled(X[1000:], labs[1000:]))
    assert g.row_lab.numel() >= n
    check_row_lab(g)
    compare_paths(g, [datum(q) for q in Q], "1300 rows")


def test_a_label_missing_from_labels_takes_the_per_datum_path():
    X, labs, Q = make_labelled(30, 3, 97)
    g = driver("euclidean", params("euclidean", None, 64), device=dev())
    g.train(labelled(X, labs))
    obj = g.pack()
    obj = {**obj, "labels": {k: v for k, v in obj["labels"].items() if k != labs[0]}}
    h = driver("euclidean", params("euclidean", None, 64), device=dev())
    h.unpack(obj)
    assert h._stray is True
    check_row_lab(h)
    qs = [datum(q) for q in Q]
    res = h.classify(qs)
    assert res == h._classify_each(qs)
    assert all([lab for lab, _ in r] == list(h.labels) + [labs[0]] for r in res)


# ------------------------------------------------------------------ server
@pytest.fixture
def gpu_server(tmp_path):
    from jubatus_amd.framework.server_helper import ServerHelper
    from jubatus_amd.framework.server_util import ServerArgv
    from jubatus_amd.server import get_serv
    a = ServerArgv.parse(["-p", "9199", "-b", "127.0.0.1", "-f", NN_CFG, "-d", str(tmp_path),
                          "-c", "4", "--gpu", "0"], "classifier")
    a.port = 0
    h = ServerHelper(get_serv("classifier"), a, install_signals=False)
    h.start(block=False)
    yield h
    h.stop()


def test_python_gpu_server_against_the_cpu_driver(gpu_server):
    from jubatus_amd.client import Classifier, Datum
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.models.nn_classifier import NNClassifier
    cfg = json.load(open(NN_CFG))
    cpu = NNClassifier(cfg["method"], cfg["parameter"], DatumToFvConverter(cfg["converter"]))
    X, labs, Q = make_labelled(64, 8, 98)                   # k = 128 >= 64 rows: no ties to break

    def same(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert [r.label for r in g] == [lab for lab, _ in w]
            for r, (lab, v) in zip(g, w):
                assert abs(r.score - v) <= 1e-4 * max(1.0, abs(v)), (lab, r.score, v)

    with Classifier("127.0.0.1", gpu_server.argv.port, "", timeout=60) as c:
        for lo in (0, 32):
            batch = labelled(X[lo:lo + 32], labs[lo:lo + 32])
            assert c.train([[lab, Datum(d)] for lab, d in batch]) == 32
            assert cpu.train(batch) == 32
        assert c.set_label("spare") is True and cpu.set_label("spare") is True
        qs = [datum(q) for q in Q]
        got = c.classify([Datum(q) for q in qs])
        same(got, cpu.classify(qs))
        assert any(r.score > 0 for g in got for r in g)
        assert all(dict((r.label, r.score) for r in g)["spare"] == 0.0 for g in got)
        assert c.get_labels() == cpu.get_labels()
        st = list(c.get_status().values())[0]
        assert st["method"] == "NN" and st["nn.storage"] == "hbm" and st["nn.num_rows"] == "64"
        assert c.delete_label(labs[0]) is True and cpu.delete_label(labs[0]) is True
        same(c.classify([Datum(q) for q in qs]), cpu.classify(qs))
        assert c.classify([]) == []
        assert c.clear() is True
        assert c.classify([Datum(qs[0])]) == [[]]
