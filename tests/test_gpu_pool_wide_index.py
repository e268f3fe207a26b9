"""The pass planner of InvertedIndex (models/similarity.py _wide_passes) behind query_device /
query and the nearest-neighbour drivers, JUBATUS_POOL_WIDE=1, against the host InvertedIndex.
A device list is held to rtol 1e-6 twice: every returned row against that row's oracle
distance, and the ascending list against the oracle's k smallest - a swap at a near-tie
passes, a wrong row does not. (Random 8-of-64 rows: no distance near 0.)"""
import functools
import json
import os

import numpy as np
import pytest

from helpers import ROOT
from test_gpu_pool_wide import dev
from test_nn_regression import datum, make_data, scored
from test_nn_vote import labelled, make_labelled

pytestmark = pytest.mark.gpu

NROWS, RTOL = 700, 1e-6


def sparse_rows(n, nfeat, width, seed):
    rng = np.random.default_rng(seed)
    return [(np.sort(rng.choice(nfeat, width, replace=False)), rng.normal(size=width).astype(np.float32))
            for _ in range(n)]


def index(euclid, rows, device, removed=()):
    from jubatus_amd.models.similarity import InvertedIndex
    ix = InvertedIndex(euclid, device)
    ix.set_rows(list(range(len(rows))), rows)
    for s in removed:
        ix.remove(s)
    return ix


@pytest.fixture
def wide(monkeypatch):
    """JUBATUS_POOL_WIDE=1 -> the query counts of the wide passes taken"""
    from jubatus_amd.ops import hip
    taken, scan_wide = [], hip.pool_scan_wide
    monkeypatch.setattr(hip, "pool_scan_wide", lambda *a: (taken.append(a[4]), scan_wide(*a))[1])
    monkeypatch.setenv("JUBATUS_POOL_WIDE", "1")
    return taken


@functools.lru_cache(maxsize=None)
def case(euclid, nq):
    """-> (device index, queries, oracle distances [nq, NROWS])"""
    rows, queries = sparse_rows(NROWS, 64, 8, 1), sparse_rows(nq, 64, 8, 2 + nq)
    c = index(euclid, rows, None, (3, 77, 699))
    s = np.stack([c.scores(q, NROWS).astype(np.float64) for q in queries])
    ref = s if euclid else np.where(np.isfinite(s), 1.0 - s, np.inf)
    return index(euclid, rows, dev(), (3, 77, 699)), queries, ref


@pytest.mark.parametrize("euclid", [False, True])
@pytest.mark.parametrize("nq,k", [(40, 5), (40, 200), (200, 5), (200, 200)])
def test_query_device_and_query_against_the_host_index(nq, k, euclid, wide):
    g, queries, ref = case(euclid, nq)
    dist, row = (t.cpu().numpy() for t in g.query_device(queries, NROWS, k))
    lists = g.query(queries, NROWS, k, False)
    assert dist.shape == row.shape == (nq, k) and [len(r) for r in lists] == nq * [k]
    assert wide == 2 * ([40] if nq == 40 else [64, 64, 64])          # the last 8 of 200: pool_scan
    for d, r in ((dist, row), (np.asarray([[x for _, x in r] for r in lists]),
                               np.asarray([[s for s, _ in r] for r in lists]))):
        for q in range(nq):                                   # in query order: ref[q] is query q's
            assert len(set(r[q].tolist())) == k and np.all(np.diff(d[q]) >= 0)
            for want in (ref[q, r[q]], np.sort(ref[q])[:k]):
                assert np.all(np.abs(d[q] - want) <= RTOL * np.abs(want)), q


@pytest.mark.parametrize("width,wide_queries", [(100, 192), (300, 0)])
def test_mixed_batch_splits_into_narrower_passes(width, wide_queries, wide, monkeypatch):
    """100 features a query: 12 passes of 16 queries; the 8 around the oversize query and the
    last one take pool_scan. Nine queries of 300 features fit no wide pass: all pool_scan."""
    from jubatus_amd.ops import hip
    rng = np.random.default_rng(width)
    assert hip.pool_wide_qm(1, 2000) == 0
    queries = [(np.arange(q * width, (q + 1) * width), rng.normal(size=width).astype(np.float32))
               for q in range(200)]
    queries.insert(100, (np.arange(200 * width, 200 * width + 2000), rng.normal(size=2000).astype(np.float32)))
    g = index(True, sparse_rows(500, 200 * width + 2000, 40, 3), dev())
    d1 = g.query_device(queries, 500, 7)[0].cpu().numpy()
    assert wide == (wide_queries // 16) * [16]
    monkeypatch.setenv("JUBATUS_POOL_WIDE", "0")
    d0 = g.query_device(queries, 500, 7)[0].cpu().numpy()
    assert len(wide) == wide_queries // 16 and d1.shape == d0.shape == (201, 7)
    assert np.all(np.abs(d1 - d0) <= RTOL * d0)


@pytest.mark.parametrize("kind,name", [("classifier", "cosine.json"), ("classifier", "euclidean.json"),
                                       ("regression", "cosine.json")])
def test_drivers_reach_the_wide_scan(kind, name, wide):
    """40 datums against the CPU driver, with the tolerances of test_gpu_nn_vote.py (1e-4
    max(1, |v|)) and test_gpu_nn_regression.py (2e-4 max|t|). Seeds 84 / 63: every query has the
    k-th neighbour gap that test_nn_vote.kth_gap_holds / test_nn_regression.oracle ask for."""
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.models.nn_classifier import NNClassifier
    from jubatus_amd.models.nn_regression import NNRegression
    cfg = json.load(open(os.path.join(ROOT, "config", kind, name)))
    p, cls = cfg["parameter"], NNClassifier if kind == "classifier" else NNRegression
    X, y, Q = make_labelled(300, 40, 84) if kind == "classifier" else make_data(300, 40, 63)
    data = labelled(X, y) if kind == "classifier" else scored(X, y)
    g, c = (cls(cfg["method"], p, DatumToFvConverter(cfg["converter"]), device=d) for d in (dev(), None))
    assert g.train(data) == c.train(data) == 300
    qs = [datum(q) for q in Q]
    got, want = (d.estimate(qs) if kind == "regression" else d.classify(qs) for d in (g, c))
    assert wide == [40]
    if kind == "regression":
        assert np.abs(np.asarray(got) - np.asarray(want)).max() <= 2e-4 * np.abs(y).max()
        return
    for a, b in zip(got, want):
        assert [lab for lab, _ in a] == [lab for lab, _ in b]
        assert all(abs(x - v) <= 1e-4 * max(1.0, abs(v)) for (_, x), (_, v) in zip(a, b))
