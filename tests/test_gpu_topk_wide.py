"""Neighbour lists of 129 to 4096 entries (csrc/hip/topk_wide.hip: histogram
select, tie pass, collect, sort) against NumPy: fp32 popcount / hash_num and
1 - score are exactly reproducible, so rows must match np.lexsort on
(distance, row); euclid_lsh goes through __cosf and is held to fp64
law-of-cosines distances at the bar test_gpu_engines.py uses (1e-4). "Range"
below is one block's row range, 2048."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1
BIG = 70_000          # dozens of blocks a query


def dev():
    import torch
    return torch.device("cuda", 0)


def table(n, hash_num, seed, nq=3):
    """random signatures with the bits past hash_num clear, norms, and nq
    queries near stored rows -> uint64 [n, w], float32 [n], uint64 [nq, w], float32 [nq]"""
    rng = np.random.default_rng(seed)
    w = (hash_num + 63) // 64
    tb = rng.integers(0, 2**64, (n, w), dtype=np.uint64)
    if hash_num % 64:
        tb[:, -1] &= np.uint64((1 << (hash_num % 64)) - 1)
    qb = tb[rng.integers(0, n, nq)] ^ (tb[rng.integers(0, n, nq)] & tb[rng.integers(0, n, nq)])
    return tb, rng.random(n, dtype=np.float32) + 0.5, qb, rng.random(nq, dtype=np.float32) + 0.5


def hamming(qb, tb):
    x = (qb[:, None, :] ^ tb[None, :, :]).view(np.uint8)
    return np.unpackbits(x, axis=-1).sum(-1)


def expect(d32, k):
    """[nq, k] (distance, row) by lexsort; NaN / +inf never returned, padding after"""
    nq, n = d32.shape
    od, oi = np.full((nq, k), np.inf, np.float32), np.full((nq, k), INT_MAX, np.int32)
    for q in range(nq):
        o = np.lexsort((np.arange(n), d32[q]))
        o = o[d32[q][o] < np.inf][:k]
        od[q, :o.size], oi[q, :o.size] = d32[q][o], o
    return od, oi


def run_hamming(tb, tn, qb, qn, valid, hash_num, metric, k):
    import torch
    from jubatus_amd.ops import hip
    t = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev())  # noqa: E731
    d, i = hip.topk_hamming(t(qb), t(qn), len(qb), t(tb), t(tn), t(valid), len(tb), hash_num, metric, k)
    return d.cpu().numpy(), i.cpu().numpy()


def run_scores(sc, k, flip):
    import torch
    from jubatus_amd.ops import hip
    d, i = hip.topk_scores(torch.from_numpy(sc).to(dev()), sc.shape[0], sc.shape[1], k, flip)
    return d.cpu().numpy(), i.cpu().numpy()


def check_exact(got, d32, k):
    wd, wi = expect(d32, k)
    np.testing.assert_array_equal(got[1], wi)
    np.testing.assert_allclose(got[0], wd, rtol=0, atol=1e-6)


# k at the boundaries x nrows in {k - 1, k, 3 ranges + 1, BIG}; nq, hash_num
# (one word, a partial word, eight words) and lsh / minhash rotate over them
SHAPES = [(k, nr, (1, 3)[j % 2], (64, 100, 512)[(i + j) % 3], (0, 2)[(i + j) % 2])
          for i, k in enumerate((129, 130, 1000, 4096))
          for j, nr in enumerate((k - 1, k, 3 * 2048 + 1, BIG))]


@pytest.mark.parametrize("k,nrows,nq,hash_num,metric", SHAPES)
def test_hamming_matches_lexsort(k, nrows, nq, hash_num, metric):
    tb, tn, qb, qn = table(nrows, hash_num, seed=k + nrows, nq=nq)
    valid = np.ones(nrows, np.uint8)
    valid[::37] = 0
    d32 = hamming(qb, tb).astype(np.float32) / np.float32(hash_num)
    d32[:, valid == 0] = np.inf
    check_exact(run_hamming(tb, tn, qb, qn, valid, hash_num, metric, k), d32, k)


@pytest.mark.parametrize("case", ["all_tied", "hash16", "mostly_invalid"])
def test_hamming_ties_and_padding(case):
    if case == "all_tied":          # every row the same signature: rows 0..199
        tb, tn, qb, qn = table(3 * 2048 + 1, 64, seed=1, nq=1)
        tb[:] = tb[0]
        valid, k, hash_num = np.ones(len(tb), np.uint8), 200, 64
    elif case == "hash16":          # 17 distinct distances: the tie run crosses block ranges
        tb, tn, qb, qn = table(BIG, 16, seed=2)
        valid, k, hash_num = np.ones(len(tb), np.uint8), 1000, 16
    else:                           # 150 valid rows, k = 200: 150 entries, then padding
        tb, tn, qb, qn = table(3 * 2048 + 1, 64, seed=3)
        valid, k, hash_num = np.zeros(len(tb), np.uint8), 200, 64
        valid[np.random.default_rng(4).choice(len(tb), 150, replace=False)] = 1
    d32 = hamming(qb, tb).astype(np.float32) / np.float32(hash_num)
    d32[:, valid == 0] = np.inf
    got = run_hamming(tb, tn, qb, qn, valid, hash_num, 0, k)
    check_exact(got, d32, k)
    if case == "all_tied":
        np.testing.assert_array_equal(got[1][0], np.arange(200))
    if case == "mostly_invalid":
        assert np.all(got[1][:, 150:] == INT_MAX) and np.all(np.isinf(got[0][:, 150:]))


@pytest.mark.parametrize("case,flip", [("special", True), ("special", False), ("quantised", True),
                                       ("quantised", False), ("short", True)])
def test_scores_match_lexsort(case, flip):
    rng = np.random.default_rng(5)
    if case == "special":           # NaN, -inf, an exact 1.0 (distance +0), 1 + 2^-23 (negative under flip), -0
        sc = rng.random((3, 3 * 2048 + 1), dtype=np.float32)
        sc[:, 5::11] = np.nan
        sc[:, 7::13] = -np.inf
        sc[:, 100::501] = 1.0
        sc[:, 3000::701] = np.float32(1.0) + np.float32(2.0**-23)
        sc[:, 9::1001] = -0.0
        k = 200
    elif case == "quantised":       # 60 levels: heavy ties in float keys, across block ranges
        sc = (rng.integers(0, 60, (3, BIG)) / np.float32(60)).astype(np.float32)
        k = 1000
    else:                           # nrows = k - 1
        sc = rng.random((1, 4095), dtype=np.float32)
        k = 4096
    with np.errstate(invalid="ignore"):
        d32 = (np.float32(1.0) - sc) if flip else sc.copy()
    d32[np.isnan(d32)] = np.inf
    check_exact(run_scores(sc, k, flip), d32, k)


def test_shared_scratch_and_repeat():
    """two calls on different inputs back to back (the chain zeroes its own
    histograms and counters), then the first again: the same bits"""
    a = table(BIG, 64, seed=6)
    b = table(3 * 2048 + 1, 64, seed=7)
    va, vb = np.ones(BIG, np.uint8), np.ones(3 * 2048 + 1, np.uint8)
    ga = run_hamming(a[0], a[1], a[2], a[3], va, 64, 1, 1000)
    gb = run_hamming(b[0], b[1], b[2], b[3], vb, 64, 0, 1000)
    ga2 = run_hamming(a[0], a[1], a[2], a[3], va, 64, 1, 1000)
    check_exact(gb, hamming(b[2], b[0]).astype(np.float32) / np.float32(64), 1000)
    assert ga[0].tobytes() == ga2[0].tobytes() and ga[1].tobytes() == ga2[1].tobytes()


@pytest.mark.parametrize("nrows,k,hash_num", [(BIG, 160, 64), (3 * 2048 + 1, 1000, 100), (4096, 4096, 512)])
def test_euclid_lsh(nrows, k, hash_num):
    tb, tn, qb, qn = table(nrows, hash_num, seed=8)
    valid = np.ones(nrows, np.uint8)
    valid[::41] = 0
    a, b = qn.astype(np.float64)[:, None], tn.astype(np.float64)[None, :]
    ref = np.sqrt(np.maximum(0.0, a * a + b * b - 2 * a * b * np.cos(np.pi * hamming(qb, tb) / hash_num)))
    ref[:, valid == 0] = np.inf
    d, i = run_hamming(tb, tn, qb, qn, valid, hash_num, 1, k)
    want = np.sort(ref, axis=1)[:, :k]
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        assert np.all(np.diff(d, axis=1)[fin[:, 1:]] >= 0)
    assert np.all(np.isinf(d[~fin])) and np.all(i[~fin] == INT_MAX)
    np.testing.assert_allclose(d[fin], want[fin], rtol=1e-4, atol=1e-4)
    for q in range(len(qb)):
        rows = i[q][fin[q]]
        assert len(set(rows.tolist())) == rows.size
        kth = want[q][fin[q]][-1]
        assert np.all(ref[q][rows] <= kth + 1e-4 + 1e-4 * kth)
    if k == 160:                    # the k <= 128 path's bits
        d128, i128 = run_hamming(tb, tn, qb, qn, valid, hash_num, 1, 128)
        assert d[:, :128].tobytes() == d128.tobytes() and i[:, :128].tobytes() == i128.tobytes()


def _rows(n, seed):
    r = random.Random(seed)
    return [(r.sample(range(1 << 12), 12), [r.gauss(0, 1) for _ in range(12)]) for _ in range(n)]


@pytest.mark.parametrize("kind", ["lsh", "inverted_index", "inverted_index_euclid"])
def test_drivers_at_k200(kind):
    """query and query_device of the GPU index at k = 200 against the CPU index of the same rows"""
    from jubatus_amd.models.similarity import InvertedIndex, LshIndex
    n, k = 700, 200
    rs, q = _rows(n, 9), _rows(2, 10)
    if kind == "lsh":
        g, c = LshIndex("lsh", 64, 7, dev()), LshIndex("lsh", 64, 7, None)
    else:
        g, c = (InvertedIndex(kind.endswith("euclid"), d) for d in (dev(), None))
    for ix in (g, c):
        ix.set_rows(list(range(n)), rs)
        ix.remove(11)
    if kind == "lsh":               # identical signatures on both sides, as test_gpu_engines.py
        c.bits[:n] = g.bits[:n].cpu().numpy().view(np.uint64)
    for one in q:                   # single queries: what the drivers send to the wide kernel
        (w,), (a,) = c.query([one], n, k, similar=False), g.query([one], n, k, similar=False)
        dd, di = g.query_device([one], n, k)
        assert tuple(dd.shape) == (1, k) and tuple(di.shape) == (1, k)
        assert len(w) == len(a) == k and 11 not in [r for r, _ in a]
        np.testing.assert_allclose([s for _, s in a], [s for _, s in w], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(dd.cpu().numpy()[0], [s for _, s in w], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("cfg", ["recommender/lsh.json", "recommender/inverted_index.json"])
def test_native_recommender_similar_row_200(cfg, tmp_path):
    """similar_row_from_id(id, 200) of the native jubarecommender against the Python server"""
    from helpers import config_path
    from test_native_row_servers import Pair, _datum, _norm, _same_ranked
    pair = Pair("recommender", open(config_path(cfg)).read(), tmp_path)
    try:
        rng = random.Random(12)
        for j in range(260):
            d = _datum(rng, False)
            for c in (pair.n, pair.p):
                c.call("update_row", "", f"r{j}", d)
        for rid in ("r0", "r131"):
            a, b = (_norm(c.call("similar_row_from_id", "", rid, 200)) for c in (pair.n, pair.p))
            assert len(a) > 128
            _same_ranked(a, b, rid)
    finally:
        pair.close()
