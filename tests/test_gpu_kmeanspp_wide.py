"""csrc/hip/kmeanspp_wide.hip (k-means++ seeding on the whole GPU) against a
float64 reference of the same draw rule, teacher-forced: every draw is checked
under the kernel's own earlier picks (one fp32 rounding near a boundary would
fork an exact trajectory), and the clustering driver's use of the chain."""
import functools
import random

import numpy as np
import pytest

from jubatus_amd.fv_converter.converter import DatumToFvConverter

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 1, 2), (300, 5, 17), (2500, 64, 128),
          (600, 1030, 16),                       # 33 chunks, the last 6 columns wide
          (17000, 3, 40), (70000, 2, 8),         # 128 and 320 rows a workgroup: one and two tiles
          (16384, 3, 12), (16385, 3, 12)]        # 256 workgroups x 64 rows exactly, and one row more
U = {"random": None, "first": 0.0, "last": 1.0 - 2.0 ** -53}
EPS = 2.0 ** -24


def dev():
    import torch
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def inputs(n, d, m):
    import torch
    g = torch.Generator().manual_seed(n + d + m)
    k = min(8, n)
    X = (torch.randn(k, d, generator=g) * 6.0)[torch.arange(n) % k] + torch.randn(n, d, generator=g)
    w = torch.rand(n, generator=g) + 0.5
    w[::7] = 0.0                                 # row 0 carries no mass
    return X, w, torch.rand(m, generator=g, dtype=torch.float64).tolist()


def run(X, w, u, m):
    from jubatus_amd.ops import hip
    rows, status, nearest, d2 = hip.kmeanspp_wide(X.to(dev()), w.to(dev()), u, m)
    return rows, status, nearest.cpu().numpy(), d2.cpu().numpy()


def check(X, w, u, m, rows, status, nearest, d2):
    """every draw against the float64 rule under the kernel's earlier picks, then d2 and nearest"""
    X, w = X.double().numpy(), w.double().numpy()
    n, d = X.shape
    D, mind, off = [], np.full(n, np.inf), 0
    for j in range(m):
        if j:
            D.append(((X - X[rows[j - 1]]) ** 2).sum(1))
            mind = np.minimum(mind, D[-1])
        p = mind * w if j else w
        cum = np.cumsum(p)
        total = cum[-1]
        if status == j + 1:                      # the zero-mass stop
            assert total <= 0.0 and rows[j] == -1
            break
        target, r, tol = u[j] * total, rows[j], 4 * (d + 3) * EPS * total
        assert total > 0.0 and 0 <= r < n
        assert (cum[r - 1] if r else 0.0) - tol <= target <= cum[r] + tol, (j, r)
        assert p[r] > 0.0 or r == n - 1, (j, r)
        off += r != min(int(np.searchsorted(cum, target, side="right")), n - 1)
    else:
        assert status == 0
        D.append(((X - X[rows[m - 1]]) ** 2).sum(1))
        mind = np.minimum(mind, D[-1])
    print(f"{off} of {m} picks off the exact bisect, status {status}")
    if D:
        D = np.stack(D, 1)
        assert np.all(np.abs(d2 - mind) <= 2 * (d + 2) * EPS * mind)
        assert nearest.min() >= 0 and nearest.max() < D.shape[1]
        assert np.all(D[np.arange(n), nearest] <= (1 + 4 * (d + 2) * EPS) * mind)


@pytest.mark.parametrize("regime", list(U))
@pytest.mark.parametrize("n,d,m", SHAPES)
def test_draws_follow_the_float64_rule(n, d, m, regime):
    X, w, u = inputs(n, d, m)
    u = u if U[regime] is None else [U[regime]] * m
    check(X, w, u, m, *run(X, w, u, m))


def test_two_runs_give_the_same_bits():
    X, w, u = inputs(2500, 64, 128)
    a, b = run(X, w, u, 128), run(X, w, u, 128)
    assert a[0] == b[0] and a[1] == b[1] == 0
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3].view(np.int32), b[3].view(np.int32))


def raw(X, w, u, m, out, status, nearest, work, nbytes=None):
    """jb_kmeanspp_wide on the caller's buffers -> rc"""
    from jubatus_amd.ops import hip
    return hip._fn("jb_kmeanspp_wide")(hip._p(X), X.shape[0], X.shape[1], hip._p(w), hip._p(u), m, hip._p(out),
                                       hip._p(status), hip._p(nearest), hip._p(work),
                                       work.numel() if nbytes is None else nbytes, hip._stream())


def test_zero_mass_stops_the_chain():
    """5 distinct rows: draw 5 finds no mass; the launches behind it write nothing"""
    import torch
    from jubatus_amd.ops import hip
    n, m = 600, 8
    X = torch.randn(5, 3, generator=torch.Generator().manual_seed(1))[torch.arange(n) % 5].contiguous().to(dev())
    w = inputs(n, 3, m)[1].to(dev())
    u = torch.tensor(inputs(n, 3, m)[2], dtype=torch.float64, device=dev())
    out = torch.full((m + 1,), -7, dtype=torch.int32, device=dev())
    status = torch.full((2,), -7, dtype=torch.int32, device=dev())
    nearest = torch.full((n + 1,), -7, dtype=torch.int32, device=dev())
    work = torch.empty(hip._fn("jb_kmeanspp_wide_work")(n, 3, m), dtype=torch.uint8, device=dev())
    assert raw(X, w, u, m, out, status, nearest, work) == 0
    out, nearest = out.tolist(), nearest.tolist()
    assert status.tolist() == [6, -7] and out[5:] == [-1, -7, -7, -7] and nearest[n] == -7
    assert sorted(r % 5 for r in out[:5]) == [0, 1, 2, 3, 4]
    assert [out[a] % 5 for a in nearest[:n]] == [i % 5 for i in range(n)]
    assert not work[work.numel() - 4 * n:].view(torch.float32).any()      # d2: every row on a chosen row


def test_range_and_shape_checks():
    import torch
    from jubatus_amd.ops import hip
    X, w, u = (t.to(dev()) if hasattr(t, "to") else t for t in inputs(300, 5, 17))
    assert hip.kmeanspp_wide(X, w, u * 20, 301) is None
    assert hip._fn("jb_kmeanspp_wide_work")(300, 5, 301) == 0
    with pytest.raises(ValueError):
        hip.kmeanspp_wide(X, w[:299], u, 17)
    ud = torch.tensor(u, dtype=torch.float64, device=dev())
    out = torch.full((18,), -7, dtype=torch.int32, device=dev())
    work = torch.empty(hip._fn("jb_kmeanspp_wide_work")(300, 5, 17), dtype=torch.uint8, device=dev())
    assert raw(X, w, ud, 301, out, out[17:], None, work) != 0
    assert raw(X, w, ud, 17, out, out[17:], None, work, work.numel() - 1) != 0
    assert out.tolist() == [-7] * 18                                      # nothing was launched
    assert not hip.kmeanspp_wide_pays(1000, 10, 100)                      # the four-wave kernel takes it
    assert not hip.kmeanspp_wide_pays(300, 5, 301)


def test_clustering_driver_seeds_and_compresses_with_the_chain(monkeypatch):
    """compressive_kmeans with the chain forced: the device engine seeds with
    it, takes its nearest table in _compress (no n x m sqdist there) and agrees
    with the host engine"""
    import torch
    from jubatus_amd.models.clustering import Clustering
    monkeypatch.setenv("JB_KMEANSPP_WIDE", "1")
    p = {"k": 8, "compressor_method": "compressive_kmeans", "bucket_size": 2100, "compressed_bucket_size": 64,
         "seed": 0}
    conv = {"num_rules": [{"key": "*", "type": "num"}]}
    r = random.Random(3)
    truth = [[r.gauss(0, 6) for _ in range(24)] for _ in range(8)]
    pts = [{f"f{q:04d}": c + r.gauss(0, 1) for q, c in enumerate(truth[i % 8])} for i in range(2100)]
    g = Clustering("kmeans", p, DatumToFvConverter(conv), dev())
    h = Clustering("kmeans", p, DatumToFvConverter(conv))
    seen = {"compressing": False, "sqdist": 0}
    compress, sqdist = g._compress, g._sqdist

    def counted_compress(ps, m):
        seen["compressing"] = True
        try:
            return compress(ps, m)
        finally:
            seen["compressing"] = False

    def counted_sqdist(X, C):
        seen["sqdist"] += seen["compressing"]
        return sqdist(X, C)

    monkeypatch.setattr(g, "_compress", counted_compress)
    monkeypatch.setattr(g, "_sqdist", counted_sqdist)
    for e in (g, h):
        e.push(pts)
    assert g._kpp_wide_runs > 0 and g._lloyd_iters is not None and seen["sqdist"] == 0
    assert g.get_revision() == h.get_revision() == 1
    torch.testing.assert_close(g.centers.cpu(), h.centers, rtol=1e-3, atol=1e-3)
