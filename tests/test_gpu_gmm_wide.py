"""csrc/hip/gmm_wide.hip (GMM EM on the whole GPU, for k x dims past one
workgroup's LDS) against a float64 EM of the same formulas, and the
clustering driver's use of it."""
import math
import random

import pytest

from jubatus_amd.fv_converter.converter import DatumToFvConverter

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (65, 1, 3), (300, 17, 5), (777, 33, 130), (1100, 40, 103), (2500, 64, 128),
          (600, 260, 16),
          (2100, 1024, 8)]   # the largest k: slabs of 16 points, LDS past 64 KiB
REGIMES = {"separated": (6.0, 20), "overlapping": (0.5, 3)}


def dev():
    import torch
    return torch.device("cuda", 0)


def inputs(n, k, d, spread):
    import torch
    g = torch.Generator().manual_seed(n + k + d)
    centers = torch.randn(k, d, generator=g) * spread
    X = centers[torch.arange(n) % k] + torch.randn(n, d, generator=g)
    w = torch.rand(n, generator=g) + 0.5
    w[::7] = 0.0
    return X, w, X[:k].clone()


def em64(X, w, C, iters):
    """the EM of models/clustering.py _em in double -> C, var, pi, assign"""
    import torch
    X, w, C = X.double(), w.double(), C.double()
    var = torch.ones_like(C)
    pi = torch.full((C.shape[0],), 1.0 / C.shape[0], dtype=torch.float64)

    def logp():
        q2 = torch.stack([((X - c) ** 2 / v).sum(1) for c, v in zip(C, var)], 1)
        return torch.log(pi.clamp_min(1e-12))[None] - 0.5 * torch.log(2 * math.pi * var).sum(1)[None] - 0.5 * q2
    for _ in range(iters):
        r = torch.softmax(logp(), 1) * w[:, None]
        nk = r.sum(0).clamp_min(1e-9)
        C = (r.T @ X) / nk[:, None]
        var = ((r.T @ (X * X)) / nk[:, None] - C * C).clamp_min(1e-6)
        pi = nk / nk.sum()
    return C, var, pi, logp().argmax(1)


def run_wide(X, w, C0, iters):
    import torch
    from jubatus_amd.ops import hip
    k, d = C0.shape
    C, var = C0.clone().to(dev()), torch.ones(k, d, device=dev())
    pi = torch.full((k,), 1.0 / k, device=dev())
    assign = torch.full((X.shape[0],), -1, dtype=torch.int32, device=dev())
    assert hip.gmm_em_wide(X.to(dev()), w.to(dev()), C, var, pi, iters, assign)
    return C.cpu(), var.cpu(), pi.cpu(), assign.cpu()


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("n,k,d", SHAPES)
def test_gmm_em_wide_matches_float64_em(n, k, d, regime):
    import torch
    spread, iters = REGIMES[regime]
    X, w, C0 = inputs(n, k, d, spread)
    rC, rvar, rpi, rassign = em64(X, w, C0, iters)
    C, var, pi, assign = run_wide(X, w, C0, iters)
    print(f"max |dC| {(C - rC).abs().max():.3g} |dvar| {(var - rvar).abs().max():.3g} "
          f"|dpi| {(pi - rpi).abs().max():.3g} assign differs at {int((assign != rassign).sum())} of {n}")
    torch.testing.assert_close(C, rC.float(), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(var, rvar.float(), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(pi, rpi.float(), rtol=1e-3, atol=1e-4)
    assert int((assign != rassign).sum()) <= 0.01 * n


def test_gmm_em_wide_is_bit_identical_across_launches():
    import torch
    X, w, C0 = inputs(1100, 40, 103, 0.5)
    a, b = run_wide(X, w, C0, 3), run_wide(X, w, C0, 3)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_gmm_em_wide_range_and_shape_checks():
    import torch
    from jubatus_amd.ops import hip

    def call(n, k, d, kc=None, dc=None):
        z = lambda *s: torch.ones(*s, device=dev())   # noqa: E731
        return hip.gmm_em_wide(z(n, d), z(n), z(kc or k, dc or d), z(k, d), z(k), 1)
    assert call(4, 1025, 2) is False
    assert call(2, 1024, 4097) is False
    with pytest.raises(ValueError):
        call(10, 3, 5, dc=4)
    with pytest.raises(ValueError):
        call(10, 3, 5, kc=4)


def test_clustering_driver_takes_the_wide_em_past_the_workgroup_limit():
    """k 8 over 600 numeric keys (k x dims 4800, past gmm_em_kernel's LDS):
    the device engine runs gmm_wide.hip, not the torch loop (_em_assign is
    set), and agrees with the host engine, which draws the same seeds"""
    import torch
    from jubatus_amd.models.clustering import Clustering
    p = {"k": 8, "compressor_method": "simple", "bucket_size": 64, "compressed_bucket_size": 32, "seed": 0}
    conv = {"num_rules": [{"key": "*", "type": "num"}]}
    r = random.Random(3)
    truth = [[r.gauss(0, 6) for _ in range(600)] for _ in range(8)]
    pts = [{f"f{q:03d}": c + r.gauss(0, 1) for q, c in enumerate(truth[i % 8])} for i in range(128)]
    g = Clustering("gmm", p, DatumToFvConverter(conv), dev())
    h = Clustering("gmm", p, DatumToFvConverter(conv))
    for e in (g, h):
        e.push(pts[:64])
        e.push(pts[64:])
    assert g.centers.is_cuda and g.centers.shape == (8, 600) and g.get_revision() == h.get_revision() == 2
    assert g._em_assign is not None
    torch.testing.assert_close(g.centers.cpu(), h.centers, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(g.variances.cpu(), h.variances, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(g.mix_weights.cpu(), h.mix_weights, rtol=1e-3, atol=1e-4)
