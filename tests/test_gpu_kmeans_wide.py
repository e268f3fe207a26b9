"""csrc/hip/kmeans_wide.hip (weighted Lloyd on the whole GPU, for k x dims
past one workgroup's LDS) against a float64 Lloyd of the same rule, and the
clustering driver's use of it."""
import functools
import random

import pytest

from jubatus_amd.fv_converter.converter import DatumToFvConverter

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (65, 3, 1), (300, 5, 17), (777, 130, 33), (600, 16, 260), (2500, 128, 64),
          (2100, 1024, 8),    # the largest k: slabs of 16 points, LDS past 64 KiB
          (17000, 5, 3)]      # 266 slabs on 256 workgroups
REGIMES = {"separated": 6.0, "overlapping": 0.5}


def dev():
    import torch
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def inputs(n, k, d, spread):
    import torch
    g = torch.Generator().manual_seed(n + k + d)
    centers = torch.randn(k, d, generator=g) * spread
    X = centers[torch.arange(n) % k] + torch.randn(n, d, generator=g)
    w = torch.rand(n, generator=g) + 0.5
    w[::7] = 0.0
    return X, w, X[:k].clone()


def d2(X, C):
    return ((X.double()[:, None, :] - C.double()[None, :, :]) ** 2).sum(-1)


def means64(X, w, a, C):
    """float64 weighted means of X under the assignment a; an empty centre keeps C's row"""
    import torch
    X, w, C = X.double(), w.double(), C.double()
    ws = torch.zeros(C.shape[0], dtype=torch.float64).index_add_(0, a.long(), w)
    S = torch.zeros_like(C).index_add_(0, a.long(), X * w[:, None])
    return torch.where(ws[:, None] > 0, S / ws.clamp_min(1e-12)[:, None], C)


def lloyd64(X, w, C, iters, atol, rtol):
    """the rule of lloyd_kernel / _recluster in double -> C, assign, update iterations run"""
    C, done = C.double(), 0
    for _ in range(iters):
        new = means64(X, w, d2(X, C).argmin(1), C)
        stop = bool(((new - C).abs() <= atol + rtol * C.abs()).all())
        C, done = new, done + 1
        if stop:
            break
    return C, d2(X, C).argmin(1), done


def run_wide(X, w, C0, iters, atol=1e-6, rtol=1e-5):
    from jubatus_amd.ops import hip
    C = C0.clone().to(dev())
    assign, done = hip.lloyd_wide(X.to(dev()), w.to(dev()), C, iters, atol, rtol)
    a = assign.cpu().long()
    assert int(a.min()) >= 0 and int(a.max()) < C0.shape[0]
    return C.cpu(), a, done


def close_to(C, ref, X):
    import torch
    print(f"max |dC| {(C - ref).abs().max():.3g}")
    torch.testing.assert_close(C, ref.float(), rtol=1e-4, atol=1e-4 * float(X.abs().max()))


def check_one_step(X, w, C0, exact):
    import torch
    n, d = X.shape
    C, a0, done = run_wide(X, w, C0, 0)
    assert done == 0 and torch.equal(C, C0)
    D = d2(X, C0)
    excess = D[torch.arange(n), a0] - D.min(1).values
    bound = 4 * (d + 2) * 2.0 ** -24 * ((X.double() ** 2).sum(1) + (C0.double() ** 2).sum(1).max())
    print(f"largest excess / bound {float((excess / bound).max()):.3g}, "
          f"{int((a0 != D.argmin(1)).sum())} of {n} differ from the float64 arg-min")
    assert bool((excess <= bound).all())
    if exact:
        assert torch.equal(a0, D.argmin(1))
    C, _, done = run_wide(X, w, C0, 1)
    assert done == 1
    close_to(C, means64(X, w, a0, C0), X)
    return C


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("n,k,d", SHAPES)
def test_lloyd_wide_one_step_matches_float64(n, k, d, regime):
    X, w, C0 = inputs(n, k, d, REGIMES[regime])
    check_one_step(X, w, C0, regime == "separated")


def test_lloyd_wide_empty_centre_keeps_its_bits():
    import torch
    X, w, C0 = inputs(300, 5, 17, 6.0)
    C0 = C0.clone()
    C0[2] = 1e3
    C = check_one_step(X, w, C0, True)
    assert torch.equal(C[2], C0[2])


@pytest.mark.parametrize("n,k,d", [(300, 5, 17), (777, 130, 33), (600, 16, 260)])
def test_lloyd_wide_converges_as_float64_lloyd(n, k, d):
    import torch
    X, w, C0 = inputs(n, k, d, 6.0)
    rC, ra, rdone = lloyd64(X, w, C0, 100, 1e-6, 1e-5)
    C, a, done = run_wide(X, w, C0, 100)
    print(f"iterations {done} (float64 {rdone})")
    assert done == rdone and torch.equal(a, ra)
    close_to(C, rC, X)


def test_lloyd_wide_is_bit_identical_across_launches():
    import torch
    X, w, C0 = inputs(1100, 103, 40, 0.5)
    a, b = run_wide(X, w, C0, 3), run_wide(X, w, C0, 3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_lloyd_wide_range_and_shape_checks():
    import torch
    from jubatus_amd.ops import hip

    def call(n, k, d, kc=None, dc=None, nw=None):
        z = lambda *s: torch.ones(*s, device=dev())   # noqa: E731
        return hip.lloyd_wide(z(n, d), z(nw or n), z(kc or k, dc or d), 1, 1e-6, 1e-5)
    assert call(4, 1025, 2) is None
    assert call(2, 1024, 4097) is None
    with pytest.raises(ValueError):
        call(10, 3, 5, dc=4)
    with pytest.raises(ValueError):
        call(10, 3, 5, nw=9)


# (n, d, k) -> bytes of the Lloyd and of the GMM EM workspace: 4 (fixed + G partial) with G = min(slabs,
# 256, room), Lloyd fixed 4 + k and partial k d + k, GMM fixed k d + 2 k and partial 2 k d + k. The 256 MiB
# cap on the workspace (room) binds in the two rows at n 100000; the last two are outside the range.
WORK_BYTES = [(1, 1, 1, 28, 24), (65, 1, 3, 76, 108), (17000, 3, 5, 20516, 35940), (777, 33, 130, 442536, 889200),
              (2100, 8, 1024, 4870160, 9232384),
              (100000, 2048, 1024, 260177936, 260116480),   # G 31 and 15
              (100000, 4096, 1024, 251723792, 251695104),   # G 15 and 7
              (4, 2, 1025, 0, 0), (2, 4097, 1024, 0, 0)]


@pytest.mark.parametrize("n,d,k,lloyd,gmm", WORK_BYTES)
def test_wide_workspace_sizes(n, d, k, lloyd, gmm):
    """the geometry the two whole-GPU chains share (csrc/hip/jb_slab.hpp), through their work-size entries"""
    from jubatus_amd.ops import hip
    assert int(hip._fn("jb_lloyd_wide_work")(n, d, k)) == lloyd
    assert int(hip._fn("jb_gmm_em_wide_work")(n, d, k)) == gmm


@pytest.mark.parametrize("keys", [600, 1100])   # k x dims 4800: lloyd_kernel's; 8800: past its LDS, the wide chain
def test_clustering_driver_runs_lloyd_on_the_device(keys):
    """k 8 over `keys` numeric keys, method kmeans: the device engine runs a
    Lloyd kernel, not the torch loop (_lloyd_iters is set), and agrees with
    the host engine, which draws the same seeds"""
    import torch
    from jubatus_amd.models.clustering import Clustering
    p = {"k": 8, "compressor_method": "simple", "bucket_size": 64, "compressed_bucket_size": 32, "seed": 0}
    conv = {"num_rules": [{"key": "*", "type": "num"}]}
    r = random.Random(3)
    truth = [[r.gauss(0, 6) for _ in range(keys)] for _ in range(8)]
    pts = [{f"f{q:04d}": c + r.gauss(0, 1) for q, c in enumerate(truth[i % 8])} for i in range(128)]
    g = Clustering("kmeans", p, DatumToFvConverter(conv), dev())
    h = Clustering("kmeans", p, DatumToFvConverter(conv))
    for e in (g, h):
        e.push(pts[:64])
        e.push(pts[64:])
    assert g.centers.is_cuda and g.centers.shape == (8, keys) and g.get_revision() == h.get_revision() == 2
    assert g._lloyd_iters is not None and h._lloyd_iters is None
    torch.testing.assert_close(g.centers.cpu(), h.centers, rtol=1e-3, atol=1e-3)
    assert g.assign == h.assign
