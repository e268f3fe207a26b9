"""csrc/hip/dbscan.hip (ops.hip.dbscan) against the brute-force float64
oracle of the five rules (dbscan_oracle.py): labels, masses, core flags and
every bit of the adjacency bitmap, at the sizes where the kernels change
path (16-row tile, 64-bit word, K step of 4), on graph shapes that stress the
lock-free union, on random floats behind a guard band, and through the GPU
driver and server. Every case but the last two is a few hundred points."""
import functools
import json

import numpy as np
import pytest

from dbscan_oracle import clusters, oracle

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                 # fp32 unit roundoff


def gamma(k):
    return k * U / (1.0 - k * U)


def _dev():
    import torch
    return torch.device("cuda", 0)


def gpu_dbscan(X, w, eps, mcp):
    """-> (label [n] int64, mass [n] float32, A [n, n] bool, tail bits [n, 64 nw - n] bool)"""
    import torch
    from jubatus_amd.ops import hip
    Xd = torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(_dev())
    wd = torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(_dev())
    label, mass, adj = hip.dbscan(Xd, wd, eps, mcp)        # raises when status != 0
    n = X.shape[0]
    assert label.dtype == torch.int32 and label.shape == (n,)
    assert mass.dtype == torch.float32 and mass.shape == (n,)
    assert adj.dtype == torch.int64 and adj.shape == (n, (n + 63) // 64)
    words = adj.cpu().numpy().view(np.uint64)
    bits = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    bits = bits.reshape(n, -1)
    return label.cpu().numpy().astype(np.int64), mass.cpu().numpy(), bits[:, :n], bits[:, n:]


def check(X, w, eps, mcp):
    """the GPU result equals the oracle's, and the bitmap invariants hold"""
    X = np.asarray(X, np.float32)
    w = np.asarray(w, np.float32)
    want_label, want_core, want_mass, want_A, _ = oracle(X, w, eps, mcp)
    label, mass, A, tail = gpu_dbscan(X, w, eps, mcp)
    assert not tail.any(), "bits for columns >= n are set"
    assert A.diagonal().all()
    assert (A == A.T).all()
    assert (A == want_A).all(), np.argwhere(A != want_A)[:8]
    assert (mass.astype(np.float64) == want_mass).all()
    assert ((mass >= np.float32(mcp)) == want_core).all()
    assert (label == want_label).all(), np.flatnonzero(label != want_label)[:8]
    return want_label, want_core, want_mass


# ---------------------------------------------------------------- shapes
def integer_case(n, d, seed=0):
    """small-integer coordinates (every fp32 distance exact, eps^2 = 2.25 is no
    integer: no pair on the threshold), weights multiples of 0.25 (every mass
    exact in any order, zeros among them), and min_core_point taken from the
    masses themselves, so at least one point is core by equality. Positions
    along dim 0 leave gaps (several components); the next two dims add 0..2."""
    rng = np.random.default_rng(1000 * n + d + seed)
    X = np.zeros((n, d), np.float32)
    X[:, 0] = rng.integers(0, max(2, (3 * n) // 4), n)
    for j in range(1, min(d, 3)):
        X[:, j] = rng.integers(0, 2, n)
    if d > 3:
        X[:, d - 1] = 3 * rng.integers(0, 2, n)     # the padded K step matters: 9 apart or 0
    w = rng.integers(0, 9, n).astype(np.float32) * 0.25
    w[0] = 0.5                                      # some mass is positive, also at n = 1
    mass = oracle(X, w, 1.5, 1.0)[2]
    pos = np.sort(mass[mass > 0])
    return X, w, float(pos[pos.size // 2])          # the median of the positive masses


@pytest.mark.parametrize("d", [1, 3, 4, 5, 17])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 129, 257])
def test_shapes_against_the_oracle(n, d):
    X, w, mcp = integer_case(n, d)
    _, core, mass = check(X, w, 1.5, mcp)
    assert (mass == mcp).any(), "no point is core by equality"
    assert core[mass == mcp].all()


# ---------------------------------------------------------------- graphs
PERM = np.random.default_rng(7).permutation(257)


def test_shuffled_chain_is_one_component_labelled_zero():
    """257 points on a line, spacing 1, eps 1.5, in a fixed shuffled order: one
    component of diameter 256, the longest this n allows; the end points have
    mass 2 = min_core_point"""
    X = PERM.astype(np.float32)[:, None]
    label, core, _ = check(X, np.ones(257), 1.5, 2.0)
    assert core.all() and (label == 0).all()
    assert (label[np.argsort(PERM)] == 0).all()         # in line order too


def bridge_case(order):
    a = [x * 0.5 for x in range(0, 21)]                  # 0 .. 10, spacing 0.5
    b = [12.5 + x * 0.5 for x in range(0, 21)]           # 12.5 .. 22.5
    pts = {"ab": a + b + [11.25], "ba": b + a + [11.25]}[order]
    return np.asarray(pts, np.float32)[:, None]


@pytest.mark.parametrize("order", ["ab", "ba"])
def test_chains_bridged_by_a_non_core_point_stay_two_clusters(order):
    """11.25 is within eps = 1.6 of one end of each chain only (mass 3 < 4,
    the ends have mass 4): a border of both, it takes the lower label and
    the chains stay apart"""
    label, core, _ = check(bridge_case(order), np.ones(43), 1.6, 4.0)
    assert core[:42].all() and not core[42]
    assert label.tolist() == [0] * 21 + [21] * 21 + [0]
    assert [len(g) for g in clusters(label)] == [22, 21]


def test_duplicated_points():
    X = np.repeat(np.asarray([[1, 2, 3], [1, 2, 3], [9, 9, 9], [4, 0, 4]], np.float32), 5, axis=0)
    label, _, mass = check(X, np.full(20, 0.5), 0.5, 2.5)
    assert label.tolist() == [0] * 10 + [10] * 5 + [15] * 5 and mass.tolist() == [5.0] * 10 + [2.5] * 10


def test_zero_weight_points():
    # a weightless square (noise), a square beside a weightless point (border)
    X = np.asarray([[0, 0], [0, 1], [1, 0], [1, 1], [10, 0], [10, 1], [11, 0], [11, 1], [12, 1]],
                   np.float32)
    w = np.asarray([0, 0, 0, 0, 1, 1, 1, 1, 0], np.float32)
    label, core, _ = check(X, w, 1.5, 4.0)
    assert label.tolist() == [-1] * 4 + [4] * 5 and core.tolist() == [False] * 4 + [True] * 4 + [False]


def test_all_noise():
    X = (10.0 * np.arange(130, dtype=np.float32))[:, None] * np.ones((1, 3), np.float32)
    label, core, _ = check(X, np.ones(130), 1.5, 2.0)
    assert (label == -1).all() and not core.any()


def test_one_cluster_holds_everything():
    rng = np.random.default_rng(3)
    X = rng.integers(0, 2, (200, 5)).astype(np.float32)       # the corners of a cube: d2 <= 5
    label, core, _ = check(X, np.ones(200), 2.5, 10.0)
    assert core.all() and (label == 0).all()


# ---------------------------------------------------------------- floats
N_F, D_F, EPS_F, MCP_F, SEED_F = 257, 17, 3.0, 12.0, 4


@functools.lru_cache(maxsize=None)
def float_case():
    rng = np.random.default_rng(SEED_F)
    centers = rng.uniform(-3.0, 3.0, (6, D_F))
    X = (centers[rng.integers(0, 6, N_F)] + 0.5 * rng.standard_normal((N_F, D_F))).astype(np.float32)
    w = rng.uniform(0.5, 1.5, N_F).astype(np.float32)
    return X, w, oracle(X, w, EPS_F, MCP_F)


def float_band(X):
    """[n, n] bound on |fp32 d2 - exact d2| (derivation: test_random_floats)"""
    X = np.asarray(X, np.float64)
    xn = (X * X).sum(1)
    return gamma(X.shape[1] + 2) * (xn[:, None] + xn[None, :] + 2.0 * (np.abs(X) @ np.abs(X).T))


def test_random_floats_behind_a_guard_band():
    """Random fp32 points cannot be checked pair by pair without a guard band:
    the kernel's distance differs from the float64 oracle's, and one flipped
    edge can merge two components. The band: the kernel evaluates

        d2 = fl(fl(xn_i + xn_j) - 2 g),   xn = fl(sum_k x_k^2),   g = fl(sum_k x_ik x_jk)

    (the factor 2 is exact). Each of the 3 d products takes part in at most d
    roundings inside its own sum (d - 1 additions and its own rounding; an
    fma chain has fewer) and in the 2 of the final additions, so by the
    standard bound of an fp32 dot product of length d + 2 (Higham, Accuracy and
    Stability of Numerical Algorithms, (3.5)), for any summation order,

        |d2 - exact| <= gamma_{d+2} (xn_i + xn_j + 2 sum_k |x_ik x_jk|),
        gamma_k = k u / (1 - k u),  u = 2^-24.

    The inputs are fp32 numbers handed to the oracle as they are and eps^2 = 9
    is an fp32 number, so nothing else rounds; max(., 0) moves a value towards
    the exact one. With no pair inside the band every compare agrees with the
    oracle's, hence the whole bitmap. The masses: an fp32 sum of m <= n weights
    in any order is within gamma_{m-1} sum w <= gamma_n mass of the exact one,
    so no mass may lie that close to min_core_point. The seed was chosen on
    the CPU; both counts are asserted, never skipped."""
    X, w, (want_label, want_core, want_mass, want_A, d2) = float_case()
    in_band = np.abs(d2 - EPS_F * EPS_F) <= float_band(X)
    np.fill_diagonal(in_band, False)
    assert in_band.sum() == 0
    assert (np.abs(want_mass - MCP_F) > gamma(N_F) * want_mass).all()
    # the case is not degenerate: several clusters, border and noise points, near misses
    assert len(clusters(want_label)) >= 3 and (~want_core).sum() >= 10 and (want_label < 0).any()
    assert (np.abs(d2 - EPS_F * EPS_F) < 0.05).sum() >= 10
    label, mass, A, tail = gpu_dbscan(X, w, EPS_F, MCP_F)
    assert not tail.any() and (A == A.T).all() and (A == want_A).all()
    assert (np.abs(mass - want_mass) <= gamma(N_F) * want_mass).all()
    assert ((mass >= np.float32(MCP_F)) == want_core).all()
    assert (label == want_label).all()


def test_three_launches_are_bitwise_identical():
    X, w, _ = float_case()
    runs = [gpu_dbscan(X, w, EPS_F, MCP_F) for _ in range(3)]
    for r in runs[1:]:
        assert (r[0] == runs[0][0]).all()
        assert r[1].tobytes() == runs[0][1].tobytes()
        assert (r[2] == runs[0][2]).all() and (r[3] == runs[0][3]).all()


def test_limits_raise_before_any_launch():
    import torch
    from jubatus_amd.ops import hip
    assert hip.DBSCAN_MAX_N == 65536
    w = torch.ones(hip.DBSCAN_MAX_N + 1, dtype=torch.float32, device=_dev())
    with pytest.raises(ValueError, match="over the limit"):
        hip.dbscan(w[:, None].contiguous(), w, 1.0, 2.0)
    X = torch.ones((8, 2), dtype=torch.float32, device=_dev())
    for bad in ((X, w[:7], 1.0, 2.0), (X[:, :0], w[:8], 1.0, 2.0), (X[0], w[:8], 1.0, 2.0),
                (X, w[:8], 0.0, 2.0), (X, w[:8], 1.0, 0.0)):
        with pytest.raises(ValueError):
            hip.dbscan(*bad)
    # the C entry refuses the same on its own (-2, nothing queued)
    st = torch.zeros(1, dtype=torch.int32, device=_dev())
    buf = torch.zeros(64, dtype=torch.int64, device=_dev())
    p = buf.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    for n, d in ((0, 2), (hip.DBSCAN_MAX_N + 1, 2), (8, 0)):
        assert hip._fn("jb_dbscan")(p, n, d, p, p, 1.0, 2.0, p, p, p, p, p, st.data_ptr(), s) == -2


# ---------------------------------------------------------------- driver, server
CONV = {"num_rules": [{"key": "*", "type": "num"}]}


def _param(n):
    return {"eps": 1.5, "min_core_point": 3.0, "compressor_method": "simple", "bucket_size": n,
            "compressed_bucket_size": n, "bucket_length": 2, "seed": 1}


def _points(n, d):
    X = integer_case(n, d)[0]
    return [{f"f{j:02d}": float(v) for j, v in enumerate(row)} for row in X]


def _members(ms):
    out = []
    for g in ms:
        out.append([(float(m.weight if hasattr(m, "weight") else m[0]),
                     sorted((m.point if hasattr(m, "point") else m[1]).num_values)) for m in g])
    return out


@pytest.mark.parametrize("n,d", [(65, 3), (129, 5), (257, 17)])
def test_gpu_driver_agrees_with_the_host_path(n, d):
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.models.clustering import Clustering
    pts = _points(n, d)
    g = Clustering("dbscan", _param(n), DatumToFvConverter(CONV), device=_dev())
    c = Clustering("dbscan", _param(n), DatumToFvConverter(CONV))
    for drv in (g, c):
        drv.push(pts)
        assert drv.get_revision() == 1
    assert g.get_status()["storage"] == "hbm" and c.get_status()["storage"] == "host"
    got, want = _members(g.get_core_members()), _members(c.get_core_members())
    assert got == want and len(want) >= 2
    assert g.get_status()["noise"] == c.get_status()["noise"]


def test_gpu_server_end_to_end(tmp_path):
    from jubatus_amd.client import Clustering as ClusteringClient
    from jubatus_amd.client import Datum
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    from jubatus_amd.framework.server_helper import ServerHelper
    from jubatus_amd.framework.server_util import ServerArgv
    from jubatus_amd.models.clustering import Clustering
    from jubatus_amd.server import get_serv
    n, d = 129, 5
    pts = _points(n, d)
    cfg = tmp_path / "dbscan.json"
    cfg.write_text(json.dumps({"method": "dbscan", "converter": CONV, "parameter": _param(n)}))
    a = ServerArgv.parse(["-p", "9199", "-b", "127.0.0.1", "-f", str(cfg), "-d", str(tmp_path),
                          "--gpu", "0"], "clustering")
    a.port = 0
    h = ServerHelper(get_serv("clustering"), a, install_signals=False)
    h.start(block=False)
    try:
        ref = Clustering("dbscan", _param(n), DatumToFvConverter(CONV))
        ref.push(pts)
        with ClusteringClient("127.0.0.1", h.argv.port, "") as c:
            assert c.push([Datum(p) for p in pts]) is True
            assert c.get_revision() == 1
            assert _members(c.get_core_members()) == _members(ref.get_core_members())
            with pytest.raises(Exception, match="get_k_center is not supported by dbscan"):
                c.get_k_center()
            (st,) = c.get_status().values()
            assert st["storage"] == "hbm" and st["clusters"] == ref.get_status()["clusters"]
    finally:
        h.stop()
