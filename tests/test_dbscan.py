"""clustering engine, method dbscan, on the host path (models/clustering.py
dbscan_host, NumPy float64) against the brute-force oracle of the five rules
(dbscan_oracle.py): through push / get_core_members, MIX, pack / unpack, the
status keys, the CPU server over RPC and the native server's hand-over.
The dbscan definition is this project's own (docs/clustering_dbscan.md)."""
import json
import os
import subprocess

import numpy as np
import pytest

from dbscan_oracle import clusters, oracle
from helpers import ROOT, start_standalone
from jubatus_amd.client import Clustering as ClusteringClient
from jubatus_amd.client import Datum
from jubatus_amd.fv_converter.converter import DatumToFvConverter
from jubatus_amd.models.clustering import Clustering, NotPerformed, NotSupported

CONV = {"num_rules": [{"key": "*", "type": "num"}]}
NATIVE = os.path.join(ROOT, "jubatus_amd", "native_bin", "jubaclustering")
BASE_KEYS = {"method", "k", "revision", "pending", "buckets", "compressor_method", "storage",
             "converter"}


def make(n, eps, mcp, **p):
    """a driver whose first bucket closes at the n-th point, uncompressed"""
    param = {"eps": eps, "min_core_point": mcp, "compressor_method": "simple", "bucket_size": n,
             "compressed_bucket_size": n, "bucket_length": 2, "seed": 1}
    param.update(p)
    return Clustering("dbscan", param, DatumToFvConverter(CONV))


def as_points(xy):
    return [{"x": float(x), "y": float(y)} for x, y in xy]


def got_members(drv_or_list):
    """[[(w, x, y) ...] ...] of get_core_members (driver tuples or client objects)"""
    ms = drv_or_list.get_core_members() if hasattr(drv_or_list, "get_core_members") else drv_or_list
    out = []
    for g in ms:
        row = []
        for m in g:
            w, d = (m.weight, m.point) if hasattr(m, "weight") else m
            nv = dict(d.num_values)
            row.append((float(w), float(nv["x"]), float(nv["y"])))
        out.append(row)
    return out


def want_members(xy, w, eps, mcp):
    label = oracle(np.asarray(xy, np.float64), w, eps, mcp)[0]
    return [[(float(w[i]), float(xy[i][0]), float(xy[i][1])) for i in g] for g in clusters(label)], label


def blob(cx, cy):
    return [(cx + dx, cy + dy) for dx in (0, 1) for dy in (0, 1)]      # 2 x 2 unit square


def run(xy, eps, mcp):
    c = make(len(xy), eps, mcp)
    c.push(as_points(xy))
    assert c.get_revision() == 1
    want, label = want_members(xy, np.ones(len(xy)), eps, mcp)
    assert got_members(c) == want
    return c, label


def test_two_blobs_and_noise():
    xy = blob(1, 1) + [(50, 50)] + blob(20, 1) + [(-40, 7)]
    c, label = run(xy, 1.5, 3.0)
    assert label.tolist() == [0, 0, 0, 0, -1, 5, 5, 5, 5, -1]
    assert len(c.get_core_members()) == 2
    st = c.get_status()
    assert st["clusters"] == "2" and st["noise"] == "2"


def test_border_point_takes_the_lower_label():
    # columns of three points at x = 1, 2 and x = 5, 6; (3.5, 2) is within
    # eps = 1.6 of (2, 2) and (5, 2) only: mass 3 < 4, a border of both
    left = [(x, y) for x in (1, 2) for y in (1, 2, 3)]
    right = [(x, y) for x in (5, 6) for y in (1, 2, 3)]
    for xy in (left + [(3.5, 2)] + right, right + [(3.5, 2)] + left):
        c, label = run(xy, 1.6, 4.0)
        assert label[6] == 0 and sorted(set(label.tolist())) == [0, 7]
        got = c.get_core_members()
        assert [len(g) for g in got] == [7, 6]                 # the border joins the first only


def test_groups_linked_only_through_a_non_core_point_stay_apart():
    a = [(x, 1) for x in (0, 0.5, 1, 1.5, 2)]
    b = [(x, 1) for x in (4.5, 5, 5.5, 6, 6.5)]
    xy = a + b + [(3.25, 1)]             # 1.25 from (2, 1) and from (4.5, 1): mass 3
    c, label = run(xy, 1.6, 4.0)
    assert label.tolist() == [0] * 5 + [5] * 5 + [0]
    assert len(c.get_core_members()) == 2


def test_all_noise_gives_no_cluster_and_the_revision_advances():
    xy = [(10 * i, 1) for i in range(6)]
    c, label = run(xy, 1.5, 2.0)
    assert (label == -1).all() and c.get_core_members() == []
    c.push(as_points([(x + 5, y) for x, y in xy]))
    assert c.get_revision() == 2 and c.get_core_members() == []
    assert c.get_status()["clusters"] == "0" and c.get_status()["noise"] == "12"


@pytest.mark.parametrize("mcp,n_clusters", [(4.0, 1), (4.5, 0)])
def test_single_heavy_point_is_core_by_its_own_weight(mcp, n_clusters):
    # four far points compressed to one of weight 4 (simple: weights scaled up)
    c = make(4, 1.5, mcp, compressed_bucket_size=1)
    c.push(as_points([(0, 1), (100, 1), (200, 1), (300, 1)]))
    assert c.get_revision() == 1
    got = c.get_core_members()
    assert len(got) == n_clusters
    if n_clusters:
        assert len(got[0]) == 1 and got[0][0][0] == 4.0


@pytest.mark.parametrize("param", [{}, {"eps": 1.0}, {"min_core_point": 2.0},
                                   {"eps": 0, "min_core_point": 2.0}, {"eps": -1.0, "min_core_point": 2.0},
                                   {"eps": 1.0, "min_core_point": 0}, {"eps": 1.0, "min_core_point": -3},
                                   {"eps": "1.0", "min_core_point": 2.0},
                                   {"eps": float("nan"), "min_core_point": 2.0}])
def test_eps_and_min_core_point_are_required_and_positive(param):
    with pytest.raises(ValueError):
        Clustering("dbscan", param, DatumToFvConverter(CONV))


@pytest.mark.parametrize("comp", ["compressive_kmeans", "compressive_gmm", "nope"])
def test_compressor_must_be_simple(comp):
    with pytest.raises(ValueError):
        make(10, 1.0, 2.0, compressor_method=comp)


def test_k_is_ignored():
    assert make(10, 1.0, 2.0, k=0).get_revision() == 0


def test_queries():
    c = make(8, 1.5, 3.0)
    with pytest.raises(NotPerformed):
        c.get_core_members()
    for before in (True, False):
        with pytest.raises(NotSupported, match="get_k_center is not supported by dbscan"):
            c.get_k_center()
        with pytest.raises(NotSupported, match="get_nearest_center is not supported by dbscan"):
            c.get_nearest_center({"x": 1.0, "y": 1.0})
        with pytest.raises(NotSupported, match="get_nearest_members is not supported by dbscan"):
            c.get_nearest_members({"x": 1.0, "y": 1.0})
        if before:
            c.push(as_points(blob(1, 1) + blob(9, 9)))
    assert len(c.get_core_members()) == 2
    assert issubclass(NotSupported, RuntimeError)


def test_pack_unpack_reclusters_to_the_same_members():
    xy = blob(1, 1) + [(50, 50)] + blob(20, 1) + [(7, 7), (8, 8)]
    c = make(9, 1.5, 3.0)
    c.push(as_points(xy))
    assert c.get_revision() == 1 and len(c.pending) == 2
    obj = c.pack()
    assert obj["method"] == "dbscan"
    d = make(9, 1.5, 3.0)
    d.unpack(obj)
    assert d.get_revision() == 1 and len(d.pending) == 2
    assert got_members(d) == got_members(c) == want_members(xy[:9], np.ones(9), 1.5, 3.0)[0]
    d.clear()
    assert d.get_revision() == 0
    with pytest.raises(NotPerformed):
        d.get_core_members()


def test_mix_members_equal_the_oracle_over_the_union():
    # each server holds half of every square: alone all is noise, mixed two clusters
    xa = [(1, 1), (2, 2), (20, 1), (21, 2), (70, 70)]
    xb = [(1, 2), (2, 1), (20, 2), (21, 1), (-70, 70)]
    a, b = make(5, 1.5, 3.0), make(5, 1.5, 3.0)
    a.push(as_points(xa))
    b.push(as_points(xb))
    assert a.get_core_members() == [] and b.get_core_members() == []
    mixed = Clustering.mix_diff(a.get_diff(), b.get_diff())
    assert a.put_diff(mixed) and b.put_diff(mixed)
    assert a.get_revision() == 2
    for drv, xy in ((a, xa + xb), (b, xb + xa)):
        want, label = want_members(xy, np.ones(10), 1.5, 3.0)
        assert got_members(drv) == want and len(want) == 2 and (label == -1).sum() == 2


def test_status_keys():
    c = make(8, 1.5, 3.0)
    st = c.get_status()
    assert set(st) == BASE_KEYS | {"eps", "min_core_point", "clusters", "noise"}
    assert st["method"] == "dbscan" and float(st["eps"]) == 1.5 and float(st["min_core_point"]) == 3.0
    assert all(isinstance(v, str) for v in st.values())
    km = Clustering("kmeans", {"k": 2}, DatumToFvConverter(CONV))
    assert set(km.get_status()) == BASE_KEYS


def _config(n=10):
    return {"method": "dbscan", "converter": CONV,
            "parameter": {"eps": 1.5, "min_core_point": 3.0, "compressor_method": "simple",
                          "bucket_size": n, "compressed_bucket_size": n, "bucket_length": 2,
                          "forgetting_factor": 0.0, "forgetting_threshold": 0.5, "seed": 0}}


def test_server(tmp_path):
    xy = blob(1, 1) + [(50, 50)] + blob(20, 1) + [(-40, 7)]
    h = start_standalone("clustering", json.dumps(_config(len(xy))), tmp_path)
    try:
        with ClusteringClient("127.0.0.1", h.argv.port, "") as c:
            with pytest.raises(Exception, match="not performed"):
                c.get_core_members()
            assert c.push([Datum(p) for p in as_points(xy[:4])]) is True
            assert c.get_revision() == 0
            assert c.push([Datum(p) for p in as_points(xy[4:])]) is True
            assert c.get_revision() == 1
            assert got_members(c.get_core_members()) == want_members(xy, np.ones(len(xy)), 1.5, 3.0)[0]
            with pytest.raises(Exception, match="get_k_center is not supported by dbscan"):
                c.get_k_center()
            with pytest.raises(Exception, match="get_nearest_members is not supported by dbscan"):
                c.get_nearest_members(Datum({"x": 1.0, "y": 1.0}))
            (st,) = c.get_status().values()
            assert st["method"] == "dbscan" and st["clusters"] == "2" and st["noise"] == "2"
            c.save("d")
            assert c.clear() is True and c.get_revision() == 0
            assert c.load("d") is True and c.get_revision() == 1
            assert len(c.get_core_members()) == 2
    finally:
        h.stop()


@pytest.mark.skipif(not os.path.exists(NATIVE), reason="native jubaclustering not built")
def test_native_server_hands_dbscan_to_python(tmp_path):
    p = tmp_path / "dbscan.json"
    p.write_text(json.dumps(_config()))
    r = subprocess.run([NATIVE, "--native-check", "-f", str(p)], capture_output=True, text=True,
                       timeout=30)
    assert r.stdout.strip().startswith("python:"), (r.stdout, r.stderr)
