"""Label capacities above 1024 (2048 .. 16384) on the paths that need no GPU:
the host driver (models/classifier.py over models/linear_oracle.py), model
files and jubadump, the native server's host backend, the label re-layout of
a two-rank MIX, the cap error and the free-memory check before the tables
grow. The GPU side is tests/test_gpu_many_labels.py."""
import json
import os
import random
import socket
import subprocess
import time

import numpy as np
import pytest
import torch.multiprocessing as mp

from helpers import ROOT
from jubatus_amd.fv_converter.converter import DatumToFvConverter
from jubatus_amd.models import classifier as clf_mod
from jubatus_amd.models import linear_oracle as lo
from jubatus_amd.models.classifier import LABEL_CAPS, ClassifierConfigError, LinearClassifier

BIN = os.path.join(ROOT, "jubatus_amd", "native_bin", "jubaclassifier")


def _conv(H):
    return {"string_rules": [{"key": "*", "type": "str", "sample_weight": "bin", "global_weight": "bin"}],
            "num_rules": [{"key": "*", "type": "num"}], "hash_max_size": H}


def _cfg(method, H):
    full = {"string_filter_types": {}, "string_filter_rules": [], "num_filter_types": {},
            "num_filter_rules": [], "string_types": {}, "num_types": {}}
    full.update(_conv(H))
    return {"converter": full, "method": method, "parameter": {"regularization_weight": 1.0}}


def _stream(nlabels, extra, seed):
    """one sample of every label in label order, then ``extra`` random ones;
    the wire form [label, [string values, num values, binary values]]"""
    rng = random.Random(seed)
    ys = list(range(nlabels)) + [rng.randrange(nlabels) for _ in range(extra)]
    return [[f"L{y}", [[["w", f"t{y % 97}"], ["u", f"n{rng.randrange(40)}"]],
                       [["x", (y % 7 - 3) * 0.5 + rng.gauss(0, 1)]], []]] for y in ys]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _payload(nlabels, H, method="PA"):
    """an empty model with ``nlabels`` registered labels (the model file form)"""
    return {"method": method, "H": H, "labels": [f"L{i}" for i in range(nlabels)],
            "counts": [0] * nlabels, "rows": b"", "W": b"", "P": b"", "weights": None}


def test_one_definition_of_the_capacities():
    from jubatus_amd.ops import hip
    assert hip.LABEL_CAPS is LABEL_CAPS
    assert LABEL_CAPS[:8] == (8, 16, 32, 64, 128, 256, 512, 1024)
    assert LABEL_CAPS[8:] == (2048, 4096, 8192, 16384)


def test_1100_labels_train_and_classify_like_the_oracle():
    H = 2048
    c = LinearClassifier("AROW", {"regularization_weight": 1.0}, DatumToFvConverter(_conv(H)))
    data = _stream(1100, 100, seed=1)
    for i in range(0, len(data), 100):
        assert c.train([(l, d) for l, d in data[i:i + 100]]) == 100
    assert c.LC == 2048 and c.get_status()["label_capacity"] == "2048"
    labels = c.get_labels()
    assert len(labels) == 1100 and sum(labels.values()) == len(data)
    # the same stream straight through the oracle: label ids by first occurrence
    conv = DatumToFvConverter(_conv(H))
    W = np.zeros((H, 2048), np.float32)
    P = np.ones((H, 2048), np.float32)
    active = np.zeros(2048, np.int32)
    ids, upd = {}, 0
    for i in range(0, len(data), 100):
        for lab, _ in data[i:i + 100]:        # a request registers its labels, then trains
            active[ids.setdefault(lab, len(ids))] = 1
        for lab, d in data[i:i + 100]:
            idx, val = conv.hashed(conv.convert(d))
            upd += lo.train_one(W, P, np.asarray(idx, np.int64), np.asarray(val, np.float32),
                                ids[lab], active, lo.AROW, 1.0)
    assert c.train_stats()["updated"] == upd and upd > 1100
    np.testing.assert_array_equal(c.W, W)
    np.testing.assert_array_equal(c.P, P)
    q = [d for _, d in data[:20]]
    for d, res in zip(q, c.classify(q)):
        idx, val = conv.hashed(conv.convert(d))
        s = lo.scores(W, np.asarray(idx, np.int64), np.asarray(val, np.float32))
        got = dict(res)
        assert len(got) == 1100
        for lab, y in ids.items():
            assert got[lab] == float(s[y]), (lab, got[lab], s[y])


def test_growth_1024_to_2048_keeps_every_score():
    H = 1024
    c = LinearClassifier("AROW", {"regularization_weight": 1.0}, DatumToFvConverter(_conv(H)))
    data = _stream(1024, 60, seed=2)
    c.train([(l, d) for l, d in data])
    assert c.LC == 1024
    probe = [data[5][1], data[700][1]]
    before = [dict(r) for r in c.classify(probe)]
    assert c.set_label("label 1025") is True
    assert c.LC == 2048 and c.W.shape == (H, 2048) and c.P.shape == (H, 2048)
    after = [dict(r) for r in c.classify(probe)]
    for b, a in zip(before, after):
        assert len(b) == 1024 and len(a) == 1025
        assert a.pop("label 1025") == 0.0
        assert a == b                       # bit-equal: float equality of every score
    assert any(v != 0.0 for v in before[0].values())


def test_label_16385_is_refused_and_the_model_stays():
    H = 64
    c = LinearClassifier("PA", None, DatumToFvConverter(_conv(H)))
    c.unpack(_payload(16384, H))
    assert c.LC == 16384 and len(c.get_labels()) == 16384
    c.train([("L16383", {"w": "a", "x": 1.0}), ("L0", {"w": "b", "x": -1.0})])
    W = c.W.copy()
    want = f"at most {LABEL_CAPS[-1]} labels are supported"
    assert want == "at most 16384 labels are supported"
    with pytest.raises(ClassifierConfigError, match=want):
        c.set_label("one too many")
    with pytest.raises(ClassifierConfigError, match=want):
        c.train([("another", {"w": "a"})])
    assert c.LC == 16384 and c.W.shape == (H, 16384)
    np.testing.assert_array_equal(c.W, W)
    names = c.get_labels()
    assert len(names) == 16384 and "one too many" not in names and "another" not in names
    assert c.set_label("L5") is False
    top = max(c.classify([{"w": "a", "x": 1.0}])[0], key=lambda t: t[1])[0]
    assert top == "L16383"
    assert c.train([("L7", {"w": "c", "x": 0.5})]) == 1


def test_free_memory_check_refuses_growth_past_1024(monkeypatch):
    """the hook's wiring on the host driver (host tables are not checked by
    default: the hook returns None there)"""
    H = 1024
    assert clf_mod.device_free_bytes(None) is None
    c = LinearClassifier("AROW", {"regularization_weight": 1.0}, DatumToFvConverter(_conv(H)))
    c.unpack(_payload(1024, H, "AROW"))
    c.train([("L3", {"w": "a", "x": 1.0}), ("L9", {"w": "b", "x": -1.0})])
    W, P = c.W.copy(), c.P.copy()
    seen = []

    def one_mib(device):
        seen.append(device)
        return 1 << 20
    monkeypatch.setattr(clf_mod, "device_free_bytes", one_mib)
    need = H * 2048 * 8 + 4 * 2048
    assert c.table_bytes(2048) == need
    with pytest.raises(ClassifierConfigError) as e:
        c.set_label("label 1025")
    msg = str(e.value)
    for part in ("1025 labels", "label capacity 2048", f"hash_max_size {H}", f"{need} bytes",
                 f"{1 << 20} bytes are free"):
        assert part in msg, (part, msg)
    assert seen == [None]
    assert c.LC == 1024 and c.W.shape == (H, 1024)
    np.testing.assert_array_equal(c.W, W)
    np.testing.assert_array_equal(c.P, P)
    assert len(c.get_labels()) == 1024 and "label 1025" not in c.get_labels()
    assert c.train([("L3", {"w": "a", "x": 1.0})]) == 1          # still serves
    W = c.W.copy()
    # growing within 1024 is not checked, and with room the same call grows
    small = LinearClassifier("PA", None, DatumToFvConverter(_conv(H)))
    for i in range(9):
        small.set_label(f"s{i}")
    assert small.LC == 16 and len(seen) == 1
    monkeypatch.undo()
    assert c.set_label("label 1025") is True and c.LC == 2048
    np.testing.assert_array_equal(c.W[:, :1024], W)


def test_model_file_round_trip_1500_labels_and_jubadump(tmp_path):
    from helpers import start_standalone
    from jubatus_amd.cmd import jubadump
    from jubatus_amd.common.mprpc import RpcClient
    from jubatus_amd.framework.server_helper import ServerHelper
    from jubatus_amd.framework.server_util import ServerArgv
    from jubatus_amd.server import get_serv

    data = _stream(1500, 50, seed=3)
    q = [d for _, d in data[:10]]
    h = start_standalone("classifier", json.dumps(_cfg("AROW", 1024)), tmp_path)
    try:
        with RpcClient("127.0.0.1", h.argv.port, 60.0) as c:
            for i in range(0, len(data), 310):
                assert c.call("train", "", data[i:i + 310]) == len(data[i:i + 310])
            got = c.call("classify", "", q)
            (_, st), = c.call("get_status", "").items()
            assert st[b"label_capacity" if b"label_capacity" in st else "label_capacity"] in (b"2048", "2048")
            (_, path), = c.call("save", "", "many").items()
            path = path.decode() if isinstance(path, bytes) else path
    finally:
        h.stop()
    dumped = jubadump.dump(path)
    assert dumped["model"]["method"] == "AROW" and dumped["model"]["hash_max_size"] == 1024
    assert len(dumped["model"]["labels"]) == 1500
    assert sum(dumped["model"]["labels"].values()) == len(data)
    assert any("L1499" in row for row in dumped["model"]["weights"].values())
    a = ServerArgv.parse(["-p", "9199", "-b", "127.0.0.1", "-m", path, "-d", str(tmp_path), "--cpu"],
                         "classifier")
    a.port = 0
    h2 = ServerHelper(get_serv("classifier"), a, install_signals=False)
    h2.start(block=False)
    try:
        with RpcClient("127.0.0.1", h2.argv.port, 60.0) as c:
            assert c.call("classify", "", q) == got
            assert len(c.call("get_labels", "")) == 1500
    finally:
        h2.stop()


def _start_native(args, timeout=60):
    from jubatus_amd.common.mprpc import RpcClient, RpcIOError, RpcTimeoutError
    port = _free_port()
    env = dict(os.environ, PATH="/nonexistent", JUBATUS_FORCE_CPU="1")
    p = subprocess.Popen([BIN, "-p", str(port), "-b", "127.0.0.1", *args], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, env=env)
    deadline = time.time() + timeout
    while time.time() < deadline:
        try:
            c = RpcClient("127.0.0.1", port, 60.0)
            c.call("get_config", "")
            return p, c
        except (OSError, RpcIOError, RpcTimeoutError):
            if p.poll() is not None:
                break
            time.sleep(0.1)
    out = p.stdout.read().decode(errors="replace") if p.poll() is not None else ""
    p.kill()
    raise AssertionError(f"server did not start: {out}")


def _stop(p, c):
    c.close()
    p.terminate()
    p.wait(timeout=30)


def _plain(rows):
    return [{(k.decode() if isinstance(k, bytes) else k): v for k, v in r} for r in rows]


def _close(got, want, tol=1e-3):
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w)
        for k in w:
            assert abs(g[k] - w[k]) <= tol * max(1.0, abs(w[k])), (k, g[k], w[k])


def test_native_host_backend_1100_labels_and_model_files(tmp_path):
    """the native server without a GPU: 1100 labels over RPC against the host
    driver, its model file into the Python server and the Python server's
    model file into it"""
    from jubatus_amd.common.mprpc import RpcClient
    from jubatus_amd.framework.server_helper import ServerHelper
    from jubatus_amd.framework.server_util import ServerArgv
    from jubatus_amd.server import get_serv

    cfg = _cfg("AROW", 1024)
    cfg_file = tmp_path / "many.json"
    cfg_file.write_text(json.dumps(cfg))
    data = _stream(1100, 100, seed=4)
    q = [d for _, d in data[:12]]
    ref = LinearClassifier("AROW", cfg["parameter"], DatumToFvConverter(cfg["converter"]))
    for i in range(0, len(data), 100):
        ref.train([(l, d) for l, d in data[i:i + 100]])
    want = [dict(r) for r in ref.classify(q)]
    p, c = _start_native(["-f", str(cfg_file), "-d", str(tmp_path)])
    try:
        for i in range(0, len(data), 100):
            assert c.call("train", "", data[i:i + 100]) == 100
        got = _plain(c.call("classify", "", q))
        assert len(got[0]) == 1100
        _close(got, want)
        (_, st), = c.call("get_status", "").items()
        st = {(k.decode() if isinstance(k, bytes) else k): (v.decode() if isinstance(v, bytes) else v)
              for k, v in st.items()}
        assert st["backend"] == "host" and st["label_capacity"] == "2048", st
        assert int(st["train.samples_updated"]) == ref.train_stats()["updated"]
        assert len(c.call("get_labels", "")) == 1100
        (_, npath), = c.call("save", "", "n1").items()
        npath = npath.decode() if isinstance(npath, bytes) else npath
    finally:
        _stop(p, c)
    # native file -> Python server -> Python file
    a = ServerArgv.parse(["-p", "9199", "-b", "127.0.0.1", "-m", npath, "-d", str(tmp_path), "--cpu"],
                         "classifier")
    a.port = 0
    h = ServerHelper(get_serv("classifier"), a, install_signals=False)
    h.start(block=False)
    try:
        with RpcClient("127.0.0.1", h.argv.port, 60.0) as pc:
            _close(_plain(pc.call("classify", "", q)), got, tol=1e-5)
            assert len(pc.call("get_labels", "")) == 1100
            (_, ppath), = pc.call("save", "", "p1").items()
            ppath = ppath.decode() if isinstance(ppath, bytes) else ppath
    finally:
        h.stop()
    # Python file -> native
    p, c = _start_native(["-m", ppath, "-d", str(tmp_path)])
    try:
        assert _plain(c.call("classify", "", q)) == got
        assert len(c.call("get_labels", "")) == 1100
    finally:
        _stop(p, c)


def _mix_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        H = 256
        c = LinearClassifier("AROW", {"regularization_weight": 1.0}, DatumToFvConverter(_conv(H)))
        # rank 0: L0 .. L699, rank 1: L500 .. L1099 (they share L500 .. L699)
        mine = range(0, 700) if rank == 0 else range(500, 1100)
        c.unpack({"method": "AROW", "H": H, "labels": [f"L{i}" for i in mine],
                  "counts": [0] * len(mine), "rows": b"", "W": b"", "P": b"", "weights": None})
        rng = random.Random(10 + rank)
        probe = "L10" if rank == 0 else "L1000"
        data = [(probe, {"w": "only here", "x": 1.0})]
        data += [(f"L{rng.choice(list(mine))}", {"w": f"t{rng.randrange(30)}", "x": rng.gauss(0, 1)})
                 for _ in range(60)]
        c.train(data)
        assert c.LC == 1024
        pre = c.W[:, c.labels.lookup(probe)].copy()
        c.mix(None)
        names = [n for n in c.labels.names()]
        q.put((rank, c.LC, len(c.get_labels()), names,
               c.W.copy(), c.P.copy(),
               pre, c.W[:, c.labels.lookup(probe)].copy()))
    finally:
        dist.destroy_process_group()


def test_two_rank_mix_relays_the_label_union():
    """ranks with 700 and 600 labels that share 200: one MIX leaves both with
    the 1100-label union (label capacity 2048), the same column order and
    equal tables; a column only one rank trained is halved by the mean"""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mix_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, LC, nlabels, names, W, P, pre, post in res:
        assert LC == 2048 and nlabels == 1100 and len(names) == 1100
        assert np.abs(pre).max() > 0
        np.testing.assert_allclose(post, pre * 0.5, rtol=1e-6, atol=0)
    assert res[0][3] == res[1][3] and set(res[0][3]) == {f"L{i}" for i in range(1100)}
    # the fold is T += mean - snapshot on each rank's own table: equal up to
    # the rounding of that sum, not bit by bit
    assert res[0][4].shape == (256, 2048) and np.abs(res[0][4]).max() > 0
    np.testing.assert_allclose(res[0][4], res[1][4], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res[0][5], res[1][5], rtol=1e-5, atol=1e-6)
