"""The nearest-neighbour classifiers' label table (models/nn_classifier.py) on
the host: the ``row_lab`` invariant after every operation that moves a row or
a label, batched train against one-by-one train, label ids, and the classify
paths of the CPU driver.

Invariant: for every live row ``row_lab[slot_of[rid]] ==
label_id[row_label[rid]]``, or -1 when the row has no tag; ids are distinct,
below ``next_id`` and never reused before clear() / unpack().

This module also holds what tests/test_gpu_nn_vote.py runs against the device:
the data, the invariant check, the float64 vote over fp32 top-k lists (the
oracle of csrc/hip/nn_vote.hip) and the driver cases. Ties at the k-th
neighbour would let two top-k implementations keep different rows, so every
case with k < rows is checked here, on the CPU driver, to have its k-th and
(k+1)-th distances more than 1e-4 relative apart for every query
(test_driver_cases_have_a_gap_at_the_kth_neighbour; the seeds were chosen with
that test alone); the lsh and minhash cases, whose distances are multiples of
1 / hash_num, use k >= rows.
"""
import msgpack
import numpy as np
import pytest

from test_nn_regression import CONVERTER, HASH_NUM, datum, make_data

TIE_GAP = 1e-4
NLABELS = 5
METHODS = [("NN", "euclid_lsh"), ("cosine", None), ("euclidean", None)]

# (method, inner, k, rows, seed) of the GPU driver comparison: every index
# kind; k above TOPK_MAX_K = 128 (the torch.topk branch of query_device) with
# k above the row count (lsh) and below it (euclidean, 150)
DRIVER_CASES = [("NN", "lsh", 300, 200, 81), ("NN", "minhash", 128, 100, 82),
                ("NN", "euclid_lsh", 10, 300, 83), ("cosine", None, 10, 300, 84),
                ("euclidean", None, 10, 300, 185), ("euclidean", None, 150, 300, 86)]
GROWTH_CASE = ("euclidean", None, 5, 1300, 87)          # past the first 1024 slots
NQ = 12


# -------------------------------------------------------------------- data
def converter():
    from jubatus_amd.fv_converter.converter import DatumToFvConverter
    return DatumToFvConverter(CONVERTER)


def params(method, inner, k, alpha=1.0, **extra):
    p = {"nearest_neighbor_num": k, "local_sensitivity": alpha, **extra}
    if method == "NN":
        p.update({"method": inner, "parameter": {"hash_num": HASH_NUM}})
    return p


def driver(method, parameter, device=None, prefix=None):
    from jubatus_amd.models.nn_classifier import NNClassifier
    d = NNClassifier(method, parameter, converter(), device=device)
    if prefix is not None:
        d.prefix = prefix
    return d


def make_labelled(n, nq, seed, nlabels=NLABELS):
    """n rows and nq queries, N(0,1)^6 (test_nn_regression.make_data); the
    label is the quantile bucket of the rows' linear score: "L0" .. """
    X, y, Q = make_data(n, nq, seed)
    edges = np.quantile(y, np.linspace(0, 1, nlabels + 1)[1:-1])
    labs = [f"L{int(b)}" for b in np.searchsorted(edges, y)]
    return X, labs, Q


def labelled(X, labs):
    return [(lab, datum(x)) for x, lab in zip(X, labs)]


def check_row_lab(drv):
    """the invariant of models/nn_classifier.py, on NumPy or on the device"""
    slot_of = drv.engine.rows.slot_of
    t = drv.row_lab.cpu().numpy() if hasattr(drv.row_lab, "cpu") else drv.row_lab
    assert t.dtype == np.int32 and t.ndim == 1
    assert len(t) >= max(1024, drv.engine.rows.nslots)
    for rid, s in slot_of.items():
        lab = drv.row_label.get(rid)
        assert t[s] == (-1 if lab is None else drv.label_id[lab]), (rid, s, lab)
    ids = list(drv.label_id.values())
    assert len(set(ids)) == len(ids) and all(0 <= i < drv.next_id for i in ids)
    assert set(drv.labels) <= set(drv.label_id)
    assert {lab for lab in drv.row_label.values()} <= set(drv.label_id)


# ------------------------------------------------------------------ oracle
def vote64(dist, row, row_lab, nrows, nlabels, mode, alpha):
    """the float64 oracle of csrc/hip/nn_vote.hip on [nq, k] fp32 lists ->
    (out, n, scale), each [nq, nlabels]: the votes, the kept entries and
    sum |w| per (query, label). An entry is kept iff d is finite, 0 <= row <
    nrows and 0 <= row_lab[row] < nlabels."""
    dist, row, row_lab = np.asarray(dist), np.asarray(row), np.asarray(row_lab)
    nq = dist.shape[0]
    out = np.zeros((nq, nlabels))
    cnt = np.zeros((nq, nlabels), np.int64)
    scale = np.zeros((nq, nlabels))
    for q in range(nq):
        for d, r in zip(dist[q], row[q]):
            if not np.isfinite(d) or not 0 <= r < nrows:
                continue
            lab = int(row_lab[r])
            if not 0 <= lab < nlabels:
                continue
            w = 1.0 - float(d) if mode == 1 else np.exp(-float(alpha) * float(d))
            out[q, lab] += w
            cnt[q, lab] += 1
            scale[q, lab] += abs(w)
    return out, cnt, scale


def neighbour_stats(drv, nb):
    """per label of the per-datum path's list ``nb`` [(row id, value)]: the
    float64 vote, the entries and sum |w| -> {label: (vote, n, scale)}"""
    st = {}
    for rid, v in nb:
        lab = drv.row_label.get(rid)
        if lab is None:
            continue
        w = float(v) if drv.similar else np.exp(-drv.alpha * float(v))
        s, n, a = st.get(lab, (0.0, 0, 0.0))
        st[lab] = (s + w, n + 1, a + abs(w))
    return st


def kth_gap_holds(method, inner, X, labs, Q, k):
    """on the CPU driver: the k-th and (k+1)-th neighbour distances of every
    query differ by more than TIE_GAP relative (vacuous when k >= rows)"""
    d = driver(method, params(method, inner, k))
    d.train(labelled(X, labs))
    for q in Q:
        nb = d.engine.query_datum(datum(q), k + 1, False)
        if len(nb) <= k:
            continue
        a, b = nb[k - 1][1], nb[k][1]
        if not b - a > TIE_GAP * abs(b):
            return False
    return True


def same_answers(ra, rb, tol=1e-12):
    """the same labels with the same scores, whatever the order of the labels
    and of the float64 additions behind a score"""
    return len(ra) == len(rb) and all(
        set(dict(x)) == set(dict(y)) and all(abs(dict(x)[k] - dict(y)[k]) <= tol for k in dict(x))
        for x, y in zip(ra, rb))


# ------------------------------------------------------------------- tests
@pytest.mark.parametrize("method,inner", METHODS)
def test_row_lab_invariant_with_eviction_deletion_and_slot_reuse(method, inner):
    X, labs, Q = make_labelled(40, 3, 91)
    d = driver(method, params(method, inner, 8, unlearner="lru",
                              unlearner_parameter={"max_size": 12}))
    check_row_lab(d)
    assert len(d.row_lab) == 1024 and np.all(d.row_lab == -1)
    assert d.train(labelled(X[:8], labs[:8])) == 8
    check_row_lab(d)
    assert d.train(labelled(X[8:20], labs[8:20])) == 12          # evicts the first 8
    assert len(d.engine.rows.slot_of) == 12 and d.engine.rows.nslots < 20   # slots reused
    assert set(d.row_label) == set(d.engine.rows.slot_of)
    check_row_lab(d)
    # delete a label: its rows leave, its id stays retired
    victim = d.row_label[next(iter(d.engine.rows.slot_of))]
    vid = d.label_id[victim]
    freed = [s for r, s in d.engine.rows.slot_of.items() if d.row_label[r] == victim]
    assert d.delete_label(victim) is True
    assert victim not in d.labels and d.label_id[victim] == vid
    assert all(d.row_lab[s] == -1 for s in freed)
    check_row_lab(d)
    # new training takes the freed slots, under new labels
    before = d.engine.rows.nslots
    fresh = [(f"N{i % 2}", datum(x)) for i, x in enumerate(X[20:20 + len(freed)])]
    assert d.train(fresh) == len(freed)
    assert d.engine.rows.nslots == before
    assert sorted(s for r, s in d.engine.rows.slot_of.items() if d.row_label[r][0] == "N") == \
        sorted(freed)
    assert d.label_id["N0"] != vid and d.label_id["N1"] != vid
    check_row_lab(d)
    assert d.set_label("spare") is True and d.label_id["spare"] == d.next_id - 1
    check_row_lab(d)
    res = d.classify([datum(q) for q in Q])
    assert all([lab for lab, _ in r] == list(d.labels) for r in res)
    assert all(victim != lab for r in res for lab, _ in r)
    # the victim trained again keeps its retired id
    d.train([(victim, datum(X[30]))])
    assert d.label_id[victim] == vid
    check_row_lab(d)
    d.clear()
    assert d.label_id == {} and d.next_id == 0 and len(d.row_lab) == 1024
    assert np.all(d.row_lab == -1)
    check_row_lab(d)


@pytest.mark.parametrize("method,inner", METHODS)
def test_row_lab_invariant_after_put_diff_and_unpack(method, inner):
    from jubatus_amd.models.nn_classifier import NNClassifier
    X, labs, Q = make_labelled(60, 4, 92)
    p = params(method, inner, 7)
    a, b = driver(method, p), driver(method, p)
    a.train(labelled(X[:25], labs[:25]))
    b.train(labelled(X[25:50], [f"B{lab}" for lab in labs[25:50]]))
    b.engine.set_row("untagged-0", datum(X[50]))          # a row that arrives without a tag
    db = b.get_diff()
    assert db["tags"]["untagged-0"] is None
    mixed = NNClassifier.mix_diff(a.get_diff(), db)
    assert a.put_diff(mixed) is True and b.put_diff(mixed) is True
    for drv in (a, b):
        assert len(drv.engine.rows.slot_of) == 51
        check_row_lab(drv)
        assert drv.row_lab[drv.engine.rows.slot_of["untagged-0"]] == -1
        assert set(drv.labels) == set(drv.label_id)
    # the two servers may number the labels differently; both answer the same
    qs = [datum(q) for q in Q]
    assert same_answers(a.classify(qs), b.classify(qs))
    # a removed row
    gone = f"{a.prefix}-0"
    a.engine.clear_row(gone)
    mixed = NNClassifier.mix_diff(a.get_diff(), b.get_diff())
    assert gone in mixed["rows"]["removed"]
    a.put_diff(mixed)
    b.put_diff(mixed)
    for drv in (a, b):
        assert gone not in drv.row_label and gone not in drv.engine.rows.slot_of
        check_row_lab(drv)
    # a row that takes the freed slot, then a model file into a fresh driver
    b.train(labelled(X[51:53], labs[51:53]))
    check_row_lab(b)
    obj = msgpack.unpackb(msgpack.packb(b.pack()), strict_map_key=False)
    assert set(obj) == {"method", "engine", "row_label", "labels", "seq"}
    c = driver(method, p)
    c.train(labelled(X[:3], ["old"] * 3))                 # forgotten by unpack
    c.unpack(obj)
    check_row_lab(c)
    assert "old" not in c.label_id and list(c.label_id)[:len(c.labels)] == list(c.labels)
    assert c.row_lab[c.engine.rows.slot_of["untagged-0"]] == -1
    assert [[lab for lab, _ in r] for r in c.classify(qs)] == [list(b.labels)] * len(qs)
    assert same_answers(c.classify(qs), b.classify(qs))
    assert msgpack.packb(c.pack()) == msgpack.packb(b.pack())


@pytest.mark.parametrize("unlearner", [None, "lru"])
@pytest.mark.parametrize("method,inner", METHODS + [("NN", "lsh"), ("NN", "minhash")])
def test_batch_train_equals_one_by_one(method, inner, unlearner):
    X, labs, Q = make_labelled(30, 4, 93)
    extra = {"unlearner": "lru", "unlearner_parameter": {"max_size": 20}} if unlearner else {}
    p = params(method, inner, 6, **extra)
    a, b = driver(method, p, prefix="fixed"), driver(method, p, prefix="fixed")
    assert a.train(labelled(X[:13], labs[:13])) == 13
    assert a.train(labelled(X[13:], labs[13:])) == 17
    assert a.train([]) == 0
    for ex in labelled(X, labs):
        assert b.train([ex]) == 1
    assert list(a.row_label) == [f"fixed-{i}" for i in range(10 if unlearner else 0, 30)]
    assert msgpack.packb(a.pack()) == msgpack.packb(b.pack())
    assert a.labels == b.labels and a.label_id == b.label_id and a.seq == b.seq == 30
    assert a.engine.rows.slot_of == b.engine.rows.slot_of
    assert np.array_equal(a.row_lab, b.row_lab)
    check_row_lab(a)
    qs = [datum(q) for q in Q]
    assert a.classify(qs) == b.classify(qs)


def test_cpu_classify_keeps_the_per_datum_arithmetic():
    import math
    X, labs, Q = make_labelled(50, 5, 94)
    for method, inner in METHODS:
        d = driver(method, params(method, inner, 9, 0.5))
        assert d.classify([]) == []
        assert d.classify([datum(Q[0])]) == [[]]
        d.set_label("known")
        assert d.classify([datum(q) for q in Q[:2]]) == [[("known", 0.0)]] * 2
        d.train(labelled(X, labs))
        qs = [datum(q) for q in Q]
        got = d.classify(qs)
        assert got == d._classify_each(qs)
        for q, res in zip(qs, got):
            assert [lab for lab, _ in res] == list(d.labels)
            want = {lab: 0.0 for lab in d.labels}
            for rid, v in d.engine.query_datum(q, 9, d.similar):
                want[d.row_label[rid]] += v if d.similar else math.exp(-0.5 * v)
            assert dict(res) == want
        assert d.classify([]) == []
        check_row_lab(d)


def test_a_label_the_model_file_does_not_list_takes_the_per_datum_path():
    X, labs, Q = make_labelled(20, 2, 95)
    a = driver("euclidean", params("euclidean", None, 20))
    a.train(labelled(X, labs))
    obj = msgpack.unpackb(msgpack.packb(a.pack()), strict_map_key=False)
    hidden = labs[0]
    del obj["labels"][hidden]                                   # a hand-made model file
    b = driver("euclidean", params("euclidean", None, 20))
    b.unpack(obj)
    assert b._stray is True
    check_row_lab(b)
    res = b.classify([datum(q) for q in Q])
    for r in res:
        assert [lab for lab, _ in r] == list(b.labels) + [hidden]   # the extra label, last
        assert dict(r)[hidden] > 0
    assert b.set_label(hidden) is True and b._stray is False
    a.unpack(msgpack.unpackb(msgpack.packb(a.pack()), strict_map_key=False))
    assert a._stray is False


@pytest.mark.parametrize("method,inner,k,n,seed", DRIVER_CASES + [GROWTH_CASE])
def test_driver_cases_have_a_gap_at_the_kth_neighbour(method, inner, k, n, seed):
    X, labs, Q = make_labelled(n, NQ, seed)
    if inner in ("lsh", "minhash"):
        assert k >= n
    assert kth_gap_holds(method, inner, X, labs, Q, k)


def test_vote64_on_a_hand_made_list():
    dist = np.asarray([[0.0, 0.5, np.inf, np.nan, 1.5, 0.25]], np.float32)
    row = np.asarray([[0, 1, 2 ** 31 - 1, 0, 2, 3]], np.int32)
    row_lab = np.asarray([1, 1, 0, -1], np.int32)
    out, n, scale = vote64(dist, row, row_lab, 4, 2, 1, 1.0)
    assert out.tolist() == [[-0.5, 1.5]] and n.tolist() == [[1, 2]] and scale.tolist() == [[0.5, 1.5]]
    out, n, _ = vote64(dist, row, row_lab, 2, 2, 0, 0.0)      # rows 2 and 3 are out of range
    assert out.tolist() == [[0.0, 2.0]] and n.tolist() == [[0, 2]]
