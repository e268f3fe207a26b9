"""Nearest-neighbor classifiers: NN (LSH family), cosine, euclidean.

Reference: classifier configs config/classifier/{nn,cosine,euclidean}.json
(jubatus/server/server/classifier_serv.cpp:91-117 builds jubatus_core's
nearest_neighbor_classifier / inverted-index classifiers, EXTERNAL).
Parameters: ``nearest_neighbor_num`` (k), ``local_sensitivity`` (alpha),
for NN also ``method`` (lsh / euclid_lsh / minhash) + ``parameter``
(hash_num), optional ``unlearner`` / ``unlearner_parameter``.

Training stores each example as a row (id = "<prefix>-<seq>", a per-server
sequence) tagged with its label, one bulk row write per train call;
classification takes the k nearest rows on the row engine (GPU XOR-popcount /
sparse scan kernels, models/similarity.py) and scores each label by
sum exp(-alpha * distance) over its neighbours (NN, euclidean) or by the
summed cosine similarity (cosine). Every known label is reported (0 when no
neighbour carries it). MIX: the versioned rows (row engine) plus label counts.

Storage: ``row_label`` {row id: label} on the host (model files, MIX);
``label_id`` {label: int}, an id given when a label is first seen (train,
set_label, put_diff, unpack) and never reused before clear() or unpack(), so
a deleted label's id stays retired; and ``row_lab``, int32 indexed by the
row's slot (NumPy, or a tensor in HBM that grows with the engine's capacity).
For every live row ``row_lab[slot_of[rid]] == label_id[row_label[rid]]``, or
-1 when the row has no tag, after train, unlearner eviction and slot reuse,
delete_label, put_diff, unpack and clear; it is kept with one scatter per
batch.

classify has two paths. On a GPU the batch is converted once, the device
top-k is taken once (once per inverted-index batch; models/similarity.py
query_device), csrc/hip/nn_vote.hip votes the [nq, k] lists into
[nq, ids] label columns through ``row_lab`` and one copy brings them back.
The per-datum path (``_classify_each``: engine.query_datum and a host
``_score`` per datum) serves the CPU driver, a single datum on the LSH
indexes (measured faster there: profiles/nn_classifier_classify.md), and the
GPU driver when a live row carries a label that ``labels`` does not know (a
hand-made model file: that label is reported after the known ones).
"""
from __future__ import annotations

import math
import threading
import uuid
from typing import Any, Sequence

import numpy as np

from ..fv_converter.converter import DatumToFvConverter
from ..fv_converter.datum import as_datum
from .row_engine import LSH_METHODS, RowEngine

MODE_DISTANCE, MODE_SIMILARITY = 0, 1      # csrc/hip/nn_vote.hip
_MIN_CAP = 1024


class NNClassifier:
    def __init__(self, method: str, parameter: dict, converter: DatumToFvConverter, device: Any = None):
        p = dict(parameter or {})
        self.method = method
        self.k = int(p.get("nearest_neighbor_num", 128))
        self.alpha = float(p.get("local_sensitivity", 1.0))
        if self.k <= 0 or self.alpha < 0:
            raise ValueError("nearest_neighbor_num must be positive, local_sensitivity >= 0")
        if method in ("NN", "nearest_neighbor"):
            idx_method = p.get("method", "lsh")
            if idx_method not in LSH_METHODS:
                raise ValueError(f"unknown nearest neighbor method: {idx_method}")
            idx_param = p.get("parameter") or {}
            self.similar = False
            # one datum: the LSH indexes' single-launch query into pinned host
            # memory is ahead of the fused path (profiles/nn_classifier_classify.md)
            self._each_for_one = True
        elif method == "cosine":
            idx_method, idx_param, self.similar = "inverted_index", {}, True
        elif method == "euclidean":
            idx_method, idx_param, self.similar = "inverted_index_euclid", {}, False
        else:
            raise ValueError(f"unsupported nn classifier method: {method}")
        if idx_method not in LSH_METHODS:
            self._each_for_one = False
        self.engine = RowEngine(idx_method, idx_param, converter, device,
                                p.get("unlearner"), p.get("unlearner_parameter"))
        self.device = device
        self.on_device = device is not None
        if self.on_device:
            import torch
            self.torch = torch
        self.mode = MODE_SIMILARITY if self.similar else MODE_DISTANCE
        self.prefix = uuid.uuid4().hex[:8]
        self._lock = threading.RLock()
        self.clear()

    def clear(self) -> None:
        with self._lock:
            self.engine.clear()
            self.row_label: dict[str, str] = {}
            self.labels: dict[str, int] = {}
            self.seq = 0
            self._reset_ids()

    # ------------------------------------------------------------- row_lab
    def _reset_ids(self) -> None:
        self.label_id: dict[str, int] = {}
        self.next_id = 0
        self.row_lab = self._unlabelled(_MIN_CAP)
        self._stray = False     # a live row's label is missing from self.labels

    def _id(self, label: str) -> int:
        i = self.label_id.get(label)
        if i is None:
            i = self.label_id[label] = self.next_id
            self.next_id += 1
        return i

    def _unlabelled(self, n: int):
        if self.on_device:
            return self.torch.full((n,), -1, dtype=self.torch.int32, device=self.device)
        return np.full(n, -1, dtype=np.int32)

    def _write(self, slots: np.ndarray, ids: np.ndarray) -> None:
        """row_lab[slots] = ids (one device scatter); the table grows with
        the engine"""
        need = self.engine.rows.nslots
        cap = len(self.row_lab)
        if need > cap:
            while cap < need:
                cap *= 2
            grown = self._unlabelled(cap)
            grown[:len(self.row_lab)] = self.row_lab
            self.row_lab = grown
        if not slots.size:
            return
        if self.on_device:
            t = self.torch
            self.row_lab.index_copy_(0, t.from_numpy(slots).to(self.device),
                                     t.from_numpy(ids).to(self.device))
        else:
            self.row_lab[slots] = ids

    def _scatter(self, rids) -> None:
        """row_lab[slot_of[rid]] = the id of row_label[rid] (-1 without a tag)
        for the live rows among ``rids``"""
        slot_of = self.engine.rows.slot_of
        live = list(dict.fromkeys(r for r in rids if r in slot_of))
        slots = np.fromiter((slot_of[r] for r in live), np.int64, len(live))
        tags = (self.row_label.get(r) for r in live)
        ids = np.fromiter((-1 if lab is None else self._id(lab) for lab in tags), np.int32,
                          len(live))
        self._write(slots, ids)

    def _find_stray(self) -> None:
        labels = self.labels
        self._stray = any(lab not in labels for lab in set(self.row_label.values()))

    # --------------------------------------------------------------- train
    def train(self, data: Sequence[tuple[str, Any]]) -> int:
        items = [(label, as_datum(d)) for label, d in data]
        with self._lock:
            rows = []
            for label, d in items:
                rid = f"{self.prefix}-{self.seq}"
                self.seq += 1
                rows.append((rid, d))
                self.row_label[rid] = label
                self.labels[label] = self.labels.get(label, 0) + 1
                self._id(label)
            if rows:
                self.engine.set_rows(rows)
            self._gc()
            self._scatter([rid for rid, _ in rows])
            if self._stray:
                self._find_stray()
            return len(items)

    def _gc(self) -> None:
        """drop labels of rows the unlearner evicted"""
        if self.engine.unlearner.kind:
            live = self.engine.rows.slot_of
            for rid in [r for r in self.row_label if r not in live]:
                del self.row_label[rid]

    def _score(self, neighbors: list[tuple[str, float]]) -> dict[str, float]:
        sc = {lab: 0.0 for lab in self.labels}
        for rid, v in neighbors:
            lab = self.row_label.get(rid)
            if lab is None:
                continue
            sc[lab] = sc.get(lab, 0.0) + (v if self.similar else math.exp(-self.alpha * v))
        return sc

    # ------------------------------------------------------------ classify
    def _classify_each(self, data: Sequence[Any]) -> list[list[tuple[str, float]]]:
        """the per-datum path: one query and one host vote per datum"""
        with self._lock:
            out = []
            for d in data:
                nb = self.engine.query_datum(as_datum(d), self.k, self.similar)
                out.append(list(self._score(nb).items()))
            return out

    def _classify_fused(self, ds: list) -> list[list[tuple[str, float]]]:
        """the device path: one conversion, one device top-k, one vote kernel
        and one copy of [nq, ids] for the whole batch"""
        labels = list(self.labels)
        n = self.engine.rows.nslots
        if n == 0 or not self.engine.rows.slot_of or not labels:
            return [[(lab, 0.0) for lab in labels] for _ in ds]
        from ..ops import hip
        dist, row = self.engine.index.query_device(self.engine.fvs_of(ds), n, self.k)
        out = hip.nn_vote(dist, row, len(ds), int(dist.shape[1]), self.row_lab, n, self.next_id,
                          self.mode, self.alpha)
        cols = [self.label_id[lab] for lab in labels]       # retired ids are not reported
        votes = out.cpu().numpy()[:, cols].astype(np.float64).tolist()
        return [list(zip(labels, v)) for v in votes]

    def classify(self, data: Sequence[Any]) -> list[list[tuple[str, float]]]:
        ds = [as_datum(d) for d in data]
        if not ds:
            return []
        with self._lock:
            if self.on_device and not self._stray and not (len(ds) == 1 and self._each_for_one):
                return self._classify_fused(ds)
            return self._classify_each(ds)

    # -------------------------------------------------------------- labels
    def get_labels(self) -> dict[str, int]:
        with self._lock:
            return dict(self.labels)

    def set_label(self, label: str) -> bool:
        with self._lock:
            if label in self.labels:
                return False
            self.labels[label] = 0
            self._id(label)
            if self._stray:
                self._find_stray()
            return True

    def delete_label(self, label: str) -> bool:
        with self._lock:
            if label not in self.labels:
                return False
            slot_of = self.engine.rows.slot_of
            gone = [r for r, lab in self.row_label.items() if lab == label]
            slots = np.asarray([slot_of[r] for r in gone if r in slot_of], np.int64)
            for rid in gone:
                self.engine.clear_row(rid)
                del self.row_label[rid]
            del self.labels[label]
            self._write(slots, np.full(slots.size, -1, np.int32))
            return True

    # ----------------------------------------------------------------- MIX
    def get_diff(self) -> dict:
        with self._lock:
            rows = self.engine.get_diff()
            tagged = {rid: self.row_label.get(rid) for rid in rows["rows"]}
            return {"rows": rows, "tags": tagged, "labels": dict(self.labels)}

    @staticmethod
    def mix_diff(a: dict, b: dict) -> dict:
        tags = dict(a["tags"])
        tags.update(b["tags"])
        labels = dict(a["labels"])
        for k, v in b["labels"].items():
            labels[k] = max(labels.get(k, 0), v)
        return {"rows": RowEngine.mix_diff(a["rows"], b["rows"]), "tags": tags, "labels": labels}

    def put_diff(self, mixed: dict) -> bool:
        with self._lock:
            self.engine.put_diff(mixed["rows"])
            for rid, lab in mixed["tags"].items():
                if lab is not None:
                    self.row_label[rid] = lab
            for rid in mixed["rows"]["removed"]:
                self.row_label.pop(rid, None)
            counts: dict[str, int] = {lab: 0 for lab in mixed["labels"]}
            counts.update({lab: 0 for lab in self.labels})
            for lab in self.row_label.values():
                counts[lab] = counts.get(lab, 0) + 1
            self.labels = counts
            for lab in counts:
                self._id(lab)
            self._scatter(list(mixed["rows"]["rows"]) + list(mixed["tags"]))
            self._stray = False             # every tag was just counted into labels
            return True

    def pack(self) -> dict:
        with self._lock:
            return {"method": self.method, "engine": self.engine.pack(), "row_label": self.row_label,
                    "labels": self.labels, "seq": self.seq}

    def unpack(self, obj: dict) -> None:
        with self._lock:
            self.engine.unpack(obj["engine"])
            self.row_label = dict(obj["row_label"])
            self.labels = {k: int(v) for k, v in obj["labels"].items()}
            self.seq = int(obj["seq"])
            self._reset_ids()
            for lab in self.labels:
                self._id(lab)
            self._scatter(list(self.engine.rows.slot_of))
            self._find_stray()

    def get_status(self) -> dict[str, str]:
        st = {"method": self.method, "num_labels": str(len(self.labels)),
              "nearest_neighbor_num": str(self.k), "local_sensitivity": str(self.alpha)}
        st.update({f"nn.{k}": v for k, v in self.engine.get_status().items()})
        return st
