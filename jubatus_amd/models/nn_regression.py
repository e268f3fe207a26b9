"""Nearest-neighbour regression: ``method`` NN (LSH family), cosine or
euclidean.

The reference (Jubatus 0.9.2) ships PA regression only. These three methods
are defined by this project, after the nearest-neighbour classifier
(models/nn_classifier.py); the float64 brute force in
tests/test_nn_regression.py is the oracle, and parity with later Jubatus
releases is unpinned.

Parameters: ``nearest_neighbor_num`` (k, an int > 0, default 128), ``weight``
("uniform", the default, or "distance"), ``local_sensitivity`` (alpha >= 0,
default 1.0, read with ``weight: distance`` only); for NN also ``method`` (lsh
/ euclid_lsh / minhash, default lsh) and ``parameter`` (hash_num); optional
``unlearner`` / ``unlearner_parameter``. cosine runs on ``inverted_index``,
euclidean on ``inverted_index_euclid``.

train stores each example as the row "<prefix>-<seq>" of a RowEngine and its
score as the row's target. estimate takes, per datum, the k nearest live rows
with the distance d_j the top-k reports (the lsh / minhash fraction, the
euclid_lsh or euclid distance, 1 - cosine) and the targets t_j:
    uniform                        w_j = 1
    distance, NN and euclidean     w_j = exp(-alpha (d_j - d_min)), d_min the
                                   smallest d_j of the query: the nearest row
                                   weighs 1, whatever alpha
    distance, cosine               w_j = max(0, 1 - d_j)
    estimate = sum w_j t_j / sum w_j    (0.0 without a neighbour or when
                                         sum w_j == 0)

Storage: ``row_target`` {row id: target} on the host (model files, MIX) and
``targets``, fp32 indexed by the row's slot (NumPy, or a tensor in HBM that
grows with the engine's capacity). For every live row
``targets[slot_of[rid]] == row_target[rid]``, after train, unlearner eviction
and slot reuse, put_diff, unpack and clear.

On a GPU estimate converts the whole batch, takes the device top-k once
(once per inverted-index batch; models/similarity.py query_device), reduces
with csrc/hip/nn_reduce.hip and copies nq floats back. Without one it
reduces engine.query_datum's lists in NumPy fp32.

MIX: {"rows": the row engine's diff, "targets": {rid: y}}.
"""
from __future__ import annotations

import threading
import uuid
from typing import Any, Sequence

import numpy as np

from ..common.exceptions import ArgumentError
from ..fv_converter.converter import DatumToFvConverter
from ..fv_converter.datum import as_datum
from .regression import RegressionConfigError
from .row_engine import LSH_METHODS, RowEngine

NN_METHODS = ("NN", "cosine", "euclidean")
WEIGHTS = ("uniform", "distance")
MODE_UNIFORM, MODE_DISTANCE, MODE_SIMILARITY = 0, 1, 2     # csrc/hip/nn_reduce.hip
_MIN_CAP = 1024


def reduce_host(d: np.ndarray, t: np.ndarray, mode: int, alpha: float) -> float:
    """the estimate of one query from its neighbours' distances and targets,
    in NumPy fp32 (the --cpu backend; twin of csrc/hip/nn_reduce.hip)"""
    d = np.asarray(d, np.float32)
    t = np.asarray(t, np.float32)
    keep = np.isfinite(d)
    d, t = d[keep], t[keep]
    if d.size == 0:
        return 0.0
    if mode == MODE_DISTANCE:
        w = np.exp(-np.float32(alpha) * (d - d.min())).astype(np.float32)
    elif mode == MODE_SIMILARITY:
        w = np.maximum(np.float32(0), np.float32(1) - d)
    else:
        w = np.ones_like(d)
    sw = w.sum(dtype=np.float32)
    if not sw > 0:
        return 0.0
    return float((w * t).sum(dtype=np.float32) / sw)


class NNRegression:
    def __init__(self, method: str, parameter: dict | None, converter: DatumToFvConverter,
                 device: Any = None):
        if method not in NN_METHODS:
            raise RegressionConfigError(f"unsupported regression method: {method}")
        p = dict(parameter or {})
        k = p.get("nearest_neighbor_num", 128)
        if isinstance(k, bool) or not isinstance(k, int) or k <= 0:
            raise RegressionConfigError("nearest_neighbor_num must be an integer > 0")
        alpha = p.get("local_sensitivity", 1.0)
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or \
                not 0 <= alpha < float("inf"):
            raise RegressionConfigError("local_sensitivity must be a number >= 0")
        weight = p.get("weight", "uniform")
        if weight not in WEIGHTS:
            raise RegressionConfigError(f"unknown weight: {weight!r} (uniform or distance)")
        if method == "NN":
            idx_method = p.get("method", "lsh")
            if idx_method not in LSH_METHODS:
                raise RegressionConfigError(f"unknown nearest neighbor method: {idx_method}")
            idx_param = p.get("parameter") or {}
        elif method == "cosine":
            idx_method, idx_param = "inverted_index", {}
        else:
            idx_method, idx_param = "inverted_index_euclid", {}
        self.method, self.k, self.alpha, self.weight = method, k, float(alpha), weight
        if weight == "uniform":
            self.mode = MODE_UNIFORM
        else:
            self.mode = MODE_SIMILARITY if method == "cosine" else MODE_DISTANCE
        try:
            self.engine = RowEngine(idx_method, idx_param, converter, device,
                                    p.get("unlearner"), p.get("unlearner_parameter"))
        except (ValueError, TypeError) as e:
            raise RegressionConfigError(str(e)) from e
        self.device = device
        self.gpu = device is not None
        if self.gpu:
            import torch
            self.torch = torch
        self.prefix = uuid.uuid4().hex[:8]
        self._lock = threading.RLock()
        self.clear()

    def clear(self) -> None:
        with self._lock:
            self.engine.clear()
            self.row_target: dict[str, float] = {}
            self.seq = 0
            self.targets = self._zeros(_MIN_CAP)

    # ------------------------------------------------------------- targets
    def _zeros(self, n: int):
        if self.gpu:
            return self.torch.zeros(n, dtype=self.torch.float32, device=self.device)
        return np.zeros(n, dtype=np.float32)

    def _scatter(self, rids) -> None:
        """targets[slot_of[rid]] = row_target[rid] for the live rows among
        ``rids`` (one device scatter); the table grows with the engine"""
        slot_of = self.engine.rows.slot_of
        live = [r for r in rids if r in slot_of and r in self.row_target]
        need = self.engine.rows.nslots
        cap = len(self.targets)
        if need > cap:
            while cap < need:
                cap *= 2
            grown = self._zeros(cap)
            grown[:len(self.targets)] = self.targets
            self.targets = grown
        if not live:
            return
        slots = np.fromiter((slot_of[r] for r in live), np.int64, len(live))
        vals = np.fromiter((self.row_target[r] for r in live), np.float32, len(live))
        if self.gpu:
            t = self.torch
            self.targets.index_copy_(0, t.from_numpy(slots).to(self.device),
                                     t.from_numpy(vals).to(self.device))
        else:
            self.targets[slots] = vals

    def _gc(self) -> None:
        """drop the targets of rows that are gone (unlearner, MIX removals)"""
        slot_of = self.engine.rows.slot_of
        if len(self.row_target) != len(slot_of):
            for rid in [r for r in self.row_target if r not in slot_of]:
                del self.row_target[rid]

    # --------------------------------------------------------------- train
    def train(self, data: Sequence) -> int:
        data = list(data)
        if not data:
            return 0
        items = []
        for it in data:
            if not isinstance(it, (list, tuple)) or len(it) != 2:
                raise ArgumentError("scored_datum must be [score, datum]")
            score, d = it
            if isinstance(score, bool) or not isinstance(score, (int, float)):
                raise ArgumentError("score must be a number")
            items.append((float(score), as_datum(d)))
        with self._lock:
            rows = []
            for score, d in items:
                rid = f"{self.prefix}-{self.seq}"
                self.seq += 1
                rows.append((rid, d))
                self.row_target[rid] = score
            self.engine.set_rows(rows)
            self._gc()
            self._scatter([rid for rid, _ in rows])
        return len(items)

    # ------------------------------------------------------------ estimate
    def estimate(self, data: Sequence) -> list[float]:
        ds = [as_datum(d) for d in data]
        if not ds:
            return []
        with self._lock:
            n = self.engine.rows.nslots
            if n == 0 or not self.engine.rows.slot_of:
                return [0.0] * len(ds)
            if self.gpu:
                from ..ops import hip
                dist, row = self.engine.index.query_device(self.engine.fvs_of(ds), n, self.k)
                out, _ = hip.nn_reduce(dist, row, len(ds), int(dist.shape[1]), self.targets, n,
                                       self.mode, self.alpha)
                res = out.cpu().tolist()
                return [float(x) for x in res]
            slot_of = self.engine.rows.slot_of
            res = []
            for d in ds:
                nb = [(slot_of[rid], v) for rid, v in self.engine.query_datum(d, self.k, False)
                      if rid in slot_of]
                res.append(reduce_host(np.asarray([v for _, v in nb], np.float32),
                                       self.targets[[s for s, _ in nb]], self.mode, self.alpha))
            return res

    # ----------------------------------------------------------------- MIX
    def get_diff(self) -> dict:
        with self._lock:
            rows = self.engine.get_diff()
            return {"rows": rows, "targets": {rid: self.row_target[rid] for rid in rows["rows"]
                                              if rid in self.row_target}}

    @staticmethod
    def mix_diff(a: dict, b: dict) -> dict:
        targets = dict(a["targets"])
        targets.update(b["targets"])
        return {"rows": RowEngine.mix_diff(a["rows"], b["rows"]), "targets": targets}

    def put_diff(self, mixed: dict) -> bool:
        with self._lock:
            self.engine.put_diff(mixed["rows"])
            slot_of = self.engine.rows.slot_of
            for rid, y in mixed["targets"].items():
                if rid in slot_of:
                    self.row_target[rid] = float(y)
            for rid in mixed["rows"]["removed"]:
                if rid not in slot_of:
                    self.row_target.pop(rid, None)
            self._gc()
            self._scatter(list(mixed["targets"]))
            return True

    # ------------------------------------------------------------- persist
    def pack(self) -> dict:
        with self._lock:
            return {"method": self.method, "engine": self.engine.pack(),
                    "row_target": dict(self.row_target), "seq": self.seq}

    def unpack(self, obj: dict) -> None:
        with self._lock:
            if obj.get("method", self.method) != self.method:
                raise ValueError(f"model method {obj.get('method')} differs from the configured "
                                 f"{self.method}")
            if "row_target" not in obj or "engine" not in obj:
                raise ValueError("not a nearest-neighbour regression model")
            self.engine.unpack(obj["engine"])
            slot_of = self.engine.rows.slot_of
            self.row_target = {rid: float(y) for rid, y in obj["row_target"].items()
                               if rid in slot_of}
            self.seq = int(obj["seq"])
            self.targets = self._zeros(_MIN_CAP)
            self._scatter(list(self.row_target))

    def get_status(self) -> dict[str, str]:
        st = {"method": self.method, "nearest_neighbor_num": str(self.k), "weight": self.weight,
              "local_sensitivity": str(self.alpha), "num_targets": str(len(self.row_target))}
        st.update({f"nn.{k}": v for k, v in self.engine.get_status().items()})
        return st
