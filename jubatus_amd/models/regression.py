"""Online regression driver: ``method`` PA, PA1, PA2, perceptron, CW, AROW or
NHERD.

Reference surface: jubatus/server/server/regression_serv.cpp:95-156 (train,
estimate, clear) over jubatus_core's PA regression (EXTERNAL). Parameters:
``sensitivity`` (epsilon of the insensitive loss, scaled by the running
target standard deviation, >= 0, default 0.1), ``regularization_weight``
(C > 0; default 3.40282e38 for PA / PA1 / PA2, required for CW / AROW /
NHERD) and ``learning_rate`` (> 0, default 1.0, perceptron only).

The reference (Jubatus 0.9.2) ships PA regression only. The other six rules
are defined by this project: the classifier's formulas (linear_oracle.py)
with one label, no rival label, and ``1 - margin`` replaced by ``loss``. The
oracle is our own; parity with later Jubatus releases is unpinned.

Rule (also the numerical oracle of csrc/hip/regression.hip):
    count, sum, sum2 of the targets; sd = sqrt(max(0, sum2/count - (sum/count)^2))
    err = y - w.x ; sgn = sign(err) ; loss = |err| - sensitivity * sd
    S = 1/P (P: diagonal precision, initial value 1, stored as
    linear_oracle.py stores it) ; v = sum x_i^2 S_i
    PA          loss > 0, ||x||^2 > 0:  w += sgn * min(C, loss) / ||x||^2 * x
    PA1         same:  tau = min(C, loss / ||x||^2) ;  w += sgn tau x
    PA2         same:  tau = loss / (||x||^2 + 1/(2C))
    perceptron  same:  tau = learning_rate
    AROW        same:  beta = 1 / (v + 1/C), alpha = loss beta ;
                w += sgn alpha S x ;  P += beta x^2 / (1 - beta S x^2)
    NHERD       same:  alpha = loss / (v + 1/C) ;  w as AROW ;
                beta = (C^2 v + 2C) / (1 + C v)^2 ;  P as AROW
    CW          v > 0 and gamma > 0:  m = -loss, phi = C, b = 1 + 2 phi m,
                gamma = (-b + sqrt(max(0, b^2 - 8 phi (m - phi v)))) / (4 phi v) ;
                w += sgn gamma S x ;  P += 2 gamma phi x^2
    a sample reads w and P as they were before it and then adds its
    increments; an index repeated inside a sample counts once per occurrence,
    in w.x, in ||x||^2, in v and in the update, on w and on P, and every
    occurrence's increment is computed from the pre-sample P
    estimate = w.x for every method

Storage: w[H] (hashed features), and P[H] for CW / AROW / NHERD, in HBM on a
GPU, NumPy otherwise.
MIX: all-reduce mean of w, of the precisions P (as the classifier mixes) and
of the target statistics.

Several requests submitted together (``train_requests``) on a GPU:
``concurrent_update="atomic"`` (the default) trains every request as its own
stream with float atomics, so with sensitivity > 0 the model depends on launch
timing; ``"exact"`` leaves the model as if the requests had been applied one
after the other (the reference under its model lock), by one launch of
csrc/hip/regression_ordered.hip over the requests laid out back to back. One
request, and the host backend, are sequential in either mode.
"""
from __future__ import annotations

import math
import threading
from typing import Any, Sequence

import msgpack
import numpy as np

from ..common.exceptions import ArgumentError
from ..fv_converter.converter import DatumToFvConverter
from ..fv_converter.datum import as_datum


class RegressionConfigError(ValueError):
    pass


METHODS = ("PA", "PA1", "PA2", "perceptron", "CW", "AROW", "NHERD")
UPDATE_MODES = ("atomic", "exact")
COVARIANCE_METHODS = ("CW", "AROW", "NHERD")


def train_one(w: np.ndarray, stats: np.ndarray, idx, val, y: float, C: float, eps: float,
              method: str = "PA", P: np.ndarray | None = None) -> None:
    """one online update in NumPy fp32 (the host oracle and the --cpu backend).
    C is the learning rate for perceptron; P is the precision table of CW /
    AROW / NHERD."""
    if method != "PA":
        return _train_one_m(w, P, stats, idx, val, y, C, eps, method)
    m = np.asarray(idx) >= 0
    idx = np.asarray(idx, np.int64)[m]
    x = np.asarray(val, np.float32)[m]
    dot = float((x * w[idx]).sum(dtype=np.float32)) if len(idx) else 0.0
    stats[0] += y
    stats[1] += y * y
    stats[2] += 1.0
    avg = stats[0] / stats[2]
    sd = math.sqrt(max(0.0, stats[1] / stats[2] - avg * avg))
    err = y - dot
    sgn = 1.0 if err > 0 else -1.0
    loss = sgn * err - eps * sd
    nrm = float((x * x).sum())
    if loss > 0 and nrm > 0:
        coeff = sgn * min(C, loss) / nrm
        # per occurrence: an index repeated inside the sample takes every increment
        np.add.at(w, idx, np.float32(coeff) * x)


def _train_one_m(w, P, stats, idx, val, y, C, eps, method) -> None:
    """PA1 / PA2 / perceptron / CW / AROW / NHERD (module docstring)"""
    if method not in METHODS:
        raise ValueError(f"unknown regression method {method}")
    cov = method in COVARIANCE_METHODS
    m = np.asarray(idx) >= 0
    idx = np.asarray(idx, np.int64)[m]
    x = np.asarray(val, np.float32)[m]
    dot = float((x * w[idx]).sum(dtype=np.float32)) if len(idx) else 0.0
    stats[0] += y
    stats[1] += y * y
    stats[2] += 1.0
    avg = stats[0] / stats[2]
    sd = math.sqrt(max(0.0, stats[1] / stats[2] - avg * avg))
    err = y - dot
    sgn = 1.0 if err > 0 else -1.0
    loss = sgn * err - eps * sd
    nrm = float((x * x).sum())
    a = (np.float32(1.0) / P[idx]).astype(np.float32) if cov else None   # the pre-sample S
    var = float((x * x * a).sum()) if cov else 0.0
    beta = 0.0
    if method == "CW":
        if not var > 0:
            return
        mm, phi = -loss, C
        b = 1.0 + 2.0 * phi * mm
        tau = (-b + math.sqrt(max(0.0, b * b - 8.0 * phi * (mm - phi * var)))) / (4.0 * phi * var)
        if not tau > 0:
            return
        beta = 2.0 * tau * phi
    elif not (loss > 0 and nrm > 0):
        return
    elif method == "PA1":
        tau = min(C, loss / nrm)
    elif method == "PA2":
        tau = loss / (nrm + 0.5 / C)
    elif method == "perceptron":
        tau = C
    elif method == "AROW":
        beta = 1.0 / (var + 1.0 / C)
        tau = loss * beta
    else:
        tau = loss / (var + 1.0 / C)
        cv = 1.0 + C * var
        beta = (C * C * var + 2.0 * C) / (cv * cv)
    # per occurrence, on w and on P, every increment from the pre-sample P
    if not cov:
        np.add.at(w, idx, np.float32(sgn * tau) * x)
        return
    np.add.at(w, idx, (np.float32(sgn * tau) * a * x).astype(np.float32))
    bx2 = np.float32(beta) * x * x
    dp = bx2 if method == "CW" else bx2 / (np.float32(1.0) - bx2 * a)
    np.add.at(P, idx, dp.astype(np.float32))


class Regression:
    def __init__(self, method: str, parameter: dict | None, converter: DatumToFvConverter,
                 device: Any = None, concurrent_update: str = "atomic"):
        if method not in METHODS:
            raise RegressionConfigError(f"unsupported regression method: {method}")
        if concurrent_update not in UPDATE_MODES:
            raise RegressionConfigError("concurrent_update must be 'atomic' or 'exact'")
        self.concurrent_update = concurrent_update
        self._pending: list = []        # status words of ordered launches not checked yet
        p = dict(parameter or {})
        self.cov = method in COVARIANCE_METHODS
        self.eps = float(p.get("sensitivity", 0.1))
        if self.cov and "regularization_weight" not in p:
            raise RegressionConfigError(f"{method} requires parameter regularization_weight")
        self.C = float(p.get("regularization_weight", 3.40282e+38))
        if self.eps < 0 or not self.C > 0:
            raise RegressionConfigError("sensitivity must be >= 0 and regularization_weight > 0")
        if method == "perceptron":
            self.C = float(p.get("learning_rate", 1.0))     # the step of the rule
            if not self.C > 0:
                raise RegressionConfigError("learning_rate must be > 0")
        self.method = method
        self.conv = converter
        self.H = converter.hash_max_size
        self.device = device
        self.gpu = device is not None
        self._lock = threading.RLock()
        if self.gpu:
            import torch
            from ..ops.feature_pipeline import FeaturePipeline
            self.torch = torch
            self.pipe = FeaturePipeline(converter, device)
        self.clear()

    def clear(self) -> None:
        with self._lock:
            self._check_ordered()
            if self.gpu:
                t = self.torch
                self.w = t.zeros(self.H, dtype=t.float32, device=self.device)
                self.stats = t.zeros(3, dtype=t.float32, device=self.device)
                self.P = t.ones(self.H, dtype=t.float32, device=self.device) if self.cov else None
            else:
                self.w = np.zeros(self.H, dtype=np.float32)
                self.stats = np.zeros(3, dtype=np.float64)
                self.P = np.ones(self.H, dtype=np.float32) if self.cov else None
            self.conv.weights.clear()

    # -------------------------------------------------------------- train
    def train_requests(self, bodies: Sequence[Any]) -> int:
        """raw msgpack list<scored_datum> bodies, one update stream each"""
        with self._lock:
            if self.gpu and self.pipe.fast:
                b = self.pipe.from_requests(list(bodies), 2)
                if b.n:
                    self._launch(b, b.labels.view(self.torch.float32), b.stream_ptr, b.nstreams)
                return b.n
        n = 0
        for body in bodies:
            n += self.train(msgpack.unpackb(bytes(body), raw=False))
        return n

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
        if self.gpu and self.pipe.fast:
            body = msgpack.packb([[s, d.to_msgpack()] for s, d in items], use_bin_type=False)
            return self.train_requests([body])
        with self._lock:
            rows = [self.conv.hashed(self.conv.convert_and_update_weight(d)) for _, d in items]
            if self.gpu:
                b = self.pipe.from_rows(rows, None)
                tg =self.torch.tensor([s for s, _ in items], dtype=self.torch.float32,
                                       device=self.device)
                self._launch(b, tg, b.stream_ptr, 1)
            else:
                for (s, _), (idx, val) in zip(items, rows):
                    train_one(self.w, self.stats, idx, val, s, self.C, self.eps, self.method, self.P)
        return len(items)

    def _check_ordered(self) -> None:
        """the status words of the ordered launches since the last check (a
        device synchronisation when there are any); a launch that stopped
        early raises here, on the first synchronising call behind it"""
        if self._pending:
            from ..ops import hip
            pending, self._pending = self._pending, []
            for st in pending:
                hip.regression_ordered_check(st)

    def _launch(self, b, targets, stream_ptr, nstreams: int) -> None:
        from ..ops import hip
        if nstreams > 1 and self.concurrent_update == "exact":
            # the requests lie back to back in request order: sample order is the serial order
            scratch = self.torch.empty_like(b.fval) if self.cov else None
            self._pending.append(hip.regression_train_ordered(
                b.row_ptr, b.fidx, b.fval, targets, b.n, self.w, self.stats, self.C, self.eps,
                method=self.method, P=self.P, slot_scratch=scratch))
            if len(self._pending) >= 64:
                self._check_ordered()
            return
        if self.method == "PA":
            hip.regression_train(b.row_ptr, b.fidx, b.fval, targets, stream_ptr, nstreams, self.w,
                                 self.stats, self.C, self.eps, concurrent=nstreams > 1)
            return
        # the parking place of the P increments of samples past the kernel's register slots
        scratch = self.torch.empty_like(b.fval) if self.cov else None
        hip.regression_train(b.row_ptr, b.fidx, b.fval, targets, stream_ptr, nstreams, self.w,
                             self.stats, self.C, self.eps, concurrent=nstreams > 1,
                             method=self.method, P=self.P, slot_scratch=scratch)

    # ----------------------------------------------------------- estimate
    def estimate(self, data: Sequence) -> list[float]:
        ds = [as_datum(d) for d in data]
        if not ds:
            return []
        rows = [self.conv.hashed(self.conv.convert(d)) for d in ds]
        with self._lock:
            self._check_ordered()
            if self.gpu:
                from ..ops import hip
                b = self.pipe.from_rows(rows, None)
                out = self.torch.empty(len(ds), dtype=self.torch.float32, device=self.device)
                hip.regression_estimate(b.row_ptr, b.fidx, b.fval, b.n, self.w, out)
                return [float(x) for x in out.cpu().tolist()]
            res = []
            for idx, val in rows:
                i = np.asarray(idx, np.int64)
                m = i >= 0
                res.append(float((np.asarray(val, np.float32)[m] * self.w[i[m]]).sum()))
            return res

    # ---------------------------------------------------------- persist/mix
    def _host(self) -> tuple[np.ndarray, np.ndarray]:
        self._check_ordered()
        if self.gpu:
            return self.w.cpu().numpy(), self.stats.cpu().numpy().astype(np.float64)
        return self.w, self.stats

    def pack(self) -> dict:
        """PA / PA1 / PA2 / perceptron: the non-zero rows of w. CW / AROW /
        NHERD: the rows with w != 0 or P != 1, and "P" (fp32) over them."""
        with self._lock:
            w, st = self._host()
            if not self.cov:
                rows = np.nonzero(w)[0].astype(np.int64)
                return {"method": self.method, "H": self.H, "rows": rows.tobytes(),
                        "w": w[rows].astype(np.float32).tobytes(), "stats": [float(x) for x in st],
                        "weights": self.conv.weights.pack()}
            P = self.P.cpu().numpy() if self.gpu else self.P
            rows = np.nonzero((w != 0) | (P != 1))[0].astype(np.int64)
            return {"method": self.method, "H": self.H, "rows": rows.tobytes(),
                    "w": w[rows].astype(np.float32).tobytes(), "stats": [float(x) for x in st],
                    "weights": self.conv.weights.pack(), "P": P[rows].astype(np.float32).tobytes()}

    def unpack(self, obj: dict) -> None:
        with self._lock:
            if int(obj["H"]) != self.H:
                raise ValueError("model hash_max_size differs from the configuration")
            if obj.get("method", self.method) != self.method:
                raise ValueError(f"model method {obj.get('method')} differs from the configured "
                                 f"{self.method}")
            self.clear()
            rows = np.frombuffer(obj["rows"], dtype=np.int64)
            w = np.zeros(self.H, np.float32)
            w[rows] = np.frombuffer(obj["w"], dtype=np.float32)
            st = np.asarray(obj["stats"], dtype=np.float64)
            P = None
            if self.cov:
                P = np.ones(self.H, np.float32)          # an absent "P": the initial precision
                if obj.get("P") is not None:
                    P[rows] = np.frombuffer(obj["P"], dtype=np.float32)
            if self.gpu:
                self.w.copy_(self.torch.from_numpy(w))
                self.stats.copy_(self.torch.from_numpy(st.astype(np.float32)))
                if self.cov:
                    self.P.copy_(self.torch.from_numpy(P))
            else:
                self.w, self.stats, self.P = w, st, P
            if obj.get("weights"):
                self.conv.weights.unpack(obj["weights"])

    def _tables(self):
        import torch
        ts = [self.w, self.P, self.stats] if self.cov else [self.w, self.stats]
        return ts if self.gpu else [torch.from_numpy(t) for t in ts]

    def mix(self) -> int:
        from ..parallel import collective as coll
        with self._lock:
            ts = self._tables()
            coll.allreduce_mean_(ts)
            return sum(t.numel() * t.element_size() for t in ts)

    def broadcast_from(self, src: int, apply: bool = True) -> None:
        """model hand-over from rank ``src``; apply=False: take part in the
        collective without replacing the local model (an up-to-date member)"""
        import torch
        import torch.distributed as dist
        with self._lock:
            for t in self._tables():
                if apply or dist.get_rank() == src:
                    dist.broadcast(t, src=src)
                else:
                    dist.broadcast(torch.empty_like(t), src=src)

    def pair_mix(self, peer: int) -> None:
        import torch
        import torch.distributed as dist
        with self._lock:
            for t in self._tables():
                buf = torch.empty_like(t)
                for r in dist.batch_isend_irecv([dist.P2POp(dist.isend, t, peer),
                                                 dist.P2POp(dist.irecv, buf, peer)]):
                    r.wait()
                t.add_(buf).mul_(0.5)

    def get_status(self) -> dict[str, str]:
        return {"num_features": str(self.H), "method": self.method,
                "storage": "hbm" if self.gpu else "host",
                "train.update_mode": self.concurrent_update}


PARegression = Regression      # the name from when PA was the only method
