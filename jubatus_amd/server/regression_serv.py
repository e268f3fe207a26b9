"""jubaregression server glue (reference jubatus/server/server/regression_serv.cpp).

train(list<scored_datum>) [update], estimate(list<datum>) [analysis],
clear() [update] (regression.idl:25-31).

Config: {"method", "parameter", "converter"}. The linear methods (PA, PA1,
PA2, perceptron, CW, AROW, NHERD) run on the hashed-table driver
(models/regression.py); NN / cosine / euclidean run on the nearest-neighbour
driver over the row engine (models/nn_regression.py). The native
jubaregression serves the linear methods only and hands the other three to
this server.

JUBATUS_REGRESSION_UPDATE_MODE (atomic | exact; unset or anything else:
atomic) is the linear driver's ``concurrent_update``: how a batch of queued
train requests is applied on a GPU (models/regression.py).
"""
from __future__ import annotations

import os

import msgpack

from ..common.exceptions import ArgumentError
from ..common.mprpc import split_params
from ..framework.engine_serv import EngineServ
from ..fv_converter.converter import DatumToFvConverter, device_hash_max_size
from ..models.regression import UPDATE_MODES, Regression

NN_METHODS = ("NN", "cosine", "euclidean")


def build_regression(cfg: dict, device):
    method = cfg.get("method")
    if method in NN_METHODS:
        from ..models.nn_regression import NNRegression
        return NNRegression(method, cfg.get("parameter"),
                            DatumToFvConverter(cfg.get("converter") or {}), device=device)
    # (any other name: Regression raises "unsupported regression method")
    mode = os.environ.get("JUBATUS_REGRESSION_UPDATE_MODE", "atomic")
    return Regression(method, cfg.get("parameter"),
                      DatumToFvConverter(cfg.get("converter") or {},
                                         default_hash_max_size=(device_hash_max_size()
                                                                if device is not None else None)),
                      device=device, concurrent_update=mode if mode in UPDATE_MODES else "atomic")


class RegressionServ(EngineServ):
    type_name = "regression"

    def build_driver(self, cfg: dict):
        return build_regression(cfg, self.device)

    def train(self, data) -> int:
        self.check_set_config()
        if not isinstance(data, list):
            raise ArgumentError("train: data must be a list")
        return self.driver.train(data)

    def raw_train(self, params: bytes) -> int:
        """zero-copy path (GPU fv_hash) for list<scored_datum> bodies"""
        self.check_set_config()
        parts = split_params(params)
        if len(parts) != 2:
            raise ArgumentError("train: expected 2 arguments")
        try:
            if not hasattr(self.driver, "train_requests"):     # the row-engine driver
                return self.train(msgpack.unpackb(bytes(parts[1]), raw=False))
            return self.driver.train_requests([parts[1]])
        except TypeError as e:
            raise ArgumentError(str(e)) from e

    def estimate(self, data) -> list[float]:
        self.check_set_config()
        if not isinstance(data, list):
            raise ArgumentError("estimate: data must be a list")
        return self.driver.estimate(data)
