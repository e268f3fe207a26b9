"""Brute-force float64 oracle of the five DBSCAN rules
(docs/clustering_dbscan.md), shared by test_dbscan.py and test_gpu_dbscan.py.
It is written from the definition and imports nothing from the driver."""
import numpy as np


def oracle(X, w, eps, min_core_point):
    """-> (label [n] int64: smallest point index of the cluster or -1,
    core [n] bool, mass [n] float64, A [n, n] bool, d2 [n, n] float64)"""
    X = np.asarray(X, np.float64)
    w = np.asarray(w, np.float64)
    n = X.shape[0]
    diff = X[:, None, :] - X[None, :, :]
    d2 = (diff * diff).sum(-1)
    A = d2 <= float(eps) * float(eps)                 # rule 1
    A[np.arange(n), np.arange(n)] = True
    mass = np.array([w[A[i]].sum() for i in range(n)])   # rule 2, own weight included
    core = mass >= min_core_point
    label = np.full(n, -1, np.int64)
    for i in range(n):                                # rule 3: ascending, so i is the minimum
        if not core[i] or label[i] >= 0:
            continue
        label[i] = i
        stack = [i]
        while stack:
            a = stack.pop()
            for b in np.flatnonzero(A[a] & core & (label < 0)):
                label[b] = i
                stack.append(int(b))
    for i in range(n):                                # rule 4
        if not core[i]:
            nb = np.flatnonzero(A[i] & core)
            label[i] = label[nb].min() if nb.size else -1
    return label, core, mass, A, d2


def clusters(label):
    """rule 5: point indices per cluster, clusters by ascending label"""
    label = np.asarray(label)
    return [np.flatnonzero(label == r).tolist() for r in np.unique(label[label >= 0])]
