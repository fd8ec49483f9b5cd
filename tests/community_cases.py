# -*- coding: utf-8 -*-
"""The neighbour lists the community tests run on (test_community_host.py, test_community_gpu.py), from plain NumPy: brute-force
float64 distances, every row ordered by (distance, index) as knn() orders it, padded with -1 where fewer rows exist; and the
reference runs on them, computed once per process."""
import numpy as np

import community_reference as cr

GAMMAS = (0.5, 1.0, 2.0)
WEIGHTS = ('snn', 'count')


def knn_lists(Y, k):
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[0]
    sq = (Y * Y).sum(1)
    D = sq[:, None] + sq[None, :] - 2.0 * (Y @ Y.T)
    same = (Y[:, None, :] == Y[None, :, :]).all(2) if n <= 700 else None
    if same is not None:
        D[same] = 0.0                                              # bit-identical rows are at distance 0 exactly
    np.fill_diagonal(D, np.inf)
    order = np.argsort(D, axis=1, kind='stable')[:, :k]
    idx = np.full((n, k), -1, dtype=np.int32)
    m = min(k, n - 1)
    idx[:, :m] = order[:, :m]
    return idx


def blobs(seed, n, d, centres, spread, scale):
    rng = np.random.default_rng(seed)
    mu = rng.normal(size=(centres, d)) * scale
    truth = np.arange(n) % centres
    return mu[truth] + rng.normal(size=(n, d)) * spread, truth


def _star():
    idx = np.zeros((5001, 1), dtype=np.int32)                      # every leaf lists the hub, the hub lists leaf 1
    idx[0, 0] = 1
    return idx


def _identical_rows():
    Y, truth = blobs(5, 600, 20, 3, 1.0, 3.0)                      # three blobs of 200 rows in 20 dimensions
    Y[:30:3] = Y[truth == 0].mean(0)                               # ten bit-identical rows at the centre of blob 0: its hubs
    return knn_lists(Y, 12)


_cases = {}


def case(name):
    """{'indices': (n, k) int32, 'truth': the blobs' labels or None}."""
    if name not in _cases:
        truth = None
        if name == 'blobs130':
            Y, truth = blobs(1, 130, 6, 4, 1.0, 4.0)
            idx = knn_lists(Y, 4)
        elif name == 'blobs600':
            Y, truth = blobs(2, 600, 8, 6, 1.0, 10.0)              # six separated blobs
            idx = knn_lists(Y, 10)
        elif name == 'blobs2500':
            Y, truth = blobs(3, 2500, 6, 8, 1.0, 1.5)              # eight overlapping blobs
            idx = knn_lists(Y, 15)
        elif name == 'noise2000':
            idx = knn_lists(np.random.default_rng(4).normal(size=(2000, 10)), 15)
        elif name == 'identical':
            idx = _identical_rows()
        elif name == 'tiny':
            idx = knn_lists(np.random.default_rng(6).normal(size=(5, 3)), 8)        # rows that are mostly -1
        elif name == 'star':
            idx = _star()
        else:
            raise KeyError(name)
        _cases[name] = {'indices': idx, 'truth': truth}
    return _cases[name]


KNN_CASES = ('blobs130', 'blobs600', 'blobs2500', 'noise2000', 'identical', 'tiny', 'star')
ALL_CASES = KNN_CASES + ('aggregated',)

_graphs, _runs = {}, {}


def graph(name, weights):
    """(crow, col, weight) of a case by the reference; 'aggregated' is level 1 of the blobs2500 run at resolution 1 (self entries)."""
    key = (name, weights)
    if key not in _graphs:
        if name == 'aggregated':
            g = run('blobs2500', weights, 1.0)['trace'][1]['graph']
            _graphs[key] = (g[0], g[1], g[2])
        else:
            _graphs[key] = cr.snn_graph(case(name)['indices'], weights)
    return _graphs[key]


def run(name, weights, gamma):
    """The reference's louvain() of a case, with its trace."""
    key = (name, weights, float(gamma))
    if key not in _runs:
        _runs[key] = cr.louvain(*graph(name, weights), gamma=gamma, keep=True)
    return _runs[key]
