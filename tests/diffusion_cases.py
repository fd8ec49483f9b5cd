# -*- coding: utf-8 -*-
"""The seeded cases of the diffusion tests (test_diffusion_host.py, test_diffusion_gpu.py), from plain NumPy: brute-force float64
distances cast to float32, every row ordered by (distance, index) as knn() orders it and padded with -1 / inf; and the reference
quantities on them (tests/diffusion_reference.py), computed once per process and never changed."""
import numpy as np

import diffusion_reference as dr

N_COMPS = 15
CONNECTED = ('path600', 'y1500', 'blobs2000')


def knn_lists(Y, k):
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[0]
    sq = (Y * Y).sum(1)
    D = np.maximum(sq[:, None] + sq[None, :] - 2.0 * (Y @ Y.T), 0.0)
    np.fill_diagonal(D, np.inf)
    order = np.argsort(D, axis=1, kind='stable')[:, :k]
    m = min(k, n - 1)
    idx = np.full((n, k), -1, dtype=np.int32)
    d2 = np.full((n, k), np.inf, dtype=np.float32)
    idx[:, :m] = order[:, :m]
    d2[:, :m] = np.take_along_axis(D, order[:, :m], 1).astype(np.float32)
    return idx, d2


def _path(seed=11, n=600, d=10):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.random(n))
    Y = rng.normal(size=(n, d)) * 0.03
    Y[:, 0] += 4.0 * t
    Y[:, 1] += np.sin(1.5 * np.pi * t)
    Y[:, 2] += np.cos(1.5 * np.pi * t)
    return Y, t


def _y(seed=12, n=1500, d=8):
    rng = np.random.default_rng(seed)
    s = rng.random(n)
    branch = np.arange(n) % 3                                      # 0: the trunk, 1 and 2: the two arms
    Y = rng.normal(size=(n, d)) * 0.03
    Y[:, 0] += np.where(branch == 0, 2.0 * s, 2.0 + np.where(branch == 1, 1.4, 0.9) * s)       # (arms of unequal length: no
    Y[:, 1] += np.where(branch == 0, 0.0, np.where(branch == 1, 1.4 * s, -0.9 * s))            #  near-degenerate pairs)
    return Y, np.where(branch == 0, s, 1.0 + s)


def _blobs(seed, n, d, centres, spread, scale):
    rng = np.random.default_rng(seed)
    mu = rng.normal(size=(centres, d)) * scale
    truth = np.arange(n) % centres
    return mu[truth] + rng.normal(size=(n, d)) * spread, truth


_cases = {}


def case(name):
    """{'indices': (n, k) int32, 'sq_distances': (n, k) float32, 't': the curve parameter or None}."""
    if name not in _cases:
        t = None
        if name == 'path600':
            Y, t = _path()
            k = 10
        elif name == 'y1500':
            Y, t = _y()
            k = 15
        elif name == 'blobs2000':
            Y, _ = _blobs(13, 2000, 6, 6, 1.0, 1.5)                # six overlapping blobs
            k = 15
        elif name == 'tiny':
            Y, k = np.random.default_rng(14).normal(size=(5, 3)), 2
        elif name == 'two_islands':
            Y, _ = _blobs(15, 400, 5, 2, 1.0, 40.0)                # two blobs that no neighbour list bridges
            k = 10
        else:
            raise KeyError(name)
        idx, d2 = knn_lists(Y, k)
        _cases[name] = {'indices': idx, 'sq_distances': d2, 't': t}
    return _cases[name]


def star(leaves=5000):
    """(crow, col, val, x) of a star: row 0 holds `leaves` entries, every leaf one; seeded values of both signs."""
    rng = np.random.default_rng(16)
    n = leaves + 1
    crow = np.concatenate([[0], leaves + np.arange(n)]).astype(np.int64)
    col = np.concatenate([np.arange(1, n), np.zeros(leaves)]).astype(np.int32)
    return crow, col, rng.normal(size=2 * leaves), rng.normal(size=n)


_ref = {}


def reference(name):
    """Of a case: {'T', 'z', 'P', 'csr', 'labels', and for a connected case 'eigenvalues', 'components' (the top N_COMPS + 1 by
    eigh, so that every returned pair has a lower neighbour), 'spectrum'}."""
    if name not in _ref:
        c = case(name)
        T, z, P = dr.dense_transition(c['indices'], c['sq_distances'])
        out = {'T': T, 'z': z, 'P': P, 'csr': dr.csr_of(T, P), 'labels': dr.components(P)}
        if out['labels'].max() == 0:
            m = min(N_COMPS + 1, T.shape[0])
            out['eigenvalues'], out['components'], out['spectrum'] = dr.eigh_top(T, m)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ref[name] = out
    return _ref[name]


def start(name, seed=0):
    """The start vector diffusion_map(seed=seed) draws for the case."""
    import torch
    gen = torch.Generator()
    gen.manual_seed(int(seed))
    return torch.randn(case(name)['indices'].shape[0], dtype=torch.float64, generator=gen).numpy()


def gaps(spectrum, m):
    """gap_l of the m leading eigenvalues: the distance to the nearest OTHER eigenvalue of the reference spectrum."""
    lam = np.asarray(spectrum)
    g = np.empty(m)
    for l in range(m):
        g[l] = min(lam[l - 1] - lam[l] if l else np.inf, lam[l] - lam[l + 1] if l + 1 < lam.size else np.inf)
    return g
