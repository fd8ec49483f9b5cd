# -*- coding: utf-8 -*-
"""Float64 NumPy restatement of the exact k-nearest-neighbour search of oriana_amd/cluster.py (oriana_knn), the seeded inputs of
its tests and the bounds the tests hold the kernel to.  Every bound comes from the arithmetic (u = 2^-24 is the unit roundoff of
float32), none was measured on the code under test:

  distance   the kernel forms f = sum_j (q_j - c_j)^2 in float32 in the direct difference form: one rounding for each
             difference, one for each fused multiply-add, all terms non-negative, so f is within (d + 3) u D of the float64
             value D (kmeans_reference.py derives the same bound for the same chain).
  selection  let s_0 <= s_1 <= .. be the float64 distances of a query's eligible candidates and eps = 4 (d + 3) u.  A query is
             CLEAR if it has at most k candidates or s_k >= s_{k-1} (1 + eps).  For a clear query every candidate outside the
             true k nearest has f >= s_k (1 - (d + 3) u) > s_{k-1} (1 + (d + 3) u) >= the f of every candidate inside, so the
             float32 selection returns exactly the reference's index SET (the order inside the set may differ among near-ties).
             For every query, clear or not, a returned neighbour has f <= the k-th smallest f <= s_{k-1} (1 + (d + 3) u), hence
             D <= s_{k-1} (1 + (d + 3) u) / (1 - (d + 3) u) <= s_{k-1} (1 + eps).
  condition  the share of non-clear queries of every seeded case is at most kmeans_reference.NEAR_TIE_CAP.

The seeded inputs are kmeans_reference.blobs with its three duplicated rows re-drawn: with a duplicate among the candidates,
s_k == s_{k-1} for every query that has the pair at its k-th place, which is a property of the input and not of the search
(small cases reach 7 % non-clear queries).  Exact duplicates get a test of their own.
"""
import numpy as np

import kmeans_reference as kr

U = kr.U
NEAR_TIE_CAP = kr.NEAR_TIE_CAP


def eps(d):
    return 4.0 * (d + 3) * U


def masked_distances(Y, Q=None, exclude=False, q0=0, y0=0):
    """(nq, n) float64 squared distances of the rows of Q (default: Y) to the rows of Y, direct difference form; +inf where
    `exclude` bars the pair (global candidate index y0 + j == global query index q0 + i)."""
    Y = np.asarray(Y, dtype=np.float64)
    Q = Y if Q is None else np.asarray(Q, dtype=np.float64)
    D = kr.distances(Q, Y)
    if exclude:
        j = np.arange(Q.shape[0]) + q0 - y0
        ok = (j >= 0) & (j < Y.shape[0])
        D[np.nonzero(ok)[0], j[ok]] = np.inf
    return D


def neighbors(Y, Q=None, k=1, exclude=False, q0=0, y0=0):
    """The k nearest candidates of every query under (float64 distance, index): global indices (nq, k) int64 padded with -1,
    their distances padded with +inf, and the masked distance matrix."""
    D = masked_distances(Y, Q, exclude, q0, y0)
    nq, n = D.shape
    order = np.argsort(D, axis=1, kind='stable')                  # (stable: the lower index first among equal distances)
    idx = np.full((nq, k), -1, dtype=np.int64)
    dist = np.full((nq, k), np.inf)
    m = min(k, n)
    if m:
        top = order[:, :m]
        dd = np.take_along_axis(D, top, axis=1)
        idx[:, :m] = np.where(np.isfinite(dd), top + y0, -1)
        dist[:, :m] = dd
    return idx, dist, D


def clear_queries(D, k, d):
    """The clear-query mask of a masked distance matrix."""
    nq, n = D.shape
    if n <= k:
        return np.ones(nq, dtype=bool)
    s = np.sort(D, axis=1)
    return ~np.isfinite(s[:, k]) | (s[:, k] >= s[:, k - 1] * (1.0 + eps(d)))


def blobs(seed, n, d, n_blobs):
    """kmeans_reference.blobs with the rows it duplicates (n - 1, n // 2 and 5 for n >= 8) re-drawn from their own blobs."""
    Y, which, centers = kr.blobs(seed, n, d, n_blobs)
    if n >= 8:
        rng = np.random.default_rng(seed + 5000)
        scale = np.ones(d)
        scale[0] = 1e3
        if d > 1:
            scale[1] = 1e-3
        for r in (n - 1, n // 2, 5):
            Y[r] = (centers[which[r]] + rng.normal(size=d) * scale).astype(np.float32)
    return Y, which


def check(Y, idx, d2, k, Q=None, exclude=False, q0=0, y0=0, what=''):
    """A result (idx (nq, k) int32, d2 (nq, k) float32) against the reference: the shape of every row, the exact order, the
    index sets of the clear queries, and the two bounds for all queries.  Returns the share of non-clear queries."""
    n, d = np.asarray(Y).shape
    ref_idx, _, D = neighbors(Y, Q, k, exclude, q0, y0)
    nq = D.shape[0]
    assert idx.shape == (nq, k) and d2.shape == (nq, k) and idx.dtype == np.int32 and d2.dtype == np.float32, what
    clear = clear_queries(D, k, d)
    s = np.sort(D, axis=1)
    for i in range(nq):
        m = int(min(k, np.isfinite(D[i]).sum()))
        got = idx[i, :m].astype(np.int64)
        assert np.all(idx[i, m:] == -1) and np.all(np.isposinf(d2[i, m:])), (what, i)          # the padded tail
        assert np.all(got >= y0) and np.all(got < y0 + n) and np.unique(got).size == m, (what, i)
        if exclude:
            assert q0 + i not in got, (what, i)
        f = d2[i, :m]
        assert np.all((f[:-1] < f[1:]) | ((f[:-1] == f[1:]) & (got[:-1] < got[1:]))), (what, i)   # sorted by (f, index)
        if clear[i]:
            assert set(got.tolist()) == set(ref_idx[i, :m].tolist()), (what, i)
        Dg = D[i, got - y0]
        if m:
            assert np.all(Dg <= s[i, m - 1] * (1.0 + eps(d))), (what, i)
        assert np.all(np.abs(f.astype(np.float64) - Dg) <= (d + 3) * U * Dg), (what, i)
    return 1.0 - float(clear.mean()) if nq else 0.0


# single-call cases: name, rows n, features d, k ('max': oriana_knn_max_neighbors(d)), extra row stride, separate queries (None:
# the rows themselves, each left out of its own list).  The query tile has 64 rows, a step 8 candidates, a work-group 4 waves.
CASES = [
    ('one_row', 1, 3, 1, 0, None),
    ('tile_minus', 63, 2, 5, 0, None),
    ('tile', 64, 3, 15, 2, None),
    ('tile_plus', 65, 20, 15, 0, None),
    ('cand7', 7, 2, 1, 1, None),
    ('cand8', 8, 1, 15, 3, None),
    ('cand9', 9, 20, 1, 0, None),
    ('cand71', 71, 65, 15, 3, None),
    ('short_tail', 5, 6, 8, 0, None),
    ('n_minus_one', 16, 20, 15, 0, None),
    ('five_tiles_stride', 313, 100, 15, 4, None),
    ('d64_maxk', 130, 64, 'max', 0, None),
    ('d65', 100, 65, 10, 0, None),
    ('d256_maxk', 129, 256, 'max', 5, None),
    ('d1_maxk', 200, 1, 'max', 0, None),
    ('d100_maxk', 150, 100, 'max', 0, None),
    ('many_tiles', 1000, 100, 30, 0, None),
    ('d6', 700, 6, 15, 0, None),
    ('d2_k1', 300, 2, 1, 0, None),
    ('queries_one_candidate', 1, 3, 1, 0, 3),
    ('queries', 71, 100, 15, 4, 65),
]
INVARIANCE_CASE = dict(seed=21, n=700, d=100, k=15, n_blobs=8)


def resolve_case(case, lib):
    name, n, d, k, extra, nq = case
    if k == 'max':
        k = int(lib.oriana_knn_max_neighbors(d))
    return name, n, d, k, extra, nq


def case_inputs(case):
    """Y (n, d) float32 and the separate queries (nq, d) float32 or None of a case (seeded by its name)."""
    name, n, d, _, _, nq = case
    seed = sum(ord(ch) for ch in name)
    Y, _ = blobs(seed, n, d, 4)
    Q = None
    if nq is not None:
        Q = blobs(seed + 1, max(nq, 8), d, 4)[0][:nq]
    return Y, Q
