# -*- coding: utf-8 -*-
"""Float64 NumPy restatement of the silhouette of oriana_amd/cluster.py (oriana_cluster_distance_sums, silhouette_from_sums), the
seeded inputs of its tests and the bounds the tests hold the kernel to.

Definition (scikit-learn's silhouette_samples, Euclidean metric).  Rows Y (n, d), labels in [0, C), n_c the size of cluster c,
d(i, j) the Euclidean distance; for row i with label A:
    S[c, i] = sum_{j: label(j) = c} d(i, j)          (the row itself is a term d(i, i) = 0)
    a(i) = S[A, i] / (n_A - 1),   b(i) = min over the non-empty c != A of S[c, i] / n_c,   s(i) = (b - a) / max(a, b),
    s(i) = 0 (and a(i) = 0) where n_A = 1,   s(i) = 0 where max(a, b) = 0.

Every bound comes from the arithmetic (u = 2^-24 is the unit roundoff of float32), none was measured on the code under test:

  pair       the kernel forms f = sum_j (q_j - c_j)^2 in float32 in the direct difference form: one rounding for each
             difference, one for each fused multiply-add, all terms non-negative, so f is within (d + 3) u D of the float64 value
             D (kmeans_reference.py derives the same bound for the same chain).  f of two bit-identical rows is exactly 0.
  distance   sqrt halves a relative error to first order and the correctly rounded sqrtf adds u: sqrtf(f) is within
             ((d + 3) / 2 + 1) u of the true distance, to first order; one more u covers the second-order terms at d <= 256
             (((d + 3) u)^2 / 8 < 1e-10 u there).
  sums       the conversion to float64 is exact; a float64 sum of at most n non-negative terms adds a relative (n - 1) 2^-53 in
             any order.  Every entry of S is held to EPS_S * S_ref with EPS_S = ((d + 3) / 2 + 2) u + n 2^-53; a reference entry
             of exactly 0 (every row of that cluster identical to the query) must come back as exactly 0.
  a, b       one division each: EPS_S + 2^-52, relative.
  values     s is a continuous function of (a, b): under relative perturbations of at most e of both, b - a moves by at most
             e (a + b) <= 2 e max(a, b) and max(a, b) by a factor within [1 - e, 1 + e], so |delta s| <= 2 e / (1 - e); the
             values are held to that plus 4 * 2^-53 for their own subtraction and division.
  partitions two partitions of the same call (`blocks`, candidate chunks, query blocks, row shards) add the same terms bit for
             bit in another order: S agrees within 2 n 2^-53 S.
No query is excused: the silhouette has no near-tie cases (the arg-min of b may move between two clusters, its value does not).

Property of the inputs: every non-zero difference of two entries of one feature is far above the float32 underflow of its square
(kmeans_reference.blobs: the smallest feature scale is 1e-3, so differences are around 1e-3 and their squares around 1e-6,
against 1.2e-38; tests/test_silhouette_host.py checks the smallest non-zero difference of every case against 2^-40), so no
product of the chain is flushed or loses bits to the subnormal range and the (d + 3) u bound holds as stated.
"""
import numpy as np

import kmeans_reference as kr

U = kr.U
MIN_DIFFERENCE = 2.0 ** -40


def eps_sums(n, d):
    return ((d + 3) / 2.0 + 2.0) * U + n * 2.0 ** -53


def eps_ab(n, d):
    return eps_sums(n, d) + 2.0 ** -52


def tol_values(e):
    """The bound on |delta s| under relative perturbations of at most e of a and b."""
    return 2.0 * e / (1.0 - e) + 4.0 * 2.0 ** -53


def eps_partition(n):
    return 2.0 * n * 2.0 ** -53


def distance_sums(Y, labels, C, Q=None):
    """S (C, nq) float64: the sums of the Euclidean distances of the rows of Q (default: Y) to the rows of every cluster."""
    Y = np.asarray(Y, dtype=np.float64)
    Q = Y if Q is None else np.asarray(Q, dtype=np.float64)
    labels = np.asarray(labels)
    S = np.zeros((C, Q.shape[0]))
    for a in range(0, Q.shape[0], 256):
        D = np.sqrt(kr.distances(Q[a:a + 256], Y))
        for c in range(C):
            S[c, a:a + 256] = D[:, labels == c].sum(axis=1)
    return S


def from_sums(S, counts, labels):
    """values, a, b of rows with the sums S (C, m), their labels (m,) and the cluster sizes counts (C,)."""
    S = np.asarray(S, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    m = labels.size
    own = counts[labels]
    a = np.where(own > 1, S[labels, np.arange(m)] / np.maximum(own - 1, 1), 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = np.where(counts[:, None] > 0, S / counts[:, None], np.inf)
    mean[labels, np.arange(m)] = np.inf
    b = mean.min(axis=0)
    top = np.maximum(a, b)
    ok = (own > 1) & (top > 0)
    values = np.where(ok, (b - a) / np.where(ok, top, 1.0), 0.0)
    return values, a, b


def silhouette(Y, labels, C=None):
    """S, counts, values, a, b of a labelling of the rows of Y."""
    labels = np.asarray(labels, dtype=np.int64)
    C = int(labels.max()) + 1 if C is None else C
    counts = np.bincount(labels, minlength=C).astype(np.int64)
    S = distance_sums(Y, labels, C)
    return (S, counts) + from_sums(S, counts, labels)


def check_sums(S, S_ref, n, d, what='', extra=0.0):
    """Every entry of S within EPS_S (+ extra) of the reference, relative; exact zeros where the reference is zero."""
    assert S.shape == S_ref.shape and S.dtype == np.float64, what
    assert np.all(np.isfinite(S)), what
    zero = S_ref == 0.0
    assert np.all(S[zero] == 0.0), what
    err = np.abs(S - S_ref)
    bound = (eps_sums(n, d) + extra) * S_ref
    worst = float((err[~zero] / S_ref[~zero]).max()) if (~zero).any() else 0.0
    print('%s: sums worst relative error %.3e, bound %.3e' % (what, worst, eps_sums(n, d) + extra))
    assert np.all(err <= bound), what


def check_result(res, ref, n, d, what='', extra=0.0):
    """values, a, b of a result (NumPy arrays) against (S, counts, values, a, b) of silhouette()."""
    _, counts, values, a, b = ref
    e = eps_ab(n, d) + extra
    for key, want in (('a', a), ('b', b)):
        got = res[key]
        assert got.shape == want.shape and got.dtype == np.float64 and np.all(np.isfinite(got)), (what, key)
        assert np.all(got[want == 0.0] == 0.0), (what, key)
        err = np.abs(got - want)
        print('%s: %s worst relative error %.3e, bound %.3e' % (what, key, float((err / np.where(want > 0, want, 1.0)).max()), e))
        assert np.all(err <= e * want), (what, key)
    got = res['values']
    assert got.shape == values.shape and got.dtype == np.float64 and np.all(np.isfinite(got)), what
    err = float(np.abs(got - values).max())
    print('%s: values worst error %.3e, bound %.3e' % (what, err, tol_values(e)))
    assert err <= tol_values(e), what
    assert np.all(np.abs(got) <= 1.0), what


# ---- the seeded inputs -----------------------------------------------------------------------------------------------------
# name, rows n, features d, clusters C, extra row stride, how the labels come about ('blobs': the blob of each row)
CASES = [
    ('image_is_y', 700, 100, 7, 0, 'blobs'),
    ('padded_image', 300, 3, 4, 0, 'blobs'),
    ('d1', 130, 1, 2, 0, 'blobs'),
    ('d256', 200, 256, 3, 0, 'blobs'),
    ('stride25', 257, 20, 5, 5, 'blobs'),
    ('one_row_tile', 65, 5, 3, 0, 'blobs'),
    ('edges', 200, 8, 9, 0, 'sizes'),
    ('fours', 600, 16, 150, 0, 'fours'),
]
EDGE_SIZES = {0: 1, 1: 2, 2: 7, 3: 8, 5: 9, 6: 63, 7: 64, 8: 46}       # id 4 has no rows
PARTITION_CASE = dict(seed=21, n=700, d=100, n_blobs=8)


def case_inputs(case):
    """Y (n, d) float32 and labels (n,) int64 of a case (seeded by its name)."""
    name, n, d, C, _, how = case
    seed = sum(ord(ch) for ch in name)
    Y, which, _ = kr.blobs(seed, n, d, C if how == 'blobs' else 8)
    rng = np.random.default_rng(seed + 1)
    if how == 'blobs':
        labels = which.astype(np.int64)
    elif how == 'sizes':
        labels = rng.permutation(np.concatenate([np.full(s, c, dtype=np.int64) for c, s in EDGE_SIZES.items()]))
    else:
        labels = rng.permutation(np.repeat(np.arange(C, dtype=np.int64), n // C))
    assert labels.shape == (n,)
    return Y, labels


def zeros_case():
    """Exact zeros: clusters 0 and 1 are the same single point repeated (10 and 12 times: a = b = 0 for their rows), clusters 2
    and 3 are blobs with a row duplicated inside cluster 2 and a row of cluster 2 duplicated in cluster 3."""
    d = 5
    Y, which, _ = kr.blobs(77, 60, d, 2)
    point = np.array([[1.5, -2.0, 0.25, 3.0, 1e-3]], dtype=np.float32)
    Y = np.concatenate([np.repeat(point, 22, axis=0), Y]).astype(np.float32)
    labels = np.concatenate([np.zeros(10), np.ones(12), which + 2]).astype(np.int64)
    two, three = np.nonzero(labels == 2)[0], np.nonzero(labels == 3)[0]
    Y[two[1]] = Y[two[0]]
    Y[three[0]] = Y[two[2]]
    order = np.random.default_rng(78).permutation(Y.shape[0])
    return Y[order], labels[order]


def min_nonzero_difference(Y):
    """The smallest non-zero |y_ik - y_jk| over all pairs of rows and all features."""
    best = np.inf
    for k in range(Y.shape[1]):
        gaps = np.diff(np.sort(np.asarray(Y[:, k], dtype=np.float64)))
        gaps = gaps[gaps > 0]
        if gaps.size:
            best = min(best, float(gaps.min()))
    return best
