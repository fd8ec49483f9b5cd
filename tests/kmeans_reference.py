# -*- coding: utf-8 -*-
"""Float64 NumPy restatement of the k-means of oriana_amd/cluster.py, the seeded inputs of its tests and the bounds the tests
hold the kernel to.  Every bound comes from the arithmetic (u = 2^-24 is the unit roundoff of float32), none was measured on
the code under test:

  distance   the kernel forms d2 = sum_k (y_k - c_k)^2 in float32 in the direct difference form: one rounding for each
             difference, one for each fused multiply-add, all terms non-negative, so its relative error is at most (d + 3) u.
  labels     hence the float32 arg-min equals the float64 one whenever second_best >= best * (1 + 4 (d + 3) u); the rows inside
             that gap are near-ties and are left out of a label comparison (at most NEAR_TIE_CAP of a case's rows).
  sums       against float64 sums over the kernel's own labels, per element
             (T - 1) u sum_{i in c} |y_ik| + n 2^-52 sum_{i in c} |y_ik|,  T = oriana_kmeans_partial_rows().
  inertia    relative (d + 3) u + n 2^-52 against the float64 sum over the kernel's own labels.
  mind       relative (d + 3) u per element.
"""
import numpy as np

U = 2.0 ** -24
NEAR_TIE_CAP = 0.005


def distances(Y, centers):
    """(n, C) float64 squared distances, direct difference form."""
    Y = np.asarray(Y, dtype=np.float64)
    c = np.asarray(centers, dtype=np.float64)
    d2 = np.zeros((Y.shape[0], c.shape[0]))
    for k in range(Y.shape[1]):
        d2 += (Y[:, k, None] - c[None, :, k]) ** 2
    return d2


def assign(Y, centers):
    """labels (the smallest index on a tie), the minimum distance, and the near-tie mask of the rows."""
    d2 = distances(Y, centers)
    n, C = d2.shape
    d = np.asarray(Y).shape[1]
    labels = np.argmin(d2, axis=1)
    best = d2[np.arange(n), labels] if n else np.zeros(0)
    if C > 1 and n:
        part = np.partition(d2, 1, axis=1)
        second = part[:, 1]
        near = second < best * (1.0 + 4.0 * (d + 3) * U)
    else:
        near = np.zeros(n, dtype=bool)
    return labels.astype(np.int64), best, near


def cluster_sums(Y, labels, C):
    """float64 sums, sums of absolute values and counts of the rows of each label."""
    Y = np.asarray(Y, dtype=np.float64)
    d = Y.shape[1]
    sums, asums = np.zeros((C, d)), np.zeros((C, d))
    np.add.at(sums, labels, Y)
    np.add.at(asums, labels, np.abs(Y))
    counts = np.bincount(labels, minlength=C).astype(np.int64)
    return sums, asums, counts


def tolerance_scale(Y):
    return float(np.var(np.asarray(Y, dtype=np.float64), axis=0).mean())


def lloyd(Y, init, max_iter, tol):
    """Lloyd's iteration as cluster.kmeans runs one restart: the centres are kept in float64 and rounded to float32 for the
    assignment, new centres are sums / counts, AN EMPTY CLUSTER KEEPS ITS PREVIOUS CENTRE, the restart has converged when
    sum |new - old|^2 <= tol * mean_k Var(Y[:, k]); then one more assignment with the final centres.
    Returns labels, centers, inertia, n_iter, converged, the near-tie mask accumulated over every assignment, and
    sum_{i in c} |y_ik| / count_c of the last update (the scale of the bound on the centres; 0 where the centre was kept)."""
    Y64 = np.asarray(Y, dtype=np.float64)
    centers = np.array(init, dtype=np.float64)
    C = centers.shape[0]
    thr = tol * tolerance_scale(Y64)
    n_iter, converged = 0, False
    near_any = np.zeros(Y64.shape[0], dtype=bool)
    scale = np.zeros_like(centers)
    for _ in range(max_iter):
        labels, _, near = assign(Y64, centers.astype(np.float32))
        near_any |= near
        sums, asums, counts = cluster_sums(Y64, labels, C)
        scale = asums / np.maximum(counts, 1)[:, None]
        new = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], centers)
        shift = float(((new - centers) ** 2).sum())
        centers = new
        n_iter += 1
        if shift <= thr:
            converged = True
            break
    labels, best, near = assign(Y64, centers.astype(np.float32))
    near_any |= near
    return labels, centers, float(best.sum()), n_iter, converged, near_any, scale


def kmeanspp_pick(mind, u):
    """The k-means++ pick: the first row whose float64 cumulative weight exceeds u * total (the last row of positive weight
    should u * total round up to the total)."""
    cum = np.cumsum(np.asarray(mind, dtype=np.float64))
    idx = int(np.searchsorted(cum, u * cum[-1], side='right'))
    if idx >= cum.size:
        idx = int(np.nonzero(np.asarray(mind) > 0)[0][-1])
    return idx


def adjusted_rand_index(a, b):
    a, b = np.asarray(a), np.asarray(b)
    _, ai = np.unique(a, return_inverse=True)
    _, bi = np.unique(b, return_inverse=True)
    M = np.zeros((ai.max() + 1, bi.max() + 1))
    np.add.at(M, (ai, bi), 1)
    comb = lambda x: x * (x - 1) / 2.0
    s, sa, sb, tot = comb(M).sum(), comb(M.sum(1)).sum(), comb(M.sum(0)).sum(), comb(a.size)
    exp = sa * sb / tot
    return float((s - exp) / (0.5 * (sa + sb) - exp)) if 0.5 * (sa + sb) != exp else 1.0


# ---- the seeded inputs -----------------------------------------------------------------------------------------------------
def blobs(seed, n, d, n_blobs):
    """Gaussian blobs (centres N(0, 3^2), noise N(0, 1)) as float32, a few exact duplicate rows, feature 0 scaled by 1e3 and
    feature 1 by 1e-3 (where they exist).  Returns Y, the blob of each row and the (scaled) blob centres."""
    rng = np.random.default_rng(seed)
    mu = rng.normal(0.0, 3.0, size=(n_blobs, d))
    which = rng.integers(0, n_blobs, size=n)
    Y = mu[which] + rng.normal(size=(n, d))
    scale = np.ones(d)
    scale[0] = 1e3
    if d > 1:
        scale[1] = 1e-3
    Y = (Y * scale).astype(np.float32)
    if n >= 8:
        Y[n - 1], Y[n // 2], Y[5] = Y[0], Y[1], Y[1]
        which[n - 1], which[n // 2], which[5] = which[0], which[1], which[1]
    return Y, which, mu * scale


def step_centers(seed, Y, C, R):
    """(R, C, d) float32 centres of a single-step case: rows of Y where there are enough, otherwise draws of the rows' own
    per-feature spread."""
    rng = np.random.default_rng(seed + 1000)
    n, d = Y.shape
    out = np.empty((R, C, d), dtype=np.float32)
    sd = Y.astype(np.float64).std(axis=0) + 1e-3
    mean = Y.astype(np.float64).mean(axis=0)
    for r in range(R):
        if C <= n:
            out[r] = Y[rng.choice(n, size=C, replace=False)] + (0.05 * sd * rng.normal(size=(C, d))).astype(np.float32)
        else:
            out[r] = (mean + sd * rng.normal(size=(C, d))).astype(np.float32)
    return out


# single-step cases: (name, n, d, C, R, extra row stride, blocks).  C = 'max': oriana_kmeans_max_centers(d); R = 'G+1' / '2G+1'
# with G = oriana_kmeans_group(d, C).  The row tile has 64 rows: 63 / 64 / 65 are the tile and its neighbours.
STEP_CASES = [
    ('one_row', 1, 1, 1, 1, 0, 0),
    ('tile_minus', 63, 2, 2, 3, 0, 0),
    ('tile', 64, 3, 5, 1, 0, 0),
    ('tile_plus', 65, 20, 20, 'G+1', 0, 0),
    ('five_tiles_two_blocks', 313, 100, 20, '2G+1', 0, 2),
    ('d64_maxc', 130, 64, 'max', 2, 0, 0),
    ('d65_stride', 100, 65, 5, 1, 3, 0),
    ('d128_maxc', 70, 128, 'max', '2G+1', 0, 0),
    ('d256_maxc', 65, 256, 'max', 'G+1', 0, 0),
    ('d256', 129, 256, 2, 1, 5, 0),
    ('d1_maxc', 200, 1, 'max', 1, 0, 0),
    ('many_tiles', 1000, 100, 20, '2G+1', 0, 0),
]
FULL_CASE = dict(seed=77, n=3000, d=20, C=5)


def resolve_case(case, lib):
    name, n, d, C, R, extra, blocks = case
    if C == 'max':
        C = int(lib.oriana_kmeans_max_centers(d))
    G = int(lib.oriana_kmeans_group(d, C))
    R = {'G+1': G + 1, '2G+1': 2 * G + 1}.get(R, R)
    return name, n, d, C, R, extra, blocks


def case_inputs(case, lib):
    """Y (n, d) float32 and centres (R, C, d) float32 of a resolved single-step case (seeded by its position-free name)."""
    name, n, d, C, R, extra, blocks = resolve_case(case, lib)
    seed = sum(ord(ch) for ch in name)
    Y, _, _ = blobs(seed, n, d, min(max(C, 1), 8))
    return Y, step_centers(seed, Y, C, R)
