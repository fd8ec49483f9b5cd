# -*- coding: utf-8 -*-
"""SciPy / NumPy reference of cluster_rank_sums() / marker_genes(method='wilcoxon') on the dense X (tests only).

The ranks are scipy.stats.rankdata(method='average') per gene over ALL cells on V = X * scale[:, None] in float64, the scale
formed as the model forms it (target_sum / row sums in float64 NumPy, 0 for a cell without counts).  Rank sums are sums of
half-integers below 2^53: exact in float64 in any order.  The tie term is counted in Python integers and the statistic is
assembled in longdouble.

The score bound comes from the arithmetic of markers.wilcoxon_from_rank_sums, not from its output: the numerator
R - n_c (N + 1) / 2 is a difference of half-integers below 2^53 and exact.  The denominator takes at most eight float64
roundings: the products n_c n_r and (n_c n_r)(N + 1), the tie quotient (N^3 - N - T) / (N^3 - N) of two integers converted once
each (exact below 2^53, and a correctly rounded conversion otherwise: counted with the quotient as two), its product, the
division by 12, the square root, and the final division.  Each is within 2^-53 relative and the square root halves what
reaches it, hence |score - ref| <= 8 * 2^-53 * |ref| (the reference's own longdouble error is 2^-11 of that); where the
reference's sigma is 0 the score is exactly 0."""
import numpy as np
import scipy.stats

U = 2.0 ** -53
SCORE_ROUNDINGS = 8


def scale_of(X, normalize=True, target_sum=1e4):
    if not normalize:
        return np.ones(X.shape[0])
    tot = X.sum(axis=1)
    with np.errstate(divide='ignore'):
        return np.where(tot > 0, float(target_sum) / tot, 0.0)


def values(X, normalize=True, target_sum=1e4):
    return X * scale_of(X, normalize, target_sum)[:, None]


def tie_terms(V):
    """T_j = sum over the tie runs of column j of t^3 - t, in Python integers: (m,) object."""
    T = np.empty(V.shape[1], dtype=object)
    for j in range(V.shape[1]):
        T[j] = sum(int(k) ** 3 - int(k) for k in np.unique(V[:, j], return_counts=True)[1])
    return T


def rank_sums(X, labels, C, normalize=True, target_sum=1e4, ranked=None, tied=None):
    """'rank_sum' (C, m) float64, 'tie_term' (m,) Python integers (object), 'n_expressing' (C, m) float64, 'sizes' (C,) int64.
    labels outside [0, C) are ranked and belong to no cluster.  ranked, tied: 'ranks' and 'tie_term' of an earlier call on the
    same values (they do not depend on the labels)."""
    labels = np.asarray(labels)
    V = values(X, normalize, target_sum)
    ranks = scipy.stats.rankdata(V, axis=0, method='average') if ranked is None else ranked
    m = X.shape[1]
    R = np.zeros((C, m))
    cnt = np.zeros((C, m))
    sizes = np.zeros(C, dtype=np.int64)
    for c in range(C):
        mask = labels == c
        sizes[c] = int(mask.sum())
        R[c] = ranks[mask].sum(axis=0)
        cnt[c] = (X[mask] != 0).sum(axis=0)
    T = tie_terms(V) if tied is None else tied
    return {'rank_sum': R, 'tie_term': T, 'n_expressing': cnt, 'sizes': sizes, 'ranks': ranks}


def scores(ref, tie_correct=False):
    """'scores', 'auc', 'sigma' (C, m) longdouble from rank_sums(); NaN rows for an id without cells, score 0 where sigma is 0."""
    R, sizes, T = ref['rank_sum'].astype(np.longdouble), ref['sizes'], ref['tie_term']
    N = int(sizes.sum())
    ld = np.longdouble
    n_c = sizes.astype(ld)[:, None]
    n_r = ld(N) - n_c
    var = n_c * n_r * ld(N + 1) / ld(12)
    if tie_correct:
        full = N ** 3 - N
        # (integers up to N^3 < 2^63 are exact in an x87 longdouble; where longdouble is float64 the quotient is still one rounding)
        frac = np.array([ld(full - int(t)) / ld(full) for t in T], dtype=ld)
        var = var * frac[None, :]
    sigma = np.sqrt(var)
    live = (sizes > 0)[:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        sc = np.where(sigma > 0, (R - n_c * ld(N + 1) / ld(2)) / sigma, ld(0))
        auc = (R - n_c * (n_c + 1) / ld(2)) / (n_c * n_r)
    nan = ld(np.nan)
    return {'scores': np.where(live, sc, nan), 'auc': np.where(live, auc, nan), 'sigma': np.where(live, sigma, nan)}


def score_bound(ref_scores):
    return SCORE_ROUNDINGS * U * np.abs(ref_scores.astype(np.float64))


def assert_scores(got, ref, what):
    """got (C, m) float64 against scores(): the NaN pattern, exact zeros where sigma is 0, the derived bound everywhere else."""
    rs, sg = ref['scores'].astype(np.float64), ref['sigma'].astype(np.float64)
    assert got.shape == rs.shape and got.dtype == np.float64, what
    assert np.array_equal(np.isnan(got), np.isnan(rs)), what
    ok = ~np.isnan(rs)
    assert (got[ok & (sg == 0)] == 0).all(), what
    diff = np.abs(got.astype(np.longdouble) - ref['scores'])[ok].astype(np.float64)
    b = score_bound(rs)[ok]
    worst = float((diff[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    print('%s: scores largest diff / bound = %.3g' % (what, worst))
    assert (diff <= b).all(), what
