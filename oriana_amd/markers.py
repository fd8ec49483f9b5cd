# -*- coding: utf-8 -*-
"""Marker genes of a cell clustering from per-cluster moments: the host half of FactorModel.marker_genes() (models/base.py).

The device half (csrc/groupstats.hip) leaves, per cluster c and gene j, the number of expressing cells and the sums of y and
y^2 over them, y the (log-normalised) count; the zeros of X contribute 0 to both sums, so with the cluster sizes these ARE the
moments over all cells of the cluster.  Everything here is float64 NumPy on (C, m) arrays and imports without a GPU.  It is
scanpy's ``rank_genes_groups(method='t-test')``: each cluster against the rest, Welch's statistic.  p-values are left out on
purpose: the returned scores and degrees of freedom are all a t distribution needs.

method='wilcoxon' (csrc/ranksum.hip, FactorModel.cluster_rank_sums()) has its host half here too: plan_rank_panels cuts the
genes into the panels the device sorts one at a time, wilcoxon_from_rank_sums turns exact rank sums into the rank-sum statistic.
"""
import numpy as np

__all__ = ['welch_from_moments', 'wilcoxon_from_rank_sums', 'plan_rank_panels', 'rank']


def _mean_var(s1, s2, n):
    """Mean and unbiased variance of groups of n cells from their sums; n (C, 1) > 0.  var = max(0, (s2 - s1^2 / n) / (n - 1)),
    0 where n < 2."""
    mean = s1 / n
    with np.errstate(divide='ignore', invalid='ignore'):
        var = np.where(n > 1, np.maximum(0.0, (s2 - s1 * s1 / n) / (n - 1)), 0.0)
    return mean, var


def welch_from_moments(cnt, s1, s2, sizes, log1p=True):
    """Each cluster against the rest, from moments.

    cnt, s1, s2 : (C, m) -- per cluster and gene the number of cells with a non-zero count, the sum and the sum of squares of
    the values.  sizes : (C,) cells per cluster (global).  log1p : the values are log1p-transformed (the fold change is then
    taken on expm1 of the means, as scanpy does).  With N = sum sizes, n_r = N - n_c and the rest's moments = column totals
    minus the cluster's, for every non-empty cluster c:

        mean = s1 / n,  var = max(0, (s2 - s1^2 / n) / (n - 1))  (0 where n < 2)
        score = (mean_c - mean_r) / sqrt(var_c / n_c + var_r / n_r), exactly 0 where that denominator is 0
        df    = Welch-Satterthwaite, NaN where undefined (a group of one cell with variance in play, or no variance at all)
        pct_in = cnt_c / n_c,  pct_out = cnt_r / n_r
        logfoldchange = log2((expm1(mean_c) + 1e-9) / (expm1(mean_r) + 1e-9)), without log1p log2((mean_c + 1e-9) / (mean_r + 1e-9))

    Returns a dict of (C, m) float64 arrays: 'scores', 'df', 'logfoldchanges', 'pct_in', 'pct_out', 'mean_in', 'mean_out',
    'var_in', 'var_out'.  The rows of an empty cluster are NaN.  ValueError for fewer than 2 non-empty clusters (no rest)."""
    cnt, s1, s2 = (np.asarray(a, dtype=np.float64) for a in (cnt, s1, s2))
    sizes = np.asarray(sizes)
    if cnt.ndim != 2 or s1.shape != cnt.shape or s2.shape != cnt.shape or sizes.shape != (cnt.shape[0],):
        raise ValueError('cnt, s1, s2 must be (C, m) and sizes (C,)')
    if (sizes < 0).any():
        raise ValueError('sizes must not be negative')
    live = sizes > 0
    if int(live.sum()) < 2:
        raise ValueError('a marker test needs at least 2 non-empty clusters, got %d' % int(live.sum()))
    n_c = sizes.astype(np.float64)[:, None]
    n_r = float(sizes.sum()) - n_c
    safe_c = np.where(live[:, None], n_c, 1.0)                  # (an empty cluster's rows are overwritten below)
    mean_c, var_c = _mean_var(s1, s2, safe_c)
    mean_r, var_r = _mean_var(s1.sum(0)[None, :] - s1, s2.sum(0)[None, :] - s2, n_r)
    a, b = var_c / safe_c, var_r / n_r
    den = np.sqrt(a + b)
    with np.errstate(divide='ignore', invalid='ignore'):
        scores = np.where(den > 0, (mean_c - mean_r) / den, 0.0)
        # (a / (n - 1) with n = 1 has a = 0: 0 / 0 = NaN there, as the definition has it)
        df = (a + b) ** 2 / (a * a / (safe_c - 1.0) + b * b / (n_r - 1.0))
        df = np.where(np.isfinite(df), df, np.nan)
        if log1p:
            lfc = np.log2((np.expm1(mean_c) + 1e-9) / (np.expm1(mean_r) + 1e-9))
        else:
            lfc = np.log2((mean_c + 1e-9) / (mean_r + 1e-9))
    out = {'scores': scores, 'df': df, 'logfoldchanges': lfc, 'pct_in': cnt / safe_c,
           'pct_out': (cnt.sum(0)[None, :] - cnt) / n_r, 'mean_in': mean_c, 'mean_out': mean_r, 'var_in': var_c,
           'var_out': var_r}
    for k in out:
        out[k] = np.where(live[:, None], out[k], np.nan)
    return out


def plan_rank_panels(nnz_packed, gd, budget_records):
    """Cut the packed genes into the panels oriana_rank_sums takes: contiguous runs of whole gene tiles (32 genes inside the
    dense block [0, gd), 256 in the sliced part [gd, m), the last one possibly partial), never across gd, each holding at most
    `budget_records` stored counts -- except a single tile above the budget, which is a panel of its own (the caller sizes its
    scratch to the largest panel).  nnz_packed : (m,) stored counts per gene in packed order.  Returns [(g0, g1, records)]."""
    nnz = np.asarray(nnz_packed, dtype=np.int64)
    m, gd, budget = int(nnz.shape[0]), int(gd), int(budget_records)
    if nnz.ndim != 1 or gd < 0 or gd > m or gd % 32 or budget < 0:
        raise ValueError('nnz_packed must be (m,), gd a multiple of 32 within [0, m] and the budget not negative')
    panels = []
    for lo, hi, tile in ((0, gd, 32), (gd, m, 256)):
        g0, held = lo, 0
        for t0 in range(lo, hi, tile):
            t1 = min(hi, t0 + tile)
            rec = int(nnz[t0:t1].sum())
            if t0 > g0 and held + rec > budget:
                panels.append((g0, t0, held))
                g0, held = t0, 0
            held += rec
        if hi > g0:
            panels.append((g0, hi, held))
    return panels


def wilcoxon_from_rank_sums(rank_sum, tie_term, sizes, tie_correct=False):
    """Each cluster against the rest, from rank sums: scanpy's ``rank_genes_groups(method='wilcoxon')``.

    rank_sum : (C, m) -- per cluster and gene the sum of the ranks of the cluster's cells, the ranks taken over all N = sum sizes
    cells with ties averaged (half-integers, exact in float64).  tie_term : (m,) integers T_j = sum over the tie runs of
    t^3 - t.  sizes : (C,) cells per cluster.  With n_c = sizes, n_r = N - n_c, for every non-empty cluster:

        u      = rank_sum - n_c (n_c + 1) / 2,  auc = u / (n_c n_r)
        sigma^2 = n_c n_r (N + 1) / 12, times (N^3 - N - T_j) / (N^3 - N) with tie_correct (the numerator formed in exact integers)
        scores = (rank_sum - n_c (N + 1) / 2) / sigma, exactly 0 where sigma is 0 (every cell tied, under the correction)

    Returns a dict of (C, m) float64 arrays 'scores', 'auc', 'u'.  The rows of an empty cluster are NaN.  ValueError for fewer
    than 2 non-empty clusters (no rest)."""
    R = np.asarray(rank_sum, dtype=np.float64)
    sizes = np.asarray(sizes)
    T = np.asarray(tie_term)
    if R.ndim != 2 or sizes.shape != (R.shape[0],) or T.shape != (R.shape[1],):
        raise ValueError('rank_sum must be (C, m), tie_term (m,) and sizes (C,)')
    if sizes.dtype.kind not in 'iu' or T.dtype.kind not in 'iuO':
        raise ValueError('sizes and tie_term must be integers')
    if (sizes < 0).any():
        raise ValueError('sizes must not be negative')
    live = sizes > 0
    if int(live.sum()) < 2:
        raise ValueError('a marker test needs at least 2 non-empty clusters, got %d' % int(live.sum()))
    N = int(sizes.sum())
    n_c = sizes.astype(np.float64)[:, None]
    n_r = float(N) - n_c
    pairs = np.where(live[:, None], n_c * n_r, 1.0)             # (an empty cluster's rows are overwritten below)
    u = R - n_c * (n_c + 1.0) / 2.0
    var = pairs * float(N + 1)
    if tie_correct:
        # N^3 - N - T_j in Python integers, one conversion each: 1 - T / (N^3 - N) would cancel where nearly every cell is tied
        full = N ** 3 - N
        left = np.array([float(full - int(t)) for t in T], dtype=np.float64)
        var = var * (left / float(full))[None, :]
    sigma = np.sqrt(var / 12.0)
    num = R - n_c * float(N + 1) / 2.0                          # (half-integers below 2^53: exact)
    with np.errstate(divide='ignore', invalid='ignore'):
        scores = np.where(sigma > 0, num / sigma, 0.0)
    out = {'scores': scores, 'auc': u / pairs, 'u': u}
    for k in out:
        out[k] = np.where(live[:, None], out[k], np.nan)
    return out


def rank(scores, n_top):
    """Per cluster the gene indices by (-score, gene index), NaN scores last (among themselves by index): a deterministic
    total order.  scores (C, m) -> (C, min(n_top, m)) int64."""
    scores = np.asarray(scores, dtype=np.float64)
    if scores.ndim != 2:
        raise ValueError('scores must be (C, m)')
    n_top = int(n_top)
    if n_top < 0:
        raise ValueError('n_top must not be negative')
    # (a stable sort of -score: ties keep the gene order, NaN sorts behind every number, -0.0 ties with 0.0)
    order = np.argsort(-scores, axis=1, kind='stable')
    return order[:, :min(n_top, scores.shape[1])].astype(np.int64)
