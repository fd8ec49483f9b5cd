# -*- coding: utf-8 -*-
"""NumPy reference of gene_scores() / score_genes() on the dense X (tests only).

scores = Y @ W in ``longdouble``, Y = marker_reference.transform(X): y = log1p(x * target_sum / total_i), 0 at the zeros.

The bound (u = 2^-53), derived as marker_reference derives its moment bounds, from the arithmetic of the code under test and the
number format, never measured on it.  The kernel forms, per stored count of cell i, y = log1p(fl(x * scale_i)) and
acc_s = fma(W[j, s], y, acc_s):
  - y itself is within 6 u y of the reference's value (marker_reference: the product rounds once, u y; the scale is one rounded
    division, u y; log1p within 1 ulp = 2 u on the device and within 1 ulp on the reference's side, 4 u y);
  - the product W[j, s] * y is exact inside the fma, whose single rounding belongs to the sum; counted as one more u |W y|
    per term all the same, so that a kernel that multiplies and adds separately is covered too;
  - a sum of c terms in ANY order adds at most (c - 1) u times the sum of the magnitudes, to first order; the second-order
    terms are covered by counting 2 c instead of c - 1 (c u < 2^-30 for every matrix this project packs).
Together (6 + 1 + c - 1) u sum_j |W[j, s]| y_ij < (2 c_i + 8) u sum_j |W[j, s]| y_ij with c_i the stored counts of cell i: the
bound the issue states.  A cell without a stored count has bound 0: its score must be exactly 0.  In the raw mode with
integer weights every partial sum is an integer below 2^53 and the tests ask for equality instead.
"""
import numpy as np

import marker_reference as mr

U = mr.U
LD = mr.LD


def scores(X, W, **kw):
    """(reference scores (n, S) longdouble, bound (n, S) float64)."""
    X = np.asarray(X, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    if W.ndim == 1:
        W = W[:, None]
    Y = mr.transform(X, **kw)
    ref = Y @ W.astype(LD)
    mag = (Y @ np.abs(W).astype(LD)).astype(np.float64)
    return ref, bound((X != 0).sum(axis=1), mag)


def bound(c, mag):
    """(2 c_i + 8) u mag: c (n,) the stored counts per cell, mag (n, S) = sum_j |W[j, s]| y_ij."""
    c = np.asarray(c, dtype=np.float64)
    return (2.0 * c[:, None] + 8.0) * U * np.asarray(mag, dtype=np.float64)


def gene_means(X, **kw):
    """The mean of the transformed counts per gene, longdouble, and the bound of the device's value: moment_bounds of the
    one-cluster 'sum' over n, plus the division's rounding."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    cnt, s1, s2, _ = mr.moments(X, np.zeros(n, dtype=np.int64), 1, **kw)
    b1, _ = mr.moment_bounds(cnt, s1, s2)
    mean = s1[0] / LD(n)
    return mean, b1[0] / n + U * mean.astype(np.float64)
