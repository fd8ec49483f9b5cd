# -*- coding: utf-8 -*-
"""NumPy reference of cell_totals() / cluster_gene_stats() / marker_genes() on the dense X (tests only).

The moments are direct masked sums in ``longdouble``; the Welch statistic is the two-pass definition (``np.var(ddof=1)``) on the
transformed dense matrix.  The bounds below are derived here from the arithmetic of the code under test and the number format,
never measured on it.

Moment bounds (u = 2^-53, the unit roundoff of float64).  The kernel forms, per non-zero count, y = log1p(fl(x * scale_i)) and
y^2 and adds them in an arbitrary order:
  - the product rounds once: relative u on the argument a = x * scale_i, and d log1p(a) = da / (1 + a) <= u * a / (1 + a)
    <= u * log1p(a), because a / ((1 + a) log(1 + a)) <= 1: at most u * y;
  - scale_i = target_sum / total_i is one correctly rounded division on either side (the reference divides in longdouble):
    another u * y at most by the same argument;
  - log1p itself is within 1 ulp = 2 u (relative) on the device, within 1 ulp on the reference's side (longdouble, far less);
  - a sum of cnt terms in any order adds at most (cnt - 1) u times the sum of the magnitudes (all terms are positive).
Together (cnt - 1 + 1 + 1 + 2 + 2) u * sum y < (2 cnt + 8) u * sum y, the bound the issue states, and for the squares, whose
relative error is twice the value's plus one rounding of the product, (cnt - 1 + 2 * 6 + 1) u * sum y^2 < (2 cnt + 16) u sum y^2.

Welch bounds.  From moments with errors e1 <= B1, e2 <= B2 (the bounds above; in the raw mode 0) the assembly in float64 adds
its own roundings.  Each quantity below carries an absolute bound propagated by first-order interval arithmetic, with a
safety factor of 4 on the rounding constants of the assembly (a dozen float64 operations per element):
  mean = s1 / n                                        : em = B1 / n + 2 u |mean|
  ss = s2 - s1^2 / n  (the cancellation)               : ess = B2 + 2 |s1| B1 / n + 4 u (s2 + s1^2 / n)
  var = max(0, ss / (n - 1))                           : ev = ess / (n - 1) + 4 u var      (max(0, .) is 1-Lipschitz)
  q = var_c / n_c + var_r / n_r, den = sqrt(q)         : eq = ev_c / n_c + ev_r / n_r + 4 u q
  score = d / den, d = mean_c - mean_r                 : ed = em_c + em_r + 2 u (|mean_c| + |mean_r|)
      |score' - score| <= ed / den_lo + |d| (1 / den_lo - 1 / den),  den_lo = sqrt(max(q - eq, 0))
      (infinite where q - eq <= 0 while q > 0: there the cancellation has eaten the variance and nothing is claimed, except
       q == 0 exactly in the reference AND in the code, which must give exactly 0)
The rest's moments are column totals minus the cluster's, formed in float64: their bounds are the sums of all clusters' bounds
plus C u times the column total (C - 1 additions and one subtraction of positive numbers).
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def totals(X):
    return np.asarray(X, dtype=np.float64).sum(axis=1)


def transform(X, normalize=True, target_sum=1e4, log1p=True):
    """The dense transformed matrix in longdouble: y = log1p(x * target_sum / total_i), 0 at the zeros."""
    Y = np.asarray(X, dtype=np.float64).astype(LD)
    if normalize:
        tot = Y.sum(axis=1)
        scale = np.where(tot > 0, LD(target_sum) / np.where(tot > 0, tot, LD(1)), LD(0))
        Y = Y * scale[:, None]
    if log1p:
        Y = np.log1p(Y)
    return Y


def moments(X, labels, C, **kw):
    """(cnt, s1, s2) (C, m) by masked sums in longdouble, and sizes (C,) int64."""
    X = np.asarray(X, dtype=np.float64)
    labels = np.asarray(labels)
    Y = transform(X, **kw)
    m = X.shape[1]
    cnt = np.zeros((C, m), dtype=np.int64)
    s1 = np.zeros((C, m), dtype=LD)
    s2 = np.zeros((C, m), dtype=LD)
    sizes = np.zeros(C, dtype=np.int64)
    for c in range(C):
        sel = labels == c
        sizes[c] = int(sel.sum())
        if sizes[c]:
            cnt[c] = (X[sel] != 0).sum(axis=0)
            s1[c] = Y[sel].sum(axis=0)
            s2[c] = (Y[sel] * Y[sel]).sum(axis=0)
    return cnt, s1, s2, sizes


def moment_bounds(cnt, s1, s2):
    """The issue's bounds on 'sum' and 'sumsq' (the derivation is in the module docstring)."""
    c = cnt.astype(np.float64)
    return (2 * c + 8) * U * np.asarray(s1, dtype=np.float64), (2 * c + 16) * U * np.asarray(s2, dtype=np.float64)


def welch_two_pass(X, labels, C, log1p=True, **kw):
    """Welch's statistic of every cluster against the rest by the two-pass definition on the transformed dense matrix."""
    labels = np.asarray(labels)
    Y = transform(X, log1p=log1p, **kw)
    Xn = np.asarray(X) != 0
    m = Y.shape[1]
    keys = ('scores', 'df', 'logfoldchanges', 'pct_in', 'pct_out', 'mean_in', 'mean_out', 'var_in', 'var_out', 'q')
    out = {k: np.full((C, m), np.nan, dtype=LD) for k in keys}
    for c in range(C):
        sel = labels == c
        nc, nr = int(sel.sum()), int((~sel).sum())
        if nc == 0:
            continue
        A, B = Y[sel], Y[~sel]
        mc, mr = A.mean(axis=0), B.mean(axis=0)
        vc = A.var(axis=0, ddof=1) if nc > 1 else np.zeros(m, dtype=LD)
        vr = B.var(axis=0, ddof=1) if nr > 1 else np.zeros(m, dtype=LD)
        a, b = vc / nc, vr / nr
        q = a + b
        with np.errstate(divide='ignore', invalid='ignore'):
            out['scores'][c] = np.where(q > 0, (mc - mr) / np.sqrt(q), LD(0))
            df = q * q / (a * a / LD(nc - 1) + b * b / LD(nr - 1))
            out['df'][c] = np.where(np.isfinite(df), df, np.nan)
            if log1p:
                out['logfoldchanges'][c] = np.log2((np.expm1(mc) + LD(1e-9)) / (np.expm1(mr) + LD(1e-9)))
            else:
                out['logfoldchanges'][c] = np.log2((mc + LD(1e-9)) / (mr + LD(1e-9)))
        out['pct_in'][c] = Xn[sel].mean(axis=0)
        out['pct_out'][c] = Xn[~sel].mean(axis=0)
        out['mean_in'][c], out['mean_out'][c], out['var_in'][c], out['var_out'][c], out['q'][c] = mc, mr, vc, vr, q
    return out


def welch_bounds(s1, s2, sizes, B1, B2):
    """Absolute bounds on 'scores', the means and the variances of an assembly from moments that are within (B1, B2) of the
    (C, m) float64 moments (s1, s2); see the module docstring.  Rows of empty clusters are NaN."""
    s1, s2, B1, B2 = (np.asarray(a, dtype=np.float64) for a in (s1, s2, B1, B2))
    live = sizes > 0
    n_c = sizes.astype(np.float64)[:, None]
    n_r = float(sizes.sum()) - n_c

    def side(t1, t2, b1, b2, n):
        n = np.where(n > 0, n, 1.0)
        mean = t1 / n
        em = b1 / n + 2 * U * np.abs(mean)
        ess = b2 + 2 * np.abs(t1) * b1 / n + 4 * U * (t2 + t1 * t1 / n)
        nm1 = np.where(n > 1, n - 1, 1.0)
        var = np.where(n > 1, np.maximum(0.0, (t2 - t1 * t1 / n) / nm1), 0.0)
        ev = np.where(n > 1, ess / nm1 + 4 * U * var, 0.0)
        return mean, em, var, ev, n

    mc, emc, vc, evc, nc = side(s1, s2, B1, B2, n_c)
    # (the rest's moments are fl(fl(sum_c s) - s_c): C - 1 additions and one subtraction of positive float64 numbers, at most
    #  C u sum_c s on top of the clusters' own bounds)
    C = s1.shape[0]
    t1, t2 = s1.sum(0)[None], s2.sum(0)[None]
    mr, emr, vr, evr, nr = side(t1 - s1, t2 - s2, B1.sum(0)[None] + C * U * t1 + 0 * B1, B2.sum(0)[None] + C * U * t2 + 0 * B2, n_r)
    q = vc / nc + vr / nr
    eq = evc / nc + evr / nr + 4 * U * q
    d = mc - mr
    ed = emc + emr + 2 * U * (np.abs(mc) + np.abs(mr))
    with np.errstate(divide='ignore', invalid='ignore'):
        den, den_lo = np.sqrt(q), np.sqrt(np.maximum(q - eq, 0.0))
        es = np.where(den_lo > 0, ed / den_lo + np.abs(d) * (1.0 / den_lo - 1.0 / den), np.inf)
        es = np.where(q == 0, 0.0, es)
    out = {'scores': es, 'mean_in': emc, 'mean_out': emr, 'var_in': evc, 'var_out': evr, 'q': q, 'eq': eq}
    return {k: np.where(live[:, None], v, np.nan) for k, v in out.items()}
