# -*- coding: utf-8 -*-
"""float64 restatement of FactorModel.gene_deviance() / cell_deviance() (the table in the comment above _axis_terms in
models/base.py), every sum in long double.

With Lambda = U V^T, N = {X != 0}, keep0 = {X == 0} minus the mask {round(D_hat) == 0} of the ZI models, pi the dropout
probabilities (1 without a dropout node) and mu_j = mean_i X_ij, per entry (i, j):

    factors: N: log pi_j - Lambda_ij + x log Lambda_ij      keep0: log(pi_j e^-Lambda_ij + 1 - pi_j)      else 0
    counts : N: log pi_j + x log x - x                      else 0
    mean   : N: log pi_j - mu_j + x log mu_j                X == 0: t_j = log(pi_j e^-mu_j + 1 - pi_j)  (0 exactly where mu_j = 0)

summed over the cells of a gene (axis 'genes') or over the genes of a cell (axis 'cells'), and on either axis

    reconstruction_deviance = -2 (factors - counts),      explained_deviance = (factors - mean) / (counts - mean)

as literal float64 values: a gene without a count has counts = mean = 0, so its explained deviance is not finite (-inf when
its zero term is negative, NaN when that is 0 as well); a rate that is exactly 0 at a non-zero count gives -inf.

`axes` also returns a bound for every element, derived from the arithmetic and never measured on the code under test, by the
rule and with the constants of tests/test_metrics_gpu.py and tests/deviance_path_reference.py.  Where the HIP rate is the row
pass's float32 value (a stored entry of the sliced layout whose float32 rate is at least 1e-10; `may32` below takes half of
that, see deviance_path_reference.path) |d Lambda| <= gamma Lambda with gamma = (K + 3) 2^-24: gamma sum Lambda where
sum_N Lambda is used, -log1p(-gamma) sum x on the x log Lambda sum.  Everything else (the dense block, the float64 fall-back,
the dropout term, the closed-form zero term, counts, mean) is float64: ACC relative to the sum of the absolute terms -- for
`mean` of the terms of both forms the model may use (the per-entry one above; per gene the closed form
(n - nnz_j) t_j + nnz_j (log pi_j - mu_j) + colsum_j log mu_j, per cell sum_j t_j + sum_N (c1_j + x c2_j) with
c1_j = log pi_j - mu_j - t_j, which puts 2 sum_N |t_j| on top).  Each bound is the larger of that and F_REF times the distance
of the float32 evaluation (the rate from float32 factors where the HIP code may use it) from float64.
"""
import numpy as np

from deviance_path_reference import ACC, F_REF, _log_zero_term

KEYS = ('factors', 'counts', 'mean', 'reconstruction_deviance', 'explained_deviance')


def _ld(a, axis):
    return np.sum(np.asarray(a, dtype=np.longdouble), axis=axis)


def _public(f, c, mn):
    with np.errstate(divide='ignore', invalid='ignore'):
        return -2.0 * (f - c), (f - mn) / (c - mn)


def diff(got, ref):
    """|got - ref|, 0 where both are the same infinity or both NaN."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        same = (got == ref) | (np.isnan(got) & np.isnan(ref))
        return np.where(same, 0.0, np.abs(got - ref))


def axes(X, U, V, pi, keep0, zi, f32_cols=None):
    """{'genes': r, 'cells': r}: r holds the five float64 arrays of KEYS and r['tol'] their bounds, element by element.
    `f32_cols`: boolean per gene, True where the HIP code takes the rate from the float32 row pass (the sliced layout; False:
    the dense block of a hybrid layout).  `zi`: the model has a dropout node (its zero term comes from a float64 kernel, not
    from column sums)."""
    X = np.asarray(X, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    pi = np.asarray(pi, dtype=np.float64)
    n, m = X.shape
    K = U.shape[1]
    N = X != 0
    Z = ~N
    P = np.broadcast_to(pi[np.newaxis, :], (n, m))
    f32_at = N & np.broadcast_to((np.ones(m, dtype=bool) if f32_cols is None else np.asarray(f32_cols, dtype=bool))[np.newaxis, :],
                                 (n, m))
    Lam = U @ V.T
    Lam32 = U.astype(np.float32) @ V.astype(np.float32).T
    lam_f = np.where(f32_at & (Lam32 >= np.float32(1e-10)), Lam32.astype(np.float64), Lam)
    may32 = f32_at & (Lam32 >= np.float32(5e-11))
    mu = X.sum(axis=0, dtype=np.longdouble).astype(np.float64) / n
    Mu = np.broadcast_to(mu[np.newaxis, :], (n, m))
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        lpi = np.where(N, np.log(P), 0.0)
        xlx = np.where(N, X * np.log(np.where(N, X, 1.0)) - X, 0.0)
        T = np.where(Mu > 0, _log_zero_term(Mu, P), 0.0)                      # t_j, one row per cell
        mean_n = np.where(N, lpi - Mu + X * np.log(np.where(Mu > 0, Mu, 1.0)), 0.0)
        Mn = np.where(N, mean_n, T)
        tz0 = np.where(keep0, _log_zero_term(Lam, P), 0.0)
        lam_n = np.where(N, Lam, 0.0)

        def xlog_of(L):
            return np.where(N, X * np.log(np.where(N, L, 1.0)), 0.0)
        xlog, xlog_f = xlog_of(Lam), xlog_of(lam_f)
        Fm = lpi - lam_n + xlog + tz0
        Fm_f = lpi - np.where(N, lam_f, 0.0) + xlog_f + tz0
    Cm = lpi + xlx
    g = (K + 3) * 2.0 ** -24
    nnz_t = np.where(N, np.abs(T), 0.0)
    # the closed form of a gene's mean: (n - nnz_j) t_j + nnz_j (log pi_j - mu_j) + colsum_j log mu_j
    with np.errstate(divide='ignore', invalid='ignore'):
        closed = np.where(N, np.abs(lpi - Mu) + np.abs(X * np.log(np.where(Mu > 0, Mu, 1.0))), np.abs(T))
    out = {}
    for name, ax in (('genes', 0), ('cells', 1)):
        def s(a):
            return _ld(a, ax).astype(np.float64)
        f, c, mn, f_f = s(Fm), s(Cm), s(Mn), s(Fm_f)
        rd, ed = _public(f, c, mn)
        rd_f, ed_f = _public(f_f, c, mn)
        a_lpi, a_xlx = s(np.abs(lpi)), s(np.abs(xlx))
        b_c = ACC * (a_xlx + a_lpi)
        b_m = ACC * (s(np.abs(Mn)) + s(closed) + 2.0 * s(nnz_t) + a_lpi)
        den = np.abs(c - mn)

        def bounds(gam):
            """gam = gamma: the bound of the kernels; gam = 0: float64 accumulation alone (two evaluations of the same
            arithmetic that differ in the order of the atomics)."""
            with np.errstate(invalid='ignore'):
                b_lam = gam * s(np.where(may32, Lam, 0.0)) + ACC * s(lam_n)
                b_xlog = -np.log1p(-gam) * s(np.where(may32, X, 0.0)) + ACC * s(np.abs(xlog))
                if zi:           # the dropout kernel: float64 matrix cores
                    b_f = ACC * (s(np.abs(tz0)) + s(np.where(keep0, Lam, 0.0))) + b_lam + b_xlog + ACC * a_lpi
                else:            # -(sum over all entries of the gene / cell) from float64 column sums: sum_N Lambda cancels
                    b_f = ACC * s(Lam) + b_xlog + ACC * a_lpi
                b_ed = np.where(den > 0, (b_f + b_m + np.abs(ed) * (b_c + b_m)) / np.where(den > 0, den, 1.0), np.inf)
            return {'factors': b_f, 'counts': b_c, 'mean': b_m, 'reconstruction_deviance': 2.0 * (b_f + b_c),
                    'explained_deviance': b_ed}
        tol, tol_acc = bounds(g), bounds(0.0)
        with np.errstate(invalid='ignore'):
            for q, a_f, a in (('factors', f_f, f), ('reconstruction_deviance', rd_f, rd), ('explained_deviance', ed_f, ed)):
                tol[q] = np.fmax(tol[q], F_REF * diff(a_f, a))
        out[name] = {'factors': f, 'counts': c, 'mean': mn, 'reconstruction_deviance': rd, 'explained_deviance': ed,
                     'tol': tol, 'tol_acc': tol_acc}
    return out


def check(got, ref, what='', tol='tol'):
    """Every element of the five arrays of `got` (the dict of gene_deviance / cell_deviance) against one axis of `axes`: a
    reference value that is not finite is matched exactly, a finite one within its own bound.  Prints the largest diff / bound
    ratio and the smallest and largest bound per array; returns the largest ratio."""
    worst = 0.0
    for q in KEYS:
        g, r, t = np.asarray(got[q]), ref[q], ref[tol][q]
        assert g.dtype == np.float64 and g.shape == r.shape, (what, q, g.dtype, g.shape, r.shape)
        fin = np.isfinite(r)
        exact = diff(g[~fin], r[~fin])
        assert not exact.size or np.all(exact == 0.0), '%s %s: got %r where the reference is %r (elements %r)' % (
            what, q, g[~fin], r[~fin], np.nonzero(~fin)[0])
        d = np.abs(g[fin] - r[fin])
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(d == 0, 0.0, d / t[fin])
        big = float(ratio.max()) if ratio.size else 0.0
        print('%s %s: largest diff / bound %.3e, bounds %.3e .. %.3e' % (what, q, big, t[fin].min() if ratio.size else 0.0,
                                                                         t[fin].max() if ratio.size else 0.0))
        bad = ~(np.isfinite(g[fin]) & (d <= t[fin]))
        assert not bad.any(), '%s %s: elements %r got %r ref %r diff %r > bound %r' % (
            what, q, np.nonzero(fin)[0][bad], g[fin][bad], r[fin][bad], d[bad], t[fin][bad])
        worst = max(worst, big)
    return worst
