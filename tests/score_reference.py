# -*- coding: utf-8 -*-
"""float64 NumPy reference of GaP.score_samples: a cell's share of the collapsed variational bound of pCMF with the gene side
frozen, term by term, and the evaluation bound of the HIP value.

For a cell i with shapes a1_i., the rate a2_row (K numbers, the same for every cell), lu_i. the float32 E[log U] the data term is
evaluated at and lv = E[log V] (float32), both promoted to float64:

    data_i    = sum_{j: x_ij != 0} x_ij logsumexp_k(lu_ik + lv_jk)
    lgamma_i  = sum_{j: x_ij != 0} lgamma(x_ij + 1)
    product_i = sum_k (a1_ik / a2_row_k) sum_v_k                         sum_v = sum_j V_hat_j.
    kl_i      = sum_k KL(Gamma(a1_ik, a2_row_k) || Gamma(alpha1_k, alpha2_k))
    score_i   = data_i - lgamma_i - product_i - kl_i

sum_i score_i - KL_V is the bound of tests/elbo_reference.py.  The entries come from elbo_reference.log_den_nnz and
elbo_reference.gamma_kl_pieces; every term carries the sum of the absolute values of the pieces it is added up from, and
`cell_bounds` is elbo_reference.elbo_bounds applied per cell: g = (K + 3) 2^-24 relative on the float32 den of the row pass
(-log1p(-g) x_ij on every entry of the data term), ACC = 1e-12 relative to sum |piece| for everything summed in float64.
"""
import numpy as np
from scipy.special import gammaln

import elbo_reference as er

CELL_TERMS = ('data', 'lgamma', 'product', 'kl')


def _rowsum_ld(rows, values, n):
    """Per-row sums of `values` (one row index each) accumulated in long double."""
    out = np.zeros(n, dtype=np.longdouble)
    np.add.at(out, rows, np.asarray(values, dtype=np.longdouble))
    return out.astype(np.float64)


def cell_terms(X, lu, lv, a1, a2_row, sum_v, alpha1, alpha2):
    """{'data', 'lgamma', 'product', 'kl', 'score', 'sum_x': (n,) arrays, 'abs': {term: (n,) sum of |piece|}}."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)          # the counts the packed layout holds
    a1 = np.asarray(a1, dtype=np.float64)
    n, K = a1.shape
    a2 = np.broadcast_to(np.asarray(a2_row, dtype=np.float64), (n, K))
    with np.errstate(all='ignore'):
        ii, jj, ld = er.log_den_nnz(X, lu, lv)
    x = X[ii, jj]
    prod = (a1 / a2) * np.asarray(sum_v, dtype=np.float64)[None, :]
    pieces = er.gamma_kl_pieces(a1, a2, alpha1, alpha2)
    ld_sum = lambda a: np.sum(np.asarray(a, dtype=np.longdouble), axis=1).astype(np.float64)
    t = dict(data=_rowsum_ld(ii, x * ld, n), lgamma=_rowsum_ld(ii, gammaln(x + 1.0), n), product=ld_sum(prod),
             kl=ld_sum(np.sum(np.asarray(pieces, dtype=np.longdouble), axis=0)), sum_x=_rowsum_ld(ii, x, n))
    t['abs'] = dict(data=_rowsum_ld(ii, np.abs(x * ld), n), lgamma=t['lgamma'], product=ld_sum(np.abs(prod)),
                    kl=sum(ld_sum(np.abs(p)) for p in pieces))
    t['score'] = t['data'] - t['lgamma'] - t['product'] - t['kl']
    return t


def cell_bounds(t, K):
    """Bound of each term of the HIP evaluation per cell, and of the score ('score': their sum)."""
    g = (K + 3) * 2.0 ** -24
    b = {k: er.ACC * t['abs'][k] for k in CELL_TERMS}
    b['data'] = b['data'] + -np.log1p(-g) * t['sum_x']
    b['score'] = sum(b[k] for k in CELL_TERMS)
    return b


def monotone_allowance(t0, t1, lu0, lu1, K):
    """How far a cell's score may drop from the state of t0 to a later state of the same fold-in (t1): the evaluation bounds
    of the two values, and the float32 cast of E[log U] -- an iteration is exact coordinate ascent for the uncast psi(a1) -
    log a2_row, and the cast moves a log den of the cell by a float32 rounding of lu, charged per unit count as
    2^-24 max_k |lu_ik| at the larger of the two states."""
    cast = 2.0 ** -24 * np.maximum(np.abs(lu0).max(axis=1), np.abs(lu1).max(axis=1))
    return cell_bounds(t0, K)['score'] + cell_bounds(t1, K)['score'] + t0['sum_x'] * cast
