# -*- coding: utf-8 -*-
"""float64 NumPy reference of ZIGaP.fold_in_score_samples: a held-out cell's variational bound under ZI-pCMF with the gene side
frozen and q(Z), q(d) collapsed at their optima, term by term, and the evaluation bound of the HIP value.

Frozen: V_hat (float64), lv = E[log V] (float32), pi_d, alpha1, alpha2;  pi~_j = min(max(pi_d_j, 1e-10), 1 - 1e-10), the two
override values of zigap.py:133-134.  For a cell i with the pair (a1_i., a2_i.):

    U_hat_i = a1_i / a2_i      Lambda_ij = U_hat_i . V_hat_j      z_ij = logit(pi~_j) - Lambda_ij
    lu_ik     = float32(psi(a1_ik) - log a2_ik)                               (unshifted; promoted to float64)
    data_i    = sum_{x_ij != 0} x_ij logsumexp_k(lu_ik + lv_jk)               lgamma_i = sum_{x_ij != 0} lgamma(x_ij + 1)
    dropout_i = sum_j log(1 - pi~_j) + sum_{x_ij != 0} z_ij + sum_{x_ij = 0} softplus(z_ij)
    kl_i      = sum_k KL(Gamma(a1_ik, a2_ik) || Gamma(alpha1_k, alpha2_k))
    score_i   = data_i - lgamma_i + dropout_i - kl_i

data, lgamma and kl are score_reference.cell_terms' (evaluated with a per-cell rate and no product term) and keep its bounds.

`dropout_bound` is the a-priori bound of the C entry oriana_zi_cell_bound (the two sums over j, without the cell-independent
sum_j log(1 - pi~_j)).  With u = 2^-24 (the unit roundoff of float32) and g_ij the entry's value (z or softplus(z)), the
kernel's operation sequence gives, to first order in u:
  1. U_hat and V_hat are cast to float32: each product U_ik V_jk moves by at most 2 u relative; all K are positive, so
     Lambda moves by at most 2 u Lambda.
  2. The matrix instruction is a chain of K single-rounding float32 FMAs in k order from 0 (zero-padded steps add exactly 0):
     at most K u Lambda more.
  3. logit(pi~_j) is cast to float32 (u |logit|) and x = logit - Lambda is one float32 subtraction (u |x| <= u (|logit| +
     Lambda)).  So |x - z| <= u [(K + 3) Lambda + 2 |logit|].  g(z) = z or softplus(z) has slope at most 1: the same bound holds
     for g(x) - g(z).
  4. softplus(x) = max(x, 0) + log1p(exp(-|x|)) in float32: t = exp(-|x|) in [0, 1] within 3 ulp = 6 u relative, log1p within
     2 ulp = 4 u relative (the limits of the OpenCL C specification, which the device library keeps); d log1p(t) = dt / (1 + t)
     <= rel(t) log1p(t) on [0, 1], so the logarithm term carries at most 10 u of itself, the addition u of the result: <= 11 u g.
  5. the 16 values a lane holds of one tile are added in float32, one after the other: <= 15 u sum |g| over them.
  6. tiles, lane halves and gene ranges are added in float64 (<= 20 000 additions: < 1e-11 relative, far below u).
Hence the shape  u sum_j [c1(K) Lambda_ij + c2 |logit pi~_j| + c3 (1 + |g_ij|)]  with c1(K) = K + 3, c2 = 2, c3 = 26 (steps 4 and
5).  The constant 1 beside |g| is not needed to first order: it covers what the first-order count drops (terms of order u^2 K^2,
step 6, the float64 logit before its cast).  None of the constants is fitted to a measured error.
"""
import numpy as np
from scipy.special import logit

import elbo_reference as er
import score_reference as sr
import zi_foldin_reference as zr

CELL_TERMS = ('data', 'lgamma', 'dropout', 'kl')
PI_FLOOR = 1e-10
U32 = 2.0 ** -24
C2, C3 = 2.0, 26.0


def c1(K):
    return K + 3.0


def pi_tilde(pi_d):
    return np.minimum(np.maximum(np.asarray(pi_d, dtype=np.float64), PI_FLOOR), 1.0 - PI_FLOOR)


def dropout_entries(X, V_hat, pi_d, U_hat):
    """(Lambda (n, m), logit(pi~) [m], g (n, m)): g_ij = z_ij where x_ij != 0, softplus(z_ij) elsewhere."""
    Lam = zr._dot(np.asarray(U_hat, dtype=np.float64), np.asarray(V_hat, dtype=np.float64).T)
    lg = logit(pi_tilde(pi_d))
    z = lg[None, :] - Lam
    g = np.where(np.asarray(X) != 0, z, np.logaddexp(0.0, z))
    return Lam, lg, g


def _ld_rows(a):
    return np.sum(np.asarray(a, dtype=np.longdouble), axis=1).astype(np.float64)


def dropout_sums(X, V_hat, pi_d, U_hat):
    """What oriana_zi_cell_bound returns: sum_j g_ij per cell (long double sums), and the pieces (Lambda, logits, g)."""
    Lam, lg, g = dropout_entries(X, V_hat, pi_d, U_hat)
    return _ld_rows(g), Lam, lg, g


def dropout_bound(K, Lam, logits, g):
    """The a-priori bound of the entry per cell (see the module's text for the constants)."""
    per = c1(K) * Lam + C2 * np.abs(logits)[None, :] + C3 * (1.0 + np.abs(g))
    return U32 * _ld_rows(per)


def cell_terms(X, lu, lv, a1, a2, V_hat, pi_d, alpha1, alpha2):
    """{'data', 'lgamma', 'dropout', 'kl', 'score', 'sum_x': (n,) arrays, 'abs': {term: (n,) sum of |piece|},
    'dropout_bound': (n,) the entry's bound}."""
    a1 = np.asarray(a1, dtype=np.float64)
    a2 = np.asarray(a2, dtype=np.float64)
    K = a1.shape[1]
    t = sr.cell_terms(X, lu, lv, a1, a2, np.zeros(K), alpha1, alpha2)          # (no product term: sum_v = 0)
    del t['product'], t['abs']['product']
    s, Lam, lg, g = dropout_sums(X, V_hat, pi_d, a1 / a2)
    const = np.log1p(-pi_tilde(pi_d))
    t['dropout'] = s + float(np.sum(const.astype(np.longdouble)))
    t['abs']['dropout'] = _ld_rows(np.abs(g)) + float(np.abs(const).sum())
    t['dropout_bound'] = dropout_bound(K, Lam, lg, g)
    t['score'] = t['data'] - t['lgamma'] + t['dropout'] - t['kl']
    return t


def cell_bounds(t, K):
    """Bound of each term of the HIP evaluation per cell, and of the score ('score': their sum): data, lgamma, kl as
    score_reference.cell_bounds; dropout: the entry's bound, and ACC relative to sum |piece| for the float64 additions around it."""
    g = (K + 3) * 2.0 ** -24
    b = {k: er.ACC * t['abs'][k] for k in CELL_TERMS}
    b['data'] = b['data'] + -np.log1p(-g) * t['sum_x']
    b['dropout'] = b['dropout'] + t['dropout_bound']
    b['score'] = sum(b[k] for k in CELL_TERMS)
    return b
