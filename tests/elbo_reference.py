# -*- coding: utf-8 -*-
"""float64 NumPy reference of the variational bound of pCMF (GaP.elbo) and the evaluation bound of the HIP value.

Gamma(shape, rate) throughout, q(U_ik) = Gamma(a1_ik, a2_ik), q(V_jk) = Gamma(b1_jk, b2_jk), priors Gamma(alpha1_k, alpha2_k)
and Gamma(beta1_k, beta2_k), q(Z) at its multinomial optimum:

    ELBO = sum_{x != 0} [x log den - lgamma(x + 1)] - sum_k (sum_i U_hat_ik)(sum_j V_hat_jk) - KL_U - KL_V
    log den_ij = logsumexp_k(log_U_hat_ik + log_V_hat_jk)

`elbo_terms` evaluates the five terms on a model state (`model.state()`: the stored float32 log expectations promoted to
float64, everything else float64), each with the sum of the absolute values of the pieces it is added up from.
`elbo_bounds` turns those into the bound of each term of the HIP evaluation, derived from the arithmetic:

  * data term: the row pass forms den' = sum_k FU_ik FV_jk from float32 shifted exponentials -- two roundings of the
    factors, a K-term float32 dot, a reciprocal and the float32 product s = x / den' -- so den' is off by at most
    g = (K + 3) 2^-24 relative (all terms are positive) and x log den by at most -log1p(-g) x;
  * every term is a float64 sum (atomics in any order, log / exp / lgamma / digamma to a few ulp): ACC = 1e-12 relative to
    the sum of |piece| over everything that is added up (for a KL: its five pieces per element, which the kernel forms
    separately -- their sum cancels, their rounding errors do not).
"""
import numpy as np
from scipy.special import gammaln, logsumexp, psi

ACC = 1e-12
TERMS = ('data', 'lgamma', 'product', 'kl_u', 'kl_v')


def _ld(a):
    return float(np.sum(np.asarray(a, dtype=np.longdouble)))


def gamma_kl_pieces(s1, s2, p1, p2):
    """The five pieces of KL(Gamma(s1, s2) || Gamma(p1, p2)) per element (p broadcast over the rows)."""
    s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    p1 = np.broadcast_to(np.asarray(p1, dtype=np.float64), s1.shape)
    p2 = np.broadcast_to(np.asarray(p2, dtype=np.float64), s1.shape)
    return ((s1 - p1) * psi(s1), -gammaln(s1), gammaln(p1), p1 * (np.log(s2) - np.log(p2)), s1 * (p2 - s2) / s2)


def gamma_kl(s1, s2, p1, p2):
    """(KL summed over the side, sum of |piece|)."""
    pieces = gamma_kl_pieces(s1, s2, p1, p2)
    return _ld(np.sum(pieces, axis=0)), sum(_ld(np.abs(p)) for p in pieces)


def log_den_nnz(X, lu, lv, chunk=1 << 22):
    """(rows, columns, log den) at the non-zero counts; the (nnz, K) sums are formed in chunks."""
    lu, lv = np.asarray(lu, dtype=np.float64), np.asarray(lv, dtype=np.float64)
    ii, jj = np.nonzero(X)
    out = np.empty(ii.size, dtype=np.float64)
    step = max(1, chunk // max(lu.shape[1], 1))
    for a in range(0, ii.size, step):
        b = min(ii.size, a + step)
        out[a:b] = logsumexp(lu[ii[a:b]] + lv[jj[a:b]], axis=1)
    return ii, jj, out


def elbo_terms(X, st):
    """{'data', 'lgamma', 'product', 'kl_u', 'kl_v', 'elbo', 'sum_x', 'abs': {...}} of the state `st` (model.state() keys)."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)          # the counts the model holds
    ii, jj, ld = log_den_nnz(X, st['log_U_hat'], st['log_V_hat'])
    x = X[ii, jj]
    su = np.sum(np.asarray(st['U_hat'], dtype=np.longdouble), axis=0).astype(np.float64)
    sv = np.sum(np.asarray(st['V_hat'], dtype=np.longdouble), axis=0).astype(np.float64)
    kl_u, abs_u = gamma_kl(st['a1'], st['a2'], st['alpha1'], st['alpha2'])
    kl_v, abs_v = gamma_kl(st['b1'], st['b2'], st['beta1'], st['beta2'])
    t = dict(data=_ld(x * ld), lgamma=_ld(gammaln(x + 1.0)), product=_ld(su * sv), kl_u=kl_u, kl_v=kl_v, sum_x=_ld(x))
    t['abs'] = dict(data=_ld(np.abs(x * ld)), lgamma=t['lgamma'], product=_ld(np.abs(su * sv)), kl_u=abs_u, kl_v=abs_v)
    t['elbo'] = t['data'] - t['lgamma'] - t['product'] - t['kl_u'] - t['kl_v']
    return t


def elbo_bounds(t, K):
    """Bound of each term of the HIP evaluation and of the value ('elbo': their sum)."""
    g = (K + 3) * 2.0 ** -24
    b = {k: ACC * t['abs'][k] for k in TERMS}
    b['data'] += -np.log1p(-g) * t['sum_x']
    b['elbo'] = sum(b[k] for k in TERMS)
    return b


def uncollapsed_elbo(X, lu, lv, U, V, kl_u, kl_v):
    """The bound with an explicit optimal q(Z_ij.) = Multinomial(x_ij, r_ij.), r_ijk = softmax_k(lu_ik + lv_jk):
        E_q[log p(X, Z | U, V)] + H[q(Z)] - KL_U - KL_V,
        E_q[log p(X, Z | U, V)] = sum_ijk [x_ij r_ijk (lu_ik + lv_jk) - U_ik V_jk] - sum_ijk E[log z_ijk!]
        H[q(Z)]                 = sum_ij [-lgamma(x_ij + 1) - x_ij sum_k r_ijk log r_ijk] + sum_ijk E[log z_ijk!]
    (Z_ijk ~ Poisson(U_ik V_jk) with x_ij = sum_k z_ijk; E[log z!] under the multinomial enters both with opposite signs and
    is left out of both).  Dense (n, m, K): for small cases only."""
    X = np.asarray(X, dtype=np.float64)
    S = lu[:, None, :] + lv[None, :, :]
    r = np.exp(S - logsumexp(S, axis=2, keepdims=True))
    ell = _ld(X[:, :, None] * r * S) - _ld(U[:, None, :] * V[None, :, :])
    with np.errstate(divide='ignore', invalid='ignore'):
        rlogr = np.where(r > 0, r * np.log(r), 0.0)
    ent = -_ld(gammaln(X + 1.0)) - _ld(X[:, :, None] * rlogr)
    return ell + ent - kl_u - kl_v
