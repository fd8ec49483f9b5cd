# -*- coding: utf-8 -*-
"""float64 NumPy restatement of GaP.transform: pCMF's cell-side update with the gene side frozen, and its freezing loop.

For a cell i that the model was not fitted on, with E[log V] (the model's float32 expectation), alpha1 and
a2 = alpha2 + sum_j V_hat (K numbers, the same for every cell and every iteration) held fixed:

    lu_ik   = float32(psi(a1_ik) - log a2_k)                  (the float32 cast of the sweep's E[log U])
    r_ij.   = softmax_k(lu_ik + lv_jk)
    T(a1)_ik = max(1e-15, alpha1_k + sum_j x_ij r_ijk)

Everything but the stated cast is float64.  `fold_in` iterates T per cell: a cell whose update satisfies
|T(a1) - a1| <= tol * a1 in every factor is frozen -- it keeps the a1 it has and is never touched again.
"""
import numpy as np
from scipy.special import psi


def elog_u(a1, a2_row):
    with np.errstate(all='ignore'):
        return (psi(np.asarray(a1, dtype=np.float64)) - np.log(np.asarray(a2_row, dtype=np.float64))[None, :]).astype(np.float32)


def T64(X, log_V_hat, alpha1, a2_row, a1, chunk=32):
    """One update of every row of a1 (n', K) for the counts X (n', m)."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)          # the counts the packed layout holds
    lu = elog_u(a1, a2_row).astype(np.float64)
    # the softmax does not see a shift of a cell's row: take the row maximum out BEFORE lv is added -- at a clamped shape
    # lu = -1e15, where float64 resolves 0.125 and lu + lv would round the gene side away
    lu = lu - lu.max(axis=1, keepdims=True)
    lv = np.asarray(log_V_hat, dtype=np.float64)
    Z = np.zeros_like(lu)
    for r0 in range(0, X.shape[0], chunk):
        S = lu[r0:r0 + chunk, None, :] + lv[None, :, :]
        S -= S.max(axis=2, keepdims=True)
        e = np.exp(S)
        r = e / e.sum(axis=2, keepdims=True)
        Z[r0:r0 + chunk] = np.einsum('ij,ijk->ik', X[r0:r0 + chunk], r)
    return np.maximum(1e-15, np.asarray(alpha1, dtype=np.float64)[None, :] + Z)


def default_start(X, alpha1):
    """alpha1 + rowsum(x) / K: one update under uniform responsibilities."""
    X = np.asarray(X, dtype=np.float64)
    K = np.asarray(alpha1).shape[0]
    return np.maximum(1e-15, np.asarray(alpha1, dtype=np.float64)[None, :] + X.sum(axis=1, keepdims=True) / K)


def fold_in(X, log_V_hat, alpha1, a2_row, a1_0, n_iter, tol):
    """(a1, froze_at): froze_at[i] is the 0-based iteration at which cell i met the criterion, n_iter if it never did."""
    X = np.asarray(X, dtype=np.float64)
    a1 = np.array(a1_0, dtype=np.float64, copy=True)
    n = a1.shape[0]
    froze_at = np.full(n, n_iter, dtype=np.int64)
    act = np.arange(n)
    for it in range(n_iter):
        if act.size == 0:
            break
        new = T64(X[act], log_V_hat, alpha1, a2_row, a1[act])
        conv = np.all(np.abs(new - a1[act]) <= tol * a1[act], axis=1)
        froze_at[act[conv]] = it
        a1[act[~conv]] = new[~conv]
        act = act[~conv]
    return a1, froze_at


def float64_sweeps(X, a1, b1, sweeps):
    """`sweeps` CAVI sweeps of pCMF in float64 from the shapes (a1, b1) with unit rates (the start of the models): the
    fitted state {alpha1, alpha2, b1, b2, V_hat, log_V_hat (float32), sum_V} a fold-in reads.  Order of the updates as the
    reference's sweep: E-step (cells from the old expectations, then genes from the new U_hat), then the M-step."""
    from oracle.cavi_oracle import inverse_digamma
    X = np.asarray(X, dtype=np.float64)
    n, m = X.shape
    K = a1.shape[1]
    a1 = np.maximum(1e-15, np.array(a1, dtype=np.float64)); b1 = np.maximum(1e-15, np.array(b1, dtype=np.float64))
    a2 = np.ones((n, K)); b2 = np.ones((m, K))
    alpha1 = np.ones(K); alpha2 = np.ones(K); beta1 = np.ones(K); beta2 = np.ones(K)

    def expectations():
        return a1 / a2, b1 / b2, psi(a1) - np.log(a2), psi(b1) - np.log(b2)

    def mstep(U, V, lu, lv):
        al1 = np.maximum(1e-15, inverse_digamma(np.log(alpha2) + lu.mean(axis=0)))
        al2 = np.maximum(1e-15, al1 / U.mean(axis=0))
        be1 = np.maximum(1e-15, inverse_digamma(np.log(beta2) + lv.mean(axis=0)))
        be2 = np.maximum(1e-15, be1 / V.mean(axis=0))
        return al1, al2, be1, be2

    U, V, lu, lv = expectations()
    alpha1, alpha2, beta1, beta2 = mstep(U, V, lu, lv)
    for _ in range(sweeps):
        S = lu[:, None, :] + lv[None, :, :]
        S -= S.max(axis=2, keepdims=True)
        e = np.exp(S)
        r = X[:, :, None] * (e / e.sum(axis=2, keepdims=True))
        a1 = np.maximum(1e-15, alpha1[None, :] + r.sum(axis=1))
        a2 = np.maximum(1e-15, alpha2[None, :] + V.sum(axis=0)[None, :]) * np.ones((n, 1))
        U = a1 / a2
        b1 = np.maximum(1e-15, beta1[None, :] + r.sum(axis=0))
        b2 = np.maximum(1e-15, beta2[None, :] + U.sum(axis=0)[None, :]) * np.ones((m, 1))
        U, V, lu, lv = expectations()
        alpha1, alpha2, beta1, beta2 = mstep(U, V, lu, lv)
    return dict(alpha1=alpha1, alpha2=alpha2, beta1=beta1, beta2=beta2, a1=a1, a2=a2, b1=b1, b2=b2, V_hat=V,
                log_V_hat=lv.astype(np.float32), sum_V=V.sum(axis=0))


def planted_query(fit, n_new=150, seed=17, zero_cell=23):
    """`n_new` fresh cells drawn from the fitted gene side: Gamma(1) loadings against V_hat, Poisson counts; one all-zero cell."""
    rng = np.random.default_rng(seed)
    K = fit['V_hat'].shape[1]
    U = rng.gamma(1.0, 1.0, size=(n_new, K))
    X = rng.poisson(U @ fit['V_hat'].T).astype(np.float64)
    X[zero_cell, :] = 0
    return X
