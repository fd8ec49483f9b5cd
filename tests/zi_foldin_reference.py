# -*- coding: utf-8 -*-
"""float64 NumPy restatement of ZIGaP.fold_in: ZI-pCMF's cell-side update with the gene side frozen, and its freezing loop.

A new cell i carries the pair (a1_i, a2_i), K float64 values each.  With V_hat (float64), E[log V] (the model's float32
expectation), pi_d and the priors alpha1, alpha2 held fixed, one iteration applies the map T, both outputs from the OLD pair
(the reference's sweep order, zigap.py:115-136: the rate reads the D_hat formed from the U_hat that enters the sweep):

    lu_ik   = float32(psi(a1_ik) - log a2_ik)            U_hat_ik = a1_ik / a2_ik
    Z_ik    = sum_j x_ij softmax_k(lu_i. + lv_j.)        (D_hat = float32(1 - 1e-10) = 1 at the non-zeros: the pCMF row pass)
    d_ij    = 1                                          where x_ij != 0
            = 1e-10 / 1 - 1e-10                          where pi_d_j <= 0 / >= 1
            = float32(sigmoid(logit(pi_d_j) - U_hat_i . V_hat_j))   elsewhere        (zigap.py:131-136, bernoulli.py:45)
    a1'_ik  = max(1e-15, nan_to_num(alpha1_k + Z_ik))
    a2'_ik  = max(1e-15, nan_to_num(alpha2_k + sum_j d_ij V_hat_jk))

Everything but the two stated casts (lu, d) is float64.  `fold_in` iterates T per cell: a cell whose update satisfies
|a1' - a1| <= tol * a1 and |a2' - a2| <= tol * a2 in every factor is frozen -- it keeps the pair it has and is never touched
again.  The D_hat[i, k] index of zigap.py:94 (reference_quirks) touches only the per-gene sums: it does not enter the cell side.
"""
import functools

import numpy as np
from scipy.special import expit, logit, psi


def _clamp(v):
    return np.maximum(1e-15, np.nan_to_num(v))


def _dot(A, B):
    """A @ B by einsum's own loops: a row of the result does not depend on which other rows are in A (a BLAS product blocks by
    shape, and a cell folded in alone would differ in the last bit from the same cell in a batch)."""
    return np.einsum('ij,jk->ik', A, B)


def elog_u(a1, a2):
    with np.errstate(all='ignore'):
        return (psi(np.asarray(a1, dtype=np.float64)) - np.log(np.asarray(a2, dtype=np.float64))).astype(np.float32)


def dropout_f32(X, V_hat, pi_d, U_hat):
    """d (n', m) float32: the dropout posterior of the new cells, as Bernoulli.mean casts it."""
    pi_d = np.asarray(pi_d, dtype=np.float64)
    with np.errstate(all='ignore'):
        p = expit(logit(pi_d)[None, :] - _dot(np.asarray(U_hat, dtype=np.float64), np.asarray(V_hat, dtype=np.float64).T))
    p[:, pi_d <= 0] = 1e-10
    p[:, pi_d >= 1] = 1 - 1e-10
    p[np.asarray(X) != 0] = 1 - 1e-10
    return p.astype(np.float32)


def responsibilities_sum(X, lu, log_V_hat, chunk=32):
    """Z_ik = sum_j x_ij softmax_k(lu_i. + lv_j.)"""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)          # the counts the packed layout holds
    lu = np.asarray(lu, dtype=np.float64)
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
    return Z


def T64(X, log_V_hat, V_hat, pi_d, alpha1, alpha2, a1, a2):
    """One update of every row of the pair (a1, a2), each (n', K), for the counts X (n', m): (a1', a2')."""
    a1 = np.asarray(a1, dtype=np.float64)
    a2 = np.asarray(a2, dtype=np.float64)
    V = np.asarray(V_hat, dtype=np.float64)
    Z = responsibilities_sum(X, elog_u(a1, a2), log_V_hat)
    d = dropout_f32(X, V, pi_d, a1 / a2).astype(np.float64)
    return (_clamp(np.asarray(alpha1, dtype=np.float64)[None, :] + Z),
            _clamp(np.asarray(alpha2, dtype=np.float64)[None, :] + _dot(d, V)))


def default_start(X, alpha1, alpha2, V_hat):
    """a1 = alpha1 + rowsum(x) / K (uniform responsibilities); a2 = alpha2 + sum_j V_hat, the pCMF rate: no dropout yet."""
    X = np.asarray(X, dtype=np.float64)
    K = np.asarray(alpha1).shape[0]
    a1 = _clamp(np.asarray(alpha1, dtype=np.float64)[None, :] + X.sum(axis=1, keepdims=True) / K)
    a2 = _clamp(np.asarray(alpha2, dtype=np.float64) + np.asarray(V_hat, dtype=np.float64).sum(axis=0))[None, :] * np.ones((X.shape[0], 1))
    return a1, a2


def fold_in(X, log_V_hat, V_hat, pi_d, alpha1, alpha2, a1_0, a2_0, n_iter, tol):
    """(a1, a2, froze_at): froze_at[i] is the 0-based iteration at which cell i met the criterion, n_iter if it never did."""
    X = np.asarray(X, dtype=np.float64)
    a1 = np.array(a1_0, dtype=np.float64, copy=True)
    a2 = np.array(a2_0, dtype=np.float64, copy=True)
    n = a1.shape[0]
    froze_at = np.full(n, n_iter, dtype=np.int64)
    act = np.arange(n)
    for it in range(n_iter):
        if act.size == 0:
            break
        n1, n2 = T64(X[act], log_V_hat, V_hat, pi_d, alpha1, alpha2, a1[act], a2[act])
        conv = (np.all(np.abs(n1 - a1[act]) <= tol * a1[act], axis=1) & np.all(np.abs(n2 - a2[act]) <= tol * a2[act], axis=1))
        froze_at[act[conv]] = it
        a1[act[~conv]] = n1[~conv]
        a2[act[~conv]] = n2[~conv]
        act = act[~conv]
    return a1, a2, froze_at


def planted_counts(rng, n=293, m=131, K=3):
    """Counts of the shape of tests/test_elbo_gpu._planted with dropouts: Gamma(1) factors of rank K, Poisson counts, each gene
    kept with a probability of its own drawn from U(0.5, 0.95); and a Gamma(1) start (a1, b1)."""
    Ut = rng.gamma(1.0, 1.0, size=(n, K))
    Vt = rng.gamma(1.0, 1.0, size=(m, K))
    pi_true = rng.uniform(0.5, 0.95, size=m)
    X = (rng.poisson(Ut @ Vt.T) * (rng.random((n, m)) < pi_true)).astype(np.float64)
    return X, rng.gamma(1.0, 1.0, size=(n, K)), rng.gamma(1.0, 1.0, size=(m, K)), K


def float64_zi_sweeps(X, a1, b1, sweeps):
    """`sweeps` CAVI sweeps of ZI-pCMF in float64 from the shapes (a1, b1) with unit rates and p_d = (X > 0) (the start of
    the models, zigap.py:77): the fitted state a fold-in reads, keyed like FactorModel.state().  Order of the updates as the
    reference's sweep (cells from the old expectations and the old D_hat, genes from the new U_hat, then D from both new
    factors; the M-step last), with D_hat[i, j] in the per-gene sums (no index quirk) and D_hat the float32 cast of p_d."""
    from oracle.cavi_oracle import inverse_digamma
    X = np.asarray(X, dtype=np.float64)
    n, m = X.shape
    K = a1.shape[1]
    a1 = np.array(a1, dtype=np.float64)
    b1 = np.array(b1, dtype=np.float64)
    a2 = np.ones((n, K))
    b2 = np.ones((m, K))
    alpha2 = np.ones(K)
    beta2 = np.ones(K)
    p_d = (X > 0).astype(np.float64)

    def resp(lu, lv):
        S = lu[:, None, :] + lv[None, :, :]
        S -= S.max(axis=2, keepdims=True)
        e = np.exp(S)
        return X[:, :, None] * (e / e.sum(axis=2, keepdims=True))

    def dq(U, V, pi_d):
        with np.errstate(all='ignore'):
            p = expit(logit(pi_d)[None, :] - U @ V.T)
        p[:, pi_d <= 0] = 1e-10
        p[:, pi_d >= 1] = 1 - 1e-10
        p[X != 0] = 1 - 1e-10
        return p

    def mstep(U, V, lu, lv, alpha2, beta2):
        al1 = np.maximum(1e-15, inverse_digamma(np.log(alpha2) + lu.mean(axis=0)))
        al2 = np.maximum(1e-15, al1 / U.mean(axis=0))
        be1 = np.maximum(1e-15, inverse_digamma(np.log(beta2) + lv.mean(axis=0)))
        be2 = np.maximum(1e-15, be1 / V.mean(axis=0))
        return al1, al2, be1, be2

    U, V, lu, lv = a1 / a2, b1 / b2, psi(a1) - np.log(a2), psi(b1) - np.log(b2)
    alpha1, alpha2, beta1, beta2 = mstep(U, V, lu, lv, alpha2, beta2)
    pi_d = p_d.mean(axis=0)
    for _ in range(sweeps):
        D = p_d.astype(np.float32).astype(np.float64)
        r = resp(lu, lv)
        a1 = np.maximum(1e-15, alpha1 + (D[:, :, None] * r).sum(axis=1))
        a2 = np.maximum(1e-15, alpha2 + D @ V)
        U = a1 / a2
        lu = psi(a1) - np.log(a2)
        b1 = np.maximum(1e-15, beta1 + (D[:, :, None] * r).sum(axis=0))
        b2 = np.maximum(1e-15, beta2 + D.T @ U)
        V = b1 / b2
        lv = psi(b1) - np.log(b2)
        p_d = dq(U, V, pi_d)
        alpha1, alpha2, beta1, beta2 = mstep(U, V, lu, lv, alpha2, beta2)
        pi_d = p_d.mean(axis=0)
    return dict(alpha1=alpha1, alpha2=alpha2, beta1=beta1, beta2=beta2, a1=a1, a2=a2, b1=b1, b2=b2, pi_d=pi_d, p_d=p_d,
                V_hat=V, log_V_hat=lv.astype(np.float32))


def planted_query(fit, rng, n_new=150, zero_cell=23):
    """`n_new` fresh cells drawn from the fitted gene side: Gamma(1) loadings against V_hat, Poisson counts, each count kept
    with the fitted pi_d of its gene; one all-zero cell."""
    K = fit['V_hat'].shape[1]
    m = fit['V_hat'].shape[0]
    U = rng.gamma(1.0, 1.0, size=(n_new, K))
    X = (rng.poisson(U @ fit['V_hat'].T) * (rng.random((n_new, m)) < fit['pi_d'])).astype(np.float64)
    X[zero_cell, :] = 0
    return X


@functools.lru_cache(maxsize=None)
def planted_case(seed=5, sweeps=40, zero_cell=23):
    """The planted case of the tests: (X, a1, b1, K) of planted_counts, its 40-sweep float64 ZI fit, and 150 fresh cells -- one
    random stream, in this order.  Cached: the callers only read it."""
    rng = np.random.default_rng(seed)
    X, a1, b1, K = planted_counts(rng)
    fit = float64_zi_sweeps(X, a1, b1, sweeps)
    Xq = planted_query(fit, rng, zero_cell=zero_cell)
    for v in (X, a1, b1, Xq) + tuple(fit.values()):
        v.setflags(write=False)
    return (X, a1, b1, K), fit, Xq
