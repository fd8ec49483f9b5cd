# -*- coding: utf-8 -*-
"""float64 NumPy restatement of SparseGaP.project() / SparseZIGaP.project(): the cell-side update of the sparse models with the
gene side frozen, the masked-uniform start, and the freezing loop.

The frozen gene side: lv = E[log V'] (the model's float32 expectation), V'_hat (float64), p_s, the threshold tau, pi_d (sparse
ZI-pCMF) and the priors alpha1, alpha2.  From them, once per call:

    S~ = float32(p_s > tau)        S_hat = float32(p_s)        Veff = S_hat * V'_hat  (float64)

One iteration applies the map T to a cell's a1 (sparse pCMF) or to its pair (a1, a2) (sparse ZI-pCMF), everything from the OLD
values (sparse_gap.py:81-97, 118-122; sparse_zigap.py:100-116, 138-144, 163-169):

    lu_ik  = float32(psi(a1_ik) - log a2_ik)
    e_ijk  = exp(lu_ik + lv_jk) S~_jk        den_ij = sum_k e_ijk, 0 -> 1
    Z_ik   = sum_j S_hat_jk x_ij e_ijk / den_ij                     (D_hat = float32(1 - 1e-10) = 1 at the non-zeros)
    a1'_ik = max(1e-15, nan_to_num(alpha1_k + Z_ik))
    sparse pCMF:     a2_k    = max(1e-15, nan_to_num(alpha2_k + sum_j Veff_jk))            the same for every cell, never moves
    sparse ZI-pCMF:  a2'_ik  = max(1e-15, nan_to_num(alpha2_k + sum_j d_ij Veff_jk)),      d = zi_foldin_reference.dropout_f32
                                                                                           with V_hat := Veff

Everything but the stated casts (lu, S_hat, d) is float64; the exponentials are taken after a shift by the largest exponent
among a gene's UNMASKED factors, which e / den does not see (a gene with every factor masked has den = 0 -> 1 and e = 0: it
contributes exactly nothing to a1).  With S~ = S_hat = 1 the arithmetic is that of transform_reference.T64 /
zi_foldin_reference.T64, operation for operation.  The loop freezes a cell as those modules' fold_in do.
"""
import functools

import numpy as np

import zi_foldin_reference as zr

TAU = 0.5


def _clamp(v):
    return np.maximum(1e-15, np.nan_to_num(v))


def masks(p_s, tau=TAU):
    """(S~, S_hat): float32(p_s > tau) and the float32 cast of p_s, as float64 arrays."""
    p_s = np.asarray(p_s, dtype=np.float64)
    return (p_s > tau).astype(np.float32).astype(np.float64), p_s.astype(np.float32).astype(np.float64)


def effective_V(S_hat, Vp_hat):
    return np.asarray(S_hat, dtype=np.float64) * np.asarray(Vp_hat, dtype=np.float64)


def a2_row(alpha2, S_hat, Vp_hat):
    """alpha2 + sum_j S_hat V'_hat, clamped: the rate of every cell of sparse pCMF, and where a2 of sparse ZI-pCMF starts."""
    return _clamp(np.asarray(alpha2, dtype=np.float64) + effective_V(S_hat, Vp_hat).sum(axis=0))


def responsibilities_sum(X, lu, log_V_hat, S_tilde, S_hat, chunk=32):
    """Z_ik = sum_j S_hat_jk x_ij e_ijk / den_ij,  e_ijk = exp(lu_ik + lv_jk) S~_jk,  den_ij = sum_k e_ijk (0 -> 1)."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)          # the counts the packed layout holds
    lu = np.asarray(lu, dtype=np.float64)
    # (the row maximum of lu first, as transform_reference: at a clamped shape lu = -1e15 and lu + lv would round lv away)
    lu = lu - lu.max(axis=1, keepdims=True)
    lv = np.asarray(log_V_hat, dtype=np.float64)
    St = np.asarray(S_tilde, dtype=np.float64)[None, :, :]
    Sh = np.asarray(S_hat, dtype=np.float64)[None, :, :]
    Z = np.zeros_like(lu)
    with np.errstate(invalid='ignore'):
        for r0 in range(0, X.shape[0], chunk):
            S = lu[r0:r0 + chunk, None, :] + lv[None, :, :]
            mx = np.where(St > 0, S, -np.inf).max(axis=2, keepdims=True)
            S -= np.where(np.isfinite(mx), mx, 0.0)                 # (a fully masked gene: any shift, e = 0 below)
            e = np.exp(np.where(St > 0, S, -np.inf))                # (= exp(S) S~ without evaluating a masked exponent)
            den = e.sum(axis=2, keepdims=True)
            r = e / np.where(den > 0, den, 1.0)
            Z[r0:r0 + chunk] = np.einsum('ij,ijk->ik', X[r0:r0 + chunk], r * Sh)
    return Z


def T64(X, log_V_hat, S_tilde, S_hat, alpha1, a2_row_, a1):
    """Sparse pCMF: one update of every row of a1 (n', K); the rate a2_row_ [K] does not move."""
    lu = zr.elog_u(a1, np.asarray(a2_row_, dtype=np.float64)[None, :])
    return _clamp(np.asarray(alpha1, dtype=np.float64)[None, :] + responsibilities_sum(X, lu, log_V_hat, S_tilde, S_hat))


def T64_zi(X, log_V_hat, S_tilde, S_hat, Vp_hat, pi_d, alpha1, alpha2, a1, a2):
    """Sparse ZI-pCMF: one update of every row of the pair (a1, a2), each (n', K): (a1', a2')."""
    a1 = np.asarray(a1, dtype=np.float64)
    a2 = np.asarray(a2, dtype=np.float64)
    V = effective_V(S_hat, Vp_hat)
    Z = responsibilities_sum(X, zr.elog_u(a1, a2), log_V_hat, S_tilde, S_hat)
    d = zr.dropout_f32(X, V, pi_d, a1 / a2).astype(np.float64)
    return (_clamp(np.asarray(alpha1, dtype=np.float64)[None, :] + Z),
            _clamp(np.asarray(alpha2, dtype=np.float64)[None, :] + zr._dot(d, V)))


def default_start(X, alpha1, S_tilde, S_hat):
    """a1 = alpha1 + sum_j x_ij S_hat_jk S~_jk / max(1, sum_k S~_jk): one update under responsibilities uniform over each
    gene's unmasked factors.  alpha1 + rowsum(x) / K when nothing is masked and S_hat = 1."""
    X = np.asarray(X, dtype=np.float64)
    St = np.asarray(S_tilde, dtype=np.float64)
    W = np.asarray(S_hat, dtype=np.float64) * St / np.maximum(1.0, St.sum(axis=1, keepdims=True))
    return _clamp(np.asarray(alpha1, dtype=np.float64)[None, :] + zr._dot(X, W))


def fold_in(X, log_V_hat, S_tilde, S_hat, alpha1, a2_row_, a1_0, n_iter, tol):
    """Sparse pCMF: (a1, froze_at); froze_at[i] is the 0-based iteration at which cell i met |T(a1) - a1| <= tol * a1 in every
    factor (it keeps the a1 it has and is never touched again), n_iter if it never did."""
    X = np.asarray(X, dtype=np.float64)
    a1 = np.array(a1_0, dtype=np.float64, copy=True)
    froze_at = np.full(a1.shape[0], n_iter, dtype=np.int64)
    act = np.arange(a1.shape[0])
    for it in range(n_iter):
        if act.size == 0:
            break
        new = T64(X[act], log_V_hat, S_tilde, S_hat, alpha1, a2_row_, a1[act])
        conv = np.all(np.abs(new - a1[act]) <= tol * a1[act], axis=1)
        froze_at[act[conv]] = it
        a1[act[~conv]] = new[~conv]
        act = act[~conv]
    return a1, froze_at


def fold_in_zi(X, log_V_hat, S_tilde, S_hat, Vp_hat, pi_d, alpha1, alpha2, a1_0, a2_0, n_iter, tol):
    """Sparse ZI-pCMF: (a1, a2, froze_at); a cell freezes when both halves of its pair move by at most tol (relative)."""
    X = np.asarray(X, dtype=np.float64)
    a1 = np.array(a1_0, dtype=np.float64, copy=True)
    a2 = np.array(a2_0, dtype=np.float64, copy=True)
    froze_at = np.full(a1.shape[0], n_iter, dtype=np.int64)
    act = np.arange(a1.shape[0])
    for it in range(n_iter):
        if act.size == 0:
            break
        n1, n2 = T64_zi(X[act], log_V_hat, S_tilde, S_hat, Vp_hat, pi_d, alpha1, alpha2, a1[act], a2[act])
        conv = (np.all(np.abs(n1 - a1[act]) <= tol * a1[act], axis=1) & np.all(np.abs(n2 - a2[act]) <= tol * a2[act], axis=1))
        froze_at[act[conv]] = it
        a1[act[~conv]] = n1[~conv]
        a2[act[~conv]] = n2[~conv]
        act = act[~conv]
    return a1, a2, froze_at


# ---- the planted case ---------------------------------------------------------------------------------------------------------

def planted_counts(rng, zi, n=293, m=131, K=3):
    """Counts of rank K whose gene loadings are SPARSE: each gene loads on each factor with probability 0.6 (Gamma(1) loadings of
    scale 5; a gene that draws no factor is all-zero), Gamma(1) cell loadings, Poisson counts; `zi`: each gene kept with a
    probability of its own from U(0.5, 0.95).  And a Gamma(1) start (a1, b1).  With loadings of scale 1 the 40-sweep fit masks
    nine genes in ten entirely and the fresh cells are nearly empty; at this scale about a third of the genes end up fully
    masked and most of the others keep one or two factors."""
    Ut = rng.gamma(1.0, 1.0, size=(n, K))
    Vt = rng.gamma(1.0, 5.0, size=(m, K)) * (rng.random((m, K)) < 0.6)
    X = rng.poisson(Ut @ Vt.T)
    if zi:
        X = X * (rng.random((n, m)) < rng.uniform(0.5, 0.95, size=m))
    return X.astype(np.float64), rng.gamma(1.0, 1.0, size=(n, K)), rng.gamma(1.0, 1.0, size=(m, K)), K


def float64_sparse_sweeps(X, a1, b1, sweeps, zi):
    """`sweeps` CAVI sweeps of the sparse model from the shapes (a1, b1), the reference's sweep restated by oracle/cavi_oracle.py
    with its loop nest in float64 (`exact`) and D_hat[i, j] in the per-gene sums: the fitted state project() reads, keyed like
    FactorModel.state() (V_hat is V'_hat, log_V_hat the float32 E[log V'])."""
    from oracle import cavi_oracle as co
    O = (co.OracleSparseZIGaP if zi else co.OracleSparseGaP)(X, a1.shape[1], a1, b1, tau=TAU)
    O.exact = True
    for _ in range(sweeps):
        O.step()
    st = O.state()
    st['log_V_hat'] = np.asarray(st['log_V_hat'], dtype=np.float32)
    return st


def planted_query(fit, rng, zi, n_new=150, zero_cell=23):
    """`n_new` fresh cells drawn from the fitted gene side: Gamma(1) loadings against S_hat * V'_hat plus a background of 0.05,
    Poisson counts (`zi`: each kept with the fitted pi_d of its gene); one all-zero cell."""
    V = effective_V(masks(fit['p_s'])[1], fit['V_hat'])
    U = rng.gamma(1.0, 1.0, size=(n_new, V.shape[1]))
    X = rng.poisson(U @ V.T + 0.05)             # (a faint background: counts at the fully masked genes too)
    if zi:
        X = X * (rng.random(X.shape) < fit['pi_d'])
    X = X.astype(np.float64)
    X[zero_cell, :] = 0
    return X


@functools.lru_cache(maxsize=None)
def planted_case(zi, seed=5, sweeps=40, zero_cell=23):
    """The planted case of the tests: (X, a1, b1, K) of planted_counts, its 40-sweep float64 sparse fit, and 150 fresh cells --
    one random stream, in this order.  Cached: the callers only read it."""
    rng = np.random.default_rng(seed)
    X, a1, b1, K = planted_counts(rng, zi)
    fit = float64_sparse_sweeps(X, a1, b1, sweeps, zi)
    Xq = planted_query(fit, rng, zi, zero_cell=zero_cell)
    for v in (X, a1, b1, Xq) + tuple(fit.values()):
        v.setflags(write=False)
    return (X, a1, b1, K), fit, Xq
