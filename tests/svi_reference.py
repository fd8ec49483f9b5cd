# -*- coding: utf-8 -*-
"""float64 NumPy restatement of GaP.partial_fit: one stochastic variational update of pCMF's gene side from a batch of cells.

A `state` is a dict with the priors alpha1, alpha2, beta1, beta2 [K] and the gene side b1, b2 (m, K); V_hat (m, K) and the
float32 log_V_hat (m, K) are read where the state carries them (a GPU model's state(): the expectations its kernels formed)
and are b1 / b2 and float32(psi(b1) - log b2) otherwise.  For a batch X_B (n_B, m) out of a population of n_total cells:

  1. local step   a2_row = max(1e-15, alpha2 + sum_j V_hat); a1 (n_B, K) by transform_reference.fold_in from a1_0 (default
                  transform_reference.default_start) until every cell froze at `tol` or `n_iter` is reached;
  2. statistics   lu = float32(psi(a1) - log a2_row), r_ij. = softmax_k(lu_i. + lv_j.),
                  Z_j[j,k] = sum_{i in B} x_ij r_ijk,   sum_u[k] = sum_{i in B} a1_ik / a2_row_k;
  3. global step  scale = n_total / n_B,
                  b1 <- max(1e-15, (1 - rho) b1 + rho (beta1 + scale Z_j)),   b2 <- max(1e-15, (1 - rho) b2 + rho (beta2 + scale sum_u))
                  (the convex form: rho = 0 returns b bit for bit, rho = 1 the batch estimate), then V_hat, log_V_hat from the pair.

Everything but the stated float32 casts is float64.  The priors are not moved.
`population_bound` scores a state: pCMF's collapsed variational bound of a set of cells, each folded in against the state's
gene side (tests/score_reference.py per cell), minus the gene side's Kullback-Leibler term.
"""
import numpy as np
from scipy.special import psi

import elbo_reference as er
import score_reference as sr
import transform_reference as tr

BOUND_TOL = 1e-4                  # population_bound's fold-in: its criterion ...
BOUND_ITERS = 300                 # ... and its budget


def elog_v(b1, b2):
    with np.errstate(all='ignore'):
        return (psi(np.asarray(b1, dtype=np.float64)) - np.log(np.asarray(b2, dtype=np.float64))).astype(np.float32)


def gene_side(state):
    """(V_hat float64, log_V_hat float32) of a state: as stored where it carries them, else from b1, b2."""
    V = np.asarray(state['V_hat'], dtype=np.float64) if 'V_hat' in state else np.asarray(state['b1'], np.float64) / np.asarray(state['b2'], np.float64)
    lv = np.asarray(state['log_V_hat'], dtype=np.float32) if 'log_V_hat' in state else elog_v(state['b1'], state['b2'])
    return V, lv


def cell_rate(state):
    """a2_row = max(1e-15, alpha2 + sum_j V_hat)."""
    return np.maximum(1e-15, np.asarray(state['alpha2'], dtype=np.float64) + gene_side(state)[0].sum(axis=0))


def gene_sums(X, lu, lv, chunk=32):
    """Z_j (m, K) = sum_i x_ij softmax_k(lu_ik + lv_jk) in float64 from the float32 expectations."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)          # the counts the packed layout holds
    lu = np.asarray(lu, dtype=np.float64)
    # (the softmax does not see a shift of a cell's row: see transform_reference.T64)
    lu = lu - lu.max(axis=1, keepdims=True) if lu.shape[0] else lu
    lv = np.asarray(lv, dtype=np.float64)
    Z = np.zeros_like(lv)
    for r0 in range(0, X.shape[0], chunk):
        S = lu[r0:r0 + chunk, None, :] + lv[None, :, :]
        S -= S.max(axis=2, keepdims=True)
        e = np.exp(S)
        r = e / e.sum(axis=2, keepdims=True)
        Z += np.einsum('ij,ijk->jk', X[r0:r0 + chunk], r)
    return Z


def blend(old, target, rho):
    """max(1e-15, nan_to_num((1 - rho) old + rho target))."""
    return np.maximum(1e-15, np.nan_to_num((1.0 - rho) * np.asarray(old, dtype=np.float64) + rho * target))


def partial_fit(X_B, state, n_total, rho, a1_0=None, n_iter=300, tol=1e-4):
    """(the new state, info): info = {a1, froze_at, a2_row, Z_j, sum_u} of the batch.  The new state holds the priors of the old
    one, the blended b1, b2 and the V_hat / log_V_hat formed from them."""
    X_B = np.asarray(X_B, dtype=np.float64)
    n_B = X_B.shape[0]
    if n_total < n_B:
        raise ValueError('n_total < n_B')
    V, lv = gene_side(state)
    alpha1 = np.asarray(state['alpha1'], dtype=np.float64)
    a2_row = cell_rate(state)
    if a1_0 is None:
        a1_0 = tr.default_start(X_B, alpha1)
    a1, froze_at = tr.fold_in(X_B, lv, alpha1, a2_row, np.maximum(1e-15, a1_0), n_iter, tol)
    Z_j = gene_sums(X_B, tr.elog_u(a1, a2_row), lv)
    sum_u = (a1 / a2_row[None, :]).sum(axis=0)
    new = {k: np.array(state[k], dtype=np.float64, copy=True) for k in ('alpha1', 'alpha2', 'beta1', 'beta2')}
    if n_B == 0:
        new['b1'], new['b2'] = np.array(state['b1'], np.float64, copy=True), np.array(state['b2'], np.float64, copy=True)
    else:
        scale = float(n_total) / n_B
        new['b1'] = blend(state['b1'], new['beta1'][None, :] + scale * Z_j, rho)
        new['b2'] = blend(state['b2'], (new['beta2'] + scale * sum_u)[None, :], rho)
    new['V_hat'] = new['b1'] / new['b2']
    new['log_V_hat'] = elog_v(new['b1'], new['b2'])
    return new, dict(a1=a1, froze_at=froze_at, a2_row=a2_row, Z_j=Z_j, sum_u=sum_u)


def population_bound(X, state, return_froze=False):
    """The collapsed bound of the cells X under the state's gene side: every cell folded in from the default start at tol
    1e-4 within 300 iterations, sum_i score_i (score_reference.cell_terms) - KL(q(V) || p(V))."""
    X = np.asarray(X, dtype=np.float64)
    V, lv = gene_side(state)
    alpha1, alpha2 = np.asarray(state['alpha1'], np.float64), np.asarray(state['alpha2'], np.float64)
    a2_row = cell_rate(state)
    a1, froze_at = tr.fold_in(X, lv, alpha1, a2_row, tr.default_start(X, alpha1), BOUND_ITERS, BOUND_TOL)
    t = sr.cell_terms(X, tr.elog_u(a1, a2_row), lv, a1, a2_row, V.sum(axis=0), alpha1, alpha2)
    kl_v = er.gamma_kl(state['b1'], state['b2'], state['beta1'], state['beta2'])[0]
    value = float(np.sum(np.asarray(t['score'], dtype=np.longdouble))) - kl_v
    return (value, froze_at) if return_froze else value


# ---- the warm-started stream of the planted case (tests/test_partial_fit_host.py, tests/test_partial_fit_gpu.py) -------------

WARM_CELLS = 73                   # the cells the gene side is fitted on first; also the batch size of the stream
STREAM_SEED = 3
KAPPA = 0.7


def warm_state(X, a1, b1, sweeps=40):
    """The float64 fit of the first WARM_CELLS cells (transform_reference.float64_sweeps) as a state, and the fit itself."""
    fit = tr.float64_sweeps(X[:WARM_CELLS], a1[:WARM_CELLS], b1, sweeps)
    return {k: fit[k] for k in ('alpha1', 'alpha2', 'beta1', 'beta2', 'b1', 'b2', 'V_hat', 'log_V_hat')}, fit


def stream_batches(n, n_calls, batch=WARM_CELLS, seed=STREAM_SEED):
    """The row indices of `n_calls` successive batches: per epoch one permutation of default_rng(seed), cut into batches of
    `batch`, the remainder dropped."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n_calls:
        perm = rng.permutation(n)
        out.extend(perm[i * batch:(i + 1) * batch] for i in range(n // batch))
    return out[:n_calls]


def stream_rho(t, tau0=1.0, kappa=KAPPA):
    """The step size of call t = 0, 1, ...: min(1, (tau0 + t) ** -kappa)."""
    return min(1.0, (tau0 + t) ** -kappa)
