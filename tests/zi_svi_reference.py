# -*- coding: utf-8 -*-
"""float64 NumPy restatement of ZIGaP.fold_in_fit: one stochastic variational update of ZI-pCMF's gene side from a batch of cells.

A `state` is a dict with the priors alpha1, alpha2, beta1, beta2 [K], the gene side b1, b2 (m, K) and pi_d [m]; V_hat (m, K) and the
float32 log_V_hat (m, K) are read where the state carries them and are b1 / b2 and float32(psi(b1) - log b2) otherwise
(svi_reference.gene_side).  For a batch X_B (n_B, m) out of a population of n_total cells:

  1. local    (a1, a2) (n_B, K) by zi_foldin_reference.fold_in from a1_0 (default zi_foldin_reference.default_start; a2 always
              starts at alpha2 + sum_j V_hat) until every cell froze at `tol` or `n_iter` is reached;
  2. stats    U_hat = a1 / a2,  lu = float32(psi(a1) - log a2),
              Z_j[j,k] = sum_{i in B} x_ij softmax_k(lu_i. + lv_j.)                    (svi_reference.gene_sums: D_hat = 1 at the non-zeros)
              d = zi_foldin_reference.dropout_f32(X_B, V_hat, pi_d, U_hat) promoted to float64
              G[j,k] = sum_{i in B} d_ij U_hat_ik,    dsum[j] = sum_{i in B} d_ij;
  3. global   scale = n_total / n_B,
              b1 <- max(1e-15, nan_to_num((1 - rho) b1 + rho (beta1 + scale Z_j)))     (svi_reference.blend)
              b2 <- max(1e-15, nan_to_num((1 - rho) b2 + rho (beta2 + scale G)))
              pi_d <- (1 - rho) pi_d + rho dsum / n_B                                  (update_pi_d; else pi_d stays)
              then V_hat, log_V_hat from the pair.

Everything but the stated float32 casts (lu, d, log_V_hat) is float64.  The priors are not moved.
`population_bound` scores a state: the sum over a set of cells of each cell's collapsed ZI bound (zi_score_reference.cell_terms),
every cell folded in against the state's gene side, minus the gene side's Kullback-Leibler term.
"""
import numpy as np

import elbo_reference as er
import svi_reference as svi
import zi_foldin_reference as zr
import zi_score_reference as zs

PRIORS = ('alpha1', 'alpha2', 'beta1', 'beta2')
WARM_KEYS = PRIORS + ('b1', 'b2', 'pi_d', 'V_hat', 'log_V_hat')


def _f64(state, k):
    return np.asarray(state[k], dtype=np.float64)


def batch_statistics(X_B, V, lv, pi_d, a1, a2):
    """(Z_j, G, dsum) of step 2 at the pairs (a1, a2)."""
    X_B = np.asarray(X_B, dtype=np.float64)
    U = a1 / a2
    Z_j = svi.gene_sums(X_B, zr.elog_u(a1, a2), lv)
    d = zr.dropout_f32(X_B, V, pi_d, U).astype(np.float64)
    return Z_j, zr._dot(d.T, U), d.sum(axis=0)


def fold_in_fit(X_B, state, n_total, rho, a1_0=None, n_iter=300, tol=1e-4, update_pi_d=True):
    """(the new state, info): info = {a1, a2, froze_at, Z_j, G, dsum} of the batch.  The new state holds the priors of the old one,
    the blended b1, b2, pi_d and the V_hat / log_V_hat formed from the pair."""
    X_B = np.asarray(X_B, dtype=np.float64)
    n_B = X_B.shape[0]
    if n_total < n_B:
        raise ValueError('n_total < n_B')
    V, lv = svi.gene_side(state)
    alpha1, alpha2, pi_d = _f64(state, 'alpha1'), _f64(state, 'alpha2'), _f64(state, 'pi_d')
    s1, s2 = zr.default_start(X_B, alpha1, alpha2, V)
    if a1_0 is not None:
        s1 = np.maximum(1e-15, np.nan_to_num(np.asarray(a1_0, dtype=np.float64)))
    a1, a2, froze_at = zr.fold_in(X_B, lv, V, pi_d, alpha1, alpha2, s1, s2, n_iter, tol)
    Z_j, G, dsum = batch_statistics(X_B, V, lv, pi_d, a1, a2)
    new = {k: np.array(state[k], dtype=np.float64, copy=True) for k in PRIORS + ('b1', 'b2', 'pi_d')}
    if n_B > 0:
        scale = float(n_total) / n_B
        new['b1'] = svi.blend(state['b1'], new['beta1'][None, :] + scale * Z_j, rho)
        new['b2'] = svi.blend(state['b2'], new['beta2'][None, :] + scale * G, rho)
        if update_pi_d:
            new['pi_d'] = (1.0 - rho) * pi_d + rho * (dsum / n_B)
    new['V_hat'] = new['b1'] / new['b2']
    new['log_V_hat'] = svi.elog_v(new['b1'], new['b2'])
    return new, dict(a1=a1, a2=a2, froze_at=froze_at, Z_j=Z_j, G=G, dsum=dsum)


def population_bound(X, state, return_froze=False):
    """The collapsed ZI bound of the cells X under the state's gene side: every cell folded in from the default start at
    svi_reference.BOUND_TOL within BOUND_ITERS iterations, sum_i score_i - KL(q(V) || p(V))."""
    X = np.asarray(X, dtype=np.float64)
    V, lv = svi.gene_side(state)
    alpha1, alpha2, pi_d = _f64(state, 'alpha1'), _f64(state, 'alpha2'), _f64(state, 'pi_d')
    s1, s2 = zr.default_start(X, alpha1, alpha2, V)
    a1, a2, froze_at = zr.fold_in(X, lv, V, pi_d, alpha1, alpha2, s1, s2, svi.BOUND_ITERS, svi.BOUND_TOL)
    t = zs.cell_terms(X, zr.elog_u(a1, a2), lv, a1, a2, V, pi_d, alpha1, alpha2)
    kl_v = er.gamma_kl(state['b1'], state['b2'], state['beta1'], state['beta2'])[0]
    value = float(np.sum(np.asarray(t['score'], dtype=np.longdouble))) - kl_v
    return (value, froze_at) if return_froze else value


def warm_state(X, a1, b1, sweeps=40):
    """The float64 ZI fit of the first svi_reference.WARM_CELLS cells (zi_foldin_reference.float64_zi_sweeps) as a state, and the
    fit itself."""
    w = svi.WARM_CELLS
    fit = zr.float64_zi_sweeps(X[:w], a1[:w], b1, sweeps)
    return {k: fit[k] for k in WARM_KEYS}, fit


def stream(X, warm, n_calls, update_pi_d=True, n_iter=300, tol=1e-4):
    """The warm-started stream of the tests: svi_reference.stream_batches / stream_rho over the cells X.  (states [warm, after
    call 1, ...], infos)."""
    n = X.shape[0]
    states, infos = [warm], []
    for t, rows in enumerate(svi.stream_batches(n, n_calls)):
        new, info = fold_in_fit(X[rows], states[-1], n, svi.stream_rho(t), n_iter=n_iter, tol=tol, update_pi_d=update_pi_d)
        states.append(new)
        infos.append(info)
    return states, infos
