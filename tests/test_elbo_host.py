# -*- coding: utf-8 -*-
"""The formula of the variational bound itself, without a GPU: the collapsed form that GaP.elbo evaluates
(tests/elbo_reference.py) against the uncollapsed bound with an explicit optimal multinomial q(Z)."""
import numpy as np
from scipy.special import psi

import elbo_reference as er


def _case(seed=0, n=40, m=30, K=3):
    rng = np.random.default_rng(seed)
    X = (rng.poisson(3.0, size=(n, m)) * (rng.random((n, m)) < 0.4)).astype(np.float64)
    X[:, 4] = 0
    X[7, :] = 0
    st = dict(a1=rng.gamma(2.0, 1.0, size=(n, K)), a2=rng.gamma(3.0, 0.5, size=(n, K)),
              b1=rng.gamma(2.0, 1.0, size=(m, K)), b2=rng.gamma(3.0, 0.5, size=(m, K)),
              alpha1=rng.gamma(2.0, 1.0, size=K), alpha2=rng.gamma(2.0, 1.0, size=K),
              beta1=rng.gamma(2.0, 1.0, size=K), beta2=rng.gamma(2.0, 1.0, size=K))
    st['U_hat'] = st['a1'] / st['a2']
    st['V_hat'] = st['b1'] / st['b2']
    st['log_U_hat'] = psi(st['a1']) - np.log(st['a2'])
    st['log_V_hat'] = psi(st['b1']) - np.log(st['b2'])
    return X, st


def test_collapsed_bound_equals_uncollapsed_bound_at_the_optimal_qz():
    X, st = _case()
    t = er.elbo_terms(X, st)
    full = er.uncollapsed_elbo(X, st['log_U_hat'], st['log_V_hat'], st['U_hat'], st['V_hat'], t['kl_u'], t['kl_v'])
    assert np.isfinite(full) and np.isfinite(t['elbo'])
    assert abs(t['elbo'] - full) <= 1e-10 * abs(full), (t['elbo'], full)


def test_optimal_qz_maximises_the_uncollapsed_bound():
    """Any other q(Z) gives a smaller value: collapsing can only raise the bound (what makes the collapsed value monotone)."""
    X, st = _case(1)
    t = er.elbo_terms(X, st)
    rng = np.random.default_rng(2)
    lu = st['log_U_hat'] + 0.3 * rng.standard_normal(st['log_U_hat'].shape)      # a q(Z) built from other logs
    S = lu[:, None, :] + st['log_V_hat'][None, :, :]
    r = np.exp(S - S.max(axis=2, keepdims=True))
    r /= r.sum(axis=2, keepdims=True)
    S0 = st['log_U_hat'][:, None, :] + st['log_V_hat'][None, :, :]
    other = (er._ld(X[:, :, None] * r * (S0 - np.log(r))) - t['lgamma'] - t['product'] - t['kl_u'] - t['kl_v'])
    assert other < t['elbo']


def test_gamma_kl_is_zero_at_the_prior_and_positive_elsewhere():
    p1, p2 = np.array([0.7, 2.0, 30.0]), np.array([1.5, 0.2, 4.0])
    kl, _ = er.gamma_kl(np.tile(p1, (5, 1)), np.tile(p2, (5, 1)), p1, p2)
    assert abs(kl) <= 1e-12
    kl, _ = er.gamma_kl(np.tile(p1 * 1.3, (5, 1)), np.tile(p2 * 0.8, (5, 1)), p1, p2)
    assert kl > 0
    # against a quadrature of the definition for one pair
    from scipy import integrate, stats
    q, p = stats.gamma(a=1.7, scale=1 / 2.5), stats.gamma(a=0.9, scale=1 / 0.6)
    num, _ = integrate.quad(lambda u: q.pdf(u) * (q.logpdf(u) - p.logpdf(u)), 0, np.inf)
    kl, _ = er.gamma_kl(np.array([[1.7]]), np.array([[2.5]]), np.array([0.9]), np.array([0.6]))
    assert abs(kl - num) <= 1e-7 * abs(num)
