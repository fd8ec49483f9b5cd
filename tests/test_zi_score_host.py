# -*- coding: utf-8 -*-
"""The per-cell bound of ZIGaP.fold_in_score_samples without a GPU: the float64 reference of tests/zi_score_reference.py does
not decrease along the fold-in map, reduces to the pCMF score when no gene drops out, stays finite at the edges, and the new C
entry checks its arguments before any HIP call."""
import ctypes

import numpy as np
import pytest

import score_reference as sr
import zi_foldin_reference as zr
import zi_score_reference as zs

ZERO_CELL = 23


def _terms(Xq, fit, a1, a2, pi_d=None):
    return zs.cell_terms(Xq, zr.elog_u(a1, a2), fit['log_V_hat'], a1, a2, fit['V_hat'], fit['pi_d'] if pi_d is None else pi_d,
                         fit['alpha1'], fit['alpha2'])


def test_score_does_not_decrease_along_the_fold_in():
    """The map T of fold_in() takes q(Z) and q(d) at their optimum for the pair that enters and moves (a1, a2) to their joint
    optimum under those: iterations 0 .. 60 of the planted case from the default start, every cell, every step.  What a step may
    lose is the map's own float32 casts of E[log U] and d (1.2e-4 nats at worst here): it sits inside the evaluation bounds of the
    two values, which is all the allowance there is."""
    (X, a1, b1, K), fit, Xq = zr.planted_case(zero_cell=ZERO_CELL)
    a, b = zr.default_start(Xq, fit['alpha1'], fit['alpha2'], fit['V_hat'])
    worst, worst_share, prev, first = 0.0, 0.0, None, None
    for it in range(61):
        t = _terms(Xq, fit, a, b)
        assert all(np.isfinite(t[k]).all() for k in zs.CELL_TERMS + ('score',))
        if prev is not None:
            d = t['score'] - prev['score']
            allow = zs.cell_bounds(prev, K)['score'] + zs.cell_bounds(t, K)['score']
            worst, worst_share = min(worst, d.min()), max(worst_share, (-d / allow).max())
            assert np.all(d >= -allow), 'iteration %d: cells %r dropped by %r (allowed %r)' % (
                it, np.nonzero(d < -allow)[0], d[d < -allow], allow[d < -allow])
        else:
            first = t
        if it in (0, 1, 2, 5, 20, 60):
            print('iteration %d: mean score %.4f' % (it, t['score'].mean()))
        assert t['data'][ZERO_CELL] == 0 and t['lgamma'][ZERO_CELL] == 0
        prev = t
        a, b = zr.T64(Xq, fit['log_V_hat'], fit['V_hat'], fit['pi_d'], fit['alpha1'], fit['alpha2'], a, b)
    print('worst step %.3e nats (%.1f %% of its allowance); mean score %.4f -> %.4f; the all-zero cell: %.4f' % (
        worst, 100 * worst_share, first['score'].mean(), prev['score'].mean(), prev['score'][ZERO_CELL]))
    assert prev['score'].mean() > first['score'].mean()
    assert np.isfinite(prev['score'][ZERO_CELL]) and not Xq[ZERO_CELL].any()


def test_without_dropout_it_is_the_pcmf_score():
    """Every pi_d = 1 (pi~ = 1 - 1e-10) and U_hat scaled so that Lambda <= 5: the value is score_reference's pCMF score at the
    same pair; per entry the two differ by at most 1e-10 e^Lambda."""
    (X, a1, b1, K), fit, Xq = zr.planted_case(zero_cell=ZERO_CELL)
    m = Xq.shape[1]
    rng = np.random.default_rng(3)
    a = rng.gamma(1.0, 1.0, size=(Xq.shape[0], K)) + 0.1
    sum_v = fit['V_hat'].sum(axis=0)
    a2_row = np.maximum(1e-15, fit['alpha2'] + sum_v)
    a2_row = a2_row * max(1.0, ((a / a2_row) @ fit['V_hat'].T).max() / 5.0)
    b = np.broadcast_to(a2_row, a.shape).copy()
    assert ((a / b) @ fit['V_hat'].T).max() <= 5.0 + 1e-12
    lu = zr.elog_u(a, b)
    zi = zs.cell_terms(Xq, lu, fit['log_V_hat'], a, b, fit['V_hat'], np.ones(m), fit['alpha1'], fit['alpha2'])
    pc = sr.cell_terms(Xq, lu, fit['log_V_hat'], a, a2_row, sum_v, fit['alpha1'], fit['alpha2'])
    d = np.abs(zi['score'] - pc['score'])
    tol = m * 1e-10 * np.exp(5.0)
    print('largest difference %.3e (bound %.3e)' % (d.max(), tol))
    assert np.all(d <= tol)
    assert np.all(np.abs(zi['dropout'] + pc['product']) <= tol)
    for k in ('data', 'lgamma', 'kl'):
        assert np.array_equal(zi[k], pc[k]), k


def test_edges_are_finite():
    """The all-zero cell; a cell that expresses a gene whose pi_d is 0 (log pi~ = log 1e-10, not -inf); pi_d = 1 (log(1 - pi~) =
    log 1e-10); large Lambda at both kinds of entry."""
    (X, a1, b1, K), fit, Xq = zr.planted_case(zero_cell=ZERO_CELL)
    Xq = np.array(Xq)
    pi_d = np.array(fit['pi_d'])
    pi_d[4], pi_d[9] = 0.0, 1.0
    Xq[2, 4] = 3.0
    assert pi_d[4] == 0 and Xq[2, 4] != 0 and not Xq[ZERO_CELL].any()
    a, b = zr.default_start(Xq, fit['alpha1'], fit['alpha2'], fit['V_hat'])
    a[5] *= 200.0                                             # Lambda of a few hundred: softplus at both ends
    t = _terms(Xq, fit, a, b, pi_d=pi_d)
    for k in zs.CELL_TERMS + ('score',):
        assert np.isfinite(t[k]).all(), k
    bd = zs.cell_bounds(t, K)
    assert all(np.isfinite(bd[k]).all() and (bd[k] >= 0).all() for k in zs.CELL_TERMS + ('score',))
    # the expressed gene with pi_d = 0 costs the cell log(1e-10) - Lambda against a gene it could drop out of
    s, Lam, lg, g = zs.dropout_sums(Xq, fit['V_hat'], pi_d, a / b)
    assert g[2, 4] == lg[4] - Lam[2, 4] and abs(lg[4] - np.log(1e-10)) < 1e-9
    assert np.all(g[Xq == 0] >= 0)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    return ctypes.CDLL(g.build())


def test_new_entry_checks_its_arguments_without_gpu(lib):
    """As test_abi.test_argument_errors_without_gpu: validation comes before any HIP call."""
    P, I = ctypes.c_void_p, ctypes.c_int64
    f = lib.oriana_zi_cell_bound
    f.restype, f.argtypes = ctypes.c_int, [P] * 6 + [I, I, I, I, P]
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    assert f(p, p, p, p, p, p, 4, 8, 8, 129, None) == -2         # ORIANA_EKRANGE
    assert f(p, p, p, p, p, p, 4, 8, 8, 0, None) == -1           # ORIANA_EINVAL: K <= 0
    assert f(p, p, p, p, p, p, 4, 8, 8, -3, None) == -1
    assert f(p, p, p, p, p, p, -1, 8, 8, 3, None) == -1
    assert f(p, p, p, p, p, p, 4, -8, 0, 3, None) == -1
    assert f(p, p, p, p, p, p, 4, 8, 9, 3, None) == -1           # more real genes than genes
    for miss in range(6):
        args = [p, p, p, p, p, p, 4, 8, 8, 3, None]
        args[miss] = None
        assert f(*args) == -1, miss                              # a missing pointer
    assert f(None, None, None, None, None, None, 0, 8, 8, 3, None) == 0      # no cells: nothing to do
    s = lib.oriana_zi_cell_bound_scratch_doubles
    s.restype, s.argtypes = I, [I, I, I]
    assert s(0, 8, 3) == 0 and s(4, 0, 3) == 0 and s(4, 8, 0) == 0 and s(4, 8, 129) == 0 and s(-1, 8, 3) == 0
