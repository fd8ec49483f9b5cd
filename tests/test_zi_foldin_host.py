# -*- coding: utf-8 -*-
"""The float64 reference of ZIGaP.fold_in (tests/zi_foldin_reference.py) on its own: no GPU.

The planted case (293 x 131, K = 3, per-gene dropout from U(0.5, 0.95)) is fitted for 40 float64 ZI sweeps, then 150 fresh
cells drawn from the fitted gene side (one of them all-zero) are folded in at tol = 1e-4.  Every cell must freeze within 300
iterations: the cap is a condition of the test, not a measurement (the map met it with every cell frozen by iteration 80)."""
import numpy as np
import pytest

import zi_foldin_reference as zr

TOL = 1e-4
N_ITER = 300
ZERO_CELL = 23


def _args(fit):
    return fit['log_V_hat'], fit['V_hat'], fit['pi_d'], fit['alpha1'], fit['alpha2']


@pytest.fixture(scope='module')
def planted_fold_in():
    _, fit, Xq = zr.planted_case(zero_cell=ZERO_CELL)
    s1, s2 = zr.default_start(Xq, fit['alpha1'], fit['alpha2'], fit['V_hat'])
    a1q, a2q, froze = zr.fold_in(Xq, *_args(fit), s1, s2, N_ITER, TOL)
    return fit, Xq, s1, s2, a1q, a2q, froze


def test_every_cell_freezes(planted_fold_in):
    fit, Xq, s1, s2, a1q, a2q, froze = planted_fold_in
    print('freeze iterations: min %d median %d max %d, %d distinct' % (froze.min(), np.median(froze), froze.max(),
                                                                       np.unique(froze).size))
    assert froze.max() < N_ITER, '%d cells never froze' % int((froze == N_ITER).sum())
    assert np.unique(froze).size > 1, 'every cell froze at the same iteration'
    assert np.isfinite(a1q).all() and (a1q >= 1e-15).all() and np.isfinite(a2q).all() and (a2q >= 1e-15).all()
    # the dropout posterior takes rate away: the fitted rates sit below the pCMF rate the cells started from
    assert (a2q <= s2 * (1 + 1e-12)).all() and (a2q < s2).any()


def test_all_zero_cell(planted_fold_in):
    fit, Xq, s1, s2, a1q, a2q, froze = planted_fold_in
    assert not Xq[ZERO_CELL].any()
    assert np.array_equal(a1q[ZERO_CELL], np.maximum(1e-15, fit['alpha1']))


def test_frozen_cells_are_fixed_points_within_tol(planted_fold_in):
    fit, Xq, s1, s2, a1q, a2q, froze = planted_fold_in
    n1, n2 = zr.T64(Xq, *_args(fit), a1q, a2q)
    assert np.all(np.abs(n1 - a1q) <= TOL * a1q) and np.all(np.abs(n2 - a2q) <= TOL * a2q)


def test_a_longer_budget_changes_nothing(planted_fold_in):
    """Frozen cells are never rewritten: a longer budget, and folding in a subset, give the same rows bit for bit."""
    fit, Xq, s1, s2, a1q, a2q, froze = planted_fold_in
    b1, b2, fr = zr.fold_in(Xq, *_args(fit), s1, s2, N_ITER + 50, TOL)
    assert np.array_equal(b1, a1q) and np.array_equal(b2, a2q) and np.array_equal(fr, froze)
    sub = np.array([0, 5, ZERO_CELL, 77, 149])
    c1, c2, frs = zr.fold_in(Xq[sub], *_args(fit), s1[sub], s2[sub], N_ITER + 50, TOL)
    assert np.array_equal(c1, a1q[sub]) and np.array_equal(c2, a2q[sub]) and np.array_equal(frs, froze[sub])


def test_one_update_is_the_sweeps_cell_update():
    """T64 on the training cells, from the state a sweep starts in, gives that sweep's a1, up to the float32 cast of
    E[log U] that the float64 sweeps do not make."""
    (X, a1, b1, K), _, _ = zr.planted_case(zero_cell=ZERO_CELL)
    f0 = zr.float64_zi_sweeps(X, a1, b1, 3)
    f1 = zr.float64_zi_sweeps(X, a1, b1, 4)
    # (a1 only: the sweep's rate reads the D_hat its predecessor stored, formed with the pi_d of BEFORE that sweep's M-step, while
    #  T64 forms the posterior from the state at hand -- the rate halves agree at a fixed point of the fit, not sweep by sweep)
    n1, _ = zr.T64(X, f0['log_V_hat'], f0['V_hat'], f0['pi_d'], f0['alpha1'], f0['alpha2'], f0['a1'], f0['a2'])
    err = np.max(np.abs(n1 - f1['a1']) / (np.abs(f1['a1']) + f1['a1'].max(axis=0)))
    print('T64 a1 against the float64 sweep: %.3e' % err)
    assert err <= 1e-5
