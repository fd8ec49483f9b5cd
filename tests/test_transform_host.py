# -*- coding: utf-8 -*-
"""The float64 reference of GaP.transform (tests/transform_reference.py) on its own: no GPU.

The planted case of tests/test_elbo_gpu._planted (293 x 131, K = 3) is fitted for 40 float64 sweeps, then 150 fresh cells
drawn from the fitted gene side (one of them all-zero) are folded in at tol = 1e-4.  Every cell must freeze within 300
iterations: the cap is a condition of the test, not a measurement."""
import numpy as np
import pytest

import transform_reference as tr
from test_elbo_gpu import _planted

TOL = 1e-4
N_ITER = 300
ZERO_CELL = 23


@pytest.fixture(scope='module')
def planted_fold_in():
    X, a1, b1, K = _planted()
    fit = tr.float64_sweeps(X, a1, b1, 40)
    Xq = tr.planted_query(fit, zero_cell=ZERO_CELL)
    a2_row = np.maximum(1e-15, fit['alpha2'] + fit['sum_V'])
    start = tr.default_start(Xq, fit['alpha1'])
    a1q, froze = tr.fold_in(Xq, fit['log_V_hat'], fit['alpha1'], a2_row, start, N_ITER, TOL)
    return fit, Xq, a2_row, start, a1q, froze


def test_every_cell_freezes(planted_fold_in):
    fit, Xq, a2_row, start, a1q, froze = planted_fold_in
    print('freeze iterations: min %d median %d max %d' % (froze.min(), np.median(froze), froze.max()))
    assert froze.max() < N_ITER, '%d cells never froze' % int((froze == N_ITER).sum())
    assert np.unique(froze).size > 1, 'every cell froze at the same iteration'
    assert np.isfinite(a1q).all() and (a1q >= 1e-15).all()


def test_frozen_cells_are_fixed_points_within_tol(planted_fold_in):
    fit, Xq, a2_row, start, a1q, froze = planted_fold_in
    new = tr.T64(Xq, fit['log_V_hat'], fit['alpha1'], a2_row, a1q)
    assert np.all(np.abs(new - a1q) <= TOL * a1q)


def test_all_zero_cell(planted_fold_in):
    fit, Xq, a2_row, start, a1q, froze = planted_fold_in
    assert not Xq[ZERO_CELL].any()
    assert np.array_equal(a1q[ZERO_CELL], np.maximum(1e-15, fit['alpha1'])) and froze[ZERO_CELL] == 0


def test_a_frozen_cell_does_not_depend_on_the_others(planted_fold_in):
    """Folding in a subset gives bit for bit the rows of the full run, and so does a larger n_iter."""
    fit, Xq, a2_row, start, a1q, froze = planted_fold_in
    sub = np.array([0, 5, ZERO_CELL, 77, 149])
    a1s, frs = tr.fold_in(Xq[sub], fit['log_V_hat'], fit['alpha1'], a2_row, start[sub], N_ITER + 50, TOL)
    assert np.array_equal(a1s, a1q[sub]) and np.array_equal(frs, froze[sub])


def test_one_update_is_the_sweeps_cell_update():
    """T64 on the training cells, from the state a sweep starts in, is that sweep's a1 (float64 up to the float32 cast of
    E[log U], which the float64 sweep above does not make)."""
    X, a1, b1, K = _planted()
    f0 = tr.float64_sweeps(X, a1, b1, 3)
    f1 = tr.float64_sweeps(X, a1, b1, 4)
    # the fourth sweep reads E[log U] = psi(a1) - log a2 with the a2 the THIRD sweep stored (alpha2 and sum_j V_hat of its
    # start), not alpha2 + sum_j V_hat of the state at hand: feed T64 that rate
    got = tr.T64(X, f0['log_V_hat'], f0['alpha1'], f0['a2'][0], f0['a1'])
    err = np.max(np.abs(got - f1['a1']) / (np.abs(f1['a1']) + f1['a1'].max(axis=0)))
    print('T64 against the float64 sweep: %.3e' % err)
    assert err <= 1e-5
