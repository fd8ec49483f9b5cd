# -*- coding: utf-8 -*-
"""The per-cell bound of GaP.score_samples without a GPU: the float64 reference of tests/score_reference.py adds up to the
bound of tests/elbo_reference.py, it does not decrease along a fold-in, and the two new C entries check their arguments
before any HIP call."""
import ctypes

import numpy as np
import pytest

import elbo_reference as er
import score_reference as sr
import transform_reference as tr
from test_elbo_gpu import _planted, _small

ZERO_CELL = 23


def test_cell_terms_add_up_to_the_bound():
    """On a model's own cells, with its own a1, rate and float32 E[log U], the four per-cell terms summed over the cells are
    the first four terms of the bound, and sum_i score_i - KL_V is the bound."""
    X, a1, b1, K = _small()
    X[17, :] = 0
    fit = tr.float64_sweeps(X, a1, b1, 2)
    a2_row = fit['a2'][0]
    assert np.array_equal(fit['a2'], np.broadcast_to(a2_row, fit['a2'].shape))
    st = dict(fit, U_hat=fit['a1'] / fit['a2'], log_U_hat=tr.elog_u(fit['a1'], a2_row))
    ref = er.elbo_terms(X, st)
    t = sr.cell_terms(X, st['log_U_hat'], st['log_V_hat'], st['a1'], a2_row, fit['sum_V'], st['alpha1'], st['alpha2'])
    for cell, whole in zip(sr.CELL_TERMS, er.TERMS[:4]):
        got, tol = er._ld(t[cell]), 1e-12 * ref['abs'][whole]
        print('%s: cells %.17g whole %.17g (bound %.3e)' % (cell, got, ref[whole], tol))
        assert abs(got - ref[whole]) <= tol
        assert abs(er._ld(t['abs'][cell]) - ref['abs'][whole]) <= 1e-12 * ref['abs'][whole]
    assert abs(er._ld(t['score']) - ref['kl_v'] - ref['elbo']) <= 1e-12 * sum(ref['abs'].values())
    assert abs(er._ld(t['sum_x']) - ref['sum_x']) <= 1e-12 * ref['sum_x']
    assert t['data'][17] == 0 and t['lgamma'][17] == 0 and t['sum_x'][17] == 0
    b = sr.cell_bounds(t, K)
    assert all(b[k].shape == (X.shape[0],) and (b[k] >= 0).all() for k in sr.CELL_TERMS + ('score',))
    assert np.all(b['score'] >= b['data']) and np.all(b['data'][t['sum_x'] > 0] > 0)


def test_score_does_not_decrease_along_the_fold_in():
    """One fold-in iteration is exact coordinate ascent on a cell's score (the rate is already the optimal one): iterations
    0 .. 40 of the planted case from the default start, every cell, every step, in float64."""
    X, a1, b1, K = _planted()
    fit = tr.float64_sweeps(X, a1, b1, 40)
    Xq = tr.planted_query(fit, zero_cell=ZERO_CELL)
    a2_row = np.maximum(1e-15, fit['alpha2'] + fit['sum_V'])
    a = tr.default_start(Xq, fit['alpha1'])
    worst, worst_share, prev, first = 0.0, 0.0, None, None
    for it in range(41):
        lu = tr.elog_u(a, a2_row)
        t = sr.cell_terms(Xq, lu, fit['log_V_hat'], a, a2_row, fit['sum_V'], fit['alpha1'], fit['alpha2'])
        if prev is not None:
            d = t['score'] - prev[0]['score']
            allow = sr.monotone_allowance(prev[0], t, prev[1], lu, K)
            worst, worst_share = min(worst, d.min()), max(worst_share, (-d / allow).max())
            assert np.all(d >= -allow), 'iteration %d: cells %r dropped by %r (allowed %r)' % (
                it, np.nonzero(d < -allow)[0], d[d < -allow], allow[d < -allow])
        else:
            first = t
        # the all-zero cell sits at the prior's shape from the start on: no data, exactly -(product + kl)
        assert np.array_equal(a[ZERO_CELL], fit['alpha1'])
        assert t['data'][ZERO_CELL] == 0 and t['score'][ZERO_CELL] == -(t['product'][ZERO_CELL] + t['kl'][ZERO_CELL])
        prev = (t, lu)
        a = tr.T64(Xq, fit['log_V_hat'], fit['alpha1'], a2_row, a)
    print('worst step %.3e (%.1f %% of its allowance); mean score %.6f -> %.6f' % (worst, 100 * worst_share,
                                                                                  first['score'].mean(), t['score'].mean()))
    assert t['score'].mean() > first['score'].mean()


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    return ctypes.CDLL(g.build())


def test_new_entries_check_their_arguments_without_gpu(lib):
    """As test_abi.test_argument_errors_without_gpu: validation comes before any HIP call."""
    from oriana_amd._lib import OrianaCounts
    P, I = ctypes.c_void_p, ctypes.c_int64
    f = lib.oriana_cell_bound_nnz
    f.restype, f.argtypes = ctypes.c_int, [ctypes.POINTER(OrianaCounts), P, P, P, P, P, I, P, P]
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    empty = OrianaCounts()                                   # zero-initialised: no rows, no tiles
    assert f(None, p, p, p, p, p, 3, p, None) == -1          # ORIANA_EINVAL: no layout
    assert f(ctypes.byref(empty), p, p, p, p, p, 0, p, None) == -1           # K <= 0
    assert f(ctypes.byref(empty), p, p, p, p, p, -2, p, None) == -1
    for miss in range(1, 8):
        if miss == 6:
            continue
        args = [ctypes.byref(empty), p, p, p, p, p, 3, p, None]
        args[miss] = None
        assert f(*args) == -1, miss                          # a missing pointer
    assert f(ctypes.byref(empty), p, p, p, p, p, 3, p, None) == 0            # an empty layout is fine
    g = lib.oriana_gamma_kl_rows
    g.restype, g.argtypes = ctypes.c_int, [P, P, P, ctypes.c_int, P, P, I, I, P]
    assert g(p, p, p, 1, p, p, -1, 3, None) == -1
    assert g(p, p, p, 1, p, p, 4, 0, None) == -1
    assert g(p, p, p, 1, p, p, 4, 1025, None) == -1
    for miss in (0, 1, 2, 4, 5):
        args = [p, p, p, 1, p, p, 4, 3, None]
        args[miss] = None
        assert g(*args) == -1, miss
    assert g(None, None, None, 0, None, None, 0, 3, None) == 0               # no rows: nothing to do
