# -*- coding: utf-8 -*-
"""The float64 reference of GaP.partial_fit (tests/svi_reference.py) on its own: no GPU.

The warm-started stream: the planted case of tests/test_elbo_gpu._planted (293 x 131, K = 3); the gene side is fitted for 40
float64 sweeps on the first 73 cells only, its priors are kept, and the 293 cells are then streamed in batches of 73 (per epoch
one permutation of default_rng(3), the 1-cell remainder dropped) with rho_t = (1 + t) ** -0.7.  Each state is scored by the
collapsed bound of all 293 cells folded in against it.  The 300-iteration budget and the ordering of the bounds are conditions
of the test, not measurements."""
import numpy as np
import pytest

import svi_reference as svi
import transform_reference as tr
from test_elbo_gpu import _planted

TOL = 1e-4
N_ITER = 300


@pytest.fixture(scope='module')
def stream():
    X, a1, b1, K = _planted()
    warm, fit = svi.warm_state(X, a1, b1)
    states, infos = [warm], []
    for t, rows in enumerate(svi.stream_batches(X.shape[0], 8)):
        new, info = svi.partial_fit(X[rows], states[-1], X.shape[0], svi.stream_rho(t), n_iter=N_ITER, tol=TOL)
        states.append(new)
        infos.append(info)
    return X, fit, states, infos


def test_every_cell_of_every_batch_freezes(stream):
    X, fit, states, infos = stream
    worst = [int(i['froze_at'].max()) for i in infos]
    print('latest freeze per batch: %r' % worst)
    assert all(w < N_ITER for w in worst)
    assert all(i['a1'].shape == (svi.WARM_CELLS, 3) and np.isfinite(i['a1']).all() for i in infos)


def test_the_population_bound_rises_along_the_stream(stream):
    X, fit, states, infos = stream
    vals, froze = zip(*(svi.population_bound(X, states[t], return_froze=True) for t in (0, 4, 8)))
    print('population bound: warm %.1f, after 4 batches %.1f, after 8 batches %.1f' % vals)
    assert all(f.max() < svi.BOUND_ITERS for f in froze), 'a cell of the scoring fold-in never froze'
    assert vals[0] < vals[1] < vals[2]


def test_the_priors_are_not_moved(stream):
    X, fit, states, infos = stream
    for k in ('alpha1', 'alpha2', 'beta1', 'beta2'):
        assert all(np.array_equal(s[k], states[0][k]) for s in states), k


def test_rho_zero_returns_the_gene_side_bit_for_bit(stream):
    X, fit, states, infos = stream
    new, info = svi.partial_fit(X[100:173], states[0], X.shape[0], 0.0, n_iter=N_ITER, tol=TOL)
    assert np.array_equal(new['b1'], states[0]['b1']) and np.array_equal(new['b2'], states[0]['b2'])
    assert info['Z_j'].sum() > 0                     # (the statistics were formed; the step size alone kept them out)


def test_rho_one_on_the_training_cells_is_the_batch_estimate(stream):
    """rho = 1, n_total = n_B, the batch the cells the gene side was fitted on: b1 = beta1 + Z_j exactly (scale = 1, the old
    value multiplied by 0), and the same for b2."""
    X, fit, states, infos = stream
    Xw = X[:svi.WARM_CELLS]
    new, info = svi.partial_fit(Xw, states[0], svi.WARM_CELLS, 1.0, n_iter=N_ITER, tol=TOL)
    assert np.array_equal(new['b1'], np.maximum(1e-15, states[0]['beta1'][None, :] + info['Z_j']))
    assert np.array_equal(new['b2'], np.broadcast_to(np.maximum(1e-15, states[0]['beta2'] + info['sum_u']), new['b2'].shape))


def test_n_total_below_the_batch_is_refused(stream):
    X, fit, states, infos = stream
    with pytest.raises(ValueError):
        svi.partial_fit(X[:10], states[0], 9, 0.5)
