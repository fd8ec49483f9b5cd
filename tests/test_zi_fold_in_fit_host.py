# -*- coding: utf-8 -*-
"""The float64 restatement of ZIGaP.fold_in_fit (tests/zi_svi_reference.py) on its own: no GPU.

The warm-started stream: the planted case of tests/zi_foldin_reference.planted_case (293 x 131, K = 3, dropouts); the gene side is
fitted for 40 float64 ZI sweeps on the first 73 cells only, its priors are kept, and the 293 cells are then streamed in batches of
73 (svi_reference.stream_batches: per epoch one permutation of default_rng(3), the 1-cell remainder dropped) with
rho_t = (1 + t) ** -0.7.  Each state is scored by the sum of the collapsed ZI cell bounds of all 293 cells folded in against it
minus KL_V.  The 300-iteration budget, the batch order and the ordering of the bounds are conditions of the test, not
measurements (observed: the latest freeze at iteration 107; the bound rises at every checkpoint in both variants)."""
import numpy as np
import pytest

import svi_reference as svi
import zi_foldin_reference as zr
import zi_svi_reference as zsvi

TOL = 1e-4
N_ITER = 300
CHECKPOINTS = (1, 2, 4, 8)


@pytest.fixture(scope='module')
def case():
    (X, a1, b1, K), _, _ = zr.planted_case()
    warm, fit = zsvi.warm_state(X, a1, b1)
    return X, K, warm


@pytest.fixture(scope='module', params=[True, False], ids=['pi_d-blended', 'pi_d-fixed'])
def stream(request, case):
    X, K, warm = case
    states, infos = zsvi.stream(X, warm, 8, update_pi_d=request.param, n_iter=N_ITER, tol=TOL)
    return X, states, infos, request.param


def test_every_cell_of_every_batch_freezes(stream):
    X, states, infos, _ = stream
    worst = [int(i['froze_at'].max()) for i in infos]
    print('latest freeze per batch: %r' % worst)
    assert all(w < N_ITER for w in worst)
    assert all(i[k].shape == (svi.WARM_CELLS, 3) and np.isfinite(i[k]).all() for i in infos for k in ('a1', 'a2'))


def test_the_population_bound_rises_along_the_stream(stream):
    X, states, infos, blended = stream
    vals, froze = zip(*(zsvi.population_bound(X, states[t], return_froze=True) for t in (0,) + CHECKPOINTS))
    print('population bound (%s): warm %.1f, after calls 1, 2, 4, 8: %s'
          % ('pi_d blended' if blended else 'pi_d fixed', vals[0], ' '.join('%.1f' % v for v in vals[1:])))
    assert all(f.max() < svi.BOUND_ITERS for f in froze), 'a cell of the scoring fold-in never froze'
    for before, after in zip(vals[:-1], vals[1:]):
        assert after > before and after > vals[0]


def test_the_priors_are_not_moved_and_pi_d_follows_the_switch(stream):
    X, states, infos, blended = stream
    for k in zsvi.PRIORS:
        assert all(np.array_equal(s[k], states[0][k]) for s in states), k
    same = [np.array_equal(s['pi_d'], states[0]['pi_d']) for s in states[1:]]
    assert not any(same) if blended else all(same)
    assert all(((s['pi_d'] >= 0) & (s['pi_d'] <= 1)).all() for s in states)


def test_rho_zero_returns_the_state_bit_for_bit(case):
    X, K, warm = case
    new, info = zsvi.fold_in_fit(X[100:173], warm, X.shape[0], 0.0, n_iter=N_ITER, tol=TOL)
    for k in ('b1', 'b2', 'pi_d'):
        assert np.array_equal(new[k], warm[k]), k
    assert info['Z_j'].sum() > 0 and info['G'].sum() > 0           # (the statistics were formed; the step size alone kept them out)


def test_rho_one_at_scale_one_is_the_batch_estimate(case):
    """rho = 1, n_total = n_B: b1 = beta1 + Z_j, b2 = beta2 + G, pi_d = dsum / n_B exactly (the old value multiplied by 0)."""
    X, K, warm = case
    w = svi.WARM_CELLS
    new, info = zsvi.fold_in_fit(X[:w], warm, w, 1.0, n_iter=N_ITER, tol=TOL)
    assert np.array_equal(new['b1'], np.maximum(1e-15, warm['beta1'][None, :] + info['Z_j']))
    assert np.array_equal(new['b2'], np.maximum(1e-15, warm['beta2'][None, :] + info['G']))
    assert np.array_equal(new['pi_d'], info['dsum'] / w)
    # d is 1 at every non-zero count and a probability elsewhere
    nnz = (X[:w] != 0).sum(axis=0)
    assert (info['dsum'] >= nnz).all() and (info['dsum'] <= w).all()


def test_pi_d_one_is_the_pcmf_map(case):
    """pi_d = 1 in every gene: d = float32(1 - 1e-10) = 1 everywhere, the cell rate is alpha2 + sum_j V_hat and the gene rate the
    column sums of U_hat -- svi_reference.partial_fit on the same batch."""
    X, K, warm = case
    st = dict(warm, pi_d=np.ones_like(warm['pi_d']))
    rows = svi.stream_batches(X.shape[0], 1)[0]
    got, gi = zsvi.fold_in_fit(X[rows], st, X.shape[0], 0.6, n_iter=N_ITER, tol=TOL)
    ref, ri = svi.partial_fit(X[rows], {k: st[k] for k in st if k != 'pi_d'}, X.shape[0], 0.6, n_iter=N_ITER, tol=TOL)
    assert np.array_equal(gi['froze_at'], ri['froze_at'])
    for k in ('b1', 'b2'):
        e = float(np.max(np.abs(got[k] - ref[k]) / np.abs(ref[k])))
        print('%s: %.3e relative (bound 1e-12)' % (k, e))
        assert e <= 1e-12, k
    assert np.array_equal(gi['dsum'], np.full(X.shape[1], float(len(rows)))) and np.array_equal(got['pi_d'], st['pi_d'])


def test_no_cells_change_nothing(case):
    X, K, warm = case
    new, info = zsvi.fold_in_fit(X[:0], warm, 10, 1.0)
    for k in ('b1', 'b2', 'pi_d') + zsvi.PRIORS:
        assert np.array_equal(new[k], warm[k]), k
    assert info['a1'].shape == (0, K)


def test_n_total_below_the_batch_is_refused(case):
    X, K, warm = case
    with pytest.raises(ValueError):
        zsvi.fold_in_fit(X[:10], warm, 9, 0.5)
