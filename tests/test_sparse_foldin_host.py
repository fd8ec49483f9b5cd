# -*- coding: utf-8 -*-
"""The float64 reference of SparseGaP.project() / SparseZIGaP.project() (tests/sparse_foldin_reference.py) on its own: no GPU.

The planted case (293 x 131, K = 3, gene loadings present with probability 0.6) is fitted for 40 sweeps of the sparse model with
the loop nest in float64 -- about a third of the genes end up with every factor masked, most others keep one or two -- then 150
fresh cells drawn from the fitted gene side (one of them all-zero) are folded in at tol = 1e-4 from the masked-uniform start.
Every cell must freeze within 300 iterations: the cap is a condition of the test, not a measurement."""
import numpy as np
import pytest

import sparse_foldin_reference as sr
import transform_reference as tr
import zi_foldin_reference as zr

TOL = 1e-4
N_ITER = 300
ZERO_CELL = 23


def _gene_side(fit):
    St, Sh = sr.masks(fit['p_s'])
    return fit['log_V_hat'], St, Sh


def _fold(fit, Xq, n_iter, zi, rows=None):
    """(a1, a2 -- the K-vector for sparse pCMF --, froze_at) from the default start; `rows`: fold in that subset alone."""
    lv, St, Sh = _gene_side(fit)
    a2r = sr.a2_row(fit['alpha2'], Sh, fit['V_hat'])
    X = Xq if rows is None else Xq[rows]
    s1 = sr.default_start(X, fit['alpha1'], St, Sh)
    if zi:
        s2 = a2r[None, :] * np.ones((X.shape[0], 1))
        return sr.fold_in_zi(X, lv, St, Sh, fit['V_hat'], fit['pi_d'], fit['alpha1'], fit['alpha2'], s1, s2, n_iter, TOL)
    a1, froze = sr.fold_in(X, lv, St, Sh, fit['alpha1'], a2r, s1, n_iter, TOL)
    return a1, a2r, froze


@pytest.fixture(scope='module', params=[False, True], ids=['sparse-pcmf', 'sparse-zi'])
def planted_fold_in(request):
    zi = request.param
    _, fit, Xq = sr.planted_case(zi, zero_cell=ZERO_CELL)
    return (zi, fit, Xq) + tuple(_fold(fit, Xq, N_ITER, zi))


# ---- (a) without masks it is the dense models' map, exactly -------------------------------------------------------------------

def test_unmasked_map_is_the_pcmf_map_exactly():
    _, fit, Xq = sr.planted_case(False, zero_cell=ZERO_CELL)
    ones = np.ones_like(fit['p_s'])
    a2r = sr.a2_row(fit['alpha2'], ones, fit['V_hat'])
    assert np.array_equal(a2r, np.maximum(1e-15, fit['alpha2'] + fit['V_hat'].sum(axis=0)))
    s = sr.default_start(Xq, fit['alpha1'], ones, ones)
    assert np.allclose(s, tr.default_start(Xq, fit['alpha1']), rtol=1e-15, atol=0)      # (x / K summed against a sum over K: an ulp)
    a1 = np.random.default_rng(3).gamma(1.0, 1.0, size=s.shape)
    got = sr.T64(Xq, fit['log_V_hat'], ones, ones, fit['alpha1'], a2r, a1)
    assert np.array_equal(got, tr.T64(Xq, fit['log_V_hat'], fit['alpha1'], a2r, a1))
    g1, gf = sr.fold_in(Xq, fit['log_V_hat'], ones, ones, fit['alpha1'], a2r, s, 40, TOL)
    r1, rf = tr.fold_in(Xq, fit['log_V_hat'], fit['alpha1'], a2r, s, 40, TOL)
    assert np.array_equal(g1, r1) and np.array_equal(gf, rf)


def test_unmasked_map_is_the_zi_map_exactly():
    _, fit, Xq = sr.planted_case(True, zero_cell=ZERO_CELL)
    ones = np.ones_like(fit['p_s'])
    args = (fit['log_V_hat'], fit['V_hat'], fit['pi_d'], fit['alpha1'], fit['alpha2'])
    rng = np.random.default_rng(4)
    a1, a2 = rng.gamma(1.0, 1.0, size=(Xq.shape[0], 3)), rng.gamma(20.0, 1.0, size=(Xq.shape[0], 3))
    g1, g2 = sr.T64_zi(Xq, fit['log_V_hat'], ones, ones, fit['V_hat'], fit['pi_d'], fit['alpha1'], fit['alpha2'], a1, a2)
    r1, r2 = zr.T64(Xq, *args, a1, a2)
    assert np.array_equal(g1, r1) and np.array_equal(g2, r2)
    g = sr.fold_in_zi(Xq, fit['log_V_hat'], ones, ones, fit['V_hat'], fit['pi_d'], fit['alpha1'], fit['alpha2'], a1, a2, 25, TOL)
    r = zr.fold_in(Xq, *args, a1, a2, 25, TOL)
    assert all(np.array_equal(x, y) for x, y in zip(g, r))


# ---- (b) a fully masked gene ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('zi', [False, True], ids=['sparse-pcmf', 'sparse-zi'])
def test_fully_masked_gene_contributes_nothing_to_a1(zi):
    """Counts at genes whose every factor is masked do not reach a1 (bit for bit), whatever S_hat and E[log V'] say there; with
    sparse pCMF they reach nothing at all (the rate is a column sum of the gene side alone).  The ZI rate does see them: x != 0
    puts d = 1 where the sigmoid would have been."""
    _, fit, Xq = sr.planted_case(zi, zero_cell=ZERO_CELL)
    lv, St, Sh = _gene_side(fit)
    dead = St.sum(axis=1) == 0
    assert dead.mean() >= 0.2 and (Xq[:, dead] != 0).any(), 'the planted case has no counts at fully masked genes'
    X0 = np.array(Xq)
    X0[:, dead] = 0
    Sh2, lv2 = np.array(Sh), np.array(lv)
    Sh2[dead] = 0.7
    lv2[dead] += 3.0
    assert np.array_equal(sr.default_start(Xq, fit['alpha1'], St, Sh), sr.default_start(X0, fit['alpha1'], St, Sh2))
    a1 = np.random.default_rng(5).gamma(1.0, 1.0, size=(Xq.shape[0], 3))
    if zi:
        a2 = np.random.default_rng(6).gamma(20.0, 1.0, size=a1.shape)
        rest = (fit['V_hat'], fit['pi_d'], fit['alpha1'], fit['alpha2'], a1, a2)
        g1, g2 = sr.T64_zi(Xq, lv, St, Sh, *rest)
        h1, h2 = sr.T64_zi(X0, lv2, St, Sh, *rest)
        assert np.array_equal(g1, h1)
        assert not np.array_equal(g2, h2), 'the rate should see the non-zero mask of every gene'
    else:
        a2r = sr.a2_row(fit['alpha2'], Sh, fit['V_hat'])
        assert np.array_equal(sr.T64(Xq, lv, St, Sh, fit['alpha1'], a2r, a1), sr.T64(X0, lv2, St, Sh2, fit['alpha1'], a2r, a1))
        g = sr.fold_in(Xq, lv, St, Sh, fit['alpha1'], a2r, a1, 30, TOL)
        h = sr.fold_in(X0, lv2, St, Sh2, fit['alpha1'], a2r, a1, 30, TOL)
        assert np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1])


# ---- (c) (d) the loop ----------------------------------------------------------------------------------------------------------

def test_every_cell_freezes(planted_fold_in):
    zi, fit, Xq, a1, a2, froze = planted_fold_in
    print('zi=%s freeze iterations: min %d median %d max %d, %d distinct' % (zi, froze.min(), np.median(froze), froze.max(),
                                                                            np.unique(froze).size))
    assert froze.max() < N_ITER, '%d cells never froze' % int((froze == N_ITER).sum())
    assert np.unique(froze).size > 1, 'every cell froze at the same iteration'
    assert np.isfinite(a1).all() and (a1 >= 1e-15).all() and np.isfinite(a2).all() and (a2 >= 1e-15).all()


def test_all_zero_cell_stays_at_the_prior(planted_fold_in):
    zi, fit, Xq, a1, a2, froze = planted_fold_in
    assert not Xq[ZERO_CELL].any()
    assert np.array_equal(a1[ZERO_CELL], np.maximum(1e-15, fit['alpha1']))
    assert zi or froze[ZERO_CELL] == 0               # (the zero-inflated cell's rate still moves: its posterior reads U_hat)


def test_frozen_cells_are_fixed_points_within_tol(planted_fold_in):
    zi, fit, Xq, a1, a2, froze = planted_fold_in
    lv, St, Sh = _gene_side(fit)
    if zi:
        n1, n2 = sr.T64_zi(Xq, lv, St, Sh, fit['V_hat'], fit['pi_d'], fit['alpha1'], fit['alpha2'], a1, a2)
        assert np.all(np.abs(n2 - a2) <= TOL * a2)
    else:
        n1 = sr.T64(Xq, lv, St, Sh, fit['alpha1'], a2, a1)
    assert np.all(np.abs(n1 - a1) <= TOL * a1)


def test_a_cells_result_does_not_depend_on_its_batch(planted_fold_in):
    """Frozen cells are never rewritten: a longer budget, and folding in a subset alone, give the same rows bit for bit."""
    zi, fit, Xq, a1, a2, froze = planted_fold_in
    b1, b2, fr = _fold(fit, Xq, N_ITER + 50, zi)
    assert np.array_equal(b1, a1) and np.array_equal(b2, a2) and np.array_equal(fr, froze)
    sub = np.array([0, 5, ZERO_CELL, 77, 149])
    c1, c2, frs = _fold(fit, Xq, N_ITER + 50, zi, rows=sub)
    assert np.array_equal(c1, a1[sub]) and np.array_equal(frs, froze[sub])
    assert np.array_equal(c2, a2[sub] if zi else a2)
