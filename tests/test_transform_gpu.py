# -*- coding: utf-8 -*-
"""GaP.transform() on the GPU against the float64 restatement of tests/transform_reference.py.

Shapes are those of tests/test_elbo_gpu.py (a partial last row tile, two column tiles with the last one partial, an
all-zero cell, an all-zero gene, a gene expressed everywhere).  The bound on one update is helpers.RTOL, the project's stated
bound for variational parameters: the HIP map and the float64 one differ by the float32 evaluation of the same sums."""
import numpy as np
import pytest
import torch

import transform_reference as tr
from helpers import RTOL, err_colrel
from test_elbo_gpu import (DENSE_DENSITY, HYBRID_KS, KS, M_COLS, N_ROWS, TINY_ALL, TINY_SOME, _counts, _model, _planted,
                           _twin_bound)

pytestmark = pytest.mark.gpu

ZERO_CELL = 11                    # of _counts


def _a2_row(st):
    return np.maximum(1e-15, st['alpha2'] + st['V_hat'].sum(axis=0))


def _fitted(K, dd, sweeps=2):
    G = _model(_counts(K), K, dense_density=dd, seed=K)
    assert (G.counts.gd >= 32) if dd else G.counts.gd == 0
    for _ in range(sweeps):
        G.step()
    return G


def _reference_update(G, Xq, a1_0):
    st = G.state()
    a2 = _a2_row(st)
    return tr.T64(Xq, st['log_V_hat'], st['alpha1'], a2, a1_0), a2


def _check_one_update(G, Xq, a1_0, what):
    ref, a2 = _reference_update(G, Xq, np.maximum(1e-15, a1_0))
    E, a1, a2_row, froze = G.transform(Xq, n_iter=1, tol=0, init=a1_0, return_params=True)
    e1, e2, e3 = err_colrel(a1, ref), err_colrel(E, ref / a2[None, :]), err_colrel(a2_row, a2)
    print('%s: a1 %.3e E[U] %.3e a2_row %.3e (bound %.1e)' % (what, e1, e2, e3, RTOL))
    assert E.dtype == np.float64 and E.shape == a1.shape == a1_0.shape and froze.shape == (a1_0.shape[0],)
    assert np.isfinite(a1).all() and np.isfinite(E).all()
    assert e3 <= 1e-12
    assert e1 <= RTOL and e2 <= RTOL
    return a1, ref


# ---- 1. one iteration against float64 -----------------------------------------------------------------------------------------

def _cases(more=()):
    return [pytest.param(K, dd, id='K%d-%s' % (K, 'hybrid' if dd else 'sliced'))
            for K in KS + tuple(more) for dd in ([None, DENSE_DENSITY] if K in HYBRID_KS else [None])]


# (33, 50, 126: the fold-in update with one and two factors per lane -- every K of KS but 1 takes four, or the element kernel)
@pytest.mark.parametrize('K,dd', _cases(more=(33, 50, 126)))
def test_one_iteration_against_float64(K, dd):
    G = _fitted(K, dd)
    Xq = _counts(K + 50)
    a1_0 = np.random.default_rng(70 + K).gamma(1.0, 1.0, size=(N_ROWS, K))
    _check_one_update(G, Xq, a1_0, 'K=%d %s' % (K, 'hybrid' if dd else 'sliced'))


def test_unaligned_buffers_take_the_element_kernel():
    """heldout.fold_in on an a1 that is 8- but not 16-byte aligned (where oriana_gamma_update_finalize_lazy answers
    ORIANA_EKRANGE): the same update within the same bound."""
    from oriana_amd import engine, heldout
    K = 100
    G = _fitted(K, None)
    Xq = _counts(K + 50)
    a1_0 = np.random.default_rng(70 + K).gamma(1.0, 1.0, size=(N_ROWS, K))
    ref, a2 = _reference_update(G, Xq, a1_0)
    ct = engine.CountTiles.from_dense(Xq, G.device)
    buf = torch.zeros(N_ROWS * K + 2, dtype=torch.float64, device=G.device)
    off = 1 if buf.data_ptr() % 16 == 0 else 0
    a1 = buf[off:off + N_ROWS * K].view(N_ROWS, K)
    assert a1.data_ptr() % 16 == 8
    a1.copy_(torch.from_numpy(a1_0))
    froze, left, done = heldout.fold_in(ct, K, G._log_V_hat, G.alpha1.tensor, torch.from_numpy(a2).to(G.device), a1, 1, 0.0)
    e = err_colrel(a1.cpu().numpy(), ref)
    print('unaligned a1: %.3e' % e)
    assert done == 1 and e <= RTOL
    assert buf[0 if off else -1] == 0 and buf[-1 if off else -2] == 0, 'the update wrote outside a1'


# ---- 2. it is the sweep's cell update -----------------------------------------------------------------------------------------
# A sweep reads E[log U] = psi(a1) - log a2 with the a2 the PREVIOUS sweep stored (that sweep's alpha2 + sum_j V_hat), while a
# fold-in forms the rate from the priors and the gene side at hand.  The two are the same map exactly when the stored a2 is that
# rate, so the twins are put into such a state first: a2 = alpha2 + sum_j V_hat of the current state, expectations recomputed
# (what a model holds after loading such a checkpoint).  From there step()'s cell update and one fold-in iteration of the
# training cells from a1 evaluate the same sums with the same priors.

@pytest.mark.parametrize('K,dd', [(20, None), (100, DENSE_DENSITY)], ids=['K20-sliced', 'K100-hybrid'])
def test_one_iteration_is_the_sweeps_cell_update(K, dd):
    X = _counts(K)
    A = _fitted(K, dd)
    B = _model(X, K, dense_density=dd, seed=K)
    st = A.state()
    st['a2'] = np.ascontiguousarray(np.broadcast_to(_a2_row(st), st['a2'].shape))
    for G in (A, B):
        G.load_state(st)
        G.update_expectations()
    got = A.transform(X, n_iter=1, tol=0, init=A.a1[:], return_params=True)[1]
    B.step()
    ref = B.a1[:]
    e = err_colrel(got, ref)
    print('transform against step(): %.3e (bound %.1e)' % (e, 2 * RTOL))
    assert e <= 2 * RTOL
    assert err_colrel(A.a1[:], st['a1']) == 0.0, 'transform() moved the model\'s own a1'


# ---- 3. convergence and freezing ----------------------------------------------------------------------------------------------

TOL = 1e-4


@pytest.fixture(scope='module')
def planted():
    """The planted case of tests/test_transform_host.py: the float64 fit loaded into a GPU model, and the fresh cells."""
    import oriana_amd.models as M
    X, a1, b1, K = _planted()
    fit = tr.float64_sweeps(X, a1, b1, 40)
    G = M.GaP(X, k=K, init=(a1, b1))
    G.load_state({k: fit[k] for k in ('alpha1', 'alpha2', 'beta1', 'beta2', 'a1', 'a2', 'b1', 'b2')})
    G.update_expectations()
    return G, tr.planted_query(fit, zero_cell=23)


def test_every_cell_freezes_at_a_fixed_point(planted):
    G, Xq = planted
    E, a1, a2_row, froze = G.transform(Xq, n_iter=300, tol=TOL, return_params=True)
    print('freeze iterations: min %d median %d max %d; unconverged %d' % (froze.min(), np.median(froze), froze.max(),
                                                                          G.transform_unconverged_))
    assert G.transform_unconverged_ == 0 and froze.max() < 300
    st = G.state()
    res = err_colrel(tr.T64(Xq, st['log_V_hat'], st['alpha1'], a2_row, a1), a1)
    print('residual %.3e (bound %.3e)' % (res, TOL + RTOL))
    assert res <= TOL + RTOL
    assert np.unique(froze).size > 1, 'every cell froze at the same iteration'
    assert np.array_equal(E, a1 / a2_row[None, :])
    # frozen cells are never rewritten: a longer budget changes nothing, bit for bit
    E2, a1_2, _, froze2 = G.transform(Xq, n_iter=400, tol=TOL, return_params=True)
    assert np.array_equal(a1_2, a1) and np.array_equal(froze2, froze) and np.array_equal(E2, E)
    # ... and a cell that does not freeze within the budget is counted and reported at n_iter
    _, _, _, froze3 = G.transform(Xq, n_iter=3, tol=TOL, return_params=True)
    assert G.transform_unconverged_ == int((froze3 == 3).sum()) == int((froze >= 3).sum())


# ---- 4. edge rows -------------------------------------------------------------------------------------------------------------

def test_all_zero_cell_freezes_at_the_prior():
    K = 20
    G = _fitted(K, None)
    Xq = _counts(3)
    assert not Xq[ZERO_CELL].any()
    E, a1, a2_row, froze = G.transform(Xq, n_iter=5, tol=1e-4, return_params=True)
    assert np.array_equal(a1[ZERO_CELL], np.maximum(1e-15, G.alpha1[:])) and froze[ZERO_CELL] == 0
    # from a start of the caller's it gets there with the first update and freezes at the second
    a1_0 = np.random.default_rng(4).gamma(1.0, 1.0, size=(N_ROWS, K))
    E, a1, a2_row, froze = G.transform(Xq, n_iter=5, tol=1e-4, init=a1_0, return_params=True)
    assert np.array_equal(a1[ZERO_CELL], np.maximum(1e-15, G.alpha1[:])) and froze[ZERO_CELL] == 1


def test_shapes_at_the_clamp_take_the_fallback():
    """Cells whose start puts two factors, or every factor, at 1e-15: E[log U] ~ -1e15 there, the row of the all-clamped cell
    cannot take the shifted form (the slow path evaluates its entries)."""
    K = 20
    G = _fitted(K, None)
    Xq = _counts(3)
    a1_0 = np.random.default_rng(5).gamma(1.0, 1.0, size=(N_ROWS, K))
    for i in TINY_SOME:
        a1_0[i, [2, 11]] = 1e-15
    a1_0[TINY_ALL, :] = 1e-15
    assert all((Xq[i] != 0).any() for i in TINY_SOME + (TINY_ALL,))
    a1, ref = _check_one_update(G, Xq, a1_0, 'clamped starts')
    assert (a1[TINY_ALL] > 1e-15).any()


@pytest.mark.parametrize('nq', [1, 255])
def test_short_batches(nq):
    K = 20
    G = _fitted(K, None)
    Xq = _counts(9)[12:12 + nq]
    a1_0 = np.random.default_rng(6).gamma(1.0, 1.0, size=(nq, K))
    _check_one_update(G, Xq, a1_0, 'n\' = %d' % nq)
    E = G.transform(Xq, n_iter=3)
    assert E.shape == (nq, K) and np.isfinite(E).all()


# ---- 5. the call leaves the model alone ---------------------------------------------------------------------------------------

def _held_tensors(G):
    """As tests/test_elbo_gpu.py, with nothing left out: transform() works on a workspace of its own, so not even the scratch
    of the model's workspace may change."""
    from oriana_amd.parameters import Parameter
    out = {}
    for owner, prefix in ((G, ''), (G._ws, 'ws.')):
        for k, v in vars(owner).items():
            if isinstance(v, Parameter) and getattr(v, 'materialised', True):
                v = v.tensor
            if isinstance(v, torch.Tensor):
                out[prefix + k] = v.detach().cpu().numpy().tobytes()
    for k, v in G._ws._extra.items():
        out['ws.extra.' + k] = v.detach().cpu().numpy().tobytes()
    return out


def _transform_leaves_state_alone(G, Xq, **kw):
    ws = G._ws
    before = _held_tensors(G)
    flags = (ws.fu_pending, ws.fu_source, ws.FU.data_ptr(), ws.prep_blocks, G._u_stale, G._v_sums_in_acc, G._ver, G.n_sweeps,
             getattr(G.a2, 'materialised', True))
    G.transform(Xq, **kw)
    after = _held_tensors(G)
    assert (ws.fu_pending, ws.fu_source, ws.FU.data_ptr(), ws.prep_blocks, G._u_stale, G._v_sums_in_acc, G._ver, G.n_sweeps,
            getattr(G.a2, 'materialised', True)) == flags
    changed = [k for k in before if after.get(k) != before[k]]
    assert not changed and before.keys() == after.keys(), 'transform() wrote %s' % changed


def test_transform_keeps_the_prepared_factor():
    n, m, K = 8200, 200, 128                           # n K >= 2^20: the fused preparation and the lazy form engage
    rng = np.random.default_rng(12)
    X = (rng.poisson(3.0, size=(n, m)) * (rng.random((n, m)) < 0.1)).astype(np.float64)
    G = _model(X, K, seed=12)
    G.step()
    G.step()
    assert G._ws.fu_pending and G._u_stale and not G.a2.materialised, 'the case covers neither the fused preparation nor the lazy cell side'
    Xq = (rng.poisson(3.0, size=(300, m)) * (rng.random((300, m)) < 0.1)).astype(np.float64)
    _transform_leaves_state_alone(G, Xq, n_iter=7, tol=1e-4)
    G.step()
    _transform_leaves_state_alone(G, Xq, n_iter=2, tol=0)


def _three_sweeps(K, dd, with_transform):
    X = _counts(K + 1)
    G = _model(X, K, dense_density=dd, seed=K + 1)
    Xq = _counts(K + 2)[:300]
    for _ in range(3):
        if with_transform:
            _transform_leaves_state_alone(G, Xq, n_iter=3)
        G.step()
    torch.cuda.synchronize()
    return G.state(), G.n


@pytest.mark.parametrize('K,dd', [(20, None), (100, DENSE_DENSITY)], ids=['K20-sliced', 'K100-hybrid'])
def test_transform_does_not_disturb_the_sweep(K, dd):
    (b, n), (a, _) = _three_sweeps(K, dd, False), _three_sweeps(K, dd, True)
    tol = _twin_bound(n, 3)
    for k in b:
        e = err_colrel(a[k], b[k]) if b[k].size else 0.0
        assert e <= tol, '%s: the run with transform() calls is %.3e from the one without (bound %.3e)' % (k, e, tol)


# ---- 6. errors and input variants ---------------------------------------------------------------------------------------------

def test_wrong_gene_count():
    from oriana_amd import engine
    G = _fitted(20, None, sweeps=0)
    with pytest.raises(ValueError, match='genes'):
        G.transform(np.zeros((4, M_COLS + 1)))
    with pytest.raises(ValueError, match='genes'):
        G.transform(engine.CountTiles.from_dense(_counts(1)[:40, :200], G.device))
    with pytest.raises(ValueError, match='init'):
        G.transform(_counts(1)[:40], init=np.ones((41, 20)))


@pytest.mark.parametrize('name', ['ZIGaP', 'SparseGaP', 'SparseZIGaP'])
def test_other_models_say_so(name):
    G = _model(_counts(2)[:300], 5, name=name, seed=2)
    with pytest.raises(NotImplementedError, match='pCMF'):
        G.transform(_counts(3)[:10])


def test_input_variants_agree():
    """SciPy sparse, CountMatrix-like, tensor and prebuilt CountTiles inputs give the dense-input result."""
    import scipy.sparse as sp
    from oriana_amd import engine
    K = 20
    G = _fitted(K, None)
    Xq = _counts(8)[:300]
    a1_0 = np.random.default_rng(8).gamma(1.0, 1.0, size=(300, K))
    base = G.transform(Xq, n_iter=4, tol=0, init=a1_0)

    class Wrapped:
        shape = Xq.shape

        def as_array(self):
            return Xq
    variants = {'csr': sp.csr_matrix(Xq), 'as_array': Wrapped(), 'tensor': torch.from_numpy(Xq).to(G.device),
                'tiles': engine.CountTiles.from_scipy(sp.csr_matrix(Xq), G.device)}
    for name, v in variants.items():
        e = err_colrel(G.transform(v, n_iter=4, tol=0, init=a1_0), base)
        print('%s: %.3e' % (name, e))
        assert e <= RTOL, name
    # the default start needs no dense copy either
    e = err_colrel(G.transform(variants['csr'], n_iter=4), G.transform(Xq, n_iter=4))
    assert e <= RTOL
