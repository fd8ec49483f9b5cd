# -*- coding: utf-8 -*-
"""GaP.score_samples() / score() and heldout.cell_bounds on the GPU against the float64 reference of tests/score_reference.py.

Shapes and models are those of tests/test_elbo_gpu.py (the smallest that cross a partial last row tile and two gene tiles, with
an all-zero cell, an all-zero gene and a gene expressed everywhere); the bounds are elbo_reference.elbo_bounds per cell
(score_reference.cell_bounds): g = (K + 3) 2^-24 on the float32 den of the row pass, 1e-12 relative to the sum of |piece| for
everything that is summed in float64.  The reference is evaluated at the a1 and the float32 E[log U] a call returns."""
import numpy as np
import pytest
import torch

import score_reference as sr
import transform_reference as tr
from test_elbo_gpu import DENSE_DENSITY, HYBRID_KS, KS, M_COLS, TINY_SOME, _counts, _model, _planted, _twin_bound

pytestmark = pytest.mark.gpu

NQ = 256 + 37                     # a partial second row tile
ZERO_CELL = 11                    # of _counts
ZERO_GENE = 5                     # of _counts: no count in the fit


def _query(seed, n=NQ):
    """Held-out cells over the genes of _counts: the all-zero cell, and one count at the gene the fit never saw expressed."""
    Xq = _counts(seed, n=n)
    assert not Xq[:, ZERO_GENE].any() and (n <= ZERO_CELL or not Xq[ZERO_CELL].any())
    Xq[min(3, n - 1), ZERO_GENE] = 4.0
    return Xq


def _fitted(K, dd, sweeps=2):
    G = _model(_counts(K), K, dense_density=dd, seed=K)
    assert (G.counts.gd >= 32 and G.counts.dense is not None) if dd else G.counts.gd == 0
    for _ in range(sweeps):
        G.step()
    return G


def _reference(G, Xq, out):
    """The float64 terms at the a1 / log_U_hat the call returned; the rate and sum_j V_hat from the model's state."""
    st = G.state()
    sum_v = st['V_hat'].sum(axis=0)
    a2_row = np.maximum(1e-15, st['alpha2'] + sum_v)
    assert np.max(np.abs(out['a2_row'] - a2_row) / a2_row) <= 1e-12
    return sr.cell_terms(Xq, out['log_U_hat'], st['log_V_hat'], out['a1'], a2_row, sum_v, st['alpha1'], st['alpha2'])


def _check_cells(out, ref, K, what):
    """Every cell's four terms and its score within the bound."""
    tol = sr.cell_bounds(ref, K)
    n = ref['score'].shape[0]
    for k in sr.CELL_TERMS + ('score',):
        assert out[k].dtype == np.float64 and out[k].shape == (n,)
        d = np.abs(out[k] - ref[k])
        i = int(np.argmax(d - tol[k]))
        print('%s %s: worst cell %d HIP %.17g ref %.17g diff %.3e bound %.3e; max diff / bound %.3f' % (
            what, k, i, out[k][i], ref[k][i], d[i], tol[k][i], np.max(d / np.maximum(tol[k], 1e-300))))
    for k in sr.CELL_TERMS + ('score',):
        d = np.abs(out[k] - ref[k])
        bad = np.nonzero(~(np.isfinite(out[k]) & (d <= tol[k])))[0]
        assert bad.size == 0, '%s %s: cells %r: HIP %r ref %r bound %r' % (what, k, bad.tolist(), out[k][bad], ref[k][bad],
                                                                         tol[k][bad])
    assert np.array_equal(out['score'], out['data'] - out['lgamma'] - out['product'] - out['kl'])
    return tol


# ---- 1. the terms against float64 ---------------------------------------------------------------------------------------------

def _cases():
    return [pytest.param(K, dd, id='K%d-%s' % (K, 'hybrid' if dd else 'sliced'))
            for K in KS for dd in ([None, DENSE_DENSITY] if K in HYBRID_KS else [None])]


@pytest.mark.parametrize('K,dd', _cases())
def test_terms_against_float64(K, dd):
    G = _fitted(K, dd)
    Xq = _query(K + 50)
    out = G.score_samples(Xq, n_iter=10, return_terms=True)
    assert set(out) == {'score', 'data', 'lgamma', 'product', 'kl', 'a1', 'a2_row', 'froze_at', 'log_U_hat'}
    assert out['log_U_hat'].dtype == np.float32 and out['log_U_hat'].shape == out['a1'].shape == (NQ, K)
    ref = _reference(G, Xq, out)
    _check_cells(out, ref, K, 'K=%d %s' % (K, 'hybrid' if dd else 'sliced'))
    # the all-zero cell: no data, the prior's shape, exactly -(product + kl)
    z = ZERO_CELL
    assert out['data'][z] == 0 and out['lgamma'][z] == 0 and out['score'][z] == -(out['product'][z] + out['kl'][z])
    assert np.array_equal(out['a1'][z], np.maximum(1e-15, G.alpha1[:]))
    # log_U_hat is the unshifted float32 E[log U] of the returned shapes.  The Gamma node's kernel casts a1 and a2_row to float32
    # first (a psi'(a) <= 2 + |psi(a)|), rounds psi and the float32 log, then the difference; the restatement rounds once
    from scipy.special import psi
    lu = tr.elog_u(out['a1'], out['a2_row']).astype(np.float64)
    room = 2.0 ** -24 * (2 * np.abs(psi(out['a1'])) + 3 + 3 * np.abs(np.log(out['a2_row']))[None, :] + 2 * np.abs(lu))
    assert np.all(np.abs(out['log_U_hat'] - lu) <= room)


# ---- 2. the cells add up to the bound of elbo() -------------------------------------------------------------------------------

@pytest.mark.parametrize('K,dd', [(20, None), (100, DENSE_DENSITY)], ids=['K20-sliced', 'K100-hybrid'])
def test_cells_add_up_to_the_elbo_terms(K, dd):
    """heldout.cell_bounds on the model's own cells (packed sliced), at the model's own a1, rate and stored float32 E[log U]:
    the column sums are the first four terms of GaP._elbo_terms().  (The rate is `_a2_row` while the lazy cell side is in
    effect, else the row every cell of the stored a2 holds -- what _elbo_terms reads.)"""
    from oriana_amd import heldout
    X = _counts(K)
    G = _fitted(K, dd)
    whole = G._elbo_terms().cpu().numpy()
    lazy = G._a2_row is not None and not getattr(G.a2, 'materialised', True)
    a2_row = (G._a2_row if lazy else G.a2.tensor[0]).clone()
    if not lazy:
        assert torch.equal(G.a2.tensor, a2_row.expand_as(G.a2.tensor))
    ct = G._query_counts(X)
    assert ct.gd == 0 and ct.n == G.n
    sum_v = G._V_hat.sum(0)
    t = heldout.cell_bounds(ct, K, G.a1.tensor, a2_row, G._log_U_hat, G._log_V_hat, sum_v, G.alpha1.tensor, G.alpha2.tensor)
    assert t.dtype == torch.float64 and tuple(t.shape) == (G.n, 4)
    got = t.cpu().numpy()
    st = G.state()
    ref = sr.cell_terms(X, st['log_U_hat'], st['log_V_hat'], st['a1'], a2_row.cpu().numpy(), sum_v.cpu().numpy(), st['alpha1'],
                        st['alpha2'])
    tol = sr.cell_bounds(ref, K)
    for c, k in enumerate(sr.CELL_TERMS):
        s, b = float(np.sum(got[:, c].astype(np.longdouble))), 2.0 * float(tol[k].sum())
        print('%s: cells %.17g elbo %.17g diff %.3e bound %.3e' % (k, s, whole[c], abs(s - whole[c]), b))
        assert abs(s - whole[c]) <= b, k


# ---- 3. entries the shifted form cannot represent -----------------------------------------------------------------------------

def test_shapes_at_the_clamp_take_the_fallback():
    """Cells that start with two factors, or every factor, at 1e-15 and are scored there (n_iter=0): E[log U] ~ -1e15, the
    all-clamped cell cannot take the shifted form and its entries are the float64 log-sum-exp inside the kernel."""
    from oriana_amd import engine, heldout
    K = 20
    G = _fitted(K, None)
    Xq = _query(3)
    some, every = [i for i in TINY_SOME if i < NQ], NQ - 1
    a1_0 = np.random.default_rng(5).gamma(1.0, 1.0, size=(NQ, K))
    for i in some:
        a1_0[i, [2, 11]] = 1e-15
    a1_0[every, :] = 1e-15
    assert len(some) == 3 and all((Xq[i] != 0).any() for i in some + [every])
    out = G.score_samples(Xq, n_iter=0, init=a1_0, return_terms=True)
    assert np.array_equal(out['a1'], np.maximum(1e-15, a1_0)) and out['log_U_hat'][every].max() < -1e14
    assert all(np.isfinite(out[k]).all() for k in sr.CELL_TERMS + ('score',))
    ref = _reference(G, Xq, out)
    _check_cells(out, ref, K, 'fallback')
    # the same evaluation on a workspace at hand: the row pass left NaN sentinels, and the values are the same bit for bit
    ct = G._query_counts(Xq)
    ws = engine.ZWorkspace(ct, K)
    dev = G.device
    sum_v = G._accV[0] if G._v_sums_in_acc else G._sumV[0]
    t = heldout.cell_bounds(ct, K, torch.from_numpy(out['a1']).to(dev), torch.from_numpy(out['a2_row']).to(dev),
                           torch.from_numpy(out['log_U_hat']).to(dev), G._log_V_hat, sum_v.contiguous(), G.alpha1.tensor,
                           G.alpha2.tensor, ws=ws).cpu().numpy()
    assert torch.isnan(ws.s_rs).any(), 'the row pass left no NaN sentinel: the fall-back was not exercised'
    for c, k in enumerate(sr.CELL_TERMS):
        assert np.array_equal(t[:, c], out[k]), k


# ---- 4. monotone along the fold-in --------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def planted():
    """The planted case of tests/transform_reference.py: the float64 fit loaded into a GPU model, and the fresh cells."""
    import oriana_amd.models as M
    X, a1, b1, K = _planted()
    fit = tr.float64_sweeps(X, a1, b1, 40)
    G = M.GaP(X, k=K, init=(a1, b1))
    G.load_state({k: fit[k] for k in ('alpha1', 'alpha2', 'beta1', 'beta2', 'a1', 'a2', 'b1', 'b2')})
    G.update_expectations()
    return G, tr.planted_query(fit, zero_cell=23)


def test_score_does_not_decrease_along_the_fold_in(planted):
    G, Xq = planted
    K = G.k
    prev = None
    for n_iter in (0, 1, 2, 5, 20):
        out = G.score_samples(Xq, n_iter=n_iter, tol=0, return_terms=True)
        ref = _reference(G, Xq, out)
        if prev is not None:
            d = out['score'] - prev[0]['score']
            allow = sr.monotone_allowance(prev[1], ref, prev[0]['log_U_hat'], out['log_U_hat'], K)
            print('n_iter %d: smallest increment %.3e, largest drop / allowance %.3f, mean score %.6f' % (
                n_iter, d.min(), (-d / allow).max(), out['score'].mean()))
            bad = np.nonzero(d < -allow)[0]
            assert bad.size == 0, 'n_iter %d: cells %r dropped by %r (allowed %r)' % (n_iter, bad.tolist(), d[bad], allow[bad])
            assert out['score'].mean() > prev[0]['score'].mean()
        prev = (out, ref)


# ---- 5. the call itself -------------------------------------------------------------------------------------------------------

def test_two_calls_agree_bit_for_bit(planted):
    G, Xq = planted
    a, b = G.score_samples(Xq, return_terms=True), G.score_samples(Xq, return_terms=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(G.score_samples(Xq), a['score'])
    # the fold-in is transform()'s
    E, a1, a2_row, froze = G.transform(Xq, return_params=True)
    assert np.array_equal(a1, a['a1']) and np.array_equal(a2_row, a['a2_row']) and np.array_equal(froze, a['froze_at'])


def test_score_is_the_mean(planted):
    G, Xq = planted
    s = G.score_samples(Xq, n_iter=7)
    v = G.score(Xq, n_iter=7)
    assert isinstance(v, float) and v == float(s.mean())
    assert G.score(Xq, n_iter=7, return_terms=True) == v


def _score_leaves_state_alone(G, Xq, **kw):
    from test_transform_gpu import _held_tensors
    ws = G._ws
    flags = lambda: (ws.fu_pending, ws.fu_source, ws.FU.data_ptr(), ws.prep_blocks, G._u_stale, G._v_sums_in_acc, G._ver,
                     G.n_sweeps, getattr(G.a2, 'materialised', True))
    before, f0 = _held_tensors(G), flags()
    G.score_samples(Xq, **kw)
    after = _held_tensors(G)
    assert flags() == f0
    changed = [k for k in before if after.get(k) != before[k]]
    assert not changed and before.keys() == after.keys(), 'score_samples() wrote %s' % changed


def _three_sweeps(K, dd, with_score):
    X = _counts(K + 1)
    G = _model(X, K, dense_density=dd, seed=K + 1)
    Xq = _query(K + 2)
    for _ in range(3):
        if with_score:
            _score_leaves_state_alone(G, Xq, n_iter=3)
        G.step()
    if with_score:
        _score_leaves_state_alone(G, Xq, n_iter=0)
    torch.cuda.synchronize()
    return G.state(), G.n


@pytest.mark.parametrize('K,dd', [(20, None), (100, DENSE_DENSITY)], ids=['K20-sliced', 'K100-hybrid'])
def test_score_does_not_disturb_the_model(K, dd):
    """Everything the model and its workspace hold is bit-identical after a call, and the sweeps that follow are those of a
    twin that never scored (twins of this code base: within the atomic-order bound of tests/test_elbo_gpu.py)."""
    from helpers import err_colrel
    (b, n), (a, _) = _three_sweeps(K, dd, False), _three_sweeps(K, dd, True)
    tol = _twin_bound(n, 3)
    for k in b:
        e = err_colrel(a[k], b[k]) if b[k].size else 0.0
        assert e <= tol, '%s: the run with score_samples() calls is %.3e from the one without (bound %.3e)' % (k, e, tol)


@pytest.mark.parametrize('nq', [0, 1, 255])
def test_batch_sizes(nq):
    K = 20
    G = _fitted(K, None)
    Xq = _query(9)[12:12 + nq] if nq else np.zeros((0, M_COLS))
    out = G.score_samples(Xq, n_iter=3, return_terms=True)
    for k in sr.CELL_TERMS + ('score', 'froze_at'):
        assert out[k].shape == (nq,), k
    assert out['a1'].shape == out['log_U_hat'].shape == (nq, K) and out['score'].dtype == np.float64
    assert G.score_samples(Xq, n_iter=3).shape == (nq,)
    if nq == 0:
        assert np.isnan(G.score(Xq))
        return
    _check_cells(out, _reference(G, Xq, out), K, 'n\' = %d' % nq)
    assert G.score(Xq, n_iter=3) == float(out['score'].mean())


def test_wrong_gene_count():
    G = _fitted(20, None, sweeps=0)
    with pytest.raises(ValueError, match='genes'):
        G.score_samples(np.zeros((4, M_COLS + 1)))
    with pytest.raises(ValueError, match='genes'):
        G.score(np.zeros((4, M_COLS - 1)))


@pytest.mark.parametrize('name', ['ZIGaP', 'SparseGaP', 'SparseZIGaP'])
def test_other_models_say_so(name):
    G = _model(_counts(2)[:300], 5, name=name, seed=2)
    with pytest.raises(NotImplementedError, match='pCMF'):
        G.score_samples(_counts(3)[:10])
    with pytest.raises(NotImplementedError, match='pCMF'):
        G.score(_counts(3)[:10])


# ---- 6. the score picks the planted number of factors -------------------------------------------------------------------------

def test_held_out_score_peaks_at_the_planted_k():
    """Rank-3 Gamma-Poisson counts, fits with 1, 3 and 8 factors, 150 cells none of them saw: the mean held-out score is highest
    at 3 (float64: -263.77, -239.56, -248.38 nats per cell), where elbo() on the training cells keeps rising with k."""
    import oriana_amd.models as M
    rng = np.random.default_rng(0)
    Vt = rng.gamma(1.0, 1.0, (131, 3))
    Ut = rng.gamma(1.0, 1.0, (293, 3))
    X = rng.poisson(Ut @ Vt.T).astype(np.float64)
    Uq = rng.gamma(1.0, 1.0, (150, 3))
    Xq = rng.poisson(Uq @ Vt.T).astype(np.float64)
    scores = {}
    for k in (1, 3, 8):
        r = np.random.default_rng(10 + k)
        G = M.GaP(X, k=k, init=(r.gamma(1.0, 1.0, (293, k)), r.gamma(1.0, 1.0, (131, k))))
        G.fit(60)
        scores[k] = G.score(Xq)
        print('k = %d: mean held-out score %.4f (unconverged cells: %d)' % (k, scores[k], G.transform_unconverged_))
    assert all(np.isfinite(v) for v in scores.values())
    assert scores[3] > scores[1] and scores[3] > scores[8], scores
