# -*- coding: utf-8 -*-
"""SparseGaP.project() / SparseZIGaP.project() and oriana_row_spmm_active on the GPU against the float64 restatement of
tests/sparse_foldin_reference.py.

Shapes are those of tests/test_elbo_gpu.py: 805 x 301 -- a partial last cell tile, two gene tiles, four 256-cell row blocks; an
all-zero cell, an all-zero gene, a gene expressed everywhere.  Two sweeps from a random start leave p_s ~ 1, which would test no
mask, so the gene side is a swept model with a p_s of the test's own loaded over it (_gene_prob): U(0, 1) entries, a quarter of
the genes (and the gene expressed everywhere) at 0.1 in every factor -- fully masked --, one gene at 0.9 everywhere, entries at
exactly 0 and exactly 1.  K is one per form of the sparse row phase: 20 (generic two-image kernel), 50 (k64 two-image kernel),
100 (k100 s_rs pass + second row product), 128 (generic s_rs pass + second row product).  The bound on one update is helpers.RTOL,
the project's stated bound for variational parameters."""
import numpy as np
import pytest
import torch

import sparse_foldin_reference as sr
from helpers import RTOL, err_colrel
from test_elbo_gpu import M_COLS, N_ROWS, TINY_ALL, TINY_SOME, _counts, _model, _twin_bound
from test_transform_gpu import _held_tensors

pytestmark = pytest.mark.gpu

KS = (20, 50, 100, 128)
NAMES = ('SparseGaP', 'SparseZIGaP')
ZERO_CELL = 11                    # of _counts
EVERYWHERE = 250                  # of _counts: the gene expressed in every cell
GENE_09 = 100
DEV = 'cuda'


def _gene_prob(K, seed):
    rng = np.random.default_rng(500 + seed)
    P = rng.uniform(0.0, 1.0, size=(M_COLS, K))
    P[1::4] = 0.1                                  # 75 of 301 genes: every factor masked
    P[EVERYWHERE] = 0.1                            # ... and the gene every cell has a count at
    P[GENE_09] = 0.9
    P[10, 0] = P[20, K - 1] = 0.0
    P[30, 0] = P[40, K - 1] = 1.0
    assert ((P <= 0.5).all(axis=1)).mean() >= 0.2
    return P


_models = {}


def _fitted(name, K):
    """A model swept twice from a random start with the test's p_s loaded over it (cached: project() only reads it -- which
    test_project_leaves_the_model_alone checks)."""
    if (name, K) not in _models:
        G = _model(_counts(K), K, name=name, seed=K)
        for _ in range(2):
            G.step()
        G.load_state({'p_s': _gene_prob(K, K)})
        G.update_expectations()
        _models[name, K] = G
    return _models[name, K]


def _gene_side(G):
    st = G.state()
    St, Sh = sr.masks(st['p_s'], G.tau)
    return st, St, Sh


def _reference_update(G, Xq, s1):
    """(a1', a2' -- the K-vector for SparseGaP --) of the float64 map from the start s1 and the default rate."""
    st, St, Sh = _gene_side(G)
    a2r = sr.a2_row(st['alpha2'], Sh, st['V_hat'])
    if G.zi:
        s2 = a2r[None, :] * np.ones((Xq.shape[0], 1))
        return sr.T64_zi(Xq, st['log_V_hat'], St, Sh, st['V_hat'], st['pi_d'], st['alpha1'], st['alpha2'], s1, s2)
    return sr.T64(Xq, st['log_V_hat'], St, Sh, st['alpha1'], a2r, s1), a2r


def _rate_matrix(G, a2, nq):
    return a2 if G.zi else a2[None, :]


def _check_one_update(G, Xq, a1_0, what):
    r1, r2 = _reference_update(G, Xq, np.maximum(1e-15, a1_0))
    E, a1, a2, froze = G.project(Xq, n_iter=1, tol=0, init=a1_0, return_params=True)
    nq, K = a1_0.shape
    e1, e2, e3 = err_colrel(a1, r1), err_colrel(a2, r2), err_colrel(E, r1 / _rate_matrix(G, r2, nq))
    print('%s %s: a1 %.3e a2 %.3e E[U] %.3e (bound %.1e)' % (type(G).__name__, what, e1, e2, e3, RTOL))
    assert E.dtype == a1.dtype == a2.dtype == np.float64 and froze.dtype == np.int32
    assert E.shape == a1.shape == (nq, K) and a2.shape == ((nq, K) if G.zi else (K,)) and froze.shape == (nq,)
    assert np.isfinite(a1).all() and np.isfinite(a2).all() and np.isfinite(E).all()
    assert np.array_equal(E, a1 / _rate_matrix(G, a2, nq))
    assert e1 <= RTOL and e2 <= RTOL and e3 <= RTOL
    return a1, a2


# ---- 1. one iteration against float64 -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('name', NAMES)
def test_one_iteration_against_float64(name, K):
    G = _fitted(name, K)
    Xq = _counts(K + 50)
    a1_0 = np.random.default_rng(70 + K).gamma(1.0, 1.0, size=(N_ROWS, K))
    _check_one_update(G, Xq, a1_0, 'K=%d' % K)


# ---- 2. edge starts and short batches -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', NAMES)
def test_shapes_at_the_clamp(name):
    """Cells whose start puts two factors, or every factor, at 1e-15 (E[log U] ~ -1e15 there)."""
    K = 20
    G = _fitted(name, K)
    Xq = _counts(3)
    a1_0 = np.random.default_rng(5).gamma(1.0, 1.0, size=(N_ROWS, K))
    for i in TINY_SOME:
        a1_0[i, [2, 11]] = 1e-15
    a1_0[TINY_ALL, :] = 1e-15
    assert all((Xq[i] != 0).any() for i in TINY_SOME + (TINY_ALL,))
    a1, a2 = _check_one_update(G, Xq, a1_0, 'clamped starts')
    assert (a1[TINY_ALL] > 1e-15).any()


@pytest.mark.parametrize('nq', [1, 255])
@pytest.mark.parametrize('name', NAMES)
def test_short_batches(name, nq):
    K = 20
    G = _fitted(name, K)
    Xq = _counts(9)[12:12 + nq]
    a1_0 = np.random.default_rng(6).gamma(1.0, 1.0, size=(nq, K))
    _check_one_update(G, Xq, a1_0, 'n\' = %d' % nq)
    E = G.project(Xq, n_iter=3)
    assert E.shape == (nq, K) and np.isfinite(E).all()


@pytest.mark.parametrize('name', NAMES)
def test_no_cells(name):
    G = _fitted(name, 20)
    E, a1, a2, froze = G.project(np.zeros((0, M_COLS)), return_params=True)
    assert E.shape == a1.shape == (0, 20) and a2.shape == ((0, 20) if G.zi else (20,)) and froze.shape == (0,)
    assert G.project_unconverged_ == 0


# ---- 3. the default start -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,K', [('SparseGaP', K) for K in KS] + [('SparseZIGaP', 50)])
def test_default_start_is_the_masked_uniform_update(name, K):
    """n_iter = 0 returns the start itself: alpha1 + sum_j x_ij S_hat_jk S~_jk / max(1, sum_k S~_jk), and the default rate."""
    G = _fitted(name, K)
    Xq = _counts(K + 60)
    st, St, Sh = _gene_side(G)
    ref = sr.default_start(Xq, st['alpha1'], St, Sh)
    E, a1, a2, froze = G.project(Xq, n_iter=0, return_params=True)
    a2r = sr.a2_row(st['alpha2'], Sh, st['V_hat'])
    e1, e2 = err_colrel(a1, ref), err_colrel(a2, a2r[None, :] * np.ones((N_ROWS, 1)) if G.zi else a2r)
    print('%s K=%d default start: a1 %.3e a2 %.3e (bound %.1e)' % (name, K, e1, e2, RTOL))
    assert e1 <= RTOL and e2 <= 1e-12
    assert np.array_equal(a1[ZERO_CELL], np.maximum(1e-15, st['alpha1']))
    assert (froze == 0).all() and G.project_unconverged_ == N_ROWS


# ---- 4. convergence and freezing ----------------------------------------------------------------------------------------------

TOL = 1e-4
PLANTED_ZERO_CELL = 23


@pytest.fixture(scope='module', params=[False, True], ids=['sparse-pcmf', 'sparse-zi'])
def planted(request):
    """The planted case of tests/test_sparse_foldin_host.py: the float64 sparse fit loaded into a GPU model, and the fresh cells."""
    import oriana_amd.models as M
    zi = request.param
    (X, a1, b1, K), fit, Xq = sr.planted_case(zi, zero_cell=PLANTED_ZERO_CELL)
    G = (M.SparseZIGaP if zi else M.SparseGaP)(np.array(X), k=K, init=(np.array(a1), np.array(b1)), tau=sr.TAU)
    keys = ('alpha1', 'alpha2', 'beta1', 'beta2', 'a1', 'a2', 'b1', 'b2', 'pi_s', 'p_s') + (('pi_d', 'p_d') if zi else ())
    G.load_state({k: np.array(fit[k]) for k in keys})
    G.update_expectations()
    return G, np.array(Xq)


def _residual(G, Xq, a1, a2):
    """err_colrel between the float64 map at (a1, a2) and (a1, a2): how far the result is from a fixed point."""
    st, St, Sh = _gene_side(G)
    if G.zi:
        n1, n2 = sr.T64_zi(Xq, st['log_V_hat'], St, Sh, st['V_hat'], st['pi_d'], st['alpha1'], st['alpha2'], a1, a2)
        return max(err_colrel(n1, a1), err_colrel(n2, a2))
    assert err_colrel(a2, sr.a2_row(st['alpha2'], Sh, st['V_hat'])) <= 1e-12
    return err_colrel(sr.T64(Xq, st['log_V_hat'], St, Sh, st['alpha1'], a2, a1), a1)


def test_every_cell_freezes_at_a_fixed_point(planted):
    G, Xq = planted
    _, St, _ = _gene_side(G)
    assert (St.sum(axis=1) == 0).mean() >= 0.2, 'the planted fit lost its fully masked genes on the way into the model'
    E, a1, a2, froze = G.project(Xq, n_iter=300, tol=TOL, return_params=True)
    print('%s freeze iterations: min %d median %d max %d; unconverged %d' % (type(G).__name__, froze.min(), np.median(froze),
                                                                             froze.max(), G.project_unconverged_))
    assert G.project_unconverged_ == 0 and froze.max() < 300
    res = _residual(G, Xq, a1, a2)
    print('residual %.3e (bound %.3e)' % (res, TOL + RTOL))
    assert res <= TOL + RTOL
    assert np.unique(froze).size > 1, 'every cell froze at the same iteration'
    assert np.array_equal(E, a1 / _rate_matrix(G, a2, Xq.shape[0]))
    assert not Xq[PLANTED_ZERO_CELL].any() and np.array_equal(a1[PLANTED_ZERO_CELL], np.maximum(1e-15, G.alpha1[:]))
    # frozen cells are never rewritten: a longer budget changes nothing, bit for bit
    E2, a1_2, a2_2, froze2 = G.project(Xq, n_iter=400, tol=TOL, return_params=True)
    assert np.array_equal(a1_2, a1) and np.array_equal(a2_2, a2) and np.array_equal(froze2, froze) and np.array_equal(E2, E)
    # ... and a cell that does not freeze within the budget is counted and reported at n_iter
    _, _, _, froze3 = G.project(Xq, n_iter=3, tol=TOL, return_params=True)
    assert G.project_unconverged_ == int((froze3 == 3).sum()) == int((froze >= 3).sum())


# ---- 5. the call leaves the model alone ---------------------------------------------------------------------------------------

def _flags(G):
    ws = G._ws
    kept = getattr(G, '_DV_next', None)
    zi = (G._pd_sum_fresh, G.n_kept_products, G.p_d.materialised, sorted(G._padbuf),
          None if kept is None else (kept[0].data_ptr(), kept[1], kept[0].cpu().numpy().tobytes())) if G.zi else ()
    return (ws.fu_pending, ws.fu_source, ws.FU.data_ptr(), ws.prep_blocks, ws.rows_nslab, getattr(G, '_u_stale', None),
            G._v_sums_in_acc, G._ver, G.n_sweeps, G._S_tilde.data_ptr(), G._S_hat.data_ptr(), G._Veff.data_ptr()) + zi


def _project_leaves_state_alone(G, Xq, **kw):
    before, flags = _held_tensors(G), _flags(G)
    assert {'_S_tilde', '_S_hat', 'p_s', '_Veff'} <= before.keys()
    G.project(Xq, **kw)
    after = _held_tensors(G)
    assert _flags(G) == flags
    changed = [k for k in before if after.get(k) != before[k]]
    assert not changed and before.keys() == after.keys(), 'project() wrote %s' % changed


@pytest.mark.parametrize('name,K', [('SparseGaP', 100), ('SparseZIGaP', 50)])
def test_project_leaves_the_model_alone(name, K):
    """On the state with the test's p_s loaded: _S_tilde still holds the threshold of the last SWEEP's p_s there, so a project()
    that thresholded into the model's buffer would show."""
    G = _fitted(name, K)
    St = sr.masks(G.state()['p_s'], G.tau)[0]
    assert not np.array_equal(G._S_tilde.cpu().numpy().astype(np.float64), St), 'the case cannot tell the two buffers apart'
    _project_leaves_state_alone(G, _counts(K + 2)[:300], n_iter=3)
    _project_leaves_state_alone(G, _counts(K + 2)[:300], n_iter=2, tol=0, init=np.ones((300, K)))


def _three_sweeps(name, K, with_project):
    G = _model(_counts(K + 1), K, name=name, seed=K + 1)
    Xq = _counts(K + 2)[:300]
    for _ in range(3):
        if with_project:
            _project_leaves_state_alone(G, Xq, n_iter=3)
        G.step()
    if with_project:
        assert not G.zi or G._DV_next is not None, 'the case does not cover a kept D_hat V product'
        _project_leaves_state_alone(G, Xq, n_iter=2, tol=0)
    torch.cuda.synchronize()
    return G.state(), G.n


@pytest.mark.parametrize('name,K', [('SparseGaP', 100), ('SparseZIGaP', 50)])
def test_project_does_not_disturb_the_sweep(name, K):
    (b, n), (a, _) = _three_sweeps(name, K, False), _three_sweeps(name, K, True)
    tol = _twin_bound(n, 3)
    for k in b:
        e = err_colrel(a[k], b[k]) if b[k].size else 0.0
        assert e <= tol, '%s: the run with project() calls is %.3e from the one without (bound %.3e)' % (k, e, tol)


# ---- 6. without masks it is transform() ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('K', [20, 100])
def test_unmasked_project_is_transform(K):
    """A SparseGaP with p_s = 1 loaded and a GaP carrying the same Gamma state run the same map (two-image / two-launch row phase
    against the plain row pass)."""
    X = _counts(K)
    S = _model(X, K, name='SparseGaP', seed=K)
    for _ in range(2):
        S.step()
    st = S.state()
    S.load_state({'p_s': np.ones((M_COLS, K))})
    S.update_expectations()
    G = _model(X, K, name='GaP', seed=K)
    G.load_state({k: st[k] for k in ('alpha1', 'alpha2', 'beta1', 'beta2', 'a1', 'a2', 'b1', 'b2')})
    G.update_expectations()
    Xq = _counts(K + 50)[:300]
    a1_0 = np.random.default_rng(8).gamma(1.0, 1.0, size=(300, K))
    for kw in (dict(n_iter=4, tol=0, init=a1_0), dict(n_iter=4, tol=0)):
        got, ref = S.project(Xq, return_params=True, **kw), G.transform(Xq, return_params=True, **kw)
        e = [err_colrel(g, r) for g, r in zip(got[:3], ref[:3])]
        print('K=%d %s: E[U] %.3e a1 %.3e a2_row %.3e (bound %.1e)' % (K, sorted(kw), e[0], e[1], e[2], RTOL))
        assert max(e) <= RTOL


# ---- 7. errors and pins -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', NAMES)
def test_errors(name):
    from oriana_amd import engine
    G = _fitted(name, 20)
    with pytest.raises(ValueError, match='genes'):
        G.project(np.zeros((4, M_COLS + 1)))
    with pytest.raises(ValueError, match='genes'):
        G.project(engine.CountTiles.from_dense(_counts(1)[:40, :200], G.device))
    with pytest.raises(ValueError, match='init'):
        G.project(_counts(1)[:40], init=np.ones((41, 20)))
    with pytest.raises(ValueError, match='dense_density'):
        G.project(engine.CountTiles.from_dense(_counts(1), G.device, dense_density=0.5))
    with pytest.raises(NotImplementedError, match='pCMF') as exc:
        G.transform(_counts(3)[:10])
    assert 'project' in str(exc.value)
    for call in (G.score_samples, G.score):
        with pytest.raises(NotImplementedError, match='pCMF'):
            call(_counts(3)[:10])
    assert not hasattr(G, 'fold_in') and not hasattr(G, 'fold_in_score_samples') and not hasattr(G, 'fold_in_score')
    assert 'fold_in_score' not in type(G)._no_score


def test_zero_inflated_k_range():
    wide = _model(_counts(2)[:300], 129, name='SparseZIGaP', seed=2)
    with pytest.raises(ValueError, match='128'):
        wide.project(_counts(3)[:10])
    E = _model(_counts(2)[:300], 129, name='SparseGaP', seed=2).project(_counts(3)[:10], n_iter=2)
    assert E.shape == (10, 129) and np.isfinite(E).all()


# ---- 8. the second row product skips frozen row blocks ------------------------------------------------------------------------

def _spmm(ct, s_rs, FV, K, active='plain'):
    """R (n, Kp) pre-filled with NaN after oriana_row_spmm ('plain') or oriana_row_spmm_active (a uint8 tensor, or None = NULL)."""
    from oriana_amd import engine
    from oriana_amd._lib import call, ptr, stream_ptr
    R = torch.full((ct.n, engine.kpad(K)), float('nan'), dtype=torch.float32, device=DEV)
    if isinstance(active, str):
        call('oriana_row_spmm', ct.sparse_struct, ptr(s_rs), None, ptr(FV), ptr(R), K, stream_ptr())
    else:
        call('oriana_row_spmm_active', ct.sparse_struct, ptr(s_rs), None, ptr(FV), ptr(R), ptr(active), K, stream_ptr())
    torch.cuda.synchronize()
    return R.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('sort_rows', [False, True], ids=['rows-as-given', 'rows-sorted'])
@pytest.mark.parametrize('K', [100, 128])
def test_row_spmm_active(K, sort_rows):
    from oriana_amd import engine
    ct = engine.CountTiles.from_dense(_counts(K + 7), DEV, sort_rows=sort_rows)
    assert ct.nrb == 4 and (ct.row_perm is not None) == sort_rows
    g = torch.Generator(device='cpu').manual_seed(K)
    s_rs = torch.rand(max(ct.rslots, 1), generator=g).to(DEV)
    FV = torch.rand(M_COLS, engine.kpad(K), generator=g).to(DEV)
    full = _spmm(ct, s_rs, FV, K)
    assert np.isfinite(full).all(), 'oriana_row_spmm left rows of R unwritten'
    act = lambda a: torch.from_numpy(a.astype(np.uint8)).to(DEV)
    caller_row = ct.row_perm.cpu().numpy() if sort_rows else np.arange(N_ROWS)          # packed row -> the caller's
    # every cell active, and active = NULL: the bits of oriana_row_spmm
    assert _same_bits(_spmm(ct, s_rs, FV, K, act(np.ones(N_ROWS))), full)
    assert _same_bits(_spmm(ct, s_rs, FV, K, None), full)
    # the packed row blocks 1 and 3 (3 is the partial one) off: their rows stay NaN, the others are bit-identical
    off = np.zeros(N_ROWS, dtype=bool)
    off[256:512] = off[768:] = True
    a = np.ones(N_ROWS)
    a[caller_row[off]] = 0
    got = _spmm(ct, s_rs, FV, K, act(a))
    assert np.isnan(got[off]).all(), 'rows of a skipped block were written'
    assert _same_bits(got[~off], full[~off])
    # a random per-cell mask: every active row is bit-identical (rows of frozen cells may hold anything)
    a = (np.random.default_rng(K).random(N_ROWS) < 0.5).astype(np.float64)
    a[caller_row[:256]] = 0                                                            # (and one whole block off again)
    got = _spmm(ct, s_rs, FV, K, act(a))
    on = a[caller_row] != 0
    assert on.any() and _same_bits(got[on], full[on])
    assert np.isnan(got[:256]).all()
