# -*- coding: utf-8 -*-
"""ZIGaP.fold_in_fit() and its two C entries, oriana_zi_gene_rate and oriana_svi_gene_update_mat, on the GPU against the float64
restatement of tests/zi_svi_reference.py.

Shapes are those of tests/test_zi_foldin_gpu.py: 805 x 301, mp = 304 -- a partial last cell tile, inert genes, an all-zero cell, a
gene expressed everywhere; its rate_case (Lambda of order 1, one pi_d at 0, one at 1, more than 20 % of the entries in the
sigmoid's middle).  K = 20, 50, 100, 128: 1, 2, 4, 4 factor tiles of the new kernel -- not 3, and at 805 cells (13 ranges of 64) a
range neither leaves the matrix core nor float32: k_gene_rate<3>, the other forms of its factor loop, the flush at 256 cells and the
spill at 4096 are run by tests/test_zi_heldout_forms_gpu.py.  The end-to-end stream is the planted 293 x 131, K = 3 case of
tests/test_zi_fold_in_fit_host.py."""
import numpy as np
import pytest
import torch

import svi_reference as svi
import zi_foldin_reference as zr
import zi_svi_reference as zsvi
from helpers import KEY_ATOL, RTOL, err_colrel
from test_elbo_gpu import DENSE_DENSITY, M_COLS, N_ROWS, _counts, _model, _twin_bound
from test_partial_fit_gpu import KERNEL_KS, _operands, _stored_pair_expectations, _svi
from test_zi_foldin_gpu import KS, MP, PI_ONE, PI_ZERO, _f64, _fitted, _masks, _padded, _storing, rate_case  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
DEV = 'cuda'
EPS = 2.0 ** -52
N_TOTAL, RHO = 5000, 0.4
GENE_KEYS = ('b1', 'b2', 'V_hat', 'log_V_hat')
STATE_KEYS = zsvi.PRIORS + ('b1', 'b2', 'pi_d', 'V_hat', 'log_V_hat')


# ---- 1. the rate entry against float64 ----------------------------------------------------------------------------------------

def _ranges(n, K, mp=MP):
    from oriana_amd import _lib
    return int(_lib.load().oriana_zi_gene_rate_ranges(n, mp, K))


def _gene_rate(X, U, V, pi_d, mp=MP):
    """oriana_zi_gene_rate into NaN-filled outputs with NaN-filled scratch: (G (mp, K), dsum [mp]) on the device; mp: the gene
    count the entry is given (the genes of V, then inert ones)."""
    from oriana_amd import _lib
    from oriana_amd._lib import call, ptr, stream_ptr
    n, K = U.shape
    _, mask, _ = _masks(X, mp=mp)
    Vp, pip = _padded(V, pi_d, mp)
    Ud = _f64(U)
    scratch = torch.full((int(_lib.load().oriana_zi_gene_rate_scratch_doubles(n, mp, K)),), float('nan'), dtype=F64, device=DEV)
    G = torch.full((mp, K), float('nan'), dtype=F64, device=DEV)
    dsum = torch.full((mp,), float('nan'), dtype=F64, device=DEV)
    call('oriana_zi_gene_rate', ptr(G), ptr(dsum), ptr(Ud), ptr(Vp), ptr(pip), ptr(mask), ptr(scratch), n, mp, K, stream_ptr())
    torch.cuda.synchronize()
    return G, dsum


@pytest.mark.parametrize('nq', [N_ROWS, 1, 255])
@pytest.mark.parametrize('K', KS)
def test_gene_rate_against_float64(rate_case, K, nq):
    X, U, V, pi_d, _ = rate_case(K)
    if nq < N_ROWS:
        X, U = X[12:12 + nq], U[12:12 + nq]
    d = zr.dropout_f32(X, V, pi_d, U).astype(np.float64)
    refG, refd = d.T @ U, d.sum(axis=0)
    G, dsum = _gene_rate(X, U, V, pi_d)
    G2, dsum2 = _gene_rate(X, U, V, pi_d)
    S = _ranges(nq, K)
    e = err_colrel(G[:M_COLS].cpu().numpy(), refG)
    ed = float(np.max(np.abs(dsum[:M_COLS].cpu().numpy() - refd))) / nq
    print('K=%d n\'=%d: %d cell ranges; G against float64 %.3e (bound %.1e); dsum / n\' %.3e absolute (bound %.1e)'
          % (K, nq, S, e, RTOL, ed, KEY_ATOL['p_d']))
    assert bool(torch.isfinite(G).all()) and bool(torch.isfinite(dsum).all()), 'an element of G or dsum was not written'
    assert torch.equal(G, G2) and torch.equal(dsum, dsum2), 'two runs differ'
    assert e <= RTOL
    # a mean of probabilities, each within the bound, is within it
    assert ed <= KEY_ATOL['p_d']
    if nq == N_ROWS:
        assert S > 1, 'the case does not cover more than one cell range'
    # the two column overrides: 1 at the non-zeros and 1e-10 at the zeros (pi_d = 0), 1 everywhere (pi_d = 1).  The first is a
    # sum of S partials nnz_r + 1e-10 (cells_r - nnz_r), each two roundings, added in order: (S + 3) ulp of the total
    nnz = float((X[:, PI_ZERO] != 0).sum())
    want = nnz + 1e-10 * (nq - nnz)
    got0, got1 = float(dsum[PI_ZERO]), float(dsum[PI_ONE])
    print('  pi_d = 0 column: %.17g against %.17g; pi_d = 1 column: %.17g' % (got0, want, got1))
    assert abs(got0 - want) <= (S + 3) * EPS * want
    assert got1 == float(nq)


# ---- 2. the rate entry against the storing path on the GPU --------------------------------------------------------------------

@pytest.mark.parametrize('K', KS)
def test_gene_rate_against_the_storing_entry(rate_case, K):
    """D from oriana_dropout_sweep_fused_tiles (ORIANA_MATRIX_F32) and D^T U in float64: two results, each within the header's 3e-7
    of float64 (the argument of test_zi_foldin_gpu.test_rate_against_float64)."""
    X, U, V, pi_d, _ = rate_case(K)
    G, _ = _gene_rate(X, U, V, pi_d)
    _, D = _storing(X, U, V, pi_d, 0)
    ref = torch.from_numpy(D[:, :M_COLS]).to(DEV).double().T @ _f64(U)
    e = err_colrel(G[:M_COLS].cpu().numpy(), ref.cpu().numpy())
    print('K=%d: G against the stored D_hat^T U %.3e (bound 6e-7)' % (K, e))
    assert e <= 6e-7


# ---- 3. return codes ----------------------------------------------------------------------------------------------------------

def test_gene_rate_return_codes():
    from oriana_amd import _lib
    from oriana_amd._lib import ptr, stream_ptr
    f = _lib.load().oriana_zi_gene_rate
    t = torch.zeros(64, dtype=F64, device=DEV)
    assert f(ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), 4, 4, 129, stream_ptr()) == -2       # ORIANA_EKRANGE
    assert f(ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), 4, 4, 0, stream_ptr()) == -1         # ORIANA_EINVAL
    G = torch.full((4, 5), float('nan'), dtype=F64, device=DEV)
    dsum = torch.full((4,), float('nan'), dtype=F64, device=DEV)
    assert f(ptr(G), ptr(dsum), None, None, None, None, None, 0, 4, 5, stream_ptr()) == 0                 # no cells: zeros, written
    torch.cuda.synchronize()
    assert bool((G == 0).all()) and bool((dsum == 0).all())
    lib = _lib.load()
    assert lib.oriana_zi_gene_rate_scratch_doubles(0, 4, 5) == 0 and lib.oriana_zi_gene_rate_scratch_doubles(4, 4, 129) == 0


# ---- 4. the blend with a matrix statistic --------------------------------------------------------------------------------------

def _svi_mat(d, rate, scale, rho):
    """One oriana_svi_gene_update_mat on clones of d's b1, b2: (b1, b2, E, Elog, sums (2, K), Z)."""
    from oriana_amd._lib import call, ptr, stream_ptr
    m, K = d['b1'].shape
    b1, b2, E = d['b1'].clone(), d['b2'].clone(), torch.empty(m, K, dtype=F64, device=DEV)
    El, sums, Z = torch.empty(m, K, dtype=F32, device=DEV), torch.zeros(2, K, dtype=F64, device=DEV), d['Z'].clone()
    call('oriana_svi_gene_update_mat', ptr(b1), ptr(b2), ptr(E), ptr(El), ptr(sums[0]), ptr(sums[1]), ptr(d['beta1']), ptr(d['beta2']),
         ptr(Z), None, None, 1, None, ptr(rate), float(scale), float(rho), m, K, stream_ptr())
    torch.cuda.synchronize()
    return b1, b2, E, El, sums, Z


def _rate_matrix(K, m=M_COLS):
    return np.random.default_rng(900 + K).gamma(2.0, 30.0, size=(m, K))


@pytest.mark.parametrize('K', KERNEL_KS)
def test_mat_blend_against_float64(K):
    scale, rho = 3.7, 0.3
    h, d = _operands(K)
    rate = _rate_matrix(K)
    b1, b2, E, El, sums, Z = _svi_mat(d, _f64(rate), scale, rho)
    assert torch.equal(Z, d['Z'])
    ref1 = np.maximum(1e-15, (1 - rho) * h['b1'] + rho * (h['beta1'][None, :] + scale * h['Z'].astype(np.float64)))
    ref2 = np.maximum(1e-15, (1 - rho) * h['b2'] + rho * (h['beta2'][None, :] + scale * rate))
    e1 = float(np.max(np.abs(b1.cpu().numpy() - ref1) / ref1))
    e2 = float(np.max(np.abs(b2.cpu().numpy() - ref2) / ref2))
    print('K=%d: b1 %.3e b2 %.3e relative to NumPy float64 (bound 1e-14)' % (K, e1, e2))
    assert e1 <= 1e-14 and e2 <= 1e-14
    E0, El0, sums0 = _stored_pair_expectations(b1, b2)
    assert torch.equal(E, E0) and torch.equal(El, El0)
    assert float(((sums - sums0).abs() / sums0.abs().clamp_min(1e-300)).max()) <= 1e-12
    assert torch.isfinite(E).all() and torch.isfinite(El).all()


@pytest.mark.parametrize('K', KERNEL_KS)
def test_mat_blend_at_the_ends_of_rho(K):
    h, d = _operands(K)
    rate = _rate_matrix(K)
    b1, b2, E, El, _, _ = _svi_mat(d, _f64(rate), 3.7, 0.0)
    assert torch.equal(b1, d['b1']) and torch.equal(b2, d['b2'])
    E0, El0, _ = _stored_pair_expectations(d['b1'], d['b2'])
    assert torch.equal(E, E0) and torch.equal(El, El0)
    # rho = 1, scale = 1: the old pair multiplied by 0, prior + statistic in one rounding
    b1, b2, _, _, _, _ = _svi_mat(d, _f64(rate), 1.0, 1.0)
    assert np.array_equal(b1.cpu().numpy(), np.maximum(1e-15, h['beta1'][None, :] + h['Z'].astype(np.float64)))
    assert np.array_equal(b2.cpu().numpy(), np.maximum(1e-15, h['beta2'][None, :] + rate))


@pytest.mark.parametrize('K', KERNEL_KS)
def test_mat_blend_of_equal_rows_is_the_vector_entry(K):
    h, d = _operands(K)
    rate = d['sum_u'][None, :].expand(M_COLS, K).contiguous()
    got, ref = _svi_mat(d, rate, 3.7, 0.3), _svi(d, 3.7, 0.3)
    for x, y in zip(got[:4] + got[5:], ref[:4] + ref[5:]):
        assert torch.equal(x, y)
    assert float(((got[4] - ref[4]).abs() / ref[4].abs().clamp_min(1e-300)).max()) <= 1e-12


# ---- 5. one call against float64 ----------------------------------------------------------------------------------------------

def _ref_state(st):
    return {k: st[k] for k in STATE_KEYS}


def _one_call(K, nb, n_iter):
    """The errors of one fold_in_fit call (given start, no freezing) against the reference on the same state."""
    G = _fitted(K)
    Xq = _counts(K + 50) if nb == N_ROWS else _counts(9)[12:12 + nb]
    n_total = N_TOTAL if nb == N_ROWS else 10 * nb
    a1_0 = np.random.default_rng(70 + K).gamma(1.0, 1.0, size=(nb, K))
    st = G.state()
    ref, info = zsvi.fold_in_fit(Xq, _ref_state(st), n_total, RHO, a1_0, n_iter, 0.0)
    assert G.fold_in_fit(Xq, n_total, rho=RHO, init=a1_0, n_iter=n_iter, tol=0) is G
    got = G.state()
    errs = {k: err_colrel(got[k], ref[k]) for k in GENE_KEYS}
    e_pi = float(np.max(np.abs(got['pi_d'] - ref['pi_d'])))
    print('K=%d n_B=%d n_iter=%d: %s pi_d %.3e absolute' % (K, nb, n_iter, ' '.join('%s %.3e' % kv for kv in errs.items()), e_pi))
    assert all(np.isfinite(got[k]).all() for k in GENE_KEYS + ('pi_d',))
    assert G.fold_in_fit_unconverged_ == nb and G.fold_in_fit_rho_ == RHO and G.n_batches_ == 1
    return errs, e_pi


@pytest.mark.parametrize('nb', [N_ROWS, 1, 5])
@pytest.mark.parametrize('K', KS)
def test_one_call_against_float64(K, nb):
    errs, e_pi = _one_call(K, nb, 1)
    assert max(errs.values()) <= RTOL, errs
    assert e_pi <= RHO * KEY_ATOL['p_d']


# Three iterations of the local step before the statistics: the float32 evaluation error of each iteration's sums and of d
# enters the next one's pair.  Measured on an MI355X, worst over the four K in err_colrel (the convention of N_ITER3_BOUND in
# tests/test_partial_fit_gpu.py; each at K = 128 but b2, K = 20; one iteration: 3.1e-7, 1.8e-7, 2.4e-7, 1.5e-7):
N_ITER3_MEASURED = dict(b1=3.954e-7, b2=2.661e-7, V_hat=3.097e-7, log_V_hat=1.360e-7)
N_ITER3_BOUND = min(1e-4, 3 * max(N_ITER3_MEASURED.values()))       # three times the measured worst value, never above 1e-4


@pytest.mark.parametrize('K', KS)
def test_three_iterations_against_float64(K):
    errs, e_pi = _one_call(K, N_ROWS, 3)
    assert max(errs.values()) <= N_ITER3_BOUND, errs


# ---- 6. the state after a call is coherent ------------------------------------------------------------------------------------

def test_state_after_a_call_is_what_load_state_leaves():
    """Everything a sweep, fold_in() and fold_in_score() read from the gene side, against a twin that loaded the state."""
    K = 50
    X = _counts(K)
    A = _model(X, K, name='ZIGaP', seed=K)
    for _ in range(2):
        A.step()
    assert A._DV_next is not None, 'the case does not cover a kept D_hat V product'
    A.fold_in_fit(_counts(K + 50)[:300], N_TOTAL, rho=RHO, n_iter=4)
    assert A._DV_next is None
    B = _model(X, K, name='ZIGaP', seed=K)
    B.load_state(A.state())
    Xq = _counts(K + 51)[:200]
    a1_0 = np.random.default_rng(K).gamma(1.0, 1.0, size=(200, K))
    ta, tb = (G.fold_in(Xq, n_iter=1, tol=0, init=a1_0) for G in (A, B))
    assert err_colrel(ta, tb) <= RTOL
    sa, sb = (G.fold_in_score(Xq, n_iter=3) for G in (A, B))
    print('fold_in_score: %.17g against the twin\'s %.17g' % (sa, sb))
    assert abs(sa - sb) <= RTOL * abs(sb)
    kept = A.n_kept_products
    A.step(); B.step()
    assert A.n_kept_products == kept, 'the sweep after the call used a product formed from the old V_hat'
    sa, sb = A.state(), B.state()
    tol = _twin_bound(A.n, 3)
    for k in sa:
        e = err_colrel(sa[k], sb[k]) if sb[k].size else 0.0
        print('%s: %.3e (bound %.3e)' % (k, e, tol))
        assert e <= tol, k


def test_graph_capture_is_not_offered_on_zi_models():
    """The gene side is written in place so that a captured sweep would keep its buffers -- but capture_graph() refuses the
    zero-inflated models (their lazy p_d is host-side state), so there is no captured ZI sweep to run the twin test with."""
    A = _model(_counts(20), 20, name='ZIGaP', seed=20)
    with pytest.raises(RuntimeError, match='zero-inflated'):
        A.capture_graph()


# ---- 7. what a call does not write --------------------------------------------------------------------------------------------

def test_cell_side_priors_and_masks_are_not_written():
    K = 20
    G = _fitted(K)
    kept = {k: getattr(G, k).tensor.clone() for k in ('a1', 'a2', 'alpha1', 'alpha2', 'beta1', 'beta2')}
    for k in ('_log_U_hat', '_U_hat', '_Dp', '_nzmask', '_nztiles', '_nnz_gene_p', '_pd_sum_p'):
        kept[k] = getattr(G, k).clone()
    fresh, unconv = G._pd_sum_fresh, G.fold_in_unconverged_
    written = lambda: (G.b1.tensor, G.b2.tensor, G._V_hat, G._log_V_hat, G.pi_d.tensor, G._sumV)
    ptrs = tuple(t.data_ptr() for t in written())
    before, pi_before = G.b1[:].copy(), G.pi_d[:].copy()
    Xb = _counts(K + 50)
    assert G.n_batches_ == 0 and G.fold_in_fit_rho_ is None and G.fold_in_fit_unconverged_ is None
    for t, want in enumerate((1.0, 2.0 ** -0.7, 3.0 ** -0.7)):
        G.fold_in_fit(Xb[100 * t:100 * t + 100], N_TOTAL, n_iter=3)
        assert G.n_batches_ == t + 1 and G.fold_in_fit_rho_ == want
        assert G.fold_in_fit_unconverged_ is not None and G._v_sums_in_acc is False and G._DV_next is None
    assert G.fold_in_unconverged_ == unconv and G._pd_sum_fresh == fresh
    assert ptrs == tuple(t.data_ptr() for t in written()), 'a buffer was replaced'
    assert not np.array_equal(G.b1[:], before) and not np.array_equal(G.pi_d[:], pi_before)
    for k, t in kept.items():
        now = getattr(G, k)
        assert torch.equal(now if isinstance(now, torch.Tensor) else now.tensor, t), k
    pi_now = G.pi_d.tensor.clone()
    G.fold_in_fit(Xb[:50], N_TOTAL, rho=0.25, tau0=2.0, kappa=1.0, n_iter=1, update_pi_d=False)
    assert G.fold_in_fit_rho_ == 0.25 and G.n_batches_ == 4
    assert torch.equal(G.pi_d.tensor, pi_now), 'update_pi_d=False moved pi_d'
    torch.cuda.synchronize()
    assert torch.allclose(G._sumV[0], G._V_hat.sum(0), rtol=1e-12, atol=0)


# ---- 8. the stream ------------------------------------------------------------------------------------------------------------

def test_warm_started_stream_recovers_the_float64_gain():
    """The stream of tests/test_zi_fold_in_fit_host.py through the GPU model: after 4 and after 8 calls the float64 population
    bound of the model's gene side has at least 90 % of the float64 stream's gain over the warm state."""
    import oriana_amd.models as M
    (X, a1, b1, K), _, _ = zr.planted_case()
    X, a1, b1 = np.array(X), np.array(a1), np.array(b1)
    n, w = X.shape[0], svi.WARM_CELLS
    warm, fit = zsvi.warm_state(X, a1, b1)
    states, _ = zsvi.stream(X, warm, 8)
    base = zsvi.population_bound(X, warm)
    G = M.ZIGaP(X[:w], k=K, init=(a1[:w], b1))
    G.load_state({k: np.array(fit[k]) for k in zsvi.PRIORS + ('a1', 'a2', 'b1', 'b2', 'pi_d', 'p_d')})
    G.update_expectations()
    for t, rows in enumerate(svi.stream_batches(n, 8)):
        G.fold_in_fit(X[rows], n, n_iter=300, tol=1e-4)
        assert G.fold_in_fit_unconverged_ == 0 and G.fold_in_fit_rho_ == svi.stream_rho(t)
        if t + 1 in (4, 8):
            st = G.state()
            got = zsvi.population_bound(X, {k: st[k] for k in zsvi.PRIORS + ('b1', 'b2', 'pi_d')})
            want = zsvi.population_bound(X, states[t + 1])
            print('after %d calls: GPU %.3f float64 %.3f |GPU - float64| %.3e; gains %.1f against %.1f over the warm %.1f'
                  % (t + 1, got, want, abs(got - want), got - base, want - base, base))
            assert want > base
            assert got - base >= 0.9 * (want - base)
    for k in zsvi.PRIORS:
        assert np.array_equal(G.state()[k], fit[k]), k


# ---- 9. no (n_B, m) matrix ----------------------------------------------------------------------------------------------------

def test_footprint_stays_below_one_D_hat():
    import scipy.sparse as sp
    import oriana_amd.models as M
    from oriana_amd import engine
    nq, m, K = 4096, 8192, 50
    rng = np.random.default_rng(77)

    def draw(n):
        A = sp.random(n, m, density=0.02, format='csr', random_state=rng, data_rvs=lambda s: rng.poisson(3.0, size=s) + 1.0)
        return A.astype(np.float64)
    G = M.ZIGaP(draw(64), k=K, init=(rng.gamma(1.0, 1.0, size=(64, K)), rng.gamma(1.0, 1.0, size=(m, K))))
    G.step()
    ct = engine.CountTiles.from_scipy(draw(nq), G.device)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    G.fold_in_fit(ct, 100000, n_iter=2)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    one_D_hat = nq * ((m + 3) // 4 * 4) * 4
    print('peak growth across fold_in_fit: %.1f MB; one D_hat of the batch: %.1f MB' % (peak / 1e6, one_D_hat / 1e6))
    assert np.isfinite(G.b2[:]).all() and np.isfinite(G.pi_d[:]).all()
    assert peak < one_D_hat


# ---- 10. refusals and edges ---------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused():
    from oriana_amd import engine
    G = _fitted(20, sweeps=0)
    Xb = _counts(1)[:40]
    st = G.state()
    for kw in (dict(tau0=0.0), dict(tau0=-1.0), dict(kappa=0.5), dict(kappa=1.01), dict(rho=-0.01), dict(rho=1.01)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            G.fold_in_fit(Xb, 1000, **kw)
    with pytest.raises(ValueError, match='n_total'):
        G.fold_in_fit(Xb, 39)
    with pytest.raises(ValueError, match=r'fold_in_fit\(\).*genes'):
        G.fold_in_fit(np.zeros((4, M_COLS + 1)), 1000)
    with pytest.raises(ValueError, match='sliced layout'):
        G.fold_in_fit(engine.CountTiles.from_dense(_counts(1), G.device, dense_density=DENSE_DENSITY), 1000)
    with pytest.raises(ValueError, match='init'):
        G.fold_in_fit(Xb, 1000, init=np.ones((41, 20)))
    G.sharded = True                                    # (what a row-sharded model says of itself)
    with pytest.raises(NotImplementedError, match='sharding'):
        G.fold_in_fit(Xb, 1000)
    G.sharded = False
    now = G.state()
    assert all(np.array_equal(now[k], st[k]) for k in st) and G.n_batches_ == 0
    wide = _model(_counts(2)[:300], 129, name='ZIGaP', seed=2)
    with pytest.raises(ValueError, match='128'):
        wide.fold_in_fit(_counts(3)[:10], 1000)


def test_no_cells_change_nothing():
    G = _fitted(20, sweeps=1)
    st, sums, ver = G.state(), G._sumV.clone(), G._ver
    assert G.fold_in_fit(np.zeros((0, M_COLS)), 10, rho=1.0) is G
    now = G.state()
    assert all(np.array_equal(now[k], st[k]) for k in st) and torch.equal(G._sumV, sums)
    assert G.n_batches_ == 0 and G.fold_in_fit_rho_ is None and G._ver == ver


def test_partial_fit_points_to_fold_in_fit():
    G = _model(_counts(2)[:300], 5, name='ZIGaP', seed=2)
    with pytest.raises(NotImplementedError, match='pCMF') as ei:
        G.partial_fit(_counts(3)[:10], 1000)
    assert 'fold_in_fit' in str(ei.value)
    S = _model(_counts(2)[:300], 5, name='SparseZIGaP', seed=2)
    assert not hasattr(S, 'fold_in_fit')
    with pytest.raises(NotImplementedError, match='pCMF'):
        S.partial_fit(_counts(3)[:10], 1000)
