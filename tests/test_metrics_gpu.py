# -*- coding: utf-8 -*-
"""The convergence metrics (reconstruction_deviance, explained_deviance, frobenius_norm, loglikelihood_X) of every model,
kernel family and layout against a float64 restatement written here, term by term.

The reference (`_reference`) evaluates the formulas of models/base.py (the comment above _count_constants: reference
base.py:58-87 with sparse_zigap.py:44-51) on the model's own state: X as the float32 counts the model holds, promoted to
float64; U_hat, V_eff = V_hat * S_hat and pi_d in float64; D_hat as the float32 values the model holds, with
M = {round(D_hat) == 0}.  Every sum is taken in long double.

Tolerances are derived from the arithmetic, never measured on the code under test (`_bounds`): the row pass forms
Lambda at the stored entries from float32 casts of the factors -- a K-term float32 dot, two casts, a reciprocal and the
float32 s = x / Lambda -- so |dLambda_ij| <= gamma Lambda_ij with gamma = (K + 3) 2^-24 (all factors are non-negative:
sum_k U_ik V_jk = Lambda_ij), propagated into each sum.  Everything else (the dense block, the float64 fall-back, the
dropout metric kernel, the Gram matrices) is float64.  As in tests/helpers.py (PS_FACTOR), the bound is the larger of
that and F_REF times the distance of a float32 evaluation (Lambda from float32 factors, as the reference's own float32
arithmetic forms it) from float64.  Two runs of the same sweeps (sections 4 and 5) differ only in the order in which float
atomics combine partial sums and are held to `_twin_bound`, an atomic-order bound of the same kind.
"""
import numpy as np
import pytest
import torch

from helpers import err_colrel

pytestmark = pytest.mark.gpu

F_REF = 8.0                      # times the float32 evaluation's distance from float64 (helpers.PS_FACTOR)
ACC = 1e-12                      # float64 accumulation (atomics in any order, log / exp to an ulp), relative to sum |term|
KS = (1, 20, 36, 50, 64, 68, 84, 100, 128, 129, 200, 256)
KP = {1: 16, 20: 20, 36: 36, 50: 52, 64: 64, 68: 68, 84: 84, 100: 100, 128: 128, 129: 160, 200: 224, 256: 256}
MODELS = (('GaP', True), ('ZIGaP', True), ('ZIGaP', False), ('SparseGaP', True), ('SparseZIGaP', True))
N_ROWS = 3 * 256 + 37            # a partial last row tile
M_COLS = 301                     # not a multiple of 4 or 32; two column tiles, the last one partial
DENSE_DENSITY = 0.5


def _ld(a):
    return np.sum(np.asarray(a, dtype=np.longdouble))


def _counts(seed, n=N_ROWS, m=M_COLS):
    """Integer counts: 70 genes dense enough for the hybrid block (-> gd = 64), the rest at 15 %; an all-zero gene (5), an
    all-zero cell (11), a gene expressed in every cell but that one (250)."""
    rng = np.random.default_rng(seed)
    dens = np.full(m, 0.15)
    dens[:70] = 0.8
    X = ((rng.poisson(rng.gamma(0.6, 4.0, size=(n, m))) + 1) * (rng.random((n, m)) < dens)).astype(np.float64)
    X[:, 250] = rng.poisson(6.0, size=n) + 1
    X[:, 5] = 0
    X[11, :] = 0
    return X


def _model(name, X, K, quirks=True, dense_density=None, seed=0, **kw):
    import oriana_amd.models as M
    rng = np.random.default_rng(1000 + seed)
    n, m = X.shape
    a1 = rng.gamma(1.0, 1.0, size=(n, K))
    b1 = rng.gamma(1.0, 1.0, size=(m, K))
    return getattr(M, name)(X, k=K, init=(a1, b1), reference_quirks=quirks, dense_density=dense_density, **kw)


HYBRID_KS = (1, 20, 36, 50, 64, 68, 84, 100)    # the K the dense-block kernels are compiled for (engine.dense_supported)


def _evaluate(X, U, V, pi, keep0, lam_fix=None):
    """The public values and the internal terms for the rate matrix U V^T (float64 unless U, V are float32).  `lam_fix`:
    the float64 rates that replace the entries below 1e-10 (the region the HIP code evaluates in float64)."""
    N = X != 0
    Lam = (U @ V.T).astype(np.float64)
    if lam_fix is not None:
        small = ~(Lam >= 1e-10)
        Lam[small] = lam_fix[small]
    n, m = X.shape
    P = np.broadcast_to(pi[np.newaxis, :], (n, m))
    x, lam, p = X[N], Lam[N], P[N]
    lz, pz = Lam[keep0], P[keep0]
    mu = X.sum(axis=0, dtype=np.longdouble).astype(np.float64) / n
    Mu = np.broadcast_to(mu[np.newaxis, :], (n, m))
    Z = ~N
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        xlogl = x * np.log(lam)
        # (pi = 1, the models without a dropout node: log(pi e^-L + 1 - pi) reduces to -L -- literally evaluated it would
        #  underflow to log 0 from L ~ 745 on, which is no property of the model)
        tz0 = np.where(pz == 1.0, -lz, np.log(pz * np.exp(-lz) + (1.0 - pz)))
        lpi = np.log(p)
        xlx = x * np.log(x) - x
        mean_z = np.where(P[Z] == 1.0, -Mu[Z], np.log(P[Z] * np.exp(-Mu[Z]) + (1.0 - P[Z])))
        mean_n = lpi - Mu[N] + x * np.log(np.where(Mu[N] > 0, Mu[N], 1.0))
    t = dict(nz=np.array([_ld(lam), _ld(xlogl), _ld(lam * lam), _ld(x * lam)], dtype=np.float64),
             zz=np.array([_ld(tz0), _ld(lz * lz)], dtype=np.float64),
             xc=np.array([_ld(xlx), _ld(x * x)], dtype=np.float64))
    ll_x = _ld(lpi) + _ld(xlx)                                            # zeros: log(pi + 1 - pi) = 0
    ll_uv = _ld(tz0) + _ld(lpi) - _ld(lam) + _ld(xlogl)                   # M: Lambda = 0, log 1 = 0
    ll_mean = _ld(mean_z) + _ld(mean_n)
    t.update(ll_x=float(ll_x), ll_uv=float(ll_uv), ll_mean=float(ll_mean), rd=float(-2.0 * (ll_uv - ll_x)),
             ed=float((ll_uv - ll_mean) / (ll_x - ll_mean)),
             fn=float(np.sqrt(_ld((lam - x) ** 2) + _ld(lz * lz))))
    t['abs'] = dict(lam=float(_ld(lam)), x=float(_ld(x)), lam2=float(_ld(lam * lam)), xlam=float(_ld(x * lam)),
                    xlogl=float(_ld(np.abs(xlogl))), tz0=float(_ld(np.abs(tz0))), lz=float(_ld(lz)), lz2=float(_ld(lz * lz)),
                    lpi=float(_ld(np.abs(lpi))), xlx=float(_ld(np.abs(xlx))), x2=float(_ld(x * x)),
                    mean=float(_ld(np.abs(mean_z)) + _ld(np.abs(mean_n))),
                    all_lam=float(_ld(Lam)), all_lam2=float(_ld(Lam * Lam)))
    return t


def _reference(G, X):
    """float64 reference of the model's metrics on its current state, with the tolerances of every value."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)           # the counts the model holds
    n, m = X.shape
    U = G.U_hat
    V = G.V_hat * G.S_hat.astype(np.float64) if G.sparse else G.V_hat
    pi = G.pi_d[:] if G.zi else np.ones(m)
    keep0 = (X == 0) & (np.round(G.D_hat.astype(np.float64)) != 0) if G.zi else (X == 0)
    ref = _evaluate(X, U, V, pi, keep0)
    ref['colsum'] = X.sum(axis=0, dtype=np.longdouble).astype(np.float64)
    ref['colnnz'] = (X != 0).sum(axis=0).astype(np.float64)
    # the float32 evaluation: Lambda from float32 factors in float32
    lam64 = U @ V.T
    f32 = _evaluate(X, U.astype(np.float32), V.astype(np.float32), pi, keep0, lam_fix=lam64)
    ref['tol'] = _bounds(ref, f32, G.k, G.zi)
    return ref


def _bounds(ref, f32, K, zi):
    a = ref['abs']
    g = (K + 3) * 2.0 ** -24
    b_nz = np.array([g * a['lam'], -np.log1p(-g) * a['x'], (2 * g + g * g) * a['lam2'], g * a['xlam']])
    b_nz += ACC * np.array([a['lam'], a['xlogl'], a['lam2'], a['xlam']])
    if zi:                       # the dropout metric kernel: float64 matrix cores
        b_zz = ACC * np.array([a['tz0'] + a['lz'], a['lz2']])
    else:                        # (all entries, from float64 Gram matrices) - (non-zeros)
        b_zz = np.array([b_nz[0] + ACC * a['all_lam'], b_nz[2] + ACC * a['all_lam2']])
    b_llx = ACC * (a['xlx'] + a['lpi'])
    if zi:
        b_lluv = b_zz[0] + b_nz[0] + b_nz[1] + ACC * a['lpi']
    else:                        # ll_uv = -(all_lam - nz[0]) - nz[0] + nz[1] + ...: sum_N Lambda cancels
        b_lluv = ACC * a['all_lam'] + b_nz[1] + ACC * a['lpi']
    b_mean = ACC * (a['mean'] + a['lpi'])
    den = abs(ref['ll_x'] - ref['ll_mean'])
    b_ed = (b_lluv + b_mean + abs(ref['ed']) * (b_llx + b_mean)) / den if den > 0 else np.inf
    if zi:
        b_f2 = b_nz[2] + 2 * b_nz[3] + b_zz[1] + ACC * (a['x2'] + a['lam2'] + 2 * a['xlam'])
    else:                        # sum_N Lambda^2 cancels against the Gram term
        b_f2 = 2 * b_nz[3] + ACC * (a['all_lam2'] + a['x2'] + 2 * a['xlam'])
    # |sqrt(A) - sqrt(B)| = |A - B| / (sqrt(A) + sqrt(B)) and sqrt(A) >= sqrt(max(B - b_f2, 0))
    # (This is a worst case: every float32 rate off by gamma in the same direction.  The rounding errors of the rates are not
    #  all of one sign, so on planted high-count data -- K = 4, mean 3000 -- the norm comes out ~100 times closer than the
    #  bound, 2.9e-5 against 2.5e-3 relative: the bound tells an error of the arithmetic from a wrong term, not the digits.)
    f = ref['fn']
    b_fn = b_f2 / (f + np.sqrt(max(f * f - b_f2, 0.0))) if f > 0 else np.sqrt(b_f2)
    tol = dict(nz=b_nz, zz=b_zz, ll_x=b_llx, ll_uv=b_lluv, ll_mean=b_mean, rd=2 * (b_lluv + b_llx), ed=b_ed, fn=b_fn)
    for k in ('nz', 'zz'):
        tol[k] = np.fmax(tol[k], F_REF * _diff(f32[k], ref[k]))
    for k in ('ll_x', 'll_uv', 'll_mean', 'rd', 'ed', 'fn'):
        tol[k] = float(np.fmax(tol[k], F_REF * _diff(f32[k], ref[k])))
    return tol


def _hip(G):
    colsum, colnnz, xc = G._count_constants()
    ll_x, ll_uv, ll_mean, nz, zz, _ = G._loglikelihoods()
    return dict(colsum=colsum.cpu().numpy(), colnnz=colnnz.cpu().numpy(), xc=xc.cpu().numpy(), nz=nz.cpu().numpy(),
                zz=zz.cpu().numpy(), ll_x=ll_x, ll_uv=ll_uv, ll_mean=ll_mean, rd=G.reconstruction_deviance(),
                ed=G.explained_deviance(), fn=G.frobenius_norm(), ll=[G.loglikelihood_X(w) for w in ('counts', 'factors', 'mean')])


def _diff(got, ref):
    """|got - ref|, 0 where both are the same infinity (an infinite reference is matched exactly, never within a bound)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.where(got == ref, 0.0, np.abs(got - ref))


def _check(G, X, what, integer=True):
    ref = _reference(G, X)
    got = _hip(G)
    tol = ref['tol']
    if integer:                  # integer counts, totals below 2^53: exact
        assert np.array_equal(got['colsum'], ref['colsum']), '%s colsum: max diff %.17g' % (
            what, np.abs(got['colsum'] - ref['colsum']).max())
    else:
        assert np.all(np.abs(got['colsum'] - ref['colsum']) <= 1e-13 * np.abs(ref['colsum'])), what + ' colsum'
    assert np.array_equal(got['colnnz'], ref['colnnz']), what + ' colnnz'
    assert np.all(np.abs(got['xc'] - ref['xc']) <= 1e-13 * np.array([ref['abs']['xlx'], ref['abs']['x2']])), \
        '%s xc %r vs %r' % (what, got['xc'], ref['xc'])
    for k in ('nz', 'zz'):
        d = _diff(got[k], ref[k])
        assert np.all(np.isfinite(d) & (d <= tol[k])), '%s %s: diff %r > bound %r (HIP %r, ref %r)' % (
            what, k, d, tol[k], got[k], ref[k])
    for k in ('ll_x', 'll_uv', 'll_mean', 'rd', 'ed', 'fn'):
        d = float(_diff(got[k], ref[k]))
        assert np.isfinite(d) and d <= tol[k], '%s %s: HIP %.17g ref %.17g diff %.3e > bound %.3e' % (
            what, k, got[k], ref[k], d, tol[k])
    for v, k in zip(got['ll'], ('ll_x', 'll_uv', 'll_mean')):
        d = float(_diff(v, ref[k]))
        assert np.isfinite(d) and d <= tol[k], '%s loglikelihood_X %s' % (what, k)
    return got, ref


# ---- 2. the case matrix ---------------------------------------------------------------------------------------------------

def _cases():
    out = []
    for name, quirks in MODELS:
        for K in KS:
            for dd in ([None, DENSE_DENSITY] if K in HYBRID_KS else [None]):
                out.append(pytest.param(name, quirks, K, dd, id='%s%s-K%d-%s' % (name, '' if quirks else '-noquirks', K,
                                                                                   'hybrid' if dd else 'sliced')))
    return out


@pytest.mark.parametrize('name,quirks,K,dd', _cases())
def test_metrics_against_float64(name, quirks, K, dd):
    """Every model, every Kp family of the row pass in the form the metrics use, both ZI metric kernels (K <= 128 and
    above), the sliced and the hybrid layout: two sweeps from a seeded start, then each metric term against float64."""
    from oriana_amd import engine
    assert engine.dense_supported(K) == (K in HYBRID_KS), 'the hybrid cases of this matrix are out of date'
    X = _counts(K)
    G = _model(name, X, K, quirks=quirks, dense_density=dd, seed=K)
    assert G._ws.Kp == KP[K], 'K=%d runs in the Kp=%d family, expected %d' % (K, G._ws.Kp, KP[K])
    if dd:
        assert G.counts.gd >= 32 and G.counts.dense is not None, 'the hybrid case has no dense block'
    else:
        assert G.counts.gd == 0
    for _ in range(2):
        G.step()
    _check(G, X, '%s K=%d %s' % (name, K, 'hybrid' if dd else 'sliced'))


# ---- 3. edge entries ------------------------------------------------------------------------------------------------------

TINY_ROWS = (0, 7, 15, 240, 247, 255, 256 + 16 * 5 + 3, 768 + 7, 800, 804)    # row-in-slice 0 / 7 / 15, slices 0 / 15, last tile
UNDERFLOW_ROWS = (255, 804)                                                   # float32(U_hat) == 0 on these rows


@pytest.mark.parametrize('name,K,dd', [('GaP', 20, None), ('GaP', 20, DENSE_DENSITY), ('SparseZIGaP', 68, None),
                                       ('ZIGaP', 100, DENSE_DENSITY), ('SparseGaP', 200, None)])
def test_metric_float64_fallback(name, K, dd):
    """Cells whose rates are below 1e-10 at every stored entry: the row pass leaves its NaN sentinel and k_metric_nnz
    recomputes Lambda in float64, finding the cell from the slot position.  A wrong cell makes x log Lambda differ by
    orders of magnitude.  Hybrid: the same cells' dense genes go through k_dn_metric."""
    X = _counts(3)
    G = _model(name, X, K, dense_density=dd, seed=3)
    if dd:
        assert G.counts.gd >= 32
    G.step()
    U = G.U_hat.copy()
    for i in TINY_ROWS:
        U[i] *= 1e-13
    for i in UNDERFLOW_ROWS:
        U[i] *= 1e-38                                  # ~1e-51: below float32's smallest subnormal
    assert not np.any(U[list(UNDERFLOW_ROWS)].astype(np.float32))
    assert all((X[i] != 0).any() for i in TINY_ROWS)
    G.load_state({'U_hat': U})
    got, ref = _check(G, X, '%s K=%d fallback' % (name, K))
    assert torch.isnan(G._ws.s_rs).any(), 'the row pass left no NaN sentinel: the fall-back was not exercised'
    for k in ('ll_x', 'll_uv', 'll_mean', 'rd', 'ed', 'fn'):
        assert np.isfinite(got[k]) and np.isfinite(ref[k]), k
    assert np.all(np.isfinite(got['nz'])) and np.all(np.isfinite(got['zz']))


@pytest.mark.parametrize('dd', [None, DENSE_DENSITY])
def test_metric_rate_exactly_zero(dd):
    """S_hat = 0 on a whole gene of a sparse model: Lambda = 0 exactly at its non-zero counts, so x log Lambda = -inf --
    the same -inf / +inf as the float64 formulas, not NaN (hybrid: one dense gene and one sliced gene)."""
    X = _counts(4)
    K = 20
    G = _model('SparseGaP', X, K, dense_density=dd, seed=4)
    G.step()
    p_s = G.p_s[:].copy()
    genes = [20, 150] if dd else [150]
    if dd:
        pos = {int(j): p for p, j in enumerate(G.counts.col_perm.cpu().numpy())}
        assert pos[20] < G.counts.gd <= pos[150]
    p_s[genes] = 0.0
    G.load_state({'p_s': p_s})
    assert not G.S_hat[genes].any() and all((X[:, j] != 0).any() for j in genes)
    ref = _reference(G, X)
    got = _hip(G)
    assert ref['ll_uv'] == -np.inf and ref['rd'] == np.inf
    assert got['ll_uv'] == -np.inf and got['rd'] == np.inf and got['ll'][1] == -np.inf
    assert got['nz'][1] == -np.inf and np.all(np.isfinite(got['nz'][[0, 2, 3]]))
    assert got['ed'] == -np.inf
    assert abs(got['fn'] - ref['fn']) <= ref['tol']['fn']


@pytest.mark.parametrize('name,quirks,K', [('ZIGaP', False, 20), ('ZIGaP', True, 200), ('SparseZIGaP', True, 84)])
def test_metric_dropout_half_boundary(name, quirks, K):
    """M = {round(D_hat) == 0} (base.py:60): D_hat = 0.5 exactly is masked (round half to even), one float32 ulp above is
    not, one below is; on zero entries of a ZI model, both ZI metric kernels (K <= 128 and above)."""
    X = _counts(5)
    G = _model(name, X, K, quirks=quirks, seed=5)
    G.step()
    p_d = G.p_d[:].copy()
    zi, zj = np.nonzero(X == 0)
    rng = np.random.default_rng(5)
    pick = rng.permutation(zi.size)[:3 * (zi.size // 6)]
    vals = [np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))]
    for q, v in enumerate(vals):
        sel = pick[q::3]
        p_d[zi[sel], zj[sel]] = np.float64(v)
    G.load_state({'p_d': p_d})
    D = G.D_hat
    for v in vals:
        assert (D == v).sum() > 1000
    _check(G, X, '%s K=%d D_hat = 0.5' % (name, K))


def test_metric_count_edges_dense_block():
    """A gene with a count of 65534 is eligible for the uint16 dense block, one with 65535 is not (engine.py: counts in
    [0, 65535)); both dense enough.  Their constants and metrics on both sides of gd."""
    X = _counts(6)
    X[:300, 30] = 65534
    X[:300, 31] = 65535
    G = _model('GaP', X, 20, dense_density=DENSE_DENSITY, seed=6)
    pos = {int(j): p for p, j in enumerate(G.counts.col_perm.cpu().numpy())}
    assert pos[30] < G.counts.gd <= pos[31], (pos[30], pos[31], G.counts.gd)
    G.step()
    _check(G, X, 'counts 65534 / 65535')


@pytest.mark.parametrize('name', ['GaP', 'SparseZIGaP'])
def test_metric_count_edges_large_sliced(name):
    """A sliced gene with 17 counts of 1000001 in one 256-row tile: their sum (17000017) is past float32's exact range,
    so the per-gene sums of the count constants must not be formed in float32."""
    X = _counts(7)
    X[10:27, 40] = 1000001
    X[300:340, 41] = 999999
    G = _model(name, X, 12, seed=7)
    G.step()
    got, ref = _check(G, X, '%s large counts' % name)
    assert got['colsum'][40] == 17 * 1000001 + X[:10, 40].sum() + X[27:, 40].sum()


@pytest.mark.parametrize('name', ['GaP', 'ZIGaP'])
def test_metric_non_integer_counts(name):
    """Non-integer float counts (the reference's float X): every constant and term in float64 semantics."""
    rng = np.random.default_rng(8)
    X = _counts(8) * rng.uniform(0.3, 1.7, size=(N_ROWS, M_COLS))
    G = _model(name, X, 36, dense_density=DENSE_DENSITY, seed=8)
    assert G.counts.gd == 0                              # (no gene of non-integer counts is eligible for the dense block)
    G.step()
    _check(G, X, '%s float counts' % name, integer=False)


@pytest.mark.parametrize('name', ['GaP', 'SparseGaP'])
def test_metric_well_fitted_high_counts(name):
    """A planted rank-K Poisson matrix with a mean count of ~3000, fitted: the Frobenius norm is a small difference of
    large sums there (sum_N x Lambda against the Gram term), the deviance a small difference of log-likelihoods."""
    rng = np.random.default_rng(9)
    n, m, K = N_ROWS, M_COLS, 4
    Ut = rng.gamma(2.0, 1.0, size=(n, K))
    Vt = rng.gamma(2.0, 1.0, size=(m, K))
    L = Ut @ Vt.T
    L *= 3000.0 / L.mean()
    X = rng.poisson(L).astype(np.float64)
    G = _model(name, X, K, seed=9)
    c = np.sqrt(3000.0 / (Ut @ Vt.T).mean())
    G.load_state({'U_hat': Ut * c, 'V_hat': Vt * c, 'log_U_hat': np.log(Ut * c), 'log_V_hat': np.log(Vt * c)})
    # the planted rates themselves: what is left is the Poisson noise, ~1 / sqrt(3000) of the counts
    assert G.frobenius_norm() < 0.05 * np.sqrt((X ** 2).sum()), 'not fitted'
    _check(G, X, '%s high counts, planted' % name)
    for _ in range(3):
        G.step()
    _check(G, X, '%s high counts, 3 sweeps on' % name)


# ---- 4. the metrics leave the sweep alone ---------------------------------------------------------------------------------

# What the metric call may overwrite: the scratch of the row pass (its outputs R, s_cs, s_rs and the slow-path flags), which
# every sweep rewrites before it reads it, and the sparse models' V_hat * S_hat (_Veff), which every reader forms anew
# (_effective_V, the SparseZIGaP sweep).  Everything else a model or its workspace holds must come out bit for bit.
METRIC_SCRATCH = ('ws.R', 'ws.s_cs', 'ws.s_rs', 'ws.tile_flag', '_Veff')


def _held_tensors(G):
    """Host copies of every tensor the model and its workspace hold (lazy parameters only when materialised)."""
    from oriana_amd.parameters import Parameter
    G._U_hat                                            # (pCMF: resolve the lazy U_hat first -- that is no write of the metrics)
    out = {}
    for owner, prefix in ((G, ''), (G._ws, 'ws.')):
        for k, v in vars(owner).items():
            if isinstance(v, Parameter) and getattr(v, 'materialised', True):
                v = v.tensor
            if isinstance(v, torch.Tensor) and prefix + k not in METRIC_SCRATCH:
                out[prefix + k] = v.detach().cpu().numpy().tobytes()
    return out


def _metrics_leave_state_alone(G):
    before = _held_tensors(G)
    G.reconstruction_deviance()
    G.frobenius_norm()
    after = _held_tensors(G)
    changed = [k for k in before if after.get(k) != before[k]]
    assert not changed, 'the metric call wrote %s' % changed


def _twin_bound(n, sweeps):
    """err_colrel between two runs of the same sweeps that differ only in the order in which float atomics combine partial
    sums (none of the paths is bitwise reproducible: the Gamma updates' float64 column sums and the dense block's per-gene
    sums are atomics across work-groups).  A float32 sum of p non-negative partials moves by at most (p - 1) 2^-24 relative
    when reordered, p <= ceil(n / 32) (the finest cell tiling, 32-cell dense tiles); each further sweep is allowed to double
    what it receives.  (A workspace the metrics clobbered gives errors of order 1.)"""
    return 2.0 ** sweeps * ((n + 31) // 32) * 2.0 ** -24


def _twin_states(name, K, dd, metrics, graph=False):
    X = _counts(K + 1)
    G = _model(name, X, K, dense_density=dd, seed=K + 1)
    if graph:
        G.capture_graph()
    for it in range(3):
        G.step()
        if metrics and it < 2:
            _metrics_leave_state_alone(G)
    torch.cuda.synchronize()
    return G.state(), G.n


def _twins_agree(run, sweeps=3):
    (b1, n), (b2, _) = run(False), run(False)
    a, _ = run(True)
    tol = _twin_bound(n, sweeps)
    for k in b1:
        e0 = err_colrel(b2[k], b1[k]) if b1[k].size else 0.0
        assert e0 <= tol, '%s: two metric-free runs are %.3e apart, beyond the atomic-order bound %.3e' % (k, e0, tol)
        e = err_colrel(a[k], b1[k]) if b1[k].size else 0.0
        assert e <= tol, '%s: the run with metric calls is %.3e from the one without (bound %.3e)' % (k, e, tol)


@pytest.mark.parametrize('name,quirks,K,dd', [p for p in _cases() if p.values[2] in (20, 64, 100)])
def test_metrics_do_not_disturb_the_sweep(name, quirks, K, dd):
    """step; metrics; step; metrics; step against step; step; step.  The metric call reuses the sweep's workspace (R, s_cs,
    s_rs, tile_flag): it must leave every other tensor of the model and the workspace bit for bit as it was, and the sweeps
    after it must agree with the metric-free ones within the atomic-order bound."""
    _twins_agree(lambda metrics: _twin_states(name, K, dd, metrics))


def test_metrics_do_not_disturb_a_replayed_graph():
    _twins_agree(lambda metrics: _twin_states('GaP', 64, None, metrics, graph=True))


# ---- 5. load_state after a sweep (the lazy U_hat of pCMF) -----------------------------------------------------------------

@pytest.mark.parametrize('keys', [('a1',), ('a2',), ('a1', 'a2'), ('U_hat',)], ids='+'.join)
def test_load_state_after_a_sweep_lazy_vs_stored(keys, monkeypatch):
    """After step(), a partial state: the keys not loaded keep their values, and state(), the metrics and the next
    step() agree between the lazy cell side (a2, U_hat evaluated on access) and the stored one (ORIANA_LAZY_U=0)."""
    import oriana_amd.models as Mo
    rng = np.random.default_rng(11)
    n, m, K = 8200, 200, 128                           # n K >= 2^20: the lazy form engages
    X = (rng.poisson(3.0, size=(n, m)) * (rng.random((n, m)) < 0.1)).astype(np.float64)
    a1 = rng.gamma(1.0, size=(n, K)); b1 = rng.gamma(1.0, size=(m, K))
    models = {}
    for lazy in ('0', '1'):
        monkeypatch.setenv('ORIANA_LAZY_U', lazy)
        models[lazy] = Mo.GaP(X, k=K, init=(a1, b1))
    A, B = models['0'], models['1']
    A.step(); B.step()
    assert B._u_stale, 'the lazy form did not engage'
    new = {'a1': A.a1[:] * 1.5, 'a2': A.a2[:] * 2.0, 'U_hat': A.U_hat * 0.7}
    part = {k: new[k] for k in keys}
    # each model's own values before the load; the lazy one's as it would evaluate them (reading them would resolve U_hat)
    before = {'stored': A.state(),
              'lazy': {'a1': B.a1[:], 'a2': B._a2_row.expand(n, K).cpu().numpy(),
                       'U_hat': torch.div(B.a1.tensor, B._a2_row).cpu().numpy()}}
    assert B._u_stale
    for what, G in (('stored', A), ('lazy', B)):
        G.load_state(part)
        st = G.state()
        for k in ('a1', 'a2', 'U_hat'):
            if k in keys:
                assert np.array_equal(st[k], part[k]), '%s %s was not loaded' % (what, k)
            else:
                assert np.array_equal(st[k], before[what][k]), '%s: %s changed by loading %s' % (what, k, '+'.join(keys))
    sa, sb = A.state(), B.state()
    for k in sa:
        assert err_colrel(sb[k], sa[k]) <= _twin_bound(n, 1), 'after load: %s' % k
    _check(A, X, 'stored, after loading %s' % '+'.join(keys))
    _check(B, X, 'lazy, after loading %s' % '+'.join(keys))
    A.step(); B.step()
    sa, sb = A.state(), B.state()
    for k in sa:
        assert err_colrel(sb[k], sa[k]) <= _twin_bound(n, 2), 'next sweep: %s' % k
