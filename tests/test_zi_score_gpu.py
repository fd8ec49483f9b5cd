# -*- coding: utf-8 -*-
"""ZIGaP.fold_in_score_samples() / fold_in_score(), heldout.zi_cell_bounds and the C entry oriana_zi_cell_bound on the GPU against
the float64 reference of tests/zi_score_reference.py.

Shapes are those of tests/test_zi_foldin_gpu.py: 805 x 301 -- a partial last cell tile, m % 4 != 0 (so inert genes exist), an
all-zero cell, an all-zero gene, a gene expressed everywhere; K = 20, 50, 100, 128 are NT = 1, 2, 4, 4 of k_dropout_sweep with 20,
50 (odd pairs: K / 2 = 25 steps), 100 and the full 128 factors -- NT = 3 and the factor loop's other forms (fewer than four steps, a
body that runs zero times, three steps left over) are run by tests/test_zi_heldout_forms_gpu.py.  The bound on the entry is
zi_score_reference.dropout_bound, derived from the kernel's operation sequence; data, lgamma and kl keep score_reference's bounds."""
import numpy as np
import pytest
import torch

import zi_foldin_reference as zr
import zi_score_reference as zs
from test_elbo_gpu import M_COLS, N_ROWS, _counts, _model
from test_zi_foldin_gpu import (KS, MP, PI_ONE, PI_ZERO, PLANTED_ZERO_CELL, ZERO_CELL, _f64, _fitted, _gene_side, _masks, _padded,
                                planted, rate_case)          # noqa: F401  (planted, rate_case: fixtures)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TERMS = ('score', 'data', 'lgamma', 'dropout', 'kl', 'a1', 'a2', 'froze_at', 'log_U_hat')


# ---- 1. the entry against float64 ---------------------------------------------------------------------------------------------

def _splits(n, K, mp=MP):
    """The number of gene ranges the entry cuts (n, mp) into on this device, from the documented size of its scratch."""
    from oriana_amd import _lib
    sd = int(_lib.load().oriana_zi_cell_bound_scratch_doubles(n, mp, K))
    rest = sd - 32 * ((mp + 63) // 64)
    assert rest > 0 and rest % n == 0
    return sd, rest // n


def _entry(X, U, V, pi_d, fill=float('nan'), mp=MP, m_real=M_COLS):
    """oriana_zi_cell_bound over scratch and out filled with `fill`; mp: the gene count the entry is given, m_real of them real."""
    from oriana_amd._lib import call, ptr, stream_ptr
    n, K = U.shape
    _, mask, _ = _masks(X, mp=mp)
    Vp, pip = _padded(V, pi_d, mp)
    sd, _ = _splits(n, K, mp)
    scratch = torch.full((sd,), fill, dtype=torch.float64, device=DEV)
    out = torch.full((n,), fill, dtype=torch.float64, device=DEV)
    call('oriana_zi_cell_bound', ptr(out), ptr(_f64(U)), ptr(Vp), ptr(pip), ptr(mask), ptr(scratch), n, mp, m_real, K, stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('nq', [N_ROWS, 1, 255])
@pytest.mark.parametrize('K', KS)
def test_entry_against_float64(rate_case, K, nq):
    X, U, V, pi_d, _ = rate_case(K)
    if nq < N_ROWS:
        X, U = np.ascontiguousarray(X[12:12 + nq]), np.ascontiguousarray(U[12:12 + nq])
        assert _splits(nq, K)[1] > 1, 'one gene range: the ordered combine is not exercised'
    assert pi_d[PI_ZERO] == 0 and pi_d[PI_ONE] == 1 and (nq < N_ROWS or (X[:, PI_ZERO] != 0).any())
    ref, Lam, lg, g = zs.dropout_sums(X, V, pi_d, U)
    bound = zs.dropout_bound(K, Lam, lg, g)
    got = _entry(X, U, V, pi_d)
    d = np.abs(got - ref)
    i = int(np.argmax(d / bound))
    print('K=%d n\'=%d (%d gene ranges): worst cell %d HIP %.17g ref %.17g diff %.3e bound %.3e; max error / bound %.3f' % (
        K, nq, _splits(nq, K)[1], i, got[i], ref[i], d[i], bound[i], np.max(d / bound)))
    assert np.isfinite(got).all(), 'NaN sentinel left in out, or a non-finite value'
    assert np.all(d <= bound)
    # a second run, over scratch and out filled with another sentinel: bit-identical
    assert np.array_equal(_entry(X, U, V, pi_d, fill=float('inf')), got)


def test_entry_k_range():
    from oriana_amd import _lib
    from oriana_amd._lib import ptr, stream_ptr
    t = torch.zeros(64, dtype=torch.float64, device=DEV)
    rc = _lib.load().oriana_zi_cell_bound(ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), 4, 4, 4, 129, stream_ptr())
    assert rc == -2                                                 # ORIANA_EKRANGE


# ---- 2. the terms of the public call against float64 --------------------------------------------------------------------------

def _reference(G, Xq, out):
    """The float64 terms at the pair and the float32 E[log U] the call returned; the gene side from the model's state."""
    lv, V, pi_d, al1, al2 = _gene_side(G)
    return zs.cell_terms(Xq, out['log_U_hat'], lv, out['a1'], out['a2'], V, pi_d, al1, al2)


def _check_cells(out, ref, K, what):
    tol = zs.cell_bounds(ref, K)
    n = ref['score'].shape[0]
    for k in zs.CELL_TERMS + ('score',):
        assert out[k].dtype == np.float64 and out[k].shape == (n,)
        d = np.abs(out[k] - ref[k])
        i = int(np.argmax(d - tol[k]))
        print('%s %s: worst cell %d HIP %.17g ref %.17g diff %.3e bound %.3e; max diff / bound %.3f' % (
            what, k, i, out[k][i], ref[k][i], d[i], tol[k][i], np.max(d / np.maximum(tol[k], 1e-300))))
    for k in zs.CELL_TERMS + ('score',):
        d = np.abs(out[k] - ref[k])
        bad = np.nonzero(~(np.isfinite(out[k]) & (d <= tol[k])))[0]
        assert bad.size == 0, '%s %s: cells %r: HIP %r ref %r bound %r' % (what, k, bad.tolist(), out[k][bad], ref[k][bad],
                                                                         tol[k][bad])
    assert np.array_equal(out['score'], out['data'] - out['lgamma'] + out['dropout'] - out['kl'])
    return tol


@pytest.mark.parametrize('K', KS)
def test_terms_against_float64(K):
    G = _fitted(K)
    Xq = _counts(K + 50)
    out = G.fold_in_score_samples(Xq, n_iter=10, return_terms=True)
    assert set(out) == set(TERMS)
    assert out['log_U_hat'].dtype == np.float32 and out['log_U_hat'].shape == out['a1'].shape == out['a2'].shape == (N_ROWS, K)
    assert G.fold_in_unconverged_ == int((out['froze_at'] == 10).sum())
    _check_cells(out, _reference(G, Xq, out), K, 'K=%d' % K)
    z = ZERO_CELL
    assert not Xq[z].any() and out['data'][z] == 0 and out['lgamma'][z] == 0 and np.isfinite(out['score'][z])
    # log_U_hat is the unshifted float32 E[log U] of the returned pair (the Gamma node's kernel: casts of a1 and a2, psi, log)
    from scipy.special import psi
    lu = zr.elog_u(out['a1'], out['a2']).astype(np.float64)
    room = 2.0 ** -24 * (2 * np.abs(psi(out['a1'])) + 3 + 3 * np.abs(np.log(out['a2'])) + 2 * np.abs(lu))
    assert np.all(np.abs(out['log_U_hat'] - lu) <= room)
    # the plain call and the mean
    s = G.fold_in_score_samples(Xq, n_iter=10)
    assert np.array_equal(s, out['score'])
    v = G.fold_in_score(Xq, n_iter=10)
    assert isinstance(v, float) and v == float(s.mean()) and G.fold_in_score(Xq, n_iter=10, return_terms=True) == v


@pytest.mark.parametrize('nq', [1, 255])
def test_short_batches(nq):
    K = 20
    G = _fitted(K)
    Xq = _counts(9)[12:12 + nq]
    out = G.fold_in_score_samples(Xq, n_iter=3, return_terms=True)
    _check_cells(out, _reference(G, Xq, out), K, 'n\' = %d' % nq)
    assert G.fold_in_score(Xq, n_iter=3) == float(out['score'].mean())


def test_a_gene_the_fit_never_saw_expressed_stays_finite():
    """The all-zero gene of _counts: its pi_d is 0 or the 1e-10 the column override leaves, pi~ = 1e-10 either way; a held-out
    cell that expresses it pays log(1e-10) - Lambda there, not -inf.  (pi_d = 0 exactly, expressed: the entry test's PI_ZERO.)"""
    K = 20
    G = _fitted(K)
    zero_gene = 5
    assert not _counts(K)[:, zero_gene].any() and G.state()['pi_d'][zero_gene] <= 1.1e-10
    Xq = _counts(K + 50)
    Xq[3, zero_gene] = 4.0
    out = G.fold_in_score_samples(Xq, n_iter=4, return_terms=True)
    assert np.isfinite(out['score']).all()
    _check_cells(out, _reference(G, Xq, out), K, 'unseen gene expressed')


# ---- 3. the call leaves everything else alone ---------------------------------------------------------------------------------

def test_two_calls_agree_and_fold_in_is_unchanged(planted):
    G, Xq = planted
    E0, a1_0, a2_0, fr_0 = G.fold_in(Xq, return_params=True)
    a, b = G.fold_in_score_samples(Xq, return_terms=True), G.fold_in_score_samples(Xq, return_terms=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    E1, a1_1, a2_1, fr_1 = G.fold_in(Xq, return_params=True)
    for x, y in ((E0, E1), (a1_0, a1_1), (a2_0, a2_1), (fr_0, fr_1)):
        assert np.array_equal(x, y)
    # the fold-in of the scoring call is fold_in()'s
    assert np.array_equal(a['a1'], a1_0) and np.array_equal(a['a2'], a2_0) and np.array_equal(a['froze_at'], fr_0)


def test_scoring_does_not_disturb_the_sweep(monkeypatch):
    """tests/test_zi_foldin_gpu._three_sweeps with every fold_in() call replaced by a scoring call: around each call everything
    the model and its workspace hold is bit-identical (_held_tensors and the flags, inside the helper), and the three sweeps are
    those of a twin that never scored.  Two runs of the same sweeps are not bit-reproducible in this code base (the float64 atomics
    of the dense ZI products): the twins are compared as every twin test here compares them, within the atomic-order bound."""
    import oriana_amd.models as M
    import test_zi_foldin_gpu as tz
    from helpers import err_colrel
    from test_elbo_gpu import _twin_bound
    K = 50
    b, n, kb = tz._three_sweeps(K, False)
    calls = []

    def scoring(self, X, **kw):
        calls.append(kw)
        return self.fold_in_score_samples(X, **kw)
    monkeypatch.setattr(M.ZIGaP, 'fold_in', scoring)
    a, _, ka = tz._three_sweeps(K, True)
    assert len(calls) == 4 and ka == kb >= 1
    tol = _twin_bound(n, 3)
    for k in b:
        e = err_colrel(a[k], b[k]) if b[k].size else 0.0
        assert e <= tol, '%s: the run with scoring calls is %.3e from the one without (bound %.3e)' % (k, e, tol)


# ---- 4. monotone along the fold-in --------------------------------------------------------------------------------------------

def test_score_does_not_decrease_along_the_fold_in(planted):
    G, Xq = planted
    K = G.k
    prev = None
    for n_iter in (0, 1, 2, 5, 20):
        out = G.fold_in_score_samples(Xq, n_iter=n_iter, tol=0, return_terms=True)
        ref = _reference(G, Xq, out)
        if prev is not None:
            d = out['score'] - prev[0]['score']
            allow = zs.cell_bounds(prev[1], K)['score'] + zs.cell_bounds(ref, K)['score']
            print('n_iter %d: smallest increment %.3e, largest drop / allowance %.3f, mean score %.6f' % (
                n_iter, d.min(), (-d / allow).max(), out['score'].mean()))
            bad = np.nonzero(d < -allow)[0]
            assert bad.size == 0, 'n_iter %d: cells %r dropped by %r (allowed %r)' % (n_iter, bad.tolist(), d[bad], allow[bad])
            assert out['score'].mean() > prev[0]['score'].mean()
        else:
            print('n_iter 0: mean score %.6f' % out['score'].mean())
        assert np.isfinite(out['score'][PLANTED_ZERO_CELL]) and not Xq[PLANTED_ZERO_CELL].any()
        prev = (out, ref)


# ---- 5. errors and edges ------------------------------------------------------------------------------------------------------

def test_no_cells():
    G = _fitted(20, sweeps=1)
    Xq = np.zeros((0, M_COLS))
    out = G.fold_in_score_samples(Xq, return_terms=True)
    for k in zs.CELL_TERMS + ('score', 'froze_at'):
        assert out[k].shape == (0,), k
    assert out['a1'].shape == out['a2'].shape == out['log_U_hat'].shape == (0, 20) and out['score'].dtype == np.float64
    assert G.fold_in_score_samples(Xq).shape == (0,) and np.isnan(G.fold_in_score(Xq)) and G.fold_in_unconverged_ == 0


def test_errors():
    G = _fitted(20, sweeps=0)
    with pytest.raises(ValueError, match='genes'):
        G.fold_in_score_samples(np.zeros((4, M_COLS + 1)))
    with pytest.raises(ValueError, match='init'):
        G.fold_in_score(_counts(1)[:40], init=np.ones((41, 20)))
    wide = _model(_counts(2)[:300], 129, name='ZIGaP', seed=2)
    with pytest.raises(ValueError, match='128'):
        wide.fold_in_score_samples(_counts(3)[:10])
    with pytest.raises(NotImplementedError, match='pCMF') as exc:
        G.score_samples(_counts(3)[:10])
    assert 'fold_in_score_samples' in str(exc.value) and 'fold_in_score_samples' in G._no_score
    with pytest.raises(NotImplementedError, match='pCMF'):
        G.score(_counts(3)[:10])
    S = _model(_counts(2)[:300], 5, name='SparseZIGaP', seed=2)
    assert not hasattr(S, 'fold_in_score_samples') and not hasattr(S, 'fold_in_score')
    assert 'fold_in_score' not in S._no_score
