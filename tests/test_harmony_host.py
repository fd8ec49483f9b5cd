# -*- coding: utf-8 -*-
"""Harmony batch correction without a GPU: the closed-form ridge weights against harmonypy's linear system, what the float64
restatement (tests/harmony_reference.py) does to seeded blobs, the objective's third term, the decision margins of the
stopping-rule case, and every argument error of the library entries and of the Python calls before a launch."""
import ctypes
import types

import numpy as np
import pytest
import torch

import harmony_reference as hr

EINVAL, EKRANGE = -1, -2


# ---- the closed form ---------------------------------------------------------------------------------------------------------------
def _ridge_case(seed, n, d, K, B, absent=None):
    rng = np.random.RandomState(seed)
    Z = rng.normal(size=(n, d)) * 3.0
    batch = np.arange(n) % B
    rng.shuffle(batch)
    R = rng.dirichlet(np.ones(K), size=n)
    if absent is not None:
        R[batch == absent[1], absent[0]] = 0.0
    return Z, batch, R


@pytest.mark.parametrize('B,lam,absent', [(3, [1.0, 1.0, 1.0], None), (4, [0.5, 1.0, 2.0, 4.0], None), (3, [1.0, 2.0, 0.25], (1, 2)),
                                          (1, [1.0], None)])
def test_closed_form_is_harmonypys_linear_system(B, lam, absent):
    Z, batch, R = _ridge_case(5 + B, 200, 6, 4, B, absent)
    lam = np.asarray(lam)
    S, O, _ = hr.moments(Z, R, batch, B)
    W, w0 = hr.ridge_weights(S, O, lam)
    scale = np.abs(Z).max()
    for k in range(R.shape[1]):
        ref = hr.ridge_solve(Z, R[:, k], batch, lam)
        assert np.abs(W[k] - ref[1:]).max() <= 1e-13 * scale, (k, np.abs(W[k] - ref[1:]).max())
        assert np.abs(w0[k] - ref[0]).max() <= 1e-13 * scale
    if absent is not None:
        assert O[absent[0], absent[1]] == 0.0 and np.all(W[absent[0], absent[1]] == 0.0)       # (S = 0, O = 0: nothing to remove)
    if B == 1:
        # one batch: the intercept takes the weighted mean up to the ridge's shrinkage, W removes nothing that is batch-specific
        Zc, _ = hr.correct(Z, R, batch, W)
        mean = S[:, 0] / O[:, 0, None]
        assert np.abs(w0 - mean).max() <= 1e-13 * scale and np.abs(W).max() <= 1e-13 * scale and np.abs(Zc - Z).max() <= 1e-12 * scale


def test_closed_form_torch_twin():
    from oriana_amd import cluster
    Z, batch, R = _ridge_case(3, 150, 5, 3, 3, (0, 1))
    R[:, 2] = 0.0                                                  # an empty cluster: the denominator of w0 is 0, W = 0
    S, O, _ = hr.moments(Z, R, batch, 3)
    lam = np.array([1.0, 0.5, 2.0])
    W = cluster.harmony_ridge_weights(torch.as_tensor(S), torch.as_tensor(O), torch.as_tensor(lam)).numpy()
    ref = hr.ridge_weights(S, O, lam)[0]
    assert np.isfinite(W).all() and np.all(W[2] == 0.0)
    assert np.abs(W - ref).max() <= 1e-14 * np.abs(ref).max()


# ---- what the restatement does ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def blob_run():
    Z, cell, batch = hr.blobs()
    return Z, cell, batch, hr.harmony(Z, batch, n_clusters=12, centers=hr.kmeans_start(Z, 12))


def test_blobs_are_mixed_and_types_kept(blob_run):
    Z, cell, batch, out = blob_run
    Pr = np.bincount(batch) / float(len(batch))
    before = hr.knn_shares(Z, batch)
    after, purity = hr.knn_shares(out['corrected'], batch), hr.knn_shares(out['corrected'], cell)
    print('same-batch share %.4f -> %.4f (sum Pr^2 = %.4f), type purity %.4f, rounds %s' % (before, after, (Pr ** 2).sum(), purity, out['rounds']))
    assert before >= 0.99
    assert abs(after - (Pr ** 2).sum()) <= 0.05
    assert purity >= 0.99
    assert out['n_iter'] == len(out['rounds']) == len(out['objective']) - 1 and sum(out['rounds']) == len(out['objective_rounds'])
    assert np.allclose(out['responsibilities'].sum(1), 1.0, atol=1e-12)


def test_a_type_missing_from_a_batch_is_not_smeared():
    Z, cell, batch = hr.blobs(drop=(0, 0))
    assert not ((cell == 0) & (batch == 0)).any() and len(Z) < 1200
    out = hr.harmony(Z, batch, n_clusters=12, centers=hr.kmeans_start(Z, 12))
    purity = hr.knn_shares(out['corrected'], cell)
    print('type purity %.4f' % purity)
    assert purity >= 0.99


def test_third_term_from_O_and_E_is_the_per_cell_form():
    rng = np.random.RandomState(0)
    n, K, B = 500, 7, 3
    batch = rng.randint(0, B, size=n)
    R = rng.dirichlet(np.ones(K) * 0.3, size=n)
    O = hr.batch_sums(R, batch, B)
    E = O.sum(1)[:, None] * (np.bincount(batch, minlength=B) / float(n))[None, :]
    theta = np.array([2.0, 0.5, 1.0])
    a, b = hr.diversity_term(O, E, theta, 0.1), hr.diversity_term_per_cell(R, batch, O, E, theta, 0.1)
    assert abs(a - b) <= 1e-12 * max(1.0, abs(a))


def test_stopping_case_margins():
    """Every decision of the stopping-rule case is further from its threshold than 100 times what the kernels' derived error can
    move its ratio by: the GPU test may compare rounds, n_iter and converged with the restatement."""
    c = hr.STOP
    Z, _, batch = hr.blobs(seed=c['blob_seed'])
    out = hr.harmony(Z, batch, n_clusters=c['K'], centers=hr.start_centers(Z, c['K']), max_iter=c['max_iter'], max_rounds=c['max_rounds'],
                     eps_cluster=c['eps_cluster'], eps_harmony=c['eps_harmony'], seed=c['seed'], with_bounds=True)
    assert len(out['checks']) == len(out['rounds']) + out['n_iter'] and out['converged'] and out['n_iter'] > 1
    worst = min(abs(r - eps) / err for r, eps, err in out['checks'])
    print('rounds %s, n_iter %d, least margin / error %.1f' % (out['rounds'], out['n_iter'], worst))
    assert worst > 100.0


def test_end_to_end_tolerance_record():
    """The recorded distance of the float32-state run from the float64 run (the end-to-end tolerance of the GPU test is
    E2E_FACTOR times the value measured at run time) is what this machine measures, within a factor of two."""
    Z, _, batch = hr.blobs()
    got = hr.e2e_distances(Z, batch)[2]
    print(got)
    for key, rec in hr.E2E_MEASURED.items():
        assert rec / 2.0 <= got[key] <= rec * 2.0, (key, got[key], rec)


def test_restatement_is_independent_of_the_callers_order():
    Z, _, batch = hr.blobs(n=240)
    c0 = hr.start_centers(Z, 5)
    a = hr.harmony(Z, batch, n_clusters=5, centers=c0, max_iter=2, max_rounds=5, eps_cluster=None, eps_harmony=None)
    assert a['rounds'] == [5, 5] and a['corrected'].shape == Z.shape and a['batch_sizes'].sum() == 240
    assert hr.block_cuts(7, 20) == list(range(8)) and hr.block_cuts(1200, 20)[1] == 60 and hr.default_clusters(1200) == 40
    assert hr.default_clusters(10) == 1 and hr.default_clusters(10 ** 6) == 100 and hr.default_clusters(45) == 2


# ---- argument errors through the library, no GPU -----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from oriana_amd import _lib
    return _lib.load()


def test_queries(lib):
    assert lib.oriana_harmony_max_clusters(100) >= 100 and lib.oriana_harmony_max_batches() >= 8
    assert lib.oriana_harmony_max_clusters(0) == 0 and lib.oriana_harmony_max_clusters(257) == 0
    assert 1 <= lib.oriana_harmony_max_clusters(256) <= lib.oriana_harmony_max_clusters(4)
    assert 1 <= lib.oriana_harmony_partial_rows() <= 64
    for name in ('assign', 'moments', 'correct'):
        f = getattr(lib, 'oriana_harmony_%s_scratch_bytes' % name)
        assert f(1000, 100, 100, 8, 0) >= 0 and f(1000, 100, 100, 8, 0) % 16 == 0 and f(0, 3, 2, 1, 3) >= 0
        assert f(-1, 3, 2, 1, 0) == EINVAL and f(5, 0, 2, 1, 0) == EINVAL and f(5, 3, 0, 1, 0) == EINVAL and f(5, 3, 2, 0, 0) == EINVAL
        assert f(5, 3, 2, 1, -1) == EINVAL
        assert f(5, 257, 2, 1, 0) == EKRANGE and f(5, 3, lib.oriana_harmony_max_clusters(3) + 1, 1, 0) == EKRANGE
        assert f(5, 3, 2, lib.oriana_harmony_max_batches() + 1, 0) == EKRANGE


def test_entry_argument_errors_without_gpu(lib):
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16                  # a host address: no entry gets as far as using it
    A, M, C = lib.oriana_harmony_assign, lib.oriana_harmony_moments, lib.oriana_harmony_correct
    kmax, bmax = lib.oriana_harmony_max_clusters(3), lib.oriana_harmony_max_batches()
    # assign(Z, n, d, ldz, batch, centers, K, P, B, inv_sigma, R, O_blk, sums, scratch, blocks, stream)
    ok = [p, 5, 3, 3, p, p, 2, p, 1, 10.0, p, p, p, p, 0, None]
    for at, val, code in ((1, -1, EINVAL), (2, 0, EINVAL), (3, 2, EINVAL), (6, 0, EINVAL), (8, 0, EINVAL), (14, -1, EINVAL),
                          (9, 0.0, EINVAL), (9, float('inf'), EINVAL), (9, float('nan'), EINVAL), (0, None, EINVAL), (4, None, EINVAL),
                          (5, None, EINVAL), (7, None, EINVAL), (10, None, EINVAL), (11, None, EINVAL), (12, None, EINVAL),
                          (13, None, EINVAL), (13, p + 4, EINVAL), (2, 257, EKRANGE), (6, kmax + 1, EKRANGE), (8, bmax + 1, EKRANGE)):
        a = list(ok)
        a[at] = val
        if at == 2 and val == 257:
            a[3] = 257
        assert A(*a) == code, ('assign', at, val)
    # moments(X, n, d, ldx, R, K, batch, B, S, O, scratch, blocks, stream)
    ok = [p, 5, 3, 3, p, 2, p, 1, p, p, p, 0, None]
    for at, val, code in ((1, -1, EINVAL), (2, 0, EINVAL), (3, 2, EINVAL), (5, 0, EINVAL), (7, 0, EINVAL), (11, -1, EINVAL),
                          (0, None, EINVAL), (4, None, EINVAL), (6, None, EINVAL), (8, None, EINVAL), (9, None, EINVAL),
                          (10, None, EINVAL), (10, p + 8, EINVAL), (5, kmax + 1, EKRANGE), (7, bmax + 1, EKRANGE)):
        a = list(ok)
        a[at] = val
        assert M(*a) == code, ('moments', at, val)
    # correct(Z, n, d, ldz, R, K, batch, W, B, Zcorr, Zcos, scratch, blocks, stream)
    ok = [p, 5, 3, 3, p, 2, p, p, 1, p, p, p, 0, None]
    for at, val, code in ((1, -1, EINVAL), (2, 0, EINVAL), (3, 2, EINVAL), (5, 0, EINVAL), (8, 0, EINVAL), (12, -1, EINVAL),
                          (0, None, EINVAL), (4, None, EINVAL), (6, None, EINVAL), (7, None, EINVAL), (9, None, EINVAL),
                          (10, None, EINVAL), (11, None, EINVAL), (11, p + 4, EINVAL), (5, kmax + 1, EKRANGE), (8, bmax + 1, EKRANGE)):
        a = list(ok)
        a[at] = val
        assert C(*a) == code, ('correct', at, val)
    # an empty input is a no-op that needs no data pointers (correct makes no HIP call at all)
    assert C(None, 0, 3, 3, None, 2, None, p, 1, None, None, p, 0, None) == 0


# ---- the Python calls refuse before a launch ------------------------------------------------------------------------------------------
def _no_launch(monkeypatch):
    from oriana_amd import cluster
    calls = []

    def boom(*a, **k):
        calls.append(a[0] if a else None)
        raise AssertionError('launched')
    monkeypatch.setattr(cluster, 'call', boom)
    monkeypatch.setattr(cluster, 'kmeans', boom)
    return cluster, calls


def test_harmony_errors_before_a_launch(monkeypatch):
    cluster, calls = _no_launch(monkeypatch)
    Z, _, batch = hr.blobs(n=90)
    Y = torch.as_tensor(Z)
    c0 = hr.start_centers(Z, 3)
    good = dict(n_clusters=3, centers=c0)
    with pytest.raises(ValueError, match='device tensor'):          # everything else is in order: the last check before the work
        cluster.harmony(Y, batch, **good)
    bad_nan, bad_zero = Y.clone(), Y.clone()
    bad_nan[7, 3] = float('nan')
    bad_zero[11] = 0.0
    gap = batch.copy()
    gap[gap == 1] = 3                                             # batch 1 occurs nowhere
    for args, kw in (((bad_nan, batch), good), ((bad_zero, batch), good), ((Y, gap), good), ((Y, -batch), good),
                     ((Y, batch[:-1]), good), ((Y, batch.astype(np.float64)), good), ((Y.double(), batch), good),
                     ((Y.t().contiguous().t(), batch), good), ((Y[:, 0], batch), good),
                     ((Y, batch), dict(good, n_clusters=0)), ((Y, batch), dict(good, n_clusters=91)), ((Y, batch), dict(good, sigma=0.0)),
                     ((Y, batch), dict(good, theta=-1.0)), ((Y, batch), dict(good, theta=[1.0, 2.0])), ((Y, batch), dict(good, ridge=0.0)),
                     ((Y, batch), dict(good, ridge=[1.0, 0.0, 1.0])), ((Y, batch), dict(good, n_blocks=0)), ((Y, batch), dict(good, max_iter=0)),
                     ((Y, batch), dict(good, max_rounds=0)), ((Y, batch), dict(good, blocks=-1)), ((Y, batch), dict(good, eps_cluster=-1.0)),
                     ((Y, batch), dict(good, eps_harmony=float('nan'))), ((Y, batch), dict(good, centers=c0[:2])),
                     ((Y, batch), dict(good, centers=np.zeros_like(c0))),
                     ((Y, batch), dict(n_clusters=cluster.harmony_max_clusters(8) + 1, centers=None))):
        with pytest.raises(ValueError):
            cluster.harmony(*args, **kw)
    wide = torch.ones(200, 100)
    with pytest.raises(ValueError, match='centers='):              # the k-means start serves fewer clusters than the kernels here
        cluster.harmony(wide, np.arange(200) % 2, n_clusters=100)
    from oriana_amd import dist as odist
    monkeypatch.setattr(odist, 'world_size', lambda pg=None: 2)
    with pytest.raises(NotImplementedError):
        cluster.harmony(Y, batch, pg=object(), **good)
    assert not calls


def test_raw_calls_refuse_before_a_launch(monkeypatch):
    cluster, calls = _no_launch(monkeypatch)
    n, d, K, B = 70, 5, 3, 2
    X, R = torch.zeros(n, d), torch.zeros(n, K)
    batch = torch.zeros(n, dtype=torch.int32)
    cen, P, W = torch.zeros(K, d), torch.ones(K, B), torch.zeros(K, B, d)
    small = torch.zeros(16, dtype=torch.uint8)                    # every call here needs more scratch than this
    with pytest.raises(ValueError, match='scratch'):
        cluster.harmony_assign(X, batch, cen, P, 10.0, R, scratch=small)
    with pytest.raises(ValueError, match='scratch'):
        cluster.harmony_moments(X, R, batch, B, scratch=small)
    with pytest.raises(ValueError, match='scratch'):
        cluster.harmony_correct(X, R, batch, W, scratch=small)
    for f in (lambda: cluster.harmony_assign(X, batch.long(), cen, P, 10.0, R), lambda: cluster.harmony_assign(X, batch, cen[:2], P, 10.0, R),
              lambda: cluster.harmony_assign(X, batch, cen, P, 0.0, R), lambda: cluster.harmony_assign(X, batch, cen, P, 10.0, R, rows=(5, 71)),
              lambda: cluster.harmony_assign(X, batch, cen, P.double(), 10.0, R), lambda: cluster.harmony_assign(X.double(), batch, cen, P, 10.0, R),
              lambda: cluster.harmony_moments(X, R[:-1], batch, B), lambda: cluster.harmony_moments(X, R, batch, 0),
              lambda: cluster.harmony_moments(X, R, batch, B, S=torch.zeros(K, B, d)),
              lambda: cluster.harmony_correct(X, R, batch, W[:, :, :-1]), lambda: cluster.harmony_correct(X, R, batch, W, Zcos=torch.zeros(n, d + 1))):
        with pytest.raises(ValueError):
            f()
    with pytest.raises(_lib_error()):                              # beyond the limits: the size query refuses, nothing is launched
        cluster.harmony_moments(X, R, batch, cluster.harmony_max_batches() + 1)
    assert not calls


def _lib_error():
    from oriana_amd import _lib
    return _lib.OrianaHipError


def test_integrate_cells_errors_before_a_launch(monkeypatch):
    cluster, calls = _no_launch(monkeypatch)
    from oriana_amd import dist as odist
    from oriana_amd.models.base import FactorModel
    me = types.SimpleNamespace(pg=None, k=4)
    me._cell_feature_columns = types.MethodType(FactorModel._cell_feature_columns, me)
    me._cell_features = lambda *a, **k: (_ for _ in ()).throw(AssertionError('the features were touched'))
    batch = np.zeros(10, dtype=np.int64)
    for kw in (dict(features='mean'), dict(factors=[0, 4]), dict(factors=[]), dict(pg=None)):
        with pytest.raises(ValueError):
            FactorModel.integrate_cells(me, batch, **kw)
    monkeypatch.setattr(odist, 'world_size', lambda pg=None: 2)
    with pytest.raises(NotImplementedError):
        FactorModel.integrate_cells(me, batch)
    assert not calls
