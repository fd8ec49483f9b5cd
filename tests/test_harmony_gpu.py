# -*- coding: utf-8 -*-
"""Harmony batch correction on the device (csrc/harmony.hip, cluster.harmony, FactorModel.integrate_cells) against the float64
restatement and the derived bounds of tests/harmony_reference.py: the three entries at the smallest shapes at which they can go
wrong, their determinism and scratch contract, the whole driver end to end, the stopping rule, and the model method."""
import numpy as np
import pytest
import torch

import helpers
import harmony_reference as hr

pytestmark = pytest.mark.gpu

# (n, d, K, B): one row; a partial tile; one row past a tile with K a whole step; five tiles with two feature blocks, K past a
# lane group and 13 steps; an odd everything
CASES = [(1, 1, 1, 1), (63, 5, 3, 2), (65, 4, 8, 1), (257, 100, 100, 5), (300, 7, 9, 3)]
MORE = CASES + [(1025, 7, 9, 3)]                                   # 17 tiles of ~21 rows per batch: past the float32 promotion at T rows, many times
INV_SIGMA = 10.0
_cache = {}


def _case(n, d, K, B, seed=0):
    key = (n, d, K, B, seed)
    if key not in _cache:
        rng = np.random.RandomState(100 * seed + n + d + K + B)
        Z = (rng.normal(size=(n, d)) * 2.0 + rng.normal(size=(1, d))).astype(np.float32)
        Zcos = hr.normalize_rows(Z).astype(np.float32)
        batch = rng.randint(0, B, size=n).astype(np.int64)
        cen = hr.normalize_rows(rng.normal(size=(K, d))).astype(np.float32)
        P = np.exp(rng.uniform(np.log(0.1), np.log(10.0), size=(K, B))).astype(np.float32)
        R = rng.dirichlet(np.ones(K) * 0.5, size=n).astype(np.float32)
        R[rng.rand(n, K) < 0.1] = 0.0
        W = (rng.normal(size=(K, B, d)) * 0.5).astype(np.float32)
        _cache[key] = dict(Z=Z, Zcos=Zcos, batch=batch, cen=cen, P=P, R=R, W=W)
    return _cache[key]


def _dev(c):
    return {k: torch.as_tensor(v.astype(np.int32) if k == 'batch' else v).cuda() for k, v in c.items()}


def _assign(c, t, rows=None, blocks=0, scratch=None, inv_sigma=INV_SIGMA):
    """One guarded call: R (NaN-filled before), O_blk, sums as NumPy, and the guards' checks."""
    from oriana_amd import cluster
    n, K = c['Zcos'].shape[0], c['cen'].shape[0]
    B = c['P'].shape[1]
    R, ck_r = helpers.guarded_out((n, K), torch.float32, 'nan')
    O, ck_o = helpers.guarded_out((K, B), torch.float64, 'nan')
    s, ck_s = helpers.guarded_out((2,), torch.float64, 'nan')
    cluster.harmony_assign(t['Zcos'], t['batch'], t['cen'], t['P'], inv_sigma, R, rows=rows, blocks=blocks, scratch=scratch, O_blk=O, sums=s)
    torch.cuda.synchronize()
    for ck in (ck_r, ck_o, ck_s):
        ck('harmony_assign')
    return R.cpu().numpy(), O.cpu().numpy(), s.cpu().numpy()


def _check_assign(c, got, rows, inv_sigma=INV_SIGMA, what=''):
    R, O, s = got
    a, b = rows
    Rr, dist, Or, sd, se = hr.assign(c['Zcos'][a:b], c['batch'][a:b], c['cen'], c['P'], inv_sigma)
    bd = hr.assign_bounds(c['Zcos'][a:b], c['batch'][a:b], c['cen'], c['P'], inv_sigma)
    eR, eO = np.abs(R[a:b] - Rr), np.abs(O - Or)
    print('%s R %.3e of its bound, O_blk %.3e, sum R dist %.3e, sum R log R %.3e' % (
        what, (eR / bd['R']).max(), (eO / np.maximum(bd['O_blk'], 1e-300)).max(), abs(s[0] - sd) / bd['rd'], abs(s[1] - se) / max(bd['re'], 1e-300)))
    assert np.isfinite(R[a:b]).all() and np.isfinite(O).all() and np.isfinite(s).all()
    assert (eR <= bd['R']).all(), (what, (eR / bd['R']).max())
    assert (eO <= bd['O_blk']).all(), (what, eO.max())
    assert abs(s[0] - sd) <= bd['rd'] and abs(s[1] - se) <= bd['re'], (what, s, sd, se, bd['rd'], bd['re'])
    assert np.isnan(R[:a]).all() and np.isnan(R[b:]).all(), 'rows of R outside the range were written'


# ---- assign --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_assign(shape):
    c = _case(*shape)
    _check_assign(c, _assign(c, _dev(c)), (0, shape[0]), what=str(shape))


def test_assign_range_inside_tiles_with_an_absent_batch():
    c = dict(_case(300, 7, 9, 3))
    a, b = 70, 200                                                  # starts and ends inside a tile of the matrix and of the range
    batch = c['batch'].copy()
    batch[a:b][batch[a:b] == 2] = 0                                 # batch 2 is absent from the range
    c['batch'] = batch
    got = _assign(c, _dev(c), rows=(a, b))
    _check_assign(c, got, (a, b), what='range')
    assert np.all(got[1][:, 2] == 0.0)


def test_assign_identical_centres_and_underflow():
    c = dict(_case(63, 5, 3, 2))
    cen = c['cen'].copy()
    cen[1] = cen[0]
    P = c['P'].copy()
    P[1] = P[0]
    c['cen'], c['P'] = cen, P
    R, _, _ = got = _assign(c, _dev(c))
    _check_assign(c, got, (0, 63), what='identical')
    assert np.array_equal(R[:, 0].view(np.int32), R[:, 1].view(np.int32))
    # a centre opposite to the rows at sigma = 0.01: (dist - min) / sigma is near 400, e_k underflows to exactly 0
    c = dict(_case(63, 5, 3, 2))
    Zcos = hr.normalize_rows(np.abs(c['Z']) + 0.5).astype(np.float32)
    cen = c['cen'].copy()
    cen[0] = hr.normalize_rows(np.ones((1, 5)))[0]
    cen[2] = -cen[0]
    c['Zcos'], c['cen'] = Zcos, cen
    R, _, s = got = _assign(c, _dev(c), inv_sigma=100.0)
    _check_assign(c, got, (0, 63), inv_sigma=100.0, what='underflow')
    assert np.all(R[:, 2] == 0.0) and np.isfinite(s[1])


# ---- moments and correct ---------------------------------------------------------------------------------------------------------
def _moments(c, t, blocks=0, scratch=None):
    from oriana_amd import cluster
    K, B, d = c['W'].shape
    S, ck_s = helpers.guarded_out((K, B, d), torch.float64, 'nan')
    O, ck_o = helpers.guarded_out((K, B), torch.float64, 'nan')
    cluster.harmony_moments(t['Z'], t['R'], t['batch'], B, blocks=blocks, scratch=scratch, S=S, O=O)
    torch.cuda.synchronize()
    ck_s('harmony_moments S')
    ck_o('harmony_moments O')
    return S.cpu().numpy(), O.cpu().numpy()


def _correct(c, t, blocks=0, scratch=None):
    from oriana_amd import cluster
    n, d = c['Z'].shape
    Zc, ck_a = helpers.guarded_out((n, d), torch.float32, 'nan')
    Zs, ck_b = helpers.guarded_out((n, d), torch.float32, 'nan')
    cluster.harmony_correct(t['Z'], t['R'], t['batch'], t['W'], blocks=blocks, scratch=scratch, Zcorr=Zc, Zcos=Zs)
    torch.cuda.synchronize()
    ck_a('harmony_correct Zcorr')
    ck_b('harmony_correct Zcos')
    return Zc.cpu().numpy(), Zs.cpu().numpy()


@pytest.mark.parametrize('shape', MORE, ids=lambda s: 'x'.join(map(str, s)))
def test_moments(shape):
    from oriana_amd import cluster
    c = _case(*shape)
    n, B = shape[0], shape[3]
    S, O = _moments(c, _dev(c))
    Sr, Or, SA = hr.moments(c['Z'], c['R'], c['batch'], B)
    bS, bO = hr.moments_bounds(SA, Or, n, cluster.harmony_partial_rows())
    assert np.isfinite(S).all() and np.isfinite(O).all(), 'an element was not written'
    eS, eO = np.abs(S - Sr), np.abs(O - Or)
    print('%s S %.3e of its bound, O %.3e' % (shape, (eS / np.maximum(bS, 1e-300)).max(), (eO / np.maximum(bO, 1e-300)).max()))
    assert (eS <= bS).all() and (eO <= bO).all()


@pytest.mark.parametrize('shape', MORE, ids=lambda s: 'x'.join(map(str, s)))
def test_correct(shape):
    c = dict(_case(*shape))
    n = shape[0]
    if n > 3:                                                       # a row whose corrected value is exactly 0: a zero row of Zcos
        Z, R = c['Z'].copy(), c['R'].copy()
        Z[3], R[3] = 0.0, 0.0
        c['Z'], c['R'] = Z, R
    Zc, Zs = _correct(c, _dev(c))
    assert np.isfinite(Zc).all() and np.isfinite(Zs).all(), 'an element was not written'
    Zcr, Zsr = hr.correct(c['Z'], c['R'], c['batch'], c['W'])
    bc, bs = hr.correct_bounds(c['Z'], c['R'], c['batch'], c['W'])
    eC, eS = np.abs(Zc - Zcr), np.abs(Zs - Zsr)
    live = np.isfinite(bs).all(1)
    print('%s Zcorr %.3e of its bound, Zcos %.3e' % (shape, (eC / np.maximum(bc, 1e-300)).max(), (eS[live] / np.maximum(bs[live], 1e-300)).max()))
    assert (eC <= bc).all() and (eS[live] <= bs[live]).all()
    if n > 3:
        assert not live[3] and live.sum() == n - 1 and np.all(Zc[3] == 0.0) and np.all(Zs[3] == 0.0)
    else:
        assert live.all()


# ---- at the limits: the dynamic LDS of the assign and correct kernels is at its largest -------------------------------------------
def test_assign_at_the_cluster_and_batch_limits():
    from oriana_amd import cluster
    K, B = cluster.harmony_max_clusters(4), cluster.harmony_max_batches()
    assert K >= 100 and B == 64
    c = _case(70, 4, K, B)
    _check_assign(c, _assign(c, _dev(c)), (0, 70), what='limits')
    S, O = _moments(c, _dev(c))
    Sr, Or, SA = hr.moments(c['Z'], c['R'], c['batch'], B)
    bS, bO = hr.moments_bounds(SA, Or, 70, cluster.harmony_partial_rows())
    assert (np.abs(S - Sr) <= bS).all() and (np.abs(O - Or) <= bO).all()


def test_correct_at_the_cluster_limit_of_the_widest_rows():
    from oriana_amd import cluster
    K = cluster.harmony_max_clusters(256)
    c = _case(70, 256, K, 3)
    Zc, Zs = _correct(c, _dev(c))
    Zcr, Zsr = hr.correct(c['Z'], c['R'], c['batch'], c['W'])
    bc, bs = hr.correct_bounds(c['Z'], c['R'], c['batch'], c['W'])
    assert (np.abs(Zc - Zcr) <= bc).all() and (np.abs(Zs - Zsr) <= bs).all()
    _check_assign(c, _assign(c, _dev(c)), (0, 70), what='widest')


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def test_determinism():
    c = _case(300, 7, 9, 3)
    t = _dev(c)
    n, K = 300, 9
    base = _assign(c, t)
    again = _assign(c, t)
    for x, y in zip(base, again):
        assert np.array_equal(_bits(x), _bits(y))
    Rr, dist, _, _, _ = hr.assign(c['Zcos'], c['batch'], c['cen'], c['P'], INV_SIGMA)
    tol_rd = 2.0 * n * 2.0 ** -53 * float((np.abs(Rr) * np.abs(dist)).sum())
    tol_re = 2.0 * n * 2.0 ** -53 * float(np.abs(hr.xlogx(Rr)).sum())
    for blocks in (1, 2):
        R, O, s = _assign(c, t, blocks=blocks)
        assert np.array_equal(_bits(R), _bits(base[0]))
        assert (np.abs(O - base[1]) <= 2.0 * n * 2.0 ** -53 * np.abs(base[1])).all()
        assert abs(s[0] - base[2][0]) <= tol_rd and abs(s[1] - base[2][1]) <= tol_re
    lo, hi = _assign(c, t, rows=(0, 137)), _assign(c, t, rows=(137, n))
    assert np.array_equal(_bits(lo[0][:137]), _bits(base[0][:137])) and np.array_equal(_bits(hi[0][137:]), _bits(base[0][137:]))
    assert (np.abs(lo[1] + hi[1] - base[1]) <= 2.0 * n * 2.0 ** -53 * np.abs(base[1])).all()
    # moments: the same bits on repetition, within the order bound across `blocks`; correct: the same bits always
    S0, O0 = _moments(c, t)
    S1, O1 = _moments(c, t)
    assert np.array_equal(_bits(S0), _bits(S1)) and np.array_equal(_bits(O0), _bits(O1))
    _, _, SA = hr.moments(c['Z'], c['R'], c['batch'], 3)
    for blocks in (1, 2):
        S, O = _moments(c, t, blocks=blocks)
        assert (np.abs(S - S0) <= 2.0 * n * 2.0 ** -53 * SA).all() and (np.abs(O - O0) <= 2.0 * n * 2.0 ** -53 * np.abs(O0)).all()
    Z0 = _correct(c, t)
    for blocks in (0, 1, 2):
        Zb = _correct(c, t, blocks=blocks)
        assert np.array_equal(_bits(Z0[0]), _bits(Zb[0])) and np.array_equal(_bits(Z0[1]), _bits(Zb[1]))


# ---- the scratch contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', sorted(helpers.SCRATCH_VARIANTS))
def test_scratch_contract(variant):
    from oriana_amd import _lib
    lib = _lib.load()
    n, d, K, B = 300, 7, 9, 3
    c, other = _case(n, d, K, B), _case(n, d, K, B, seed=1)
    t, to = _dev(c), _dev(other)
    for name, run in (('assign', _assign), ('moments', _moments), ('correct', _correct)):
        nbytes = int(getattr(lib, 'oriana_harmony_%s_scratch_bytes' % name)(n, d, K, B, 0))
        assert nbytes > 0 and nbytes % 16 == 0
        base = run(c, t)
        buf, check = helpers.guarded_variant(nbytes, variant)
        if variant == 'stale':
            run(other, to, scratch=buf)
        got = run(c, t, scratch=buf)
        check('oriana_harmony_%s, %s scratch' % (name, variant))
        for x, y in zip(base, got):
            assert np.array_equal(_bits(x), _bits(y)), (name, variant)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_end_to_end_fixed_rounds():
    """The whole driver against the float64 restatement at the tolerance the restatement itself sets: E2E_FACTOR times the distance
    of its float32-state run from its float64 run.  Measured on an MI355X: 'corrected' 1.04e-06 against 4 x 5.88e-07,
    'responsibilities' 5.27e-07 against 4 x 1.57e-07, 'objective_rounds' 2.59e-05 against 4 x 2.19e-05.  (With a plain fmaf chain
    for the dot products the responsibilities were 7.84e-07 away and missed it: DESIGN.md 5r.)"""
    from oriana_amd import cluster
    Z, _, batch = hr.blobs()
    ref, _, dist = hr.e2e_distances(Z, batch)
    e = hr.E2E
    out = cluster.harmony(torch.as_tensor(Z).cuda(), batch, n_clusters=e['K'], centers=hr.start_centers(Z, e['K']), eps_cluster=None,
                          eps_harmony=None, max_iter=e['max_iter'], max_rounds=e['max_rounds'], seed=e['seed'])
    assert out['rounds'] == [e['max_rounds']] * e['max_iter'] and out['n_iter'] == e['max_iter'] and not out['converged']
    assert np.array_equal(out['batch_sizes'], ref['batch_sizes']) and len(out['objective']) == e['max_iter'] + 1
    got = {'corrected': out['corrected'].cpu().numpy(), 'responsibilities': out['responsibilities'].cpu().numpy(),
           'objective_rounds': np.asarray(out['objective_rounds'])}
    err = {k: float(np.abs(got[k] - np.asarray(ref[k])).max()) for k in got}
    for k in got:
        print('%s: %.3e from the restatement, tolerance %.1f x %.3e' % (k, err[k], hr.E2E_FACTOR, dist[k]))
    for k in got:
        assert err[k] <= hr.E2E_FACTOR * dist[k], (k, err[k], dist[k])
    assert out['objective'][1:] == [out['objective_rounds'][i * e['max_rounds'] + e['max_rounds'] - 1] for i in range(e['max_iter'])]


def test_stopping_rule():
    from oriana_amd import cluster
    c = hr.STOP
    Z, _, batch = hr.blobs(seed=c['blob_seed'])
    kw = dict(n_clusters=c['K'], centers=hr.start_centers(Z, c['K']), max_iter=c['max_iter'], max_rounds=c['max_rounds'],
              eps_cluster=c['eps_cluster'], eps_harmony=c['eps_harmony'], seed=c['seed'])
    ref = hr.harmony(Z, batch, **kw)
    out = cluster.harmony(torch.as_tensor(Z).cuda(), batch, **kw)
    print(out['rounds'], out['n_iter'], out['converged'], ref['rounds'], ref['n_iter'], ref['converged'])
    assert out['rounds'] == ref['rounds'] and out['n_iter'] == ref['n_iter'] and out['converged'] == ref['converged']


def test_default_start():
    """The default start (k-means on the normalised rows) runs and is the same bits on repetition; a sanity check of what it does to
    the blobs (the restatement's figures are asserted on the host, from a NumPy k-means start)."""
    from oriana_amd import cluster
    Z, cell, batch = hr.blobs()
    Y = torch.as_tensor(Z).cuda()
    a = cluster.harmony(Y, batch, n_clusters=12, max_iter=4)
    b = cluster.harmony(Y, torch.as_tensor(batch), n_clusters=12, max_iter=4)
    assert torch.equal(a['corrected'], b['corrected']) and torch.equal(a['responsibilities'], b['responsibilities'])
    assert a['objective_rounds'] == b['objective_rounds']
    corrected = a['corrected'].cpu().numpy()
    share, purity = hr.knn_shares(corrected, batch), hr.knn_shares(corrected, cell)
    print('same-batch share %.4f, type purity %.4f, rounds %s' % (share, purity, a['rounds']))
    assert share <= 0.7 and purity >= 0.9


# ---- the model method --------------------------------------------------------------------------------------------------------------
def _batch_counts(seed=0, n=300, m=40, B=3):
    """Counts with a batch-specific gene scaling: every gene's rate is multiplied by a factor drawn per (batch, gene)."""
    rng = np.random.default_rng(seed)
    batch = rng.permutation(np.arange(n) % B).astype(np.int64)
    kind = rng.integers(0, 2, size=n)
    rate = rng.gamma(2.0, 2.0, size=(2, m))
    scale = np.exp(rng.normal(0.0, 0.7, size=(B, m)))
    return rng.poisson(rate[kind] * scale[batch]).astype(np.float64), batch


def _same_state(a, b):
    return a.keys() == b.keys() and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a)


@pytest.mark.parametrize('name', ['GaP', 'ZIGaP'])
def test_integrate_cells(name):
    from oriana_amd import cluster
    from test_deviance_path_gpu import _model
    X, batch = _batch_counts()
    G = _model(name, X, 4)
    G.fit(5)
    before = G.state()
    out = G.integrate_cells(batch, n_clusters=6, max_iter=2)
    assert isinstance(out['corrected'], np.ndarray) and out['corrected'].shape == (300, 4) and out['features'].shape == (300, 4)
    assert np.array_equal(out['factors'], np.arange(4)) and out['responsibilities'].shape == (300, 6)
    ref = cluster.harmony(torch.as_tensor(out['features']).cuda(), batch, n_clusters=6, max_iter=2)
    assert np.array_equal(_bits(out['corrected']), _bits(ref['corrected'].cpu().numpy()))
    assert out['rounds'] == ref['rounds'] and out['objective'] == ref['objective']
    t = G.integrate_cells(batch, n_clusters=6, max_iter=2, as_tensor=True)
    assert all(isinstance(t[k], torch.Tensor) and t[k].is_cuda for k in ('corrected', 'responsibilities', 'centers', 'features'))
    assert np.array_equal(_bits(t['corrected'].cpu().numpy()), _bits(out['corrected']))
    nb = cluster.knn(t['corrected'], 5)                            # (feeds the neighbour search as it is)
    assert tuple(nb['indices'].shape) == (300, 5)
    sub = G.integrate_cells(batch, n_clusters=6, max_iter=2, factors=[0, 2], features='mean_log')
    assert sub['features'].shape == (300, 2) and np.array_equal(sub['factors'], [0, 2]) and sub['corrected'].shape == (300, 2)
    assert _same_state(before, G.state())
