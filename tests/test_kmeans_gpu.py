# -*- coding: utf-8 -*-
"""oriana_kmeans_step and cluster.kmeans on the GPU against the float64 restatement of tests/kmeans_reference.py, under the
bounds derived there (none of them measured on the kernel)."""
import numpy as np
import pytest
import torch

import kmeans_reference as kr

pytestmark = pytest.mark.gpu

U = kr.U


@pytest.fixture(scope='module')
def lib():
    from oriana_amd import _lib
    return _lib.load()


def _dev(Y, extra=0):
    """Y on the device, optionally as the leading columns of a wider matrix (row stride d + extra)."""
    n, d = Y.shape
    if not extra:
        return torch.from_numpy(Y).cuda()
    wide = torch.full((n, d + extra), float('nan'), dtype=torch.float32, device='cuda')
    wide[:, :d] = torch.from_numpy(Y).cuda()
    return wide[:, :d]


def _check_restart(Y, cen_r, out, labels, r, T, what):
    """One restart of a step against the reference: labels outside near-ties, counts exactly, sums / inertia / mind within the
    derived bounds, all against float64 sums over the kernel's own labels."""
    n, d = Y.shape
    C = cen_r.shape[0]
    ref_labels, _, near = kr.assign(Y, cen_r)
    print('%s restart %d: near-tie share %.2e' % (what, r, near.mean() if n else 0.0))
    assert near.mean() <= kr.NEAR_TIE_CAP
    labels = labels.astype(np.int64)
    assert labels.min() >= 0 and labels.max() < C
    assert np.array_equal(labels[~near], ref_labels[~near]), what
    d2 = kr.distances(Y, cen_r)
    own = d2[np.arange(n), labels]
    # (a near-tie row may take either label: its own distance is within the gap of the best)
    assert np.all(own <= d2.min(axis=1) * (1.0 + 4.0 * (d + 3) * U))
    sums, asums, counts = kr.cluster_sums(Y, labels, C)
    assert np.array_equal(out['counts'][r], counts), what
    bound = (T - 1) * U * asums + n * 2.0 ** -52 * asums
    err = np.abs(out['sums'][r] - sums)
    print('%s restart %d: sums error / bound %.3f' % (what, r, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound), what
    assert np.all(out['sums'][r][counts == 0] == 0.0)
    inertia = own.sum()
    assert abs(out['inertia'][r] - inertia) <= ((d + 3) * U + n * 2.0 ** -52) * inertia, what
    assert np.all(np.abs(out['mind'][r].astype(np.float64) - own) <= (d + 3) * U * own), what


def _run_step(Yd, cen, blocks=0, label_restart=0):
    from oriana_amd import cluster
    o = cluster.lloyd_step(Yd, torch.from_numpy(cen).cuda(), label_restart=label_restart, want_mind=True, blocks=blocks)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize('case', kr.STEP_CASES, ids=[c[0] for c in kr.STEP_CASES])
def test_single_step(lib, case):
    from oriana_amd import cluster
    name, n, d, C, R, extra, blocks = kr.resolve_case(case, lib)
    Y, cen = kr.case_inputs(case, lib)
    Yd = _dev(Y, extra)
    T = cluster.partial_rows()
    first = None
    for r in range(R):
        out = _run_step(Yd, cen, blocks=blocks, label_restart=r)
        if first is None:
            first = out
        else:                                   # the label restart changes nothing else
            for k in ('sums', 'counts', 'inertia', 'mind'):
                assert np.array_equal(out[k], first[k]), k
        _check_restart(Y, cen[r], out, out['labels'], r, T, name)


def test_identical_centres_and_a_far_centre():
    Y, _, _ = kr.blobs(11, 300, 20, 3)
    cen = kr.step_centers(11, Y, 4, 1)
    cen[0, 2] = cen[0, 1]                       # two bit-identical centres: every row takes the lower index
    cen[0, 3] = 1e6                             # far from all data
    out = _run_step(_dev(Y), cen)
    assert out['counts'][0, 2] == 0 and out['counts'][0, 3] == 0 and out['counts'][0].sum() == 300
    assert not np.isin(out['labels'], (2, 3)).any()
    assert np.all(out['sums'][0, 2:] == 0.0)
    # exact duplicate rows get the same label
    n = Y.shape[0]
    assert out['labels'][n - 1] == out['labels'][0] and out['labels'][n // 2] == out['labels'][1] == out['labels'][5]
    # kmeans keeps the centre of a cluster that stays empty (the twin centre wins rows once its lower twin has moved)
    from oriana_amd import cluster
    res = cluster.kmeans(_dev(Y), 4, init=cen[0], max_iter=20)
    assert res['n_iter'] >= 1 and np.array_equal(res['centers'][3], cen[0, 3].astype(np.float64))
    assert not np.isin(res['labels'], (3,)).any()


@pytest.mark.parametrize('blocks', [2, 0])
def test_determinism_and_batching(lib, blocks):
    d, C = 100, 20
    G = int(lib.oriana_kmeans_group(d, C))
    R = 2 * G + 1
    Y, _, _ = kr.blobs(21, 700, d, 8)
    cen = kr.step_centers(21, Y, C, R)
    Yd = _dev(Y)
    a = _run_step(Yd, cen, blocks=blocks, label_restart=R - 1)
    b = _run_step(Yd, cen, blocks=blocks, label_restart=R - 1)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    if blocks:
        # restart r inside the batch equals the same restart run alone, bit for bit (the same work-groups along the rows)
        for r in (0, G - 1, G, R - 1):
            one = _run_step(Yd, cen[r:r + 1], blocks=blocks, label_restart=0)
            for k in ('sums', 'counts', 'inertia', 'mind'):
                assert np.array_equal(one[k][0], a[k][r]), (k, r)
            if r == R - 1:
                assert np.array_equal(one['labels'], a['labels'])


@pytest.fixture(scope='module')
def full():
    f = kr.FULL_CASE
    Y, which, _ = kr.blobs(f['seed'], f['n'], f['d'], f['C'])
    inits = np.stack([Y[np.random.default_rng(r).choice(f['n'], size=f['C'], replace=False)] for r in range(6)])
    refs = [kr.lloyd(Y, inits[r], 300, 1e-4) for r in range(6)]
    return Y, which, inits, refs


def _compare_run(Y, res, refs, T):
    """Every restart of a run against lloyd() replayed from the same init."""
    from oriana_amd import cluster
    n, d = Y.shape
    Yd = _dev(Y)
    for r, (labels, centers, inertia, n_iter, conv, near, scale) in enumerate(refs):
        got = cluster.lloyd_step(Yd, torch.from_numpy(res['all_centers'][r:r + 1].astype(np.float32)).cuda(), label_restart=0)
        got_labels = got['labels'].cpu().numpy().astype(np.int64)
        print('restart %d: near-tie share over the run %.2e, n_iter %d / %d' % (r, near.mean(), res['n_iters'][r], n_iter))
        assert near.mean() <= kr.NEAR_TIE_CAP
        rel = ((d + 3) * U + n * 2.0 ** -52)
        if np.array_equal(got_labels, labels):
            bound = ((T - 1) * U + n * 2.0 ** -52) * scale + 2.0 ** -52 * np.abs(centers)
            assert np.all(np.abs(res['all_centers'][r] - centers) <= bound)
            assert res['n_iters'][r] == n_iter and bool(res['converged'][r]) == conv
            assert abs(res['inertias'][r] - inertia) <= 2 * rel * inertia
        else:
            # a near-tie row flipped somewhere along the run: only near-tie rows may differ, and the inertia holds its bound
            # up to the near-tie gap of the flipped rows
            assert not np.any((got_labels != labels) & ~near)
            assert abs(res['inertias'][r] - inertia) <= (2 * rel + 4 * (d + 3) * U) * inertia


def test_full_run_explicit_inits(full):
    from oriana_amd import cluster
    Y, _, inits, refs = full
    res = cluster.kmeans(_dev(Y), 5, n_init=6, init=inits, restarts_per_pass=4)
    assert res['best'] == int(np.argmin(res['inertias'])) and res['inertia'] == res['inertias'][res['best']]
    assert res['labels'].dtype == np.int32 and res['labels'].shape == (Y.shape[0],)
    assert np.array_equal(res['centers'], res['all_centers'][res['best']]) and res['n_iter'] == res['n_iters'][res['best']]
    assert np.array_equal(res['init_centers'], inits.astype(np.float64))
    _compare_run(Y, res, refs, cluster.partial_rows())
    # check_every only decides when the host looks
    res1 = cluster.kmeans(_dev(Y), 5, n_init=6, init=inits, check_every=1)
    for k in ('all_centers', 'n_iters', 'converged', 'inertias', 'labels'):
        assert np.array_equal(res[k], res1[k]), k
    print('ARI of the best restart against the blobs: %.4f' % kr.adjusted_rand_index(res['labels'], full[1]))


def test_max_iter_zero_returns_the_inits_assignment(full):
    from oriana_amd import cluster
    Y, _, inits, _ = full
    res = cluster.kmeans(_dev(Y), 5, init=inits[2], max_iter=0)
    labels, _, near = kr.assign(Y, inits[2])
    assert res['n_iter'] == 0 and not res['converged'][0]
    assert np.array_equal(res['centers'], inits[2].astype(np.float64))
    assert np.array_equal(res['labels'][~near], labels[~near])


def test_kmeanspp_and_random_init(full):
    from oriana_amd import cluster
    Y, _, _, _ = full
    Yd = _dev(Y)
    n, C, n_init = Y.shape[0], 5, 6
    res = cluster.kmeans(Yd, C, n_init=n_init, seed=3, max_iter=0, restarts_per_pass=4)
    u = cluster.draws(3, n_init, C).numpy()
    rows = {Y[i].tobytes(): i for i in range(n - 1, -1, -1)}
    for r in range(n_init):
        cen = res['init_centers'][r].astype(np.float32)
        for j in range(C):
            assert cen[j].tobytes() in rows                                   # the centres are rows of Y
        assert np.array_equal(cen[0], Y[min(int(u[r, 0] * n), n - 1)])
        for j in range(1, C):
            mind = cluster.lloyd_step(Yd, torch.from_numpy(cen[None, :j].copy()).cuda(), want_mind=True)['mind'][0].cpu().numpy()
            assert np.array_equal(cen[j], Y[kr.kmeanspp_pick(mind, u[r, j])]), (r, j)
    again = cluster.kmeans(Yd, C, n_init=n_init, seed=3, max_iter=0)
    assert np.array_equal(again['init_centers'], res['init_centers']) and np.array_equal(again['labels'], res['labels'])
    other = cluster.kmeans(Yd, C, n_init=n_init, seed=4, max_iter=0)
    assert not np.array_equal(other['init_centers'][:, 0], res['init_centers'][:, 0])
    # a full k-means++ run replays like an explicit one
    run = cluster.kmeans(Yd, C, n_init=n_init, seed=3, restarts_per_pass=4)
    refs = [kr.lloyd(Y, run['init_centers'][r], 300, 1e-4) for r in range(n_init)]
    _compare_run(Y, run, refs, cluster.partial_rows())
    rnd = cluster.kmeans(Yd, C, n_init=3, init='random', seed=5, max_iter=0)
    for r in range(3):
        idx = cluster.distinct_rows(cluster.draws(5, 3, C)[r].tolist(), n)
        assert len(set(idx)) == C and np.array_equal(rnd['init_centers'][r].astype(np.float32), Y[idx])


def test_errors_before_a_launch(monkeypatch):
    from oriana_amd import cluster
    calls = []
    monkeypatch.setattr(cluster, 'lloyd_step', lambda *a, **k: calls.append(1) or (_ for _ in ()).throw(AssertionError('launched')))
    Y = torch.randn(50, 100, device='cuda')
    bad = Y.clone()
    bad[7, 3] = float('inf')
    for args in ((bad, 3), (Y, 51), (Y, 82)):
        with pytest.raises(ValueError):
            cluster.kmeans(*args)
    bad[7, 3] = float('nan')
    with pytest.raises(ValueError):
        cluster.kmeans(bad, 3)
    assert not calls
