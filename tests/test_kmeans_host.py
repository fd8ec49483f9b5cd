# -*- coding: utf-8 -*-
"""k-means without a GPU: the float64 restatement against scikit-learn, the near-tie share of every seeded input of the GPU
tests, the k-means++ pick on hand-made weights, and every argument error that needs no device."""
import ctypes

import numpy as np
import pytest
import torch

import kmeans_reference as kr


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from oriana_amd import _lib
    return _lib.load()


def test_restatement_matches_scikit_learn():
    cl = pytest.importorskip('sklearn.cluster')
    Y, _, _ = kr.blobs(5, 600, 6, 4)
    Y = Y.astype(np.float64)
    rng = np.random.default_rng(1)
    init = Y[rng.choice(Y.shape[0], size=4, replace=False)]
    # The restatement rounds the centres to float32 for every assignment and scikit-learn does not; that moves a distance by
    # far less than the near-tie gap, so on an input without a near-tie along the whole run the two must take the same path.
    labels, centers, inertia, n_iter, conv, near, _ = kr.lloyd(Y, init, 300, 1e-4)
    assert not near.any()
    assert np.bincount(labels, minlength=4).min() > 0                       # no cluster empties
    km = cl.KMeans(n_clusters=4, init=init, n_init=1, algorithm='lloyd', max_iter=300, tol=1e-4).fit(Y)
    assert np.array_equal(km.labels_, labels)
    np.testing.assert_allclose(km.cluster_centers_, centers, rtol=1e-12, atol=1e-12 * np.abs(centers).max())
    assert km.n_iter_ == n_iter and conv


def test_near_tie_share_of_every_gpu_input(lib):
    for case in kr.STEP_CASES:
        name, n, d, C, R, extra, blocks = kr.resolve_case(case, lib)
        Y, cen = kr.case_inputs(case, lib)
        assert Y.shape == (n, d) and cen.shape == (R, C, d)
        for r in range(R):
            _, _, near = kr.assign(Y, cen[r])
            assert near.mean() <= kr.NEAR_TIE_CAP, (name, r, near.mean())
    f = kr.FULL_CASE
    Y, _, _ = kr.blobs(f['seed'], f['n'], f['d'], f['C'])
    for r in range(6):
        init = Y[np.random.default_rng(r).choice(f['n'], size=f['C'], replace=False)]
        near = kr.lloyd(Y, init, 300, 1e-4)[5]
        assert near.mean() <= kr.NEAR_TIE_CAP, (r, near.mean())


def test_assign_ties_take_the_lowest_index():
    Y = np.array([[0.0, 0.0], [2.0, 0.0]])
    labels, best, near = kr.assign(Y, np.array([[1.0, 0.0], [1.0, 0.0], [5.0, 5.0]]))
    assert labels.tolist() == [0, 0] and best.tolist() == [1.0, 1.0] and near.all()


def test_lloyd_keeps_the_centre_of_an_empty_cluster():
    Y = np.array([[0.0], [1.0], [10.0], [11.0]])
    init = np.array([[0.5], [10.5], [1000.0]])
    labels, centers, inertia, n_iter, conv, _, _ = kr.lloyd(Y, init, 10, 0.0)
    assert labels.tolist() == [0, 0, 1, 1] and centers[2, 0] == 1000.0 and conv and n_iter == 1
    assert inertia == 1.0


def test_kmeanspp_pick_on_hand_made_weights():
    w = np.array([0.0, 0.0, 3.0, 0.0, 1.0, 0.0])
    assert kr.kmeanspp_pick(w, 0.0) == 2                      # u = 0: the first positive row
    picks = {kr.kmeanspp_pick(w, u) for u in np.linspace(0.0, 1.0, 101, endpoint=False)}
    assert picks == {2, 4}                                    # a zero-weight row is never picked
    assert kr.kmeanspp_pick(w, 0.74) == 2 and kr.kmeanspp_pick(w, 0.75) == 4
    assert kr.kmeanspp_pick(w, 1.0) == 4                      # u * total == total: the last positive row


def test_distinct_rows_are_distinct_and_in_range():
    from oriana_amd import cluster
    for n, C in ((5, 5), (7, 3), (1000, 20)):
        u = cluster.draws(3, 4, C)
        for r in range(4):
            g = cluster.distinct_rows(u[r].tolist(), n)
            assert len(set(g)) == C and min(g) >= 0 and max(g) < n
    assert torch.equal(cluster.draws(3, 4, 5), cluster.draws(3, 4, 5)) and not torch.equal(cluster.draws(3, 4, 5), cluster.draws(4, 4, 5))


def test_helper_entries(lib):
    assert lib.oriana_kmeans_max_centers(0) == 0 and lib.oriana_kmeans_max_centers(257) == 0
    assert lib.oriana_kmeans_max_centers(100) == 81 and lib.oriana_kmeans_max_centers(64) == 128
    assert lib.oriana_kmeans_max_centers(256) == 32 and lib.oriana_kmeans_max_centers(1) == 2048
    for d in (1, 2, 3, 20, 64, 65, 100, 128, 256):
        cmax = lib.oriana_kmeans_max_centers(d)
        assert cmax * ((d + 3) // 4 * 4) <= 8192 < (cmax + 1) * ((d + 3) // 4 * 4)
        assert lib.oriana_kmeans_group(d, cmax) in (2, 4) and lib.oriana_kmeans_group(d, 1) == 4
        assert lib.oriana_kmeans_group(d, cmax + 1) == 0
        assert lib.oriana_kmeans_scratch_bytes(1000, d, cmax, 3, 2) > 0
        assert lib.oriana_kmeans_scratch_bytes(1000, d, cmax + 1, 3, 2) == -2
    assert lib.oriana_kmeans_partial_rows() >= 1 and lib.oriana_kmeans_tile_rows() == 64
    assert lib.oriana_kmeans_scratch_bytes(-1, 4, 2, 1, 0) == -1


def test_step_argument_errors_without_gpu(lib):
    """All argument validation happens before any HIP call."""
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    p -= p % 16

    def step(Y=p, n=10, d=4, ldy=4, centers=p, C=2, R=1, sums=p, counts=p, inertia=p, labels=None, lr=0, mind=None, scratch=p,
             blocks=0):
        return lib.oriana_kmeans_step(Y, n, d, ldy, centers, C, R, sums, counts, inertia, labels, lr, mind, scratch, blocks, None)

    for kw in (dict(n=-1), dict(d=0), dict(C=0), dict(R=0), dict(ldy=3), dict(blocks=-1), dict(centers=None), dict(sums=None),
               dict(counts=None), dict(inertia=None), dict(scratch=None), dict(Y=None), dict(labels=p, lr=1), dict(labels=p, lr=-1),
               dict(scratch=p + 4)):
        assert step(**kw) == -1, kw                                          # ORIANA_EINVAL
    assert step(d=257, ldy=257) == -2 and step(d=100, ldy=100, C=82) == -2            # ORIANA_EKRANGE
    assert step(d=100, ldy=100, C=82, centers=None) == -2                    # (the range before the pointers)
    assert step(C=0, d=300, ldy=300) == -1                                   # (the sizes before the range)


def test_kmeans_value_errors_without_a_device(lib):
    from oriana_amd import cluster
    Y = torch.zeros(10, 4)
    bad = [dict(n_clusters=0), dict(n_clusters=11), dict(n_clusters=2, n_init=0), dict(n_clusters=2, max_iter=-1),
           dict(n_clusters=2, tol=-1.0), dict(n_clusters=2, check_every=0), dict(n_clusters=2, init='bogus'),
           dict(n_clusters=2, init=np.zeros((3, 4))), dict(n_clusters=2, n_init=3, init=np.zeros((2, 2, 4))),
           dict(n_clusters=2, init=np.zeros((2, 5))), dict(n_clusters=2, restarts_per_pass=0), dict(n_clusters=2, tol=float('nan'))]
    for kw in bad:
        with pytest.raises(ValueError):
            cluster.kmeans(Y, **kw)
    with pytest.raises(ValueError):
        cluster.kmeans(Y.double(), 2)
    with pytest.raises(ValueError):
        cluster.kmeans(torch.zeros(10, 8)[:, ::2], 2)
    with pytest.raises(ValueError):
        cluster.kmeans(np.zeros((10, 4), np.float32), 2)
    with pytest.raises(ValueError):
        cluster.kmeans(torch.zeros(3000, 100), 82)                            # beyond max_centers(100)
    with pytest.raises(ValueError):
        cluster.kmeans(torch.zeros(300, 300), 2)                              # d not served


def test_cluster_cells_value_errors_without_a_device():
    from oriana_amd.models import GaP
    m = object.__new__(GaP)
    m.k = 6
    for kw in (dict(features='bogus'), dict(factors=[6]), dict(factors=[-1]), dict(factors=[]), dict(factors=[0.5]),
               dict(factors=[[0, 1]]), dict(pg=None)):
        with pytest.raises(ValueError):
            m.cluster_cells(3, **kw)
