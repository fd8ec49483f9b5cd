# -*- coding: utf-8 -*-
"""The silhouette and the adjusted Rand index without a GPU: the float64 restatement against scikit-learn, silhouette_from_sums
on CPU tensors, the plan, every ValueError that needs no device, every argument error of the C entry, and adjusted_rand()."""
import ctypes

import numpy as np
import pytest
import torch

import kmeans_reference as kr
import silhouette_reference as sr


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from oriana_amd import _lib
    return _lib.load()


def _small():
    """90 rows in 4 used ids of 6: id 2 is a singleton, id 4 unused, rows 0 and 89 identical.  Unit-scale blobs: scikit-learn
    forms its float64 distances as |x|^2 + |y|^2 - 2 x.y, which loses digits to cancellation under kmeans_reference.blobs'
    feature scale of 1e3 (9e-15 on the values there), so it is compared where it is accurate itself."""
    rng = np.random.default_rng(1)
    which = rng.integers(0, 3, size=90)
    Y = (rng.normal(0.0, 3.0, size=(3, 4))[which] + rng.normal(size=(90, 4))).astype(np.float32)
    Y[89], which[89] = Y[0], which[0]
    labels = which.astype(np.int64)
    labels[labels == 2] = 5
    labels[17] = 2
    return Y, labels


def test_reference_against_scikit_learn():
    metrics = pytest.importorskip('sklearn.metrics')
    Y, labels = _small()
    assert np.array_equal(Y[0], Y[89]) and (labels == 2).sum() == 1 and (labels == 4).sum() == 0
    S, counts, values, a, b = sr.silhouette(Y, labels)
    want = metrics.silhouette_samples(Y.astype(np.float64), labels, metric='euclidean')
    assert np.abs(values - want).max() <= 2e-15
    assert values[17] == 0.0 and a[17] == 0.0 and counts.tolist() == np.bincount(labels, minlength=6).tolist()
    assert abs(values.mean() - metrics.silhouette_score(Y.astype(np.float64), labels)) <= 2e-15
    # the sums themselves, against the plain pairwise form
    D = np.sqrt(((Y.astype(np.float64)[:, None, :] - Y.astype(np.float64)[None, :, :]) ** 2).sum(-1))
    for c in range(6):
        np.testing.assert_allclose(S[c], D[:, labels == c].sum(1), rtol=1e-13, atol=0)
    assert np.all(S[4] == 0.0) and S[labels[89], 0] > 0.0


def test_inputs_keep_differences_above_the_underflow():
    for case in sr.CASES:
        Y, labels = sr.case_inputs(case)
        name, n, d, C, _, _ = case
        assert Y.shape == (n, d) and labels.min() >= 0 and labels.max() < C and np.all(np.isfinite(Y)), name
        assert 2 <= (np.bincount(labels, minlength=C) > 0).sum() <= n - 1, name
        assert sr.min_nonzero_difference(Y) >= sr.MIN_DIFFERENCE, name
    Y, labels = sr.zeros_case()
    assert sr.min_nonzero_difference(Y) >= sr.MIN_DIFFERENCE
    edges = np.bincount(sr.case_inputs(sr.CASES[6])[1], minlength=9)
    assert edges.tolist() == [1, 2, 7, 8, 0, 9, 63, 64, 46]
    assert np.all(np.bincount(sr.case_inputs(sr.CASES[7])[1]) == 4)
    c = sr.PARTITION_CASE
    assert sr.min_nonzero_difference(kr.blobs(c['seed'], c['n'], c['d'], c['n_blobs'])[0]) >= sr.MIN_DIFFERENCE


def test_silhouette_from_sums_on_cpu_tensors():
    from oriana_amd import cluster
    Y, labels = _small()
    S, counts, values, a, b = sr.silhouette(Y, labels)
    for cnt, lab in ((counts, labels), (torch.from_numpy(counts), torch.from_numpy(labels)), (counts.tolist(), labels.astype(np.int32))):
        v, aa, bb = cluster.silhouette_from_sums(torch.from_numpy(S), cnt, lab)
        assert v.dtype == torch.float64 and v.device.type == 'cpu'
        assert np.abs(v.numpy() - values).max() <= 4 * 2.0 ** -53
        assert np.all(np.abs(aa.numpy() - a) <= 2.0 ** -52 * a) and np.all(np.abs(bb.numpy() - b) <= 2.0 ** -52 * b)
        assert v[17] == 0.0 and aa[17] == 0.0 and bb[17] > 0.0          # the singleton
    # a block of the rows gives that block of the values
    v, _, _ = cluster.silhouette_from_sums(torch.from_numpy(S[:, 10:40].copy()), counts, labels[10:40])
    assert np.abs(v.numpy() - values[10:40]).max() <= 4 * 2.0 ** -53
    # a = b = 0: two clusters of one repeated point each; an unused id in between
    Z, zl = sr.zeros_case()
    Sz, cz, vz, az, bz = sr.silhouette(Z, zl, C=6)
    v, aa, bb = cluster.silhouette_from_sums(torch.from_numpy(Sz), cz, zl)
    rep = zl <= 1
    assert np.all(az[rep] == 0.0) and np.all(bz[rep] == 0.0) and np.all(vz[rep] == 0.0)
    assert torch.isfinite(v).all() and np.all(v.numpy()[rep] == 0.0) and np.all(aa.numpy()[rep] == 0.0) and np.all(bb.numpy()[rep] == 0.0)
    assert np.abs(v.numpy() - vz).max() <= 4 * 2.0 ** -53
    for bad in (dict(S=torch.zeros(3, 4), counts=[2, 2, 0], labels=[0, 0, 1, 1]),
                dict(S=torch.zeros(3, 4, dtype=torch.float64), counts=[4, 0, 0], labels=[0, 0, 0, 0]),
                dict(S=torch.zeros(3, 4, dtype=torch.float64), counts=[2, 2], labels=[0, 0, 1, 1]),
                dict(S=torch.zeros(3, 4, dtype=torch.float64), counts=[2, 2, 0], labels=[0, 0, 1])):
        with pytest.raises(ValueError):
            cluster.silhouette_from_sums(**bad)


def test_plan(lib):
    from oriana_amd import cluster
    budget = cluster.SCRATCH_BUDGET
    one = lambda nq, n, d, C, blocks=0: lib.oriana_cluster_distance_sums_scratch_bytes_for(nq, n, d, C, blocks, 16, d)
    # the sizes the silhouette is meant for: one call
    qb, chunk, nbytes = cluster.silhouette_plan(262144, 262144, 100, 20)
    assert (qb, chunk) == (262144, 262144) and nbytes == one(262144, 262144, 100, 20)
    assert nbytes + 262144 * (400 + 24) + 8 * 20 * 262144 <= budget
    for nq, n, d, C in ((2 ** 20, 2 ** 20, 100, 8), (2 ** 20, 2 ** 20, 100, 1000), (2 ** 21, 2 ** 21, 6, 20), (5000, 2 ** 23, 255, 50),
                        (2 ** 18, 2 ** 18, 256, 4096)):
        qb, chunk, nbytes = cluster.silhouette_plan(nq, n, d, C)
        assert qb % 64 == 0 or qb == nq, (nq, n, d, C, qb)
        assert chunk * (4 * d + 24) <= budget // 2 or chunk == 1, (nq, n, d, C, chunk)
        assert nbytes + min(chunk, n) * (4 * d + 24) + 8 * C * min(qb, nq) <= budget, (nq, n, d, C, qb, chunk, nbytes)
        for b in {min(qb, nq), nq % qb} - {0}:
            for c in {min(chunk, n), n % chunk} - {0}:
                assert nbytes >= one(b, c, d, C), (nq, n, d, C, b, c)
    # the resident sums of a row-sharded run count in full, whatever the query block
    qb, _, _ = cluster.silhouette_plan(2 ** 18, 2 ** 18, 100, 256, resident=True)
    qf, _, _ = cluster.silhouette_plan(2 ** 18, 2 ** 18, 100, 256)
    assert qb <= qf
    # what the caller fixes stays fixed; a small budget ends at one tile of queries and one candidate, not in a loop
    assert cluster.silhouette_plan(700, 700, 100, 7, candidate_chunk=64, query_block=100)[:2] == (100, 64)
    assert cluster.silhouette_plan(700, 700, 100, 7, budget=1)[:2] == (64, 1)
    assert cluster.silhouette_plan(0, 0, 4, 2)[:2] == (1, 1)
    # the scratch: a padded image only where d is no multiple of four; 512 bytes per tile and item
    img = lambda n, d: (n * ((d + 3) // 4 * 4) * 4 + 15) // 16 * 16
    assert one(700, 900, 6, 7, 3) - img(900, 6) == one(700, 900, 8, 7, 3)
    assert lib.oriana_cluster_distance_sums_scratch_bytes_for(700, 900, 8, 7, 3, 20, 8) == one(700, 900, 8, 7, 3) + img(900, 8)
    assert lib.oriana_cluster_distance_sums_scratch_bytes_for(700, 900, 8, 7, 3, 16, 9) == one(700, 900, 8, 7, 3) + img(900, 8)
    tab = ((2 * 10 + 8) * 4 + 15) // 16 * 16
    assert one(700, 900, 8, 7, 3) == tab + 11 * 10 * 512


def test_silhouette_value_errors_without_a_device(lib):
    from oriana_amd import cluster
    assert cluster.max_clusters() == lib.oriana_cluster_distance_sums_max_clusters() >= 4096
    Y = torch.zeros(10, 4)
    Y[:, 0] = torch.arange(10)
    lab = np.arange(10) % 3
    nan = Y.clone()
    nan[3, 2] = float('nan')
    bad = [(Y.double(), lab, {}), (torch.zeros(10), lab, {}), (np.zeros((10, 4), np.float32), lab, {}), (torch.zeros(10, 8)[:, ::2], lab, {}),
           (torch.zeros(10, 300), lab, {}), (torch.zeros(10, 0), lab, {}),
           (Y, lab.astype(np.float64), {}), (Y, torch.zeros(10), {}), (Y, lab[:9], {}), (Y, np.zeros((10, 1), np.int64), {}),
           (Y, lab - 1, {}), (Y, torch.from_numpy(lab) - 1, {}),
           (Y, lab, dict(n_clusters=2)), (Y, lab, dict(n_clusters=cluster.max_clusters() + 1)), (Y, lab * 10 ** 6, {}),
           (Y, np.zeros(10, np.int64), {}), (Y, np.zeros(10, np.int64), dict(n_clusters=5)), (Y, np.arange(10), {}),
           (nan, lab, {}), (Y, lab, dict(blocks=-1)), (Y, lab, dict(candidate_chunk=0)), (Y, lab, dict(query_block=0)),
           (Y, lab, {})]                                                                   # (the last: a CPU tensor)
    for T, l, kw in bad:
        with pytest.raises(ValueError):
            cluster.silhouette(T, l, **kw)


def test_cell_silhouette_value_errors_without_a_device():
    from oriana_amd.models import GaP
    m = object.__new__(GaP)
    m.k = 6
    for kw in (dict(features='bogus'), dict(factors=[6]), dict(factors=[]), dict(pg=None)):
        with pytest.raises(ValueError):
            m.cell_silhouette(np.zeros(4, np.int64), **kw)


def test_distance_sums_argument_errors_without_gpu(lib):
    """All argument validation happens before any HIP call."""
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    p -= p % 16
    cmax = lib.oriana_cluster_distance_sums_max_clusters()
    assert cmax >= 4096

    def sums(Q=p, nq=10, ldq=4, Y=p, n=10, ldy=4, d=4, off=(0, 4, 10), C=None, out=p, lds=10, acc=0, scratch=p, blocks=0):
        arr = None if off is None else (ctypes.c_int64 * len(off))(*off)
        C = (len(off) - 1 if off is not None else 2) if C is None else C
        return lib.oriana_cluster_distance_sums(Q, nq, ldq, Y, n, ldy, d, None if arr is None else ctypes.addressof(arr), C, out, lds,
                                                acc, scratch, blocks, None)

    for kw in (dict(nq=-1), dict(n=-1, off=(0, 0, -1)), dict(d=0), dict(C=-1), dict(blocks=-1), dict(ldq=3), dict(ldy=3), dict(lds=9),
               dict(Q=None), dict(Y=None), dict(out=None), dict(scratch=None), dict(off=None), dict(scratch=p + 4),
               dict(off=(0, 11, 10)), dict(off=(1, 4, 10)), dict(off=(0, 4, 9)), dict(off=(0, 4, 11)), dict(off=(0, -1, 10)),
               dict(n=2 ** 31 - 8, off=(0, 4, 2 ** 31 - 8)), dict(nq=2 ** 31, lds=2 ** 31), dict(nq=2 ** 40, lds=2 ** 40)):
        assert sums(**kw) == -1, kw                                          # ORIANA_EINVAL
    assert sums(d=257, ldq=257, ldy=257) == -2                               # ORIANA_EKRANGE
    many = (0,) * (cmax + 1) + (10,)
    assert sums(off=many) == -2
    assert sums(off=many, out=None) == -2                                    # (the range before the pointers)
    assert sums(d=300, ldq=300, ldy=300, lds=9) == -1                        # (the sizes before the range)
    assert sums(nq=0, Q=None, lds=0) == 0                                    # no queries: a no-op, no HIP call
    assert sums(nq=0, Q=None, n=0, Y=None, off=(0, 0, 0), lds=0) == 0
    by = lib.oriana_cluster_distance_sums_scratch_bytes_for
    assert by(10, 10, 4, 2, 0, p, 4) > 0 and by(0, 0, 4, 0, 0, None, 4) >= 0
    for args in ((-1, 10, 4, 2, 0, p, 4), (10, -1, 4, 2, 0, p, 4), (10, 10, 0, 2, 0, p, 4), (10, 10, 4, -1, 0, p, 4),
                 (10, 10, 4, 2, -1, p, 4), (10, 10, 4, 2, 0, p, 3), (2 ** 31, 10, 4, 2, 0, p, 4), (10, 2 ** 31 - 8, 4, 2, 0, p, 4)):
        assert by(*args) == -1, args
    assert by(10, 10, 257, 2, 0, p, 257) == -2 and by(10, 10, 4, cmax + 1, 0, p, 4) == -2
    # the raw Python call checks a scratch it is handed and its sums before anything is launched (CPU tensors)
    from oriana_amd import cluster
    Q, Y = torch.zeros(70, 4), torch.zeros(300, 4)
    with pytest.raises(ValueError):
        cluster.distance_sums(Q, Y, [0, 100, 300], scratch=torch.empty(16, dtype=torch.uint8))
    for kw in (dict(sums=torch.zeros(2, 70)), dict(sums=torch.zeros(3, 70, dtype=torch.float64)), dict(accumulate=True),
               dict(sums=torch.zeros(70, 2, dtype=torch.float64).t())):
        with pytest.raises(ValueError):
            cluster.distance_sums(Q, Y, [0, 100, 300], **kw)
    with pytest.raises(ValueError):
        cluster.distance_sums(Q, torch.zeros(300, 5), [0, 100, 300])


def _ari_integers(M):
    """scikit-learn's pair-count formula on a contingency table, in Python integers up to the final division."""
    M = np.asarray(M)
    n = int(M.sum())
    sq = sum(int(v) ** 2 for v in M.ravel())
    fp = sum(int(v) ** 2 for v in M.sum(0)) - sq
    fn = sum(int(v) ** 2 for v in M.sum(1)) - sq
    tp, tn = sq - n, n * n - fp - fn - sq
    if fp == 0 and fn == 0:
        return 1.0
    return 2 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def test_adjusted_rand():
    from oriana_amd import cluster
    # by hand: a = (0 0 1 1), b = (0 0 1 2): table [[2 0 0] [0 1 1]]: tp = 2, fp = 0, fn = 2, tn = 8 (ordered pairs):
    # 2 (16 - 0) / ((4)(10) + (2)(8)) = 32 / 56
    assert cluster.adjusted_rand([0, 0, 1, 1], [0, 0, 1, 2]) == 32 / 56
    # a = (0 0 1 1), b = (0 1 0 1): table all ones: tp = 0, fp = fn = 4, tn = 4: 2 (0 - 16) / (4 * 8 + 4 * 8) = -0.5
    assert cluster.adjusted_rand([0, 0, 1, 1], [0, 1, 0, 1]) == -0.5
    assert cluster.adjusted_rand([0, 0, 1, 1], [1, 1, 0, 0]) == 1.0 and cluster.adjusted_rand([3, 3, 3], [0, 0, 0]) == 1.0
    assert cluster.adjusted_rand([0, 1, 2], [2, 0, 1]) == 1.0 and cluster.adjusted_rand([0], [5]) == 1.0
    # a = (0 0 0), b = (0 1 2): tp = 0, fp = 0, fn = 6, tn = 0 -> 0 / (6 * 6 + 0) = 0
    assert cluster.adjusted_rand([0, 0, 0], [0, 1, 2]) == 0.0
    rng = np.random.default_rng(5)
    a = rng.integers(0, 7, size=5000)
    b = np.where(rng.random(5000) < 0.7, a, rng.integers(0, 9, size=5000))
    got = cluster.adjusted_rand(a, b)
    assert abs(got - kr.adjusted_rand_index(a, b)) <= 1e-12
    assert got == cluster.adjusted_rand(torch.from_numpy(a), torch.from_numpy(b).to(torch.int32)) == cluster.adjusted_rand(b, a)
    # invariance under a permutation of the label ids, exactly
    perm = rng.permutation(9)
    assert cluster.adjusted_rand(a, perm[b]) == got and cluster.adjusted_rand(rng.permutation(7)[a], b) == got
    for bad in (([0, 1], [0]), ([0.0, 1.0], [0, 1]), ([0, -1], [0, 1]), ([[0, 1]], [[0, 1]]), ([0, 2 ** 20], [0, 2 ** 20])):
        with pytest.raises(ValueError):
            cluster.adjusted_rand(*bad)


def test_adjusted_rand_against_scikit_learn():
    metrics = pytest.importorskip('sklearn.metrics')
    from oriana_amd import cluster
    rng = np.random.default_rng(6)
    for n, ca, cb in ((300, 3, 4), (5000, 12, 10), (17, 17, 2)):
        a, b = rng.integers(0, ca, size=n), rng.integers(0, cb, size=n)
        b[:n // 2] = a[:n // 2] % cb
        assert abs(cluster.adjusted_rand(a, b) - metrics.adjusted_rand_score(a, b)) <= 1e-14


def test_adjusted_rand_beyond_int64_products():
    from oriana_amd import cluster
    n = 3000000
    rng = np.random.default_rng(7)
    a = torch.from_numpy(rng.integers(0, 3, size=n))
    b = torch.where(torch.from_numpy(rng.random(n) < 0.9), a, torch.from_numpy(rng.integers(0, 4, size=n)))
    M = np.zeros((3, 4), dtype=np.int64)
    np.add.at(M, (a.numpy(), b.numpy()), 1)
    sq = sum(int(v) ** 2 for v in M.ravel())
    tp, tn = sq - n, n * n - (sum(int(v) ** 2 for v in M.sum(0)) - sq) - (sum(int(v) ** 2 for v in M.sum(1)) - sq) - sq
    assert tp * tn > 2 ** 63                                                  # (the products this test is about)
    got = cluster.adjusted_rand(a, b)
    assert got == _ari_integers(M) and 0.5 < got < 1.0
