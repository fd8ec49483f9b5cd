# -*- coding: utf-8 -*-
"""The k-nearest-neighbour search without a GPU: the float64 restatement against a plain argsort, the share of non-clear queries
of every seeded input of the GPU tests, the helper entries, and every argument error that needs no device."""
import ctypes

import numpy as np
import pytest
import torch

import knn_reference as nr


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from oriana_amd import _lib
    return _lib.load()


def test_reference_against_a_plain_argsort():
    Y, _ = nr.blobs(3, 90, 7, 3)
    Q = nr.blobs(4, 20, 7, 3)[0]
    Y64, Q64 = Y.astype(np.float64), Q.astype(np.float64)
    D = ((Q64[:, None, :] - Y64[None, :, :]) ** 2).sum(-1)
    idx, dist, _ = nr.neighbors(Y, Q, 6, y0=100)
    assert np.array_equal(idx, np.argsort(D, axis=1, kind='stable')[:, :6] + 100)
    np.testing.assert_allclose(dist, np.sort(D, axis=1)[:, :6], rtol=1e-13)
    # the rows themselves, each left out of its own list, under shifted global indices
    D = ((Y64[:, None, :] - Y64[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    idx, dist, _ = nr.neighbors(Y, None, 5, exclude=True, q0=40, y0=40)
    assert np.array_equal(idx, np.argsort(D, axis=1, kind='stable')[:, :5] + 40)
    assert not np.any(idx == np.arange(40, 130)[:, None])
    # queries [10, 30) of the same rows: the exclusion follows the global indices
    part, _, _ = nr.neighbors(Y, Y[10:30], 5, exclude=True, q0=50, y0=40)
    assert np.array_equal(part, idx[10:30])
    # fewer candidates than k: the padded tail; ties take the lower index
    idx, dist, _ = nr.neighbors(Y[:4], None, 6, exclude=True)
    assert np.all(idx[:, 3:] == -1) and np.all(np.isposinf(dist[:, 3:])) and np.all(idx[:, :3] >= 0)
    T = np.array([[0.0], [1.0], [1.0], [-1.0], [5.0]], dtype=np.float32)
    idx, dist, D = nr.neighbors(T, None, 2, exclude=True)
    assert idx[0].tolist() == [1, 2] and idx[4].tolist() == [1, 2] and dist[0].tolist() == [1.0, 1.0]
    clear = nr.clear_queries(D, 2, 1)
    assert not clear[0] and clear[4] and clear[1]                 # row 0: places 2 and 3 tie; row 1: {2, 0} then 3 at 4
    assert nr.clear_queries(D, 4, 1).all() and nr.clear_queries(D, 7, 1).all()


def test_re_drawn_blobs_have_no_duplicate_rows():
    for seed, n, d in ((1, 8, 2), (2, 300, 20), (3, 64, 1)):
        Y, _ = nr.blobs(seed, n, d, 4)
        assert np.unique(Y, axis=0).shape[0] == n
        K = nr.kr.blobs(seed, n, d, 4)[0]
        keep = np.setdiff1d(np.arange(n), (n - 1, n // 2, 5))
        assert np.array_equal(Y[keep], K[keep]) and np.array_equal(K[n - 1], K[0])


def test_non_clear_share_of_every_gpu_input(lib):
    for case in nr.CASES:
        name, n, d, k, extra, nq = nr.resolve_case(case, lib)
        Y, Q = nr.case_inputs(case)
        assert Y.shape == (n, d) and (Q is None) == (nq is None) and (Q is None or Q.shape == (nq, d))
        D = nr.masked_distances(Y, Q, exclude=Q is None)
        share = 1.0 - nr.clear_queries(D, k, d).mean()
        assert share <= nr.NEAR_TIE_CAP, (name, share)
    c = nr.INVARIANCE_CASE
    Y, _ = nr.blobs(c['seed'], c['n'], c['d'], c['n_blobs'])
    share = 1.0 - nr.clear_queries(nr.masked_distances(Y, exclude=True), c['k'], c['d']).mean()
    assert share <= nr.NEAR_TIE_CAP, share


def test_helper_entries(lib):
    assert lib.oriana_knn_max_neighbors(0) == 0 and lib.oriana_knn_max_neighbors(257) == 0
    assert lib.oriana_knn_max_neighbors(-3) == 0
    for d in (1, 64, 100, 128, 256):
        kmax = lib.oriana_knn_max_neighbors(d)
        assert kmax >= 32
        # the query tile and four waves' lists fill the 160 KiB of a CU and no more
        dp = (d + 3) // 4 * 4
        assert 4 * dp * 65 + 2048 * kmax <= 160 * 1024 < 4 * dp * 65 + 2048 * (kmax + 1)
        for blocks in (0, 1, 3):
            assert lib.oriana_knn_scratch_bytes(1000, 900, d, kmax, blocks) > 0
            assert lib.oriana_knn_scratch_bytes(1000, 900, d, kmax + 1, blocks) == -2
        assert lib.oriana_knn_scratch_bytes(0, 0, d, 1, 0) >= 0
    assert lib.oriana_knn_scratch_bytes(10, 10, 257, 1, 0) == -2
    for args in ((-1, 10, 4, 2, 0), (10, -1, 4, 2, 0), (10, 10, 0, 2, 0), (10, 10, 4, 0, 0), (10, 10, 4, 2, -1)):
        assert lib.oriana_knn_scratch_bytes(*args) == -1, args
    assert lib.oriana_knn_tile_rows() == 64
    # eight waves where their lists fit beside the tile, else four; at most 64 partial lists per query
    assert lib.oriana_knn_waves(100, 15) == 8 and lib.oriana_knn_waves(100, 33) == 8 and lib.oriana_knn_waves(100, 34) == 4
    assert lib.oriana_knn_waves(256, 23) == 8 and lib.oriana_knn_waves(256, 24) == 4 and lib.oriana_knn_waves(256, 47) == 4
    assert lib.oriana_knn_waves(256, 48) == 0 and lib.oriana_knn_waves(0, 1) == 0 and lib.oriana_knn_waves(4, 0) == 0
    assert lib.oriana_knn_splits(700, 700, 100, 15, 1) == 1 and lib.oriana_knn_splits(700, 700, 100, 15, 3) == 3
    assert lib.oriana_knn_splits(700, 9, 100, 15, 3) == 1         # (at least one step per wave)
    assert 1 <= lib.oriana_knn_splits(700, 700, 100, 15, 0) <= 8
    assert lib.oriana_knn_splits(700, 10 ** 6, 100, 15, 100) == 8 and lib.oriana_knn_splits(700, 10 ** 6, 100, 40, 100) == 16
    assert lib.oriana_knn_splits(-1, 5, 100, 15, 0) == -1 and lib.oriana_knn_splits(5, 5, 100, 68, 0) == -2


def test_scratch_of_a_call_and_the_default_plan(lib):
    """The scratch a chunk of the candidates cannot shrink is bounded by splitting the queries: the default plan stays within the
    budget with a handful of calls at the sizes the search is meant for, and never walks the candidate chunk down instead."""
    from oriana_amd import cluster
    budget = cluster.SCRATCH_BUDGET
    # no image where Y serves as one (d and the row stride multiples of four, the base 16-byte aligned)
    for d, ldy, yp, direct in ((100, 100, 64, True), (100, 104, 64, True), (100, 100, 68, False), (100, 101, 64, False),
                               (6, 6, 64, False), (6, 8, 64, False)):
        full = lib.oriana_knn_scratch_bytes(1000, 900, d, 15, 0)
        own = lib.oriana_knn_scratch_bytes_for(1000, 900, d, 15, 0, yp, ldy)
        image = (900 * ((d + 3) // 4 * 4) * 4 + 15) // 16 * 16
        assert own == (full - image if direct else full), (d, ldy, yp)
    assert lib.oriana_knn_scratch_bytes_for(10, 10, 100, 15, 0, 64, 99) == -1
    assert lib.oriana_knn_scratch_bytes_for(10, 10, 100, 68, 0, 64, 100) == -2
    for nq, n, d, k, yp in ((2 ** 20, 2 ** 20, 100, 15, 64), (2 ** 20, 2 ** 20, 100, 30, 64), (2 ** 20, 2 ** 20, 100, 67, 64),
                            (2 ** 20, 2 ** 20, 100, 15, 68), (2 ** 21, 2 ** 21, 100, 15, 64), (2 ** 20, 2 ** 20, 6, 15, 64),
                            (2 ** 20, 2 ** 20, 256, 47, 64), (5000, 2 ** 22, 100, 15, 64)):
        qb, chunk, nbytes = cluster.knn_plan(nq, n, d, k, y_ptr=yp, ldy=d)
        calls = -(-nq // qb) * -(-n // chunk)
        assert qb % 64 == 0 or qb == nq, (nq, n, d, k, yp, qb)
        assert nbytes <= budget and calls <= 16, (nq, n, d, k, yp, qb, chunk, nbytes)
        assert nbytes == lib.oriana_knn_scratch_bytes_for(min(qb, nq), min(chunk, n), d, k, 0, yp, d)
    assert cluster.knn_plan(2 ** 20, 2 ** 20, 100, 15, y_ptr=64)[:2] == (2 ** 19, 2 ** 20)          # two calls, no more
    assert cluster.knn_plan(262144, 262144, 100, 30, y_ptr=64)[:2] == (262144, 262144)              # one call
    # a padded image beyond half the budget: the candidates are cut first, then the queries
    qb, chunk, nbytes = cluster.knn_plan(4096, 2 ** 24, 255, 15, y_ptr=64, ldy=255)
    assert chunk < 2 ** 24 and chunk * 256 * 4 <= budget // 2 < 2 * chunk * 256 * 4 + 2 ** 21 and qb == 4096 and nbytes <= budget
    # what the caller fixes stays fixed; a small budget ends at one tile of queries, not in a loop
    assert cluster.knn_plan(700, 700, 100, 15, candidate_chunk=64, query_block=100)[:2] == (100, 64)
    assert cluster.knn_plan(700, 700, 100, 15, budget=1)[:2] == (64, 1)
    assert cluster.knn_plan(0, 0, 4, 1) == (1, 1, 0)


def test_planned_scratch_serves_every_call_issued(lib):
    """The scratch of a call is not monotone in its queries: with blocks = 0 a shorter last block has fewer tiles, is cut into
    more candidate ranges and can need more than the full block.  The plan's bytes cover every (query block, candidate chunk)
    that knn() issues, and knn_step refuses a scratch that is too small instead of letting the kernel write past it."""
    from oriana_amd import cluster
    d, k, yp = 100, 15, 64
    one = lambda nq, n, blocks=0: lib.oriana_knn_scratch_bytes_for(nq, n, d, k, blocks, yp, d)
    cus = lib.oriana_device_cus()
    full, short = 2 * cus * 64, (2 * cus - 1) * 64               # S = 1 at two tiles per CU, S = 2 one tile below
    assert lib.oriana_knn_splits(full, 60000, d, k, 0) == 1 and lib.oriana_knn_splits(short, 60000, d, k, 0) == 2
    assert one(short, 60000) > one(full, 60000)                   # (the non-monotone pair itself)
    cases = [(full + short, 60000, full, None, 0), (full + 300 * 64, 60000, full, None, 0), (full + 64, 60000, full, 7000, 0),
             (51968, 51968, 32768, None, 0), (3 * short + 1, 60000, short, 999, 0), (full + short, 60000, full, None, 3),
             (700, 700, 640, 300, 0), (700, 700, 699, None, 0), (2 ** 20 + 64, 2 ** 20 + 64, None, None, 0)]
    for nq, n, query_block, candidate_chunk, blocks in cases:
        qb, chunk, nbytes = cluster.knn_plan(nq, n, d, k, blocks, yp, d, candidate_chunk, query_block)
        for b in {min(qb, nq), nq % qb} - {0}:
            for c in {min(chunk, n), n % chunk} - {0}:
                assert nbytes >= one(b, c, blocks), (nq, n, query_block, candidate_chunk, blocks, b, c)
    assert cluster.knn_plan(full + short, 60000, d, k, 0, yp, d, None, full)[2] == one(short, 60000)
    # the raw call checks a scratch it is handed before anything is launched (CPU tensors: only sizes and pointers are read)
    Q, Y = torch.zeros(short, d), torch.zeros(60000, d)
    idx, d2 = torch.zeros(short, k, dtype=torch.int32), torch.zeros(short, k)
    with pytest.raises(ValueError):
        cluster.knn_step(Q, Y, idx, d2, scratch=torch.empty(one(full, 60000), dtype=torch.uint8))


def test_knn_argument_errors_without_gpu(lib):
    """All argument validation happens before any HIP call."""
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)
    p -= p % 16

    def knn(Q=p, nq=10, ldq=4, q0=0, Y=p, n=10, ldy=4, y0=0, d=4, k=2, excl=0, merge=0, idx=p, d2=p, scratch=p, blocks=0):
        return lib.oriana_knn(Q, nq, ldq, q0, Y, n, ldy, y0, d, k, excl, merge, idx, d2, scratch, blocks, None)

    for kw in (dict(nq=-1), dict(n=-1), dict(d=0), dict(k=0), dict(ldq=3), dict(ldy=3), dict(blocks=-1), dict(q0=-1), dict(y0=-1),
               dict(Q=None), dict(Y=None), dict(idx=None), dict(d2=None), dict(scratch=None), dict(scratch=p + 4),
               dict(y0=2 ** 31 - 5), dict(n=2 ** 31), dict(n=2 ** 31 - 8), dict(nq=2 ** 31), dict(nq=2 ** 40, n=2 ** 40)):
        assert knn(**kw) == -1, kw                                           # ORIANA_EINVAL
    assert knn(d=257, ldq=257, ldy=257) == -2                                # ORIANA_EKRANGE
    kmax = lib.oriana_knn_max_neighbors(100)
    assert knn(d=100, ldq=100, ldy=100, k=kmax + 1) == -2
    assert knn(d=100, ldq=100, ldy=100, k=kmax + 1, idx=None) == -2          # (the range before the pointers)
    assert knn(d=300, ldq=300, ldy=300, k=0) == -1                           # (the sizes before the range)
    assert knn(nq=0, Q=None) == 0 and knn(nq=0, Q=None, n=0, Y=None) == 0    # no queries: a no-op, no HIP call
    assert knn(n=0, Y=None, merge=1) == 0                                    # nothing to merge in


def test_knn_value_errors_without_a_device(lib):
    from oriana_amd import cluster
    Y = torch.zeros(10, 4)
    assert cluster.max_neighbors(100) == lib.oriana_knn_max_neighbors(100) and cluster.max_neighbors(300) == 0
    bad = [dict(n_neighbors=0), dict(n_neighbors=-2), dict(n_neighbors=cluster.max_neighbors(4) + 1),
           dict(n_neighbors=2, exclude_self=True, queries=torch.zeros(3, 4)), dict(n_neighbors=2, queries=torch.zeros(3, 5)),
           dict(n_neighbors=2, queries=torch.zeros(3, 4, dtype=torch.float64)), dict(n_neighbors=2, queries=torch.zeros(4)),
           dict(n_neighbors=2, queries=np.zeros((3, 4), np.float32)), dict(n_neighbors=2, blocks=-1),
           dict(n_neighbors=2, candidate_chunk=0), dict(n_neighbors=2, query_block=0), dict(n_neighbors=2)]       # (the last: a CPU tensor)
    for kw in bad:
        with pytest.raises(ValueError):
            cluster.knn(Y, **kw)
    for T in (Y.double(), torch.zeros(10, 8)[:, ::2], np.zeros((10, 4), np.float32), torch.zeros(10), torch.zeros(3, 300),
              torch.zeros(3, 0), torch.zeros(10, 4).to(torch.int32)):
        with pytest.raises(ValueError):
            cluster.knn(T, 2)


def test_cell_neighbors_value_errors_without_a_device():
    from oriana_amd.models import GaP
    m = object.__new__(GaP)
    m.k = 6
    for kw in (dict(features='bogus'), dict(factors=[6]), dict(factors=[-1]), dict(factors=[]), dict(factors=[0.5]),
               dict(factors=[[0, 1]]), dict(pg=None), dict(n_neighbors=0), dict(exclude_self=False),
               dict(features='mean_log', queries=np.ones((3, 6))), dict(queries=np.ones((3, 5))), dict(queries=np.ones(6)),
               dict(queries=-np.ones((3, 6))), dict(queries=np.full((3, 6), np.nan))):
        with pytest.raises(ValueError):
            m.cell_neighbors(**kw)
