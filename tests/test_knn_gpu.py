# -*- coding: utf-8 -*-
"""oriana_knn and cluster.knn on the GPU against the float64 restatement of tests/knn_reference.py, under the bounds derived
there (none of them measured on the kernel), and the bit-for-bit independence of the result from every partition of the work."""
import numpy as np
import pytest
import torch

import kmeans_reference as kr
import knn_reference as nr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from oriana_amd import _lib
    return _lib.load()


def _dev(Y, extra=0):
    """Y on the device, optionally as the leading columns of a wider matrix (row stride d + extra) whose other columns are NaN."""
    n, d = Y.shape
    if not extra:
        return torch.from_numpy(Y).cuda()
    wide = torch.full((n, d + extra), float('nan'), dtype=torch.float32, device='cuda')
    wide[:, :d] = torch.from_numpy(Y).cuda()
    return wide[:, :d]


def _knn(Yd, k, **kw):
    from oriana_amd import cluster
    o = cluster.knn(Yd, k, **kw)
    torch.cuda.synchronize()
    assert o['indices'].is_cuda and o['sq_distances'].is_cuda
    return o['indices'].cpu().numpy(), o['sq_distances'].cpu().numpy()


@pytest.mark.parametrize('case', nr.CASES, ids=[c[0] for c in nr.CASES])
def test_single_call(lib, case):
    name, n, d, k, extra, nq = nr.resolve_case(case, lib)
    Y, Q = nr.case_inputs(case)
    idx, d2 = _knn(_dev(Y, extra), k, queries=None if Q is None else _dev(Q, extra))
    share = nr.check(Y, idx, d2, k, Q=Q, exclude=Q is None, what=name)
    print('%s: non-clear share %.2e' % (name, share))
    assert share <= nr.NEAR_TIE_CAP
    if name == 'short_tail':                    # 5 rows, k = 8: exactly 4 neighbours per row, then the padding
        assert np.all(idx[:, :4] >= 0) and np.all(idx[:, 4:] == -1) and np.all(np.isposinf(d2[:, 4:]))
    if name == 'one_row':
        assert idx.tolist() == [[-1]] and np.isposinf(d2).all()


@pytest.fixture(scope='module')
def base():
    c = nr.INVARIANCE_CASE
    Y, _ = nr.blobs(c['seed'], c['n'], c['d'], c['n_blobs'])
    Yd = _dev(Y)
    idx, d2 = _knn(Yd, c['k'])
    return Y, Yd, idx, d2


def test_invariance_case_matches_the_reference(base):
    Y, _, idx, d2 = base
    share = nr.check(Y, idx, d2, nr.INVARIANCE_CASE['k'], exclude=True, what='invariance case')
    assert share <= nr.NEAR_TIE_CAP


def test_bitwise_symmetry(base):
    _, _, idx, d2 = base
    pairs = 0
    for i in range(idx.shape[0]):
        for a, j in enumerate(idx[i]):
            back = np.nonzero(idx[j] == i)[0]
            if back.size:
                assert d2[i, a].tobytes() == d2[j, back[0]].tobytes(), (i, j)
                pairs += 1
    print('mutual pairs: %d' % pairs)
    assert pairs > 0


def test_invariance_bit_for_bit(lib, base):
    from oriana_amd import cluster
    Y, Yd, idx, d2 = base
    n, k = Y.shape[0], nr.INVARIANCE_CASE['k']

    def same(got, what):
        assert np.array_equal(got[0], idx) and got[1].tobytes() == d2.tobytes(), what

    same(_knn(Yd, k), 'the same call twice')
    for blocks in (0, 1, 3):
        same(_knn(Yd, k, blocks=blocks), 'blocks=%d' % blocks)
    d = Y.shape[1]
    assert [lib.oriana_knn_splits(n, n, d, k, b) for b in (1, 3)] == [1, 3]
    assert lib.oriana_knn_splits(n, n, d, k, 0) > 3                # (the default cuts this case finer than any of the above)
    # the work-group of four waves (k beyond what eight waves' lists leave room for) finds the same first k neighbours
    k4 = 40
    assert lib.oriana_knn_waves(d, k) == 8 and lib.oriana_knn_waves(d, k4) == 4
    wide = _knn(Yd, k4, blocks=2)
    assert np.array_equal(wide[0][:, :k], idx) and wide[1][:, :k].tobytes() == d2.tobytes()
    for chunk in (64, 100, 699):
        same(_knn(Yd, k, candidate_chunk=chunk), 'candidate_chunk=%d' % chunk)
    same(_knn(Yd, k, candidate_chunk=100, blocks=3), 'candidate_chunk=100, blocks=3')
    for qb in (64, 100, 699):
        same(_knn(Yd, k, query_block=qb), 'query_block=%d' % qb)
    same(_knn(Yd, k, query_block=192, candidate_chunk=300), 'query_block=192, candidate_chunk=300')
    # the candidate chunks merged in reverse order through raw calls
    gi = torch.empty(n, k, dtype=torch.int32, device='cuda')
    gd = torch.empty(n, k, dtype=torch.float32, device='cuda')
    starts = list(range(0, n, 100))[::-1]
    for m, a in enumerate(starts):
        cluster.knn_step(Yd, Yd[a:a + 100], gi, gd, q0=0, y0=a, exclude_self=True, merge=m > 0)
    torch.cuda.synchronize()
    same((gi.cpu().numpy(), gd.cpu().numpy()), 'chunks in reverse order')
    # the queries in two halves with their q0
    for a, b in ((0, 333), (333, n)):
        cluster.knn_step(Yd[a:b], Yd, gi[a:b], gd[a:b], q0=a, y0=0, exclude_self=True)
    torch.cuda.synchronize()
    same((gi.cpu().numpy(), gd.cpu().numpy()), 'queries in two halves')
    # a shifted global numbering shifts the indices and nothing else
    cluster.knn_step(Yd, Yd, gi, gd, q0=1000, y0=1000, exclude_self=True)
    torch.cuda.synchronize()
    same((gi.cpu().numpy() - 1000, gd.cpu().numpy()), 'q0 = y0 = 1000')


def test_a_shorter_last_query_block_that_needs_more_scratch(lib):
    """Two tiles per CU are scanned in one candidate range, one tile fewer in two: the shorter last block of this split needs more
    scratch than the full one (tests/test_knn_host.py), and the result is still the unsplit one bit for bit."""
    from oriana_amd import cluster
    d, k = 4, 3
    full = 2 * int(lib.oriana_device_cus()) * 64
    n = 2 * full - 64
    assert lib.oriana_knn_splits(full, n, d, k, 0) == 1 and lib.oriana_knn_splits(n - full, n, d, k, 0) == 2
    assert lib.oriana_knn_scratch_bytes_for(n - full, n, d, k, 0, 64, d) > lib.oriana_knn_scratch_bytes_for(full, n, d, k, 0, 64, d)
    g = torch.Generator(device='cuda')
    g.manual_seed(5)
    Yd = torch.randn(n, d, generator=g, device='cuda')
    idx, d2 = _knn(Yd, k)
    bi, bd = _knn(Yd, k, query_block=full)
    assert np.array_equal(bi, idx) and bd.tobytes() == d2.tobytes()
    with pytest.raises(ValueError):             # the raw call refuses a scratch sized for the other block
        small = torch.empty(cluster.knn_plan(full, n, d, k, y_ptr=64)[2], dtype=torch.uint8, device='cuda')
        cluster.knn_step(Yd[full:], Yd, torch.empty(n - full, k, dtype=torch.int32, device='cuda'),
                         torch.empty(n - full, k, device='cuda'), q0=full, exclude_self=True, scratch=small)


def test_exact_duplicates():
    n, d, k = 300, 20, 15
    Y, _, _ = kr.blobs(11, n, d, 3)             # rows n - 1 == 0, and n // 2 == 5 == 1
    idx, d2 = _knn(_dev(Y), k)
    assert idx[0, 0] == n - 1 and idx[n - 1, 0] == 0 and d2[0, 0] == 0.0 and d2[n - 1, 0] == 0.0
    # identical candidates in ascending index order, both at distance exactly 0
    assert idx[1, :2].tolist() == [5, n // 2] and idx[5, :2].tolist() == [1, n // 2] and idx[n // 2, :2].tolist() == [1, 5]
    for r in (1, 5, n // 2):
        assert d2[r, 0] == 0.0 and d2[r, 1] == 0.0 and d2[r, 2] > 0.0
    # a row that lists one of a set of identical rows lists them side by side at the same distance, the lower index first
    for i in range(n):
        pos = {int(j): a for a, j in enumerate(idx[i])}
        for lo, hi in ((0, n - 1), (1, 5), (5, n // 2)):
            if hi in pos and i != lo:
                assert lo in pos and pos[lo] < pos[hi] and d2[i, pos[lo]] == d2[i, pos[hi]], (i, lo, hi)
    # the k-th place tied between two identical candidates: the lower index gets it, whichever waves meet the two
    T = np.zeros((40, 3), dtype=np.float32)
    T[:, 0] = 100.0 + np.arange(40)
    T[0] = 0.0
    T[1], T[2] = (1.0, 0.0, 0.0), (0.0, 2.0, 0.0)
    T[4], T[9], T[33] = (0.0, 0.0, 3.0), (0.0, 0.0, 3.0), (0.0, 0.0, 3.0)
    for kk, want in ((3, [1, 2, 4]), (4, [1, 2, 4, 9]), (5, [1, 2, 4, 9, 33])):
        for kw in (dict(), dict(blocks=1), dict(candidate_chunk=8), dict(candidate_chunk=5)):
            ti, td = _knn(_dev(T), kk, **kw)
            assert ti[0].tolist() == want and td[0].tolist() == [1.0, 4.0, 9.0, 9.0, 9.0][:kk], (kk, kw)


def test_separate_queries():
    Y, _ = nr.blobs(31, 200, 20, 4)
    Q = nr.blobs(32, 70, 20, 4)[0]
    Q[3] = Y[7]                                 # a copy of candidate row 7: no exclusion, so it comes first at distance 0
    Q[64] = Y[64]                               # (query 64 and candidate 64 share an index and nothing else is excluded either)
    idx, d2 = _knn(_dev(Y), 15, queries=_dev(Q, 4))
    assert idx[3, 0] == 7 and d2[3, 0] == 0.0 and idx[64, 0] == 64 and d2[64, 0] == 0.0
    share = nr.check(Y, idx, d2, 15, Q=Q, what='separate queries')
    assert share <= nr.NEAR_TIE_CAP
    from oriana_amd import cluster
    same = cluster.knn(_dev(Y), 15, queries=_dev(Q), exclude_self=False, candidate_chunk=33)
    assert np.array_equal(same['indices'].cpu().numpy(), idx) and np.array_equal(same['sq_distances'].cpu().numpy(), d2)
    # the rows themselves without the exclusion: every row is its own first neighbour
    own, od = _knn(_dev(Y), 3, exclude_self=False)
    assert np.array_equal(own[:, 0], np.arange(200)) and np.all(od[:, 0] == 0.0)


def test_errors_before_a_launch(monkeypatch):
    from oriana_amd import cluster
    calls = []
    monkeypatch.setattr(cluster, 'knn_step', lambda *a, **k: calls.append(1) or (_ for _ in ()).throw(AssertionError('launched')))
    Y = torch.randn(50, 100, device='cuda')
    bad = Y.clone()
    bad[7, 3] = float('inf')
    kmax = cluster.max_neighbors(100)
    for args, kw in (((bad, 3), {}), ((Y, 0), {}), ((Y, kmax + 1), {}), ((Y, 3), dict(queries=bad)),
                     ((Y, 3), dict(queries=Y[:5], exclude_self=True)), ((Y.double(), 3), {}), ((Y[0], 3), {}),
                     ((Y, 3), dict(queries=Y[:5].cpu())), ((Y.cpu(), 3), {}), ((Y, 3), dict(queries=Y[:5, :50])),
                     ((Y.t(), 3), {}), ((torch.randn(5, 300, device='cuda'), 3), {})):
        with pytest.raises(ValueError):
            cluster.knn(*args, **kw)
    bad[7, 3] = float('nan')
    with pytest.raises(ValueError):
        cluster.knn(bad, 3)
    assert not calls
