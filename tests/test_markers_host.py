# -*- coding: utf-8 -*-
"""marker_genes() without a GPU: markers.welch_from_moments against the two-pass reference of tests/marker_reference.py within
bounds propagated from the cancellation in s2 - s1^2 / n, its edge cases, markers.rank, and the argument checks of the two new
C entries before any HIP call."""
import ctypes

import numpy as np
import pytest

import marker_reference as mr
from oriana_amd import markers


def _data(seed=0, n=90, m=40, C=3):
    """Seeded counts with genes of every kind: gene 0 all zero, gene 1 the same count in every cell (no variance anywhere),
    gene 2 expressed in cluster 1 only, gene 3 large counts on a small spread (the cancellation case)."""
    rng = np.random.default_rng(seed)
    X = (rng.poisson(rng.gamma(0.8, 3.0, size=(n, m))) * (rng.random((n, m)) < 0.6)).astype(np.float64)
    labels = rng.integers(0, C, size=n)
    X[:, 0] = 0
    X[:, 1] = 3
    X[:, 2] = np.where(labels == 1, rng.poisson(4.0, size=n) + 1, 0)
    X[:, 3] = 50000 + rng.integers(0, 3, size=n)
    return X, labels


def _f64_moments(X, labels, C, **kw):
    cnt, s1, s2, sizes = mr.moments(X, labels, C, **kw)
    return cnt.astype(np.float64), s1.astype(np.float64), s2.astype(np.float64), sizes


@pytest.mark.parametrize('log1p,normalize', [(True, True), (False, False), (True, False)])
def test_welch_from_moments_against_two_pass(log1p, normalize):
    C = 3
    X, labels = _data()
    assert X.shape == (90, 40)
    kw = dict(log1p=log1p, normalize=normalize)
    cnt, s1, s2, sizes = _f64_moments(X, labels, C, **kw)
    ref = mr.welch_two_pass(X, labels, C, **kw)
    got = markers.welch_from_moments(cnt, s1, s2, sizes, log1p=log1p)
    # the float64 moments are the longdouble ones rounded once: within u of them
    bnd = mr.welch_bounds(s1, s2, sizes, mr.U * np.abs(s1), mr.U * np.abs(s2))
    worst = 0.0
    for k in ('scores', 'mean_in', 'mean_out', 'var_in', 'var_out'):
        diff = np.abs(got[k] - ref[k].astype(np.float64))
        b = bnd[k]
        finite = np.isfinite(b)
        assert finite.mean() > 0.9, 'the bound must say something about most genes'
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = np.where(b > 0, diff / b, np.where(diff == 0, 0.0, np.inf))[finite]
        worst = max(worst, float(ratio.max()))
        print('%s: largest diff / bound = %.3g (largest diff %.3g)' % (k, ratio.max(), diff[finite].max()))
        assert (diff[finite] <= b[finite]).all(), k
    print('largest diff / bound over all arrays: %.3g' % worst)
    for k in ('pct_in', 'pct_out'):
        assert np.allclose(got[k], ref[k].astype(np.float64), rtol=4 * mr.U, atol=0)
    # the fold change and df away from the genes the cancellation dominates (gene 3): plain float64 accuracy
    keep = np.ones(X.shape[1], dtype=bool)
    keep[3] = False
    assert np.allclose(got['logfoldchanges'][:, keep], ref['logfoldchanges'].astype(np.float64)[:, keep], rtol=1e-9, atol=1e-9)
    # df = (a + b)^2 / (a^2 / (n_c - 1) + b^2 / (n_r - 1)) with a + b = q: its logarithmic derivatives in a and b are at most
    # (2 + 4 N) / q in magnitude (N = 90 cells), so where the variance is known to eq / q <= 1e-12 df is known to 1e-8 with room
    sure = bnd['eq'] <= 1e-12 * bnd['q']
    assert sure.mean() > 0.8
    assert np.allclose(got['df'][sure], ref['df'].astype(np.float64)[sure], rtol=1e-8, equal_nan=True)


def test_zero_denominator_gives_exactly_zero():
    X, labels = _data()
    cnt, s1, s2, sizes = _f64_moments(X, labels, 3, log1p=False, normalize=False)
    got = markers.welch_from_moments(cnt, s1, s2, sizes, log1p=False)
    for g in (0, 1):                                   # no count at all; the same count everywhere: no variance on either side
        assert (got['scores'][:, g] == 0).all() and not np.signbit(got['scores'][:, g]).any()
        assert np.isnan(got['df'][:, g]).all()
    assert (got['pct_in'][:, 0] == 0).all() and (got['pct_in'][:, 1] == 1).all() and (got['pct_out'][:, 1] == 1).all()
    assert got['pct_in'][1, 2] == 1 and got['pct_out'][1, 2] == 0 and got['pct_in'][0, 2] == 0
    assert got['scores'][1, 2] > 0 > got['scores'][0, 2]
    assert np.isfinite(got['scores']).all() and np.isfinite(got['logfoldchanges']).all()


def test_empty_cluster_rows_are_nan_and_too_few_clusters_raise():
    X, labels = _data()
    labels = np.where(labels == 1, 3, labels)          # ids 0, 2, 3 in use, 1 and 4 empty
    cnt, s1, s2, sizes = _f64_moments(X, labels, 5, log1p=True, normalize=True)
    assert sizes[1] == 0 and sizes[4] == 0
    got = markers.welch_from_moments(cnt, s1, s2, sizes)
    for k, v in got.items():
        assert v.shape == (5, 40)
        assert np.isnan(v[[1, 4]]).all(), k
    assert np.isfinite(got['scores'][[0, 2, 3]]).all()
    one = np.array([0, 7, 0])
    z = np.zeros((3, 4))
    with pytest.raises(ValueError):
        markers.welch_from_moments(z, z, z, one)
    with pytest.raises(ValueError):
        markers.welch_from_moments(z, z, z, np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError):
        markers.welch_from_moments(z, z, z[:2], np.array([1, 2, 3]))
    # a single cell against the rest: variance 0 inside, a defined score, no degrees of freedom
    lab1 = np.zeros(90, dtype=np.int64)
    lab1[17] = 1
    cnt, s1, s2, sizes = _f64_moments(X, lab1, 2)
    got = markers.welch_from_moments(cnt, s1, s2, sizes)
    assert (got['var_in'][1] == 0).all() and np.isfinite(got['scores']).all() and np.isnan(got['df'][1]).all()


def test_rank_ties_and_nan():
    s = np.array([[1.0, np.nan, 3.0, 1.0, -2.0, 3.0, np.nan, 0.0, -0.0],
                  [np.nan] * 9,
                  [0.0] * 9])
    r = markers.rank(s, 20)
    assert r.dtype == np.int64 and r.shape == (3, 9)
    assert r[0].tolist() == [2, 5, 0, 3, 7, 8, 4, 1, 6]
    assert r[1].tolist() == list(range(9)) and r[2].tolist() == list(range(9))
    assert markers.rank(s, 4)[0].tolist() == [2, 5, 0, 3] and markers.rank(s, 0).shape == (3, 0)
    with pytest.raises(ValueError):
        markers.rank(s[0], 3)
    with pytest.raises(ValueError):
        markers.rank(s, -1)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    return ctypes.CDLL(g.build())


def test_new_entries_check_their_arguments_without_gpu(lib):
    """As test_abi.test_argument_errors_without_gpu: validation comes before any HIP call."""
    from oriana_amd._lib import OrianaCounts, OrianaDense
    P, I = ctypes.c_void_p, ctypes.c_int64
    EINVAL, EKRANGE = -1, -2
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    CP, DP = ctypes.POINTER(OrianaCounts), ctypes.POINTER(OrianaDense)
    mg = lib.oriana_group_stats_max_groups
    mg.restype, mg.argtypes = I, []
    limit = mg()
    assert limit >= 256
    empty = ctypes.byref(OrianaCounts())                     # zero-initialised: no rows, no tiles
    none = ctypes.byref(OrianaDense(0, 0, 0, None))          # a layout without dense genes
    neg = OrianaCounts()
    neg.n = -1
    f = lib.oriana_cell_totals
    f.restype, f.argtypes = ctypes.c_int, [CP, DP, P, P, P, P]
    assert f(None, None, None, None, p, None) == EINVAL      # no layout
    assert f(empty, None, None, None, None, None) == EINVAL  # no output
    assert f(ctypes.byref(neg), None, None, None, p, None) == EINVAL
    assert f(empty, ctypes.byref(OrianaDense(0, 31, 0, p)), None, None, p, None) == EINVAL    # gd not a multiple of 32
    assert f(empty, ctypes.byref(OrianaDense(-1, 32, 0, p)), None, None, p, None) == EINVAL
    assert f(empty, ctypes.byref(OrianaDense(64, 32, 2, p)), None, None, p, None) == EINVAL   # the block's cells are not cm's
    assert f(empty, None, None, None, p, None) == 0          # an empty layout is fine, with or without a dense block
    assert f(empty, none, p, p, p, None) == 0
    g = lib.oriana_group_stats
    g.restype, g.argtypes = ctypes.c_int, [CP, DP, P, P, P, P, ctypes.c_int, I, P, P]
    assert g(None, None, None, None, p, None, 1, 3, p, None) == EINVAL
    assert g(empty, None, None, None, None, None, 1, 3, p, None) == EINVAL      # no labels
    assert g(empty, None, None, None, p, None, 1, 3, None, None) == EINVAL      # no output
    assert g(empty, None, None, None, p, None, 1, 0, p, None) == EINVAL         # C < 1
    assert g(empty, None, None, None, p, None, 1, -4, p, None) == EINVAL
    assert g(ctypes.byref(neg), None, None, None, p, None, 1, 3, p, None) == EINVAL
    assert g(empty, ctypes.byref(OrianaDense(0, 33, 0, p)), None, None, p, None, 1, 3, p, None) == EINVAL
    assert g(empty, None, None, None, p, None, 1, limit + 1, p, None) == EKRANGE
    assert g(empty, None, None, None, p, p, 0, limit, p, None) == 0             # the limit itself is served
    assert g(empty, none, p, p, p, None, 1, 1, p, None) == 0
    assert not any(buf), 'a refused or empty call wrote its output'
