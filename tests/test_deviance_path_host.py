# -*- coding: utf-8 -*-
"""The float64 restatement of deviance_path() (tests/deviance_path_reference.py) against the full metric's formulas, and
the checks of the `order` / `ks` arguments (oriana_amd/prefix.py).  No GPU."""
import numpy as np
import pytest

import deviance_path_reference as dr


def _problem(seed, n=67, m=41, K=6, zi=False):
    rng = np.random.default_rng(seed)
    X = (rng.poisson(rng.gamma(0.7, 3.0, size=(n, m))) * (rng.random((n, m)) < 0.4)).astype(np.float64)
    X[:, 3] = 0
    X[5, :] = 0
    U = rng.gamma(1.0, 1.0, size=(n, K))
    V = rng.gamma(1.0, 0.5, size=(m, K))
    if zi:
        pi = rng.uniform(0.2, 0.9, size=m)
        keep0 = (X == 0) & (rng.random((n, m)) < 0.7)
    else:
        pi = np.ones(m)
        keep0 = X == 0
    return X, U, V, pi, keep0


@pytest.mark.parametrize('zi', [False, True])
def test_full_prefix_is_the_full_metric(zi):
    """k = K with the identity order: the per-prefix restatement gives the full-metric formulas on U V^T."""
    X, U, V, pi, keep0 = _problem(1, zi=zi)
    K = U.shape[1]
    ref = dr.path(X, U, V, pi, keep0, np.arange(K), np.arange(1, K + 1), zi)
    ll_uv, ed, rd = dr.full_metric(X, U, V, pi, keep0)
    # (a running sum of K outer products against one matrix product: float64 rounding of K terms per rate)
    rel = 16 * K * 2.0 ** -53
    a = abs(ref['const']['ll_x']) + abs(ref['const']['ll_mean']) + abs(ll_uv)
    assert abs(ref['ll_uv'][-1] - ll_uv) <= rel * a * 10
    assert abs(ref['rd'][-1] - rd) <= 2 * rel * a * 10
    assert abs(ref['ed'][-1] - ed) <= rel * a * 10 / abs(ref['const']['ll_x'] - ref['const']['ll_mean']) * (1 + abs(ed))
    # the path is a path: sum_N Lambda^(k) grows with k, and every value is finite on strictly positive factors
    assert np.all(np.diff(ref['lam']) > 0) and all(np.all(np.isfinite(ref[q])) for q in ('ll_uv', 'ed', 'rd'))
    # the float32 evaluation stays within the derived bound of the float64 one (the bound is at least F_REF times it)
    for q in ('lam', 'xlog', 'll_uv', 'ed', 'rd'):
        assert np.all(dr.diff(ref['f32'][q], ref[q]) <= ref['tol'][q])


@pytest.mark.parametrize('zi', [False, True])
def test_a_permuted_order_ends_at_the_same_value(zi):
    """A permuted order with the same prefix set: the same value at k = K (and, for a permutation that keeps the first three
    factors as a set, at k = 3); different values before."""
    X, U, V, pi, keep0 = _problem(2, zi=zi)
    K = U.shape[1]
    ks = np.arange(1, K + 1)
    a = dr.path(X, U, V, pi, keep0, np.arange(K), ks, zi)
    b = dr.path(X, U, V, pi, keep0, np.array([2, 0, 1, 5, 4, 3]), ks, zi)
    for q in ('ll_uv', 'ed', 'rd'):
        for t in (2, K - 1):
            assert abs(a[q][t] - b[q][t]) <= 1e-11 * max(abs(a[q][t]), 1.0), (q, t)
        assert abs(a[q][0] - b[q][0]) > 1e-6 * abs(a[q][0]), q


def test_a_planted_zero_prefix_is_minus_infinity_at_exactly_those_k():
    """One gene masked on the first two factors of the order and expressed somewhere: its rate is exactly 0 at a non-zero
    count for k = 1, 2 and positive from k = 3 on."""
    X, U, V, pi, keep0 = _problem(3)
    K = U.shape[1]
    order = np.array([4, 1, 0, 2, 3, 5])
    assert (X[:, 7] != 0).any()
    V[7, order[:2]] = 0.0
    ref = dr.path(X, U, V, pi, keep0, order, np.arange(1, K + 1), False)
    assert np.all(ref['xlog'][:2] == -np.inf) and np.all(ref['ll_uv'][:2] == -np.inf)
    assert np.all(ref['ed'][:2] == -np.inf) and np.all(ref['rd'][:2] == np.inf)
    for q in ('xlog', 'll_uv', 'ed', 'rd', 'lam'):
        assert np.all(np.isfinite(ref[q][2:])), q
    assert np.all(np.isfinite(ref['lam']))
    # ks that skip the masked prefixes see none of it
    sub = dr.path(X, U, V, pi, keep0, order, np.array([3, K]), False)
    assert np.array_equal(sub['ed'], ref['ed'][[2, K - 1]])


def test_order_by_mass_and_argument_checks():
    from oriana_amd import prefix
    su = np.array([1.0, 3.0, 2.0, 3.0])
    sv = np.array([2.0, 1.0, 1.5, 1.0])
    o = prefix.order_by_mass(su, sv)                   # masses 2, 3, 3, 3: ties by index
    assert o.dtype == np.int64 and o.tolist() == [1, 2, 3, 0]
    assert prefix.check_order([2, 0, 1], 3).tolist() == [2, 0, 1] and prefix.check_order(np.arange(4), 4).dtype == np.int64
    for bad in ([0, 1], [0, 1, 1], [0, 1, 3], [-1, 0, 1], [0.5, 1, 2], [[0, 1, 2]], [True, False, True], 'abc'):
        with pytest.raises(ValueError):
            prefix.check_order(bad, 3)
    assert prefix.check_ks(None, 4).tolist() == [1, 2, 3, 4] and prefix.check_ks(None, 4).dtype == np.int64
    assert prefix.check_ks([1, 3], 4).tolist() == [1, 3] and prefix.check_ks([4], 4).tolist() == [4]
    assert prefix.check_ks(np.array([2.0, 4.0]), 4).tolist() == [2, 4]
    for bad in ([], [0, 1], [1, 5], [2, 2], [3, 1], [1.5], [[1, 2]], 'ab'):
        with pytest.raises(ValueError):
            prefix.check_ks(bad, 4)


def test_assemble_path():
    from oriana_amd import prefix
    out = prefix.assemble_path([1, 0], [1, 2], np.array([-np.inf, -30.0]), -10.0, -50.0)
    assert out['order'].dtype == np.int64 and out['k'].dtype == np.int64
    assert out['explained_deviance'][0] == -np.inf and out['reconstruction_deviance'][0] == np.inf
    assert out['explained_deviance'][1] == (-30.0 + 50.0) / (-10.0 + 50.0) and out['reconstruction_deviance'][1] == 40.0
