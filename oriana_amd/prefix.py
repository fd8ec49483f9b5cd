# -*- coding: utf-8 -*-
"""Host-side pieces of FactorModel.factor_order() / deviance_path() that need neither a model nor a device: the checks of
the `order` / `ks` arguments, the order by mass and the assembly of the public values from the per-prefix sums."""
import numpy as np

__all__ = ['check_order', 'check_ks', 'order_by_mass', 'assemble_path']


def _int_vector(a, what):
    a = np.asarray(a)
    if a.ndim != 1 or a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or
                                                 (np.issubdtype(a.dtype, np.floating) and np.all(a == np.floor(a)))):
        raise ValueError('%s must be a one-dimensional sequence of integers' % what)
    return a.astype(np.int64)


def check_order(order, K):
    """`order` as an int64 array; ValueError unless it is a permutation of range(K)."""
    o = _int_vector(order, 'order')
    if o.size != K or not np.array_equal(np.sort(o), np.arange(K, dtype=np.int64)):
        raise ValueError('order must be a permutation of range(%d)' % K)
    return o


def check_ks(ks, K):
    """`ks` as an int64 array (None: 1..K); ValueError unless strictly increasing integers within 1..K."""
    if ks is None:
        return np.arange(1, K + 1, dtype=np.int64)
    k = _int_vector(ks, 'ks')
    if k.size == 0 or k[0] < 1 or k[-1] > K or np.any(np.diff(k) <= 0):
        raise ValueError('ks must be strictly increasing integers within 1..%d' % K)
    return k


def order_by_mass(su, sv):
    """The factors by decreasing mass (sum_i U_ik)(sum_j V_jk), ties by index."""
    mass = np.asarray(su, dtype=np.float64) * np.asarray(sv, dtype=np.float64)
    return np.argsort(-mass, kind='stable').astype(np.int64)


def assemble_path(order, ks, ll_uv, ll_x, ll_mean):
    """The dict deviance_path() returns from ll(X | Lambda^(k)) per prefix and the two constants of the full metric."""
    ll_uv = np.asarray(ll_uv, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        ed = (ll_uv - ll_mean) / (ll_x - ll_mean)
        rd = -2.0 * (ll_uv - ll_x)
    return {'order': np.asarray(order, dtype=np.int64), 'k': np.asarray(ks, dtype=np.int64), 'explained_deviance': ed,
            'reconstruction_deviance': rd}
