# -*- coding: utf-8 -*-
"""gene_deviance() / cell_deviance() without a GPU: both axes of the float64 reference of tests/axis_deviance_reference.py add
up to the full metric of tests/deviance_path_reference.py, the explained deviance is non-finite at exactly the gene without a
count, and the three new C entries exist and check their arguments before any HIP call."""
import ctypes

import numpy as np
import pytest

import axis_deviance_reference as ar
import deviance_path_reference as dr
from test_deviance_path_gpu import _counts, N_ROWS, M_COLS

ZERO_GENE, ZERO_CELL = 5, 11


def _state(K, zi, seed=0):
    """The counts of the GPU tests and a seeded state: gamma factors, and with a dropout node pi_d in (0.05, 0.95) and a
    random mask over the zeros."""
    X = _counts(K)
    rng = np.random.default_rng(500 + seed)
    n, m = X.shape
    U = rng.gamma(1.0, 0.5, size=(n, K))
    V = rng.gamma(1.0, 0.5, size=(m, K))
    pi = rng.uniform(0.05, 0.95, size=m) if zi else np.ones(m)
    keep0 = (X == 0) & (rng.random((n, m)) < 0.7) if zi else (X == 0)
    return X, U, V, pi, keep0


@pytest.mark.parametrize('zi', [False, True])
@pytest.mark.parametrize('K', [1, 20])
def test_both_axes_add_up_to_the_full_metric(K, zi):
    X, U, V, pi, keep0 = _state(K, zi)
    assert X.shape == (N_ROWS, M_COLS) and not X[:, ZERO_GENE].any() and not X[ZERO_CELL].any()
    ref = ar.axes(X, U, V, pi, keep0, zi)
    ll_uv, ed, rd = dr.full_metric(X, U, V, pi, keep0)
    c = dr.constants(X, pi)
    P = np.broadcast_to(pi[np.newaxis, :], X.shape)
    Lam, N = U @ V.T, X != 0
    a_uv = float(np.abs(dr._log_zero_term(Lam, P)[keep0]).sum() + Lam[N].sum() + np.abs(X[N] * np.log(Lam[N])).sum()
                 + c['abs_lpi'])
    for axis in ('genes', 'cells'):
        r = ref[axis]
        assert r['factors'].shape == ((M_COLS,) if axis == 'genes' else (N_ROWS,))
        for q, whole, scale in (('factors', ll_uv, a_uv), ('counts', c['ll_x'], c['abs_xlx'] + c['abs_lpi']),
                                ('mean', c['ll_mean'], c['abs_mean'])):
            got = float(np.sum(r[q], dtype=np.longdouble))
            print('%s %s: axis sum %.17g whole %.17g (bound %.3e)' % (axis, q, got, whole, ar.ACC * scale))
            assert abs(got - whole) <= ar.ACC * scale
        assert all((r['tol'][q] >= r['tol_acc'][q]).all() and (r['tol_acc'][q] >= 0).all() for q in ar.KEYS)


@pytest.mark.parametrize('zi', [False, True])
def test_explained_deviance_is_not_finite_at_the_gene_without_counts_only(zi):
    """A gene without a count has counts_j = mean_j = 0: the literal float64 quotient is (factors_j - 0) / (0 - 0).  That is
    -inf while the gene's zero term is negative (any state whose rate for the gene is positive), and 0 / 0 = NaN once the rate
    is 0 as well -- both are checked.  Every other gene and every cell, the one without a count included, is finite."""
    K = 20
    X, U, V, pi, keep0 = _state(K, zi, seed=1)
    ref = ar.axes(X, U, V, pi, keep0, zi)
    ed = ref['genes']['explained_deviance']
    assert ref['genes']['counts'][ZERO_GENE] == 0 and ref['genes']['mean'][ZERO_GENE] == 0
    assert ed[ZERO_GENE] == -np.inf and ref['genes']['reconstruction_deviance'][ZERO_GENE] > 0
    assert np.array_equal(np.nonzero(~np.isfinite(ed))[0], [ZERO_GENE])
    assert np.all(np.isfinite(ref['cells']['explained_deviance']))
    assert ref['cells']['counts'][ZERO_CELL] == 0 and ref['cells']['mean'][ZERO_CELL] < 0
    if zi:
        keep0[:, ZERO_GENE] = False                          # every zero of the gene in the mask M: its zero term is 0
    else:
        V[ZERO_GENE] = 0.0                                   # the gene's rate is 0
    ref = ar.axes(X, U, V, pi, keep0, zi)
    ed = ref['genes']['explained_deviance']
    assert np.array_equal(np.nonzero(np.isnan(ed))[0], [ZERO_GENE]), 'NaN at exactly the all-zero gene'
    assert np.array_equal(np.nonzero(~np.isfinite(ed))[0], [ZERO_GENE])
    assert np.all(np.isfinite(ref['cells']['explained_deviance']))
    assert ar.diff(ed, ed).max() == 0 and ar.diff([np.nan, -np.inf, 1.0], [np.nan, -np.inf, 3.0]).tolist() == [0, 0, 2]


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
    for name in ('oriana_metric_nnz_axes', 'oriana_dense_metric_axes', 'oriana_dropout_metric_axes'):
        assert hasattr(lib, name), name
    f = lib.oriana_metric_nnz_axes
    f.restype, f.argtypes = ctypes.c_int, [ctypes.POINTER(OrianaCounts), P, P, P, I, P, P, P, P]
    empty = ctypes.byref(OrianaCounts())                     # zero-initialised: no rows, no tiles
    assert f(None, p, p, p, 3, p, p, p, None) == EINVAL      # no layout
    for miss in (1, 2, 3):
        args = [empty, p, p, p, 3, p, p, p, None]
        args[miss] = None
        assert f(*args) == EINVAL, miss                      # a missing pointer
    assert f(empty, p, p, p, 0, p, p, p, None) == EINVAL     # K <= 0
    assert f(empty, p, p, p, -2, p, p, p, None) == EINVAL
    assert f(empty, p, p, p, 3, p, None, None, None) == EINVAL           # no axis asked for
    assert f(empty, p, p, p, 3, None, None, p, None) == EINVAL           # the cell side needs the per-gene constants
    assert f(empty, p, p, p, 257, p, p, p, None) == EKRANGE              # no row pass above K = 256
    assert f(empty, p, p, p, 3, None, p, None, None) == 0                # an empty layout is fine; one axis alone is
    assert f(empty, p, p, p, 3, p, None, p, None) == 0
    g = lib.oriana_dense_metric_axes
    g.restype, g.argtypes = ctypes.c_int, [ctypes.POINTER(OrianaDense), P, P, P, P, I, P, P, P, P]
    none = ctypes.byref(OrianaDense(0, 0, 0, None))          # a layout without dense genes
    assert g(None, p, p, p, p, 3, p, p, p, None) == EINVAL
    assert g(ctypes.byref(OrianaDense(64, 31, 8, p)), p, p, p, p, 3, p, p, p, None) == EINVAL     # gd not a multiple of 32
    for miss in (1, 2):
        args = [none, p, p, p, p, 3, p, p, p, None]
        args[miss] = None
        assert g(*args) == EINVAL, miss
    assert g(none, p, p, p, p, 0, p, p, p, None) == EINVAL
    assert g(none, p, p, p, p, 1025, p, p, p, None) == EINVAL
    assert g(none, p, p, p, p, 3, p, None, None, None) == EINVAL
    assert g(none, p, p, p, p, 3, None, None, p, None) == EINVAL
    assert g(none, p, p, None, None, 3, p, p, p, None) == 0              # (the orderings are optional: identity)
    h = lib.oriana_dropout_metric_axes
    h.restype, h.argtypes = ctypes.c_int, [P, P, P, P, P, P, P, I, I, I, P]
    assert h(p, p, p, p, p, p, p, -1, 4, 3, None) == EINVAL
    assert h(p, p, p, p, p, p, p, 4, -1, 3, None) == EINVAL
    assert h(p, p, p, p, p, p, p, 4, 4, 0, None) == EINVAL               # K <= 0
    assert h(p, p, p, p, p, p, p, 4, 4, 257, None) == EKRANGE            # K > 256
    assert h(None, None, p, p, p, p, p, 4, 4, 3, None) == EINVAL         # no axis asked for
    for miss in (2, 3, 4, 5, 6):
        args = [p, p, p, p, p, p, p, 4, 4, 3, None]
        args[miss] = None
        assert h(*args) == EINVAL, miss
    assert h(p, None, p, p, p, p, p, 0, 4, 3, None) == 0                 # no rows: nothing to do
    assert h(None, p, p, p, p, p, p, 4, 0, 3, None) == 0
    assert not any(buf), 'a refused or empty call wrote its output'
