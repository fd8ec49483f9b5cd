# -*- coding: utf-8 -*-
"""The host side of score_genes() (oriana_amd/signatures.py, NumPy only) and the reference's bound: no GPU."""
import numpy as np
import pytest

from oriana_amd import signatures as sg
import gene_score_reference as gr

M = 40
# ten genes without expression (a ten-fold tie), thirty with distinct means in a shuffled order
MEANS = np.zeros(M)
MEANS[10:] = np.random.default_rng(0).permutation(np.arange(1, 31)) * 0.25
N_BINS = 5                                                       # n_items = round(40 / 4) = 10


def _brute_bins(means, pool, n_bins):
    n_items = max(1, int(round(len(pool) / (n_bins - 1))))
    return np.array([(1 + sum(1 for l in pool if means[l] < means[j])) // n_items for j in range(len(means))])


BINS = _brute_bins(MEANS, range(M), N_BINS)


def test_ties_share_one_rank_and_one_bin():
    assert (BINS[:10] == 0).all()                                # rank 1 for all ten: 1 // 10 = 0
    assert np.array_equal(sg.expression_bins(MEANS, np.arange(M), np.arange(M), N_BINS), BINS)
    # the expressed genes: ranks 11 .. 40 -> bins 1 (9 genes), 2 (10), 3 (10), 4 (1)
    assert [int((BINS == b).sum()) for b in range(5)] == [10, 9, 10, 10, 1]
    # a tie among expressed genes shares the lowest rank too
    means = MEANS.copy()
    lo, hi = np.argsort(means)[[18, 19]]                         # ranks 19 | 20: the edge between bins 1 and 2
    means[hi] = means[lo]
    bins = sg.expression_bins(means, np.arange(M), np.arange(M), N_BINS)
    assert bins[hi] == bins[lo] == 1 and np.array_equal(bins, _brute_bins(means, range(M), N_BINS))


def test_controls_come_from_the_bins_of_the_set_and_exclude_it():
    in2 = np.flatnonzero(BINS == 2)
    gene_set = np.array([0, 1, in2[0]])
    ctrl = sg.control_genes(MEANS, gene_set, ctrl_size=3, n_bins=N_BINS, seed=4)
    assert ctrl.dtype == np.int64 and np.array_equal(ctrl, np.unique(ctrl))
    assert not set(ctrl.tolist()) & set(gene_set.tolist())
    assert set(BINS[ctrl].tolist()) == {0, 2}                    # only the bins the set occupies
    assert (BINS[ctrl] == 0).sum() == 3 and (BINS[ctrl] == 2).sum() == 3      # ctrl_size per bin (8 and 9 candidates)
    # a ctrl_size above what a bin holds takes the whole bin, without the set's genes
    big = sg.control_genes(MEANS, gene_set, ctrl_size=50, n_bins=N_BINS)
    assert set(big.tolist()) == (set(np.flatnonzero((BINS == 0) | (BINS == 2)).tolist()) - set(gene_set.tolist()))
    # a pool: ranks and draws are the pool's
    pool = np.arange(0, M, 2)
    pb = _brute_bins(MEANS, pool, N_BINS)
    c = sg.control_genes(MEANS, [0, 12], ctrl_size=2, n_bins=N_BINS, pool=pool)
    assert set(c.tolist()) <= set(pool.tolist()) - {0, 12} and set(pb[c].tolist()) <= {int(pb[0]), int(pb[12])}


def test_the_draw_is_seeded_per_set():
    gene_set = [0, 1, int(np.flatnonzero(BINS == 3)[0])]
    kw = dict(ctrl_size=3, n_bins=N_BINS)
    a = sg.control_genes(MEANS, gene_set, seed=7, set_index=0, **kw)
    assert np.array_equal(a, sg.control_genes(MEANS, gene_set, seed=7, set_index=0, **kw))
    draws = [tuple(sg.control_genes(MEANS, gene_set, seed=7, set_index=s, **kw).tolist()) for s in range(8)]
    assert len(set(draws)) > 1                                   # (C(8, 3) C(9, 3) lists: eight equal draws do not happen)
    assert len({tuple(sg.control_genes(MEANS, gene_set, seed=s, **kw).tolist()) for s in range(8)}) > 1
    # a second set, drawn in between, leaves the first set's controls alone: the generator belongs to (seed, set_index)
    sg.control_genes(MEANS, [5, 30], seed=7, set_index=1, **kw)
    assert np.array_equal(a, sg.control_genes(MEANS, gene_set, seed=7, set_index=0, **kw))


def test_score_weights_columns():
    sets = [np.array([0, 1, 20]), np.array([5, 30, 31, 32])]
    ctrls = [sg.control_genes(MEANS, g, ctrl_size=3, n_bins=N_BINS, set_index=s) for s, g in enumerate(sets)]
    W = sg.score_weights(M, sets, ctrls)
    assert W.shape == (M, 2) and W.dtype == np.float64
    for s in range(2):
        col = W[:, s]
        assert len(np.unique(col)) == 3
        assert np.array_equal(np.flatnonzero(col > 0), np.sort(sets[s])) and np.array_equal(np.flatnonzero(col < 0), ctrls[s])
        assert (col[col > 0] == 1.0 / len(sets[s])).all() and (col[col < 0] == -1.0 / len(ctrls[s])).all()
        assert abs(col[col > 0].sum() - 1.0) <= 4 * gr.U * len(sets[s]) and abs(col[col < 0].sum() + 1.0) <= 4 * gr.U * len(ctrls[s])
        assert (col[np.setdiff1d(np.arange(M), np.concatenate([sets[s], ctrls[s]]))] == 0).all()


def test_named_sets():
    names, sets = sg.named_sets(M, {'a': [1, 2], 'b': np.array([3])})
    assert names == ['a', 'b'] and [s.tolist() for s in sets] == [[1, 2], [3]] and all(s.dtype == np.int64 for s in sets)
    names, sets = sg.named_sets(M, [[4, 5], (6,)])
    assert names == [0, 1] and [s.tolist() for s in sets] == [[4, 5], [6]]
    for bad in ([], {}, [1, 2, 3], [[1, 1]], [[M]], [[-1]], [[]], [[0.5]]):
        with pytest.raises(ValueError):
            sg.named_sets(M, bad)


def test_value_errors():
    good = [0, 1, 20]
    for bad in ([], [0, 0], [-1, 2], [M], [[0, 1]], [0.5, 1.0]):
        with pytest.raises(ValueError):
            sg.control_genes(MEANS, bad)
    for kw in ({'ctrl_size': 0}, {'ctrl_size': -3}, {'n_bins': 1}, {'n_bins': 0}, {'ctrl_size': 2.5}, {'pool': []}, {'pool': [M]}):
        with pytest.raises(ValueError):
            sg.control_genes(MEANS, good, **kw)
    with pytest.raises(ValueError):
        sg.control_genes(MEANS.reshape(4, 10), good)
    # an empty control set: the set's bin holds nothing else (the single gene of bin 4; the whole pool)
    with pytest.raises(ValueError):
        sg.control_genes(MEANS, [int(np.flatnonzero(BINS == 4)[0])], n_bins=N_BINS)
    with pytest.raises(ValueError):
        sg.control_genes(MEANS, np.arange(M), n_bins=N_BINS)
    for sets, ctrls in (([[]], [[1]]), ([[0]], [[]]), ([[0]], [[1], [2]]), ([], []), ([[M]], [[1]]), ([[0]], [[-1]]),
                        ([[0, 0]], [[1]]), ([[0]], [[1, 1]])):
        with pytest.raises(ValueError):
            sg.score_weights(M, sets, ctrls)


def test_reference_bound_is_monotone_in_the_stored_counts():
    mag = np.full((6, 2), 3.0)
    c = np.array([0, 1, 2, 50, 300, 30000])
    b = gr.bound(c, mag)
    assert b.shape == (6, 2) and (np.diff(b, axis=0) > 0).all()
    assert np.array_equal(b[:, 0], (2.0 * c + 8.0) * 2.0 ** -53 * 3.0)
    assert (gr.bound(c, np.zeros((6, 2))) == 0).all()            # nothing stored, nothing allowed
    # on a matrix: the reference's scores and bound, an all-zero cell has bound 0 and score 0
    rng = np.random.default_rng(2)
    X = rng.poisson(0.4, size=(30, M)).astype(np.float64)
    X[7] = 0
    W = rng.normal(size=(M, 3))
    ref, bnd = gr.scores(X, W)
    assert ref.shape == bnd.shape == (30, 3) and (ref[7] == 0).all() and (bnd[7] == 0).all()
    live = (X != 0).sum(axis=1) > 0
    assert (bnd[live] > 0).all()
    f64 = gr.mr.transform(X).astype(np.float64) @ W              # a float64 evaluation sits well inside
    assert (np.abs(f64 - ref.astype(np.float64)) <= bnd).all()


def test_the_entry_checks_its_arguments_without_gpu():
    """As test_markers_host: validation comes before any HIP call, and a refused or empty call writes nothing."""
    import ctypes
    import __graft_entry__ as g
    from oriana_amd._lib import OrianaCounts, OrianaDense
    lib = ctypes.CDLL(g.build())
    P, I = ctypes.c_void_p, ctypes.c_int64
    EINVAL, EKRANGE = -1, -2
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    for name in ('oriana_gene_scores_max_sets', 'oriana_gene_scores_set_chunk'):
        getattr(lib, name).restype, getattr(lib, name).argtypes = I, []
    limit, ch = lib.oriana_gene_scores_max_sets(), lib.oriana_gene_scores_set_chunk()
    assert limit >= 256 and ch in (8, 16) and limit >= 2 * ch + 3
    f = lib.oriana_gene_scores
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.POINTER(OrianaCounts), ctypes.POINTER(OrianaDense), P, P, P, ctypes.c_int, P, I, P, P]
    empty = ctypes.byref(OrianaCounts())                         # zero-initialised: no rows, no tiles
    neg = OrianaCounts()
    neg.n = -1
    assert f(None, None, None, None, None, 1, p, 1, p, None) == EINVAL          # no layout
    assert f(empty, None, None, None, None, 1, None, 1, p, None) == EINVAL      # no W
    assert f(empty, None, None, None, None, 1, p, 1, None, None) == EINVAL      # no out
    assert f(empty, None, None, None, None, 1, p, 0, p, None) == EINVAL         # S < 1
    assert f(empty, None, None, None, None, 1, p, -2, p, None) == EINVAL
    assert f(ctypes.byref(neg), None, None, None, None, 1, p, 1, p, None) == EINVAL
    assert f(empty, ctypes.byref(OrianaDense(0, 33, 0, p)), None, None, None, 1, p, 1, p, None) == EINVAL
    assert f(empty, ctypes.byref(OrianaDense(64, 32, 2, p)), None, None, None, 1, p, 1, p, None) == EINVAL
    assert f(empty, None, None, None, None, 1, p, limit + 1, p, None) == EKRANGE
    assert f(empty, None, None, None, p, 0, p, limit, p, None) == 0             # no cells: nothing to write, no launch
    assert f(empty, ctypes.byref(OrianaDense(0, 0, 0, None)), p, p, p, 1, p, 1, p, None) == 0
    assert not any(buf), 'a refused or empty call wrote its output'
