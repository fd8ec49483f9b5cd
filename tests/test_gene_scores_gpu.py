# -*- coding: utf-8 -*-
"""gene_scores() / score_genes() of every model on both layouts against the NumPy reference of tests/gene_score_reference.py on
the dense X.  With raw integer counts and integer weights every partial sum is an integer below 2^53, so those results are
compared bit for bit; the transformed ones are held to the bound derived in the reference module, never measured on the code
under test, for every cell."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import gene_score_reference as gr
from helpers import guarded_out
from test_deviance_path_gpu import _counts, _model, _free_port, N_ROWS, M_COLS, DENSE_DENSITY, ALL_MODELS

pytestmark = pytest.mark.gpu

K = 4                                  # (the scores do not depend on the factors)
ZERO_GENE, ZERO_CELL = 5, 11
TALL_ROWS = 16 * 256 + 5               # 17 row blocks, the last with 5 rows; 129 cell tiles of the dense block, the last with 5 cells
RAW = dict(normalize=False, log1p=False)
CASES = [(name, None) for name in ALL_MODELS] + [(name, DENSE_DENSITY) for name in ('GaP', 'SparseZIGaP')]
CASE_IDS = ['%s-%s' % (n, 'hybrid' if dd else 'sliced') for n, dd in CASES]
LAYOUTS = pytest.mark.parametrize('dd', [None, DENSE_DENSITY], ids=['sliced', 'hybrid'])
EINVAL, EKRANGE = -1, -2

_cache = {}


def _lib():
    from oriana_amd import _lib as L
    return L.load()


def _ch():
    return int(_lib().oriana_gene_scores_set_chunk())


def _X():
    if 'X' not in _cache:
        _cache['X'] = _counts(3)
        assert _cache['X'].shape == (N_ROWS, M_COLS) == (805, 301)
    return _cache['X']


def _G(name, dd):
    """One model per (class, layout) for the whole module: the calls under test write nothing."""
    key = (name, dd)
    if key not in _cache:
        _cache[key] = _model(name, _X(), K, dense_density=dd)
    return _cache[key]


def _int_weights(m, S, seed=0):
    """Integers from [-3, 3]; from S = 2 on the last column is 0 on every expressed gene (its only weight sits on the all-zero
    gene)."""
    W = np.random.default_rng(100 * S + seed).integers(-3, 4, size=(m, S)).astype(np.float64)
    if S >= 2:
        W[:, -1] = 0.0
        W[ZERO_GENE, -1] = 3.0
    return W


def _assert_exact(got, X, W, what):
    ref = X @ W                                                   # (integers below 2^53: exact in any order)
    assert got.dtype == np.float64 and got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, '%s: %d entries differ, first (cell, set) %s: %r != %r' % (
        what, len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


def _assert_within(got, X, W, what, **kw):
    ref, bnd = gr.scores(X, W, **kw)
    assert got.dtype == np.float64 and got.shape == ref.shape and not np.isnan(got).any(), what
    diff = np.abs(got.astype(gr.LD) - ref).astype(np.float64)
    empty = (X != 0).sum(axis=1) == 0
    assert (got[empty] == 0).all() and not np.signbit(got[empty]).any(), what
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(bnd > 0, diff / bnd, np.where(diff == 0, 0.0, np.inf))
    print('%s: largest diff / bound = %.3g' % (what, ratio.max()))
    assert (diff <= bnd).all(), '%s: %d of %d entries beyond the bound, the worst at %.3g of it' % (
        what, int((diff > bnd).sum()), diff.size, ratio.max())
    return float(ratio.max())


# ---- 1: exact -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,dd', CASES, ids=CASE_IDS)
def test_raw_scores_with_integer_weights_are_exact(name, dd):
    X, G, ch = _X(), _G(name, dd), _ch()
    for S in (1, 2, ch - 1, ch, ch + 1, 2 * ch + 3):
        W = _int_weights(M_COLS, S)
        got = G.gene_scores(W, **RAW)
        _assert_exact(got, X, W, '%s S=%d' % (name, S))
        assert (got[ZERO_CELL] == 0).all() and not np.signbit(got[ZERO_CELL]).any()
        if S >= 2:
            assert (got[:, -1] == 0).all() and (got[:, :-1] != 0).any()
    W = _int_weights(M_COLS, 3)
    one = G.gene_scores(W[:, 0], **RAW)                           # the 1-D form
    assert one.shape == (N_ROWS, 1)
    _assert_exact(one, X, W[:, :1], '%s 1-D' % name)
    t = G.gene_scores(torch.as_tensor(W, device=G.device), as_tensor=True, **RAW)
    assert isinstance(t, torch.Tensor) and t.device == G.device and t.dtype == torch.float64
    _assert_exact(t.cpu().numpy(), X, W, '%s tensor' % name)


# ---- 2: counts beyond uint16 --------------------------------------------------------------------------------------------------

def test_counts_beyond_uint16_stay_exact():
    X = _X().copy()
    X[3, 10] = 70000.0
    X[700, 20] = 2.0 ** 24 - 1
    G = _model('GaP', X, K, dense_density=DENSE_DENSITY)
    dense_genes = G.counts.col_perm.cpu().numpy()[:G.counts.gd]
    assert 10 not in dense_genes and 20 not in dense_genes and 30 in dense_genes
    W = _int_weights(M_COLS, _ch() + 1)
    W[10, 0], W[20, 0] = 3.0, -3.0
    got = G.gene_scores(W, **RAW)
    assert np.abs(got).max() >= 3 * (2.0 ** 24 - 1) - 3 * 301 * 100
    _assert_exact(got, X, W, 'big counts')


# ---- 3, 4: tall and wide ------------------------------------------------------------------------------------------------------

@LAYOUTS
def test_taller_matrix_crosses_many_row_blocks(dd):
    X = _counts(8, n=TALL_ROWS)
    G = _model('GaP', X, K, dense_density=dd)
    for S in (2, _ch() + 1):
        W = _int_weights(M_COLS, S)
        _assert_exact(G.gene_scores(W, **RAW), X, W, 'tall S=%d' % S)


def test_wider_matrix_walks_five_column_tiles_in_one_work_group():
    m = 4 * 256 + 76
    X = _counts(9, n=300, m=m)
    G = _model('GaP', X, K)
    assert G.counts.ncb == 5 and G.counts.nrb == 2
    for S in (1, _ch() + 1):
        W = _int_weights(m, S)
        _assert_exact(G.gene_scores(W, **RAW), X, W, 'wide S=%d' % S)


# ---- 5: a layout with its own cell order --------------------------------------------------------------------------------------

@LAYOUTS
def test_a_layout_with_its_own_cell_order_is_read_through_row_perm(dd):
    import oriana_amd.models as M
    from oriana_amd import engine
    X = _X()
    dev = torch.device('cuda', torch.cuda.current_device())
    counts = engine.CountTiles.from_dense(X, dev, sort_rows=True, dense_density=dd)
    assert counts.row_perm is not None and not np.array_equal(counts.row_perm.cpu().numpy(), np.arange(N_ROWS))
    assert (counts.gd > 0) == bool(dd)
    rng = np.random.default_rng(1)
    G = M.GaP(counts, k=K, init=(rng.gamma(1.0, 1.0, size=(N_ROWS, K)), rng.gamma(1.0, 1.0, size=(M_COLS, K))))
    W = _int_weights(M_COLS, _ch() + 1)
    _assert_exact(G.gene_scores(W, **RAW), X, W, 'sort_rows')
    Wr = np.random.default_rng(6).normal(size=(M_COLS, 3))
    _assert_within(G.gene_scores(Wr), X, Wr, 'sort_rows transformed')


# ---- 6: the transformed scores ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,dd', [('GaP', None), ('GaP', DENSE_DENSITY), ('SparseZIGaP', DENSE_DENSITY), ('ZIGaP', None)],
                         ids=['GaP-sliced', 'GaP-hybrid', 'SparseZIGaP-hybrid', 'ZIGaP-sliced'])
def test_transformed_scores_within_the_derived_bound(name, dd):
    """The defaults (normalised to 1e4, log1p), real weights N(0, 1), S = chunk + 1: every cell within (2 c_i + 8) u sum_j |W| y
    (gene_score_reference), and the same call twice returns identical bits.  Measured on the MI355X: at most 0.0058 of the bound at
    the defaults, 0.0086 over the other modes."""
    X, G = _X(), _G(name, dd)
    S = _ch() + 1
    W = np.random.default_rng(77).normal(size=(M_COLS, S))
    got = G.gene_scores(W)
    _assert_within(got, X, W, '%s S=%d' % (name, S))
    again = G.gene_scores(W)
    assert again.tobytes() == got.tobytes()
    for kw in (dict(log1p=False), dict(normalize=False), dict(target_sum=1e6)):
        _assert_within(G.gene_scores(W[:, :2], **kw), X, W[:, :2], '%s %s' % (name, kw), **kw)


# ---- 7, 8: the entry itself ---------------------------------------------------------------------------------------------------

def _entry(G, W, out, S, scale=None, lg=0):
    from oriana_amd._lib import ptr, stream_ptr
    ct = G.counts
    rc = _lib().oriana_gene_scores(ct.sparse_struct, ct.dense.c_struct if ct.dense is not None else None, ptr(ct.row_perm),
                                   ptr(ct.col_perm), ptr(scale), lg, ptr(W), S, ptr(out), stream_ptr())
    torch.cuda.synchronize()
    return rc


@LAYOUTS
def test_out_is_written_not_added_to_and_nothing_else_is_touched(dd):
    X, G = _X(), _G('GaP', dd)
    for S in (1, _ch() + 1):
        W = _int_weights(M_COLS, S)
        Wd = torch.as_tensor(W, device=G.device)
        out, check = guarded_out((N_ROWS, S), torch.float64, 'nan')
        assert bool(torch.isnan(out).all())
        assert _entry(G, Wd, out, S) == 0
        check('gene_scores S=%d' % S)
        _assert_exact(out.cpu().numpy(), X, W, 'guarded S=%d' % S)
        # W and out on an 8-byte but not 16-byte boundary
        wbuf = torch.zeros(M_COLS * S + 1, dtype=torch.float64, device=G.device)
        obuf = torch.full((N_ROWS * S + 2,), float('nan'), dtype=torch.float64, device=G.device)
        w8, o8 = wbuf[1:].view(M_COLS, S), obuf[1:-1].view(N_ROWS, S)
        w8.copy_(Wd)
        assert w8.data_ptr() % 16 == 8 and o8.data_ptr() % 16 == 8
        assert _entry(G, w8, o8, S) == 0
        _assert_exact(o8.cpu().numpy(), X, W, 'odd alignment S=%d' % S)
        assert bool(torch.isnan(obuf[0])) and bool(torch.isnan(obuf[-1]))


def test_entry_return_codes_leave_out_alone():
    G = _G('GaP', DENSE_DENSITY)
    limit = int(_lib().oriana_gene_scores_max_sets())
    assert limit >= 256
    Wd = torch.ones(M_COLS * 2, dtype=torch.float64, device=G.device)
    out, check = guarded_out((N_ROWS, 2), torch.float64, 'nan')
    assert _entry(G, None, out, 2) == EINVAL
    assert _entry(G, Wd, None, 2) == EINVAL
    assert _entry(G, Wd, out, 0) == EINVAL
    assert _entry(G, Wd, out, -1) == EINVAL
    assert _entry(G, Wd, out, limit + 1) == EKRANGE
    assert bool(torch.isnan(out).all())
    check('refused calls')


# ---- 9: score_genes() ---------------------------------------------------------------------------------------------------------

PLANTED = np.arange(100, 120)
OTHERS = np.arange(200, 215)
PLANTED_ROWS = slice(100, 300)
DRAW = dict(ctrl_size=10, n_bins=6)


def _planted_X():
    """_counts(3) with the counts of the 20 genes PLANTED multiplied by 6 in the rows 100 .. 299.  Left at the 15 % density
    _counts() gives them, the longdouble reference itself does not separate the rows (196 of the 200 planted rows score below
    the best other row: a planted row expresses three of the twenty genes on average and some none, and log1p(6 a) - log1p(a)
    is 1.8 per expressed gene) -- as in test_markers_gpu.test_planted_markers_come_out_on_top a factor only shows in a gene that
    is expressed.  So the genes 100 .. 169 are first given a count in every cell (Poisson(30) + 1): the planted 20 and fifty
    more, which fill the expression bins the set falls into, so that its controls are expressed everywhere too (with controls
    from the genes at 80 % density the reference still leaves 135 planted rows below the best other row).  On this input the
    reference's lowest planted row scores 1.59 and its highest other row 0.19."""
    if 'planted' not in _cache:
        X = _X().copy()
        X[:, 100:170] = np.random.default_rng(5).poisson(30.0, size=(N_ROWS, 70)) + 1
        X[ZERO_CELL, :] = 0
        X[PLANTED_ROWS, PLANTED] *= 6
        _cache['planted'] = X
    return _cache['planted']


def _bins_are_safe(mean, b, n_bins):
    """No gene can change its bin while every mean moves by at most its bound: the lowest and the highest rank a gene can take
    (the others at the far ends of their intervals) fall into the bin of the reference."""
    from oriana_amd import signatures
    m = len(mean)
    n_items = max(1, int(round(m / (n_bins - 1))))
    lo, hi = mean - b, mean + b
    bins = signatures.expression_bins(mean, np.arange(m), np.arange(m), n_bins)
    r_lo = 1 + np.array([(hi < lo[j]).sum() for j in range(m)])
    r_hi = 1 + np.array([(lo < hi[j]).sum() - (1 if lo[j] < hi[j] else 0) for j in range(m)])
    return bool(((r_lo // n_items == bins) & (r_hi // n_items == bins)).all())


def _planted_reference():
    """(controls from the reference's gene means, the weights, reference scores, bound): computed once."""
    from oriana_amd import signatures
    if 'planted_ref' not in _cache:
        X = _planted_X()
        mean, b = gr.gene_means(X)
        mean = mean.astype(np.float64)
        assert _bins_are_safe(mean, b, DRAW['n_bins']),'a gene mean lies within its bound of a bin edge'
        ctrl = [signatures.control_genes(mean, g, seed=0, set_index=s, **DRAW) for s, g in enumerate((PLANTED, OTHERS))]
        W = signatures.score_weights(M_COLS, [PLANTED, OTHERS], ctrl)
        ref, bnd = gr.scores(X, W)
        # the premise, on the reference: every planted row above every other row that holds a count
        s0 = ref[:, 0].astype(np.float64)
        rest = np.ones(N_ROWS, dtype=bool)
        rest[PLANTED_ROWS] = False
        rest &= (X != 0).sum(axis=1) > 0
        assert s0[PLANTED_ROWS].min() > s0[rest].max() + 1.0, (s0[PLANTED_ROWS].min(), s0[rest].max())
        _cache['planted_ref'] = (mean, ctrl, W, ref, bnd, rest)
    return _cache['planted_ref']


@LAYOUTS
def test_score_genes_finds_the_planted_rows(dd):
    X = _planted_X()
    mean, ctrl, W, ref, bnd, rest = _planted_reference()
    G = _model('GaP', X, K, dense_density=dd)
    got = G.score_genes({'planted': PLANTED, 'others': OTHERS}, **DRAW)
    assert got['names'] == ['planted', 'others'] and got['scores'].shape == (N_ROWS, 2)
    assert len(got['control_genes']) == 2 and all(c.dtype == np.int64 for c in got['control_genes'])
    assert all(np.array_equal(c, r) for c, r in zip(got['control_genes'], ctrl)), 'the controls of the reference means'
    assert not set(got['control_genes'][0].tolist()) & set(PLANTED.tolist())
    mb = gr.gene_means(X)[1]
    assert got['gene_means'].shape == (M_COLS,) and (np.abs(got['gene_means'] - mean) <= mb + gr.U * mean).all()
    assert np.array_equal(got['weights'], W)
    diff = np.abs(got['scores'].astype(gr.LD) - ref).astype(np.float64)
    assert (diff <= bnd).all() and (got['scores'][ZERO_CELL] == 0).all()
    s0 = got['scores'][:, 0]
    assert s0[PLANTED_ROWS].min() > s0[rest].max()
    # the lists of a result, passed back: the same bits, and no means are computed
    import oriana_amd.models.base as base
    calls, real = [], base.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    base.call = spy
    try:
        back = G.score_genes([PLANTED, OTHERS], control_genes=got['control_genes'])
    finally:
        base.call = real
    assert calls == ['oriana_gene_scores'], calls
    assert back['scores'].tobytes() == got['scores'].tobytes() and back['gene_means'] is None and back['names'] == [0, 1]
    assert np.array_equal(back['weights'], W)


# ---- 10: shards ---------------------------------------------------------------------------------------------------------------

@LAYOUTS
def test_row_shards_score_against_the_same_controls(dd):
    X = _planted_X()
    mean, ctrl, W, ref, bnd, rest = _planted_reference()
    for rows in (slice(0, 400), slice(400, N_ROWS)):
        G = _model('GaP', X[rows], K, dense_density=dd)
        got = G.score_genes([PLANTED, OTHERS], control_genes=ctrl)
        assert got['scores'].shape == (X[rows].shape[0], 2)
        diff = np.abs(got['scores'].astype(gr.LD) - ref[rows]).astype(np.float64)
        assert (diff <= bnd[rows]).all(), rows


def _worker(rank, port, X, W, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['ORIANA_FORCE_SHARDED'] = '1'            # (before construction: the collectives of a one-rank group are issued)
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        from oriana_amd import dist as odist, engine
        import oriana_amd.models as M
        dev = torch.device('cuda', 0)
        rng = np.random.default_rng(1000)
        a1 = rng.gamma(1.0, 1.0, size=(X.shape[0], K)); b1 = rng.gamma(1.0, 1.0, size=(X.shape[1], K))
        counts = engine.CountTiles.from_dense(X, dev, reduce_fn=lambda t: odist.all_reduce_sum(t), n_total=X.shape[0])
        G = M.GaP(counts, k=K, init=(a1, b1), device=dev, process_group=dist.group.WORLD)
        assert G.sharded
        sg = G.score_genes([PLANTED, OTHERS], **DRAW)
        np.savez(out, raw=G.gene_scores(W, **RAW), transformed=G.gene_scores(W), scores=sg['scores'], weights=sg['weights'],
                 gene_means=sg['gene_means'], ctrl0=sg['control_genes'][0], ctrl1=sg['control_genes'][1])
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    # (as tests/test_sharded_gpu.py: leave without the static destructors of the interpreter / c10d)
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(0)


def test_one_rank_process_group_gives_the_same_arrays(tmp_path):
    """Under a one-rank process group with ORIANA_FORCE_SHARDED=1 (a fresh child process) the scores are the plain model's bit
    for bit: a cell's score is local and its summation order fixed.  The gene means go through the all-reduce and the float64
    atomics of cluster_gene_stats(), so they agree within twice their bound; the controls drawn from them are the same."""
    X = _planted_X()
    mean, ctrl, Wref, ref, bnd, rest = _planted_reference()
    W = _int_weights(M_COLS, _ch() + 1)
    out = str(tmp_path / 'gene_scores_sharded.npz')
    mp.spawn(_worker, args=(_free_port(), X, W, out), nprocs=1, join=True)
    got = np.load(out)
    G = _model('GaP', X, K)
    _assert_exact(got['raw'], X, W, 'one-rank group')
    assert got['transformed'].tobytes() == G.gene_scores(W).tobytes()
    one = G.score_genes([PLANTED, OTHERS], **DRAW)
    assert np.array_equal(got['ctrl0'], ctrl[0]) and np.array_equal(got['ctrl1'], ctrl[1])
    assert np.array_equal(got['weights'], one['weights']) and got['scores'].tobytes() == one['scores'].tobytes()
    assert (np.abs(got['gene_means'] - one['gene_means']) <= 2 * gr.gene_means(X)[1]).all()


# ---- 11: state and validation -------------------------------------------------------------------------------------------------

def test_state_is_left_alone():
    X = _X()
    G = _model('SparseZIGaP', X, K)
    G.fit(1)
    torch.cuda.synchronize()
    before = {k: np.array(v, copy=True) for k, v in G.state().items()}
    G.gene_scores(_int_weights(M_COLS, 3))
    G.score_genes([PLANTED, OTHERS], **DRAW)
    after = G.state()
    assert sorted(before) == sorted(after)
    for k in before:
        assert before[k].tobytes() == np.asarray(after[k]).tobytes(), k


def test_value_errors_come_before_any_launch():
    G = _G('GaP', None)
    limit = int(_lib().oriana_gene_scores_max_sets())
    good = _int_weights(M_COLS, 3)
    import oriana_amd.models.base as base
    calls, real = [], base.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    base.call = spy
    try:
        nan, inf = good.copy(), good.copy()
        nan[17, 1] = np.nan
        inf[0, 0] = np.inf
        for args, kw in (((good[:-1],), {}), ((good.T,), {}), ((good.reshape(M_COLS, 3, 1),), {}), ((good[:, :0],), {}),
                         ((nan,), {}), ((inf,), {}), ((torch.as_tensor(nan),), {}), ((np.zeros((M_COLS, limit + 1)),), {}),
                         ((good,), {'target_sum': 0}), ((good,), {'target_sum': -1.0}), ((good[:, 0] != 0,), {}),
                         ((np.float64(1.0),), {})):
            with pytest.raises(ValueError):
                G.gene_scores(*args, **kw)
        sets = [PLANTED, OTHERS]
        for args, kw in ((([],), {}), (([PLANTED, []],), {}), (([[0, 0, 1]],), {}), (([[-1, 2]],), {}), (([[M_COLS]],), {}),
                         (([[0.5, 1.5]],), {}), ((PLANTED,), {}), ((sets,), {'ctrl_size': 0}), ((sets,), {'n_bins': 1}),
                         ((sets,), {'target_sum': 0.0}), ((sets,), {'gene_pool': []}), ((sets,), {'gene_pool': [M_COLS]}),
                         ((sets,), {'control_genes': [[1, 2]]}), ((sets,), {'control_genes': [[1, 2], []]}),
                         ((sets,), {'control_genes': [[1, 2], [3, 3]]}), ((sets,), {'control_genes': [[1, 2], [M_COLS]]}),
                         (([[0]] * (limit + 1),), {})):
            with pytest.raises(ValueError):
                G.score_genes(*args, **kw)
        with pytest.raises(TypeError):
            G.score_genes(sets, labels=3)
        assert calls == [], calls
        # a set whose bins hold no other gene of the pool has no controls: known once the means are
        with pytest.raises(ValueError):
            G.score_genes([[1, 2, 3]], gene_pool=[1, 2, 3], **DRAW)
        assert G.gene_scores(np.ones((M_COLS, limit)), **RAW).shape == (N_ROWS, limit)
    finally:
        base.call = real
