# -*- coding: utf-8 -*-
"""cell_totals() / cluster_gene_stats() / marker_genes() of every model on both layouts against the NumPy reference of
tests/marker_reference.py on the dense X.  Integer counts make every partial sum of the raw moments exact in float64, so those
are compared bit for bit whatever the order of the atomics; the transformed moments and the statistic are held to the bounds
derived in the reference module, never measured on the code under test."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import marker_reference as mr
from test_deviance_path_gpu import _counts, _model, _free_port, N_ROWS, M_COLS, DENSE_DENSITY, ALL_MODELS

pytestmark = pytest.mark.gpu

K = 4                                  # (the statistics do not depend on the factors)
ZERO_GENE, ZERO_CELL = 5, 11
# 1, 2, 3, 17 and two values above the kernels' cluster chunks: the sliced kernel takes at most 24 clusters per work-group (in
# even chunks: 37 = 19 + 18, 100 = 5 x 20), the dense one 32 (37 = 32 + 5, 100 = 3 x 32 + 4) -- chunk boundaries and a partial
# last chunk are crossed on both
CS = (1, 2, 3, 17, 37, 100)
TALL_ROWS = 16 * 256 + 5               # 17 row blocks: a sliced work-group takes 2 x 4 of them (8, 8, 1: three work-groups per gene
                                       # tile, the last with idle groups), the dense one 32 cell tiles (129 of them: five groups)
RAW = dict(normalize=False, log1p=False)
CASES = [(name, None) for name in ALL_MODELS] + [(name, DENSE_DENSITY) for name in ('GaP', 'SparseZIGaP')]
CASE_IDS = ['%s-%s' % (n, 'hybrid' if dd else 'sliced') for n, dd in CASES]

_cache = {}


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


def _random_labels(C, n=N_ROWS):
    return np.random.default_rng(40 + C).integers(0, C, size=n)


def _blocked_labels():
    """Seven ids in row order: id 3 without cells, id 2 a single cell, boundaries at rows 15/16 and 255/256 and inside the last,
    partial tile (row 790 of 805)."""
    lab = np.empty(N_ROWS, dtype=np.int64)
    lab[:16] = 0
    lab[16:255] = 1
    lab[255] = 2
    lab[256:600] = 4
    lab[600:790] = 5
    lab[790:] = 6
    return lab, 7


def _raw_reference(X, labels, C):
    cnt, s1, s2, sizes = mr.moments(X, labels, C, **RAW)
    return {'n_expressing': cnt.astype(np.float64), 'sum': s1.astype(np.float64), 'sumsq': s2.astype(np.float64), 'sizes': sizes}


def _assert_exact(got, ref, what):
    for k in ('n_expressing', 'sum', 'sumsq'):
        assert got[k].dtype == np.float64 and got[k].shape == ref[k].shape, (what, k)
        bad = np.argwhere(got[k] != ref[k])
        assert bad.size == 0, '%s %s: %d entries differ, first (cluster, gene) %s: %r != %r' % (
            what, k, len(bad), bad[0], got[k][tuple(bad[0])], ref[k][tuple(bad[0])])
    assert got['sizes'].dtype == np.int64 and np.array_equal(got['sizes'], ref['sizes']), what


@pytest.mark.parametrize('name,dd', [(n, dd) for n in ('GaP', 'SparseZIGaP') for dd in (None, DENSE_DENSITY)],
                         ids=['%s-%s' % (n, l) for n in ('GaP', 'SparseZIGaP') for l in ('sliced', 'hybrid')])
def test_cell_totals_equal_the_row_sums(name, dd):
    X, G = _X(), _G(name, dd)
    got = G.cell_totals()
    assert got.dtype == np.float64 and got.shape == (N_ROWS,)
    assert np.array_equal(got, X.sum(axis=1)) and got[ZERO_CELL] == 0
    again = G.cell_totals()
    assert np.array_equal(again, got) and again is not got       # (cached on the device; the caller gets a copy)


@pytest.mark.parametrize('name,dd', CASES, ids=CASE_IDS)
def test_raw_moments_are_exact(name, dd):
    X, G = _X(), _G(name, dd)
    for C in CS:
        lab = _random_labels(C)
        got = G.cluster_gene_stats(lab, n_clusters=C, **RAW)
        _assert_exact(got, _raw_reference(X, lab, C), '%s C=%d' % (name, C))
        assert (got['n_expressing'][:, ZERO_GENE] == 0).all()
    lab, C = _blocked_labels()
    ref = _raw_reference(X, lab, C)
    assert ref['sizes'][3] == 0 and ref['sizes'][2] == 1
    _assert_exact(G.cluster_gene_stats(lab, **RAW), ref, '%s blocked' % name)                      # (C from the labels)
    _assert_exact(G.cluster_gene_stats(torch.as_tensor(lab, device=G.device), n_clusters=C, **RAW), ref, '%s tensor' % name)


def test_counts_beyond_uint16_fall_to_the_sliced_layout_and_stay_exact():
    X = _X().copy()
    X[3, 10] = 70000.0
    X[700, 20] = 2.0 ** 24 - 1
    assert (X[:, 10] != 0).mean() > DENSE_DENSITY and (X[:, 20] != 0).mean() > DENSE_DENSITY
    G = _model('GaP', X, K, dense_density=DENSE_DENSITY)
    dense_genes = G.counts.col_perm.cpu().numpy()[:G.counts.gd]
    assert 10 not in dense_genes and 20 not in dense_genes and 30 in dense_genes
    assert np.array_equal(G.cell_totals(), X.sum(axis=1))
    for C in (3, 17):
        lab = _random_labels(C)
        ref = _raw_reference(X, lab, C)
        assert ref['sumsq'].max() >= (2.0 ** 24 - 1) ** 2
        _assert_exact(G.cluster_gene_stats(lab, n_clusters=C, **RAW), ref, 'big counts C=%d' % C)


@pytest.mark.parametrize('dd', [None, DENSE_DENSITY], ids=['sliced', 'hybrid'])
def test_taller_matrix_takes_the_long_work_groups(dd):
    """Enough rows for the work-group shapes of a large matrix (TALL_ROWS): several work-groups add into one (cluster, gene)."""
    X = _counts(8, n=TALL_ROWS)
    G = _model('GaP', X, K, dense_density=dd)
    assert np.array_equal(G.cell_totals(), X.sum(axis=1))
    for C in (3, 37):
        lab = _random_labels(C, n=TALL_ROWS)
        _assert_exact(G.cluster_gene_stats(lab, n_clusters=C, **RAW), _raw_reference(X, lab, C), 'tall C=%d' % C)
    lab = _random_labels(3, n=TALL_ROWS)
    _check_markers(G.marker_genes(lab), X, lab, 3, 50, 'tall')


@pytest.mark.parametrize('dd', [None, DENSE_DENSITY], ids=['sliced', 'hybrid'])
def test_a_layout_with_its_own_cell_order_is_read_through_row_perm(dd):
    """sort_rows packs the cells of a chunk by depth: labels, scales and totals stay in the caller's row order."""
    import oriana_amd.models as M
    from oriana_amd import engine
    X = _X()
    dev = torch.device('cuda', torch.cuda.current_device())
    counts = engine.CountTiles.from_dense(X, dev, sort_rows=True, dense_density=dd)
    assert counts.row_perm is not None and not np.array_equal(counts.row_perm.cpu().numpy(), np.arange(N_ROWS))
    assert (counts.gd > 0) == bool(dd)
    rng = np.random.default_rng(1)
    G = M.GaP(counts, k=K, init=(rng.gamma(1.0, 1.0, size=(N_ROWS, K)), rng.gamma(1.0, 1.0, size=(M_COLS, K))))
    assert np.array_equal(G.cell_totals(), X.sum(axis=1))
    for lab, C in ((_random_labels(17), 17), _blocked_labels()):
        _assert_exact(G.cluster_gene_stats(lab, n_clusters=C, **RAW), _raw_reference(X, lab, C), 'sort_rows C=%d' % C)
    lab = _random_labels(3)
    _check_markers(G.marker_genes(lab), X, lab, 3, 50, 'sort_rows')


@pytest.mark.parametrize('dd', [None, DENSE_DENSITY], ids=['sliced', 'hybrid'])
def test_row_shards_add_up_exactly(dd):
    X, C = _X(), 17
    lab = _random_labels(C)
    whole = _G('GaP', dd).cluster_gene_stats(lab, n_clusters=C, **RAW)
    A, B = _model('GaP', X[:400], K, dense_density=dd), _model('GaP', X[400:], K, dense_density=dd)
    a = A.cluster_gene_stats(lab[:400], n_clusters=C, **RAW)
    b = B.cluster_gene_stats(lab[400:], n_clusters=C, **RAW)
    for k in ('n_expressing', 'sum', 'sumsq', 'sizes'):
        assert np.array_equal(a[k] + b[k], whole[k]), k
    assert np.array_equal(np.concatenate([A.cell_totals(), B.cell_totals()]), X.sum(axis=1))


@pytest.mark.parametrize('name,dd', [('GaP', None), ('GaP', DENSE_DENSITY), ('SparseZIGaP', DENSE_DENSITY), ('ZIGaP', None)],
                         ids=['GaP-sliced', 'GaP-hybrid', 'SparseZIGaP-hybrid', 'ZIGaP-sliced'])
def test_transformed_moments_within_the_derived_bounds(name, dd):
    """The defaults (normalised to 1e4, log1p): 'sum' within (2 cnt + 8) u sum y, 'sumsq' within (2 cnt + 16) u sum y^2
    (marker_reference: one product rounding, at most 1 ulp per log1p on each side, any summation order)."""
    X, G = _X(), _G(name, dd)
    worst = 0.0
    for C in (3, 37):
        lab = _random_labels(C)
        cnt, s1, s2, sizes = mr.moments(X, lab, C)
        b1, b2 = mr.moment_bounds(cnt, s1, s2)
        got = G.cluster_gene_stats(lab, n_clusters=C)
        assert np.array_equal(got['n_expressing'], cnt.astype(np.float64)) and np.array_equal(got['sizes'], sizes)
        assert not np.isnan(got['sum']).any() and not np.isnan(got['sumsq']).any()
        for k, ref, b in (('sum', s1, b1), ('sumsq', s2, b2)):
            diff = np.abs(got[k].astype(np.longdouble) - ref).astype(np.float64)
            assert (got[k][cnt == 0] == 0).all(), k
            ratio = float((diff[cnt > 0] / b[cnt > 0]).max())
            worst = max(worst, ratio)
            print('%s C=%d %s: largest diff / bound = %.3g' % (name, C, k, ratio))
            assert (diff <= b).all(), (k, C)
    print('largest diff / bound: %.3g' % worst)
    # the cell without a count has scale 0, not inf: a raw-count twin (normalize=False) agrees on the expressing cells
    assert np.array_equal(G.cluster_gene_stats(lab, n_clusters=C, normalize=False)['n_expressing'], cnt.astype(np.float64))


def _check_markers(got, X, lab, C, n_top, what, **kw):
    from oriana_amd import markers
    log1p = kw.get('log1p', True)
    cnt, s1, s2, sizes = mr.moments(X, lab, C, **kw)
    ref = mr.welch_two_pass(X, lab, C, **kw)
    if kw.get('normalize', True) or log1p:
        b1, b2 = mr.moment_bounds(cnt, s1, s2)
    else:
        b1, b2 = np.zeros(cnt.shape), np.zeros(cnt.shape)
    f1, f2 = s1.astype(np.float64), s2.astype(np.float64)
    bnd = mr.welch_bounds(f1, f2, sizes, b1 + mr.U * f1, b2 + mr.U * f2)
    live = sizes > 0
    sc, rs = got['scores'], ref['scores'].astype(np.float64)
    assert sc.shape == (C, X.shape[1]) and np.isnan(sc[~live]).all() and not np.isnan(sc[live]).any()
    diff = np.abs(sc - rs)[live]
    b = bnd['scores'][live]
    said = np.isfinite(b)
    assert said.mean() > 0.95, 'the bound must say something about nearly every gene'
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(b > 0, diff / b, np.where(diff == 0, 0.0, np.inf))[said]
    print('%s: scores largest diff / bound = %.3g, largest diff %.3g' % (what, ratio.max(), diff[said].max()))
    assert (diff[said] <= b[said]).all(), what
    assert (sc[live][:, ZERO_GENE] == 0).all() and not np.signbit(sc[live][:, ZERO_GENE]).any()
    for k in ('pct_in', 'pct_out'):
        assert np.allclose(got[k][live], ref[k].astype(np.float64)[live], rtol=4 * mr.U, atol=0), (what, k)
    # the fold change: d log2(e^m - 1 + 1e-9) = e^m dm / ((e^m - 1 + 1e-9) ln 2) <= (1 + 1 / m) dm / ln 2 (the raw mode: dm / (m ln 2))
    for side, mk in (('in', 'mean_in'), ('out', 'mean_out')):
        assert np.isfinite(bnd[mk][live]).all()
    mc, mo = ref['mean_in'].astype(np.float64)[live], ref['mean_out'].astype(np.float64)[live]
    with np.errstate(invalid='ignore', divide='ignore'):
        amp = (lambda m_: 1.0 + 1.0 / np.maximum(m_, 1e-9)) if log1p else (lambda m_: 1.0 / np.maximum(m_, 1e-9))
        eb = (amp(mc) * bnd['mean_in'][live] + amp(mo) * bnd['mean_out'][live]) / np.log(2.0)
    lf, rl = got['logfoldchanges'][live], ref['logfoldchanges'].astype(np.float64)[live]
    assert np.isfinite(lf).all()
    assert (np.abs(lf - rl) <= 2 * eb + 64 * mr.U * (1.0 + np.abs(rl))).all(), what
    # df = (a + b)^2 / (a^2 / (n_c - 1) + b^2 / (n_r - 1)), a + b = q, each of a, b known to eq: the logarithmic derivatives are
    # at most (2 + 4 N) / q in magnitude (test_markers_host), so df is known to 2 (2 + 4 N) eq / q relative in first order;
    # twice that is asked wherever it is below 1e-3 (first order holds), NaN (no variance, a single cell) must match
    with np.errstate(invalid='ignore', divide='ignore'):
        tol = 4.0 * (2.0 + 4.0 * X.shape[0]) * bnd['eq'] / bnd['q']
    sure = (tol < 1e-3) & live[:, None]
    assert sure[live].mean() > 0.8
    rd = ref['df'].astype(np.float64)
    assert np.array_equal(np.isnan(got['df'][sure]), np.isnan(rd[sure])), what
    with np.errstate(invalid='ignore'):
        ok = np.isnan(rd[sure]) | (np.abs(got['df'][sure] - rd[sure]) <= (tol[sure] + 64 * mr.U) * np.abs(rd[sure]))
    assert ok.all(), what
    none = live[:, None] & (bnd['q'] == 0)
    assert np.isnan(got['df'][none]).all(), what
    assert got['genes'].dtype == np.int64 and got['genes'].shape == (C, min(n_top, X.shape[1]))
    assert np.array_equal(got['genes'], markers.rank(got['scores'], n_top)), what
    assert np.array_equal(got['sizes'], sizes)


@pytest.mark.parametrize('name,dd', CASES, ids=CASE_IDS)
def test_marker_genes_against_the_two_pass_reference(name, dd):
    X, G = _X(), _G(name, dd)
    lab = _random_labels(3)
    _check_markers(G.marker_genes(lab), X, lab, 3, 50, '%s C=3' % name)
    lab, C = _blocked_labels()                                   # an id without cells, a cluster of one cell
    _check_markers(G.marker_genes(lab, n_top=400), X, lab, C, 400, '%s blocked' % name)
    if name == 'GaP':
        lab = _random_labels(17)
        _check_markers(G.marker_genes(lab, n_top=7, **RAW), X, lab, 17, 7, '%s raw C=17' % name, **RAW)


@pytest.mark.parametrize('dd', [None, DENSE_DENSITY], ids=['sliced', 'hybrid'])
def test_planted_markers_come_out_on_top(dd):
    """Two planted clusters: rows 0-399 get genes 100-109 multiplied by 8.  The ten top genes of cluster 0 are exactly those
    (and none of them is among the top of cluster 1).  The ten genes are first given a count in every cell: at the 15 % density
    _counts() gives them the zeros dominate their variance and the two-pass reference itself does not put them on top (its
    scores for them are 0.8-3.9, an unrelated gene reaches 2.9) -- a factor of 8 only shows in a gene that is expressed."""
    X = _X().copy()
    X[:, 100:110] = np.random.default_rng(5).poisson(3.0, size=(N_ROWS, 10)) + 1
    X[ZERO_CELL, :] = 0
    X[:400, 100:110] *= 8
    lab = (np.arange(N_ROWS) >= 400).astype(np.int64)
    ref = mr.welch_two_pass(X, lab, 2)['scores'].astype(np.float64)
    assert set(np.argsort(-ref[0], kind='stable')[:10].tolist()) == set(range(100, 110)), 'the premise, on the reference'
    G = _model('GaP', X, K, dense_density=dd)
    got = G.marker_genes(lab, n_top=10)
    assert set(got['genes'][0].tolist()) == set(range(100, 110))
    assert not set(got['genes'][1].tolist()) & set(range(100, 110))
    assert (got['logfoldchanges'][0, 100:110] > 1).all()
    _check_markers(got, X, lab, 2, 10, 'planted')


def test_state_is_left_alone():
    X = _X()
    G = _model('SparseZIGaP', X, K)
    G.fit(1)
    torch.cuda.synchronize()
    before = {k: np.array(v, copy=True) for k, v in G.state().items()}
    G.cell_totals()
    G.cluster_gene_stats(_random_labels(17))
    G.marker_genes(_random_labels(3))
    after = G.state()
    assert sorted(before) == sorted(after)
    for k in before:
        assert before[k].tobytes() == np.asarray(after[k]).tobytes(), k


def test_value_errors_come_before_any_launch():
    G = _G('GaP', None)
    from oriana_amd import _lib
    limit = int(_lib.load().oriana_group_stats_max_groups())
    assert limit >= 256
    good = _random_labels(3)
    calls = []
    real = _lib.call
    import oriana_amd.models.base as base

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    base.call = spy
    try:
        bad = good.copy()
        bad[7] = -1
        for args, kw in (((bad,), {}), ((good[:-1],), {}), ((good.astype(np.float64),), {}), ((good,), {'target_sum': 0}),
                         ((good,), {'target_sum': -1.0}), ((good,), {'n_clusters': 2}), ((good,), {'n_clusters': limit + 1}),
                         ((good * (limit // 2 + 1),), {}), ((good.reshape(-1, 1),), {})):
            with pytest.raises(ValueError):
                G.cluster_gene_stats(*args, **kw)
            with pytest.raises(ValueError):
                G.marker_genes(*args, **kw)
        with pytest.raises(ValueError):
            G.marker_genes(good, n_top=-1)
        assert calls == [], calls
        with pytest.raises(ValueError):                          # a single non-empty cluster has no rest to test against
            G.marker_genes(np.zeros(N_ROWS, dtype=np.int64), n_clusters=2)
        assert G.cluster_gene_stats(good, n_clusters=limit, **RAW)['sum'].shape == (limit, M_COLS)
    finally:
        base.call = real


# ---- row sharding: a process group of one rank ------------------------------------------------------------------------------

def _worker(rank, port, X, lab, out):
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
        raw = G.cluster_gene_stats(lab, **RAW)
        mg = G.marker_genes(lab)
        np.savez(out, totals=G.cell_totals(), **{'raw_' + k: v for k, v in raw.items()}, **{'mg_' + k: v for k, v in mg.items()})
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    # (as tests/test_sharded_gpu.py: leave without the static destructors of the interpreter / c10d)
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(0)


def test_one_rank_process_group_gives_the_same_arrays(tmp_path):
    """Under a one-rank process group with ORIANA_FORCE_SHARDED=1 (a fresh child process) the packed moments and sizes go through
    the all-reduce: the raw arrays bit for bit, the transformed ones within twice the moment bound of the single-process
    model's (two runs of the same atomics), the ranking on the run's own scores."""
    from oriana_amd import markers
    X, C = _X(), 17
    lab = _random_labels(C)
    out = str(tmp_path / 'markers_sharded.npz')
    mp.spawn(_worker, args=(_free_port(), X, lab, out), nprocs=1, join=True)
    got = np.load(out)
    G = _G('GaP', None)
    assert np.array_equal(got['totals'], X.sum(axis=1))
    _assert_exact({k: got['raw_' + k] for k in ('n_expressing', 'sum', 'sumsq', 'sizes')}, _raw_reference(X, lab, C), 'one-rank group')
    one = G.marker_genes(lab)
    cnt, s1, s2, _ = mr.moments(X, lab, C)
    b1, b2 = mr.moment_bounds(cnt, s1, s2)
    assert np.array_equal(got['mg_n_expressing'], one['n_expressing']) and np.array_equal(got['mg_sizes'], one['sizes'])
    assert (np.abs(got['mg_sum'] - one['sum']) <= 2 * b1).all() and (np.abs(got['mg_sumsq'] - one['sumsq']) <= 2 * b2).all()
    _check_markers({k[3:]: got[k] for k in got.files if k.startswith('mg_')}, X, lab, C, 50, 'one-rank group')
    assert np.array_equal(got['mg_genes'], markers.rank(got['mg_scores'], 50))
