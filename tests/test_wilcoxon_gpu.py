# -*- coding: utf-8 -*-
"""cluster_rank_sums() / marker_genes(method='wilcoxon') of every model on both layouts against the SciPy reference of
tests/wilcoxon_reference.py on the dense X.  Rank sums, tie terms and counts are integers (half-integers): they are compared bit
for bit, whatever the panels and whichever sort path a gene takes; the statistic is held to the bound derived in the reference
module."""
import os
import sys

import numpy as np
import pytest
import scipy.stats
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import wilcoxon_reference as wr
from test_deviance_path_gpu import _model, _free_port, N_ROWS, M_COLS, DENSE_DENSITY
from test_markers_gpu import _X, _G, _random_labels, _blocked_labels, _check_markers, K, ZERO_GENE, CASES, CASE_IDS, RAW

pytestmark = pytest.mark.gpu

FULL_GENE = 250
CS = (2, 3, 17, 37, 100)
LAYOUTS = [None, DENSE_DENSITY]
LAYOUT_IDS = ['sliced', 'hybrid']
_refs = {}


def _ref(X, lab, C, normalize, tag='X'):
    """The reference of one (matrix, labelling, value kind), computed once; ranks and tie terms once per (matrix, value kind)."""
    base = (tag, normalize)
    if base not in _refs:
        V = wr.values(X, normalize)
        _refs[base] = (scipy.stats.rankdata(V, axis=0, method='average'), wr.tie_terms(V))
    key = (tag, normalize, C, np.asarray(lab).tobytes())
    if key not in _refs:
        _refs[key] = wr.rank_sums(X, lab, C, normalize=normalize, ranked=_refs[base][0], tied=_refs[base][1])
    return _refs[key]


def _assert_exact(got, ref, what):
    assert got['rank_sum'].dtype == np.float64 and got['rank_sum'].shape == ref['rank_sum'].shape, what
    for k in ('rank_sum', 'n_expressing'):
        bad = np.argwhere(got[k] != ref[k])
        assert bad.size == 0, '%s %s: %d entries differ, first (cluster, gene) %s: %r != %r' % (
            what, k, len(bad), bad[0], got[k][tuple(bad[0])], ref[k][tuple(bad[0])])
    assert got['tie_term'].dtype == np.int64 and got['tie_term'].shape == ref['tie_term'].shape, what
    assert [int(t) for t in got['tie_term']] == [int(t) for t in ref['tie_term']], what
    assert got['sizes'].dtype == np.int64 and np.array_equal(got['sizes'], ref['sizes']), what


def _assert_same(a, b, what):
    for k in ('rank_sum', 'tie_term', 'n_expressing', 'sizes'):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def _labellings():
    return [(_random_labels(C), C) for C in CS] + [_blocked_labels()]


@pytest.mark.parametrize('name,dd', CASES, ids=CASE_IDS)
def test_rank_sums_are_exact(name, dd):
    """1. Every (cluster, gene) bit for bit; normalize=False has integer values and tie runs of hundreds."""
    X, G = _X(), _G(name, dd)
    for lab, C in _labellings():
        for normalize in (True, False):
            got = G.cluster_rank_sums(lab, n_clusters=C, normalize=normalize)
            _assert_exact(got, _ref(X, lab, C, normalize), '%s C=%d normalize=%s' % (name, C, normalize))
        raw = G.cluster_gene_stats(lab, n_clusters=C, **RAW)
        assert np.array_equal(got['n_expressing'], raw['n_expressing'])
    lab, C = _blocked_labels()
    ref = _ref(X, lab, C, True)
    assert ref['sizes'][3] == 0 and ref['sizes'][2] == 1
    _assert_exact(G.cluster_rank_sums(lab), ref, '%s C from the labels' % name)
    _assert_exact(G.cluster_rank_sums(torch.as_tensor(lab, device=G.device), n_clusters=C), ref, '%s tensor' % name)


@pytest.mark.parametrize('dd', LAYOUTS, ids=LAYOUT_IDS)
def test_the_global_memory_sort_gives_the_same_bits(dd):
    """2. sort_cap=64: every gene with a count (the sparse ones hold 100 to 150, the 70 genes at 80 % about 644, gene 250 804) is
    cut into runs of 64, sorted in LDS and merged through global memory; sort_cap=128: most sparse genes stay in LDS, next to
    the long ones; sort_cap=1: no LDS sort at all, every gene is merged from single records."""
    X, G = _X(), _G('GaP', dd)
    nnz = (X != 0).sum(axis=0)
    assert (nnz > 64).sum() == M_COLS - 1 and (nnz > 128).sum() >= 71 and (nnz[nnz > 0] <= 128).sum() > 100
    assert nnz[FULL_GENE] == N_ROWS - 1
    for lab, C in ((_random_labels(17), 17), _blocked_labels()):
        for normalize in (True, False):
            ref = _ref(X, lab, C, normalize)
            for cap in (64, 128, 1, 100):                        # (100: a cap that is no power of two, runs of 64)
                got = G.cluster_rank_sums(lab, n_clusters=C, normalize=normalize, sort_cap=cap)
                _assert_exact(got, ref, 'sort_cap=%d C=%d normalize=%s' % (cap, C, normalize))


@pytest.mark.parametrize('dd', LAYOUTS, ids=LAYOUT_IDS)
def test_the_default_cap_is_crossed_without_forcing(dd):
    """3. More rows than the default cap: a fully expressed gene takes the global-memory path, an 80 % gene and the sparse
    ones stay in LDS."""
    from oriana_amd import _lib
    cap = int(_lib.load().oriana_rank_sums_lds_cap())
    n, m = cap + 261, 40
    rng = np.random.default_rng(77)
    dens = np.full(m, 0.1)
    dens[1:34] = 0.8                                             # (enough genes above dense_density for a dense block of 32)
    X = ((rng.poisson(rng.gamma(0.6, 4.0, size=(n, m))) + 1) * (rng.random((n, m)) < dens)).astype(np.float64)
    X[:, 0] = rng.poisson(6.0, size=n) + 1
    nnz = (X != 0).sum(axis=0)
    assert nnz[0] == n > cap and (nnz[1:34] > cap // 2).all() and (nnz[1:34] <= cap).all() and (nnz[34:] < cap // 4).all()
    G = _model('GaP', X, K, dense_density=dd)
    lab = _random_labels(3, n=n)
    for normalize in (True, False):
        got = G.cluster_rank_sums(lab, n_clusters=3, normalize=normalize)
        _assert_exact(got, _ref(X, lab, 3, normalize, tag='tall'), 'tall normalize=%s' % normalize)


@pytest.mark.parametrize('dd', LAYOUTS, ids=LAYOUT_IDS)
def test_panels_change_nothing(dd):
    """4. A scratch that admits the heaviest gene tile and no more (several panels), and one below every tile (each tile an
    oversized panel of its own), against the one-panel result."""
    from oriana_amd import markers
    X, G = _X(), _G('SparseZIGaP', dd)
    ct = G.counts
    perm = ct.col_perm.cpu().numpy() if ct.col_perm is not None else np.arange(M_COLS)
    nnz = (X != 0).sum(axis=0)[perm]
    gd = ct.gd
    tiles = [(t, t + 32) for t in range(0, gd, 32)] + [(t, min(M_COLS, t + 256)) for t in range(gd, M_COLS, 256)]
    heaviest = max(int(nnz[a:b].sum()) for a, b in tiles)
    one = markers.plan_rank_panels(nnz, gd, (1 << 30) // 24)
    assert len(one) == (2 if gd else 1)
    assert len(markers.plan_rank_panels(nnz, gd, heaviest)) > len(one)
    assert len(markers.plan_rank_panels(nnz, gd, 1)) == len(tiles)
    for lab, C in ((_random_labels(17), 17), _blocked_labels()):
        whole = G.cluster_rank_sums(lab, n_clusters=C)
        _assert_exact(whole, _ref(X, lab, C, True), 'one panel')
        for scratch_bytes in (24 * heaviest, 24, 0):
            _assert_same(G.cluster_rank_sums(lab, n_clusters=C, scratch_bytes=scratch_bytes), whole, scratch_bytes)
        _assert_same(G.cluster_rank_sums(lab, n_clusters=C, scratch_bytes=24 * heaviest, sort_cap=64), whole, 'both')


@pytest.mark.parametrize('dd', LAYOUTS, ids=LAYOUT_IDS)
def test_a_layout_with_its_own_cell_and_gene_order(dd):
    """5. sort_rows packs the cells of a chunk by depth and the genes by their counts: labels and scales are read through
    row_perm, the outputs land in the caller's gene order."""
    import oriana_amd.models as M
    from oriana_amd import engine
    X = _X()
    dev = torch.device('cuda', torch.cuda.current_device())
    counts = engine.CountTiles.from_dense(X, dev, sort_rows=True, dense_density=dd)
    assert counts.row_perm is not None and not np.array_equal(counts.row_perm.cpu().numpy(), np.arange(N_ROWS))
    assert counts.col_perm is not None and not np.array_equal(counts.col_perm.cpu().numpy(), np.arange(M_COLS))
    assert (counts.gd > 0) == bool(dd)
    rng = np.random.default_rng(1)
    G = M.GaP(counts, k=K, init=(rng.gamma(1.0, 1.0, size=(N_ROWS, K)), rng.gamma(1.0, 1.0, size=(M_COLS, K))))
    for lab, C in ((_random_labels(17), 17), _blocked_labels()):
        for normalize in (True, False):
            _assert_exact(G.cluster_rank_sums(lab, n_clusters=C, normalize=normalize, sort_cap=64), _ref(X, lab, C, normalize),
                          'sort_rows C=%d' % C)


def test_two_calls_agree_and_nothing_else_moves():
    """6. The same bits twice, state() untouched, and the t-test still answers as before."""
    X = _X()
    G = _model('SparseZIGaP', X, K)
    G.fit(1)
    torch.cuda.synchronize()
    before = {k: np.array(v, copy=True) for k, v in G.state().items()}
    lab = _random_labels(3)
    keys = sorted(G.marker_genes(lab))
    a = G.cluster_rank_sums(lab, sort_cap=64)
    b = G.cluster_rank_sums(lab, sort_cap=64)
    _assert_same(a, b, 'two calls')
    G.marker_genes(lab, method='wilcoxon')
    after = G.state()
    assert sorted(before) == sorted(after)
    for k in before:
        assert before[k].tobytes() == np.asarray(after[k]).tobytes(), k
    again = G.marker_genes(lab)
    assert sorted(again) == keys and 'df' in again and 'auc' not in again and 'rank_sum' not in again
    _check_markers(again, X, lab, 3, 50, 't-test after wilcoxon')


@pytest.mark.parametrize('name,dd', [('GaP', None), ('GaP', DENSE_DENSITY), ('SparseZIGaP', DENSE_DENSITY), ('ZIGaP', None)],
                         ids=['GaP-sliced', 'GaP-hybrid', 'SparseZIGaP-hybrid', 'ZIGaP-sliced'])
def test_marker_genes_wilcoxon(name, dd):
    """7. The statistic within the derived bound for both tie_correct values, NaN rows as the reference has them."""
    from oriana_amd import markers
    X, G = _X(), _G(name, dd)
    for (lab, C), n_top in ((( _random_labels(3), 3), 50), (_blocked_labels(), 400)):
        ref = _ref(X, lab, C, True)
        live = ref['sizes'] > 0
        for tc in (False, True):
            got = G.marker_genes(lab, n_top=n_top, method='wilcoxon', tie_correct=tc, n_clusters=C)
            wr.assert_scores(got['scores'], wr.scores(ref, tie_correct=tc), '%s C=%d tie_correct=%s' % (name, C, tc))
            _assert_exact(got, ref, 'marker_genes C=%d' % C)
            assert got['genes'].dtype == np.int64 and got['genes'].shape == (C, min(n_top, M_COLS))
            assert np.array_equal(got['genes'], markers.rank(got['scores'], n_top))
            auc = got['auc']
            assert np.array_equal(np.isnan(auc), np.isnan(wr.scores(ref)['auc'].astype(np.float64)))
            assert (auc[live] >= 0).all() and (auc[live] <= 1).all() and (auc[live][:, ZERO_GENE] == 0.5).all()
            assert (got['scores'][live][:, ZERO_GENE] == 0).all()
            assert 'df' not in got
            # fold change and fractions: from the moments, as the t-test has them
            w = markers.welch_from_moments(got['n_expressing'], got['sum'], got['sumsq'], got['sizes'])
            for k in ('logfoldchanges', 'pct_in', 'pct_out'):
                assert np.array_equal(got[k], w[k], equal_nan=True), k
    raw = G.marker_genes(lab, method='wilcoxon', normalize=False, log1p=False, sort_cap=64, scratch_bytes=24)
    _assert_exact(raw, _ref(X, lab, C, False), 'raw')
    wr.assert_scores(raw['scores'], wr.scores(_ref(X, lab, C, False)), 'raw')
    with pytest.raises(ValueError):
        G.marker_genes(lab, method='logreg')
    with pytest.raises(ValueError):
        G.marker_genes(np.zeros(N_ROWS, dtype=np.int64), method='wilcoxon', n_clusters=2)


def _entry(G, lab32, scale, C, panel, capacity, guard=0, sort_cap=0):
    """oriana_rank_sums on one panel with a scratch of exactly the size it asks for, `guard` bytes of 0xA5 behind it."""
    from oriana_amd import _lib
    ct, dev, m = G.counts, G.device, G.m
    lib = _lib.load()
    by = int(lib.oriana_rank_sums_scratch_bytes_for(capacity, panel[1] - panel[0]))
    assert by > 0 and by % 8 == 0
    scratch = torch.full((by + guard,), 0xA5, dtype=torch.uint8, device=dev)
    pos2, cnt = torch.zeros((C, m), dtype=torch.int64, device=dev), torch.zeros((C, m), dtype=torch.int64, device=dev)
    ties, ovf = torch.zeros(m, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call('oriana_rank_sums', ct.sparse_struct, ct.dense.c_struct if ct.dense is not None else None, _lib.ptr(ct.row_perm),
              _lib.ptr(ct.col_perm), _lib.ptr(lab32), _lib.ptr(scale), C, panel[0], panel[1], _lib.ptr(scratch), capacity, sort_cap,
              _lib.ptr(pos2), _lib.ptr(cnt), _lib.ptr(ties), _lib.ptr(ovf), _lib.stream_ptr())
    torch.cuda.synchronize()
    return pos2.cpu().numpy(), cnt.cpu().numpy(), ties.cpu().numpy(), int(ovf.cpu()[0]), scratch[by:].cpu().numpy()


@pytest.mark.parametrize('dd', LAYOUTS, ids=LAYOUT_IDS)
def test_the_c_entry_directly(dd):
    """8. Labels outside [0, C) are ranked and add to no cluster; a capacity one below the panel's content sets overflow and
    writes neither past the scratch nor into the outputs."""
    from oriana_amd import markers
    X, G = _X(), _G('GaP', dd)
    ct, dev, C = G.counts, G.device, 5
    lab = _random_labels(C).copy()
    lab[::7] = C + 3
    lab[3::11] = -1
    lab[5] = 2 ** 31 - 1
    lab[6] = -2 ** 31
    assert ((lab < 0) | (lab >= C)).sum() > 150
    ref = _ref(X, lab, C, True)
    assert ref['sizes'].sum() < N_ROWS - 150
    lab32 = torch.as_tensor(lab.astype(np.int32), device=dev)
    scale = torch.as_tensor(wr.scale_of(X), device=dev)
    perm = ct.col_perm.cpu().numpy() if ct.col_perm is not None else np.arange(M_COLS)
    nnz = (X != 0).sum(axis=0)
    panels = markers.plan_rank_panels(nnz[perm], ct.gd, 10 ** 9)
    assert len(panels) == (2 if dd else 1)
    pos2, cnt, ties = (np.zeros((C, M_COLS), dtype=np.int64), np.zeros((C, M_COLS), dtype=np.int64), np.zeros(M_COLS, dtype=np.int64))
    for g0, g1, rec in panels:
        p, c, t, ovf, guard = _entry(G, lab32, scale, C, (g0, g1), rec, guard=4096, sort_cap=64)
        assert ovf == 0 and (guard == 0xA5).all()
        inside = np.zeros(M_COLS, dtype=bool)
        inside[perm[g0:g1]] = True
        assert not p[:, ~inside].any() and not c[:, ~inside].any() and not t[~inside].any()     # only the panel's columns
        pos2 += p; cnt += c; ties += t
    z = N_ROWS - nnz                                             # (from X: the cells outside every cluster are still cells)
    twice = (ref['sizes'][:, None] - cnt) * (z + 1)[None, :] + 2 * cnt * z[None, :] + pos2
    assert np.array_equal(cnt.astype(np.float64), ref['n_expressing'])
    assert np.array_equal(twice / 2.0, ref['rank_sum'])
    assert [int(t) for t in ties + z ** 3 - z] == [int(t) for t in ref['tie_term']]
    for g0, g1, rec in panels:
        p, c, t, ovf, guard = _entry(G, lab32, scale, C, (g0, g1), rec - 1, guard=4096)
        assert ovf == 1 and (guard == 0xA5).all()
        assert not p.any() and not c.any() and not t.any()


# ---- row sharding: two ranks ------------------------------------------------------------------------------------------------------

def _two_rank_worker(rank, world, port, X, lab, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import oriana_amd.models as M
        import oriana_amd.models.base as base
        from oriana_amd import dist as odist, engine
        r0, r1 = odist.shard_rows(X.shape[0], rank, world)
        dev = torch.device('cuda', 0)
        rng = np.random.default_rng(1000)
        a1 = rng.gamma(1.0, 1.0, size=(X.shape[0], K)); b1 = rng.gamma(1.0, 1.0, size=(X.shape[1], K))
        counts = engine.CountTiles.from_dense(X[r0:r1], dev, reduce_fn=lambda t: odist.all_reduce_sum(t), n_total=X.shape[0])
        G = M.GaP(counts, k=K, init=(a1[r0:r1], b1), device=dev, process_group=dist.group.WORLD)
        assert G.sharded and odist.world_size(G.pg) == 2
        torch.cuda.synchronize()
        seen = []
        real_call, real_reduce = base.call, odist.all_reduce_sum
        base.call = lambda name, *a: (seen.append(name), real_call(name, *a))[1]
        odist.all_reduce_sum = lambda *a, **kw: (seen.append('all_reduce_sum'), real_reduce(*a, **kw))[1]
        raised = []
        try:
            for f in (lambda: G.cluster_rank_sums(lab[r0:r1]), lambda: G.cluster_rank_sums(lab[r0:r1], n_clusters=3),
                      lambda: G.marker_genes(lab[r0:r1], method='wilcoxon')):
                try:
                    f()
                    raised.append('nothing')
                except NotImplementedError:
                    raised.append('NotImplementedError')
        finally:
            base.call, odist.all_reduce_sum = real_call, real_reduce
        t = G.marker_genes(lab[r0:r1])                           # the t-test is additive over shards and still works
        np.savez(out % rank, raised=np.array(raised), seen=np.array(seen, dtype=str), scores=t['scores'])
        dist.barrier()
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(0)


def test_two_ranks_raise_before_any_launch_or_collective(tmp_path):
    """9. Rank sums do not add up over shards of cells: both ranks raise NotImplementedError, and neither has launched a kernel
    or entered a collective by then."""
    X = _X()
    lab = _random_labels(3)
    out = str(tmp_path / 'wilcoxon_rank%d.npz')
    mp.spawn(_two_rank_worker, args=(2, _free_port(), X, lab, out), nprocs=2, join=True)
    for rank in (0, 1):
        got = np.load(out % rank)
        assert got['raised'].tolist() == ['NotImplementedError'] * 3, rank
        assert got['seen'].tolist() == [], rank
        assert got['scores'].shape == (3, M_COLS)


def test_a_one_rank_group_works(tmp_path):
    X = _X()
    lab = _random_labels(3)
    out = str(tmp_path / 'wilcoxon_one.npz')
    mp.spawn(_one_rank_worker, args=(_free_port(), X, lab, out), nprocs=1, join=True)
    got = np.load(out)
    _assert_exact({k: got[k] for k in ('rank_sum', 'tie_term', 'n_expressing', 'sizes')}, _ref(X, lab, 3, True), 'one-rank group')


def _one_rank_worker(rank, port, X, lab, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['ORIANA_FORCE_SHARDED'] = '1'
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
        np.savez(out, **G.cluster_rank_sums(lab))
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(0)
