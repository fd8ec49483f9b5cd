# -*- coding: utf-8 -*-
"""The NumPy restatement of snn_graph / louvain (tests/community_reference.py) against independent implementations -- networkx's
modularity and its Louvain, a sparse matrix product for the shared-neighbour counts --, its sensitivity to each rule of the sweep,
and the argument errors of the Python functions and the C entries, all without a GPU."""
import ctypes

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import community_cases as cc
import community_reference as cr

# every case x both weightings for the cheap checks; the independent Louvain runs once per case (resolution 1) and, on the
# 130-row case, at every resolution
QUALITY = [(name, 'snn', 1.0) for name in cc.ALL_CASES] + [(name, 'count', 1.0) for name in cc.ALL_CASES] + \
          [('blobs130', w, g) for w in cc.WEIGHTS for g in (0.5, 2.0)]


def _nx_graph(crow, col, w):
    G = nx.Graph()
    G.add_nodes_from(range(crow.size - 1))
    rows = cr.graph_rows(crow)
    for i, j, v in zip(rows.tolist(), col.tolist(), w.tolist()):
        if i < j:
            G.add_edge(i, j, weight=v)
        elif i == j:
            G.add_edge(i, i, weight=v // 2)                        # a self entry holds the inside weight in both directions
    return G


def _sets(labels):
    return [set(np.flatnonzero(labels == c).tolist()) for c in np.unique(labels)]


def test_the_cases_are_what_they_claim():
    assert cc.case('tiny')['indices'].shape == (5, 8) and (cc.case('tiny')['indices'] == -1).sum() == 20
    crow, col, w = cc.graph('identical', 'snn')
    assert (cc.case('identical')['indices'][:30:3] >= 0).all()
    assert (np.diff(crow)[:30:3] > 128).sum() >= 8                 # the identical rows are hubs: long rows at the default cap
    crow, col, w = cc.graph('star', 'snn')
    assert np.diff(crow)[0] == 5000 and np.diff(crow)[1:].max() == 1
    crow, col, w = cc.graph('aggregated', 'snn')
    rows = cr.graph_rows(crow)
    assert (rows == col).sum() == crow.size - 1 and w[rows == col].min() > 0      # every node of the aggregated graph has a self entry
    assert np.diff(crow).max() > 8


@pytest.mark.parametrize('name', cc.KNN_CASES)
def test_snn_graph_is_the_masked_incidence_product(name):
    """6. w = (A A^T) masked by the pattern, A the closed-neighbourhood incidence; 'count' = B + B^T."""
    idx = cc.case(name)['indices']
    n = idx.shape[0]
    N = cr.neighbour_sets(idx)
    r = np.concatenate([np.full(v.size, i) for i, v in enumerate(N)])
    c = np.concatenate(N)
    B = sp.csr_matrix((np.ones(r.size, dtype=np.int64), (r, c)), shape=(n, n))
    A = (B + sp.identity(n, dtype=np.int64, format='csr')).tocsr()
    P = (B + B.T).tocsr()
    P.sort_indices()
    crow, col, w = cc.graph(name, 'count')
    assert np.array_equal(crow, P.indptr) and np.array_equal(col, P.indices) and np.array_equal(w, P.data)
    M = (A @ A.T).multiply(P > 0).tocsr()
    M.sort_indices()
    crow, col, w = cc.graph(name, 'snn')
    assert np.array_equal(crow, M.indptr) and np.array_equal(col, M.indices) and np.array_equal(w, M.data)
    assert w.min() >= 1 and col.dtype == np.int32 and w.dtype == np.int64 and crow.dtype == np.int64


def test_a_repeated_neighbour_is_refused():
    idx = cc.case('blobs130')['indices'].copy()
    idx[7, 3] = idx[7, 0]
    with pytest.raises(ValueError, match='twice'):
        cr.snn_graph(idx)
    idx[7, 3] = 7                                                  # the row's own index is skipped, not a repeat
    cr.snn_graph(idx)


@pytest.mark.parametrize('name', ('blobs130', 'blobs600', 'identical', 'tiny'))
def test_modularity_equals_networkx(name):
    """1. The reference's Q against networkx.community.modularity, both weightings, three resolutions, to 1e-12."""
    for weights in cc.WEIGHTS:
        G = _nx_graph(*cc.graph(name, weights))
        for gamma in cc.GAMMAS:
            out = cc.run(name, weights, gamma)
            want = nx.community.modularity(G, _sets(out['labels']), weight='weight', resolution=gamma)
            assert abs(out['modularity'] - want) <= 1e-12, (name, weights, gamma, out['modularity'], want)
            assert out['modularity'] == cr.modularity(*cc.graph(name, weights), out['labels'], gamma)


def test_modularity_with_self_entries_equals_networkx():
    crow, col, w = cc.graph('aggregated', 'snn')
    out = cc.run('aggregated', 'snn', 1.0)
    want = nx.community.modularity(_nx_graph(crow, col, w), _sets(out['labels']), weight='weight', resolution=1.0)
    assert abs(out['modularity'] - want) <= 1e-12


def test_separated_blobs_are_recovered():
    """2. Six separated blobs: six communities, adjusted Rand index exactly 1."""
    from oriana_amd import cluster
    truth = cc.case('blobs600')['truth']
    for weights in cc.WEIGHTS:
        out = cc.run('blobs600', weights, 1.0)
        assert out['n_communities'] == 6
        assert cluster.adjusted_rand(out['labels'], truth) == 1.0
        sizes = np.bincount(out['labels'])
        assert (np.diff(sizes) <= 0).all()                         # 0 is the largest community


@pytest.mark.parametrize('name,weights,gamma', QUALITY)
def test_quality_against_networkx_louvain(name, weights, gamma):
    """3. Q >= 0.97 x the smallest Q of five seeded runs of networkx's Louvain on the same graph."""
    G = _nx_graph(*cc.graph(name, weights))
    theirs = min(nx.community.modularity(G, nx.community.louvain_communities(G, weight='weight', resolution=gamma, seed=s),
                                         weight='weight', resolution=gamma) for s in range(5))
    ours = cc.run(name, weights, gamma)['modularity']
    print('quality %s %s gamma=%g: ours %.6f, worst of five %.6f, ratio %.4f' % (name, weights, gamma, ours, theirs,
                                                                                  ours / theirs if theirs else float('nan')))
    assert ours >= 0.97 * theirs, (name, weights, gamma, ours, theirs)


@pytest.mark.parametrize('name', cc.ALL_CASES)
def test_accepted_sweeps_raise_q_and_2m_is_kept(name):
    """4. Inside a level every accepted sweep strictly raises Q's exact numerator; 2m is the same at every level; a level
    starts at the modularity the last one ended with."""
    for weights in cc.WEIGHTS:
        for gamma in cc.GAMMAS:
            out = cc.run(name, weights, gamma)
            two_m = out['trace'][0]['graph'][4]
            last = None
            for lev, tr in zip(out['levels'], out['trace']):
                crow, col, w, deg, tm = tr['graph']
                assert tm == two_m == int(w.sum()) and lev['nodes'] == crow.size - 1
                q = []
                for comm, tot, size in tr['states'][:lev['sweeps'] + 1]:
                    _, _, I, S = cr.partition_sums(crow, col, w, deg, comm)
                    q.append(I * two_m - gamma * S)               # (2m)^2 Q, exact enough to order: the acceptance test itself
                    assert np.array_equal(tot, cr.partition_sums(crow, col, w, deg, comm)[0])
                assert all(b > a for a, b in zip(q, q[1:])), (name, weights, gamma, q)
                if last is not None:
                    assert cr.modularity_value(*cr.partition_sums(crow, col, w, deg, tr['states'][0][0])[2:], two_m, gamma) == last
                last = lev['modularity']
                assert len(lev['moved']) == lev['sweeps'] and all(m > 0 for m in lev['moved']) and not lev['hit_max_sweeps']
            assert out['modularity'] == cr.modularity(*cc.graph(name, weights), out['labels'], gamma)


@pytest.mark.parametrize('mutation', cr.MUTATIONS)
def test_each_rule_of_the_sweep_matters(mutation):
    """5. Each rule switched off changes the labels of the 130-, 600- and 2,500-row cases."""
    for name in ('blobs130', 'blobs600', 'blobs2500'):
        changed = False
        for weights in cc.WEIGHTS:
            for gamma in cc.GAMMAS:
                ref = cc.run(name, weights, gamma)['labels']
                got = cr.louvain(*cc.graph(name, weights), gamma=gamma, mutate=mutation, max_sweeps=64)['labels']
                changed |= not np.array_equal(ref, got)
        assert changed, (mutation, name)


def test_max_sweeps_is_reported():
    out = cr.louvain(*cc.graph('blobs2500', 'snn'), gamma=1.0, max_sweeps=1)
    assert out['levels'][0]['hit_max_sweeps'] and out['levels'][0]['sweeps'] == 1


# ---- 7. the errors, without a device -----------------------------------------------------------------------------------------------
def _tgraph(name='blobs130', weights='count'):
    crow, col, w = cc.graph(name, weights)
    return {'crow': torch.as_tensor(crow), 'col': torch.as_tensor(col), 'weight': torch.as_tensor(w), 'n': crow.size - 1}


def test_snn_graph_count_weights_by_torch_match_the_reference():
    from oriana_amd import cluster
    for name in ('blobs130', 'tiny', 'identical'):
        g = cluster.snn_graph(torch.as_tensor(cc.case(name)['indices']), 'count')
        crow, col, w = cc.graph(name, 'count')
        assert g['crow'].dtype == torch.int64 and g['col'].dtype == torch.int32 and g['weight'].dtype == torch.int64
        assert np.array_equal(g['crow'].numpy(), crow) and np.array_equal(g['col'].numpy(), col) and np.array_equal(g['weight'].numpy(), w)
        for gamma in cc.GAMMAS:
            assert cluster.modularity(g, cc.run(name, 'count', gamma)['labels'], gamma) == cc.run(name, 'count', gamma)['modularity']


def test_python_argument_errors(lib):
    from oriana_amd import cluster
    idx = torch.as_tensor(cc.case('blobs130')['indices'])
    for bad in (idx.to(torch.int64), idx[0], idx.numpy()):
        with pytest.raises(ValueError, match='int32'):
            cluster.snn_graph(bad)
    with pytest.raises(ValueError, match='weights'):
        cluster.snn_graph(idx, 'jaccard')
    with pytest.raises(ValueError, match='device'):
        cluster.snn_graph(idx, 'snn')
    with pytest.raises(ValueError, match='exceed'):
        cluster.snn_graph(torch.zeros(4, 200, dtype=torch.int32), 'snn')
    twice = idx.clone()
    twice[7, 3] = twice[7, 0]
    with pytest.raises(ValueError, match='twice'):
        cluster.snn_graph(twice, 'count')

    g = _tgraph()
    for res in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='resolution'):
            cluster.louvain(g, resolution=res)
    for kw in (dict(max_sweeps=0), dict(max_levels=0), dict(blocks=-1)):
        with pytest.raises(ValueError, match='required'):
            cluster.louvain(g, **kw)
    with pytest.raises(ValueError, match='row_cap'):
        cluster.louvain(g, row_cap=0)
    with pytest.raises(ValueError, match='row_cap'):
        cluster.louvain(g, row_cap=cluster.louvain_row_cap() + 1)
    with pytest.raises(ValueError, match='int64'):
        cluster.louvain(dict(g, weight=g['weight'].to(torch.int32)))
    with pytest.raises(ValueError, match='int64'):
        cluster.louvain(dict(g, col=g['col'].to(torch.int64)))
    with pytest.raises(ValueError, match='1-D'):
        cluster.louvain(dict(g, crow=g['crow'][None]))
    with pytest.raises(ValueError, match='dict'):
        cluster.louvain((g['crow'], g['col'], g['weight']))
    w = g['weight'].clone()
    w[0] += 1
    with pytest.raises(ValueError, match='asymmetric'):
        cluster.louvain(dict(g, weight=w))
    col = g['col'].clone()
    a, b = int(g['crow'][0]), int(g['crow'][1])
    assert b - a >= 2
    col[a], col[a + 1] = g['col'][a + 1], g['col'][a]
    with pytest.raises(ValueError, match='unsorted'):
        cluster.louvain(dict(g, col=col))
    one_way = cluster.snn_graph(idx, 'count')
    keep = torch.ones(one_way['col'].numel(), dtype=torch.bool)
    keep[0] = False                                                # one direction of an edge removed: asymmetric pattern
    crow = one_way['crow'].clone()
    crow[1:] -= 1
    with pytest.raises(ValueError, match='asymmetric'):
        cluster.louvain({'crow': crow, 'col': one_way['col'][keep].contiguous(), 'weight': one_way['weight'][keep].contiguous(), 'n': 130})
    with pytest.raises(ValueError, match='negative'):
        cluster.louvain(dict(g, weight=-g['weight']))
    with pytest.raises(ValueError, match='2\\^63'):
        cluster.louvain(dict(g, weight=g['weight'] * (1 << 24)))
    with pytest.raises(ValueError, match='device'):
        cluster.louvain(g)                                         # a valid graph in host memory
    with pytest.raises(ValueError, match='negative'):
        cluster.modularity(dict(g, weight=-g['weight']), np.zeros(130, dtype=np.int64))


def test_more_than_one_rank_is_refused_before_anything_else(monkeypatch):
    from oriana_amd import cluster
    from oriana_amd.models import GaP
    monkeypatch.setattr(cluster.odist, 'world_size', lambda pg=None: 2)
    with pytest.raises(NotImplementedError, match='more than one rank'):
        cluster.louvain(None, pg=object())
    m = object.__new__(GaP)
    m.k, m.pg = 6, object()
    with pytest.raises(NotImplementedError, match='more than one rank'):
        m.cell_communities()
    for kw in (dict(features='bogus'), dict(factors=[6]), dict(pg=None)):
        with pytest.raises(ValueError):
            m.cell_communities(**kw)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from oriana_amd import _lib
    return _lib.load()


_BUF = (ctypes.c_double * 8)()


@pytest.fixture(scope='module')
def p():
    """A 16-byte aligned host address inside _BUF: never dereferenced by a call that fails its argument checks."""
    a = ctypes.addressof(_BUF)
    return a - a % 16 + 16


def test_entry_argument_errors(lib, p):
    """The new entries return ORIANA_EINVAL before any HIP call."""
    from oriana_amd import _lib
    for name in ('oriana_snn_weights', 'oriana_louvain_sweep', 'oriana_louvain_row_cap', 'oriana_louvain_sweep_scratch_bytes_for'):
        assert hasattr(lib, name) and name in _lib.declared_symbols(), name

    def snn(idx=p, n=4, k=3, rp=p, col=p, w=p):
        return lib.oriana_snn_weights(idx, n, k, rp, col, w, None)

    kmax = int(lib.oriana_knn_max_neighbors(1))
    for kw in (dict(n=-1), dict(n=2 ** 31), dict(k=0), dict(k=-2), dict(k=kmax + 1), dict(idx=None), dict(rp=None)):
        assert snn(**kw) == -1, kw
    assert snn(n=0, idx=None, rp=None, col=None, w=None) == 0

    def sweep(n=4, rp=p, col=p, w=p, deg=p, two_m=10, res=1.0, comm=p, tot=p, size=p, cap=0, lrows=None, loff=None, nlong=0,
              scratch=p, sbytes=16, new=p, moved=p, over=p, blocks=0):
        return lib.oriana_louvain_sweep(n, rp, col, w, deg, two_m, res, comm, tot, size, cap, lrows, loff, nlong, scratch, sbytes, new,
                                        moved, over, blocks, None)

    cap = int(lib.oriana_louvain_row_cap())
    assert cap == 128
    for kw in (dict(n=-1), dict(n=2 ** 31), dict(two_m=-1), dict(two_m=3037000500), dict(res=0.0), dict(res=-1.0),
               dict(res=float('nan')), dict(res=float('inf')), dict(cap=-1), dict(cap=cap + 1), dict(blocks=-1), dict(nlong=-1),
               dict(nlong=5, lrows=p, loff=p), dict(nlong=1), dict(nlong=1, lrows=p), dict(nlong=1, loff=p), dict(sbytes=15),
               dict(sbytes=-1), dict(scratch=None), dict(scratch=p + 8), dict(moved=None), dict(over=None), dict(rp=None),
               dict(deg=None), dict(comm=None), dict(tot=None), dict(size=None), dict(new=None)):
        assert sweep(**kw) == -1, kw
    by = lib.oriana_louvain_sweep_scratch_bytes_for
    assert by(-1) == -1 and by(0) == 16 and by(64) == 16 + 16 * 64
