# -*- coding: utf-8 -*-
"""cluster.snn_graph / louvain_sweep / louvain and model.cell_communities on the GPU against the NumPy restatement of
tests/community_reference.py.  Every quantity of a sweep is an integer and the argmax is taken under a total order, so everything
is compared with array_equal: labels, pointers, weights, moved counts; the reported float64 modularity is formed on the host from
the same two integers and must be equal too.  No tolerance appears."""
import numpy as np
import pytest
import torch

import community_cases as cc
import community_reference as cr
from test_markers_gpu import _G, CASES, CASE_IDS

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
LEVEL_KEYS = ('nodes', 'sweeps', 'moved', 'modularity', 'hit_max_sweeps')


def _dev_graph(g):
    crow, col, w = g[0], g[1], g[2]
    return {'crow': torch.as_tensor(crow, device=DEV), 'col': torch.as_tensor(col, device=DEV), 'weight': torch.as_tensor(w, device=DEV),
            'n': crow.size - 1}


def _same_graph(got, ref, what):
    assert got['crow'].dtype == torch.int64 and got['col'].dtype == torch.int32 and got['weight'].dtype == torch.int64, what
    for k, r in zip(('crow', 'col', 'weight'), ref):
        assert np.array_equal(got[k].cpu().numpy(), r), (what, k)


def _same_run(got, ref, what):
    assert got['labels'].dtype == torch.int32 and got['labels'].is_cuda, what
    assert np.array_equal(got['labels'].cpu().numpy(), ref['labels']), what
    assert got['n_communities'] == ref['n_communities'] and got['modularity'] == ref['modularity'], what
    assert [{k: lev[k] for k in LEVEL_KEYS} for lev in got['levels']] == [{k: lev[k] for k in LEVEL_KEYS} for lev in ref['levels']], what


@pytest.mark.parametrize('name', cc.KNN_CASES)
def test_snn_graph_equals_the_reference(name):
    """1. Pointers, columns and weights, both weightings."""
    from oriana_amd import cluster
    idx = torch.as_tensor(cc.case(name)['indices'], device=DEV)
    for weights in cc.WEIGHTS:
        _same_graph(cluster.snn_graph(idx, weights), cc.graph(name, weights), (name, weights))


def test_snn_graph_refuses_a_repeated_neighbour():
    from oriana_amd import cluster
    idx = cc.case('blobs130')['indices'].copy()
    idx[7, 3] = idx[7, 0]
    for weights in cc.WEIGHTS:
        with pytest.raises(ValueError, match='twice'):
            cluster.snn_graph(torch.as_tensor(idx, device=DEV), weights)


# ---- 2. one sweep ------------------------------------------------------------------------------------------------------------------
# (case, level of the reference run, sweep of the level), each on the 'snn' run at resolution 1 and the 'count' run at 2:
# singletons, a mid-level state, the aggregated graph with self entries (from singletons and mid-level), and the two cases
# with long rows at the default cap
STATES = [('blobs2500', 0, 0), ('blobs2500', 0, 2), ('blobs2500', 1, 0), ('blobs2500', 1, 1), ('identical', 0, 0), ('identical', 0, 1),
          ('star', 0, 0), ('noise2000', 0, 1), ('tiny', 0, 0)]


@pytest.mark.parametrize('name,level,at', STATES, ids=['%s-L%d-s%d' % s for s in STATES])
def test_one_sweep_equals_the_reference(name, level, at):
    from oriana_amd import cluster
    for weights, gamma in (('snn', 1.0), ('count', 2.0)):
        tr = cc.run(name, weights, gamma)['trace'][level]
        crow, col, w, deg, two_m = tr['graph']
        comm, tot, size = tr['states'][at]
        want, moved = cr.sweep(crow, col, w, deg, two_m, comm, tot, size, gamma)
        if level > 0:
            assert (cr.graph_rows(crow) == col).any()              # self entries
        g = _dev_graph(tr['graph'])
        d = [torch.as_tensor(x, device=DEV) for x in (deg, comm, tot, size)]
        for cap in (None, 8):
            plan = cluster.louvain_plan(g, cap)
            assert int(plan['long_rows'].numel()) == int((np.diff(crow) > (cap or cluster.louvain_row_cap())).sum())
            for blocks in (0, 1, 3):
                for again in range(2):
                    out = cluster.louvain_sweep(g, d[0], two_m, d[1], d[2], d[3], gamma, plan=plan, blocks=blocks)
                    what = (name, level, at, weights, cap, blocks, again)
                    assert int(out['overflow'][0]) == 0, what
                    assert int(out['moved'][0]) == moved, what
                    assert out['comm'].dtype == torch.int32 and np.array_equal(out['comm'].cpu().numpy(), want), what
        if name == 'identical' or level > 0 or at > 0:
            assert moved > 0
    if name in ('identical', 'star'):
        assert np.diff(crow).max() > cluster.louvain_row_cap()     # long rows without forcing


# ---- 3. the full run ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', cc.ALL_CASES)
def test_louvain_equals_the_reference(name):
    """Labels, per-level node counts, sweep counts, moved lists and modularity; the same bits at row_cap = 8."""
    from oriana_amd import cluster
    for weights in cc.WEIGHTS:
        g = _dev_graph(cc.graph(name, weights))
        for gamma in cc.GAMMAS:
            ref = cc.run(name, weights, gamma)
            _same_run(cluster.louvain(g, resolution=gamma), ref, (name, weights, gamma))
            _same_run(cluster.louvain(g, resolution=gamma, row_cap=8, blocks=3), ref, (name, weights, gamma, 'row_cap=8'))
            assert cluster.modularity(g, ref['labels'], gamma) == ref['modularity']


def test_max_sweeps_and_max_levels_are_honoured():
    from oriana_amd import cluster
    g = _dev_graph(cc.graph('blobs2500', 'snn'))
    _same_run(cluster.louvain(g, max_sweeps=1), cr.louvain(*cc.graph('blobs2500', 'snn'), max_sweeps=1), 'max_sweeps=1')
    out = cluster.louvain(g, max_sweeps=1)
    assert out['levels'][0]['hit_max_sweeps'] and out['levels'][0]['sweeps'] == 1
    _same_run(cluster.louvain(g, max_levels=1), cr.louvain(*cc.graph('blobs2500', 'snn'), max_levels=1), 'max_levels=1')


# ---- 4. a scratch that is too small ------------------------------------------------------------------------------------------------
def test_a_scratch_one_byte_short_sets_the_flag_and_writes_nothing():
    from oriana_amd import cluster, _lib
    lib = _lib.load()
    tr = cc.run('identical', 'snn', 1.0)['trace'][0]
    crow, col, w, deg, two_m = tr['graph']
    comm, tot, size = tr['states'][0]
    g = _dev_graph(tr['graph'])
    d = [torch.as_tensor(x, device=DEV) for x in (deg, comm, tot, size)]
    plan = cluster.louvain_plan(g, 8)
    need = plan['scratch_bytes']
    assert need == int(lib.oriana_louvain_sweep_scratch_bytes_for(plan['slots'])) and plan['slots'] >= 64 * 600
    n, guard = crow.size - 1, 4096
    want, moved = cr.sweep(crow, col, w, deg, two_m, comm, tot, size, 1.0)
    for nbytes, over in ((need, 0), (need - 1, 1)):
        buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
        new = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        mv = torch.full((1,), -9, dtype=torch.int64, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        rc = lib.oriana_louvain_sweep(n, _lib.ptr(g['crow']), _lib.ptr(g['col']), _lib.ptr(g['weight']), _lib.ptr(d[0]), two_m, 1.0,
                                      _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), 8, _lib.ptr(plan['long_rows']),
                                      _lib.ptr(plan['long_off']), int(plan['long_rows'].numel()), _lib.ptr(buf), nbytes, _lib.ptr(new),
                                      _lib.ptr(mv), _lib.ptr(flag), 0, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and int(flag[0]) == over
        assert bool((buf[need:] == 0xA5).all())                    # the guard band behind the scratch
        if over:
            assert bool((new == -7).all()) and int(mv[0]) == -9
        else:
            assert np.array_equal(new.cpu().numpy(), want) and int(mv[0]) == moved
    with pytest.raises(_lib.OrianaHipError, match='scratch'):
        cluster.louvain(g, row_cap=8, scratch=torch.empty(need - 1, dtype=torch.uint8, device=DEV))
    _same_run(cluster.louvain(g, row_cap=8, scratch=torch.empty(need, dtype=torch.uint8, device=DEV)), cc.run('identical', 'snn', 1.0),
              'own scratch')


# ---- 5. - 7. the models ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,dd', CASES, ids=CASE_IDS)
def test_cell_communities(name, dd):
    from oriana_amd import cluster
    G = _G(name, dd)
    before, fac = G.state(), G.factors()
    k = 12
    out = G.cell_communities(n_neighbors=k)
    nb = G.cell_neighbors(k)
    idx = torch.as_tensor(nb['indices'], device=G.device)
    direct = cluster.louvain(cluster.snn_graph(idx))
    ref = cr.louvain(*cr.snn_graph(nb['indices']))
    _same_run(out, ref, name)
    _same_run(direct, ref, name)
    _same_run(G.cell_communities(graph=(nb['indices'], nb['sq_distances'])), ref, 'graph=')
    _same_run(G.cell_communities(graph=(idx, None), row_cap=8, blocks=2), ref, 'graph= on the device')
    for weights, gamma in (('count', 1.0), ('snn', 2.0)):
        _same_run(G.cell_communities(n_neighbors=k, weights=weights, resolution=gamma),
                  cr.louvain(*cr.snn_graph(nb['indices'], weights), gamma=gamma), (name, weights, gamma))
    cols = np.array([2, 0])
    sub = G.cell_neighbors(k, factors=cols)
    assert not np.array_equal(sub['indices'], nb['indices'])
    _same_run(G.cell_communities(n_neighbors=k, factors=cols), cr.louvain(*cr.snn_graph(sub['indices'])), 'factors=')
    after, fac2 = G.state(), G.factors()
    assert sorted(before) == sorted(after)
    for key in before:
        assert np.array_equal(before[key], after[key], equal_nan=True), key
    for x, y in zip(fac, fac2):
        assert np.array_equal(x, y)
    # 6. the labels feed the other cell functions as they are
    sil = G.cell_silhouette(out['labels'])
    assert sil['counts'].sum() == G.n and len(sil['counts']) == out['n_communities'] and np.isfinite(sil['mean'])
    mk = G.marker_genes(out['labels'])
    assert len(mk['sizes']) == out['n_communities'] and np.array_equal(mk['sizes'], sil['counts'])


def test_more_than_one_rank_is_refused(monkeypatch):
    """7. Before any launch: the graph is never looked at."""
    from oriana_amd import cluster
    G = _G('GaP', None)
    monkeypatch.setattr(cluster.odist, 'world_size', lambda pg=None: 2)
    with pytest.raises(NotImplementedError, match='more than one rank'):
        cluster.louvain({'crow': None}, pg=object())
    with pytest.raises(NotImplementedError, match='more than one rank'):
        G.cell_communities()
