# -*- coding: utf-8 -*-
"""cluster.louvain_sweep() with a scratch that is too small: the sweep writes nothing, so the proposed labelling it returns must be a
valid one -- cluster.louvain() sums over it (index_add_, bincount) before the host reads the overflow flag."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_an_overflowing_sweep_returns_the_labelling_it_was_given():
    from oriana_amd import cluster, _lib
    g0 = torch.Generator()
    g0.manual_seed(3)
    Y = torch.randn(300, 3, generator=g0).cuda()
    graph = cluster.snn_graph(cluster.knn(Y, 8)['indices'])
    _, _, w, n, rows, deg, two_m = cluster._check_graph(graph)
    plan = cluster.louvain_plan(graph, 1)                           # row_cap = 1: every row of the graph has a table in the scratch
    assert plan['slots'] >= 64 * n
    comm = torch.randperm(n, generator=g0).to(torch.int32).cuda()   # any labelling within [0, n)
    tot = torch.zeros(n, dtype=torch.int64, device='cuda').index_add_(0, comm.to(torch.int64), deg)
    size = torch.bincount(comm.to(torch.int64), minlength=n).to(torch.int32)
    short = torch.empty(plan['scratch_bytes'] - 1, dtype=torch.uint8, device='cuda')
    out = cluster.louvain_sweep(graph, deg, two_m, comm, tot, size, plan=plan, scratch=short)
    torch.cuda.synchronize()
    assert int(out['overflow'][0]) == 1 and int(out['moved'][0]) == 0
    assert torch.equal(out['comm'], comm)
    with pytest.raises(_lib.OrianaHipError, match='scratch'):
        cluster.louvain(graph, row_cap=1, scratch=short)
    torch.cuda.synchronize()
