# -*- coding: utf-8 -*-
"""model.cell_neighbors() on the GPU: the graph is cluster.knn on the feature matrix cluster_cells() uses, the model's state is
untouched, folded-in cells are searched against the fitted ones, and two row-sharded ranks agree with one bit for bit."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import knn_reference as nr
from test_cluster_cells_gpu import build_model, N_CELLS, N_GENES, K

pytestmark = pytest.mark.gpu


def _own_label_share(indices, labels):
    ok = indices >= 0
    return float((labels[np.where(ok, indices, 0)] == labels[:, None])[ok].mean())


@pytest.mark.parametrize('name', ['GaP', 'SparseZIGaP'])
def test_cell_neighbors_is_knn_on_the_features_and_leaves_the_state_alone(name):
    from oriana_amd import cluster
    model = build_model(name)
    before = model.state()
    order = model.factor_order()
    runs = [(dict(), model.cell_neighbors()), (dict(features='mean_log'), model.cell_neighbors(10, features='mean_log')),
            (dict(factors=order[:3]), model.cell_neighbors(15, factors=order[:3], candidate_chunk=100, blocks=2))]
    after = model.state()
    assert sorted(before) == sorted(after)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    for (kw, res), kk in zip(runs, (15, 10, 15)):
        cc = model.cluster_cells(3, n_init=1, max_iter=1, seed=0, **kw)
        assert np.array_equal(res['features'], cc['features']) and np.array_equal(res['factors'], cc['factors'])
        F = res['features']
        assert F.dtype == np.float32 and res['indices'].dtype == np.int32 and res['sq_distances'].dtype == np.float32
        assert res['indices'].shape == (N_CELLS, kk) and res['sq_distances'].shape == (N_CELLS, kk)
        direct = cluster.knn(torch.from_numpy(F).cuda(), kk)
        assert np.array_equal(direct['indices'].cpu().numpy(), res['indices'])
        assert np.array_equal(direct['sq_distances'].cpu().numpy(), res['sq_distances'])
        share = nr.check(F, res['indices'], res['sq_distances'], kk, exclude=True, what='%s %s' % (name, kw))
        print('%s %s: non-clear share %.2e, neighbours with the cell\'s own generator label %.4f'
              % (name, sorted(kw), share, _own_label_share(res['indices'], model.generator_labels)))
    assert np.array_equal(runs[2][1]['factors'], np.asarray(order[:3])) and runs[2][1]['features'].shape == (N_CELLS, 3)
    assert np.array_equal(runs[0][1]['factors'], np.arange(K))


def test_queries_from_transform():
    from oriana_amd.singlecell.generation import SyntheticCounts
    model = build_model('GaP')
    gen = SyntheticCounts(N_CELLS, N_GENES, K, seed=4, device='cuda:0', n_groups=3)
    X_new = gen.chunk(100, 170)
    before = model.state()
    E = model.transform(X_new)
    order = model.factor_order()
    for kw in (dict(), dict(factors=order[:4])):
        res = model.cell_neighbors(15, queries=E, **kw)
        cols = res['factors']
        Qf = np.log(np.asarray(E, dtype=np.float64)).astype(np.float32)[:, cols]
        assert res['indices'].shape == (70, 15) and np.array_equal(res['features'], model.cell_neighbors(1, **kw)['features'])
        share = nr.check(res['features'], res['indices'], res['sq_distances'], 15, Q=Qf, what='transform queries')
        labels = gen.labels(100, 170).cpu().numpy()
        own = float((model.generator_labels[res['indices']] == labels[:, None]).mean())
        print('queries %s: non-clear share %.2e, neighbours with the query\'s generator label %.4f' % (sorted(kw), share, own))
    # a tensor works like an array; the fitted cells' own E[U] find themselves first (nothing is excluded)
    own = model.cell_neighbors(2, queries=torch.from_numpy(model.U_hat[:9]))
    assert np.array_equal(own['indices'][:, 0], np.arange(9)) and np.all(own['sq_distances'][:, 0] == 0.0)
    after = model.state()
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    with pytest.raises(ValueError):
        model.cell_neighbors(15, queries=E, features='mean_log')
    with pytest.raises(ValueError):
        model.cell_neighbors(15, pg=None)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_match_one_bit_for_bit(tmp_path):
    world, port, out = 2, _free_port(), str(tmp_path / 'cn')
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cell_neighbors_worker.py')
    procs = [subprocess.Popen(['timeout', '-k', '10', '150', sys.executable, worker, str(r), str(world), str(port), out])
             for r in range(world)]
    codes = [p.wait() for p in procs]
    assert codes == [0, 0], codes
    got = [np.load(out + '.rank%d.npz' % r) for r in range(world)]
    from oriana_amd import cluster
    F = np.concatenate([got[0]['features'], got[1]['features']])
    idx = np.concatenate([got[0]['indices'], got[1]['indices']])
    d2 = np.concatenate([got[0]['sq_distances'], got[1]['sq_distances']])
    assert F.shape == (N_CELLS, K) and idx.shape == (N_CELLS, 15)
    # one process on the very features the two ranks searched (the sharded FIT differs from a one-rank fit in summation order,
    # which tests/test_sharded_gpu.py covers)
    single = cluster.knn(torch.from_numpy(F).cuda(), 15)
    si, sd = single['indices'].cpu().numpy(), single['sq_distances'].cpu().numpy()
    assert np.array_equal(idx, si) and d2.tobytes() == sd.tobytes()
    assert (idx[:got[0]['indices'].shape[0]] >= got[0]['indices'].shape[0]).any()      # (neighbours across the shards)
    ci = np.concatenate([got[0]['chunked_indices'], got[1]['chunked_indices']])
    cd = np.concatenate([got[0]['chunked_sq_distances'], got[1]['chunked_sq_distances']])
    assert np.array_equal(ci, si) and cd.tobytes() == sd.tobytes()
    for r in range(world):                      # each rank's own queries against all cells: a cell's E[U] finds the cell itself
        r0 = int(got[r]['row0'])
        assert np.array_equal(got[r]['query_indices'][:, 0], r0 + np.arange(7)), r
        assert np.all(got[r]['query_sq_distances'][:, 0] == 0.0)
        q = cluster.knn(torch.from_numpy(F).cuda(), 4, queries=torch.from_numpy(got[r]['features'][:7]).cuda())
        assert np.array_equal(q['indices'].cpu().numpy(), got[r]['query_indices'])
        assert q['sq_distances'].cpu().numpy().tobytes() == got[r]['query_sq_distances'].tobytes()
