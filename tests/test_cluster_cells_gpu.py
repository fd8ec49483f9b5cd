# -*- coding: utf-8 -*-
"""model.cluster_cells() on the GPU: the labels replay through the float64 restatement of tests/kmeans_reference.py from the
same starts, the model's state is untouched, and two row-sharded ranks agree with one."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import kmeans_reference as kr

pytestmark = pytest.mark.gpu

N_CELLS, N_GENES, K = 420, 300, 6


def build_model(name, r0=0, r1=N_CELLS, pg=None):
    """20 sweeps of `name` on rows [r0, r1) of the device generator's counts (3 groups), from its seeded start."""
    import oriana_amd.models as M
    from oriana_amd.singlecell.generation import SyntheticCounts
    gen = SyntheticCounts(N_CELLS, N_GENES, K, seed=4, device='cuda:0', n_groups=3, row0=r0, n=r1 - r0)
    X = gen.chunk(0, r1 - r0)
    a1, b1 = gen.initial_shapes()
    model = getattr(M, name)(X, k=K, init=(a1, b1), device='cuda:0', process_group=pg, n_total=N_CELLS)
    model.fit(20)
    model.generator_labels = gen.labels(0, r1 - r0).cpu().numpy()
    return model


def _replay(res):
    """Every restart of a cluster_cells() result against lloyd() on the returned features from the same starts."""
    from oriana_amd import cluster
    F = res['features']
    n, d = F.shape
    Fd = torch.from_numpy(F).cuda()
    T = cluster.partial_rows()
    for r in range(res['init_centers'].shape[0]):
        labels, centers, inertia, n_iter, conv, near, scale = kr.lloyd(F, res['init_centers'][r], 300, 1e-4)
        print('restart %d: near-tie share %.2e' % (r, near.mean()))
        assert near.mean() <= kr.NEAR_TIE_CAP
        got = cluster.lloyd_step(Fd, torch.from_numpy(res['all_centers'][r:r + 1].astype(np.float32)).cuda(), label_restart=0)
        got = got['labels'].cpu().numpy().astype(np.int64)
        rel = (d + 3) * kr.U + n * 2.0 ** -52
        if np.array_equal(got, labels):
            bound = ((T - 1) * kr.U + n * 2.0 ** -52) * scale + 2.0 ** -52 * np.abs(centers)
            assert np.all(np.abs(res['all_centers'][r] - centers) <= bound)
            assert res['n_iters'][r] == n_iter and bool(res['converged'][r]) == conv
            assert abs(res['inertias'][r] - inertia) <= 2 * rel * inertia
        else:
            assert not np.any((got != labels) & ~near)
            assert abs(res['inertias'][r] - inertia) <= (2 * rel + 4 * (d + 3) * kr.U) * inertia
        if r == res['best']:
            assert np.array_equal(res['labels'].astype(np.int64), got)


@pytest.mark.parametrize('name', ['GaP', 'SparseZIGaP'])
def test_cluster_cells_replays_and_leaves_the_state_alone(name):
    model = build_model(name)
    before = model.state()
    order = model.factor_order()
    runs = [model.cluster_cells(3, n_init=4, seed=0), model.cluster_cells(3, features='mean_log', n_init=4, seed=0),
            model.cluster_cells(3, factors=order[:3], n_init=4, seed=0)]
    after = model.state()
    assert sorted(before) == sorted(after)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    U_hat, logU = before['U_hat'], before['log_U_hat']
    assert np.array_equal(runs[0]['features'], np.log(U_hat).astype(np.float32)) or \
        np.allclose(runs[0]['features'], np.log(U_hat).astype(np.float32), rtol=2 ** -22, atol=0)
    assert np.array_equal(runs[1]['features'], logU)
    assert np.array_equal(runs[2]['factors'], np.asarray(order[:3])) and runs[2]['features'].shape == (N_CELLS, 3)
    assert np.array_equal(runs[0]['factors'], np.arange(K))
    for what, res in zip(('log_mean', 'mean_log', 'three factors'), runs):
        assert res['features'].dtype == np.float32 and res['labels'].shape == (N_CELLS,)
        _replay(res)
        print('%s %s: ARI against the generator\'s groups %.4f' % (name, what,
                                                                    kr.adjusted_rand_index(res['labels'], model.generator_labels)))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_match_one(tmp_path):
    world, port, out = 2, _free_port(), str(tmp_path / 'cc')
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cluster_cells_worker.py')
    procs = [subprocess.Popen(['timeout', '-k', '10', '150', sys.executable, worker, str(r), str(world), str(port), out])
             for r in range(world)]
    codes = [p.wait() for p in procs]
    assert codes == [0, 0], codes
    got = [np.load(out + '.rank%d.npz' % r) for r in range(world)]
    for k in ('all_centers', 'inertias', 'centers', 'init_centers', 'n_iters', 'converged'):
        assert np.array_equal(got[0][k], got[1][k]), k                        # every rank returns the same centres and inertias
    assert int(got[0]['best']) == int(got[1]['best'])
    from oriana_amd import cluster
    labels = np.concatenate([got[0]['labels'], got[1]['labels']])
    F = np.concatenate([got[0]['features'], got[1]['features']])
    assert F.shape == (N_CELLS, K) and labels.shape == (N_CELLS,)
    # one rank on the very features the two ranks clustered (the sharded FIT differs from a one-rank fit in summation order,
    # which tests/test_sharded_gpu.py covers): the same starts, the same restart wins, the same labels outside near-ties
    single = cluster.kmeans(torch.from_numpy(F).cuda(), 3, n_init=4, seed=0)
    assert np.array_equal(single['init_centers'], got[0]['init_centers'])
    assert single['best'] == int(got[0]['best'])
    assert np.array_equal(single['n_iters'], got[0]['n_iters']) and np.array_equal(single['converged'], got[0]['converged'])
    T = cluster.partial_rows()
    for r in range(4):                          # (both runs are within the step's bound of the float64 restatement)
        centers, scale = kr.lloyd(F, single['init_centers'][r], 300, 1e-4)[1::5]
        bound = 2 * (((T - 1) * kr.U + N_CELLS * 2.0 ** -52) * scale + 2.0 ** -52 * np.abs(centers))
        assert np.all(np.abs(got[0]['all_centers'][r] - single['all_centers'][r]) <= bound), r
    rel = 2 * ((K + 3) * kr.U + N_CELLS * 2.0 ** -52)
    assert np.all(np.abs(got[0]['inertias'] - single['inertias']) <= 2 * rel * single['inertias'])
    near = kr.lloyd(F, single['init_centers'][single['best']], 300, 1e-4)[5]
    print('two ranks: near-tie share %.2e' % near.mean())
    assert near.mean() <= kr.NEAR_TIE_CAP
    assert np.array_equal(labels[~near], single['labels'][~near])
