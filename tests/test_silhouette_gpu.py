# -*- coding: utf-8 -*-
"""oriana_cluster_distance_sums, cluster.silhouette and model.cell_silhouette on the GPU against the float64 restatement of
tests/silhouette_reference.py, under the bounds derived there (none of them measured on the kernel)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import kmeans_reference as kr
import silhouette_reference as sr

pytestmark = pytest.mark.gpu


def _dev(Y, extra=0):
    """Y on the device, optionally as the leading columns of a wider matrix (row stride d + extra) whose other columns are NaN."""
    n, d = Y.shape
    if not extra:
        return torch.from_numpy(Y).cuda()
    wide = torch.full((n, d + extra), float('nan'), dtype=torch.float32, device='cuda')
    wide[:, :d] = torch.from_numpy(Y).cuda()
    return wide[:, :d]


def _sums(Y, labels, C, extra=0, Q=None, **kw):
    """S (C, nq) by one raw call: the candidates grouped by label on the host (row stride d + extra), the queries Q or Y as they lie."""
    from oriana_amd import cluster
    order = np.argsort(labels, kind='stable')
    off = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=C))])
    S = cluster.distance_sums(_dev(Y if Q is None else Q, extra), _dev(np.ascontiguousarray(Y[order]), extra), off, **kw)
    torch.cuda.synchronize()
    assert S.is_cuda and S.dtype == torch.float64 and tuple(S.shape) == (C, (Y if Q is None else Q).shape[0])
    return S.cpu().numpy()


def _silhouette(Yd, labels, **kw):
    from oriana_amd import cluster
    o = cluster.silhouette(Yd, labels, **kw)
    torch.cuda.synchronize()
    assert all(o[k].is_cuda and o[k].dtype == torch.float64 for k in ('values', 'a', 'b'))
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in o.items()}


def _check_summary(res, ref, C):
    _, counts, values, _, _ = ref
    assert res['counts'].dtype == np.int64 and np.array_equal(res['counts'], counts)
    n = values.size                                               # (a float64 sum of n values of at most 1: n 2^-52 whatever the order)
    assert isinstance(res['mean'], float) and abs(res['mean'] - res['values'].mean()) <= n * 2.0 ** -52
    lab_means = res['cluster_means']
    assert lab_means.shape == (C,) and np.array_equal(np.isnan(lab_means), counts == 0)


@pytest.mark.parametrize('case', sr.CASES, ids=[c[0] for c in sr.CASES])
def test_single_call(case):
    name, n, d, C, extra, _ = case
    Y, labels = sr.case_inputs(case)
    ref = sr.silhouette(Y, labels, C)
    S = _sums(Y, labels, C, extra)
    sr.check_sums(S, ref[0], n, d, name)
    res = _silhouette(_dev(Y, extra), labels if name != 'padded_image' else torch.from_numpy(labels).cuda(), n_clusters=C)
    sr.check_result(res, ref, n, d, name)
    _check_summary(res, ref, C)
    for c in range(C):
        if ref[1][c]:
            assert abs(res['cluster_means'][c] - res['values'][labels == c].mean()) <= n * 2.0 ** -52
    if name == 'edges':
        single = labels == 0
        assert res['values'][single].tolist() == [0.0] and res['a'][single].tolist() == [0.0] and np.all(S[4] == 0.0)
        assert np.isnan(res['cluster_means'][4]) and res['cluster_means'][0] == 0.0


def test_exact_zeros():
    Y, labels = sr.zeros_case()
    n, d = Y.shape
    ref = sr.silhouette(Y, labels, 4)
    assert (ref[0] == 0.0).sum() == 22 * 2                         # the repeated point's rows against both of its clusters
    S = _sums(Y, labels, 4)
    sr.check_sums(S, ref[0], n, d, 'zeros')
    assert np.array_equal(S == 0.0, ref[0] == 0.0)
    res = _silhouette(_dev(Y), labels)
    sr.check_result(res, ref, n, d, 'zeros')
    rep = labels <= 1
    assert np.all(res['values'][rep] == 0.0) and np.all(res['a'][rep] == 0.0) and np.all(res['b'][rep] == 0.0)
    assert not np.isnan(res['values']).any() and not np.isnan(res['cluster_means']).any()


def test_raw_call_accumulates_and_leaves_the_padding_alone():
    from oriana_amd import cluster
    n, nq, d, C, lds = 300, 70, 20, 5, 77
    Y, which, _ = kr.blobs(41, n, d, C)
    Q = kr.blobs(42, nq, d, C)[0]
    labels = which.astype(np.int64)
    S_ref = sr.distance_sums(Y, labels, C, Q=Q)
    sr.check_sums(_sums(Y, labels, C, Q=Q), S_ref, n, d, 'separate queries')
    rng = np.random.default_rng(43)
    fill = rng.normal(size=(C, lds)) * 1e4
    big = torch.from_numpy(fill.copy()).cuda()
    order = np.argsort(labels, kind='stable')
    off = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=C))])
    out = cluster.distance_sums(_dev(Q), _dev(np.ascontiguousarray(Y[order])), off, sums=big[:, :nq], accumulate=True)
    torch.cuda.synchronize()
    assert out.data_ptr() == big.data_ptr()
    got = big.cpu().numpy()
    assert got[:, nq:].tobytes() == fill[:, nq:].tobytes()        # the sentinel columns, bit for bit
    want = fill[:, :nq] + S_ref
    # the sums within their bound, then one float64 addition onto what was there
    assert np.all(np.abs(got[:, :nq] - want) <= sr.eps_sums(n, d) * S_ref + 2.0 ** -53 * np.abs(want))
    # without accumulate the same view is overwritten, the padding still untouched
    cluster.distance_sums(_dev(Q), _dev(np.ascontiguousarray(Y[order])), off, sums=big[:, :nq])
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert got[:, nq:].tobytes() == fill[:, nq:].tobytes()
    sr.check_sums(np.ascontiguousarray(got[:, :nq]), S_ref, n, d, 'overwritten view')


@pytest.fixture(scope='module')
def base():
    c = sr.PARTITION_CASE
    Y, which, _ = kr.blobs(c['seed'], c['n'], c['d'], c['n_blobs'])
    labels = which.astype(np.int64)
    return Y, labels, _dev(Y), sr.silhouette(Y, labels, c['n_blobs'])


def test_partitions(base):
    Y, labels, Yd, ref = base
    n, d = Y.shape
    C = sr.PARTITION_CASE['n_blobs']
    first = _silhouette(Yd, labels)
    sr.check_result(first, ref, n, d, 'default')
    again = _silhouette(Yd, labels)
    for k in ('values', 'a', 'b'):
        assert again[k].tobytes() == first[k].tobytes(), k        # the same call twice: the same bits
    S0 = _sums(Y, labels, C)
    assert _sums(Y, labels, C).tobytes() == S0.tobytes()
    sr.check_sums(S0, ref[0], n, d, 'blocks=0')
    ep = sr.eps_partition(n)
    for blocks in (1, 3):
        S = _sums(Y, labels, C, blocks=blocks)
        sr.check_sums(S, ref[0], n, d, 'blocks=%d' % blocks)
        assert np.all(np.abs(S - S0) <= ep * S0), blocks

    def within(res, what):
        sr.check_result(res, ref, n, d, what)                      # each partition on its own within the reference bound
        e = ep + 2.0 ** -52
        for k in ('a', 'b'):
            assert np.all(np.abs(res[k] - first[k]) <= e * first[k]), (what, k)
        assert np.abs(res['values'] - first['values']).max() <= sr.tol_values(e), what
        assert np.array_equal(res['counts'], first['counts'])

    for blocks in (0, 1, 3):
        within(_silhouette(Yd, labels, blocks=blocks), 'blocks=%d' % blocks)
    for chunk in (64, 100, 699):
        within(_silhouette(Yd, labels, candidate_chunk=chunk), 'candidate_chunk=%d' % chunk)
    for qb in (64, 100):
        within(_silhouette(Yd, labels, query_block=qb), 'query_block=%d' % qb)
    within(_silhouette(Yd, labels, query_block=192, candidate_chunk=300, blocks=3), 'query_block=192, candidate_chunk=300, blocks=3')


def test_errors_before_a_launch(monkeypatch):
    from oriana_amd import cluster
    calls = []
    monkeypatch.setattr(cluster, 'distance_sums', lambda *a, **k: calls.append(1) or (_ for _ in ()).throw(AssertionError('launched')))
    Y = torch.randn(50, 100, device='cuda')
    lab = torch.arange(50, device='cuda') % 4
    bad = Y.clone()
    bad[7, 3] = float('inf')
    for args, kw in (((bad, lab), {}), ((Y, lab - 1), {}), ((Y, lab[:49]), {}), ((Y, lab.double()), {}), ((Y.double(), lab), {}),
                     ((Y[0], lab), {}), ((Y.cpu(), lab), {}), ((Y.t(), lab), {}), ((Y, lab * 0), {}), ((Y, torch.arange(50)), {}),
                     ((Y, lab), dict(n_clusters=3)), ((Y, lab), dict(n_clusters=cluster.max_clusters() + 1)),
                     ((torch.randn(50, 300, device='cuda'), lab), {})):
        with pytest.raises(ValueError):
            cluster.silhouette(*args, **kw)
    assert not calls


@pytest.mark.parametrize('name', ['GaP', 'SparseZIGaP'])
def test_cell_silhouette_is_silhouette_on_the_features_and_leaves_the_state_alone(name):
    from oriana_amd import cluster
    from test_cluster_cells_gpu import build_model, N_CELLS, K
    model = build_model(name)
    order = model.factor_order()
    cc = model.cluster_cells(3, n_init=2, seed=0)
    before = model.state()
    runs = [(dict(), model.cell_silhouette(cc['labels'])),
            (dict(features='mean_log'), model.cell_silhouette(cc['labels'], features='mean_log')),
            (dict(factors=order[:3]), model.cell_silhouette(cc['labels'], factors=order[:3], candidate_chunk=100, blocks=2))]
    after = model.state()
    assert sorted(before) == sorted(after)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    assert np.array_equal(runs[0][1]['features'], cc['features']) and np.array_equal(runs[0][1]['factors'], np.arange(K))
    assert np.array_equal(runs[2][1]['factors'], np.asarray(order[:3])) and runs[2][1]['features'].shape == (N_CELLS, 3)
    for kw, res in runs:
        F = res['features']
        n, d = F.shape
        assert F.dtype == np.float32 and all(res[k].dtype == np.float64 and res[k].shape == (N_CELLS,) for k in ('values', 'a', 'b'))
        part = {k: v for k, v in kw.items() if k != 'features' and k != 'factors'}
        direct = cluster.silhouette(torch.from_numpy(F).cuda(), cc['labels'], **(dict(candidate_chunk=100, blocks=2) if 'factors' in kw else part))
        for k in ('values', 'a', 'b'):
            assert direct[k].cpu().numpy().tobytes() == res[k].tobytes(), (kw, k)
        assert direct['mean'] == res['mean'] and np.array_equal(direct['counts'], res['counts'])
        ref = sr.silhouette(F, cc['labels'].astype(np.int64), 3)
        sr.check_result(res, ref, n, d, '%s %s' % (name, sorted(kw)))
        print('%s %s: mean silhouette of cluster_cells(3) %.4f' % (name, sorted(kw), res['mean']))
    with pytest.raises(ValueError):
        model.cell_silhouette(cc['labels'], pg=None)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_match_one(tmp_path):
    from oriana_amd import cluster
    from test_cluster_cells_gpu import N_CELLS, K
    world, port, out = 2, _free_port(), str(tmp_path / 'cs')
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cell_silhouette_worker.py')
    procs = [subprocess.Popen(['timeout', '-k', '10', '150', sys.executable, worker, str(r), str(world), str(port), out])
             for r in range(world)]
    codes = [p.wait() for p in procs]
    assert codes == [0, 0], codes
    got = [np.load(out + '.rank%d.npz' % r) for r in range(world)]
    F = np.concatenate([got[0]['features'], got[1]['features']])
    labels = np.concatenate([got[0]['labels'], got[1]['labels']])
    assert F.shape == (N_CELLS, K) and labels.shape == (N_CELLS,)
    # one process on the very features and labels the two ranks used
    single = _silhouette(torch.from_numpy(F).cuda(), labels, n_clusters=3)
    e = sr.eps_partition(N_CELLS) + 2.0 ** -52
    for prefix in ('', 'chunked_'):
        assert np.array_equal(got[0][prefix + 'counts'], got[1][prefix + 'counts'])
        assert np.array_equal(got[0][prefix + 'counts'], single['counts'])
        assert got[0][prefix + 'mean'] == got[1][prefix + 'mean'] and abs(float(got[0][prefix + 'mean']) - single['mean']) <= sr.tol_values(e)
        assert np.array_equal(got[0][prefix + 'cluster_means'], got[1][prefix + 'cluster_means'])
        for k in ('a', 'b'):
            v = np.concatenate([got[0][prefix + k], got[1][prefix + k]])
            assert np.all(np.abs(v - single[k]) <= e * single[k]), (prefix, k)
        v = np.concatenate([got[0][prefix + 'values'], got[1][prefix + 'values']])
        assert np.abs(v - single['values']).max() <= sr.tol_values(e), prefix
    sr.check_result(single, sr.silhouette(F, labels, 3), N_CELLS, K, 'two ranks, one process')
