# -*- coding: utf-8 -*-
"""factor_order() / deviance_path() of every model on both layouts against the float64 restatement of
tests/deviance_path_reference.py, evaluated on the model's own state (X as the float32 counts it holds, U_hat,
V_eff = V_hat * S_hat and pi_d in float64, D_hat as the float32 values it holds).  The tolerances are derived there, never
measured on the code under test; an infinite reference value is matched exactly."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import deviance_path_reference as dr

pytestmark = pytest.mark.gpu

N_ROWS = 3 * 256 + 37            # a partial last row tile
M_COLS = 301                     # not a multiple of 4; two column tiles, the last one partial
DENSE_DENSITY = 0.5
KP = {1: 16, 20: 20, 50: 52, 100: 100, 129: 160, 200: 224}
ALL_MODELS = ('GaP', 'ZIGaP', 'SparseGaP', 'SparseZIGaP')


def _counts(seed, n=N_ROWS, m=M_COLS):
    """Integer counts: 70 genes at 80 % (a dense block under dense_density = 0.5), the rest at 15 %; an all-zero gene (5), an
    all-zero cell (11), a gene expressed in every other cell (250)."""
    rng = np.random.default_rng(seed)
    dens = np.full(m, 0.15)
    dens[:70] = 0.8
    X = ((rng.poisson(rng.gamma(0.6, 4.0, size=(n, m))) + 1) * (rng.random((n, m)) < dens)).astype(np.float64)
    X[:, 250] = rng.poisson(6.0, size=n) + 1
    X[:, 5] = 0
    X[11, :] = 0
    return X


def _model(name, X, K, dense_density=None, seed=0, **kw):
    import oriana_amd.models as M
    rng = np.random.default_rng(1000 + seed)
    n, m = X.shape
    a1 = rng.gamma(1.0, 1.0, size=(n, K))
    b1 = rng.gamma(1.0, 1.0, size=(m, K))
    G = getattr(M, name)(X, k=K, init=(a1, b1), dense_density=dense_density, **kw)
    if dense_density:
        assert G.counts.gd >= 32 and G.counts.dense is not None, 'the hybrid case has no dense block'
    else:
        assert G.counts.gd == 0
    return G


def _inputs(G, X):
    """What the reference evaluates: the model's own state on the host."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    m = X.shape[1]
    U = G.U_hat
    V = G.V_hat * G.S_hat.astype(np.float64) if G.sparse else G.V_hat
    pi = G.pi_d[:] if G.zi else np.ones(m)
    keep0 = (X == 0) & (np.round(G.D_hat.astype(np.float64)) != 0) if G.zi else (X == 0)
    f32_cols = np.ones(m, dtype=bool)                   # the dense genes of a hybrid layout are evaluated in float64
    if G.counts.gd:
        f32_cols[G.counts.col_perm.cpu().numpy()[:G.counts.gd]] = False
    return X, U, V, pi, keep0, f32_cols


def _reference(G, X, order, ks=None):
    X, U, V, pi, keep0, f32_cols = _inputs(G, X)
    ks = np.arange(1, G.k + 1) if ks is None else np.asarray(ks)
    return dr.path(X, U, V, pi, keep0, order, ks, G.zi, f32_cols=f32_cols)


def _mass_order(G, X):
    _, U, V, _, _, _ = _inputs(G, X)
    mass = U.sum(axis=0) * V.sum(axis=0)
    return mass, np.argsort(-mass, kind='stable')


def _cases():
    out = [(name, K, None) for name in ALL_MODELS for K in (1, 20, 50, 100)]
    out += [(name, K, None) for name in ('GaP', 'SparseGaP') for K in (129, 200)]
    out += [(name, K, DENSE_DENSITY) for name in ('GaP', 'SparseZIGaP') for K in (20, 100)]
    return [pytest.param(n, K, dd, id='%s-K%d-%s' % (n, K, 'hybrid' if dd else 'sliced')) for n, K, dd in out]


@pytest.mark.parametrize('name,K,dd', _cases())
def test_deviance_path_against_float64(name, K, dd):
    """Two sweeps from a seeded start; then order in {None, identity, a seeded permutation} x ks in {None, [K], [1], [3, 7, K]}
    against the restatement (one reference per order, at every k), and the entry at k = K against the full metrics of the
    same model within the sum of both bounds."""
    X = _counts(K)
    G = _model(name, X, K, dense_density=dd, seed=K)
    assert G._ws.Kp == KP[K]
    for _ in range(2):
        G.step()
    mass, by_mass = _mass_order(G, X)
    got_order = G.factor_order()
    assert got_order.dtype == np.int64 and sorted(got_order.tolist()) == list(range(K))
    # (the model's column sums are device sums: where two masses are closer than their rounding either order is right)
    assert np.all(np.diff(mass[got_order]) <= 1e-12 * mass.max())
    if np.all(np.abs(np.diff(mass[by_mass])) > 1e-12 * mass.max()):
        assert np.array_equal(got_order, by_mass)
    ed_full, rd_full = G.explained_deviance(), G.reconstruction_deviance()
    ks_list = [None, [K], [1]] + ([[3, 7, K]] if K > 7 else [])
    orders = [None, np.arange(K), np.random.default_rng(77 + K).permutation(K)]
    for order in orders:
        used = got_order if order is None else np.asarray(order)
        ref = _reference(G, X, used)
        for ks in ks_list:
            what = '%s K=%d %s order=%s ks=%s' % (name, K, 'hybrid' if dd else 'sliced',
                                                 'None' if order is None else ('identity' if order is orders[1] else 'random'), ks)
            got = G.deviance_path(order=order, ks=ks)
            want_k = np.arange(1, K + 1) if ks is None else np.asarray(ks)
            assert got['order'].dtype == np.int64 and np.array_equal(got['order'], used), what
            assert got['k'].dtype == np.int64 and np.array_equal(got['k'], want_k), what
            assert got['explained_deviance'].dtype == np.float64 and got['reconstruction_deviance'].dtype == np.float64
            r = dr.subset(ref, want_k)
            print(what, 'ed diff', dr.diff(got['explained_deviance'], r['ed']).max(), 'bound', r['tol']['ed'].min())
            dr.check(got, r, what=what)
            if want_k[-1] == K:
                last = dr.subset(ref, [K])
                for q, full, v in (('ed', ed_full, got['explained_deviance'][-1]), ('rd', rd_full, got['reconstruction_deviance'][-1])):
                    bound = last['tol'][q][0] + last['tol_full'][q][0]
                    if not np.isfinite(last[q][0]):
                        assert v == full == last[q][0], what
                        continue
                    assert abs(v - full) <= bound, '%s: %s at k = K %.17g, the full metric %.17g, bound %.3e' % (what, q, v, full, bound)


TINY_ROWS = (0, 7, 15, 240, 247, 255, 256 + 16 * 5 + 3, 768 + 7, 800, 804)    # row-in-slice 0 / 7 / 15, slices 0 / 15, last tile
UNDERFLOW_ROWS = (255, 804)                                                   # float32(U_hat) == 0 on these rows


@pytest.mark.parametrize('name,K,dd', [('GaP', 20, None), ('GaP', 20, DENSE_DENSITY), ('SparseZIGaP', 50, None),
                                       ('SparseGaP', 129, None)])
def test_deviance_path_float64_fallback(name, K, dd):
    """Cells scaled by 1e-13 (rates below 1e-10 at every prefix) and by 1e-38 more (float32(U_hat) == 0): the kernel takes their
    prefixes from the float64 factors, finding the cell from the slot position, and stays within the float64 bound -- the
    reference gives these entries ACC alone.  A wrong cell makes x log Lambda differ by orders of magnitude."""
    X = _counts(3)
    G = _model(name, X, K, dense_density=dd, seed=3)
    G.step()
    U = G.U_hat.copy()
    for i in TINY_ROWS:
        U[i] *= 1e-13
    for i in UNDERFLOW_ROWS:
        U[i] *= 1e-38
    assert not np.any(U[list(UNDERFLOW_ROWS)].astype(np.float32))
    assert all((X[i] != 0).any() for i in TINY_ROWS)
    G.load_state({'U_hat': U})
    order = G.factor_order()
    ref = _reference(G, X, order)
    got = G.deviance_path()
    assert np.isfinite(ref['ed'][-1]) and np.isfinite(got['explained_deviance'][-1])
    dr.check(got, ref, what='%s K=%d fallback' % (name, K))


@pytest.mark.parametrize('dd', [None, DENSE_DENSITY])
def test_deviance_path_masked_prefix_is_minus_infinity(dd):
    """SparseGaP, S_hat = 0 on the first two factors of the order for a gene that has counts (hybrid: one dense gene and one
    sliced gene): -inf at k = 1, 2 and only there, the literal float64 value."""
    X = _counts(4)
    K = 20
    G = _model('SparseGaP', X, K, dense_density=dd, seed=4)
    G.step()
    order = G.factor_order()
    genes = [20, 150] if dd else [150]
    if dd:
        pos = {int(j): p for p, j in enumerate(G.counts.col_perm.cpu().numpy())}
        assert pos[20] < G.counts.gd <= pos[150]
    p_s = G.p_s[:].copy()
    for j in genes:
        p_s[j, order[:2]] = 0.0
    G.load_state({'p_s': p_s})
    S = G.S_hat
    assert all(not S[j, order[:2]].any() and S[j, order[2:]].any() and (X[:, j] != 0).any() for j in genes)
    ref = _reference(G, X, order)
    assert np.all(ref['ed'][:2] == -np.inf) and np.all(np.isfinite(ref['ed'][2:]))
    got = G.deviance_path(order=order)
    assert np.all(got['explained_deviance'][:2] == -np.inf) and np.all(got['reconstruction_deviance'][:2] == np.inf)
    assert np.all(np.isfinite(got['explained_deviance'][2:])) and np.all(np.isfinite(got['reconstruction_deviance'][2:]))
    dr.check(got, ref, what='masked prefix')
    sub = G.deviance_path(order=order, ks=[2, 3, K])
    dr.check(sub, dr.subset(ref, [2, 3, K]), what='masked prefix, ks')


def test_deviance_path_argument_checks_and_state():
    """Bad `order` / `ks` raise ValueError before any launch; a call writes nothing of the model's state; two calls agree
    within the atomic-order bound."""
    from oriana_amd.models import base
    X = _counts(6)
    K = 20
    G = _model('SparseZIGaP', X, K, dense_density=DENSE_DENSITY, seed=6)
    for _ in range(2):
        G.step()
    launches = []
    real = base.call
    base.call = lambda name, *a: (launches.append(name), real(name, *a))[1]
    try:
        for kw in (dict(order=[0, 1]), dict(order=list(range(K - 1)) + [0]), dict(order=np.arange(K) + 1), dict(ks=[]),
                   dict(ks=[0, 3]), dict(ks=[3, 3]), dict(ks=[5, 2]), dict(ks=[K + 1]), dict(ks=[1.5]), dict(order='x')):
            with pytest.raises(ValueError):
                G.deviance_path(**kw)
        assert not launches, launches
        torch.cuda.synchronize()
        before = {k: np.asarray(v).tobytes() for k, v in G.state().items()}
        a = G.deviance_path()
        after = {k: np.asarray(v).tobytes() for k, v in G.state().items()}
        assert 'oriana_metric_nnz_prefix' in launches and 'oriana_dense_metric_prefix' in launches
        assert launches.count('oriana_dropout_metric') == K
    finally:
        base.call = real
    changed = [k for k in before if after[k] != before[k]]
    assert not changed, 'deviance_path() wrote %s' % changed
    b = G.deviance_path()
    ref = _reference(G, X, a['order'])
    assert np.array_equal(a['order'], b['order'])
    for q, name in (('ed', 'explained_deviance'), ('rd', 'reconstruction_deviance')):
        d = dr.diff(a[name], b[name])                   # (0 where both are the same infinity: masked prefixes)
        assert np.all(d <= 2 * ref['tol_acc'][q]), '%s: two calls %r apart, bound %r' % (name, d.max(), 2 * ref['tol_acc'][q].min())


def test_prefix_entries_return_codes():
    """Both C entries: ORIANA_EINVAL on null or inconsistent arguments before any launch, 0 for an empty problem, which leaves
    `out` alone; and one direct call against the reference's internal sums."""
    from oriana_amd import _lib
    from oriana_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    X = _counts(8)
    K = 20
    G = _model('GaP', X, K, dense_density=DENSE_DENSITY, seed=8)
    G.step()
    ct, ws, dev, st = G.counts, G._ws, G.device, stream_ptr()
    U, V = G._U_hat.contiguous(), G._V_hat.contiguous()
    FU, FV = ws.extra('MU', G.n), ws.extra('MV', G.m)
    _lib.call('oriana_factor_cast_f32', ptr(FU), ptr(U), None, ptr(ct.row_perm), G.n, K, st)
    _lib.call('oriana_factor_cast_f32', ptr(FV), ptr(V), None, ptr(ct.col_perm), G.m, K, st)
    fv = ptr(FV) + 4 * ct.gd * ws.Kp
    ends = torch.tensor([1, 5, K], dtype=torch.int32, device=dev)
    out = torch.zeros(3, 2, dtype=torch.float64, device=dev)
    cm, dn = ct.sparse_struct, ct.dense.c_struct
    EINVAL = -1
    f = lib.oriana_metric_nnz_prefix
    assert f(None, ptr(FU), fv, ptr(U), ptr(V), K, ptr(ends), 3, ptr(out), st) == EINVAL
    assert f(cm, None, fv, ptr(U), ptr(V), K, ptr(ends), 3, ptr(out), st) == EINVAL
    assert f(cm, ptr(FU), None, ptr(U), ptr(V), K, ptr(ends), 3, ptr(out), st) == EINVAL
    assert f(cm, ptr(FU), fv, None, ptr(V), K, ptr(ends), 3, ptr(out), st) == EINVAL
    assert f(cm, ptr(FU), fv, ptr(U), None, K, ptr(ends), 3, ptr(out), st) == EINVAL
    assert f(cm, ptr(FU), fv, ptr(U), ptr(V), K, None, 3, ptr(out), st) == EINVAL
    assert f(cm, ptr(FU), fv, ptr(U), ptr(V), K, ptr(ends), 3, None, st) == EINVAL
    assert f(cm, ptr(FU), fv, ptr(U), ptr(V), 0, ptr(ends), 3, ptr(out), st) == EINVAL
    assert f(cm, ptr(FU), fv, ptr(U), ptr(V), K, ptr(ends), -1, ptr(out), st) == EINVAL
    assert f(cm, ptr(FU), fv, ptr(U), ptr(V), K, ptr(ends), K + 1, ptr(out), st) == EINVAL
    assert f(cm, ptr(FU), fv, ptr(U), ptr(V), K, ptr(ends), 0, ptr(out), st) == 0          # no prefix: nothing to do
    g = lib.oriana_dense_metric_prefix
    rp, cp = ptr(ct.row_perm), ptr(ct.col_perm)
    assert g(None, ptr(U), ptr(V), rp, cp, K, ptr(ends), 3, ptr(out), st) == EINVAL
    assert g(dn, None, ptr(V), rp, cp, K, ptr(ends), 3, ptr(out), st) == EINVAL
    assert g(dn, ptr(U), None, rp, cp, K, ptr(ends), 3, ptr(out), st) == EINVAL
    assert g(dn, ptr(U), ptr(V), rp, cp, K, None, 3, ptr(out), st) == EINVAL
    assert g(dn, ptr(U), ptr(V), rp, cp, K, ptr(ends), 3, None, st) == EINVAL
    assert g(dn, ptr(U), ptr(V), rp, cp, 0, ptr(ends), 3, ptr(out), st) == EINVAL
    assert g(dn, ptr(U), ptr(V), rp, cp, 1025, ptr(ends), 3, ptr(out), st) == EINVAL
    assert g(dn, ptr(U), ptr(V), rp, cp, K, ptr(ends), K + 1, ptr(out), st) == EINVAL
    assert g(dn, ptr(U), ptr(V), rp, cp, K, ptr(ends), 0, ptr(out), st) == 0
    empty = _lib.OrianaDense(G.n, 0, (G.n + 255) // 256 * 8, None)                           # a layout without dense genes
    assert g(ctypes.byref(empty), ptr(U), ptr(V), rp, cp, K, ptr(ends), 3, ptr(out), st) == 0
    torch.cuda.synchronize()
    assert not out.any(), 'a refused or empty call wrote its output'
    # the two entries together: the internal sums of the reference at k = 1, 5, K
    assert f(cm, ptr(FU), fv, ptr(U), ptr(V), K, ptr(ends), 3, ptr(out), st) == 0
    assert g(dn, ptr(U), ptr(V), rp, cp, K, ptr(ends), 3, ptr(out), st) == 0
    got = out.cpu().numpy()
    ref = _reference(G, X, np.arange(K), ks=[1, 5, K])
    for q, col in (('lam', 0), ('xlog', 1)):
        d = np.abs(got[:, col] - ref[q])
        assert np.all(d <= ref['tol'][q]), '%s: diff %r bound %r' % (q, d, ref['tol'][q])


# ---- row sharding: a process group of one rank ------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, port, X, K, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ['ORIANA_FORCE_SHARDED'] = '1'            # (before construction: the collectives of a one-rank group are issued)
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        from oriana_amd import dist as odist, engine
        import oriana_amd.models as M
        dev = torch.device('cuda', 0)
        rng = np.random.default_rng(1000 + K)
        a1 = rng.gamma(1.0, 1.0, size=(X.shape[0], K)); b1 = rng.gamma(1.0, 1.0, size=(X.shape[1], K))
        counts = engine.CountTiles.from_dense(X, dev, reduce_fn=lambda t: odist.all_reduce_sum(t), n_total=X.shape[0])
        G = M.GaP(counts, k=K, init=(a1, b1), device=dev, process_group=dist.group.WORLD)
        assert G.sharded
        G.fit(2)
        order = G.factor_order()
        p = G.deviance_path(ks=[1, 3, 7, K])
        st = G.state()
        np.savez(out, order=order, ed=p['explained_deviance'], rd=p['reconstruction_deviance'], path_order=p['order'],
                 **{'st_' + k: v for k, v in st.items()})
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    # (as tests/test_sharded_gpu.py: leave without the static destructors of the interpreter / c10d)
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(0)


def test_deviance_path_one_rank_process_group(tmp_path):
    """Under a one-rank process group with ORIANA_FORCE_SHARDED=1 (a fresh child process) the packed per-prefix sums go through
    the all-reduce: the same order and, on the same state loaded into a single-process model, the same values within the
    float64 accumulation bound."""
    K = 20
    X = _counts(9)
    out = str(tmp_path / 'path_sharded.npz')
    mp.spawn(_worker, args=(_free_port(), X, K, out), nprocs=1, join=True)
    got = np.load(out)
    G = _model('GaP', X, K, seed=9)
    G.load_state({k[3:]: got[k] for k in got.files if k.startswith('st_')})
    assert np.array_equal(G.factor_order(), got['order']) and np.array_equal(got['path_order'], got['order'])
    one = G.deviance_path(ks=[1, 3, 7, K])
    ref = _reference(G, X, got['order'], ks=[1, 3, 7, K])
    for q, name in (('ed', 'explained_deviance'), ('rd', 'reconstruction_deviance')):
        d = dr.diff(one[name], got[q])
        assert np.all(d <= 2 * ref['tol_acc'][q]), '%s: sharded and single-process %r apart, bound %r' % (name, d, 2 * ref['tol_acc'][q])
    dr.check(dict(explained_deviance=got['ed'], reconstruction_deviance=got['rd']), ref, what='one-rank group')
