# -*- coding: utf-8 -*-
"""GaP.elbo() and fit(tol=) on the GPU against the float64 reference of tests/elbo_reference.py.

Shapes follow tests/test_metrics_gpu.py (the smallest that cross a partial last row tile and two column tiles); the bounds
are those of elbo_reference.elbo_bounds, derived from the arithmetic: g = (K + 3) 2^-24 on the float32 den of the row pass,
1e-12 relative to the sum of |piece| for everything that is summed in float64.
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import elbo_reference as er

pytestmark = pytest.mark.gpu

N_ROWS = 3 * 256 + 37            # a partial last row tile
M_COLS = 301                     # two column tiles, the last one partial
DENSE_DENSITY = 0.5
KS = (1, 20, 64, 100, 129)       # one per Kp family: 16, 20, 64, 100, 160
HYBRID_KS = (1, 20, 64, 100)     # the K the dense-block kernels are compiled for (engine.dense_supported)


def _counts(seed, n=N_ROWS, m=M_COLS):
    """As tests/test_metrics_gpu.py: 70 genes dense enough for the hybrid block, the rest at 15 %; an all-zero gene (5), an
    all-zero cell (11), a gene expressed in every cell but that one (250)."""
    rng = np.random.default_rng(seed)
    dens = np.full(m, 0.15)
    dens[:70] = 0.8
    X = ((rng.poisson(rng.gamma(0.6, 4.0, size=(n, m))) + 1) * (rng.random((n, m)) < dens)).astype(np.float64)
    X[:, 250] = rng.poisson(6.0, size=n) + 1
    X[:, 5] = 0
    X[11, :] = 0
    return X


def _model(X, K, dense_density=None, seed=0, name='GaP', **kw):
    import oriana_amd.models as M
    rng = np.random.default_rng(1000 + seed)
    n, m = X.shape
    a1 = rng.gamma(1.0, 1.0, size=(n, K))
    b1 = rng.gamma(1.0, 1.0, size=(m, K))
    return getattr(M, name)(X, k=K, init=(a1, b1), dense_density=dense_density, **kw)


def _small(seed=0, n=293, m=131, K=7):
    """The case of the float64 CPU experiment: 30 % non-zeros, Gamma(1) shapes."""
    rng = np.random.default_rng(seed)
    X = ((rng.poisson(3.0, size=(n, m)) + 1) * (rng.random((n, m)) < 0.3)).astype(np.float64)
    a1 = rng.gamma(1.0, 1.0, size=(n, K))
    b1 = rng.gamma(1.0, 1.0, size=(m, K))
    return X, a1, b1, K


def _small_model(name='GaP'):
    import oriana_amd.models as M
    X, a1, b1, K = _small()
    return getattr(M, name)(X, k=K, init=(a1, b1)), X


def _check(G, X, what):
    """elbo() and each of its partial sums against the reference on the model's own state, each within its own bound."""
    ref = er.elbo_terms(X, G.state())
    tol = er.elbo_bounds(ref, G.k)
    got = dict(zip(er.TERMS, G._elbo_terms().cpu().numpy().tolist()))
    got['elbo'] = G.elbo()
    for k in er.TERMS + ('elbo',):
        d = abs(got[k] - ref[k])
        print('%s %s: HIP %.17g ref %.17g diff %.3e bound %.3e' % (what, k, got[k], ref[k], d, tol[k]))
    for k in er.TERMS + ('elbo',):
        d = abs(got[k] - ref[k])
        assert np.isfinite(got[k]) and d <= tol[k], '%s %s: HIP %.17g ref %.17g diff %.3e > bound %.3e' % (
            what, k, got[k], ref[k], d, tol[k])
    return got, ref, tol


# ---- 1. the value against float64 ---------------------------------------------------------------------------------------------

def _cases():
    return [pytest.param(K, dd, id='K%d-%s' % (K, 'hybrid' if dd else 'sliced'))
            for K in KS for dd in ([None, DENSE_DENSITY] if K in HYBRID_KS else [None])]


@pytest.mark.parametrize('K,dd', _cases())
def test_elbo_against_float64(K, dd):
    from oriana_amd import engine
    assert engine.dense_supported(K) == (K in HYBRID_KS), 'the hybrid cases of this matrix are out of date'
    X = _counts(K)
    G = _model(X, K, dense_density=dd, seed=K)
    assert (G.counts.gd >= 32 and G.counts.dense is not None) if dd else G.counts.gd == 0
    for _ in range(2):
        G.step()
    _check(G, X, 'K=%d %s' % (K, 'hybrid' if dd else 'sliced'))


TINY_SOME = (0, 7, 255, 256 + 16 * 5 + 3, 800)       # a1 = 1e-15 in two of the factors
TINY_ALL = 804                                       # ... in every factor (last row tile)


@pytest.mark.parametrize('dd', [None, DENSE_DENSITY], ids=['sliced', 'hybrid'])
def test_elbo_fallback_entries(dd):
    """Cells whose shapes sit at the clamp: E[log U] ~ -1e15 there.  The cell with every factor at the clamp cannot take the
    shifted form (NaN sentinel in s): its entries are a float64 log-sum-exp inside the kernel and the value stays finite."""
    K = 20
    X = _counts(3)
    G = _model(X, K, dense_density=dd, seed=3)
    G.step()
    a1 = G.a1[:].copy()
    for i in TINY_SOME:
        a1[i, [2, 11]] = 1e-15
    a1[TINY_ALL, :] = 1e-15
    assert all((X[i] != 0).any() for i in TINY_SOME + (TINY_ALL,))
    G.load_state({'a1': a1})
    G.update_expectations()
    assert G.log_U_hat[TINY_ALL].max() < -1e14
    got, ref, _ = _check(G, X, 'fallback %s' % ('hybrid' if dd else 'sliced'))
    assert np.isfinite(got['elbo']) and np.isfinite(ref['elbo'])
    assert torch.isnan(G._ws.s_rs).any(), 'the row pass left no NaN sentinel: the fall-back was not exercised'


# ---- 2. monotone --------------------------------------------------------------------------------------------------------------

def test_elbo_is_monotone_over_30_sweeps():
    """Every increment of elbo() is at least -(the evaluation bounds of its two values); the float64 restatement's smallest
    increment at this case was ~1.6e-3 sum(x), three orders above the bound's ~6e-7 sum(x)."""
    G, X = _small_model()
    vals, bounds = [], []
    for _ in range(31):
        vals.append(G.elbo())
        bounds.append(er.elbo_bounds(er.elbo_terms(X, G.state()), G.k)['elbo'])
        G.step()
    inc = np.diff(vals)
    slack = np.array(bounds[1:]) + np.array(bounds[:-1])
    print('increments / sum(x): min %.3e max %.3e; bound / sum(x) %.3e' % (inc.min() / X.sum(), inc.max() / X.sum(),
                                                                        max(bounds) / X.sum()))
    bad = np.nonzero(inc < -slack)[0]
    assert bad.size == 0, 'elbo() decreased at sweeps %r: %r (allowed %r)' % (bad.tolist(), inc[bad], -slack[bad])
    assert vals[-1] > vals[0]


# ---- 3. the call leaves the sweep alone ---------------------------------------------------------------------------------------
# The property tests/test_metrics_gpu.py holds for the metrics (test_metrics_do_not_disturb_the_sweep), for elbo():
#   (a) bit for bit: everything the model and its workspace hold -- the FU prepared for the next sweep, fu_pending, the
#       statistics of the preparation included -- is unchanged by the call; what it may overwrite is scratch that every sweep
#       rewrites before reading it (the row pass's R, s_cs, s_rs and flags) and the call's own (`_elbo_mu`, ws.extra).  This is
#       the deterministic statement of "the next sweep is bit-identical": it gets bit-identical inputs.
#   (b) twins: a run with elbo() between the sweeps against one without.  Two runs of the SAME sweeps are not bit-identical on
#       this code base (the Gamma updates' float64 column sums and the column pass's float32 per-gene sums are atomics across
#       work-groups -- measured at this shape: two elbo-free models already differ in alpha2 / beta2 after the constructor and
#       in every parameter after three sweeps), so twins are held to the atomic-order bound of test_metrics_gpu._twin_bound,
#       against which a clobbered workspace is off by orders of magnitude.

ELBO_SCRATCH = ('ws.R', 'ws.s_cs', 'ws.s_rs', 'ws.tile_flag', '_elbo_mu')


def _held_tensors(G):
    """Host copies of every tensor the model and its workspace hold (lazy parameters only when materialised; the lazy
    U_hat buffer as it is, stale or not: elbo() must not resolve it)."""
    from oriana_amd.parameters import Parameter
    out = {}
    for owner, prefix in ((G, ''), (G._ws, 'ws.')):
        for k, v in vars(owner).items():
            if isinstance(v, Parameter) and getattr(v, 'materialised', True):
                v = v.tensor
            if isinstance(v, torch.Tensor) and prefix + k not in ELBO_SCRATCH:
                out[prefix + k] = v.detach().cpu().numpy().tobytes()
    return out


def _elbo_leaves_state_alone(G):
    ws = G._ws
    before, flags = _held_tensors(G), (ws.fu_pending, ws.fu_source, ws.FU.data_ptr(), G._u_stale, G._v_sums_in_acc)
    G.elbo()
    after = _held_tensors(G)
    assert (ws.fu_pending, ws.fu_source, ws.FU.data_ptr(), G._u_stale, G._v_sums_in_acc) == flags
    changed = [k for k in before if after.get(k) != before[k]]
    assert not changed and before.keys() <= after.keys(), 'elbo() wrote %s' % changed


def _twin_bound(n, sweeps):
    """err_colrel between two runs of the same sweeps that differ only in the order in which float atomics combine partial
    sums (tests/test_metrics_gpu.py): a float32 sum of p non-negative partials moves by at most (p - 1) 2^-24 relative when
    reordered, p <= ceil(n / 32) (the finest cell tiling, 32-cell dense tiles); each further sweep may double what it receives."""
    return 2.0 ** sweeps * ((n + 31) // 32) * 2.0 ** -24


def _three_sweeps(K, dd, with_elbo, graph):
    X = _counts(K + 1)
    G = _model(X, K, dense_density=dd, seed=K + 1)
    if graph:
        G.capture_graph()
    if with_elbo:
        G.elbo()                                        # (the call's own scratch exists from here on)
    for _ in range(3):
        if with_elbo:
            _elbo_leaves_state_alone(G)
        G.step()
    if with_elbo:
        _elbo_leaves_state_alone(G)
    torch.cuda.synchronize()
    return G.state(), G.n


@pytest.mark.parametrize('K,dd,graph', [(20, None, False), (20, DENSE_DENSITY, False), (64, None, False), (100, None, False),
                                        (100, DENSE_DENSITY, False), (20, None, True), (64, None, True)],
                         ids=['K20-sliced', 'K20-hybrid', 'K64-sliced', 'K100-sliced', 'K100-hybrid', 'K20-graph', 'K64-graph'])
def test_elbo_does_not_disturb_the_sweep(K, dd, graph):
    """elbo; step; elbo; step; elbo; step; elbo against step; step; step, eager and with capture_graph() on both."""
    from helpers import err_colrel
    (b1, n), (b2, _) = _three_sweeps(K, dd, False, graph), _three_sweeps(K, dd, False, graph)
    a, _ = _three_sweeps(K, dd, True, graph)
    tol = _twin_bound(n, 3)
    for k in b1:
        e0 = err_colrel(b2[k], b1[k]) if b1[k].size else 0.0
        assert e0 <= tol, '%s: two elbo-free runs are %.3e apart, beyond the atomic-order bound %.3e' % (k, e0, tol)
        e = err_colrel(a[k], b1[k]) if b1[k].size else 0.0
        print('%s: elbo-free twins %.3e apart, the run with elbo() %.3e from the first (bound %.3e)' % (k, e0, e, tol))
        assert e <= tol, '%s: the run with elbo() calls is %.3e from the one without (bound %.3e)' % (k, e, tol)


def test_elbo_keeps_the_prepared_factor():
    """The cell-side update of a long matrix prepares the next sweep's FU (fu_pending) and leaves a2 / U_hat deferred: the
    call between two sweeps changes none of it."""
    n, m, K = 8200, 200, 128                           # n K >= 2^20: the fused preparation and the lazy form engage
    rng = np.random.default_rng(12)
    X = (rng.poisson(3.0, size=(n, m)) * (rng.random((n, m)) < 0.1)).astype(np.float64)
    G = _model(X, K, seed=12)
    G.step()
    G.elbo()
    G.step()
    assert G._ws.fu_pending and G._u_stale, 'the case covers neither the fused preparation nor the lazy cell side'
    _elbo_leaves_state_alone(G)
    G.step()
    _elbo_leaves_state_alone(G)


# ---- 4. the lazy cell side ----------------------------------------------------------------------------------------------------

def test_elbo_leaves_a2_deferred(monkeypatch):
    import oriana_amd.models as M
    from oriana_amd.parameters import LazyParameter
    rng = np.random.default_rng(11)
    n, m, K = 8200, 200, 128                           # n K >= 2^20: the lazy form engages
    X = (rng.poisson(3.0, size=(n, m)) * (rng.random((n, m)) < 0.1)).astype(np.float64)
    a1 = rng.gamma(1.0, size=(n, K)); b1 = rng.gamma(1.0, size=(m, K))
    monkeypatch.setenv('ORIANA_LAZY_U', '1')
    A = M.GaP(X, k=K, init=(a1, b1))
    A.step(); A.step()
    assert isinstance(A.a2, LazyParameter) and not A.a2.materialised and A._u_stale, 'the lazy form did not engage'
    e_lazy = A.elbo()
    assert not A.a2.materialised and A._u_stale, 'elbo() materialised the deferred cell side'
    st = A.state()
    ref = er.elbo_terms(X, st)
    tol = er.elbo_bounds(ref, K)['elbo']
    print('lazy %.17g ref %.17g bound %.3e' % (e_lazy, ref['elbo'], tol))
    assert abs(e_lazy - ref['elbo']) <= tol
    # the same state in a model that stores a2 and U_hat
    monkeypatch.setenv('ORIANA_LAZY_U', '0')
    B = M.GaP(X, k=K, init=(a1, b1))
    assert not isinstance(B.a2, LazyParameter)
    B.load_state(st)
    e_stored = B.elbo()
    print('stored %.17g' % e_stored)
    assert abs(e_stored - e_lazy) <= tol


# ---- 5. fit(tol=) -------------------------------------------------------------------------------------------------------------

def _planted(seed=5, n=293, m=131, K=3):
    """Counts drawn from the model itself (Gamma(1) factors of rank K, Poisson counts) and a Gamma(1) start: a well-specified
    fit with few factors, whose bound flattens within a few dozen sweeps (unstructured counts leave K near-flat directions and
    the relative change of the bound per five sweeps stays above 1e-4 for more than 200 sweeps)."""
    rng = np.random.default_rng(seed)
    X = rng.poisson(rng.gamma(1.0, 1.0, size=(n, K)) @ rng.gamma(1.0, 1.0, size=(m, K)).T).astype(np.float64)
    return X, rng.gamma(1.0, 1.0, size=(n, K)), rng.gamma(1.0, 1.0, size=(m, K)), K


def test_fit_with_tol_stops_early():
    import oriana_amd.models as M
    X, a1, b1, K = _planted()
    G = M.GaP(X, k=K, init=(a1, b1))
    assert G.fit(200, tol=1e-4, check_every=5) is G
    print('stopped after %d sweeps; trace %r' % (G.n_sweeps, G.elbo_trace_))
    assert 0 < G.n_sweeps < 200 and G.n_sweeps % 5 == 0
    sweeps = [s for s, _ in G.elbo_trace_]
    vals = np.array([v for _, v in G.elbo_trace_])
    assert sweeps == list(range(5, G.n_sweeps + 1, 5))
    assert abs(vals[-1] - vals[-2]) <= 1e-4 * abs(vals[-1])
    assert all(abs(b - a) > 1e-4 * abs(b) for a, b in zip(vals[:-2], vals[1:-1])), 'fit went on after the criterion was met'
    # non-decreasing within the evaluation bound (taken on a twin run's states at the same sweeps)
    T = M.GaP(X, k=K, init=(a1, b1))
    bounds = []
    for s in sweeps:
        while T.n_sweeps < s:
            T.step()
        bounds.append(er.elbo_bounds(er.elbo_terms(X, T.state()), T.k)['elbo'])
    slack = np.array(bounds[1:]) + np.array(bounds[:-1])
    assert np.all(np.diff(vals) >= -slack), (np.diff(vals), slack)
    # a second call goes on from where the first stopped and appends to the trace
    G.fit(5, tol=1e-4, check_every=5)
    assert G.elbo_trace_[-1][0] == G.n_sweeps == sweeps[-1] + 5 and len(G.elbo_trace_) == len(sweeps) + 1


def _record_launches(monkeypatch):
    """Every C-ABI call of the model layer by name, in order."""
    import oriana_amd.models.base as mb
    import oriana_amd.models.gap as mg
    from oriana_amd import _lib, engine
    log = []

    def call(name, *args):
        log.append(name)
        return _lib.call(name, *args)
    for mod in (mb, mg, engine):
        monkeypatch.setattr(mod, 'call', call)
    return log


def test_fit_without_tol_is_the_plain_loop(monkeypatch):
    """fit(7) launches exactly what seven step() calls launch (the same C-ABI calls in the same order, none of elbo()'s) and
    gives their states (twins: within the atomic-order bound, see section 3)."""
    from helpers import err_colrel
    A, _ = _small_model()
    B, _ = _small_model()
    log = _record_launches(monkeypatch)
    assert A.fit(7) is A
    fit_calls = list(log)
    del log[:]
    for _ in range(7):
        B.step()
    torch.cuda.synchronize()
    assert fit_calls == log and len(log) > 0
    assert not any('elbo' in c or c == 'oriana_gamma_kl' for c in fit_calls)
    assert A.n_sweeps == B.n_sweeps == 7 and not hasattr(A, 'elbo_trace_')
    sa, sb = A.state(), B.state()
    for k in sa:
        assert err_colrel(sa[k], sb[k]) <= _twin_bound(A.n, 7), k


@pytest.mark.parametrize('name', ['ZIGaP', 'SparseGaP', 'SparseZIGaP'])
def test_models_without_a_bound_say_so(name):
    G, _ = _small_model(name)
    with pytest.raises(NotImplementedError, match='coordinate ascent'):
        G.elbo()
    with pytest.raises(NotImplementedError, match='coordinate ascent'):
        G.fit(5, tol=1e-3)
    assert G.n_sweeps == 0
    G.fit(1)
    assert G.n_sweeps == 1


# ---- 6. row sharding ----------------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, X, a1, b1, K, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import oriana_amd.models as M
        from oriana_amd import dist as odist, engine
        r0, r1 = odist.shard_rows(X.shape[0], rank, world)
        dev = torch.device('cuda', 0)
        counts = engine.CountTiles.from_dense(X[r0:r1], dev, reduce_fn=lambda t: odist.all_reduce_sum(t), n_total=X.shape[0])
        model = M.GaP(counts, k=K, init=(a1[r0:r1], b1), device=dev, process_group=dist.group.WORLD)
        model.fit(2)
        value = model.elbo()
        st = model.state()
        gathered = [None] * world
        dist.all_gather_object(gathered, (value, {k: st[k] for k in ('a1', 'a2', 'U_hat', 'log_U_hat')}))
        if rank == 0:
            full = {k: np.concatenate([g[1][k] for g in gathered]) for k in gathered[0][1]}
            for k in ('b1', 'b2', 'V_hat', 'log_V_hat', 'alpha1', 'alpha2', 'beta1', 'beta2'):
                full[k] = st[k]
            full['values'] = np.array([g[0] for g in gathered])
            np.savez(out, **full)
        dist.barrier()
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    # (as tests/test_sharded_gpu.py: leave without the static destructors of the interpreter / c10d)
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(0)


def test_elbo_two_ranks_match_one(tmp_path):
    """Two ranks on one GPU (fresh child processes, gloo): the same value on both ranks, and the single-process value on the
    concatenated rows -- the same state, loaded -- within the evaluation bound."""
    import oriana_amd.models as M
    n, m, K = 2 * 256 + 91, 301, 20                    # the second shard starts inside a row tile of the whole matrix
    X = _counts(21, n=n, m=m)
    rng = np.random.default_rng(22)
    a1 = rng.gamma(1.0, 1.0, size=(n, K)); b1 = rng.gamma(1.0, 1.0, size=(m, K))
    out = str(tmp_path / 'elbo_sharded.npz')
    mp.spawn(_worker, args=(2, _free_port(), X, a1, b1, K, out), nprocs=2, join=True)
    got = np.load(out)
    values = got['values']
    assert values[0] == values[1], values
    st = {k: got[k] for k in got.files if k != 'values'}
    ref = er.elbo_terms(X, st)
    tol = er.elbo_bounds(ref, K)['elbo']
    single = M.GaP(X, k=K, init=(a1, b1))
    single.load_state(st)
    one = single.elbo()
    print('sharded %.17g single %.17g ref %.17g bound %.3e' % (values[0], one, ref['elbo'], tol))
    assert abs(values[0] - ref['elbo']) <= tol
    assert abs(values[0] - one) <= tol + er.ACC * sum(ref['abs'].values())
