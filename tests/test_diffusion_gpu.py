# -*- coding: utf-8 -*-
"""cluster.diffusion_graph / csr_spmv / basis_* / diffusion_map / diffusion_pseudotime and model.cell_diffusion / cell_pseudotime
on the GPU against the NumPy float64 restatement of tests/diffusion_reference.py.  Every bound is derived: the order-dependent
sums by their length times 2^-52, the eigenpairs by their own true residuals (recomputed in NumPy against the reference matrix),
Weyl for the values and Davis-Kahan for the vectors with the gaps of the reference spectrum.  Wherever the kernels promise fixed
bits (`blocks`, the scratch's contents, repetition) the comparison is array_equal."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import diffusion_cases as dc
import diffusion_reference as dr
import helpers
from test_markers_gpu import _G, _X, CASES, CASE_IDS, K
from test_deviance_path_gpu import _free_port

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = 2.0 ** -52
TOL = 1e-10


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _graph_of(name):
    c = dc.case(name)
    from oriana_amd import cluster
    return cluster.diffusion_graph(_dev(c['indices']), _dev(c['sq_distances']))


def _ref_graph(name):
    crow, col, val = dc.reference(name)['csr']
    return {'crow': _dev(crow), 'col': _dev(col), 'weight': _dev(val), 'n': crow.size - 1}


# ---- (a) the affinity graph --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', dc.CONNECTED + ('tiny', 'two_islands'))
def test_diffusion_graph_against_the_reference(name):
    from oriana_amd import cluster
    r = dc.reference(name)
    crow, col, val = r['csr']
    got = _graph_of(name)
    assert got['crow'].dtype == torch.int64 and got['col'].dtype == torch.int32 and got['weight'].dtype == torch.float64 and got['n'] == crow.size - 1
    assert np.array_equal(got['crow'].cpu().numpy(), crow) and np.array_equal(got['col'].cpu().numpy(), col)
    bound = (int(np.diff(crow).max()) + 16) * U                    # (the row sums are the only order-dependent step)
    w = got['weight'].cpu().numpy()
    err = np.abs(w - val) / val
    print('%s: weights rel err %.3e, bound %.3e' % (name, err.max(), bound))
    assert err.max() <= bound
    assert (np.abs(got['z'].cpu().numpy() - r['z']) <= bound * r['z']).all()
    n = crow.size - 1
    D = np.zeros((n, n))
    D[np.repeat(np.arange(n), np.diff(crow)), col] = w
    assert np.array_equal(D, D.T)                                  # bit-symmetric
    for blocks in (1, 3):
        c = dc.case(name)
        again = cluster.diffusion_graph(_dev(c['indices']), _dev(c['sq_distances']), blocks=blocks)
        assert np.array_equal(again['weight'].cpu().numpy(), w) and np.array_equal(again['z'].cpu().numpy(), got['z'].cpu().numpy())
    assert cluster.graph_components(got)['n_components'] == r['labels'].max() + 1
    assert np.array_equal(cluster.graph_components(got)['labels'].cpu().numpy(), r['labels'])


def test_diffusion_graph_takes_the_lower_rows_distance():
    """Lists whose two directions disagree: the value of row min(i, j) wins where that row lists the other node."""
    from oriana_amd import cluster
    c = dc.case('path600')
    d2 = c['sq_distances'].copy()
    d2[::2] *= np.float32(1.25)                                    # even rows state other distances than odd rows
    got = cluster.diffusion_graph(_dev(c['indices']), _dev(d2))
    T, z, P = dr.dense_transition(c['indices'], d2)
    crow, col, val = dr.csr_of(T, P)
    assert np.array_equal(T, T.T) and np.array_equal(got['col'].cpu().numpy(), col)
    assert (np.abs(got['weight'].cpu().numpy() - val) <= (int(np.diff(crow).max()) + 16) * U * val).all()


def test_diffusion_graph_refusals():
    from oriana_amd import cluster
    c = dc.case('path600')
    idx, d2 = c['indices'].copy(), c['sq_distances'].copy()
    idx[7, 3] = idx[7, 0]
    with pytest.raises(ValueError, match='twice'):
        cluster.diffusion_graph(_dev(idx), _dev(d2))
    idx = c['indices']
    d2[5] = 0
    d2[9] = 0
    with pytest.raises(ValueError, match='^2 rows'):
        cluster.diffusion_graph(_dev(idx), _dev(d2))
    d2[5, 3], d2[9, 0] = 0.25, 0.5                                 # a zero median: the smallest positive value stands in
    got = cluster.diffusion_graph(_dev(idx), _dev(d2))
    T, z, P = dr.dense_transition(idx, d2)
    crow, col, val = dr.csr_of(T, P)
    assert (np.abs(got['weight'].cpu().numpy() - val) <= (int(np.diff(crow).max()) + 16) * U * val).all()
    d2[3, 1] = -1.0
    with pytest.raises(ValueError, match='negative or not finite'):
        cluster.diffusion_graph(_dev(idx), _dev(d2))


# ---- (b) SpMV ----------------------------------------------------------------------------------------------------------------------
def _spmv_check(crow, col, val, x, what):
    from oriana_amd import cluster
    n = crow.size - 1
    rows = np.repeat(np.arange(n), np.diff(crow))
    prod = val.astype(np.longdouble) * x[col].astype(np.longdouble)
    ref, mass = np.zeros(n, dtype=np.longdouble), np.zeros(n, dtype=np.longdouble)
    np.add.at(ref, rows, prod)
    np.add.at(mass, rows, np.abs(prod))
    d = [_dev(a) for a in (crow, col, val, x)]
    first = None
    for blocks in (0, 1, 3):
        for again in range(2):
            y, check = helpers.guarded_out((n,), torch.float64, 'nan', DEV)
            assert cluster.csr_spmv(d[0], d[1], d[2], d[3], out=y, blocks=blocks) is y
            got = y.cpu().numpy()
            check(str((what, blocks, again)))
            first = got if first is None else first
            assert np.array_equal(got, first), (what, blocks, again)
    assert (np.abs(first - ref) <= np.diff(crow) * U * mass).all(), what
    assert (first[np.diff(crow) == 0] == 0).all()


def test_spmv_row_lengths_and_the_hub():
    rng = np.random.default_rng(21)
    n = 5001
    lens = np.concatenate([[0, 1, 15, 16, 17, 64, 65, 5000, 0, 33], rng.integers(0, 4, size=n - 10)])
    crow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(n, size=l, replace=False)) for l in lens]).astype(np.int32)
    _spmv_check(crow, col, rng.normal(size=col.size), rng.normal(size=n), 'lengths')
    _spmv_check(*dc.star(), 'star')
    _spmv_check(np.array([0, 1], dtype=np.int64), np.zeros(1, dtype=np.int32), np.array([1.5]), np.array([-2.0]), 'n = 1')
    _spmv_check(np.array([0, 0], dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), np.array([3.0]), 'n = 1, empty')


# ---- (c) the basis kernels ---------------------------------------------------------------------------------------------------------
def _tile():
    from oriana_amd import cluster
    return cluster.basis_tile_rows()


def _basis(rng, n, j, ld):
    """j orthonormal columns (QR of a seeded matrix) as a (j, ld) device basis whose padding is NaN."""
    Qn = np.linalg.qr(rng.normal(size=(n, j)))[0]
    Q = torch.full((j + 1, ld), float('nan'), dtype=torch.float64, device=DEV)
    Q[:j, :n] = _dev(Qn.T)
    return Qn, Q


N_NAMES = ('1', '63', '64', '65', 't-1', 't', 't+1', '3t+5')
JS = (1, 2, 5, 64, 65, 130)


def _n_of(name):
    t = _tile()
    return {'t-1': t - 1, 't': t, 't+1': t + 1, '3t+5': 3 * t + 5}.get(name) or int(name)


@pytest.mark.parametrize('nname', N_NAMES)
def test_orthogonalize(nname):
    from oriana_amd import cluster, _lib
    lib = _lib.load()
    n = _n_of(nname)
    rng = np.random.default_rng(100 + n)
    for j in (j for j in JS if j <= n):
        for ld in (n + (n & 1), n + 6 + (n & 1)):
            Qn, Q = _basis(rng, n, j, ld)
            w0 = rng.normal(size=n)
            w_ref, h_ref, b_ref = dr.cgs2(Qn, w0)
            need = int(lib.oriana_basis_orthogonalize_scratch_bytes_for(n, j))
            first = None
            for variant, blocks in (('zero', 0), ('nan', 0), ('stale', 0), ('zero', 1), ('zero', 3), ('nan', 3), ('zero', 0)):
                what = (n, j, ld, variant, blocks)
                scratch, chk_s = helpers.guarded_variant(need, variant, device=DEV)
                if variant == 'stale':                             # a valid call of the same sizes on other inputs left it like this
                    cluster.basis_orthogonalize(Q, n, j, _dev(rng.normal(size=n)), torch.zeros(j, dtype=torch.float64, device=DEV),
                                                torch.zeros(1, dtype=torch.float64, device=DEV), scratch=scratch)
                w, chk_w = helpers.guarded_out((n,), torch.float64, 'zero', DEV)
                h, chk_h = helpers.guarded_out((j,), torch.float64, 'zero', DEV)
                b2, chk_b = helpers.guarded_out((1,), torch.float64, 'nan', DEV)
                w.copy_(_dev(w0))
                cluster.basis_orthogonalize(Q, n, j, w, h, b2, passes=2, blocks=blocks, scratch=scratch)
                got = (w.cpu().numpy(), h.cpu().numpy(), b2.cpu().numpy())
                for c in (chk_s, chk_w, chk_h, chk_b):
                    c(str(what))
                if first is None:
                    first = got
                    norm = np.linalg.norm(w0)
                    assert np.abs(got[1] - h_ref).max() <= n * U * norm, what
                    assert np.abs(Qn.T @ got[0]).max() <= 8 * (n + j) * 2.0 ** -53 * norm, what
                    assert np.abs(got[0] - w_ref).max() <= 8 * (n + j) * 2.0 ** -53 * norm, what
                    assert abs(got[2][0] - got[0] @ got[0]) <= (n + 2) * U * (got[0] @ got[0]), what
                for a, b in zip(got, first):
                    assert np.array_equal(a, b), what
            # one pass is the first half of two
            w1, h1, b1 = _dev(w0), torch.zeros(j, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV)
            cluster.basis_orthogonalize(Q, n, j, w1, h1, b1, passes=1)
            r1 = dr.cgs2(Qn, w0, passes=1)
            assert np.abs(h1.cpu().numpy() - r1[1]).max() <= n * U * norm and np.abs(w1.cpu().numpy() - r1[0]).max() <= 8 * (n + j) * 2.0 ** -53 * norm
            assert torch.isnan(Q[:j, n:]).all() and torch.isnan(Q[j]).all()      # the basis itself is only read


def test_orthogonalize_refuses_a_short_scratch_and_writes_nothing():
    from oriana_amd import cluster, _lib
    lib = _lib.load()
    n, j = _tile() + 1, 5
    rng = np.random.default_rng(7)
    Qn, Q = _basis(rng, n, j, n + 1)
    need = int(lib.oriana_basis_orthogonalize_scratch_bytes_for(n, j))
    scratch, chk_s = helpers.guarded_variant(need, 'nan', device=DEV)
    w, chk_w = helpers.guarded_out((n,), torch.float64, 'nan', DEV)
    h, chk_h = helpers.guarded_out((j,), torch.float64, 'nan', DEV)
    b2, chk_b = helpers.guarded_out((1,), torch.float64, 'nan', DEV)
    rc = lib.oriana_basis_orthogonalize_f64(n, _lib.ptr(Q), n + 1, j, _lib.ptr(w), _lib.ptr(h), _lib.ptr(b2), 2, _lib.ptr(scratch), need - 1, 0,
                                            _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1
    for t in (w, h, b2, scratch.view(torch.float64)):
        assert torch.isnan(t).all()                                # (every byte still 0xFF)
    for c in (chk_s, chk_w, chk_h, chk_b):
        c('short scratch')
    with pytest.raises(ValueError, match='scratch'):
        cluster.basis_orthogonalize(Q, n, j, w, h, b2, scratch=torch.empty(need - 1, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize('nname', N_NAMES)
def test_append_and_combine(nname):
    from oriana_amd import cluster
    n = _n_of(nname)
    rng = np.random.default_rng(200 + n)
    for j in (j for j in JS if j <= n):
        ld = n + 6 + (n & 1) if j % 2 else n + (n & 1)
        Qn, Q = _basis(rng, n, j, ld)
        w0, b = rng.normal(size=n), np.array([rng.random() + 0.5])
        for again in range(2):
            Q[j] = float('nan')
            cluster.basis_append(Q, n, j, _dev(w0), _dev(b))
            col = Q[j].cpu().numpy()
            want = w0 / np.sqrt(b[0])
            assert (np.abs(col[:n] - want) <= U * np.abs(want)).all() and np.isnan(col[n:]).all(), (n, j)      # (both correctly rounded)
            if again:
                assert np.array_equal(col[:n], kept)
            kept = col[:n]
        for m in (1, 8, 15):
            S = rng.normal(size=(j, m))
            ref = Qn @ S
            mass = np.abs(Qn) @ np.abs(S)
            first = None
            for blocks in (0, 1, 3):
                for again in range(2):
                    out, chk = helpers.guarded_out((m, ld), torch.float64, 'nan', DEV)
                    assert cluster.basis_combine(Q, n, j, _dev(S), out=out, blocks=blocks) is out
                    got = out.cpu().numpy()
                    chk(str((n, j, m, blocks)))
                    assert np.isnan(got[:, n:]).all()
                    first = got if first is None else first
                    assert np.array_equal(got[:, :n], first[:, :n]), (n, j, m, blocks, again)
            assert (np.abs(first[:, :n].T - ref) <= j * U * mass).all(), (n, j, m)


# ---- (d) the solver ----------------------------------------------------------------------------------------------------------------
_maps = {}


def _map_of(name):
    from oriana_amd import cluster
    if name not in _maps:
        _maps[name] = cluster.diffusion_map(_ref_graph(name), n_comps=dc.N_COMPS, tol=TOL)
    return _maps[name]


def _true_residuals(T, lam, psi):
    return np.linalg.norm(T @ psi - psi * lam, axis=0)


def _check_pairs(out, r, m, what):
    """The derived bounds of an eigenpair set against the reference matrix and spectrum; returns the true residuals."""
    lam, psi = out['eigenvalues'], out['components'].cpu().numpy()
    assert lam.shape == (m,) and psi.shape == (r['T'].shape[0], m) and (np.diff(lam) <= 0).all(), what
    res = _true_residuals(r['T'], lam, psi)
    print('%s: steps %d, true residuals <= %.3e, estimates <= %.3e' % (what, out['steps'], res.max(), out['residuals'].max()))
    assert (res <= TOL + 1e-12).all(), what
    assert (np.abs(lam - r['eigenvalues'][:m]) <= res + 1e-12).all(), what                  # (a missed eigenvalue fails here)
    gap = dc.gaps(r['spectrum'], m)
    assert (1.0 - np.abs((psi * r['components'][:, :m]).sum(0)) <= (res / gap) ** 2 + 1e-12).all(), what
    assert np.abs(psi.T @ psi - np.eye(m)).max() <= 1e-12, what
    assert np.array_equal(psi, dr.sign_rule(psi)), what
    return res


@pytest.mark.parametrize('name', dc.CONNECTED)
def test_diffusion_map_against_eigh(name):
    from oriana_amd import cluster
    out = _map_of(name)
    r = dc.reference(name)
    assert out['converged'] and out['steps'] < r['T'].shape[0] and out['components'].is_cuda
    _check_pairs(out, r, dc.N_COMPS, name)
    for kw in ({}, {'blocks': 3}):
        again = cluster.diffusion_map(_ref_graph(name), n_comps=dc.N_COMPS, tol=TOL, **kw)
        assert again['steps'] == out['steps'] and np.array_equal(again['eigenvalues'], out['eigenvalues'])
        assert torch.equal(again['components'], out['components']), kw
    # the same run from the graph the device formed, and from an explicit start
    own = cluster.diffusion_map(_graph_of(name), n_comps=dc.N_COMPS, tol=TOL, start=dc.start(name))
    _check_pairs(own, r, dc.N_COMPS, name + ' (own graph)')


def test_tiny_runs_to_n_steps_and_is_exact():
    from oriana_amd import cluster
    r = dc.reference('tiny')
    out = cluster.diffusion_map(_graph_of('tiny'), n_comps=5)
    assert out['steps'] == 5
    lam, V, _ = dr.eigh_top(r['T'], 5)
    assert np.abs(out['eigenvalues'] - lam).max() <= 1e-12
    assert (1.0 - np.abs((out['components'].cpu().numpy() * V).sum(0)) <= 1e-12).all()


def test_max_steps_is_reported_and_islands_are_refused():
    from oriana_amd import cluster
    g = _ref_graph('blobs2000')
    out = cluster.diffusion_map(g, n_comps=dc.N_COMPS, tol=TOL, max_steps=20)
    assert out['converged'] is False and out['steps'] == 20 and out['eigenvalues'].shape == (dc.N_COMPS,)
    with pytest.raises(ValueError, match='2 connected components'):
        cluster.diffusion_map(_graph_of('two_islands'))
    n = g['n']
    for kw in (dict(n_comps=0), dict(n_comps=21, max_steps=20), dict(n_comps=n + 1), dict(start=np.zeros(n)), dict(start=np.ones(n - 1)),
               dict(start=np.full(n, np.nan)), dict(check_every=0), dict(blocks=-1)):
        with pytest.raises(ValueError):
            cluster.diffusion_map(g, **kw)


# ---- (e) pseudotime ----------------------------------------------------------------------------------------------------------------
def test_pseudotime_from_the_reference_eigenpairs():
    from oriana_amd import cluster
    for name in dc.CONNECTED:
        r = dc.reference(name)
        lam, psi = r['eigenvalues'][:dc.N_COMPS], r['components'][:, :dc.N_COMPS]
        for root in (0, 17, psi.shape[0] - 1):
            out = cluster.diffusion_pseudotime(lam, _dev(psi), root)
            d, p = dr.dpt(lam, psi, root)
            assert out['dpt'].is_cuda and (np.abs(out['dpt'].cpu().numpy() - d) <= 32 * U * d).all()
            assert (np.abs(out['pseudotime'].cpu().numpy() - p) <= 32 * U * p).all()


def test_pseudotime_end_to_end_on_the_path():
    from oriana_amd import cluster
    c, r = dc.case('path600'), dc.reference('path600')
    out = _map_of('path600')
    root = int(np.argmin(c['t']))
    got = cluster.diffusion_pseudotime(out['eigenvalues'], out['components'], root)['pseudotime'].cpu().numpy()
    assert dr.spearman(got, c['t']) >= 0.99
    m = dc.N_COMPS
    lam = r['eigenvalues'][:m]
    d_ref, p_ref = dr.dpt(lam, r['components'][:, :m], root)
    res = _true_residuals(r['T'], out['eigenvalues'], out['components'].cpu().numpy())
    gap = dc.gaps(r['spectrum'], m)
    wl = lam[1:] / (1.0 - lam[1:])
    bound = float((wl * 2 * np.sqrt(2) * res[1:] / gap[1:]).sum()) / d_ref.max() + 1e-9
    err = np.abs(got - p_ref).max()
    print('path600: |pseudotime - reference| %.3e, bound %.3e' % (err, bound))
    assert err <= bound


# ---- (f) the models ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,dd', CASES, ids=CASE_IDS)
def test_cell_diffusion_and_pseudotime(name, dd):
    G = _G(name, dd)
    before, fac = G.state(), G.factors()
    k, m = 15, 10
    out = G.cell_diffusion(n_comps=m, n_neighbors=k, tol=TOL)
    nb = G.cell_neighbors(k)
    assert np.array_equal(out['features'], nb['features']) and np.array_equal(out['factors'], np.arange(K))
    T, z, P = dr.dense_transition(nb['indices'], nb['sq_distances'])
    assert dr.components(P).max() == 0
    lam, V, spectrum = dr.eigh_top(T, m + 1)
    r = {'T': T, 'eigenvalues': lam, 'components': V, 'spectrum': spectrum}
    assert out['converged']
    _check_pairs(out, r, m, name)
    for graph in ((nb['indices'], nb['sq_distances']), (torch.as_tensor(nb['indices'], device=G.device), torch.as_tensor(nb['sq_distances'], device=G.device))):
        again = G.cell_diffusion(n_comps=m, graph=graph, tol=TOL, blocks=3)
        assert np.array_equal(again['eigenvalues'], out['eigenvalues']) and torch.equal(again['components'], out['components'])
    cols = np.array([2, 0])
    sub = G.cell_diffusion(n_comps=m, n_neighbors=k, factors=cols, tol=TOL)
    nbs = G.cell_neighbors(k, factors=cols)
    Ts, _, Ps = dr.dense_transition(nbs['indices'], nbs['sq_distances'])
    lam_s, V_s, spec_s = dr.eigh_top(Ts, m + 1)
    assert np.array_equal(sub['factors'], cols) and not np.array_equal(sub['eigenvalues'], out['eigenvalues'])
    _check_pairs(sub, {'T': Ts, 'eigenvalues': lam_s, 'components': V_s, 'spectrum': spec_s}, m, name + ' factors=')
    # pseudotime: computed afresh and from the map above, the same bits; against NumPy on the returned eigenpairs
    root = 3
    pt = G.cell_pseudotime(root, n_comps=m, n_neighbors=k, tol=TOL)
    pt2 = G.cell_pseudotime(root, diffusion=out)
    assert pt['root'] == root and torch.equal(pt['dpt'], pt2['dpt']) and torch.equal(pt['pseudotime'], pt2['pseudotime'])
    d, p = dr.dpt(out['eigenvalues'], out['components'].cpu().numpy(), root)
    assert (np.abs(pt['dpt'].cpu().numpy() - d) <= 32 * U * d).all() and (np.abs(pt['pseudotime'].cpu().numpy() - p) <= 32 * U * p).all()
    assert float(pt['pseudotime'].max()) == 1.0 and float(pt['dpt'][root]) == 0.0
    for bad in (-1, G.n, 2.5):
        with pytest.raises(ValueError, match='root'):
            G.cell_pseudotime(bad, diffusion=out)
    with pytest.raises(ValueError, match='process group'):
        G.cell_diffusion(pg=None)
    with pytest.raises(ValueError, match='process group'):
        G.cell_pseudotime(0, pg=None)
    with pytest.raises(ValueError, match='graph must be'):
        G.cell_diffusion(graph=(nb['indices'][:-1], nb['sq_distances'][:-1]))
    after, fac2 = G.state(), G.factors()
    assert sorted(before) == sorted(after)
    for key in before:
        assert np.array_equal(before[key], after[key], equal_nan=True), key
    for x, y in zip(fac, fac2):
        assert np.array_equal(x, y)


def test_more_than_one_rank_is_refused(monkeypatch):
    from oriana_amd import cluster
    G = _G('GaP', None)
    monkeypatch.setattr(cluster.odist, 'world_size', lambda pg=None: 2)
    with pytest.raises(NotImplementedError, match='more than one rank'):
        cluster.diffusion_map({'crow': None}, pg=object())
    with pytest.raises(NotImplementedError, match='more than one rank'):
        G.cell_diffusion()
    with pytest.raises(NotImplementedError, match='more than one rank'):
        G.cell_pseudotime(0)


def _worker(rank, port, X, out):
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
        d = G.cell_diffusion(n_comps=10, tol=TOL)
        pt = G.cell_pseudotime(3, diffusion=d)
        np.savez(out, eigenvalues=d['eigenvalues'], components=d['components'].cpu().numpy(), steps=d['steps'],
                 pseudotime=pt['pseudotime'].cpu().numpy())
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    # (as tests/test_sharded_gpu.py: leave without the static destructors of the interpreter / c10d)
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(0)


def test_one_rank_process_group_gives_the_same_bits(tmp_path):
    """The one-rank rehearsal group (a fresh child process): the search runs through the model's group, the map is the same."""
    out = str(tmp_path / 'diffusion_sharded.npz')
    mp.spawn(_worker, args=(_free_port(), _X(), out), nprocs=1, join=True)
    got = np.load(out)
    G = _G('GaP', None)
    d = G.cell_diffusion(n_comps=10, tol=TOL)
    assert int(got['steps']) == d['steps'] and np.array_equal(got['eigenvalues'], d['eigenvalues'])
    assert np.array_equal(got['components'], d['components'].cpu().numpy())
    assert np.array_equal(got['pseudotime'], G.cell_pseudotime(3, diffusion=d)['pseudotime'].cpu().numpy())
