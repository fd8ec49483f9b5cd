# -*- coding: utf-8 -*-
"""The NumPy restatement of the diffusion map (tests/diffusion_reference.py) against numpy.linalg.eigh and the properties the
transition matrix has by construction, the conditions under which the GPU tests are meaningful (connected cases, separated
eigenvalues, a pseudotime that orders the path), and the argument errors of the Python functions and the C entries, all without
a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import diffusion_cases as dc
import diffusion_reference as dr

EINVAL = -1


@pytest.mark.parametrize('name', dc.CONNECTED + ('tiny',))
def test_reference_transition_matrix(name):
    """Symmetric bit for bit; the top eigenvalue is 1 to 1e-12 with the eigenvector sqrt(z) / ||sqrt(z)||."""
    r = dc.reference(name)
    T, z = r['T'], r['z']
    assert np.array_equal(T, T.T) and np.array_equal(r['P'], r['P'].T) and not r['P'].diagonal().any()
    assert (T[r['P']] > 0).all() and (T[~r['P']] == 0).all()
    assert abs(r['eigenvalues'][0] - 1.0) <= 1e-12
    v0 = np.sqrt(z) / np.linalg.norm(np.sqrt(z))
    assert np.abs(r['components'][:, 0] - v0).max() <= 1e-12       # (all entries positive: the sign rule leaves it as it is)
    assert np.abs(T @ v0 - v0).max() <= 1e-14


@pytest.mark.parametrize('name', dc.CONNECTED)
def test_cases_are_connected_with_separated_eigenvalues(name):
    r = dc.reference(name)
    assert r['labels'].max() == 0
    assert np.min(-np.diff(r['eigenvalues'][:dc.N_COMPS + 1])) >= 1e-5


def test_two_islands_has_two_components():
    r = dc.reference('two_islands')
    assert r['labels'].max() == 1 and np.array_equal(r['labels'], np.arange(400) % 2)


@pytest.mark.parametrize('name', dc.CONNECTED)
def test_reference_lanczos_matches_eigh(name):
    """At tol 1e-10: every eigenvalue within its true residual + 1e-12 of eigh's (the CPU runs showed <= 7e-15), the vectors
    within the Davis-Kahan bound."""
    r = dc.reference(name)
    T = r['T']
    L = dr.lanczos(T, dc.start(name), dc.N_COMPS, tol=1e-10)
    assert L['converged'] and L['steps'] < T.shape[0]
    lam, psi = L['eigenvalues'], L['components']
    true = np.linalg.norm(T @ psi - psi * lam, axis=0)
    assert (true <= 1e-10 + 1e-12).all()
    assert (np.abs(lam - r['eigenvalues'][:dc.N_COMPS]) <= true + 1e-12).all()
    gap = dc.gaps(r['spectrum'], dc.N_COMPS)
    overlap = np.abs((psi * r['components'][:, :dc.N_COMPS]).sum(0))
    assert (1.0 - overlap <= (true / gap) ** 2 + 1e-12).all()
    assert np.abs(psi.T @ psi - np.eye(dc.N_COMPS)).max() <= 1e-12


def test_reference_pseudotime_orders_the_path():
    """The condition under which the end-to-end GPU test means something: Spearman >= 0.99 against the curve parameter."""
    c, r = dc.case('path600'), dc.reference('path600')
    root = int(np.argmin(c['t']))
    d, p = dr.dpt(r['eigenvalues'][:dc.N_COMPS], r['components'][:, :dc.N_COMPS], root)
    assert d[root] == 0 and p.max() == 1.0
    assert dr.spearman(p, c['t']) >= 0.99


def test_star_is_what_it_claims():
    crow, col, val, x = dc.star()
    assert np.diff(crow)[0] == 5000 and np.diff(crow)[1:].max() == 1 and crow[-1] == col.size == val.size == 10000


def test_reference_refusals():
    idx, d2 = (a.copy() for a in (dc.case('path600')['indices'], dc.case('path600')['sq_distances']))
    idx[7, 3] = idx[7, 0]
    with pytest.raises(ValueError, match='twice'):
        dr.dense_transition(idx, d2)
    idx, d2 = (a.copy() for a in (dc.case('path600')['indices'], dc.case('path600')['sq_distances']))
    d2[5] = 0
    d2[9] = 0
    with pytest.raises(ValueError, match='2 rows'):
        dr.dense_transition(idx, d2)
    d2[5, 3] = 0.25                                                # a zero median, replaced by the smallest positive value
    d2[9, 0] = 0.5
    assert dr.local_scale(idx, d2)[5] == 0.25 and dr.local_scale(idx, d2)[9] == 0.5


# ---- the ValueErrors of the Python functions: before any launch --------------------------------------------------------------------
def _host_graph():
    crow, col, val = dc.reference('tiny')['csr']
    return {'crow': torch.as_tensor(crow), 'col': torch.as_tensor(col), 'weight': torch.as_tensor(val), 'n': 5}


def test_diffusion_graph_value_errors():
    from oriana_amd import cluster
    idx, d2 = torch.as_tensor(dc.case('tiny')['indices']), torch.as_tensor(dc.case('tiny')['sq_distances'])
    for bad_i, bad_d in ((idx.to(torch.int64), d2), (idx[0], d2[0]), (idx[:, :0], d2[:, :0]), (idx, d2.to(torch.float64)),
                         (idx, d2[:, :1]), (idx, d2.numpy())):
        with pytest.raises(ValueError):
            cluster.diffusion_graph(bad_i, bad_d)
    with pytest.raises(ValueError, match='device'):
        cluster.diffusion_graph(idx, d2)


def test_check_graph_by_weight_dtype():
    """The float64 form of _check_graph; for int64 graphs it is what it was."""
    from oriana_amd import cluster
    g = _host_graph()
    crow, col, w, n, rows, deg, two_m = cluster._check_graph(g, torch.float64)
    assert deg is None and two_m is None and n == 5 and np.array_equal(rows.numpy(), np.repeat(np.arange(5), np.diff(g['crow'].numpy())))
    with pytest.raises(ValueError, match='weight int64'):
        cluster._check_graph(g)
    with pytest.raises(ValueError, match='weight float64'):
        cluster._check_graph(dict(g, weight=g['weight'].to(torch.int64)), torch.float64)
    for v, msg in ((float('nan'), 'finite'), (float('inf'), 'finite'), (-1.0, 'finite and not negative')):
        w2 = g['weight'].clone()
        w2[:] = v
        with pytest.raises(ValueError, match=msg):
            cluster._check_graph(dict(g, weight=w2), torch.float64)
    w2 = g['weight'].clone()
    w2[0] += 1.0
    with pytest.raises(ValueError, match='asymmetric'):
        cluster._check_graph(dict(g, weight=w2), torch.float64)
    gi = dict(g, weight=torch.ones(int(g['col'].numel()), dtype=torch.int64))
    out = cluster._check_graph(gi)
    assert out[6] == int(g['col'].numel()) and np.array_equal(out[5].numpy(), np.diff(g['crow'].numpy()))
    with pytest.raises(ValueError, match='must not be negative$'):
        cluster._check_graph(dict(gi, weight=-gi['weight']))


def test_graph_components_on_the_host():
    """Integer torch only: runs without a GPU.  Zero weights count as absent; the labels are numbered by the smallest member."""
    from oriana_amd import cluster
    for name in ('tiny', 'two_islands', 'path600'):
        r = dc.reference(name)
        crow, col, val = r['csr']
        out = cluster.graph_components({'crow': torch.as_tensor(crow), 'col': torch.as_tensor(col), 'weight': torch.as_tensor(val),
                                        'n': crow.size - 1})
        assert out['n_components'] == r['labels'].max() + 1 and np.array_equal(out['labels'].numpy(), r['labels'])
    # a path 0 - 1 - ... - 99 cut by a zero weight between 49 and 50, as an integer graph
    n = 100
    i = np.arange(n - 1)
    I, J = np.concatenate([i, i + 1]), np.concatenate([i + 1, i])
    order = np.lexsort((J, I))
    I, J = I[order], J[order]
    w = np.where(np.minimum(I, J) == 49, 0, 1).astype(np.int64)
    crow = np.concatenate([[0], np.cumsum(np.bincount(I, minlength=n))]).astype(np.int64)
    out = cluster.graph_components({'crow': torch.as_tensor(crow), 'col': torch.as_tensor(J.astype(np.int32)), 'weight': torch.as_tensor(w),
                                    'n': n})
    assert out['n_components'] == 2 and np.array_equal(out['labels'].numpy(), (np.arange(n) >= 50).astype(np.int64))


def test_diffusion_map_value_errors(monkeypatch):
    from oriana_amd import cluster
    g = _host_graph()
    with pytest.raises(ValueError, match='device'):
        cluster.diffusion_map(g)
    with pytest.raises(ValueError, match='weight float64'):
        cluster.diffusion_map(dict(g, weight=g['weight'].to(torch.int64)))
    monkeypatch.setattr(cluster.odist, 'world_size', lambda pg=None: 2)
    with pytest.raises(NotImplementedError, match='more than one rank'):
        cluster.diffusion_map({'crow': None}, pg=object())


def test_diffusion_pseudotime_on_the_host():
    """Torch on the device of `components`: on the host it is the reference within 32 x 2^-52 relative (every step before the
    root is the same bits; the two libraries' square roots are not), and it refuses a root outside [0, n)."""
    from oriana_amd import cluster
    r = dc.reference('path600')
    lam, psi = r['eigenvalues'][:dc.N_COMPS], r['components'][:, :dc.N_COMPS]
    out = cluster.diffusion_pseudotime(lam, torch.as_tensor(np.ascontiguousarray(psi)), 17)
    d, p = dr.dpt(lam, psi, 17)
    assert np.array_equal(out['dpt'].numpy() ** 2 > 0, d > 0) and out['dpt'][17] == 0
    assert (np.abs(out['dpt'].numpy() - d) <= 32 * 2.0 ** -52 * d).all() and (np.abs(out['pseudotime'].numpy() - p) <= 32 * 2.0 ** -52 * p).all()
    for root in (-1, 600, 1.5, True):
        with pytest.raises(ValueError, match='root'):
            cluster.diffusion_pseudotime(lam, torch.as_tensor(np.ascontiguousarray(psi)), root)
    with pytest.raises(ValueError):
        cluster.diffusion_pseudotime(lam[:3], torch.as_tensor(np.ascontiguousarray(psi)), 0)


# ---- ORIANA_EINVAL of the C entries: before any HIP call ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from oriana_amd import _lib
    return _lib.load()


def test_entries_return_einval_without_a_gpu(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    big = 1 << 20
    assert lib.oriana_basis_tile_rows() >= 64
    # SpMV
    assert lib.oriana_csr_spmv_f64(-1, p, p, p, p, p, 0, None) == EINVAL
    assert lib.oriana_csr_spmv_f64(1 << 31, p, p, p, p, p, 0, None) == EINVAL
    assert lib.oriana_csr_spmv_f64(4, p, p, p, p, p, -1, None) == EINVAL
    for hole in range(3):
        args = [p, p, p, p, p]
        args[(0, 3, 4)[hole]] = None
        assert lib.oriana_csr_spmv_f64(4, *args, 0, None) == EINVAL
    assert lib.oriana_csr_spmv_f64(0, None, None, None, None, None, 0, None) == 0
    # the scratch size
    need = lib.oriana_basis_orthogonalize_scratch_bytes_for
    assert need(-1, 1) == EINVAL and need(4, 0) == EINVAL and need(4, -3) == EINVAL
    t = lib.oriana_basis_tile_rows()
    for n, j in ((1, 1), (t, 5), (t + 1, 5), (3 * t + 5, 130)):
        tiles = -(-n // t)
        assert need(n, j) >= 8 * (tiles * j + j + tiles) and need(n, j) % 16 == 0
    # orthogonalize: (n, Q, ldq, j, w, h, beta2, passes, scratch, scratch_bytes, blocks, stream)
    ok = dict(n=4, Q=p, ldq=4, j=2, w=p, h=p, beta2=p, passes=2, scratch=p, scratch_bytes=big, blocks=0)

    def orth(**kw):
        a = dict(ok, **kw)
        return lib.oriana_basis_orthogonalize_f64(a['n'], a['Q'], a['ldq'], a['j'], a['w'], a['h'], a['beta2'], a['passes'], a['scratch'],
                                                  a['scratch_bytes'], a['blocks'], None)
    for kw in (dict(n=-1), dict(ldq=3), dict(ldq=2), dict(n=3, ldq=3), dict(n=3, ldq=5), dict(j=0), dict(j=-2), dict(passes=0), dict(passes=3),
               dict(blocks=-1), dict(scratch_bytes=-1), dict(scratch_bytes=need(4, 2) - 1), dict(Q=None), dict(w=None), dict(h=None),
               dict(beta2=None), dict(scratch=None), dict(Q=p + 8), dict(w=p + 8), dict(scratch=p + 8)):
        assert orth(**kw) == EINVAL, kw
    assert orth(n=0, Q=None, w=None, ldq=0) == 0
    # append: (n, Q, ldq, j, w, beta2, stream)
    for args in ((-1, p, 4, 1, p, p), (4, p, 3, 1, p, p), (4, p, 5, 1, p, p), (4, p, 4, -1, p, p), (4, None, 4, 1, p, p), (4, p, 4, 1, None, p),
                 (4, p, 4, 1, p, None), (4, p + 8, 4, 1, p, p)):
        assert lib.oriana_basis_append_f64(*args, None) == EINVAL, args
    assert lib.oriana_basis_append_f64(0, None, 0, 0, None, None, None) == 0
    # combine: (n, Q, ldq, j, S, m, out, ldo, blocks, stream)
    for args in ((-1, p, 4, 2, p, 2, p, 4, 0), (4, p, 3, 2, p, 2, p, 4, 0), (4, p, 5, 2, p, 2, p, 4, 0), (4, p, 4, 0, p, 2, p, 4, 0),
                 (4, p, 4, 2, p, -1, p, 4, 0), (4, p, 4, 2, p, 2, p, 3, 0), (4, p, 4, 2, p, 2, p, 5, 0), (4, p, 4, 2, p, 2, p, 4, -1),
                 (4, None, 4, 2, p, 2, p, 4, 0), (4, p, 4, 2, None, 2, p, 4, 0), (4, p, 4, 2, p, 2, None, 4, 0), (4, p, 4, 2, p, 2, p + 8, 4, 0)):
        assert lib.oriana_basis_combine_f64(*args, None) == EINVAL, args
    assert lib.oriana_basis_combine_f64(4, p, 4, 2, None, 0, None, 4, 0, None) == 0
    assert lib.oriana_basis_combine_f64(0, None, 0, 1, None, 3, None, 0, 0, None) == 0
