# -*- coding: utf-8 -*-
"""The t-SNE layout without a GPU: the float64 restatement against scikit-learn, its optimiser, the conditions the seeded cases
must meet for the bounds of tsne_reference to hold, the plan, the default-neighbour rule and every error that needs no device."""
import numpy as np
import pytest
import torch

import tsne_reference as tr


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from oriana_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def case():
    """300 x 8 blobs, k = 30, perplexity 10: the graph, the reference P and the PCA start."""
    X, _ = tr.blobs()
    idx, d2 = tr.graph(X, 30)
    p, beta, cond = tr.affinities(d2, 10.0)
    P, y0 = tr.joint(idx, p.astype(np.float32)), tr.pca_init(X)
    return {'X': X, 'idx': idx, 'd2': d2, 'p': p, 'beta': beta, 'P': P, 'y0': y0, 'late': tr.optimise(P, y0, 250, 100)}


def test_gradient_and_kl_against_scikit_learn(case):
    ts = pytest.importorskip('sklearn.manifold._t_sne')
    from scipy.spatial.distance import squareform
    P = case['P']
    P = P / P.sum()                                                   # (scikit-learn's objective takes a P that sums to 1)
    for seed, scale in ((1, 1e-4), (2, 1.0), (3, 30.0)):
        Y = tr.layout(seed, 300, scale).astype(np.float64)
        kl, grad = ts._kl_divergence(Y.ravel(), squareform(P, checks=False), 1.0, 300, 2)
        g, k = tr.gradient(P, Y)
        assert abs(k - kl) <= 1e-12 * abs(kl), (scale, k, kl)
        assert np.abs(g.ravel() - grad).max() <= 1e-12 * np.abs(grad).max(), scale


def test_joint_against_scikit_learn(case):
    ts = pytest.importorskip('sklearn.manifold._t_sne')
    from scipy.sparse import csr_matrix
    n, k = case['idx'].shape
    D = csr_matrix((case['d2'].ravel().astype(np.float64), case['idx'].ravel(), np.arange(0, n * k + 1, k)), shape=(n, n))
    want = ts._joint_probabilities_nn(D, 10.0, 0).toarray()
    P = case['P']
    assert np.array_equal(P != 0, want != 0)
    assert np.abs(P - want).max() <= 1e-4 * want.max()
    assert np.array_equal(P, P.T) and abs(P.sum() - 1.0) <= 1e-6


def test_reference_affinities(case):
    for k, perp in tr.AFFINITY_CASES:
        _, d2 = tr.graph(case['X'], k)
        p, beta, cond = tr.affinities(d2, perp)
        assert np.abs(tr.entropy_of(p) - np.log(perp)).max() <= 1e-12
        assert np.abs(p.sum(1) - 1.0).max() <= 1e-14 and np.all(beta > 0)
        assert cond.max() * 1e-9 < 1e-3, (k, perp, cond.max())            # the conditioning the affinity bound assumes
    # padded rows, an all-equal row
    d2 = np.array([[1.0, 2.0, 4.0, np.inf], [3.0, 3.0, 3.0, np.inf], [0.0, 0.0, 1.0, 5.0]], dtype=np.float32)
    p, beta, _ = tr.affinities(d2, 2.0)
    assert np.all(p[:2, 3] == 0.0) and np.all(p[1, :3] == 1.0 / 3) and beta[1] == 1.0
    assert p[2, 0] == p[2, 1] and abs(tr.entropy_of(p)[2] - np.log(2.0)) <= 1e-12


def test_reference_optimiser_halves_the_divergence(case):
    P, y0 = case['P'], case['y0']
    assert abs(y0[:, 0].std() - 1e-4) <= 1e-18 and abs(y0.mean(0)).max() <= 1e-12
    _, start = tr.gradient(P, y0.astype(np.float32))
    y = case['late']
    _, end = tr.gradient(P, y.astype(np.float32))
    print('KL: %.4f -> %.4f' % (start, end))
    assert np.all(np.isfinite(y)) and end <= 0.5 * start


def test_cases_meet_the_assumptions_of_the_bounds(case):
    P = case['P']
    for seed, n, scale in ((11, 300, 1e-4), (12, 300, 1e2), (13, 129, 1.0), (14, 7, 1.0)):
        Y = tr.layout(seed, n, scale)
        assert tr.min_force_term(Y, Y) >= tr.MIN_TERM, (n, scale)
    for scale in (1e-4, 1.0, 1e2):
        Y = tr.layout(21, 300, scale)
        assert tr.kl_bound(P, Y) <= 32 * tr.U, (scale, tr.kl_bound(P, Y) / tr.U)
    assert tr.kl_bound(P, case['late'].astype(np.float32)) <= 32 * tr.U


def test_step_is_scikit_learns_rule():
    y, update, gains = np.zeros((3, 2)), np.array([[1.0, -1.0], [0.0, 2.0], [-3.0, 0.5]]), np.ones((3, 2)) * np.array([1.0, 0.012])
    grad = np.array([[-2.0, -1.0], [1.0, 2.0], [-1.0, -4.0]])
    y1, u1, g1 = tr.step(y, update, gains, grad, 0.5, 10.0)
    inc = update * grad < 0
    assert np.array_equal(g1, np.where(inc, gains + 0.2, np.maximum(gains * 0.8, 0.01)))
    assert g1[0, 1] == 0.01 and np.array_equal(u1, 0.5 * update - 10.0 * g1 * grad) and np.array_equal(y1, u1)


def test_default_neighbors_and_plan(lib):
    from oriana_amd import cluster
    kmax = cluster.max_neighbors(100)
    assert cluster.tsne_default_neighbors(20.0, 100, 10 ** 5) == min(60, kmax) == 60
    assert cluster.tsne_default_neighbors(30.0, 100, 10 ** 5) == kmax
    assert cluster.tsne_default_neighbors(20.0, 100, 41) == 40
    assert cluster.tsne_default_neighbors(3.5, 8, 300) == 11 and cluster.tsne_default_neighbors(3.5, 8, 300, kmax=9) == 9
    by = lib.oriana_tsne_repulse_scratch_bytes_for
    # the size the layout is meant for: one call
    assert cluster.tsne_plan(262144) == (262144, 262144, by(262144, 262144, 0))
    assert cluster.tsne_plan(262144)[2] <= cluster.SCRATCH_BUDGET
    # what the caller fixes stays fixed; the bytes serve every call issued, the shorter last ones included
    qb, chunk, nbytes = cluster.tsne_plan(300, blocks=3, query_block=100, candidate_chunk=128)
    assert (qb, chunk) == (100, 128) and nbytes == max(by(a, b, 3) for a in (100,) for b in (128, 44))
    qb, chunk, nbytes = cluster.tsne_plan(2 ** 22, blocks=2000, budget=1 << 26)
    assert qb % 64 == 0 and nbytes <= 1 << 26 and nbytes >= by(2 ** 22 % qb or qb, 2 ** 22, 2000)
    assert cluster.tsne_plan(300, budget=1)[:2] == (64, 300)                # a small budget ends at one tile, not in a loop
    assert cluster.tsne_plan(0)[:2] == (1, 1)
    for kw in (dict(blocks=-1), dict(query_block=0), dict(candidate_chunk=0)):
        with pytest.raises(ValueError):
            cluster.tsne_plan(300, **kw)


def test_tsne_value_errors_without_a_device(lib):
    from oriana_amd import cluster
    Y = torch.randn(40, 4, generator=torch.Generator().manual_seed(0))
    g = (np.zeros((40, 12), np.int32), np.zeros((40, 12), np.float32))
    bad = [(Y.double(), {}), (torch.zeros(40), {}), (Y.numpy(), {}), (torch.zeros(40, 8)[:, ::2], {}), (torch.zeros(3, 4), {}),
           (torch.zeros(40, 0), {}), (torch.zeros(40, 300), {}),
           (Y, dict(perplexity=0.5)), (Y, dict(perplexity=float('nan'))), (Y, dict(perplexity=30.0)), (Y, dict(perplexity=5.0, n_neighbors=9)),
           (Y, dict(n_neighbors=0)), (Y, dict(n_neighbors=40)), (Y, dict(perplexity=5.0, n_neighbors=1000)),
           (Y, dict(n_iter=-1)), (Y, dict(n_iter=10, exaggeration_iter=11)), (Y, dict(exaggeration_iter=-1)), (Y, dict(check_every=0)),
           (Y, dict(early_exaggeration=0.5)), (Y, dict(learning_rate=0.0)), (Y, dict(learning_rate=-1.0)),
           (Y, dict(init='bogus')), (Y, dict(init=np.zeros((39, 2)))), (Y, dict(init=np.full((40, 2), np.nan))),
           (Y, dict(graph=(g[0], g[1][:, :11]))), (Y, dict(graph=g, n_neighbors=10)), (Y, dict(graph=g, perplexity=7.0)),
           (Y, dict(graph=(g[0][:39], g[1][:39]))), (Y, dict(bogus=1)),
           (Y, dict(perplexity=5.0))]                                            # (the last: a CPU tensor)
    for T, kw in bad:
        with pytest.raises(ValueError):
            cluster.tsne(T, **kw)


def test_raw_calls_check_their_tensors_without_a_device(lib):
    from oriana_amd import cluster
    Q, Y = torch.zeros(70, 2), torch.zeros(300, 2)
    for bad in (dict(Q=torch.zeros(70, 3)), dict(Q=Q.double()), dict(Q=torch.zeros(70, 4)[:, ::2]), dict(Y=torch.zeros(300)),
                dict(accumulate=True), dict(rep=torch.zeros(70, 2)), dict(rep=torch.zeros(71, 2, dtype=torch.float64)),
                dict(zrow=torch.zeros(70, 1, dtype=torch.float64)), dict(scratch=torch.empty(16, dtype=torch.uint8)), dict(blocks=-1)):
        kw = dict(Q=Q, Y=Y)
        kw.update(bad)
        with pytest.raises((ValueError, cluster._lib.OrianaHipError)):
            cluster.tsne_repulse(**kw)
    for D, perp in ((torch.zeros(4, 3, dtype=torch.float64), 2.0), (torch.zeros(4, 3), 0.5), (torch.zeros(12), 2.0),
                    (torch.zeros(4, 6)[:, ::2], 2.0), (torch.tensor([[1.0, 2.0, float('inf')]]), 2.0)):
        with pytest.raises(ValueError):
            cluster.tsne_affinities(D, perp)
    with pytest.raises(ValueError):
        cluster.tsne_joint(torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 2))
    with pytest.raises(ValueError):
        cluster.tsne_joint(torch.zeros(4, 3), torch.zeros(4, 3))
    P = {'crow': torch.zeros(5, dtype=torch.int64), 'col': torch.zeros(0, dtype=torch.int32), 'val': torch.zeros(0), 'n': 4,
         'sum': torch.zeros((), dtype=torch.float64)}
    for Pb, Yb in ((P, torch.zeros(5, 2)), (dict(P, col=torch.zeros(0, dtype=torch.int64)), torch.zeros(4, 2)), (P, torch.zeros(4, 3)),
                   (None, torch.zeros(4, 2))):
        with pytest.raises(ValueError):
            cluster.tsne_attract(Pb, Yb)
        with pytest.raises(ValueError):
            cluster.tsne_gradient(Pb, Yb)


def test_joint_on_cpu_tensors(case):
    """tsne_joint is torch alone: it runs on CPU tensors, and its CSR equals the reference's exactly in structure."""
    from oriana_amd import cluster
    idx, p32 = case['idx'].copy(), case['p'].astype(np.float32)
    idx[7, 3:] = -1                                                             # padding, and an exact zero
    p32[9, 4] = 0.0
    P = cluster.tsne_joint(torch.from_numpy(idx), torch.from_numpy(p32))
    crow, col, val = tr.csr_of(tr.joint(idx, np.where(idx >= 0, p32, 0.0)))
    assert np.array_equal(P['crow'].numpy(), crow) and np.array_equal(P['col'].numpy(), col)
    assert P['col'].dtype == torch.int32 and P['val'].dtype == torch.float32 and P['crow'].dtype == torch.int64
    assert np.all(np.abs(P['val'].numpy().astype(np.float64) - val) <= 2 * tr.U * val)
    assert abs(float(P['sum']) - val.astype(np.float64).sum()) <= 1e-12


def test_sharded_layouts_are_refused_without_a_device(monkeypatch):
    from oriana_amd import cluster
    from oriana_amd.models import GaP
    monkeypatch.setattr(cluster.odist, 'world_size', lambda pg=None: 2)
    with pytest.raises(NotImplementedError, match='more than one rank'):
        cluster.tsne(torch.zeros(40, 4), pg=object())
    m = object.__new__(GaP)
    m.k, m.pg = 6, object()
    with pytest.raises(NotImplementedError, match='more than one rank'):
        m.cell_layout()
    for kw in (dict(features='bogus'), dict(factors=[6]), dict(factors=[]), dict(pg=None)):
        with pytest.raises(ValueError):
            m.cell_layout(**kw)
