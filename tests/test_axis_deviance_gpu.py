# -*- coding: utf-8 -*-
"""gene_deviance() / cell_deviance() of every model on both layouts against the float64 restatement of
tests/axis_deviance_reference.py, evaluated on the model's own state as tests/test_deviance_path_gpu.py takes it (X as the
float32 counts it holds, U_hat, V_eff = V_hat * S_hat and pi_d in float64, D_hat as the float32 values it holds).  Every
element of the five arrays of both axes is held to its own bound, derived there and never measured on the code under test; a
reference value that is not finite is matched exactly.  Each case prints its largest diff / bound ratio and its bounds."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import axis_deviance_reference as ar
import deviance_path_reference as dr
from test_deviance_path_gpu import _counts, _model, _inputs, _free_port, KP, ALL_MODELS, DENSE_DENSITY, M_COLS

pytestmark = pytest.mark.gpu

LL = ('factors', 'counts', 'mean')


def _reference(G, X):
    X, U, V, pi, keep0, f32_cols = _inputs(G, X)
    return ar.axes(X, U, V, pi, keep0, G.zi, f32_cols=f32_cols)


def _check_both(G, X, what, ref=None):
    ref = _reference(G, X) if ref is None else ref
    got = {'genes': G.gene_deviance(), 'cells': G.cell_deviance()}
    assert got['genes']['factors'].shape == (G.m,) and got['cells']['factors'].shape == (G.n,)
    for axis in ('genes', 'cells'):
        assert sorted(got[axis]) == sorted(ar.KEYS)
        ar.check(got[axis], ref[axis], what='%s %s' % (what, axis))
    return got, ref


def _cases():
    out = [(name, K, None) for name in ALL_MODELS for K in (1, 20, 50, 100)]
    out += [(name, K, None) for name in ('GaP', 'SparseGaP') for K in (129, 200)]
    out += [(name, K, DENSE_DENSITY) for name in ('GaP', 'SparseZIGaP') for K in (20, 100)]
    return [pytest.param(n, K, dd, id='%s-K%d-%s' % (n, K, 'hybrid' if dd else 'sliced')) for n, K, dd in out]


@pytest.mark.parametrize('name,K,dd', _cases())
def test_axis_deviance_against_float64(name, K, dd):
    """Two sweeps from a seeded start, then both axes element by element; and the sum of each axis's three log-likelihoods
    against loglikelihood_X() of the same model within the sum of both bounds (the elements' bounds added up, and the full
    metric's own bound of tests/deviance_path_reference.py at k = K)."""
    X = _counts(K)
    G = _model(name, X, K, dense_density=dd, seed=K)
    assert G._ws.Kp == KP[K]
    if G.zi:
        assert G._mp != G.m, 'the padded gene axis of the dropout kernel is not exercised'
    for _ in range(2):
        G.step()
    what = '%s K=%d %s' % (name, K, 'hybrid' if dd else 'sliced')
    got, ref = _check_both(G, X, what)
    Xr, U, V, pi, keep0, f32_cols = _inputs(G, X)
    full = dr.path(Xr, U, V, pi, keep0, np.arange(K), [K], G.zi, f32_cols=f32_cols)
    c = full['const']
    b_full = {'factors': full['tol_full']['ll_uv'][0], 'counts': dr.ACC * (c['abs_xlx'] + c['abs_lpi']),
              'mean': dr.ACC * (c['abs_mean'] + c['abs_lpi'])}
    for given in LL:
        whole = G.loglikelihood_X(given)
        for axis in ('genes', 'cells'):
            s = float(np.sum(got[axis][given], dtype=np.longdouble))
            bound = float(ref[axis]['tol'][given].sum()) + b_full[given]
            print('%s %s sum of %s: %.17g, loglikelihood_X %.17g, bound %.3e' % (what, axis, given, s, whole, bound))
            if not np.isfinite(whole):          # (a masked factor of a sparse model: the same infinity on both sides)
                assert s == whole == float(np.sum(ref[axis][given], dtype=np.longdouble)), (what, axis, given, s, whole)
                continue
            assert abs(s - whole) <= bound, (what, axis, given, s, whole, bound)


TINY_ROWS = (0, 7, 15, 240, 247, 255, 256 + 16 * 5 + 3, 768 + 7, 800, 804)    # row-in-slice 0 / 7 / 15, slices 0 / 15, last tile
UNDERFLOW_ROWS = (255, 804)                                                   # float32(U_hat) == 0 on these rows


@pytest.mark.parametrize('name,K,dd', [('GaP', 20, None), ('GaP', 20, DENSE_DENSITY), ('SparseZIGaP', 50, None),
                                       ('SparseGaP', 129, None)])
def test_axis_deviance_float64_fallback(name, K, dd):
    """Cells scaled by 1e-13 (rates below 1e-10: the row pass leaves its NaN sentinel) and by 1e-38 more
    (float32(U_hat) == 0), as test_metrics_gpu.test_metric_float64_fallback sets them up: the kernel recomputes their rates
    from the float64 factors, finding the cell from the slot position, and the reference gives these entries ACC alone.  A
    wrong cell makes x log Lambda of that cell differ by orders of magnitude."""
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
    got, ref = _check_both(G, X, '%s K=%d fallback' % (name, K))
    assert torch.isnan(G._ws.s_rs).any(), 'the row pass left no NaN sentinel: the fall-back was not exercised'
    for axis in ('genes', 'cells'):
        assert np.all(np.isfinite(got[axis]['factors']))


@pytest.mark.parametrize('dd', [None, DENSE_DENSITY])
def test_axis_deviance_rate_exactly_zero(dd):
    """S_hat = 0 on a whole gene of a sparse model (hybrid: one dense gene and one sliced gene): the rate is exactly 0 at its
    non-zero counts, so factors = -inf (reconstruction deviance +inf, explained deviance -inf) for those genes and for the
    cells that have a count there -- exactly the elements the reference names -- and finite everywhere else."""
    X = _counts(4)
    K = 20
    G = _model('SparseGaP', X, K, dense_density=dd, seed=4)
    G.step()
    p_s = G.p_s[:].copy()
    genes = [20, 150] if dd else [150]
    if dd:
        pos = {int(j): p for p, j in enumerate(G.counts.col_perm.cpu().numpy())}
        assert pos[20] < G.counts.gd <= pos[150]
    p_s[genes] = 0.0
    G.load_state({'p_s': p_s})
    assert not G.S_hat[genes].any() and all((X[:, j] != 0).any() for j in genes)
    ref = _reference(G, X)
    cells = np.nonzero((X[:, genes] != 0).any(axis=1))[0]
    assert 0 < cells.size < X.shape[0]
    assert np.array_equal(np.nonzero(ref['genes']['factors'] == -np.inf)[0], sorted(genes))
    assert np.array_equal(np.nonzero(ref['cells']['factors'] == -np.inf)[0], cells)
    got, _ = _check_both(G, X, 'rate exactly zero %s' % ('hybrid' if dd else 'sliced'), ref=ref)
    for axis, where in (('genes', sorted(genes)), ('cells', cells)):
        g = got[axis]
        hit = np.zeros(g['factors'].size, dtype=bool)
        hit[where] = True
        assert np.all(g['factors'][hit] == -np.inf) and np.all(g['reconstruction_deviance'][hit] == np.inf)
        assert np.all(g['explained_deviance'][hit] == -np.inf)
        assert np.all(np.isfinite(g['factors'][~hit])) and np.all(np.isfinite(g['reconstruction_deviance'][~hit]))
        assert np.all(np.isfinite(g['counts'])) and np.all(np.isfinite(g['mean']))


@pytest.mark.parametrize('name,quirks,K', [('ZIGaP', False, 20), ('SparseZIGaP', True, 50)])
def test_axis_deviance_dropout_half_boundary(name, quirks, K):
    """M = {round(D_hat) == 0}: a ZI state loaded with p_d = 0.5 (masked: round half to even), one float32 ulp below (masked)
    and one above (kept) at zero counts, as test_metrics_gpu.test_metric_dropout_half_boundary sets it up.  Zeros on both
    sides of 0.5 occur in at least two genes and in at least two cells, so the mask decides elements of both axes."""
    X = _counts(5)
    G = _model(name, X, K, seed=5, reference_quirks=quirks)
    G.step()
    p_d = G.p_d[:].copy()
    zi, zj = np.nonzero(X == 0)
    rng = np.random.default_rng(5)
    pick = rng.permutation(zi.size)[:3 * (zi.size // 6)]
    vals = [np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))]
    for q, v in enumerate(vals):
        sel = pick[q::3]
        p_d[zi[sel], zj[sel]] = np.float64(v)
    G.load_state({'p_d': p_d})
    D = G.D_hat
    for v in vals:
        assert (D == v).sum() > 1000
    masked, kept = (X == 0) & (D <= np.float32(0.5)), (X == 0) & (D > np.float32(0.5))
    assert (masked.any(axis=0) & kept.any(axis=0)).sum() >= 2 and (masked.any(axis=1) & kept.any(axis=1)).sum() >= 2
    assert G._mp % 4 == 0 and G._mp != G.m                  # (the gene axis of the dropout kernel is padded)
    _check_both(G, X, '%s K=%d D_hat = 0.5' % (name, K))


def test_axis_deviance_zero_term_at_k256(monkeypatch):
    """ZIGaP at k = 256 (the float64 sweep): the dropout entry at its largest K, on 300 cells and 37 genes (one partial block
    in both directions, a gene axis padded from 37 to 40)."""
    monkeypatch.setenv('ORIANA_ZI_EXACT', '1')
    n, m, K = 300, 37, 256
    rng = np.random.default_rng(256)
    X = ((rng.poisson(rng.gamma(0.6, 4.0, size=(n, m))) + 1) * (rng.random((n, m)) < 0.3)).astype(np.float64)
    X[:, 5] = 0
    X[11, :] = 0
    G = _model('ZIGaP', X, K, seed=256, reference_quirks=False)
    assert G._ws.Kp == 256 and G._mp == 40
    for _ in range(2):
        G.step()
    _check_both(G, X, 'ZIGaP K=256')


def test_dropout_axes_entry_second_row_slab():
    """oriana_dropout_metric_axes walks the cells in slabs of 65535 x 256 rows: 300 rows more than one slab (4 genes, K = 1, so
    the matrices stay small) put the slab offset on D_hat, U, the mask and the per-cell output.  Against the same term formed
    by float64 tensor arithmetic, within ACC of the absolute terms; a masked stripe of rows straddles the slab boundary."""
    from oriana_amd import _lib
    from oriana_amd._lib import ptr, stream_ptr
    dev = torch.device('cuda', 0)
    slab = 65535 * 256
    n, m, K = slab + 300, 4, 1
    g = torch.Generator(device=dev).manual_seed(11)
    # (rates of 0.25 and more: below ~1e-4 the literal log(pi e^-Lambda + 1 - pi) loses its digits to the rounding of its
    #  argument near 1, on both sides alike, and ACC relative to the term would measure that, not the kernel)
    U = 0.5 + torch.rand(n, K, dtype=torch.float64, device=dev, generator=g) * 3.0
    V = torch.tensor([[0.5], [1.0], [2.0], [0.0]], dtype=torch.float64, device=dev)
    pi = torch.tensor([0.3, 0.6, 0.9, 0.5], dtype=torch.float64, device=dev)
    D = torch.ones(n, m, dtype=torch.float32, device=dev)
    D[slab - 100:slab + 50] = 0.25                           # in the mask M
    D[::7, 1] = 0.5                                          # exactly 0.5 is masked too
    nzmask = torch.zeros(((n + 31) // 32) * m, dtype=torch.int32, device=dev)
    nzmask[((slab + 64) // 32) * m + 2] = -1                 # 32 non-zero counts of gene 2 in the second slab
    gene = torch.zeros(m, dtype=torch.float64, device=dev)
    cell = torch.zeros(n, dtype=torch.float64, device=dev)
    _lib.call('oriana_dropout_metric_axes', ptr(gene), ptr(cell), ptr(D), ptr(U), ptr(V), ptr(pi), ptr(nzmask), n, m, K,
              stream_ptr())
    term = torch.log(pi[None, :] * torch.exp(-(U @ V.t())) + (1.0 - pi[None, :]))
    keep = D > 0.5
    keep[slab + 64:slab + 96, 2] = False
    term = torch.where(keep, term, torch.zeros_like(term))
    for got, ref, a in ((cell, term.sum(1), term.abs().sum(1)), (gene, term.sum(0), term.abs().sum(0))):
        d = (got - ref).abs()
        assert bool((d <= ar.ACC * a).all()), (float(d.max()), float((d / a.clamp(min=1e-300)).max()))
    assert float(cell[slab - 100:slab + 50].abs().max()) == 0.0 and float(cell[slab + 50:].abs().min()) > 0.0
    only_gene = torch.zeros_like(gene)
    _lib.call('oriana_dropout_metric_axes', ptr(only_gene), None, ptr(D), ptr(U), ptr(V), ptr(pi), ptr(nzmask), n, m, K,
              stream_ptr())
    assert bool(((only_gene - gene).abs() <= 2 * ar.ACC * term.abs().sum(0)).all())


def test_axis_deviance_state_launches_and_repeatability():
    """Neither call writes model state (state() is bit-identical afterwards), each computes only its own axis (the other
    output pointer of every kernel is NULL), two calls agree within the float64 accumulation bound (the kernels add with
    float64 atomics), and k > 256 with a dropout node raises ValueError before any launch."""
    from oriana_amd.models import base
    X = _counts(6)
    K = 20
    G = _model('SparseZIGaP', X, K, dense_density=DENSE_DENSITY, seed=6)
    for _ in range(2):
        G.step()
    torch.cuda.synchronize()
    before = {k: np.asarray(v).tobytes() for k, v in G.state().items()}
    launches = []
    real = base.call
    base.call = lambda name, *a: (launches.append((name, a)), real(name, *a))[1]
    try:
        g1 = G.gene_deviance()
        by_name = {name: a for name, a in launches}
        assert by_name['oriana_metric_nnz_axes'][6] is not None and by_name['oriana_metric_nnz_axes'][7] is None
        assert by_name['oriana_dense_metric_axes'][7] is not None and by_name['oriana_dense_metric_axes'][8] is None
        assert by_name['oriana_dropout_metric_axes'][0] is not None and by_name['oriana_dropout_metric_axes'][1] is None
        del launches[:]
        c1 = G.cell_deviance()
        by_name = {name: a for name, a in launches}
        assert by_name['oriana_metric_nnz_axes'][6] is None and by_name['oriana_metric_nnz_axes'][7] is not None
        assert by_name['oriana_dense_metric_axes'][7] is None and by_name['oriana_dense_metric_axes'][8] is not None
        assert by_name['oriana_dropout_metric_axes'][0] is None and by_name['oriana_dropout_metric_axes'][1] is not None
        del launches[:]
        G.k = 257
        try:
            with pytest.raises(ValueError):
                G.gene_deviance()
            with pytest.raises(ValueError):
                G.cell_deviance()
        finally:
            G.k = K
        assert not launches, [name for name, _ in launches]
    finally:
        base.call = real
    after = {k: np.asarray(v).tobytes() for k, v in G.state().items()}
    changed = [k for k in before if after[k] != before[k]]
    assert not changed, 'the calls wrote %s' % changed
    g2, c2 = G.gene_deviance(), G.cell_deviance()
    ref = _reference(G, X)
    for axis, a, b in (('genes', g1, g2), ('cells', c1, c2)):
        for q in ar.KEYS:
            d = ar.diff(a[q], b[q])
            assert np.all(d <= 2 * ref[axis]['tol_acc'][q]), '%s %s: two calls %r apart' % (axis, q, d.max())


def test_axis_deviance_leaves_a_captured_graph_replayable():
    """The calls allocate and launch outside the captured sweep and write none of its buffers: a GaP model with a captured
    graph steps on after them exactly like a twin that never made them."""
    X = _counts(7)
    K = 20
    G, H = _model('GaP', X, K, seed=7), _model('GaP', X, K, seed=7)
    G.capture_graph()
    H.capture_graph()
    G.step(); H.step()
    _check_both(G, X, 'GaP K=20 captured graph')
    G.step(); H.step()
    torch.cuda.synchronize()
    sg, sh = G.state(), H.state()
    for k in ('a1', 'a2', 'b1', 'b2'):
        np.testing.assert_allclose(sg[k], sh[k], rtol=1e-4, err_msg=k)
    _check_both(G, X, 'GaP K=20 after the replay')


# ---- row sharding: a process group of one rank ------------------------------------------------------------------------------

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
        G = M.ZIGaP(counts, k=K, init=(a1, b1), device=dev, process_group=dist.group.WORLD)
        assert G.sharded
        G.fit(2)
        g, c = G.gene_deviance(), G.cell_deviance()
        st = G.state()
        np.savez(out, **{'g_' + k: v for k, v in g.items()}, **{'c_' + k: v for k, v in c.items()},
                 **{'st_' + k: v for k, v in st.items()})
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    # (as tests/test_sharded_gpu.py: leave without the static destructors of the interpreter / c10d)
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(0)


def test_axis_deviance_one_rank_process_group(tmp_path):
    """Under a one-rank process group with ORIANA_FORCE_SHARDED=1 (a fresh child process) the packed gene sums go through the
    all-reduce: on the same state loaded into a single-process model, the same arrays within the float64 accumulation bound,
    and within the reference's bounds."""
    K = 20
    X = _counts(9)
    out = str(tmp_path / 'axes_sharded.npz')
    mp.spawn(_worker, args=(_free_port(), X, K, out), nprocs=1, join=True)
    got = np.load(out)
    G = _model('ZIGaP', X, K, seed=9)
    G.load_state({k[3:]: got[k] for k in got.files if k.startswith('st_')})
    ref = _reference(G, X)
    for axis, pre, one in (('genes', 'g_', G.gene_deviance()), ('cells', 'c_', G.cell_deviance())):
        sharded = {q: got[pre + q] for q in ar.KEYS}
        ar.check(sharded, ref[axis], what='one-rank group %s' % axis)
        for q in ar.KEYS:
            d = ar.diff(one[q], sharded[q])
            assert np.all(d <= 2 * ref[axis]['tol_acc'][q]), '%s %s: sharded and single-process %r apart' % (axis, q, d.max())
