# -*- coding: utf-8 -*-
"""GaP.partial_fit() and its kernel, oriana_svi_gene_update, on the GPU against the float64 restatement of tests/svi_reference.py.

Shapes are those of tests/test_elbo_gpu.py (805 x 301: a partial last tile on both sides, an all-zero gene, an all-zero cell;
one K per Kp family); the end-to-end stream is the planted 293 x 131, K = 3 case of tests/test_partial_fit_host.py."""
import numpy as np
import pytest
import torch

import gamma_update_reference as gr
import svi_reference as svi
from helpers import RTOL, err_colrel
from test_elbo_gpu import DENSE_DENSITY, HYBRID_KS, KS, M_COLS, N_ROWS, _counts, _model, _planted

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
ZERO_ROW = 17                     # the all-zero row of the kernel tests' Z
# ... and every K of gamma_update_reference.VEC_K (each k_svi_gene_update_vec<FIN, VEC, LPR>: four, two and one factor per lane at
# 8, 16, 32 and 64 lanes per row) with 101 and 127, odd above 64: the element-per-lane kernel, as 129
KERNEL_KS = tuple(sorted(set(KS) | set(gr.VEC_K[4] + gr.VEC_K[2] + gr.VEC_K[1]) | {101, 127}))
MAT_KS = (100, 50, 33, 101)        # the matrix entry: once per VEC, and the element-per-lane kernel


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------

def _operands(K, m=M_COLS, seed=0):
    """Old b1, b2, priors, Z >= 0 (float32, sparse, one all-zero row) and sum_u of a blend, on the device."""
    rng = np.random.default_rng(500 + K + seed)
    Z = (rng.gamma(2.0, 20.0, size=(m, K)) * (rng.random((m, K)) < 0.4)).astype(np.float32)
    Z[ZERO_ROW] = 0
    host = dict(b1=rng.gamma(1.0, 5.0, size=(m, K)) + 1e-3, b2=rng.gamma(2.0, 3.0, size=(m, K)) + 1e-3,
                beta1=rng.random(K) + 0.5, beta2=rng.random(K) + 0.5, Z=Z, sum_u=rng.random(K) * 100)
    return host, {k: torch.from_numpy(v).cuda() for k, v in host.items()}


def _svi(d, scale, rho, F=None, R=None, nslab=1, idx=None, into=None, rate=None):
    """One oriana_svi_gene_update on clones of d's b1, b2, Z: (b1, b2, E, Elog, sums (2, K), Z).  rate: an (m, K) float64 matrix
    in place of sum_u, through oriana_svi_gene_update_mat."""
    from oriana_amd._lib import call, ptr, stream_ptr
    m, K = d['b1'].shape
    if into is None:
        into = (d['b1'].clone(), d['b2'].clone(), torch.empty(m, K, dtype=F64, device='cuda'), torch.zeros(2, K, dtype=F64, device='cuda'))
    b1, b2, E, sums = into
    El = torch.empty(m, K, dtype=F32, device='cuda')
    Z = d['Z'].clone()
    call('oriana_svi_gene_update' if rate is None else 'oriana_svi_gene_update_mat', ptr(b1), ptr(b2), ptr(E), ptr(El), ptr(sums[0]),
         ptr(sums[1]), ptr(d['beta1']), ptr(d['beta2']), ptr(Z), ptr(F), ptr(R), nslab, ptr(idx), ptr(d['sum_u'] if rate is None else rate),
         float(scale), float(rho), m, K, stream_ptr())
    torch.cuda.synchronize()
    return b1, b2, E, El, sums, Z


def _stored_pair_expectations(b1, b2):
    """oriana_gamma_update(Z = NULL) on the pair: (E, Elog, sums)."""
    from oriana_amd._lib import call, ptr, stream_ptr
    m, K = b1.shape
    E, El, sums = torch.empty_like(b1), torch.empty(m, K, dtype=F32, device='cuda'), torch.zeros(2, K, dtype=F64, device='cuda')
    call('oriana_gamma_update', ptr(b1), ptr(b2), ptr(E), ptr(El), ptr(sums[0]), ptr(sums[1]), None, None, None, None, None, None,
         None, m, K, stream_ptr())
    torch.cuda.synchronize()
    return E, El, sums


def _gamma_update(d, F=None, R=None, nslab=1, idx=None):
    """oriana_gamma_update[_finalize] with prior + Z and rate_vec = sum_u: (b1, b2, E, Elog, sums, Z)."""
    from oriana_amd._lib import call, ptr, stream_ptr
    m, K = d['b1'].shape
    b1, b2, E = (torch.empty(m, K, dtype=F64, device='cuda') for _ in range(3))
    El, sums, Z = torch.empty(m, K, dtype=F32, device='cuda'), torch.zeros(2, K, dtype=F64, device='cuda'), d['Z'].clone()
    if F is None:
        call('oriana_gamma_update', ptr(b1), ptr(b2), ptr(E), ptr(El), ptr(sums[0]), ptr(sums[1]), ptr(d['beta1']), ptr(d['beta2']),
             ptr(Z), None, ptr(d['sum_u']), None, None, m, K, stream_ptr())
    else:
        call('oriana_gamma_update_finalize', ptr(b1), ptr(b2), ptr(E), ptr(El), ptr(sums[0]), ptr(sums[1]), ptr(d['beta1']),
             ptr(d['beta2']), ptr(Z), ptr(F), ptr(R), nslab, ptr(idx), ptr(d['sum_u']), m, K, stream_ptr())
    torch.cuda.synchronize()
    return b1, b2, E, El, sums, Z


def _sums_close(a, b, what):
    rel = float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())
    print('%s: column sums %.3e apart (relative; bound 1e-12)' % (what, rel))
    assert rel <= 1e-12, what


@pytest.mark.parametrize('K', KERNEL_KS)
def test_kernel_against_float64(K):
    scale, rho = 3.7, 0.3
    h, d = _operands(K)
    b1, b2, E, El, sums, Z = _svi(d, scale, rho)
    assert torch.equal(Z, d['Z']), 'the plain form wrote Z'
    ref1 = np.maximum(1e-15, (1 - rho) * h['b1'] + rho * (h['beta1'][None, :] + scale * h['Z'].astype(np.float64)))
    ref2 = np.maximum(1e-15, (1 - rho) * h['b2'] + rho * (h['beta2'] + scale * h['sum_u'])[None, :])
    e1 = float(np.max(np.abs(b1.cpu().numpy() - ref1) / ref1))
    e2 = float(np.max(np.abs(b2.cpu().numpy() - ref2) / ref2))
    print('K=%d: b1 %.3e b2 %.3e relative to NumPy float64 (bound 1e-14)' % (K, e1, e2))
    # three float64 roundings (scale * Z, + beta, the blend's two products and their sum; FMA contraction allowed)
    assert e1 <= 1e-14 and e2 <= 1e-14
    # the expectations: what oriana_gamma_update forms from that stored pair, bit for bit
    E0, El0, sums0 = _stored_pair_expectations(b1, b2)
    assert torch.equal(E, E0) and torch.equal(El, El0)
    _sums_close(sums, sums0, 'K=%d' % K)
    assert torch.isfinite(E).all() and torch.isfinite(El).all()


@pytest.mark.parametrize('K', MAT_KS)
def test_matrix_rate_entry(K):
    """oriana_svi_gene_update_mat: a matrix whose every row is sum_u gives the bits of the vector entry, plain and finalize form;
    a matrix of its own gives b2 against NumPy float64 within the bound of the vector entry, and the expectations of that pair."""
    from oriana_amd import engine
    scale, rho = 3.7, 0.3
    h, d = _operands(K)
    m, Kp = M_COLS, engine.kpad(K)
    rows = d['sum_u'][None, :].expand(m, K).contiguous()
    g = torch.Generator(device='cuda').manual_seed(K)
    F = torch.rand(m, Kp, device='cuda', generator=g)
    R = torch.rand(3, m, Kp, device='cuda', generator=g) * 50
    idx = torch.randperm(m, device='cuda', generator=g).to(torch.int32)
    for fin in ((None, None, 1, None), (F, R, 3, idx)):
        got, ref = _svi(d, scale, rho, *fin, rate=rows), _svi(d, scale, rho, *fin)
        for x, y in zip(got[:4] + got[5:], ref[:4] + ref[5:]):
            assert torch.equal(x, y)
        _sums_close(got[4], ref[4], 'K=%d rows of sum_u' % K)
    rate_h = np.random.default_rng(900 + K).random((m, K)) * 100
    b1, b2, E, El, sums, Z = _svi(d, scale, rho, rate=torch.from_numpy(rate_h).cuda())
    ref2 = np.maximum(1e-15, (1 - rho) * h['b2'] + rho * (h['beta2'][None, :] + scale * rate_h))
    e2 = float(np.max(np.abs(b2.cpu().numpy() - ref2) / ref2))
    print('K=%d: b2 %.3e relative to NumPy float64 (bound 1e-14)' % (K, e2))
    assert e2 <= 1e-14 and torch.equal(b1, _svi(d, scale, rho)[0])
    E0, El0, sums0 = _stored_pair_expectations(b1, b2)
    assert torch.equal(E, E0) and torch.equal(El, El0)
    _sums_close(sums, sums0, 'K=%d matrix rate' % K)


@pytest.mark.parametrize('K', KS)
def test_rho_zero_leaves_the_pair_bit_for_bit(K):
    h, d = _operands(K)
    b1, b2, E, El, sums, Z = _svi(d, 3.7, 0.0)
    assert torch.equal(b1, d['b1']) and torch.equal(b2, d['b2'])
    E0, El0, _ = _stored_pair_expectations(d['b1'], d['b2'])
    assert torch.equal(E, E0) and torch.equal(El, El0)


@pytest.mark.parametrize('K', KS)
def test_rho_one_is_the_gamma_update(K):
    """rho = 1, scale = 1: prior + Z and rate_vec = sum_u -- every output of oriana_gamma_update on the same inputs."""
    h, d = _operands(K)
    got, ref = _svi(d, 1.0, 1.0), _gamma_update(d)
    for x, y in zip(got[:4], ref[:4]):
        assert torch.equal(x, y)
    _sums_close(got[4], ref[4], 'K=%d' % K)


@pytest.mark.parametrize('K', KERNEL_KS)
@pytest.mark.parametrize('perm,nslab', [(True, 1), (False, 3)], ids=['perm', 'slabs'])
def test_finalize_form(K, perm, nslab):
    """Z[o] += F[p] * sum_s R[s][p] folded in: oriana_gamma_update_finalize bit for bit at rho = 1, scale = 1, and at any step
    size the plain form on the Z that oriana_finalize_slabs completes."""
    from oriana_amd import engine
    from oriana_amd._lib import call, ptr, stream_ptr
    h, d = _operands(K, seed=1)
    m, Kp = M_COLS, engine.kpad(K)
    g = torch.Generator(device='cuda').manual_seed(K + nslab)
    F = torch.rand(m, Kp, device='cuda', generator=g)
    R = torch.rand(nslab, m, Kp, device='cuda', generator=g) * 50
    idx = torch.randperm(m, device='cuda', generator=g).to(torch.int32) if perm else None
    got, ref = _svi(d, 1.0, 1.0, F, R, nslab, idx), _gamma_update(d, F, R, nslab, idx)
    for x, y in zip(got[:4] + got[5:], ref[:4] + ref[5:]):
        assert torch.equal(x, y)
    _sums_close(got[4], ref[4], 'K=%d finalize' % K)
    Zfin = d['Z'].clone()
    call('oriana_finalize_slabs', ptr(Zfin), ptr(F), ptr(R), nslab, ptr(idx), m, K, stream_ptr())
    assert torch.equal(got[5], Zfin)
    got = _svi(d, 3.7, 0.3, F, R, nslab, idx)
    ref = _svi(dict(d, Z=Zfin), 3.7, 0.3)
    for x, y in zip(got[:4] + got[5:], ref[:4] + ref[5:]):
        assert torch.equal(x, y)


@pytest.mark.parametrize('K', (20, 129))
def test_entry_at_the_clamp_stays_there(K):
    h, d = _operands(K)
    j, k = 40, K - 1
    d['beta1'][k] = 0.0
    d['Z'][j, k] = 0.0
    d['b1'][j, k] = 1e-15
    b1, b2, E, El, sums, Z = _svi(d, 3.7, 0.3)
    assert float(b1[j, k]) == 1e-15
    assert torch.isfinite(E).all() and torch.isfinite(El).all() and torch.isfinite(sums).all()
    assert float(b1[ZERO_ROW, k]) == max(1e-15, (1 - 0.3) * float(d['b1'][ZERO_ROW, k]))


def _odd_aligned(numel, fill):
    """A float64 view of `numel` elements whose address is 8 mod 16, with guard words before and after: (view, guards)."""
    buf = torch.full((numel + 4,), fill, dtype=F64, device='cuda')
    off = 1 if buf.data_ptr() % 16 == 0 else 2
    v = buf[off:off + numel]
    assert v.data_ptr() % 16 == 8
    return v, (buf[:off], buf[off + numel:])


@pytest.mark.parametrize('K', (20, 100))
def test_unaligned_float64_buffers(K):
    """b1, b2, E and the column sums at 8-mod-16 addresses (K = 100: the element-per-lane kernel; K = 20: one factor per lane):
    the results of the aligned call, nothing written outside."""
    GUARD = -7.25
    h, d = _operands(K)
    m = M_COLS
    from oriana_amd import engine
    Kp = engine.kpad(K)
    for F, R, idx in ((None, None, None), (torch.rand(m, Kp, device='cuda'), torch.rand(m, Kp, device='cuda'),
                                          torch.randperm(m, device='cuda').to(torch.int32))):
        ref = _svi(d, 3.7, 0.3, F, R, 1, idx)
        views, guards = zip(*(_odd_aligned(n, GUARD) for n in (m * K, m * K, m * K, 2 * K)))
        b1, b2, E, sums = views[0].view(m, K), views[1].view(m, K), views[2].view(m, K), views[3].view(2, K)
        b1.copy_(d['b1']); b2.copy_(d['b2']); sums.zero_()
        got = _svi(d, 3.7, 0.3, F, R, 1, idx, into=(b1, b2, E, sums))
        for x, y in zip(got[:4] + got[5:], ref[:4] + ref[5:]):
            assert torch.equal(x, y)
        _sums_close(got[4], ref[4], 'K=%d unaligned' % K)
        for lo, hi in guards:
            assert bool((lo == GUARD).all()) and bool((hi == GUARD).all()) and lo.numel() >= 1 and hi.numel() >= 1, 'a guard word was written'


def test_kernel_argument_errors():
    from oriana_amd import _lib
    from oriana_amd._lib import ptr, stream_ptr
    h, d = _operands(20)
    f = _lib.load().oriana_svi_gene_update
    E, El = torch.empty_like(d['b1']), torch.empty(M_COLS, 20, dtype=F32, device='cuda')

    def rc(K=20, rho=0.3, scale=1.0, m=M_COLS):
        return f(ptr(d['b1']), ptr(d['b2']), ptr(E), ptr(El), None, None, ptr(d['beta1']), ptr(d['beta2']), ptr(d['Z']), None, None, 1,
                 None, ptr(d['sum_u']), scale, rho, m, K, stream_ptr())
    assert rc(K=257) == -2 and rc(K=0) == -1                          # ORIANA_EKRANGE, ORIANA_EINVAL
    assert rc(rho=1.5) == -1 and rc(rho=-0.1) == -1 and rc(rho=float('nan')) == -1 and rc(scale=-1.0) == -1
    assert rc(m=0) == 0


# ---- 2. one call against float64 ----------------------------------------------------------------------------------------------

N_TOTAL, RHO = 5000, 0.4
GENE_KEYS = ('b1', 'b2', 'V_hat', 'log_V_hat')


def _fitted(K, dd, sweeps=2):
    G = _model(_counts(K), K, dense_density=dd, seed=K)
    assert (G.counts.gd >= 32) if dd else G.counts.gd == 0
    for _ in range(sweeps):
        G.step()
    return G


def _cases():
    return [pytest.param(K, dd, id='K%d-%s' % (K, 'hybrid' if dd else 'sliced'))
            for K in KS for dd in ([None, DENSE_DENSITY] if K in HYBRID_KS else [None])]


def _one_call(K, dd, n_iter):
    """The four gene-side errors of one partial_fit call (given start, no freezing) against the reference on the same state."""
    G = _fitted(K, dd)
    Xq = _counts(K + 50)
    a1_0 = np.random.default_rng(70 + K).gamma(1.0, 1.0, size=(N_ROWS, K))
    st = G.state()
    ref, info = svi.partial_fit(Xq, st, N_TOTAL, RHO, a1_0, n_iter, 0.0)
    assert G.partial_fit(Xq, N_TOTAL, rho=RHO, init=a1_0, n_iter=n_iter, tol=0) is G
    got = G.state()
    errs = {k: err_colrel(got[k], ref[k]) for k in GENE_KEYS}
    print('K=%d %s n_iter=%d: %s' % (K, 'hybrid' if dd else 'sliced', n_iter, ' '.join('%s %.3e' % kv for kv in errs.items())))
    assert all(np.isfinite(got[k]).all() for k in GENE_KEYS)
    return errs


@pytest.mark.parametrize('K,dd', _cases())
def test_one_call_against_float64(K, dd):
    errs = _one_call(K, dd, 1)
    assert max(errs.values()) <= RTOL, errs


# Three iterations of the local step before the statistics: the float32 evaluation error of each iteration's sums enters the
# next one's E[log U].  Measured on an MI355X, worst over the nine cases below in err_colrel (each at K = 129 but log_V_hat, K = 100
# hybrid; one iteration: 6.8e-7, 2.5e-7, 4.3e-7, 1.9e-7):
N_ITER3_MEASURED = dict(b1=1.103e-6, b2=7.460e-7, V_hat=3.887e-7, log_V_hat=2.161e-7)
N_ITER3_BOUND = min(1e-4, 3 * max(N_ITER3_MEASURED.values()))       # three times the measured worst value, never above 1e-4


@pytest.mark.parametrize('K,dd', _cases())
def test_three_iterations_against_float64(K, dd):
    errs = _one_call(K, dd, 3)
    assert max(errs.values()) <= N_ITER3_BOUND, errs


# ---- 3. the state after a call is coherent ------------------------------------------------------------------------------------

@pytest.mark.parametrize('K,dd,graph', [(20, None, False), (100, DENSE_DENSITY, False), (20, None, True)],
                         ids=['K20-sliced', 'K100-hybrid', 'K20-graph'])
def test_state_after_a_call_is_what_load_state_leaves(K, dd, graph):
    """Everything a sweep, elbo() and transform() read from the gene side, against a twin that loaded the state."""
    X = _counts(K)
    A = _model(X, K, dense_density=dd, seed=K)
    if graph:
        A.capture_graph()
    for _ in range(2):
        A.step()
    Xb = _counts(K + 50)[:300]
    A.partial_fit(Xb, N_TOTAL, rho=RHO, n_iter=4)
    B = _model(X, K, dense_density=dd, seed=K)
    B.load_state(A.state())
    ea, eb = A.elbo(), B.elbo()
    print('elbo: %.17g against the twin\'s %.17g' % (ea, eb))
    assert abs(ea - eb) <= 1e-9 * abs(eb)
    Xq = _counts(K + 51)[:200]
    a1_0 = np.random.default_rng(K).gamma(1.0, 1.0, size=(200, K))
    ta, tb = (G.transform(Xq, n_iter=1, tol=0, init=a1_0) for G in (A, B))
    assert err_colrel(ta, tb) <= RTOL
    A.step(); B.step()
    sa, sb = A.state(), B.state()
    for k in sa:
        e = err_colrel(sa[k], sb[k])
        print('%s: %.3e' % (k, e))
        assert e <= (1e-12 if k == 'a2' else RTOL), k


# ---- 4. what a call does not write --------------------------------------------------------------------------------------------

def test_cell_side_and_priors_are_not_written():
    K = 20
    G = _fitted(K, None)
    kept = {k: getattr(G, k).tensor.clone() for k in ('a1', 'alpha1', 'alpha2', 'beta1', 'beta2')}
    kept['log_U_hat'] = G._log_U_hat.clone()
    ptrs = tuple(t.data_ptr() for t in (G.b1.tensor, G.b2.tensor, G._V_hat, G._log_V_hat, G._sumV))
    before = G.b1[:].copy()
    Xb = _counts(K + 50)
    assert G.n_batches_ == 0 and G.partial_fit_rho_ is None
    for t, want in enumerate((1.0, 2.0 ** -0.7, 3.0 ** -0.7)):
        G.partial_fit(Xb[100 * t:100 * t + 100], N_TOTAL, n_iter=3)
        assert G.n_batches_ == t + 1 and G.partial_fit_rho_ == want
        assert G.partial_fit_unconverged_ is not None and G._v_sums_in_acc is False
    assert ptrs == tuple(t.data_ptr() for t in (G.b1.tensor, G.b2.tensor, G._V_hat, G._log_V_hat, G._sumV)), 'a buffer was replaced'
    assert not np.array_equal(G.b1[:], before)
    for k, t in kept.items():
        now = G._log_U_hat if k == 'log_U_hat' else getattr(G, k).tensor
        assert torch.equal(now, t), k
    G.partial_fit(Xb[:50], N_TOTAL, rho=0.25, tau0=2.0, kappa=1.0, n_iter=1)
    assert G.partial_fit_rho_ == 0.25 and G.n_batches_ == 4


# ---- 5. the stream ------------------------------------------------------------------------------------------------------------

def test_warm_started_stream_recovers_the_float64_gain():
    """The stream of tests/test_partial_fit_host.py through the GPU model: after 4 and after 8 batches the float64 population
    bound of the model's gene side has at least 90 % of the float64 stream's gain over the warm state."""
    import oriana_amd.models as M
    X, a1, b1, K = _planted()
    n = X.shape[0]
    warm, fit = svi.warm_state(X, a1, b1)
    batches = svi.stream_batches(n, 8)
    ref, states = warm, {}
    for t, rows in enumerate(batches):
        ref, _ = svi.partial_fit(X[rows], ref, n, svi.stream_rho(t), n_iter=300, tol=1e-4)
        states[t + 1] = ref
    base = svi.population_bound(X, warm)
    G = M.GaP(X[:svi.WARM_CELLS], k=K, init=(a1[:svi.WARM_CELLS], b1))
    G.load_state({k: fit[k] for k in ('alpha1', 'alpha2', 'beta1', 'beta2', 'a1', 'a2', 'b1', 'b2')})
    G.update_expectations()
    for t, rows in enumerate(batches):
        G.partial_fit(X[rows], n, n_iter=300, tol=1e-4)
        assert G.partial_fit_unconverged_ == 0 and G.partial_fit_rho_ == svi.stream_rho(t)
        if t + 1 in (4, 8):
            st = G.state()
            got = svi.population_bound(X, {k: st[k] for k in ('alpha1', 'alpha2', 'beta1', 'beta2', 'b1', 'b2')})
            want = svi.population_bound(X, states[t + 1])
            print('after %d batches: GPU %.3f float64 %.3f |GPU - float64| %.3e; gains %.1f against %.1f over the warm %.1f'
                  % (t + 1, got, want, abs(got - want), got - base, want - base, base))
            assert want > base
            assert got - base >= 0.9 * (want - base)
    for k in ('alpha1', 'alpha2', 'beta1', 'beta2'):
        assert np.array_equal(G.state()[k], fit[k]), k


# ---- 6. batches shorter than a tile -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nb', [0, 1, 5])
def test_short_batches(nb):
    K = 20
    G = _fitted(K, None)
    Xb = _counts(9)[12:12 + nb]
    st = G.state()
    sums = G._sumV.clone()
    ver = G._ver
    if nb == 0:
        assert G.partial_fit(Xb, 10, rho=1.0) is G
        now = G.state()
        assert all(np.array_equal(now[k], st[k]) for k in st) and torch.equal(G._sumV, sums)
        assert G.n_batches_ == 0 and G.partial_fit_rho_ is None and G._ver == ver
        return
    assert Xb.any(axis=1).all()
    a1_0 = np.random.default_rng(6).gamma(1.0, 1.0, size=(nb, K))
    # (n_B = 1: n_total = 1, rho = 1 -- b1 = beta1 + x_1j r_1jk, the old gene side multiplied by 0)
    ref, info = svi.partial_fit(Xb, st, nb, 1.0, a1_0, 1, 0.0)
    G.partial_fit(Xb, nb, rho=1.0, init=a1_0, n_iter=1, tol=0)
    got = G.state()
    for k in GENE_KEYS:
        e = err_colrel(got[k], ref[k])
        print('n_B = %d %s: %.3e' % (nb, k, e))
        assert np.isfinite(got[k]).all() and e <= RTOL, k
    assert G.n_batches_ == 1 and torch.isfinite(G._sumV).all()
    G.step()
    assert all(np.isfinite(v).all() for v in G.state().values())


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['ZIGaP', 'SparseGaP', 'SparseZIGaP'])
def test_other_models_say_so(name):
    G = _model(_counts(2)[:300], 5, name=name, seed=2)
    with pytest.raises(NotImplementedError, match='pCMF'):
        G.partial_fit(_counts(3)[:10], 1000)


def test_bad_arguments():
    from oriana_amd import engine
    G = _fitted(20, None, sweeps=0)
    Xb = _counts(1)[:40]
    st = G.state()
    for kw in (dict(tau0=0.0), dict(tau0=-1.0), dict(kappa=0.5), dict(kappa=1.01), dict(rho=-0.01), dict(rho=1.01)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            G.partial_fit(Xb, 1000, **kw)
    with pytest.raises(ValueError, match='n_total'):
        G.partial_fit(Xb, 39)
    with pytest.raises(ValueError, match=r'transform\(\).*genes'):
        G.partial_fit(np.zeros((4, M_COLS + 1)), 1000)
    with pytest.raises(ValueError, match=r'transform\(\).*genes'):
        G.partial_fit(engine.CountTiles.from_dense(_counts(1)[:40, :200], G.device), 1000)
    with pytest.raises(ValueError, match='sliced layout'):
        G.partial_fit(engine.CountTiles.from_dense(_counts(1), G.device, dense_density=DENSE_DENSITY), 1000)
    with pytest.raises(ValueError, match='init'):
        G.partial_fit(Xb, 1000, init=np.ones((41, 20)))
    now = G.state()
    assert all(np.array_equal(now[k], st[k]) for k in st) and G.n_batches_ == 0
