# -*- coding: utf-8 -*-
"""The three held-out ZI entries -- oriana_zi_foldin_rate, oriana_zi_gene_rate, oriana_zi_cell_bound -- called directly, once per
compiled instantiation and per form of the hand-pipelined factor loop (tests/zi_heldout_cases.py; the host test of that table
shows that it reaches all of them), against the float64 statements of tests/zi_foldin_reference.py and
tests/zi_score_reference.py.  Scratch is NaN-filled and of the stated size, outputs are NaN-filled where the entry writes them
and hold a sentinel where it must leave them alone.  The assertions and every bound are those of tests/test_zi_foldin_gpu.py,
tests/test_zi_fold_in_fit_gpu.py and tests/test_zi_score_gpu.py, whose helpers make the calls: none is new.  GPU only.

Largest error / bound seen on an MI355X, per instantiation (printed when the module is done: run with -s).  No case failed.
  rate against float64 (bound RTOL = 1e-5):  k_zi_row <3,0> .011 <3,1> .011 <4,0> .011 <4,1> .024 <5,0> .011 <5,1> .011 <6,0> .011
    <6,1> .020;  k_dropout_sweep_b16 <1,1> .032 <1,2> .036 <2,3> .039 <2,4> .038;  k_dropout_sweep <1> .039 <2> .043 <3> .046 <4> .047
  rate against the storing entry (6e-7): 0 in all 63 cases -- the two kernels of an instantiation are bit-identical; the storing entry
    itself is 6.9e-8 .. 4.7e-7 from float64 in err_colrel at these gene counts (at the body shape the kernels of dense_f32.hip
    3.2e-7 .. 4.7e-7, k_zi_row 1.1e-7 .. 2.4e-7)
  active rows against the all-active run (_twin_bound): 0 everywhere (one gene range: one atomic per element); active = NULL
    bit-identical to an array of ones in the three families
  gene rate, k_gene_rate<1> <2> <3> <4>:  G against float64 (RTOL) .015 .009 .010 .009;  dsum / n' (KEY_ATOL['p_d']) .045 .016 .015
    .018;  G against the stored D_hat^T U (6e-7) .246 .149 .169 .160;  the long batches 1.9e-8 .. 2.8e-8 from float64
  cell bound (dropout_bound), k_dropout_sweep<NT, false, true>:  NT = 1: .006 at the body shape, .051 at 300 x 4;  NT = 2, 3, 4: .006
    .005 .004
"""
import functools

import numpy as np
import pytest
import torch

import zi_foldin_reference as zr
import zi_heldout_cases as zc
import zi_score_reference as zs
from helpers import KEY_ATOL, RTOL, err_colrel
from test_elbo_gpu import _twin_bound
from test_zi_fold_in_fit_gpu import EPS, _gene_rate, _ranges
from test_zi_foldin_gpu import SENTINEL, _f64, _rate, _storing, check_rate, check_rate_skips_inactive
from test_zi_score_gpu import _entry, _splits

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FAMILY = {zc.TILES: 'k_zi_row', zc.B16: 'k_dropout_sweep_b16', zc.F32_FAMILY: 'k_dropout_sweep'}
ARITH = {zc.F32: 'f32', zc.BF16X3: 'bf16x3'}

WORST = {}                   # (entry, instantiation, figure) -> (largest error / bound seen, case)


@pytest.fixture(scope='module', autouse=True)
def _report():
    assert torch.cuda.is_available()
    yield
    for key in sorted(WORST):
        print('largest error / bound, %s %s, %s: %.3f (%s)' % (key + WORST[key]))


def _note(entry, inst, figure, ratio, case):
    key = (entry, inst, figure)
    if ratio >= WORST.get(key, (-1.0, ''))[0]:
        WORST[key] = (float(ratio), case)


def _instantiation(K, arithmetic, m, with_tiles):
    """'kernel<a, b>' of the rate entry for this call, from the dispatch chain itself."""
    from oriana_amd import _lib
    code = int(_lib.load().oriana_zi_dispatch(zc.UPDATE, K, arithmetic, int(with_tiles and m % 4 == 0)))
    assert code >= 0, code
    return '%s<%d,%d>' % (FAMILY[code >> 16], (code >> 8) & 255, code & 255)


def _rate_id(case):
    K, arithmetic, m, with_tiles = case[0], case[1], case[-2], case[-1]
    what = 'K%d-%s-%s%d%s' % (K, ARITH[arithmetic], 'n%d-m' % case[2] if len(case) == 5 else 'm', m, '' if with_tiles else '-noflags')
    try:
        return _instantiation(K, arithmetic, m, with_tiles) + '-' + what
    except Exception:                  # noqa: BLE001  (collected before the library is built: the case still has a name)
        return what


def _nt(K):
    from oriana_amd import _lib
    return (int(_lib.load().oriana_kpad(K)) + 31) // 32


def _form(K):
    nt, form, KS, rem = zc.K_FORMS_TABLE[K]
    return '%s KS=%d' % (form, KS) if rem is None else '%s rem=%d' % (form, rem)


# ---- the float64 references, once per (K, n, m) ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _d64(K, n=zc.N_BODY, m=zc.M_REAL):
    """The float32 dropout posterior of the reference, promoted to float64 (read-only)."""
    X, U, V, pi_d = zc.inputs(K, n, m)
    d = zr.dropout_f32(X, V, pi_d, U)
    assert zc.middle_fraction(d) > zc.MIDDLE_MIN, 'the case does not exercise the sigmoid'
    d = d.astype(np.float64)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _rate_ref(K, n=zc.N_BODY, m=zc.M_REAL):
    ref = _d64(K, n, m) @ zc.inputs(K, n, m)[2]
    ref.setflags(write=False)
    return ref


def _nan_scratch(K, mp):
    from oriana_amd import _lib
    return torch.full((int(_lib.load().oriana_dropout_sweep_scratch_floats(mp, K)),), float('nan'), dtype=torch.float32, device=DEV)


# ---- 1. oriana_zi_foldin_rate, once per instantiation and route -----------------------------------------------------------------

def _check_rate_case(K, arithmetic, n, m_real, mp, with_tiles, tag):
    inst = _instantiation(K, arithmetic, mp, with_tiles)
    X, U, V, pi_d = zc.inputs(K, n, m_real)
    ref = _rate_ref(K, n, m_real)
    scratch = _nan_scratch(K, mp)
    rep = {}
    check_rate(X, U, V, pi_d, ref, arithmetic, scratch=scratch, mp=mp, with_tiles=with_tiles, report=rep)
    print('%s: the storing entry against float64 %.3e' % (tag, rep['stored_float64']))
    _note('rate', inst, 'float64', rep['float64'] / RTOL, tag)
    _note('rate', inst, 'storing twin', rep['storing'] / 6e-7, tag)
    for name, act in zc.inactive_patterns(n).items():
        rep = {}
        scratch.fill_(float('nan'))
        check_rate_skips_inactive(X, U, V, pi_d, act, arithmetic, scratch=scratch, mp=mp, with_tiles=with_tiles, report=rep)
        _note('rate', inst, 'active rows', rep['active'] / rep['active_bound'], tag + ' ' + name)
    return inst


@pytest.mark.parametrize('case', zc.RATE_CASES, ids=_rate_id)
def test_rate_per_instantiation(case):
    """check_rate (float64; the storing entry of the same arithmetic, gene count and flags) and check_rate_skips_inactive under
    the three patterns of inactive cells, at the body shape."""
    K, arithmetic, m, with_tiles = case
    inst = _check_rate_case(K, arithmetic, zc.N_BODY, zc.M_REAL, m, with_tiles, _rate_id(case))
    if arithmetic == zc.BF16X3 and m % 4 == 0 and with_tiles and 36 < K <= 100:
        assert inst.startswith('k_zi_row'), inst
    if m % 4 or not with_tiles or arithmetic == zc.F32:
        assert not inst.startswith('k_zi_row'), inst


@pytest.mark.parametrize('case', zc.RATE_EDGE_CASES, ids=_rate_id)
def test_rate_edge_shapes(case):
    K, arithmetic, n, m, with_tiles = case
    _check_rate_case(K, arithmetic, n, m, m, with_tiles, _rate_id(case))


ONE_PER_FAMILY = ((52, zc.BF16X3), (20, zc.BF16X3), (30, zc.F32))


@pytest.mark.parametrize('K,arithmetic', ONE_PER_FAMILY, ids=lambda v: str(v))
def test_rate_no_active_cell_and_no_flags_array(K, arithmetic):
    """Every cell inactive: DV keeps the sentinel everywhere, the NaN of every U_hat row reaches nothing.  active = NULL is an
    array of ones: bit for bit where two runs over ones agree bit for bit (one gene range: one atomic per element), else within
    the bound on a reordering of the atomics."""
    assert len({_instantiation(k, a, zc.M_ALIGNED, True).split('<')[0] for k, a in ONE_PER_FAMILY}) == 3
    n, mp = zc.N_BODY, zc.M_ALIGNED
    X, U, V, pi_d = zc.inputs(K, n, zc.M_REAL)
    DV = torch.full((n, K), SENTINEL, dtype=torch.float64, device=DEV)
    got = _rate(X, np.full_like(U, np.nan), V, pi_d, arithmetic, active=torch.zeros(n, dtype=torch.uint8, device=DEV), DV=DV,
                scratch=_nan_scratch(K, mp), mp=mp)
    assert np.array_equal(got, np.full((n, K), SENTINEL)), 'a row was written with no cell active'
    ones = torch.ones(n, dtype=torch.uint8, device=DEV)
    a, b = (_rate(X, U, V, pi_d, arithmetic, active=ones, scratch=_nan_scratch(K, mp), mp=mp) for _ in range(2))
    null = _rate(X, U, V, pi_d, arithmetic, active=None, scratch=_nan_scratch(K, mp), mp=mp)
    assert np.isfinite(null).all() and err_colrel(null, _rate_ref(K, n, zc.M_REAL)) <= RTOL
    if np.array_equal(a, b):
        assert np.array_equal(null, a), 'active = NULL differs from an array of ones'
    else:
        e = err_colrel(null, a)
        print('K=%d: two runs over ones differ; NULL against ones %.3e (bound %.3e)' % (K, e, _twin_bound(n, 1)))
        assert e <= _twin_bound(n, 1)


# ---- 2. oriana_zi_gene_rate: k_gene_rate<NT> in every loop form, and past its flush and spill ------------------------------------

def _check_gene_rate(K, n, m_real, mp, tag, storing):
    X, U, V, pi_d = zc.inputs(K, n, m_real)
    d = _d64(K, n, m_real) if n <= zc.N_BODY else zr.dropout_f32(X, V, pi_d, U).astype(np.float64)
    refG, refd = d.T @ U, d.sum(axis=0)
    G, dsum = _gene_rate(X, U, V, pi_d, mp=mp)
    G2, dsum2 = _gene_rate(X, U, V, pi_d, mp=mp)
    S = _ranges(n, K, mp)
    inst = 'k_gene_rate<%d>' % _nt(K)
    e = err_colrel(G[:m_real].cpu().numpy(), refG)
    ed = float(np.max(np.abs(dsum[:m_real].cpu().numpy() - refd))) / n
    print('%s: %d cell ranges; G against float64 %.3e (bound %.1e); dsum / n\' %.3e absolute (bound %.1e)'
          % (tag, S, e, RTOL, ed, KEY_ATOL['p_d']))
    _note('gene rate', inst, 'G float64', e / RTOL, tag)
    _note('gene rate', inst, 'dsum', ed / KEY_ATOL['p_d'], tag)
    assert bool(torch.isfinite(G).all()) and bool(torch.isfinite(dsum).all()), 'an element of G or dsum was not written'
    assert torch.equal(G, G2) and torch.equal(dsum, dsum2), 'two runs differ'
    assert e <= RTOL
    assert ed <= KEY_ATOL['p_d']
    # the two column overrides (tests/test_zi_fold_in_fit_gpu.py): S partials nnz_r + 1e-10 (cells_r - nnz_r) added in order
    nnz = float((X[:, zc.PI_ZERO] != 0).sum())
    want = nnz + 1e-10 * (n - nnz)
    got0, got1 = float(dsum[zc.PI_ZERO]), float(dsum[zc.PI_ONE])
    print('  pi_d = 0 column: %.17g against %.17g; pi_d = 1 column: %.17g' % (got0, want, got1))
    assert abs(got0 - want) <= (S + 3) * EPS * want
    assert got1 == float(n)
    if storing:
        # D of oriana_dropout_sweep_fused_tiles (ORIANA_MATRIX_F32) and D^T U in float64: two results within 3e-7 of float64 each
        _, D = _storing(X, U, V, pi_d, zc.F32, scratch=_nan_scratch(K, mp), mp=mp)
        ref = torch.from_numpy(D[:, :m_real]).to(DEV).double().T @ _f64(U)
        e2 = err_colrel(G[:m_real].cpu().numpy(), ref.cpu().numpy())
        print('  G against the stored D_hat^T U %.3e (bound 6e-7)' % e2)
        _note('gene rate', inst, 'stored D_hat^T U', e2 / 6e-7, tag)
        assert e2 <= 6e-7
    return S


@pytest.mark.parametrize('K', zc.K_FORMS)
def test_gene_rate_loop_forms(K):
    S = _check_gene_rate(K, zc.N_BODY, zc.M_REAL, zc.M_ALIGNED, 'K=%d (%s)' % (K, _form(K)), storing=True)
    assert S > 1, 'the case does not cover more than one cell range'


@pytest.mark.parametrize('n,m', zc.GENE_RATE_EDGE_SHAPES)
def test_gene_rate_edge_shapes(n, m):
    _check_gene_rate(zc.GENE_EDGE_K, n, m, m, 'K=%d %d x %d' % (zc.GENE_EDGE_K, n, m), storing=True)


@pytest.mark.parametrize('K', zc.GENE_RATE_LONG_KS)
def test_gene_rate_long_batch_spills_and_goes_on(K):
    """32 ranges of 4160 cells: sixteen flushes, the spill to float64, two tiles more and the spill that adds to the partial; the
    last range (3168 cells) spills once.  36 genes: a partial second strip and two waves without a gene."""
    n = zc.LONG_N
    S = _ranges(n, K, zc.LONG_M)
    assert S == zc.GENE_RATE_RANGES, S
    ips = (-(-n // S) + 31) // 32 * 32
    assert ips > 4096 and 0 < n - (S - 1) * ips < 4096
    _check_gene_rate(K, n, zc.LONG_M, zc.LONG_M, 'K=%d long batch' % K, storing=False)


def test_gene_rate_mid_batch_passes_the_flush_only():
    n = zc.MID_N
    S = _ranges(n, zc.MID_K, zc.MID_M)
    assert S == zc.GENE_RATE_RANGES and 256 < (-(-n // S) + 31) // 32 * 32 == 288 < 4096
    _check_gene_rate(zc.MID_K, n, zc.MID_M, zc.MID_M, 'K=%d mid batch' % zc.MID_K, storing=False)


# ---- 3. oriana_zi_cell_bound: k_dropout_sweep<NT, false, true> in every loop form ------------------------------------------------

def _check_bound(K, n, m_real, mp, tag):
    X, U, V, pi_d = zc.inputs(K, n, m_real)
    assert pi_d[zc.PI_ZERO] == 0 and pi_d[zc.PI_ONE] == 1 and (n < 200 or (X[:, zc.PI_ZERO] != 0).any())
    ref, Lam, lg, g = zs.dropout_sums(X, V, pi_d, U)
    bound = zs.dropout_bound(K, Lam, lg, g)
    got = _entry(X, U, V, pi_d, mp=mp, m_real=m_real)
    S = _splits(n, K, mp)[1]
    d = np.abs(got - ref)
    i = int(np.argmax(d / bound))
    print('%s (%d gene ranges): worst cell %d HIP %.17g ref %.17g diff %.3e bound %.3e; max error / bound %.3f' % (
        tag, S, i, got[i], ref[i], d[i], bound[i], np.max(d / bound)))
    _note('cell bound', 'k_dropout_sweep<%d> bound' % _nt(K), 'float64', np.max(d / bound), tag)
    assert np.isfinite(got).all(), 'NaN sentinel left in out, or a non-finite value'
    assert np.all(d <= bound)
    # a second run, over scratch and out filled with another sentinel: bit-identical
    assert np.array_equal(_entry(X, U, V, pi_d, fill=float('inf'), mp=mp, m_real=m_real), got)
    return S


@pytest.mark.parametrize('K', zc.K_FORMS)
def test_cell_bound_loop_forms(K):
    """The body shape with one inert gene (m_real = m - 1)."""
    S = _check_bound(K, zc.N_BODY, zc.M_REAL, zc.M_ALIGNED, 'K=%d (%s)' % (K, _form(K)))
    assert S > 1, 'one gene range: the ordered combine is not exercised'


@pytest.mark.parametrize('n,m', zc.EDGE_SHAPES)
def test_cell_bound_edge_shapes(n, m):
    _check_bound(zc.GENE_EDGE_K, n, m, m, 'K=%d %d x %d' % (zc.GENE_EDGE_K, n, m))
