# -*- coding: utf-8 -*-
"""The float64 reference of the Gamma update and the M-step (tests/gamma_update_reference.py) checked on its own: how
far SciPy's digamma is from a 50-digit evaluation, that the dyadic inputs make the finalize step exact, that the bound
on E[log .] separates a faithful float32 evaluation from seven wrong ones, that the case table reaches every
instantiation of the launch switches, and that mstep_ref is the oracle's M-step.  No GPU."""
import os
import types

import numpy as np
import pytest

import gamma_update_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scipy_reference_against_mpmath_on_the_value_ladder():
    """E[log .] = digamma(f32 a1) - log(f32 a2) from SciPy against mpmath at 50 digits on A1_LADDER x A2_LADDER.  The
    difference is judged element by element against an eighth of that element's bound: a float64 cannot hold
    psi(1e-15) = -1e15 closer than 0.06, which no element near the zero of psi (bound 1.2e-7) could be asked to share.
    Measured: largest difference / bound 1.4e-9, largest difference 0.070 absolute (at a1 = 1e-15)."""
    import mpmath
    mpmath.mp.dps = 50
    a1, a2 = np.meshgrid(np.array(gr.A1_LADDER), np.array(gr.A2_LADDER), indexing='ij')
    ref = gr.gamma_update_ref(a1=a1, a2=a2)
    worst, worst_abs = 0.0, 0.0
    for i in range(a1.shape[0]):
        for j in range(a1.shape[1]):
            x = mpmath.mpf(float(np.float32(a1[i, j])))
            y = mpmath.mpf(float(np.float32(a2[i, j])))
            exact = mpmath.digamma(x) - mpmath.log(y)
            d = float(abs(mpmath.mpf(float(ref['Elog_ref'][i, j])) - exact))
            b = float(gr.elog_bound(ref['psi'][i, j], ref['lg'][i, j], ref['Elog_ref'][i, j]))
            worst, worst_abs = max(worst, d / b), max(worst_abs, d)
    print('scipy against mpmath: largest difference / bound %.3e, largest difference %.3e' % (worst, worst_abs))
    assert worst < 0.125


FIN_CASES = [c for c in gr.CASES if c[0] == 'fin']


@pytest.mark.parametrize('case', FIN_CASES, ids=gr.case_id)
def test_dyadic_inputs_make_the_finalize_step_exact(case):
    """Z[o] + F[p] * sum_s R_s[p] evaluated in float32 (a product, then a sum: two roundings) and in float64 (rounded
    once at the end) are the same bits: the step is exact, so a fused multiply-add and any order of it are too."""
    _, (nslab, row0), r, K, _, _ = case
    d, Kp = gr.case_inputs(case)
    z32 = gr.finalize_ref(d['Z'], d['F'], d['R'], K, nslab, row0, d['row_index'], dtype=np.float32)
    z64 = gr.finalize_ref(d['Z'], d['F'], d['R'], K, nslab, row0, d['row_index'], dtype=np.float64)
    assert z32.dtype == np.float32 and np.array_equal(z32, z64)
    assert d['R'].shape == (gr.slab_rows(r, nslab, row0), Kp) and (r * K < 64 or (z64 != d['Z']).any())
    # 24 bits are never needed: the value is a multiple of 2^-8 below 2^9
    z = z64.astype(np.float64) * 256
    assert np.array_equal(z, np.round(z)) and float(z64.max()) < 512


def _f32_evaluation(ref, extra_log_ulp=0):
    """A faithful float32 evaluation of E[log .]: psi and the logarithm rounded to float32 (the logarithm moved by further
    ulps on request), subtracted in float32."""
    with np.errstate(all='ignore'):
        psi = ref['psi'].astype(np.float32)
        lg = ref['lg'].astype(np.float32)
        for _ in range(extra_log_ulp):
            lg = np.nextafter(lg, np.float32(np.inf))
        return psi - lg


@pytest.mark.parametrize('case', [c for c in gr.CASES if c[2] * c[3] <= 60000], ids=gr.case_id)
def test_a_faithful_float32_evaluation_keeps_the_bound(case):
    d, _ = gr.case_inputs(case)
    ref = gr.gamma_update_ref(**d)
    assert float(gr.elog_ratio(_f32_evaluation(ref), ref).max()) < 1.0
    assert float(gr.elog_ratio(_f32_evaluation(ref, extra_log_ulp=1), ref).max()) < 1.0


def _violates(wrong, right):
    with np.errstate(all='ignore'):
        return bool((gr.elog_ratio(wrong['Elog_ref'].astype(np.float32), right) > 1.0).any())


def test_the_bound_rejects_wrong_restatements():
    rng = np.random.default_rng(7)
    r, K, nslab, row0 = 515, 100, 3, 257
    Kp = gr.kpad(K)
    d = gr.dyadic_plain(rng, r, K)
    d.update(gr.dyadic_finalize(rng, r, K, Kp, nslab, row0, extra_rows=(nslab - 1) * row0), nslab=nslab, slab_row0=row0)
    right = gr.gamma_update_ref(**d)
    assert not _violates(right, right)
    # column k + 1 in place of k
    shifted = dict(right, Elog_ref=np.roll(right['Elog_ref'], -1, axis=1))
    assert _violates(shifted, right)
    # the last slab dropped
    assert _violates(gr.gamma_update_ref(**dict(d, nslab=nslab - 1)), right)
    # slab_row0 ignored: every slab read as r whole rows
    assert _violates(gr.gamma_update_ref(**dict(d, slab_row0=0)), right)
    # rate_vec not added
    assert _violates(gr.gamma_update_ref(**dict(d, rate_vec=np.zeros(K))), right)
    # row_index applied to the packed operands: Z[o] += F[o] * R[o]
    assert _violates(gr.gamma_update_ref(**dict(d, row_index=None)), right)
    # rmul dropped
    case = ('plain', 'zi_all', 515, 50, True, True)
    assert case in gr.CASES
    z, _ = gr.case_inputs(case)
    assert _violates(gr.gamma_update_ref(**dict(z, rmul=None)), gr.gamma_update_ref(**z))
    # the clamp omitted, on the specials case
    case = ('plain', 'specials', 37, 5, True, False)
    assert case in gr.CASES
    s, _ = gr.case_inputs(case)
    right = gr.gamma_update_ref(**s)
    with np.errstate(all='ignore'):
        a1 = s['prior1'][None, :] + s['Z'].astype(np.float64)
        a2 = np.broadcast_to(s['prior2'] + s['rate_vec'], a1.shape)
    assert _violates(gr.gamma_update_ref(a1=a1, a2=a2), right)
    # ... and what the specials case holds: both clamps, the infinite shape, inf - inf
    assert right['a1'][0, 0] == 1e-15 and right['a1'][2, 2] == 1e-15 and right['a1'][4, 0] == 1e-15
    assert right['a1'][1, 1] == gr.DBL_MAX and right['Elog_ref'][1, 1] == np.inf
    assert right['a2'][0, 4] == gr.DBL_MAX and right['Elog_ref'][0, 4] == -np.inf and np.isnan(right['Elog_ref'][5, 4])
    assert np.isfinite(right['Elog_ref'][3, 3]) and right['a1'][3, 3] > 2e38


# Every instantiation the launch switches of csrc/updates.hip list: gu_scalar_launch (k_gamma_update<FIN, NT>: 256 threads,
# or 512 (plain) / 1024 (FIN) for 4096 < r <= 32768) and gu_vec_launch / gu_vec_launch_lpr over the (VEC, LPR) of gu_vec_cfg
# (k_gamma_update_vec<FIN, VEC, LPR>).
INSTANTIATIONS = [
    ('scalar', False, 256), ('scalar', False, 512), ('scalar', True, 256), ('scalar', True, 1024),
    ('vec', False, 4, 8), ('vec', False, 4, 16), ('vec', False, 4, 32), ('vec', False, 4, 64),
    ('vec', False, 2, 8), ('vec', False, 2, 16), ('vec', False, 2, 32), ('vec', False, 2, 64),
    ('vec', False, 1, 8), ('vec', False, 1, 16), ('vec', False, 1, 32), ('vec', False, 1, 64),
    ('vec', True, 4, 8), ('vec', True, 4, 16), ('vec', True, 4, 32), ('vec', True, 4, 64),
    ('vec', True, 2, 8), ('vec', True, 2, 16), ('vec', True, 2, 32), ('vec', True, 2, 64),
    ('vec', True, 1, 8), ('vec', True, 1, 16), ('vec', True, 1, 32), ('vec', True, 1, 64),
]


def _template(inst):
    return inst[:3] if inst[0] == 'scalar' else inst


def test_the_cases_reach_every_instantiation():
    reached = {}
    for case in gr.CASES:
        entry, form, r, K, aligned, prep = case
        inst = gr.instantiation(entry, r, K, aligned, prep)
        assert inst is not None, case                       # (no case is one the entry refuses)
        assert r * K <= 1.1 * (1 << 20), case
        reached.setdefault(inst, []).append(case)
    assert {_template(i) for i in reached} == set(INSTANTIATIONS) and len(set(INSTANTIATIONS)) == 28
    # every instantiation in the plain form; every FIN one with nslab in {1, 3} and slab_row0 in {0, r // 2}
    forms = {}
    for inst, cases in reached.items():
        forms.setdefault(_template(inst), set()).update(
            c[1] if isinstance(c[1], str) else (c[1][0], 'half' if c[1][1] else 0) for c in cases)
    for inst in INSTANTIATIONS:
        if inst[1]:
            assert {(1, 0), (3, 0), (1, 'half'), (3, 'half')} <= forms[inst], inst
        else:
            assert 'plain' in forms[inst], inst
    # the element-per-lane kernel: every block width, one to four column rounds, the in-wave and the two-wave reduction
    scalar = [i for i in reached if i[0] == 'scalar']
    assert {i[3] for i in scalar if i[2] == 256 and not i[1]} == {1, 4, 8, 32, 64, 128}
    assert {i[4] for i in scalar if i[2] == 256 and not i[1]} == {1, 2, 3, 4}
    for fin, nt in ((False, 512), (True, 1024)):
        assert {(i[3], i[4]) for i in scalar if i[1] == fin and i[2] == nt} >= {(4, 1), (32, 1), (128, 1), (128, 2)}
    # the ZI operands and the stored pair: the element-per-lane kernel in both group sizes and every VEC
    for form in ('zi_zr', 'zi_rr', 'zi_all', 'stored'):
        got = {_template(gr.instantiation(*((c[0],) + c[2:]))) for c in gr.CASES if c[1] == form}
        assert {('scalar', False, 256), ('scalar', False, 512)} <= got and {i[2] for i in got if i[0] == 'vec'} == {4, 2, 1}
    # the unaligned cases: VEC 1 at a K whose aligned configuration is VEC 4, and the element-per-lane kernel at K = 100
    assert gr.instantiation('plain', 16384, 64, True) == ('vec', False, 4, 16)
    assert gr.instantiation('plain', 16384, 64, False) == ('vec', False, 1, 64)
    assert gr.instantiation('fin', 10486, 100, False) == ('scalar', True, 1024, 128, 1)
    # the table of the issue: K -> LPR
    for vec, lprs in ((4, [8, 8, 16, 16, 32, 32, 64]), (2, [8, 8, 16, 16, 32, 32, 64, 64]), (1, [8, 8, 16, 16, 32, 32, 64, 64])):
        assert [gr.vec_cfg(K, True) for K in gr.VEC_K[vec]] == [(vec, l) for l in lprs]
        assert all(gr.kpad(K) for K in gr.VEC_K[vec])
    assert len(set(gr.CASES)) == len(gr.CASES)


def test_the_lazy_entry_rule():
    assert not gr.lazy_runs(5000, 20) and gr.lazy_runs(515, 20, prep=True) and gr.lazy_runs(8192, 128)
    assert not gr.lazy_runs(10486, 101) and not gr.lazy_runs(10486, 100, aligned=False) and gr.lazy_runs(16384, 64, aligned=False)
    assert not gr.lazy_runs(70, 257, prep=True)
    # ORIANA_EKRANGE for each of its reasons is among the cases, and so is a lazy launch of every FIN vector instantiation
    fin = [c for c in gr.CASES if c[0] == 'fin']
    refused = {(c[2] * c[3] < 1 << 20 and not c[5], gr.vec_cfg(c[3], c[4]) is None) for c in fin if not gr.lazy_runs(*c[2:])}
    assert refused == {(True, False), (True, True), (False, True)}
    assert ('fin', (3, 4128), 8257, 127, True, False) in fin and ('fin', (3, 5243), 10486, 100, False, False) in fin
    assert {gr.instantiation(*((c[0],) + c[2:])) for c in fin if gr.lazy_runs(*c[2:])} == {i for i in INSTANTIATIONS if i[0] == 'vec' and i[1]}
    assert gr.prep_blocks(1000, 101) == 0 and gr.prep_blocks(1000, 300) == 0 and gr.prep_blocks(515, 100) == 17


@pytest.mark.parametrize('name', ['gap_odd_rand.npz', 'zigap_c1_nmf.npz'])
def test_mstep_ref_is_the_oracles_mstep(name):
    """_OracleModel.update_prior_hyper_parameters on a golden state (the priors of sweep 1, the expectations of sweep 2)
    against mstep_ref from the column sums.  With the float32 mean of the oracle handed over as the sum, the shapes are
    the same bits and the rates differ by the summation of U_hat alone (np.mean against fsum: n 2^-53).  With the honest
    float64 sum of the float32 logs, the mean differs from np.mean's float32 accumulation by at most (n - 1) 2^-24
    mean|x| + 2^-24 |mean| =: dy, which moves inverse_digamma(y) by dy / trigamma(n1) to first order."""
    import scipy.special
    from oracle.cavi_oracle import _OracleModel
    g = np.load(os.path.join(ROOT, 'tests', 'golden', name))
    for side, p1k, p2k, ek, lk in (('u', 'alpha1', 'alpha2', 'U_hat', 'log_U_hat'), ('v', 'beta1', 'beta2', 'V_hat', 'log_V_hat')):
        E, L = g['s2/' + ek], g['s2/' + lk]
        assert L.dtype == np.float32
        n = E.shape[0]
        ns = types.SimpleNamespace(zi=False, sparse=False, alpha2=g['s1/alpha2'].copy(), beta2=g['s1/beta2'].copy(),
                                   U_hat=g['s2/U_hat'], V_hat=g['s2/V_hat'], log_U_hat=g['s2/log_U_hat'], log_V_hat=g['s2/log_V_hat'])
        _OracleModel.update_prior_hyper_parameters(ns)
        want1, want2 = getattr(ns, p1k), getattr(ns, p2k)
        p2 = g['s1/' + p2k]
        sumE = gr.colsum_ref(E)
        mean32 = np.mean(L, axis=0)
        assert mean32.dtype == np.float32
        n1, n2 = gr.mstep_ref(g['s1/' + p1k], p2, sumE, mean32.astype(np.float64) * n, float(n))
        assert np.array_equal(n1, want1), side
        np.testing.assert_allclose(n2, want2, rtol=2 * n * gr.U64, atol=0)
        sumL = gr.colsum_ref(L.astype(np.float64))
        h1, h2 = gr.mstep_ref(g['s1/' + p1k], p2, sumE, sumL, float(n))
        dy = (n - 1) * gr.U32 * np.mean(np.abs(L.astype(np.float64)), axis=0) + gr.U32 * np.abs(sumL / n)
        tol = 1.05 * dy / scipy.special.polygamma(1, want1)
        assert (np.abs(h1 - want1) <= tol).all(), (side, float((np.abs(h1 - want1) / tol).max()))
        assert (np.abs(h2 - want2) <= 1.05 * tol / (sumE / n) + 2 * n * gr.U64 * want2).all()
        # the goldens are the reference's own states
        np.testing.assert_allclose(want1, g['s2/' + p1k], rtol=1e-12)


def test_mstep_ref_edges():
    """A column of clamped shapes: every E[log .] is f32(psi(1e-15)), and the float32 nearest to -1e15 is
    -999999986991104, ABOVE -1e15 -- the new shape is 1.000000013e-15 and does not clamp.  A mean of -2e15 does (the
    shape would be 5e-16).  A column without mass: the rate is DBL_MAX."""
    n1, n2 = gr.mstep_ref(np.ones(4), np.array([1e-3, 1e-3, 1.0, 2.0]), np.array([5.0, 5.0, 0.0, 4.0]),
                          np.array([-1e21, -2e21, -3e6, 1e6]), 1e6)
    assert 1e-15 < n1[0] < 1.0000001e-15 and n1[1] == 1e-15 and n2[2] == gr.DBL_MAX and np.isfinite(n1).all() and n1[3] > 1.0
