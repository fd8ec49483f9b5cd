# -*- coding: utf-8 -*-
"""CPU-only checks of tests/logsum_reference.py: the restatements the GPU tests of tests/test_sparse_side_gpu.py rely on,
and the yardstick of their bound on Z_log."""
import numpy as np
import pytest

import logsum_reference as lr
from helpers import (golden_files, load_golden, state_of, err_colrel, ZLOG_FACTOR, ZLOG_FLOOR, ZLOG_REF_MAX,
                     ZLOG_REF_MAX_SLOW, zlog_bound)

CASES = [(f, s) for f in lr.DRIFT_FORMS for s in lr.DRIFT_SHIFTS]


@pytest.mark.parametrize('form,shift', CASES, ids=['%s-%s' % c for c in CASES])
def test_reference_float32_nest_is_a_sharp_yardstick(form, shift):
    """The bound on the HIP outputs is a multiple of the reference's own distance from the float64 value, so that distance
    must stay small on every case.  The case with one cell at lu - 80 gets the wider ZLOG_REF_MAX_SLOW: the reference rounds
    lu + lv ~ -75 to float32 before the exponential, helpers.py has the arithmetic."""
    c = lr.drift_case(form, shift)
    lim = ZLOG_REF_MAX_SLOW if c['slow'] else ZLOG_REF_MAX
    for name, ref, exact in zip(('Z_i', 'Z_j', 'Z_log'), c['ref'], c['exact']):
        assert np.isfinite(exact).all()
        assert err_colrel(ref, exact) < lim, name


@pytest.mark.parametrize('form', [f for f, (K, nest) in lr.DRIFT_FORMS.items() if nest in ('sparse', 'sparse-hybrid')])
def test_uncentred_log_sums_exceed_the_bound_under_drift(form):
    """The teeth of ZLOG_FACTOR: two plain float32 sums (no centre) are outside the bound at (-40, 38); the centred
    evaluation of the same sums is inside it; without drift both are."""
    c = lr.drift_case(form, 'u-40')
    bound = zlog_bound(err_colrel(c['ref'][2], c['exact'][2]))
    plain = err_colrel(lr.logsum_f32(c['lu'], c['lv'], c['X'], c['St'], center=False), c['exact'][2])
    centred = err_colrel(lr.logsum_f32(c['lu'], c['lv'], c['X'], c['St'], center=True), c['exact'][2])
    print('%s: un-centred %.3e, centred %.3e, bound %.3e' % (form, plain, centred, bound))
    assert plain > bound
    assert centred <= bound
    c0 = lr.drift_case(form, 'centred')
    b0 = zlog_bound(err_colrel(c0['ref'][2], c0['exact'][2]))
    for center in (False, True):
        assert err_colrel(lr.logsum_f32(c0['lu'], c0['lv'], c0['X'], c0['St'], center=center), c0['exact'][2]) <= b0


def test_zlog_constants_are_ordered():
    assert 0 < ZLOG_FLOOR < ZLOG_REF_MAX < ZLOG_REF_MAX_SLOW and ZLOG_FACTOR > 1
    assert zlog_bound(0.0) == ZLOG_FLOOR and zlog_bound(1.0) == ZLOG_FACTOR


def test_sparsity_restatement_matches_the_oracle_step():
    """logsum_reference.sparsity_update against the S update inside cavi_oracle's sweep, from a golden state after its
    first sweep (pi_s interior).  The oracle keeps tmp in float64, the reference statement adds into a float32 array: the two
    differ by at most the float32 rounding of tmp, half an ulp of |tmp|, times the sigmoid's largest slope 1 / 4."""
    from oracle import cavi_oracle as co
    g = load_golden(golden_files('sparsegap_odd_rand.npz')[0])
    M = co.MODELS['SparseGaP'](g['X'], int(g['meta/k']), g['s0/a1'], g['s0/b1'], tau=float(g['meta/tau']))
    M.load_state(state_of(g, 's1'))
    pi_s = M.pi_s.copy()
    assert ((pi_s > 0) & (pi_s < 1)).any()
    M.update_variational_parameters()
    Zlog = M.last_Z[2]
    c = M.U_hat.sum(axis=0)
    p_s, S_hat = lr.sparsity_update(pi_s, Zlog, c, M.V_hat)
    tmp = np.abs(-Zlog.astype(np.float64) + np.nan_to_num(c * M.V_hat))
    tol = 0.25 * np.spacing(tmp.astype(np.float32)).astype(np.float64) / 2 + 1e-15
    assert (np.abs(p_s - M.p_s) <= tol).all()
    assert np.array_equal(S_hat, p_s.astype(np.float32))
    # and against the reference's own next state, as closely as the oracle is held to it
    assert err_colrel(p_s, g['s2/p_s']) < 1.2e-5
    # the c_mat form: the same numbers as a matrix
    p2, _ = lr.sparsity_update(pi_s, Zlog, np.broadcast_to(c, Zlog.shape), M.V_hat)
    assert np.array_equal(p2, p_s)


def test_side_restatements_on_known_answers():
    f32 = np.float32
    # log_center: weights, rejected entries, a factor nobody counts for, the row permutation
    F = np.array([[1, 1, 0], [1, 1e-30, 0], [1, 1, 0]], f32)
    F = np.concatenate([F, np.full((3, 13), np.nan, f32)], axis=1)
    lf = np.array([[1, 2, 3], [3, 4, 5], [np.inf, 1e30, 7]], f32)
    acc = lr.log_center(F, lf, None, None, 3)
    assert acc.tolist() == [4.0, 2.0, 0.0, 2.0, 1.0, 0.0]
    assert lr.centre_of(acc, 3).tolist() == [2.0, 2.0, 0.0]
    W = np.array([[2, 0, 1], [np.nan, 1, 1], [1, 1, 1]], f32)
    assert lr.log_center(F, lf, W, None, 3).tolist() == [2.0, 0.0, 0.0, 2.0, 0.0, 0.0]
    perm = np.array([2, 0, 1], np.int32)                    # packed row p reads lf[perm[p]], W[perm[p]]
    assert lr.log_center(F, lf, None, perm, 3).tolist() == [4.0, 4.0, 0.0, 2.0, 1.0, 0.0]
    # scale_factor: zero_guard gives +0, without it the IEEE product
    Fin = np.array([[0, 2, 0] + [np.nan] * 13], f32)
    mul = np.array([[-1e15, 3, np.inf]], f32)
    g = lr.scale_factor(Fin, mul, None, 3, 1)
    assert g[0, :3].tolist() == [0.0, 6.0, 0.0] and not np.signbit(g[0, 0]) and not g[0, 3:].any()
    u = lr.scale_factor(Fin, mul, None, 3, 0)
    assert u[0, 0] == 0 and np.signbit(u[0, 0]) and np.isnan(u[0, 2])
    s = lr.scale_factor_centered(Fin, mul, np.array([8, 8, 0, 2, 4, 0], np.float64), None, 3)
    assert s[0, :3].tolist() == [0.0, 2.0, 0.0]
    # finalize_zlog adds into Zlog, in the caller's row
    Z = lr.finalize_zlog(np.array([[1, 1, 1], [5, 5, 5]], f32), np.array([[1, 0, 2] + [0] * 13], f32).repeat(2, 0),
                         np.array([[1, np.nan, 1] + [0] * 13], f32).repeat(2, 0), np.array([[2, np.inf, 2] + [0] * 13], f32).repeat(2, 0),
                         np.array([[1, 1, 1], [0, np.nan, 0]], f32), np.array([3, 3, 3, 1, 1, 1], np.float64), np.array([1, 0], np.int32), 3)
    assert Z.tolist() == [[10.0, 1.0, 19.0], [12.0, 5.0, 19.0]]
    assert lr.threshold(np.array([0.5, np.nextafter(0.5, 1), np.nan]), 0.5).tolist() == [0.0, 1.0, 0.0]
    assert lr.rowmean(np.array([[1.0, 2.0, 6.0]])).tolist() == [3.0]
    D = np.zeros((40, 2), f32); D[0, 0] = D[33, 0] = D[31, 1] = 1
    assert lr.nzmask_words(D).tolist() == [1, 1 << 31, 2, 0]
    p, Dh, cs = lr.dropout_update(np.zeros((2, 3)), np.array([0.5, 0.0, 1.0]), np.array([[0, 0, 0], [1, 0, 0]]))
    assert p.tolist() == [[0.5, 1e-10, 1 - 1e-10], [1 - 1e-10, 1e-10, 1 - 1e-10]] and abs(cs[0] - (1.5 - 1e-10)) < 1e-15
