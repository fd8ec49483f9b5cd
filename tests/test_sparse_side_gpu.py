# -*- coding: utf-8 -*-
"""The log sums Z_log under scale drift against the float64 loop nest, the element-wise kernels of csrc/dense.hip each against
its NumPy restatement (tests/logsum_reference.py) at its edges, and the second grid launch of the four entries that chunk
their grid in y.  GPU only."""
import json

import numpy as np
import pytest
import torch

import logsum_reference as lr
from helpers import err_colrel, zlog_bound

pytestmark = pytest.mark.gpu

EINVAL, EKRANGE = -1, -2                         # ORIANA_EINVAL, ORIANA_EKRANGE (include/oriana_hip.h)
F32, F64 = np.float32, np.float64


@pytest.fixture(scope='module')
def eng():
    from oriana_amd import engine
    assert torch.cuda.is_available()
    return engine


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def host(t):
    return t.cpu().numpy()


def call(name, *args):
    from oriana_amd import _lib
    return _lib.call(name, *args, _lib.stream_ptr())


def rc_of(name, *args):
    """The entry's own return code (no exception)."""
    from oriana_amd import _lib
    return int(getattr(_lib.load(), name)(*args, _lib.stream_ptr()))


def ptr(t):
    return None if t is None else t.data_ptr()


def kpad(K):
    from oriana_amd import _lib
    return int(_lib.load().oriana_kpad(int(K)))


def same_bits(got, exp):
    """Equal bit for bit; NaNs equal each other whatever their payload."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    nan = np.isnan(exp)
    if not np.array_equal(np.isnan(got), nan):
        return False
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.array_equal(got.view(u)[~nan], exp.view(u)[~nan])


# ---- 1. Z_log, Z_i, Z_j against zq_exact under drift --------------------------------------------------------------------
_hip_runs = {}


def _run_drift(eng, form, shift):
    """engine.zq on a drift case (once per case): outputs on the host, the workspace and the layout."""
    key = (form, shift)
    if key in _hip_runs:
        return _hip_runs[key]
    c = lr.drift_case(form, shift)
    n, m, K = lr.DRIFT_N, lr.DRIFT_M, c['K']
    w_nz = None
    if c['nest'] == 'sparse-zi':
        ct = eng.CountTiles.from_dense(dev(c['X']), 'cuda', side=dev(c['D']))
        w_nz = ct.side_nz
    elif c['nest'] == 'sparse-hybrid':
        ct = eng.CountTiles.from_dense(np.array(c['X']), 'cuda', dense_density=0.3)
    else:
        ct = eng.CountTiles.from_dense(np.array(c['X']), 'cuda')
    ws = eng.ZWorkspace(ct, K)
    o = [torch.empty(n, K, device='cuda'), torch.empty(m, K, device='cuda'), torch.empty(m, K, device='cuda')]
    a = dict(lu=dev(c['lu']), lv=dev(c['lv']), St=dev(c['St']), Sh=dev(c['Sh']), dq=dev(c['dq']))
    eng.zq(ws, o[0], o[1], o[2], a['lu'], a['lv'], S_tilde=a['St'], S_hat=a['Sh'], dq=a['dq'], w_nz=w_nz)
    torch.cuda.synchronize()
    _hip_runs[key] = dict(out=[host(t) for t in o], ws=ws, ct=ct, dev=a, Zlog=o[2])
    return _hip_runs[key]


DRIFT = [(f, s) for f in lr.DRIFT_FORMS for s in lr.DRIFT_SHIFTS]


@pytest.mark.parametrize('form,shift', DRIFT, ids=['%s-%s' % c for c in DRIFT])
def test_log_sums_under_scale_drift(eng, form, shift):
    """Z_i, Z_j and Z_log of every form that produces Z_log, with E[log U] / E[log V] drifted along the scale indeterminacy,
    against the float64 loop nest: no further from it than helpers.zlog_bound allows, a multiple of the reference's own
    float32 distance measured on the same inputs.  Two plain float32 sums instead of the centred ones are outside this bound
    at (-40, 38) (test_logsum_host.py)."""
    c = lr.drift_case(form, shift)
    h = _run_drift(eng, form, shift)
    ws, ct, K = h['ws'], h['ct'], c['K']
    # the form the case is meant to run
    nflag = int(ws.tile_flag.sum().item())
    assert (nflag > 0) == c['slow'], nflag               # only the cell at lu - 80 leaves the shifted form
    if c['nest'] == 'sparse-hybrid':
        assert ct.gd >= 32 and lr.DEAD_GENE in host(ct.col_perm)[:ct.gd]
    else:
        assert ct.gd == 0
    if c['nest'] != 'zi-quirk':
        assert (ws.s_rs is None) == (K <= 64)            # two factor images in LDS: the fused row pass keeps no row-side s
    assert (ws.sw_cs is not None) == (c['nest'] == 'sparse-zi')
    fig = dict(form=form, shift=shift)
    fails = []
    for name, got, ref, exact in zip(('Z_i', 'Z_j', 'Z_log'), h['out'], c['ref'], c['exact']):
        d_hip, d_ref = err_colrel(got, exact), err_colrel(ref, exact)
        fig[name] = dict(hip=d_hip, ref=d_ref)
        if not d_hip <= zlog_bound(d_ref):
            fails.append('%s: HIP is %.3e from exact, the reference arithmetic %.3e' % (name, d_hip, d_ref))
    print('ZLOG_DRIFT ' + json.dumps(fig))
    assert not fails, fails
    if c['St'] is not None:                               # the dead gene contributes exact zeros to all three
        assert not h['out'][1][lr.DEAD_GENE].any() and not h['out'][2][lr.DEAD_GENE].any()


def test_log_centre_is_applied_consistently(eng):
    """The a_k subtracted in the E[log U]-weighted factor is the a_k added back in oriana_finalize_zlog: the (-40, 38) case
    again with the centre forced to 0 in both places (acc = NULL), rebuilt by hand through the ABI entries on the workspace
    of the normal run.  The two evaluations are the same sum, so they agree to the float32 rounding of the un-centred run's
    two large terms T1 = sum_i r lu and T2 = lv Z_j, each summed in float32 over the gene's nnz_j entries: the classic bound
    nnz_j 2^-24 sum|terms| per running sum (+ 4 roundings for the products and the output); and the un-centred one is the
    farther from the float64 value.  A centre with the wrong sign or the neighbouring factor's misses the first by a_k Z_j
    or (a_k - a_k') Z_j, three orders above this tolerance."""
    form, shift = 'fused-K20', 'u-40'
    c = lr.drift_case(form, shift)
    h = _run_drift(eng, form, shift)
    ws, ct, K = h['ws'], h['ct'], c['K']
    n, m = lr.DRIFT_N, lr.DRIFT_M
    assert int(ws.tile_flag.sum().item()) == 0            # the slow path added nothing to Z_log
    GL = torch.full_like(ws.FU, float('nan'))
    call('oriana_scale_factor_centered', ptr(GL), ptr(ws.FU), ptr(h['dev']['lu']), None, ptr(ct.row_perm), n, K)
    C2 = torch.zeros_like(ws.C)
    eng.col_pass(ct, ws.s_cs, GL, C2, K, what='log')
    Zu = torch.zeros(m, K, device='cuda')
    call('oriana_finalize_zlog', ptr(Zu), ptr(ws.FV), ptr(C2), ptr(ws.C), ptr(h['dev']['lv']), None, ptr(ct.col_perm), m, K)
    Zu, Zc = host(Zu).astype(F64), h['out'][2].astype(F64)
    _, Zj, Zl = c['exact']
    T2 = c['lv'].astype(F64) * Zj
    T1 = Zl - T2
    nnz = (c['X'] != 0).sum(0)[:, None]
    tol = (nnz + 4) * 2.0 ** -24 * (np.abs(T1) + np.abs(T2) + np.abs(Zl))
    assert np.abs(T1).max() > 5 * np.abs(Zl).max()        # the drift is there: |lu| = 40 against |lu + lv| = 2 + a few sigma
    worst = float((np.abs(Zu - Zc) / np.maximum(tol, 1e-300)).max())
    d_u, d_c = err_colrel(Zu, Zl), err_colrel(Zc, Zl)
    print('ZLOG_CENTRE ' + json.dumps(dict(uncentred=d_u, centred=d_c, worst_over_tol=worst)))
    assert (np.abs(Zu - Zc) <= tol).all(), worst
    assert d_u > d_c


# ---- 2. the side kernels, each against its restatement ------------------------------------------------------------------
def _specials(rng, a, values, per=3):
    """Scatter each special value over `per` random places of `a` (in place); returns a."""
    flat = a.reshape(-1)
    for v in values:
        flat[rng.integers(0, flat.size, size=per)] = v
    return a


def _log_center_inputs(rng, r, K):
    Kp = kpad(K)
    F = np.full((r, Kp), np.nan, F32)                     # (the pad columns are never read)
    F[:, :K] = _specials(rng, rng.random((r, K)).astype(F32) + F32(0.01),
                         [0.0, F32(1e-20), np.nextafter(F32(1e-20), F32(1)), F32(1e-30)])
    lf = _specials(rng, (rng.normal(size=(r, K)) * 1.5 - 40).astype(F32), [F32(1e30), -F32(1e30), np.inf, -np.inf, np.nan])
    W = _specials(rng, (rng.random((r, K)) * 50).astype(F32), [0.0, -1.0, np.inf, np.nan])
    if K >= 2:
        F[:, K // 2] = 0.0                                # a factor that no row counts for
    return F, lf, W


@pytest.mark.parametrize('r', [1, 255, 256, 257, 700])
@pytest.mark.parametrize('K', [1, 20, 64, 65, 128, 129, 256])
def test_log_center(K, r):
    rng = np.random.default_rng(1000 * K + r)
    F, lf, W = _log_center_inputs(rng, r, K)
    perm = rng.permutation(r).astype(np.int32)
    dF, dl, dW, dp = dev(F), dev(lf), dev(W), dev(perm)
    for with_w in (False, True):
        for with_perm in (False, True):
            acc = torch.full((2 * K,), float('nan'), dtype=torch.float64, device='cuda')     # garbage: the entry zero-fills
            call('oriana_log_center', ptr(acc), ptr(dF), ptr(dl), ptr(dW) if with_w else None, ptr(dp) if with_perm else None, r, K)
            exp = lr.log_center(F, lf, W if with_w else None, perm if with_perm else None, K)
            got = host(acc)
            what = 'K=%d r=%d W=%s perm=%s' % (K, r, with_w, with_perm)
            # float64 atomics arrive in any order: 1e-13 of the sum of magnitudes (every counted log is negative here)
            assert np.isfinite(got).all(), what
            assert (np.abs(got - exp) <= 1e-13 * np.abs(exp)).all(), what
            assert ((exp[K:] == 0) == (got[K:] == 0)).all(), what
            if K >= 2:
                assert got[K // 2] == 0 and got[K + K // 2] == 0, what
            if r > 1:
                assert (got[K:] > 0).any(), what


def test_log_center_without_rows_still_clears():
    acc = torch.full((40,), 7.0, dtype=torch.float64, device='cuda')
    call('oriana_log_center', ptr(acc), None, None, None, None, 0, 20)
    assert not host(acc).any()


def _factor_inputs(rng, r, K):
    Kp = kpad(K)
    Fin = np.full((r, Kp), np.nan, F32)
    Fin[:, :K] = rng.random((r, K)).astype(F32) * (rng.random((r, K)) < 0.8)
    mul = (rng.normal(size=(r, K)) * 1.5 + 35).astype(F32)
    zeros = np.argwhere(Fin[:, :K] == 0)
    assert len(zeros) >= 6
    return Kp, Fin, mul, zeros


@pytest.mark.parametrize('K', [5, 20, 33, 100])
def test_scale_factor(K):
    rng = np.random.default_rng(K)
    r = 37
    Kp, Fin, mul, zeros = _factor_inputs(rng, r, K)
    assert Kp >= K and (Kp > K or K in (20, 100))
    perm = rng.permutation(r).astype(np.int32)
    for (i, k), v in zip(zeros, [-1e15, np.inf, np.nan, -1e15, np.inf, np.nan]):
        mul[i, k] = v                                      # where Fin == 0 in the caller's order ...
        mul[perm[i], k] = v                                # ... and through the permutation
    dF, dm, dp = dev(Fin), dev(mul), dev(perm)
    for guard in (1, 0):
        for p, pd_ in ((None, None), (perm, dp)):
            out = torch.full((r, Kp), float('nan'), device='cuda')
            call('oriana_scale_factor', ptr(out), ptr(dF), ptr(dm), ptr(pd_), r, K, guard)
            exp = lr.scale_factor(Fin, mul, p, K, guard)
            got = host(out)
            assert same_bits(got, exp), (K, guard, p is not None)
            assert not got[:, K:].any() and not np.signbit(got[:, K:]).any()
            if guard:
                assert not got[:, :K][Fin[:, :K] == 0].any() and not np.signbit(got[:, :K][Fin[:, :K] == 0]).any()
            else:
                assert np.isnan(got[:, :K][Fin[:, :K] == 0]).any() and np.signbit(got[:, :K][Fin[:, :K] == 0]).any()


@pytest.mark.parametrize('K', [5, 20, 33, 100])
def test_scale_factor_centered(K):
    rng = np.random.default_rng(100 + K)
    r = 37
    Kp, Fin, mul, zeros = _factor_inputs(rng, r, K)
    perm = rng.permutation(r).astype(np.int32)
    for (i, k), v in zip(zeros, [-1e15, np.inf, np.nan, -1e15, np.inf, np.nan]):
        mul[i, k] = v
        mul[perm[i], k] = v
    acc = np.concatenate([rng.normal(size=K) * 100 + 3000, rng.random(K) * 100 + 1])
    acc[K + K // 2] = 0.0                                 # nobody counted for this factor: its centre reads 0 ...
    acc[K // 2] = 123.0                                   # ... whatever the sum holds
    dF, dm, dp, da = dev(Fin), dev(mul), dev(perm), dev(acc)
    for a, ad in ((None, None), (acc, da)):
        for p, pd_ in ((None, None), (perm, dp)):
            out = torch.full((r, Kp), float('nan'), device='cuda')
            call('oriana_scale_factor_centered', ptr(out), ptr(dF), ptr(dm), ptr(ad), ptr(pd_), r, K)
            exp = lr.scale_factor_centered(Fin, mul, a, p, K)
            got = host(out)
            assert same_bits(got, exp), (K, a is not None, p is not None)
            assert not got[:, K:].any() and not got[:, :K][Fin[:, :K] == 0].any()
            assert not np.signbit(got[:, :K][Fin[:, :K] == 0]).any()
    # with acc = NULL it is oriana_scale_factor with zero_guard
    a, b = torch.empty(r, Kp, device='cuda'), torch.empty(r, Kp, device='cuda')
    call('oriana_scale_factor_centered', ptr(a), ptr(dF), ptr(dm), None, ptr(dp), r, K)
    call('oriana_scale_factor', ptr(b), ptr(dF), ptr(dm), ptr(dp), r, K, 1)
    assert same_bits(host(a), host(b))


@pytest.mark.parametrize('K', [5, 20, 33, 100])
def test_finalize_zlog(K):
    rng = np.random.default_rng(200 + K)
    r = 37
    Kp = kpad(K)
    FV = np.full((r, Kp), np.nan, F32)
    FV[:, :K] = rng.random((r, K)).astype(F32) * (rng.random((r, K)) < 0.8)
    C2 = (rng.normal(size=(r, Kp)) * 1e3).astype(F32)
    C = (rng.random((r, Kp)) * 30).astype(F32)
    lv = (rng.normal(size=(r, K)) * 1.5 + 38).astype(F32)
    perm = rng.permutation(r).astype(np.int32)
    zeros = np.argwhere(FV[:, :K] == 0)
    assert len(zeros) >= 6
    for (j, k), v in zip(zeros, [np.inf, np.nan, -np.inf, np.nan, np.inf, np.nan]):
        C2[j, k] = v; C[j, k] = v
        lv[j, k] = v; lv[perm[j], k] = v
    Z0 = (rng.normal(size=(r, K)) * 100 + 7).astype(F32)   # the entry ADDS: the slow path has written here before
    acc = np.concatenate([rng.normal(size=K) * 100 - 4000, rng.random(K) * 100 + 1])
    acc[K + K // 2] = 0.0
    dFV, dC2, dC, dlv, dp, da = dev(FV), dev(C2), dev(C), dev(lv), dev(perm), dev(acc)
    for a, ad in ((None, None), (acc, da)):
        for p, pd_ in ((None, None), (perm, dp)):
            Z = dev(Z0)
            call('oriana_finalize_zlog', ptr(Z), ptr(dFV), ptr(dC2), ptr(dC), ptr(dlv), ptr(ad), ptr(pd_), r, K)
            exp = lr.finalize_zlog(Z0, FV, C2, C, lv, a, p, K)
            got = host(Z)
            assert same_bits(got, exp), (K, a is not None, p is not None)
            o = np.arange(r) if p is None else p
            assert same_bits(got[o][FV[:, :K] == 0], Z0[o][FV[:, :K] == 0])       # FV == 0 adds an exact 0


@pytest.mark.parametrize('m,K,mat', [(37, 7, False), (37, 7, True), (13, 20, False), (300, 3, True)])
def test_sparsity_update(m, K, mat):
    """oriana_sparsity_update against sparse_gap.py:134-141 restated line by line (the float32 `tmp` included)."""
    assert (m * K) % 256 != 0
    rng = np.random.default_rng(m + K)
    pi = np.resize(np.array([0.3, 0.0, 1.0, 1e-10, 1 - 1e-10, 0.7, 0.5, 0.02]), m)
    Vp = rng.random((m, K)) * 40 + 0.5
    c = rng.random((m, K) if mat else K) * 60 + 1
    Zl = (c * Vp + rng.normal(size=(m, K)) * 8).astype(F32)            # t = c V' - Zlog = O(10) out of two terms of O(1e3)
    inner = (pi > 0) & (pi < 1)
    flat = rng.permutation(np.flatnonzero(np.repeat(inner, K)))[:16]        # (in rows that no override replaces)
    Vp.reshape(-1)[flat[0:2]] = np.inf                                 # c V' = inf -> nan_to_num -> the sigmoid saturates at 0
    Vp.reshape(-1)[flat[2:4]] = np.nan                                 # c V' = NaN -> 0
    Zl.reshape(-1)[flat[4:6]] = 1e4                                    # t << 0: saturates at 1
    Zl.reshape(-1)[flat[6:8]] = -1e4                                   # t >> 0: saturates at 0
    Zl.reshape(-1)[flat[8:10]] = np.nan                                # tmp NaN -> p NaN -> nan_to_num -> 0
    Zl.reshape(-1)[flat[10:12]] = np.inf
    p_s = torch.full((m, K), float('nan'), dtype=torch.float64, device='cuda')
    S_hat = torch.full((m, K), float('nan'), device='cuda')
    dc, dpi, dZ, dV = dev(c), dev(pi), dev(Zl), dev(Vp)
    call('oriana_sparsity_update', ptr(p_s), ptr(S_hat), ptr(dpi), ptr(dZ), None if mat else ptr(dc), ptr(dc) if mat else None,
         ptr(dV), m, K)
    exp, _ = lr.sparsity_update(pi, Zl, c, Vp)
    got = host(p_s)
    assert np.isfinite(got).all() and np.isfinite(exp).all()
    assert np.abs(got - exp).max() <= 1e-15
    assert same_bits(host(S_hat), got.astype(F32))
    assert (got[pi <= 0] == 1e-10).all() and (got[pi >= 1] == 1 - 1e-10).all()
    assert (got[inner] == 0).any() and (got[inner] == 1).any()        # both saturations were reached
    assert ((got[inner] > 0.01) & (got[inner] < 0.99)).sum() >= 10    # and the steep part of the sigmoid


def test_threshold():
    tau = 0.37
    rng = np.random.default_rng(5)
    p = rng.random(300)
    p[[0, 17, 255, 256, 299]] = [tau, np.nextafter(tau, 1), np.nextafter(tau, -1), np.nan, tau]
    out = torch.full((300,), float('nan'), device='cuda')
    dp = dev(p)
    call('oriana_threshold_f32', ptr(out), ptr(dp), tau, 300)
    got = host(out)
    assert same_bits(got, lr.threshold(p, tau))
    assert got[[0, 17, 255, 256, 299]].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize('K', [1, 7, 100])
def test_rowmean(K):
    rng = np.random.default_rng(K)
    A = rng.random((300, K)) * np.exp(rng.normal(size=(300, K)) * 5)
    out = torch.full((300,), float('nan'), dtype=torch.float64, device='cuda')
    dA = dev(A)
    call('oriana_rowmean_f64', ptr(out), ptr(dA), 300, K)
    assert same_bits(host(out), lr.rowmean(A))


@pytest.mark.parametrize('r,K', [(1, 1), (700, 20), (257, 130), (5000, 7)])
def test_colsum_f64(r, K):
    rng = np.random.default_rng(r + K)
    A = rng.random((r, K)) * 10
    mul = rng.random((r, K)).astype(F32)
    dA, dm = dev(A), dev(mul)
    for mv in (None, mul):
        out0 = rng.random(K)                               # the entry adds into out
        out = dev(out0)
        call('oriana_colsum_f64', ptr(out), ptr(dA), None if mv is None else ptr(dm), r, K)
        exp = out0 + lr.colsum(A, mv)
        assert (np.abs(host(out) - exp) <= 1e-13 * np.abs(exp)).all()


def test_mul_and_take_cols():
    rng = np.random.default_rng(9)
    A = rng.normal(size=777) * 1e3
    B = rng.random(777).astype(F32)
    out = torch.full((777,), float('nan'), dtype=torch.float64, device='cuda')
    dA, dB = dev(A), dev(B)
    call('oriana_mul_f64_f32', ptr(out), ptr(dA), ptr(dB), 777)
    assert same_bits(host(out), B.astype(F64) * A)
    D = rng.random((41, 13)).astype(F32)
    dD = dev(D)
    for K in (1, 5, 13):                                   # K = m is accepted
        o = torch.full((41, K), float('nan'), device='cuda')
        call('oriana_take_cols_f32', ptr(o), ptr(dD), 41, 13, K)
        assert same_bits(host(o), np.ascontiguousarray(D[:, :K]))
    o = torch.zeros(41, 14, device='cuda')
    assert rc_of('oriana_take_cols_f32', ptr(o), ptr(dD), 41, 13, 14) == EINVAL


def test_argument_answers():
    """What each entry answers to sizes and pointers it cannot serve, as its entry code and the header say: negative sizes and
    K <= 0 are ORIANA_EINVAL, a K that oriana_kpad has no width for ORIANA_EKRANGE, an empty matrix succeeds without touching a
    pointer, NULL with something to do is ORIANA_EINVAL."""
    b = torch.zeros(4096, dtype=torch.float64, device='cuda')
    p = b.data_ptr()
    assert kpad(256) == 256 and kpad(257) == 0
    tau = 0.5
    # (entry, arguments with every pointer valid and sizes 2 x 3 -- or length 6) -> 0
    good = {
        'oriana_log_center': (p, p, p, p, None, 2, 3),
        'oriana_scale_factor': (p, p, p, None, 2, 3, 1),
        'oriana_scale_factor_centered': (p, p, p, None, None, 2, 3),
        'oriana_finalize_zlog': (p, p, p, p, p, None, None, 2, 3),
        'oriana_sparsity_update': (p, p, p, p, p, None, p, 2, 3),
        'oriana_threshold_f32': (p, p, tau, 6),
        'oriana_rowmean_f64': (p, p, 2, 3),
        'oriana_colsum_f64': (p, p, None, 2, 3),
        'oriana_mul_f64_f32': (p, p, p, 6),
        'oriana_take_cols_f32': (p, p, 2, 3, 3),
        'oriana_colsum_wide_f64': (p, p, 2, 3),
        'oriana_colsum_wide_f32': (p, p, 2, 3),
        'oriana_nzmask_f32': (p, p, 2, 3),
        'oriana_dropout_update': (p, p, p, p, None, None, 2, 3),
    }
    for name, a in good.items():
        assert rc_of(name, *a) == 0, name
    torch.cuda.synchronize()

    def with_(a, i, v):
        a = list(a); a[i] = v
        return tuple(a)
    # the factor entries: (rows, K) are the last two sizes
    for name, ir, ik, required in (('oriana_log_center', 5, 6, (0, 1, 2)), ('oriana_scale_factor', 4, 5, (0, 1, 2)),
                                   ('oriana_scale_factor_centered', 5, 6, (0, 1, 2)), ('oriana_finalize_zlog', 7, 8, (0, 1, 2, 3, 4))):
        a = good[name]
        assert rc_of(name, *with_(a, ir, -1)) == EINVAL, name
        assert rc_of(name, *with_(a, ik, 0)) == EINVAL, name
        assert rc_of(name, *with_(a, ik, -5)) == EINVAL, name
        assert rc_of(name, *with_(a, ik, 257)) == EKRANGE, name
        assert rc_of(name, *with_(with_(a, ir, -1), ik, 257)) == EINVAL, name      # a bad size is reported before the range of K
        for i in required:
            assert rc_of(name, *with_(a, i, None)) == EINVAL, (name, i)
        if name != 'oriana_log_center':
            empty = tuple(None if i in required else v for i, v in enumerate(a))
            assert rc_of(name, *with_(empty, ir, 0)) == 0, name
    assert rc_of('oriana_log_center', None, None, None, None, None, 0, 3) == EINVAL          # acc is cleared even without rows
    # (rows, K) entries without a padded width
    for name, ir, ik, required in (('oriana_sparsity_update', 7, 8, (0, 1, 2, 3, 6)), ('oriana_rowmean_f64', 2, 3, (0, 1)),
                                   ('oriana_colsum_f64', 3, 4, (0, 1))):
        a = good[name]
        assert rc_of(name, *with_(a, ir, -1)) == EINVAL, name
        assert rc_of(name, *with_(a, ik, 0)) == EINVAL, name
        for i in required:
            assert rc_of(name, *with_(a, i, None)) == EINVAL, (name, i)
        empty = tuple(None if i in required else v for i, v in enumerate(a))
        assert rc_of(name, *with_(empty, ir, 0)) == 0, name
    assert rc_of('oriana_sparsity_update', p, p, p, p, None, None, p, 2, 3) == EINVAL       # neither c_vec nor c_mat
    assert rc_of('oriana_sparsity_update', p, p, p, p, None, p, p, 2, 3) == 0
    assert rc_of('oriana_colsum_f64', p, p, None, 2, 513) == EKRANGE
    # vectors
    for name, il, required in (('oriana_threshold_f32', 3, (0, 1)), ('oriana_mul_f64_f32', 3, (0, 1, 2))):
        a = good[name]
        assert rc_of(name, *with_(a, il, -1)) == EINVAL, name
        for i in required:
            assert rc_of(name, *with_(a, i, None)) == EINVAL, (name, i)
        assert rc_of(name, *with_(tuple(None if i in required else v for i, v in enumerate(a)), il, 0)) == 0, name
    # wide (rows, m) entries: either size 0 is an empty matrix
    for name, ir, required in (('oriana_colsum_wide_f64', 2, (0, 1)), ('oriana_colsum_wide_f32', 2, (0, 1)), ('oriana_nzmask_f32', 2, (0, 1)),
                               ('oriana_dropout_update', 6, (0, 1, 2, 3))):
        a = good[name]
        assert rc_of(name, *with_(a, ir, -1)) == EINVAL and rc_of(name, *with_(a, ir + 1, -1)) == EINVAL, name
        for i in required:
            assert rc_of(name, *with_(a, i, None)) == EINVAL, (name, i)
        empty = tuple(None if i in required else v for i, v in enumerate(a))
        assert rc_of(name, *with_(empty, ir, 0)) == 0 and rc_of(name, *with_(empty, ir + 1, 0)) == 0, name
    a = good['oriana_take_cols_f32']
    for i, v in ((2, -1), (3, -1), (4, 0), (4, 4), (0, None), (1, None)):
        assert rc_of('oriana_take_cols_f32', *with_(a, i, v)) == EINVAL, (i, v)
    assert rc_of('oriana_take_cols_f32', None, None, 0, 3, 3) == 0
    torch.cuda.synchronize()


# ---- 3. the second launch of the entries that chunk their grid at 65535 blocks in y ---------------------------------------
GRID_Y = 65535


def _marked(rows, m, boundary, dtype, background):
    """A constant matrix with position-dependent dyadic values (every sum of them is exact in float64, whatever the order)
    in the rows around the start, the chunk boundary and the end.  Returns (device matrix, exact column sums)."""
    A = torch.full((rows, m), background, dtype=dtype, device='cuda')
    marks = [0, 1, 255, 256, 299, boundary - 257, boundary - 1, boundary, boundary + 1, boundary + 255, boundary + 256, rows - 1]
    vals = np.array([[(1 + i) * 1024.0 + (j + 1) * 0.25 * (1 + i) for j in range(m)] for i in range(len(marks))])
    A[torch.tensor(marks, device='cuda')] = torch.from_numpy(vals).to(dtype).cuda()
    exp = background * (rows - len(marks)) + vals.sum(0)
    return A, exp


@pytest.mark.parametrize('m', [1, 3])
@pytest.mark.parametrize('name,dtype', [('oriana_colsum_wide_f64', torch.float64), ('oriana_colsum_wide_f32', torch.float32)])
def test_colsum_wide_second_launch(name, dtype, m):
    rows = GRID_Y * 256 + 300                             # the second launch starts at row 65535 * 256 and covers 300 rows
    A, exp = _marked(rows, m, GRID_Y * 256, dtype, 0.5)
    out0 = np.arange(1.0, m + 1)                           # the entry adds into out
    out = dev(out0)
    call(name, ptr(out), ptr(A), rows, m)
    got = host(out)
    del A
    assert np.array_equal(got, out0 + exp), (got - out0 - exp)


def _nz_counts(rng, rows, m, boundary):
    X = (rng.random((rows, m)) < 0.3).astype(F32) * 3
    X[boundary - 2:boundary + 2] = [[1, 0, 1], [0, 1, 0], [1, 1, 0], [0, 0, 1]]       # distinct words on either side of the boundary
    X[:2] = [[0, 1, 1], [1, 0, 0]]
    return X


def test_nzmask_second_launch():
    rows, m = GRID_Y * 32 + 40, 3                         # word row 65535 is the first of the second launch
    X = _nz_counts(np.random.default_rng(3), rows, m, GRID_Y * 32)
    nw = (rows + 31) // 32
    mask = torch.full((nw * m,), -1, dtype=torch.int32, device='cuda')
    dX = dev(X)
    call('oriana_nzmask_f32', ptr(mask), ptr(dX), rows, m)
    got = host(mask).view(np.uint32)
    exp = lr.nzmask_words(X)
    assert np.array_equal(got[:GRID_Y * m], exp[:GRID_Y * m])
    assert np.array_equal(got[GRID_Y * m:], exp[GRID_Y * m:])
    assert exp[GRID_Y * m:].any() and not np.array_equal(exp[GRID_Y * m:], exp[:2 * m])


def test_dropout_update_second_launch():
    """oriana_dropout_update past 65535 blocks of 64 rows, with the non-zero mask (itself past 65535 word rows) and the column
    sums: the documented statement in float64.  p_d to 1e-15 (one ulp of exp / log either way at p <= 1), D_hat = float32 of the
    entry's own p_d, the column sums of 4.2e6 terms to 1e-11 relative (64 sequential additions and 65537 atomics per column:
    6.6e4 x 1.1e-16 = 7.3e-12 at worst)."""
    rows, m = GRID_Y * 64 + 70, 3
    B = GRID_Y * 64
    rng = np.random.default_rng(4)
    X = _nz_counts(rng, rows, m, B)
    Lam = rng.random((rows, m)) * 6
    Lam[B - 1:B + 1] = [[0.125, 9.0, 3.0], [7.0, 0.25, 11.0]]
    pi = np.array([0.3, 0.6, 0.05])
    mask = torch.zeros(((rows + 31) // 32) * m, dtype=torch.int32, device='cuda')
    dX, dL, dpi = dev(X), dev(Lam), dev(pi)
    call('oriana_nzmask_f32', ptr(mask), ptr(dX), rows, m)
    assert np.array_equal(host(mask).view(np.uint32), lr.nzmask_words(X))
    p_d = torch.full((rows, m), float('nan'), dtype=torch.float64, device='cuda')
    D_hat = torch.full((rows, m), float('nan'), device='cuda')
    cs = torch.zeros(m, dtype=torch.float64, device='cuda')
    call('oriana_dropout_update', ptr(p_d), ptr(D_hat), ptr(dL), ptr(dpi), ptr(mask), ptr(cs), rows, m)
    exp_p, _, exp_cs = lr.dropout_update(Lam, pi, X != 0)
    got = host(p_d)
    for lo, hi in ((0, B), (B, rows)):
        assert np.abs(got[lo:hi] - exp_p[lo:hi]).max() <= 1e-15, (lo, hi)
    assert same_bits(host(D_hat), got.astype(F32))
    assert (np.abs(host(cs) - exp_cs) <= 1e-11 * exp_cs).all()
    # the same without mask and sums: the second launch's pointers alone
    call('oriana_dropout_update', ptr(p_d), ptr(D_hat), ptr(dL), ptr(dpi), None, None, rows, m)
    exp_p, _, _ = lr.dropout_update(Lam, pi)
    assert np.abs(host(p_d) - exp_p).max() <= 1e-15
