# -*- coding: utf-8 -*-
"""The log sums of the ZI / sparse loop nests and the element-wise kernels beside them, restated in plain NumPy for
tests/test_sparse_side_gpu.py and tests/test_logsum_host.py.

Written from include/oriana_hip.h (the statements of oriana_log_center, oriana_scale_factor[_centered], oriana_finalize_zlog,
oriana_sparsity_update, oriana_dropout_update, oriana_nzmask_f32, ...) and from the reference statements they cite
(sparse_gap.py:113, 134-141, 165; zigap.py:130-136, 158) -- not from the kernels.

Three parts:
  * drift_case(): the inputs of the scale-drift checks of Z_log, with the float64 value (cavi_oracle.zq_exact) and the
    reference's own float32 loop nest on the same inputs, computed once per case and shared;
  * logsum_f32(): the log sums  FV (sum_i s FU (lu - a)) + (lv + a) FV sum_i s FU  evaluated with float32 per-gene sums,
    with the per-factor centre a_k or without it (a = 0) -- what the bound on Z_log has to tell apart;
  * one function per side kernel: the documented statement in float64 (or in the number format the header names)."""
import functools
import math

import numpy as np

# ---- the drift cases ------------------------------------------------------------------------------------------------------
DRIFT_N, DRIFT_M = 300, 260                      # two gene tiles, the second ragged
DRIFT_SHIFTS = {'centred': (0.0, 0.0, False), 'u+35': (35.0, -30.0, False), 'u-40': (-40.0, 38.0, False),
                'u+35-slow': (35.0, -30.0, True)}           # (shift of E[log U], of E[log V], one cell at lu - 80)
# form -> (K, nest): every row of DESIGN.md section 0's per-form table that produces Z_log
DRIFT_FORMS = {'fused-K20': (20, 'sparse'), 'fused-K64': (64, 'sparse'), 'four-kernel-K100': (100, 'sparse'),
               'wide-K200': (200, 'sparse'), 'weighted-K64': (64, 'sparse-zi'), 'quirk-K20': (20, 'zi-quirk'),
               'hybrid-K50': (50, 'sparse-hybrid')}
DEAD_GENE = 5
SLOW_CELL = 3


def _drift_counts(rng, n, m, hybrid):
    if not hybrid:                               # the counts of test_scale_drift_keeps_the_fast_path
        return ((rng.poisson(3.0, size=(n, m)) + 1) * (rng.random((n, m)) < 0.2)).astype(np.float32)
    # dense-first gene densities of test_zq_sparse_hybrid_vs_oracle: at least 32 genes reach dense_density = 0.3
    dens = np.clip(rng.beta(1.0, 2.0, size=m), 0.01, 1.0)
    dens[:40] = np.linspace(1.0, 0.4, 40)
    X = rng.poisson(40.0, size=(n, m)).astype(np.int64) + 1
    X[rng.random((n, m)) < 0.02] = 3000
    X *= (rng.random((n, m)) < dens[None, :])
    return X.astype(np.float32)


@functools.lru_cache(maxsize=None)
def drift_case(form, shift):
    """dict(X, lu, lv, St, Sh, D, dq, K, nest, slow, exact=(Z_i, Z_j, Z_log) float64, ref=(...) the reference's float32
    nest).  Computed once; callers must not write into the arrays."""
    from oracle import cavi_oracle as co
    K, nest = DRIFT_FORMS[form]
    su, sv, slow = DRIFT_SHIFTS[shift]
    n, m = DRIFT_N, DRIFT_M
    rng = np.random.default_rng(11 + K)
    X = _drift_counts(rng, n, m, nest == 'sparse-hybrid')
    lu = (rng.normal(size=(n, K)) * 1.5 + su).astype(np.float32)
    lv = (rng.normal(size=(m, K)) * 1.5 + sv).astype(np.float32)
    if slow:
        lu[SLOW_CELL] -= 80.0
    c = dict(X=X, lu=lu, lv=lv, St=None, Sh=None, D=None, dq=None, K=K, nest=nest, slow=slow, form=form, shift=shift)
    if nest != 'zi-quirk':
        ps = rng.random((m, K))
        c['St'] = (ps > 0.3).astype(np.float32)
        c['Sh'] = ps.astype(np.float32)
        c['St'][DEAD_GENE] = 0.0                  # a gene with every factor switched off
    if nest == 'sparse-zi':
        c['D'] = rng.random((n, m)).astype(np.float32)          # a general D_hat: per-entry weights
    if nest == 'zi-quirk':
        D = rng.random((n, m)).astype(np.float32)
        D[X != 0] = 1.0                           # what the models hold (zigap.py:135): no per-entry weights needed
        c['D'] = D
        c['dq'] = np.ascontiguousarray(D[:, :K])  # zigap.py:94 reads D_hat[i, k]
    r = [np.empty((n, K), np.float32), np.empty((m, K), np.float32), np.empty((m, K), np.float32)]
    with np.errstate(all='ignore'):
        if nest in ('sparse', 'sparse-hybrid'):
            co.zq_sparse_gap(r[0], r[1], r[2], lu, lv, c['St'], c['Sh'], X)
        elif nest == 'sparse-zi':
            co.zq_sparse_zigap(r[0], r[1], r[2], lu, lv, c['St'], c['Sh'], c['D'], X)
        else:
            co.zq_zigap(r[0], r[1], r[2], lu, lv, c['D'], X, quirk=True)
        c['exact'] = co.zq_exact(lu, lv, X, c['St'], c['Sh'], c['D'], quirk=(nest == 'zi-quirk'))
    c['ref'] = tuple(r)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def logsum_f32(lu, lv, X, S_tilde=None, center=False):
    """Z_log[j, k] = sum_i r_ijk (lu_ik + lv_jk) as the shifted form evaluates it with float32 per-gene sums:
        FU = exp(lu - rowmax), FV = exp(lv - rowmax) [S_tilde], s_ij = x_ij / sum_k FU_ik FV_jk   (r_ijk = s_ij FU_ik FV_jk)
        Z_log = FV (sum_i s FU (lu - a)) + (lv + a) FV (sum_i s FU),
    the two sums over i accumulated in float32 row by row, the combination in float64 rounded once.  center=False: a = 0, two
    plain sums that are each |lu| times larger than their total once lu has drifted.  center=True: a_k = the mean of lu_ik
    weighted by the cell's own responsibility sums (float64)."""
    f32 = np.float32
    lu = np.asarray(lu, f32); lv = np.asarray(lv, f32); X = np.asarray(X, f32)
    n, K = lu.shape
    FU = np.exp(lu - lu.max(1, keepdims=True)).astype(f32)
    FV = np.exp(lv - lv.max(1, keepdims=True)).astype(f32)
    if S_tilde is not None:
        FV = FV * np.asarray(S_tilde, f32)
    den = FU.astype(np.float64) @ FV.astype(np.float64).T
    s = np.where((X != 0) & (den > 0), X / np.where(den > 0, den, 1.0), 0.0).astype(f32)
    a = np.zeros(K)
    if center:
        Zi = FU.astype(np.float64) * (s.astype(np.float64) @ FV.astype(np.float64))
        a = (Zi * lu).sum(0) / np.maximum(Zi.sum(0), 1e-300)
    G = (FU * (lu.astype(np.float64) - a).astype(f32)).astype(f32)
    C = np.zeros((lv.shape[0], K), f32)
    C2 = np.zeros_like(C)
    for i in range(n):
        nz = np.nonzero(s[i])[0]
        C[nz] += s[i, nz, None] * FU[i][None, :]              # float32 products, float32 running sums
        C2[nz] += s[i, nz, None] * G[i][None, :]
    z = FV.astype(np.float64) * (C2.astype(np.float64) + (lv.astype(np.float64) + a) * C.astype(np.float64))
    return z.astype(f32)


# ---- the side kernels, each from its statement in the header ---------------------------------------------------------------
def _src(row_index, r):
    return np.arange(r) if row_index is None else np.asarray(row_index, dtype=np.int64)


def log_center(F, logF, W, row_index, K):
    """acc[0..K) = sum w logF, acc[K..2K) = sum w over the entries that carry weight: F > 1e-20 (float32), |logF| < 1e30,
    0 < w < inf; w = W[src, k] or 1; logF and W in the caller's row order (src = row_index[row]).  float64 sums."""
    F = np.asarray(F, np.float32)
    r = F.shape[0]
    src = _src(row_index, r)
    f = F[:, :K]
    l = np.asarray(logF, np.float32)[src][:, :K]
    w = np.ones((r, K)) if W is None else np.asarray(W, np.float32)[src][:, :K].astype(np.float64)
    with np.errstate(all='ignore'):
        ok = (f > np.float32(1e-20)) & (np.abs(l) < np.float32(1e30)) & (w > 0) & np.isfinite(w)
    wl = np.where(ok, w, 0.0)
    ll = np.where(ok, l.astype(np.float64), 0.0)
    return np.concatenate([(wl * ll).sum(0), wl.sum(0)])


def centre_of(acc, K):
    """a_k = acc[k] / acc[K + k] where a cell counted, else 0; acc None: 0."""
    if acc is None:
        return np.zeros(K)
    acc = np.asarray(acc, np.float64)
    with np.errstate(all='ignore'):
        return np.where(acc[K:2 * K] > 0, acc[:K] / np.where(acc[K:2 * K] > 0, acc[K:2 * K], 1.0), 0.0)


def scale_factor(Fin, mul, row_index, K, zero_guard):
    """Fout[i, k] = Fin[i, k] * mul[src(i), k] (one float32 product), pad columns 0; zero_guard: +0 wherever Fin == 0."""
    Fin = np.asarray(Fin, np.float32)
    r, Kp = Fin.shape
    out = np.zeros((r, Kp), np.float32)
    with np.errstate(all='ignore'):
        out[:, :K] = Fin[:, :K] * np.asarray(mul, np.float32)[_src(row_index, r)][:, :K]
    if zero_guard:
        out[:, :K][Fin[:, :K] == 0] = 0.0
    return out


def scale_factor_centered(Fin, mul, acc, row_index, K):
    """Fout = float32(Fin * float32(double(mul) - a_k)), +0 where Fin == 0, pad columns 0."""
    Fin = np.asarray(Fin, np.float32)
    r, Kp = Fin.shape
    out = np.zeros((r, Kp), np.float32)
    with np.errstate(all='ignore'):
        d = (np.asarray(mul, np.float32)[_src(row_index, r)][:, :K].astype(np.float64) - centre_of(acc, K)).astype(np.float32)
        out[:, :K] = Fin[:, :K] * d
    out[:, :K][Fin[:, :K] == 0] = 0.0
    return out


def finalize_zlog(Zlog, FV, C2, C, logV, acc, row_index, K):
    """Zlog[o, k] += float32(FV[j, k] (C2[j, k] + (logV[o, k] + a_k) C[j, k])), o = row_index[j]: the bracket in float64,
    rounded once; a row with FV == 0 adds an exact 0 whatever the other operands hold.  Returns the new Zlog."""
    out = np.array(Zlog, np.float32)
    r = np.asarray(FV).shape[0]
    o = _src(row_index, r)
    f = np.asarray(FV, np.float64)[:, :K]
    with np.errstate(all='ignore'):
        v = f * (np.asarray(C2, np.float64)[:, :K] + (np.asarray(logV, np.float64)[o] + centre_of(acc, K)) * np.asarray(C, np.float64)[:, :K])
        v = np.where(f != 0, v, 0.0).astype(np.float32)
        out[o] = out[o] + v
    return out


def logit(x):
    x = np.clip(x, 1e-15, 1. - 1e-15)
    return np.log(x / (1. - x))


def sigmoid(x):
    with np.errstate(over='ignore'):
        return 1. / (1. + np.exp(-x))


def sparsity_update(pi_s, Zlog, c, Vprime_hat):
    """sparse_gap.py:134-141, line by line.  Zlog float32 (m, K); c: [K] or (m, K) float64; returns (p_s, S_hat).  `tmp` is
    a float32 array that a float64 term is added to IN PLACE: the sum is formed in float64 and rounded to float32."""
    pi_s = np.asarray(pi_s, np.float64)
    with np.errstate(all='ignore'):
        tmp = -np.asarray(Zlog, np.float32)
        tmp += np.nan_to_num(np.asarray(c, np.float64) * np.asarray(Vprime_hat, np.float64))
        p_s = sigmoid(logit(pi_s)[..., np.newaxis] - tmp)
        p_s = np.nan_to_num(p_s)
    p_s[pi_s <= 0] = 1e-10
    p_s[pi_s >= 1] = 1. - 1e-10
    return p_s, p_s.astype(np.float32)


def threshold(p, tau):
    """S_tilde = (p_s > tau) as float32 (sparse_gap.py:113); NaN compares false."""
    with np.errstate(invalid='ignore'):
        return (np.asarray(p, np.float64) > tau).astype(np.float32)


def rowmean(A):
    """mean over a short contiguous row, summed left to right (pi_s = mean(p_s, axis=1), sparse_gap.py:165)."""
    A = np.asarray(A, np.float64)
    out = np.empty(A.shape[0])
    for i in range(A.shape[0]):
        s = 0.0
        for v in A[i]:
            s = s + float(v)
        out[i] = s / A.shape[1]
    return out


def colsum(A, mul=None):
    """Exact column sums (math.fsum: NumPy's running sum down a column is biased at millions of rows)."""
    A = np.asarray(A, np.float64)
    P = A if mul is None else A * np.asarray(mul, np.float64)
    return np.array([math.fsum(P[:, j]) for j in range(P.shape[1])])


def nzmask_words(D):
    """word [(i // 32) * m + j], bit i % 32 = (D[i, j] != 0); ceil(rows / 32) * m words."""
    D = np.asarray(D)
    rows, m = D.shape
    nw = (rows + 31) // 32
    nz = np.zeros((nw * 32, m), dtype=np.uint32)
    nz[:rows] = D != 0
    return (nz.reshape(nw, 32, m) << np.arange(32, dtype=np.uint32)[None, :, None]).sum(1, dtype=np.uint32).reshape(-1)


def dropout_update(Lambda, pi_d, nz=None):
    """p_d = sigmoid(logit(pi_d)[None, :] - Lambda); columns with pi_d <= 0 -> 1e-10, pi_d >= 1 -> 1 - 1e-10; the entries of
    `nz` (X != 0) -> 1 - 1e-10 (zigap.py:130-136).  Returns (p_d, D_hat = float32(p_d), column sums of p_d)."""
    pi_d = np.asarray(pi_d, np.float64)
    p = sigmoid(logit(pi_d)[np.newaxis, :] - np.asarray(Lambda, np.float64))
    p[:, pi_d <= 0] = 1e-10
    p[:, pi_d >= 1] = 1. - 1e-10
    if nz is not None:
        p[np.asarray(nz, bool)] = 1. - 1e-10
    return p, p.astype(np.float32), colsum(p)
