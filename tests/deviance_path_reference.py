# -*- coding: utf-8 -*-
"""float64 restatement of FactorModel.deviance_path() (the formulas in the comment above factor_order in models/base.py and
the one above _count_constants), every sum in long double.

With an order o of the factors, Lambda^(k) = sum_{l < k} U[:, o_l] V[:, o_l]^T, N = {X != 0}, keep0 = {X == 0} minus the
mask {round(D_hat) == 0} of the ZI models, pi the dropout probabilities (1 without a dropout node):

    zz0^(k)   = sum_keep0 log(pi_j e^-Lambda^(k) + 1 - pi_j)
    ll_uv^(k) = zz0^(k) + sum_N log pi_j - sum_N Lambda^(k) + sum_N x log Lambda^(k)
    ll_x      = sum_N log pi_j + sum_N (x log x - x)
    ll_mean   = sum_{X == 0} log(pi_j e^-mu_j + 1 - pi_j) + sum_N (log pi_j - mu_j + x log mu_j),   mu_j = mean_i X_ij
    ed^(k)    = (ll_uv^(k) - ll_mean) / (ll_x - ll_mean),      rd^(k) = -2 (ll_uv^(k) - ll_x)

`path` evaluates this per prefix, together with the same from float32 factors (a running float32 sum in the order of the
factors, as the HIP kernel forms it) and the tolerance of every value (`_bounds`), derived from the arithmetic and never
measured on the code under test -- the rule of tests/test_metrics_gpu.py: where the kernel's rate is a float32 value (a
stored entry of the sliced layout whose float32 running sum is at least 1e-10), |d Lambda^(k)| <= gamma_k Lambda^(k) with
gamma_k = (k + 3) 2^-24; everything else (the dense block, the float64 fall-back, the dropout term, the column sums) is
float64 and gets ACC, relative to the sum of the absolute terms.  The bound is the larger of that and F_REF times the distance
of the float32 evaluation from float64.
"""
import numpy as np

F_REF = 8.0
ACC = 1e-12


def _ld(a):
    return np.sum(np.asarray(a, dtype=np.longdouble))


def _log_zero_term(lam, p):
    """log(p e^-lam + 1 - p); p = 1: -lam (the literal form underflows to log 0 from lam ~ 745 on)."""
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        return np.where(p == 1.0, -lam, np.log(p * np.exp(-lam) + (1.0 - p)))


def constants(X, pi):
    """ll_x, ll_mean, sum_N log pi and the sums of their absolute terms."""
    X = np.asarray(X, dtype=np.float64)
    n, m = X.shape
    N = X != 0
    P = np.broadcast_to(np.asarray(pi, dtype=np.float64)[np.newaxis, :], (n, m))
    mu = X.sum(axis=0, dtype=np.longdouble).astype(np.float64) / n
    Mu = np.broadcast_to(mu[np.newaxis, :], (n, m))
    x = X[N]
    with np.errstate(divide='ignore', invalid='ignore'):
        lpi = np.log(P[N])
        xlx = x * np.log(x) - x
        mean_z = _log_zero_term(Mu[~N], P[~N])
        mean_n = lpi - Mu[N] + x * np.log(np.where(Mu[N] > 0, Mu[N], 1.0))
    return dict(ll_x=float(_ld(lpi) + _ld(xlx)), ll_mean=float(_ld(mean_z) + _ld(mean_n)), lpi=float(_ld(lpi)),
                abs_lpi=float(_ld(np.abs(lpi))), abs_xlx=float(_ld(np.abs(xlx))),
                abs_mean=float(_ld(np.abs(mean_z)) + _ld(np.abs(mean_n))), sum_x=float(_ld(x)))


def _public(ll_uv, c):
    with np.errstate(invalid='ignore'):
        return (ll_uv - c['ll_mean']) / (c['ll_x'] - c['ll_mean']), -2.0 * (ll_uv - c['ll_x'])


def full_metric(X, U, V, pi, keep0):
    """The full metric's formulas on Lambda = U V^T as one matrix product: (ll_uv, ed, rd)."""
    X = np.asarray(X, dtype=np.float64)
    N = X != 0
    Lam = np.asarray(U, dtype=np.float64) @ np.asarray(V, dtype=np.float64).T
    P = np.broadcast_to(np.asarray(pi, dtype=np.float64)[np.newaxis, :], X.shape)
    c = constants(X, pi)
    with np.errstate(divide='ignore', invalid='ignore'):
        ll_uv = float(_ld(_log_zero_term(Lam[keep0], P[keep0])) + c['lpi'] - _ld(Lam[N]) + _ld(X[N] * np.log(Lam[N])))
    ed, rd = _public(ll_uv, c)
    return ll_uv, float(ed), float(rd)


def path(X, U, V, pi, keep0, order, ks, zi, f32_cols=None):
    """Per prefix length of `ks` (int array, within 1..K) in the factor order `order`: the internal sums, ll_uv, ed, rd in
    float64, the same from float32 factors, and the tolerances.  `f32_cols`: boolean per gene, True where the HIP code forms
    the rate from float32 factors (the sliced layout; False: the dense block of a hybrid layout).  `zi`: the model has a
    dropout node (its zero term comes from a float64 kernel, not from column sums)."""
    X = np.asarray(X, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    pi = np.asarray(pi, dtype=np.float64)
    order = np.asarray(order, dtype=np.int64)
    ks = np.asarray(ks, dtype=np.int64)
    n, m = X.shape
    N = X != 0
    P = np.broadcast_to(pi[np.newaxis, :], (n, m))
    x, pz = X[N], P[keep0]
    f32_at = np.broadcast_to((np.ones(m, dtype=bool) if f32_cols is None else np.asarray(f32_cols, dtype=bool))[np.newaxis, :],
                             (n, m))[N]
    c = constants(X, pi)
    U32, V32 = U.astype(np.float32), V.astype(np.float32)
    Lam = np.zeros((n, m))
    Lam32 = np.zeros((n, m), dtype=np.float32)
    want = set(int(k) for k in ks)
    names = ('lam', 'xlog', 'zz0', 'll_uv', 'ed', 'rd')
    ref = {k: [] for k in names}
    f32 = {k: [] for k in names}
    tol = {k: [] for k in names}
    tol_full = {k: [] for k in names}
    tol_acc = {k: [] for k in names}
    for l in range(int(ks[-1])):
        o = order[l]
        Lam += np.outer(U[:, o], V[:, o])
        Lam32 += np.outer(U32[:, o], V32[:, o])               # (float32 products and sums, in the order of the factors)
        k = l + 1
        if k not in want:
            continue
        lam, lz, lam32 = Lam[N], Lam[keep0], Lam32[N]
        # the float32 evaluation: the running float32 sum where it is at least 1e-10 on a float32 gene, float64 elsewhere
        lam_f = np.where(f32_at & (lam32 >= np.float32(1e-10)), lam32.astype(np.float64), lam)
        # where the HIP rate MAY be a float32 value: two float32 sums of the same k terms in different arithmetic (fused or
        # not) differ by less than gamma_k relative, so what one of them sees at 1e-10 the other sees above half of that
        may32 = f32_at & (lam32 >= np.float32(5e-11))
        tz0 = _log_zero_term(lz, pz)                          # (the zero term is float64 in both evaluations)
        s_tz0, a_tz0, s_lz = _ld(tz0), float(_ld(np.abs(tz0))), float(_ld(lz))
        lam_may, x_may, all_lam = float(_ld(lam[may32])), float(_ld(x[may32])), float(_ld(Lam.sum(axis=0)))
        out = []
        for lm in (lam, lam_f):
            with np.errstate(divide='ignore', invalid='ignore'):
                xlog = x * np.log(lm)
            s_lam, s_xlog = _ld(lm), _ld(xlog)
            ll_uv = float(s_tz0 + c['lpi'] - s_lam + s_xlog)
            ed, rd = _public(ll_uv, c)
            out.append(dict(lam=float(s_lam), xlog=float(s_xlog), zz0=float(s_tz0), ll_uv=ll_uv, ed=float(ed), rd=float(rd),
                            abs_xlog=float(_ld(np.abs(xlog))), abs_tz0=a_tz0, lz=s_lz, lam_f32=lam_may, x_f32=x_may,
                            all_lam=all_lam))
        b = _bounds(out[0], out[1], c, k, zi)
        b_full, b_acc = _bounds(out[0], None, c, k, zi, 'all'), _bounds(out[0], None, c, k, zi, 'none')
        for q in names:
            ref[q].append(out[0][q]); f32[q].append(out[1][q]); tol[q].append(b[q])
            tol_full[q].append(b_full[q]); tol_acc[q].append(b_acc[q])
    res = {q: np.array(ref[q], dtype=np.float64) for q in names}
    res['f32'] = {q: np.array(f32[q], dtype=np.float64) for q in names}
    res['tol'] = {q: np.array(tol[q], dtype=np.float64) for q in names}
    res['tol_full'] = {q: np.array(tol_full[q], dtype=np.float64) for q in names}
    res['tol_acc'] = {q: np.array(tol_acc[q], dtype=np.float64) for q in names}
    res['const'] = c
    res['k'] = ks
    return res


def subset(ref, ks):
    """The reference of `path` restricted to the prefix lengths `ks` (all of which it holds)."""
    pos = {int(k): t for t, k in enumerate(ref['k'])}
    sel = np.array([pos[int(k)] for k in ks], dtype=np.int64)
    out = {}
    for q, v in ref.items():
        if isinstance(v, dict) and q != 'const':
            out[q] = {a: b[sel] for a, b in v.items()}
        elif q == 'const':
            out[q] = v
        else:
            out[q] = v[sel]
    return out


def diff(got, ref):
    """|got - ref|, 0 where both are the same infinity."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.where(got == ref, 0.0, np.abs(got - ref))


def _bounds(r, f, c, k, zi, f32='some'):
    """f32='some': the float32 share of the prefix kernel (r['lam_f32'], r['x_f32']); 'all': every stored entry a float32 rate,
    no float32-distance term (the full metric's own bound, tests/test_metrics_gpu.py: _bounds, at K = k); 'none': float64
    accumulation alone (two evaluations of the same arithmetic that differ in the order of the atomics)."""
    g = (k + 3) * 2.0 ** -24
    lam_f32 = {'some': r['lam_f32'], 'all': r['lam'], 'none': 0.0}[f32]
    x_f32 = {'some': r['x_f32'], 'all': c['sum_x'], 'none': 0.0}[f32]
    with np.errstate(invalid='ignore'):
        b_lam = g * lam_f32 + ACC * r['lam']
        b_xlog = -np.log1p(-g) * x_f32 + ACC * r['abs_xlog']
        if zi:                   # the dropout metric kernel: float64 matrix cores
            b_zz0 = ACC * (r['abs_tz0'] + r['lz'])
            b_lluv = b_zz0 + b_lam + b_xlog + ACC * c['abs_lpi']
        else:                    # zz0 - sum_N Lambda = -(sum over all entries), from float64 column sums
            b_zz0 = b_lam + ACC * r['all_lam']
            b_lluv = ACC * r['all_lam'] + b_xlog + ACC * c['abs_lpi']
        b_llx = ACC * (c['abs_xlx'] + c['abs_lpi'])
        b_mean = ACC * (c['abs_mean'] + c['abs_lpi'])
        den = abs(c['ll_x'] - c['ll_mean'])
        b_ed = (b_lluv + b_mean + abs(r['ed']) * (b_llx + b_mean)) / den if den > 0 else np.inf
        tol = dict(lam=b_lam, xlog=b_xlog, zz0=b_zz0, ll_uv=b_lluv, ed=b_ed, rd=2 * (b_lluv + b_llx))
        for q in tol:
            tol[q] = float(np.fmax(tol[q], F_REF * diff(f[q], r[q]))) if f32 == 'some' else float(tol[q])
    return tol


def check(got, ref, keys=('ed', 'rd'), tol='tol', what=''):
    """Every value of `got` (the dict of deviance_path) against the reference: an infinite reference value is matched exactly,
    a finite one within its bound ref[tol]."""
    names = {'ed': 'explained_deviance', 'rd': 'reconstruction_deviance'}
    for q in keys:
        g = np.asarray(got[names.get(q, q)], dtype=np.float64)
        r, t = ref[q], ref[tol][q]
        assert g.shape == r.shape, (what, q, g.shape, r.shape)
        for i in range(r.size):
            if np.isfinite(r[i]):
                d = abs(g[i] - r[i])
                assert np.isfinite(g[i]) and d <= t[i], '%s %s at k=%d: got %.17g ref %.17g diff %.3e > bound %.3e' % (
                    what, q, ref['k'][i], g[i], r[i], d, t[i])
            else:
                assert g[i] == r[i], '%s %s at k=%d: got %r, the reference is %r' % (what, q, ref['k'][i], g[i], r[i])
