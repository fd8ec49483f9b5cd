# -*- coding: utf-8 -*-
"""A plain float64 statement of the Gamma shape/rate update and of the M-step (csrc/updates.hip: k_gamma_update,
k_gamma_update_vec, k_mstep_gamma, k_mstep_gamma_pair), the error bound their float32 E[log .] has to keep, inputs on which
every float32 operation of the kernels is exact, a restatement of the launch rule and the table of cases that reaches every
instantiation of it.  NumPy / SciPy only: no torch, no GPU.  Used by test_gamma_update_host.py, test_gamma_update_gpu.py
and test_fused_prep_gpu.py.

What one call computes (gap.py:96-110 with the clamps of gap.py:99-100, gamma.py:37-61; the ZI forms zigap.py:114-141):

  finalize   Z[o] += F[p] * sum_s R_s[p]          o = row_index[p]; the slabs are added in float32, in slab order; slab 0
                                                  holds every packed row, a slab s >= 1 only the rows p >= slab_row0, as
                                                  (r - slab_row0) rows that follow the slab before it
  shape      a1 = max(1e-15, nan_to_num(prior1 + z))            z = Z, or the FLOAT32 product zmul * Z
  rate       a2 = max(1e-15, nan_to_num(prior2 + rate))         rate = rate_vec[k], or rate_mat, or f64(rmul) * rate_mat
  stored     Z is None: a1 and a2 are taken as given
  E          a1 / a2
  E[log]     f32( f32(digamma(f64(f32 a1))) - logf(f32 a2) )

THE BOUND ON E[log .]  (elog_bound).  With psi = digamma(f64(f32(a1))), lg = log(f64(f32(a2))), both exact, and
u = 2^-24 (half a float32 ulp, relative), the kernel goes through four roundings:
  1. its float64 digamma: common.h states |digamma_pos_for_f32(x) - psi(x)| < 2e-13 (truncation of the series and of the
     short logarithm; the float64 roundings of the six-step recurrence are relative, a few 2^-53 |psi|, far below 3.)
  2. psi is cast to float32:                                  <= u |psi|
  3. logf: L float32 ulps, an ulp being at most 2 u |lg|:     <= L * 2u |lg|
  4. the float32 subtraction:                                 <= u |result|, a result below the normal range: 2^-149
so that  |Elog - (psi - lg)| <= u |psi| + L * 2u |lg| + u |psi - lg| + 2e-13 + 2^-149  element by element (terms of
order u^2 left out: they are 2^-24 of the bound).  No maximum over the matrix enters: an element with a small |psi| and a
small |lg| is held to an absolute error of a few 1e-8 even when its neighbour sits at the clamp (psi(1e-15) = -1e15).
L = 2: the HIP math documentation (its table of the largest ulp errors of the device functions) is not part of the
installed ROCm tree that this suite runs against, so the figure is the one the issue names as the fall-back; the OCML
sources document logf with 1 ulp, i.e. L = 2 leaves one ulp of room and no more.

EXACT INPUTS (dyadic_*).  F and Z are multiples of 2^-8 below 1 and 16, R holds integers below 64, at most three slabs:
sum_s R_s < 2^8 is exact, F * rr is a multiple of 2^-8 below 2^8 and F * rr + Z one below 2^8 + 2^4, i.e. 17 bits -- every
float32 operation of the finalize step is exact, in any order and fused or not.  zmul is a multiple of 2^-8 in [0, 1]:
zmul * Z has 20 bits.  rate_mat (multiples of 2^-10 below 64) times rmul (multiples of 2^-8 in [0, 1]) is exact in
float64, so that a compiler that contracts prior2 + rmul * rate into one fused operation forms the same bits as one that
does not.  prior1, prior2 and rate_vec are arbitrary doubles: each enters ONE float64 addition.  Z_out, a1 and a2 are
therefore compared bit for bit.
"""
import math

import numpy as np
import scipy.special

U32 = 2.0 ** -24           # half a float32 ulp, relative
U64 = 2.0 ** -53
LOGF_ULPS = 2              # L above
DIGAMMA_ABS = 2e-13        # common.h, digamma_pos_for_f32
EPS = 1e-15
DBL_MAX = np.finfo(np.float64).max

A1_LADDER = [1e-15, 1e-8, 1e-3, 0.0099, 0.01, 1.0, 5.999, 6.0, 20.0, 20.5, 1e3, 1e7, 1e30]
A2_LADDER = [1e-15, 1e-8, 1e-3, 1.0, 1e3, 1e6, 1e12]


def clamp(a):
    """np.maximum(1e-15, np.nan_to_num(a))  (gap.py:99-100)"""
    with np.errstate(all='ignore'):
        return np.maximum(EPS, np.nan_to_num(np.asarray(a, dtype=np.float64)))


def slab_rows(r, nslab, slab_row0):
    """Rows of the packed R buffer: slab 0 whole, every further slab from slab_row0 on."""
    return r + (nslab - 1) * (r - slab_row0)


def finalize_ref(Z, F, R, K, nslab=1, slab_row0=0, row_index=None, dtype=np.float64):
    """Z[o] + F[p] * sum_s R_s[p] in `dtype` arithmetic (the slab sum in float32 either way), rounded to float32."""
    Z = np.asarray(Z, dtype=np.float32)
    r = Z.shape[0]
    F = np.asarray(F, dtype=np.float32)[:r, :K]
    R = np.asarray(R, dtype=np.float32)
    rr = R[:r, :K].copy()
    for s in range(1, nslab):
        base = s * (r - slab_row0)                       # the slab is indexed by the absolute packed row
        rr[slab_row0:] = rr[slab_row0:] + R[base + slab_row0:base + r, :K]
    o = np.arange(r) if row_index is None else np.asarray(row_index, dtype=np.int64)
    with np.errstate(all='ignore'):
        out = Z.copy()
        out[o] = (F.astype(dtype) * rr.astype(dtype) + Z[o].astype(dtype)).astype(np.float32)
    return out


def expectations_ref(a1, a2):
    """E, psi, lg, Elog_ref (float64) of a shape / rate pair."""
    a1 = np.asarray(a1, dtype=np.float64)
    a2 = np.asarray(a2, dtype=np.float64)
    with np.errstate(all='ignore'):
        E = a1 / a2
        psi = scipy.special.digamma(a1.astype(np.float32).astype(np.float64))
        lg = np.log(a2.astype(np.float32).astype(np.float64))
        elog = psi - lg
    return E, psi, lg, elog


def colsum_ref(x):
    """math.fsum of every column (NaN where the column holds one; fsum raises on inf - inf, which is NaN too)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty(x.shape[1])
    for k in range(x.shape[1]):
        col = x[:, k]
        if np.isfinite(col).all():
            out[k] = math.fsum(col.tolist())
        else:
            with np.errstate(all='ignore'):
                out[k] = np.sum(col)
    return out


def gamma_update_ref(prior1=None, prior2=None, Z=None, zmul=None, rate_vec=None, rate_mat=None, rmul=None, a1=None, a2=None,
                     F=None, R=None, nslab=1, slab_row0=0, row_index=None):
    """One call of oriana_gamma_update(_prep) / oriana_gamma_update_finalize(_prep) in any of its forms; see the module text.
    finalize: F is not None (Z is then the matrix the step completes); stored pair: Z is None (a1, a2 given)."""
    out = {}
    if Z is None:
        s1 = np.array(a1, dtype=np.float64)
        s2 = np.array(a2, dtype=np.float64)
        out['Z_out'] = None
    else:
        Z = np.asarray(Z, dtype=np.float32)
        K = Z.shape[1]
        if F is not None:
            z = finalize_ref(Z, F, R, K, nslab, slab_row0, row_index)
            out['Z_out'] = z
        else:
            z = Z
            out['Z_out'] = Z.copy()
            if zmul is not None:
                with np.errstate(all='ignore'):
                    z = np.asarray(zmul, dtype=np.float32) * Z                  # float32 product, as S_hat * Z_hat_j
        if rate_mat is not None and F is None:
            rate = np.asarray(rate_mat, dtype=np.float64)
            if rmul is not None:
                rate = np.asarray(rmul, dtype=np.float32).astype(np.float64) * rate
        else:
            rate = np.broadcast_to(np.asarray(rate_vec, dtype=np.float64)[None, :], Z.shape)
        with np.errstate(all='ignore'):
            s1 = clamp(np.asarray(prior1, dtype=np.float64)[None, :] + z.astype(np.float64))
            s2 = clamp(np.asarray(prior2, dtype=np.float64)[None, :] + rate)
    E, psi, lg, elog = expectations_ref(s1, s2)
    out.update(a1=s1, a2=s2, E=E, psi=psi, lg=lg, Elog_ref=elog, sum_E=colsum_ref(E))
    return out


def elog_bound(psi, lg, elog):
    """The largest |Elog - Elog_ref| of a faithful kernel, element by element (module text); inf where the reference is."""
    with np.errstate(all='ignore'):
        return (U32 * np.abs(psi) + LOGF_ULPS * 2.0 * U32 * np.abs(lg) + U32 * np.abs(elog) + DIGAMMA_ABS + 2.0 ** -149)


def elog_ratio(got, ref):
    """|got - Elog_ref| / bound per element; inf where a non-finite reference value is not matched in place (or a
    finite one is answered by a non-finite value)."""
    got = np.asarray(got, dtype=np.float64)
    want = ref['Elog_ref']
    fin = np.isfinite(want)
    with np.errstate(all='ignore'):
        ratio = np.abs(got - want) / elog_bound(ref['psi'], ref['lg'], want)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    ratio = np.where(fin, np.where(np.isfinite(got), ratio, np.inf), np.where(same, 0.0, np.inf))
    return ratio


def colsum_tol(start, x):
    """Bound on |content - fsum(start, x_1 .. x_r)| of a column sum the kernel ADDS into `start`: the r + 1 terms are
    joined by r float64 additions in an order the launch decides (threads, shuffles, LDS, one atomic per work-group), so
    the error is at most gamma_r * (|start| + sum |x|) with gamma_r = r 2^-53 / (1 - r 2^-53) (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2), plus the rounding of the reference itself.  For start = 0 this is the
    (r - 1) 2^-53 sum |x| of an r-term sum; with a start value there is one addition more, and a single row (r = 1) is not
    exact any more."""
    x = np.asarray(x, dtype=np.float64)
    r = x.shape[0]
    with np.errstate(all='ignore'):                      # (a plain sum: its own error is of second order in the bound)
        mag = np.abs(np.asarray(start, dtype=np.float64)) + np.abs(x).sum(axis=0)
    g = r * U64 / (1.0 - r * U64)
    return (g + U64) * mag


def colsum_total(start, x):
    """fsum(start, x_1 .. x_r) per column."""
    x = np.asarray(x, dtype=np.float64)
    return colsum_ref(np.vstack([np.asarray(start, dtype=np.float64)[None, :], x]))


# ---- PREP outputs (k_gamma_update_vec, FUn != NULL: the arithmetic of factor_prep_row / k_row_stats) ------------------
STAT_MAX = 200.0


def prep_ref(elog_f32):
    """From the stored float32 E[log .] in PACKED row order: mu (row maximum, NaN for a row with a NaN), FU =
    exp(f64(el) - f64(max)) in float64 (the maximum taken over the values that are not NaN) and the statistics of the
    maxima over all rows: count and float64 sum / sum of squares over |max| <= 200, minimum over the rows without NaN."""
    el = np.asarray(elog_f32, dtype=np.float32)
    bad = np.isnan(el).any(axis=1)
    with np.errstate(all='ignore'):
        mx = np.fmax.reduce(el, axis=1)
        fu = np.exp(el.astype(np.float64) - mx.astype(np.float64)[:, None])
    mu = np.where(bad, np.float32(np.nan), mx).astype(np.float32)
    ok = ~bad
    inside = ok & (np.abs(mx) <= STAT_MAX)
    m64 = mx[inside].astype(np.float64)
    stats = dict(count=int(inside.sum()), min=(np.float32(mx[ok].min()) if ok.any() else np.float32(np.inf)),
                 sum=math.fsum(m64.tolist()), sumsq=math.fsum((m64 * m64).tolist()),
                 sum_abs=math.fsum(np.abs(m64).tolist()))
    return mu, fu, stats


# ---- M-step ------------------------------------------------------------------------------------------------------------
def mstep_ref(p1, p2, sumE, sumL, count):
    """gap.py:117-129 from the column sums: the mean of the float32 E[log .] is a float32 (np.mean over a float32
    matrix), the starting value and the five Newton steps are oracle.cavi_oracle.inverse_digamma (utils.py:39-51).
    p1 is not read (the M-step overwrites it); it is an argument because the kernels take the pair."""
    from oracle.cavi_oracle import inverse_digamma
    p2 = np.asarray(p2, dtype=np.float64)
    with np.errstate(all='ignore'):
        mean_log = (np.asarray(sumL, dtype=np.float64) / count).astype(np.float32)
        y = np.log(p2) + mean_log.astype(np.float64)
        n1 = clamp(inverse_digamma(y))
        n2 = clamp(n1 / (np.asarray(sumE, dtype=np.float64) / count))
    return n1, n2


# ---- exact inputs ------------------------------------------------------------------------------------------------------
def dyadic_plain(rng, r, K):
    """prior1, prior2, rate_vec (arbitrary doubles) and a dyadic Z with exact zeros in it."""
    Z = (rng.integers(0, 1 << 12, size=(r, K)) / 256.0).astype(np.float32)
    Z[rng.random((r, K)) < 0.1] = 0.0
    return dict(prior1=rng.random(K) + 0.5, prior2=rng.random(K) + 0.5, rate_vec=rng.random(K) * 50.0, Z=Z)


def dyadic_zi(rng, r, K):
    """zmul, rate_mat and rmul of the ZI forms (module text)."""
    return dict(zmul=(rng.integers(0, 257, size=(r, K)) / 256.0).astype(np.float32),
                rate_mat=rng.integers(0, 1 << 16, size=(r, K)) / 1024.0,
                rmul=(rng.integers(0, 257, size=(r, K)) / 256.0).astype(np.float32))


def dyadic_finalize(rng, r, K, Kp, nslab, slab_row0, extra_rows=0):
    """F (r, Kp), R (slab_rows + extra_rows, Kp) and a permutation; the padding columns K..Kp hold values too (a kernel
    that read them would show)."""
    F = (rng.integers(1, 256, size=(r, Kp)) / 256.0).astype(np.float32)
    R = rng.integers(0, 64, size=(slab_rows(r, nslab, slab_row0) + extra_rows, Kp)).astype(np.float32)
    return dict(F=F, R=R, row_index=rng.permutation(r).astype(np.int32))


def ladder_pair(r, K):
    """The stored-pair case: every a1 of A1_LADDER against every a2 of A2_LADDER, repeated over the matrix."""
    i = np.arange(r * K)
    a1 = np.array(A1_LADDER)[i % len(A1_LADDER)].reshape(r, K)
    a2 = np.array(A2_LADDER)[(i // len(A1_LADDER)) % len(A2_LADDER)].reshape(r, K)
    return a1, a2


def specials_plain(rng, r, K):
    """The specials case: NaN, +-inf, a huge and a negative Z, an infinite rate."""
    d = dyadic_plain(rng, r, K)
    Z = d['Z']
    Z[0, 0] = np.nan
    Z[1, 1 % K] = np.inf
    Z[2, 2 % K] = -np.inf
    Z[3, 3 % K] = 3e38
    Z[4, 0] = -5.0
    Z[5 % r, K - 1] = np.inf                    # the column of the infinite rate: inf - inf
    d['rate_vec'][K - 1] = np.inf
    return d


# ---- the launch rule -----------------------------------------------------------------------------------------------------
# Restates, from csrc/updates.hip: gu_vec_cfg (VEC and LPR of a K), gu_small (below 2^20 elements the element-per-lane kernel
# unless PREP outputs are asked for), gu_large_groups (512 / 1024-thread groups for 4096 < r <= 32768), pick_block (KT),
# rows_per_block / gu_vec_rpb (the number of work-groups, hence of upart blocks), and oriana_kpad of csrc/passes.hip.
def kpad(K):
    if K <= 0:
        return 0
    for t in range(1, 8):
        if K <= 16 * t:
            return 16 * t
        if t <= 6 and K <= 16 * t + 4:
            return 16 * t + 4
    for kp in (128, 160, 192, 224, 256):
        if K <= kp:
            return kp
    return 0


def vec_cfg(K, wide_ok):
    if wide_ok and K % 4 == 0 and K <= 256:
        v = 4
    elif wide_ok and K % 2 == 0 and K <= 128:
        v = 2
    elif K <= 64:
        v = 1
    else:
        return None
    lpr = 8
    while lpr * v < K:
        lpr *= 2
    return v, lpr


def rows_per_block(r, ry):
    rpb = (r + 2047) // 2048
    rpb = (rpb + ry - 1) // ry * ry
    return min(max(rpb, 4 * ry), 512)


def prep_blocks(r, K):
    """oriana_gamma_update_prep_blocks"""
    cfg = vec_cfg(K, True)
    if r <= 0 or K <= 0 or cfg is None:
        return 0
    rpb = rows_per_block(r, 4 * (64 // cfg[1]))
    return (r + rpb - 1) // rpb


def instantiation(entry, r, K, aligned=True, prep=False):
    """The kernel a call reaches: ('vec', FIN, VEC, LPR) or ('scalar', FIN, NT, KT, rounds); None where the entry refuses
    (PREP outputs without a vector configuration, or with one narrowed by unaligned pointers).  entry: 'plain' | 'fin'."""
    fin = entry == 'fin'
    cfg = vec_cfg(K, aligned)
    if prep and (cfg is None or cfg != vec_cfg(K, True)):
        return None
    if (prep or r * K >= 1 << 20) and cfg is not None:
        return ('vec', fin, cfg[0], cfg[1])
    big = 4096 < r <= 32768
    nt = (1024 if fin else 512) if big else 256
    kt = 1
    while kt < K and kt < 128:
        kt *= 2
    return ('scalar', fin, nt, kt, (K + kt - 1) // kt)


def lazy_runs(r, K, aligned=True, prep=False):
    """Does oriana_gamma_update_finalize_lazy run (False: ORIANA_EKRANGE)?  Not below 2^20 elements without PREP outputs,
    and not without a vector configuration (odd K above 64, unaligned pointers at a K above 64)."""
    if kpad(K) == 0 or r == 0 or (not prep and r * K < 1 << 20):
        return False
    cfg = vec_cfg(K, aligned)
    return cfg is not None and not (prep and cfg != vec_cfg(K, True))


# ---- the cases -----------------------------------------------------------------------------------------------------------
# (entry, form, r, K, aligned, prep); form: 'plain' | 'zi_zr' (zmul + rate_mat) | 'zi_rr' (rate_mat + rmul) | 'zi_all' |
# 'stored' | 'specials' for entry 'plain', (nslab, slab_row0) for entry 'fin'.  A finalize form needs oriana_kpad(K) != 0,
# i.e. K <= 256: the three- and four-round shapes of the element-per-lane kernel exist in the plain form only.
# What reaches what (test_gamma_update_host.py holds the table to the launch switches):
#   k_gamma_update<plain, 256>   SCALAR_256                         <FIN, 256>   the same up to K = 256
#   k_gamma_update<plain, 512>   SCALAR_BIG, ODD_WIDE, (10486, 100) unaligned     <FIN, 1024>  the same
#   k_gamma_update_vec<., VEC, LPR>, plain and FIN: VEC_K[VEC] x PREP_R with PREP outputs -- LPR 8, 8, 16, 16, 32, 32, 64(, 64)
#   along each list -- and without them VEC_LARGE (<4, 32>, <4, 64>, <1, 64>) and (16384, 64) unaligned (<1, 64>)
SCALAR_256 = [(1, 1), (37, 5), (300, 20), (129, 64), (257, 101), (50, 200), (70, 257), (33, 512), (32769, 3)]
SCALAR_BIG = [(4097, 3), (5000, 20), (4100, 127), (4200, 200)]
VEC_K = {4: [4, 20, 36, 64, 100, 128, 256], 2: [2, 6, 18, 30, 50, 62, 66, 126], 1: [1, 7, 9, 15, 17, 31, 33, 63]}
PREP_R = [1, 3, 63, 515]
VEC_LARGE = [(8192, 128), (4097, 256), (16645, 63)]
UNALIGNED = [(16384, 64), (10486, 100)]          # narrows to VEC 1; no vector configuration: the element-per-lane kernel
ODD_WIDE = [(8257, 127)]                         # 2^20 elements at an odd K above 64: no vector configuration either


def _fin_forms(r):
    return list(dict.fromkeys([(1, 0), (3, 0), (1, r // 2), (3, r // 2)]))        # (r = 1: slab_row0 = 0 twice)


def _cases():
    out = []
    for r, K in SCALAR_256 + SCALAR_BIG:
        out.append(('plain', 'plain', r, K, True, False))
        if kpad(K):
            out += [('fin', f, r, K, True, False) for f in _fin_forms(r)]
    for vec in (4, 2, 1):
        for K in VEC_K[vec]:
            for r in PREP_R:
                out.append(('plain', 'plain', r, K, True, True))
                # every (nslab, slab_row0) at the longest matrix, the form with everything in it at the short ones
                out += [('fin', f, r, K, True, True) for f in (_fin_forms(r) if r == PREP_R[-1] else [(3, r // 2)])]
    for r, K in VEC_LARGE:
        out.append(('plain', 'plain', r, K, True, False))
        out += [('fin', f, r, K, True, False) for f in _fin_forms(r)]
    for r, K in ODD_WIDE:
        out += [('plain', 'plain', r, K, True, False), ('fin', (3, r // 2), r, K, True, False)]
    for r, K in UNALIGNED:
        out.append(('plain', 'plain', r, K, False, False))
        out.append(('fin', (3, r // 2), r, K, False, False))
    # the ZI operands and the stored pair: once per kernel family and VEC
    for r, K, prep in [(300, 20, False), (5000, 20, False), (515, 100, True), (515, 50, True), (515, 33, True)]:
        out += [('plain', form, r, K, True, prep) for form in ('zi_zr', 'zi_rr', 'zi_all', 'stored')]
    out.append(('plain', 'specials', 37, 5, True, False))
    return out


CASES = _cases()


def case_id(case):
    entry, form, r, K, aligned, prep = case
    f = form if isinstance(form, str) else 's%d_from%d' % form
    return '%s-%s-%dx%d%s%s' % (entry, f, r, K, '' if aligned else '-unaligned', '-prep' if prep else '')


def case_inputs(case):
    """The host-side inputs of a case (NumPy), deterministic in the case: the keyword arguments of gamma_update_ref plus Kp."""
    entry, form, r, K, aligned, prep = case
    rng = np.random.default_rng([r, K, int(prep), sum(map(ord, case_id(case)))])
    Kp = kpad(K)
    if form == 'stored':
        a1, a2 = ladder_pair(r, K)
        if prep:
            a1 = a1.copy()
            a1[min(5, r - 1), K // 2] = np.nan         # a row with a NaN: mu_out is NaN, the row stays out of the statistics
            a1[r - 1, :] = 1e-15                        # a row at the clamp: its maximum (-1e15) enters the minimum alone
        return dict(a1=a1, a2=a2), Kp
    d = specials_plain(rng, r, K) if form == 'specials' else dyadic_plain(rng, r, K)
    if entry == 'fin':
        nslab, row0 = form
        d.update(dyadic_finalize(rng, r, K, Kp, nslab, row0), nslab=nslab, slab_row0=row0)
    elif form.startswith('zi'):
        zi = dyadic_zi(rng, r, K)
        d['rate_mat'] = zi['rate_mat']
        del d['rate_vec']                              # (the rate is the matrix: the entry takes either)
        if form in ('zi_zr', 'zi_all'):
            d['zmul'] = zi['zmul']
        if form in ('zi_rr', 'zi_all'):
            d['rmul'] = zi['rmul']
    return d, Kp
