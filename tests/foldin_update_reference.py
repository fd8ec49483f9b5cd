# -*- coding: utf-8 -*-
"""A plain float64 statement of ONE call of oriana_foldin_update / oriana_foldin_update_zi (csrc/updates.hip:
k_foldin_update<VEC, LPR, NC, ZI>, the launch between two row passes of every fold-in), the bounds its float32 outputs have to
keep, inputs on which everything else is exact, a restatement of the launch rule and the table of cases that reaches every
instantiation of it.  NumPy / SciPy only: no torch, no GPU.  Built on gamma_update_reference (the clamp, the finalize step,
the expectations and their bound, the dyadic inputs, the launch rule of gu_vec_cfg).  Used by test_foldin_update_host.py and
test_foldin_update_gpu.py.

What one call computes.  Rows are walked in PACKED order p; o = row_index[p] (o = p without an index) is the caller's row.
a1, a2, U_hat, Elog, active and froze_at are in the caller's order, F, R, FUn and mu in packed order.

  START (R is None)   a1 is taken as given (ZI: a2 too, and U_hat = a1 / a2 is written).  Every row with active[o] != 0 is
                      written; there is no freeze test; froze_at and *n_active are not touched.
  STEP                z      = f32(F[p] * sum_s R_s[p] + Z[o])          gamma_update_reference.finalize_ref
                      a1_new = clamp(alpha1 + f64(z))
                      a2_new = clamp(alpha2 + rate[o])                  ZI only; the plain kernel's rate is a2_row[K]
                      moved  = some k has not (|a1_new - a1| <= tol * a1)      ZI: or the same test on a2
                      active and not moved: active[o] = 0, froze_at[o] = it -- nothing else of the row changes
                      active and moved    : the row is WRITTEN (below)
                      active[o] == 0 on entry: nothing is written
  a WRITTEN row       a1[o] = a1_new (ZI: a2[o] = a2_new, U_hat[o] = a1_new / a2_new), Elog[o] = E[log U] minus its row
                      maximum, where E[log U] = f32(psi(f64(f32 a1_new))) - logf(f32 a2) (a row that holds a NaN is stored
                      as it is), FUn[p, :K] = exp(Elog as stored) (a NaN row: exp(E[log U] - its maximum over the values
                      that are not NaN, as gamma_update_reference.prep_ref), mu[p] = 0 (NaN for a NaN row).
  upart[4 b ..]       sum, sum of squares, count (the three over |mu| <= STAT_MAX) and minimum of mu[p] over the rows of
                      work-group b -- rows_per_block(r, 32) rows each -- a written row with its new mu, every other row
                      with the mu the buffer held; NaN rows enter none of the four.
  *n_active           STEP: += the number of rows written.

THE BOUNDS.  None is measured on the kernel.

Exact outputs.  With the dyadic inputs of gamma_update_reference every float32 operation of the finalize step is exact;
a1_new and a2_new are one IEEE float64 addition and a clamp each; the freeze predicate is a float64 subtraction, a float64
product and a comparison, none of which can be contracted into another.  So a1, a2, active, froze_at, the increment of
*n_active and the SET of rows written are compared bit for bit, for any float64 pair the buffers hold on entry.  U_hat is one
float64 division: within one float64 ulp (as E in test_gamma_update_gpu.py).  mu is 0 or NaN: bit for bit.

Stored E[log U]  (stored_bound).  Let e_k be the float64 reference of the unshifted value, b_k = elog_bound of it and el_k
the kernel's float32: |el_k - e_k| <= b_k.  The kernel stores f32(el_k - mx), mx = max_k el_k (exact: a maximum rounds
nothing), the reference e_k - M, M = max_k e_k.  |mx - M| <= D := the largest b_k among the factors that CAN be the maximum
of a faithful evaluation, i.e. those with e_k + b_k >= max_j (e_j - b_j): the kernel's maximum is attained at such a factor,
where it is within b_k of e_k <= M, and it is no smaller than el at the reference's own arg max, which is such a factor too.
The subtraction rounds once, by at most 2^-24 of its result (a difference of two floats below the normal range is exact):
    |stored - (e_k - M)| <= (b_k + D) (1 + 2^-24) + 2^-24 |e_k - M|
element by element.  Every written row without a NaN has maximum exactly 0.0f (el_k - mx at the arg max).

FUn against exp of the Elog the kernel itself stored (fun_bound).  The kernel forms f32(exp(f64(el) - f64(mx))) -- the
unrounded difference x -- while Elog holds S = f32(x), |x - S| <= 2^-24 |S|: exp(x) = exp(S) (1 + d), |d| <= expm1(2^-24 |S|)
(= 2^-24 |S| plus a second-order term below 2^-35 wherever exp(S) is a normal float32, written out rather than dropped).  The
float64 exp sits far below anything a float32 result can show (2^-40 relative allowed); the result is rounded to float32 once
(2^-24 relative, or half a subnormal step: 2^-149 absolute covers it):
    |FUn - exp(S)| <= exp(S) ((1 + 2^-24) (1 + expm1(2^-24 |S|) + 2^-40) - 1) + 2^-149
A NaN row is stored unshifted, so there x = f64(S_k) - f64(max S) is the kernel's own operand and the shift term is absent.

upart.  The mu seeds are multiples of 1/8 of magnitude at most 4 (and one -256, beyond STAT_MAX, and one NaN): a sum over the
at most 512 rows of a work-group is a multiple of 1/8 below 2^11, a sum of squares a multiple of 1/64 below 2^13 -- both
exact in float32 in any order.  Compared bit for bit.
"""
import numpy as np

import gamma_update_reference as gr

U32, U64 = gr.U32, gr.U64
SENTINEL = -7777.25           # what every buffer holds where the entry is not to write (exact in float32)
N_ACTIVE0 = 7                 # *n_active before the call: the kernel ADDS
IT = 5
TOL = 2.0 ** -6               # dyadic: tol * a1 is exact, and the tie pair below meets the predicate with equality


# ---- the launch rule (foldin_rpb, oriana_foldin_update_blocks, foldin_launch / foldin_launch_lpr) -----------------------------
def foldin_rpb(r):
    return gr.rows_per_block(r, 32)


def blocks(r):
    """oriana_foldin_update_blocks"""
    if r <= 0:
        return 0
    rpb = foldin_rpb(r)
    return (r + rpb - 1) // rpb


def instantiation(zi, K, aligned=True):
    """(VEC, LPR, NC) of the k_foldin_update<VEC, LPR, NC, ZI> a call reaches."""
    cfg = gr.vec_cfg(K, aligned)
    return (1, 64, 4) if cfg is None else (cfg[0], cfg[1], 1)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def same(got, want):
    """bit for bit, a NaN matching a NaN"""
    return np.array_equal(got, want, equal_nan=True)


def moved_ref(new, old, tol):
    """not (|new - old| <= tol * old), element by element (a NaN moves)"""
    with np.errstate(all='ignore'):
        return ~(np.abs(new - old) <= tol * old)


def upart_ref(mu, r):
    """(blocks(r), 4) float32 from the mu of every packed row (module text)."""
    rpb, nb = foldin_rpb(r), blocks(r)
    m = np.full(nb * rpb, np.nan)
    m[:r] = np.asarray(mu, dtype=np.float32).astype(np.float64)
    m = m.reshape(nb, rpb)
    ok = ~np.isnan(m)
    with np.errstate(all='ignore'):
        inside = ok & (np.abs(m) <= gr.STAT_MAX)
    mi = np.where(inside, m, 0.0)
    out = np.stack([mi.sum(axis=1), (mi * mi).sum(axis=1), inside.sum(axis=1).astype(np.float64),
                    np.where(ok, m, np.inf).min(axis=1)], axis=1)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)          # (the seeds keep every sum exact)
    return out.astype(np.float32)


def stored_bound(psi, lg, elog, stored, nanrow):
    """The largest |Elog as stored - its float64 reference| of a faithful kernel, element by element (module text)."""
    b = gr.elog_bound(psi, lg, elog)
    with np.errstate(all='ignore'):
        low = np.fmax.reduce(elog - b, axis=1)
        cand = (elog + b) >= low[:, None]
        D = np.max(np.where(cand, b, 0.0), axis=1)
        shifted = (b + D[:, None]) * (1.0 + U32) + U32 * np.abs(stored)
    return np.where(nanrow[:, None], b, shifted)


def foldin_ref(c, before):
    """One call on the inputs `c` and the buffer contents `before` (case_inputs): everything the entry may write.  Full
    arrays of what is exact (a1, a2, active, froze_at, n_active, mu, upart), and per packed row the masks `write` / `freeze`,
    o = `orow`, and the float64 references of the rest: E (U_hat), psi, lg, Elog_ref (unshifted), stored, stored_bound."""
    zi, K, r, start, tol = c['zi'], c['K'], c['r'], c['start'], c['tol']
    o = np.arange(r) if c['row_index'] is None else np.asarray(c['row_index'], dtype=np.int64)
    was = before['active'][o] != 0
    old1 = before['a1'][o]
    if start:
        n1, moved = old1, np.ones(r, dtype=bool)
        n2 = before['a2'][o] if zi else None
    else:
        z = gr.finalize_ref(c['Z'], c['F'], c['R'], K, c['nslab'], c['slab_row0'], c['row_index'])[o]
        with np.errstate(all='ignore'):
            n1 = gr.clamp(c['alpha1'][None, :] + z.astype(np.float64))
        moved = moved_ref(n1, old1, tol).any(axis=1)
        n2 = None
        if zi:
            with np.errstate(all='ignore'):
                n2 = gr.clamp(c['alpha2'][None, :] + c['rate'][o])
            moved = moved | moved_ref(n2, before['a2'][o], tol).any(axis=1)
    if not zi:
        n2 = np.broadcast_to(np.asarray(c['a2_row'], dtype=np.float64)[None, :], (r, K))
    write, freeze = was & moved, was & ~moved
    E, psi, lg, elog = gr.expectations_ref(n1, n2)
    nanrow = np.isnan(elog).any(axis=1)
    with np.errstate(all='ignore'):
        M = np.fmax.reduce(elog, axis=1)
        stored = np.where(nanrow[:, None], elog, elog - M[:, None])
    out = dict(orow=o, write=write, freeze=freeze, nanrow=nanrow, E=E, psi=psi, lg=lg, Elog_ref=elog, stored=stored,
               stored_bound=stored_bound(psi, lg, elog, stored, nanrow))
    a1 = before['a1'].copy()
    a2 = before['a2'].copy() if zi else None
    active, froze_at = before['active'].copy(), before['froze_at'].copy()
    if not start:
        a1[o[write]] = n1[write]
        if zi:
            a2[o[write]] = n2[write]
        active[o[freeze]] = 0
        froze_at[o[freeze]] = c['it']
    mu = before['mu'].copy()
    mu[write] = np.where(nanrow[write], np.float32(np.nan), np.float32(0.0))
    out.update(a1=a1, a2=a2, active=active, froze_at=froze_at, mu=mu, upart=upart_ref(mu, r),
               n_active=int(before['n_active']) + (0 if start else int(write.sum())))
    return out


# ---- the comparison (what test_foldin_update_gpu.py asserts of the device's buffers, and test_foldin_update_host.py of wrong
# restatements) ---------------------------------------------------------------------------------------------------------------------
def ratio_to(got, want, bound):
    """|got - want| / bound per element; inf where a non-finite reference value is not matched in place (or a finite one is
    answered by a non-finite value)."""
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(want)
    with np.errstate(all='ignore'):
        ratio = np.abs(got - want) / bound
    hit = (got == want) | (np.isnan(got) & np.isnan(want))
    return np.where(fin, np.where(np.isfinite(got), ratio, np.inf), np.where(hit, 0.0, np.inf))


def fun_bound(S, nanrow):
    """(exp(S), bound) of FUn for the stored Elog S (float64 of the kernel's float32; a NaN row already minus its maximum)."""
    with np.errstate(all='ignore'):
        want = np.exp(S)
        d = np.where(nanrow[:, None], 0.0, np.expm1(U32 * np.minimum(np.abs(S), 1e3)))
        rel = (1.0 + U32) * (1.0 + d + 2.0 ** -40) - 1.0
        return want, want * rel + 2.0 ** -149


def check(c, before, ref, got):
    """Every assertion of the module text on the buffers `got` of one call.  Returns the largest bound ratios."""
    zi, K, r = c['zi'], c['K'], c['r']
    o, write = ref['orow'], ref['write']
    wo = o[write]
    keep = np.ones(r, dtype=bool)
    keep[wo] = False                                      # the caller's rows that are not written
    out = {}
    # exact: the pair, the flags, the counter -- and with them the set of rows written, and that no other row's pair changes
    assert same(got['a1'], ref['a1']), 'a1'
    if zi:
        assert same(got['a2'], ref['a2']), 'a2'
    assert np.array_equal(got['active'], ref['active']), 'active'
    assert np.array_equal(got['froze_at'], ref['froze_at']), 'froze_at'
    assert int(got['n_active']) == ref['n_active'], ('n_active', int(got['n_active']), ref['n_active'])
    # U_hat: one float64 division
    if zi:
        assert same(got['U_hat'][keep], before['U_hat'][keep]), 'U_hat of a row that is not written'
        g, want = got['U_hat'][wo], ref['E'][write]
        fin = np.isfinite(want)
        assert same(g[~fin], want[~fin]), 'U_hat'
        out['U_hat'] = float((np.abs(g[fin] - want[fin]) / np.spacing(np.abs(want[fin]))).max()) if fin.any() else 0.0
        assert out['U_hat'] <= 1.0, ('U_hat', out['U_hat'])
    # the stored E[log U]
    El = got['Elog']
    assert El.dtype == np.float32 and same(El[keep], before['Elog'][keep]), 'Elog of a row that is not written'
    ratio = ratio_to(El[wo], ref['stored'][write], ref['stored_bound'][write])
    out['Elog'] = float(ratio.max()) if ratio.size else 0.0
    assert out['Elog'] <= 1.0, ('Elog', out['Elog'], np.unravel_index(int(ratio.argmax()), ratio.shape))
    nanrow = ref['nanrow'][write]
    with np.errstate(all='ignore'):
        assert (El[wo][~nanrow].max(axis=1) == 0.0).all(), 'the maximum of a written row is not 0'
    # FUn: rows that are not written and the padding columns as they were; the rest exp of what Elog holds
    FU = got['FUn']
    assert FU.dtype == np.float32 and same(FU[~write], before['FUn'][~write]), 'FUn of a row that is not written'
    assert same(FU[write][:, K:], before['FUn'][write][:, K:]), 'padding columns of FUn'
    S = El[wo].astype(np.float64)
    with np.errstate(all='ignore'):
        S = np.where(nanrow[:, None], S - np.fmax.reduce(S, axis=1, initial=-np.inf)[:, None], S)
    want, bound = fun_bound(S, nanrow)
    ratio = ratio_to(FU[write][:, :K], want, bound)
    out['FUn'] = float(ratio.max()) if ratio.size else 0.0
    assert out['FUn'] <= 1.0, ('FUn', out['FUn'], np.unravel_index(int(ratio.argmax()), ratio.shape))
    # mu and the partial statistics
    assert same(got['mu'], ref['mu']), 'mu'
    assert got['upart'].dtype == np.float32 and same(got['upart'], ref['upart']), 'upart'
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# (zi, form, r, K, aligned, indexed); form: 'start' | (nslab, slab_row0).  Per ZI and K: the start form at r = 3 and 515, the
# form with everything in it at the short r, every (nslab, slab_row0) at r = 515.  FUn is the buffer F points to (as heldout
# calls the entries) in the one-slab forms and at r = 1, 63 and the long r, a buffer of its own in the others (aliased).
# What reaches what (test_foldin_update_host.py holds the table to the launch switches): K_VEC walks LPR 8, 8, 16, 16, 32, 32,
# 64(, 64) along each VEC; 101, 127, 255 take <1, 64, 4>; unaligned, K = 100 falls to <1, 64, 4> and K = 64 narrows to <1, 64>.
K_ODD_WIDE = [101, 127, 255]
K_ALL = gr.VEC_K[4] + gr.VEC_K[2] + gr.VEC_K[1] + K_ODD_WIDE
K_UNALIGNED = [100, 64]
R_MID = (2048 * 129 + 5, 6)          # rows_per_block strictly between its floor and its cap: 160 rows per work-group
R_CAP = (2048 * 512 + 77, 4)         # the cap of 512 rows, more than 2048 work-groups
R_LONG = gr.PREP_R[-1]


def _cases():
    out = []
    h = R_LONG // 2
    for zi in (False, True):
        for K in K_ALL:
            out += [(zi, 'start', 3, K, True, False), (zi, 'start', R_LONG, K, True, True)]
            out += [(zi, (3, r // 2), r, K, True, r != 1) for r in gr.PREP_R[:-1]]
            assert gr._fin_forms(R_LONG) == [(1, 0), (3, 0), (1, h), (3, h)]
            out += [(zi, (1, 0), R_LONG, K, True, False), (zi, (3, 0), R_LONG, K, True, True),
                    (zi, (1, h), R_LONG, K, True, True), (zi, (3, h), R_LONG, K, True, False)]
        for K in K_UNALIGNED:
            out += [(zi, 'start', R_LONG, K, False, True), (zi, (3, h), R_LONG, K, False, True), (zi, (1, 0), 63, K, False, False)]
        out.append((zi, (1, 0), R_CAP[0], R_CAP[1], True, True))
    out.append((False, (1, 0), R_MID[0], R_MID[1], True, False))
    return out


CASES = _cases()


def case_id(case):
    zi, form, r, K, aligned, indexed = case
    f = form if isinstance(form, str) else 's%d_from%d' % form
    return '%s-%s-%dx%d%s%s' % ('zi' if zi else 'plain', f, r, K, '' if aligned else '-unaligned', '-indexed' if indexed else '')


def aliased(case):
    """Is FUn the buffer F points to?"""
    zi, form, r, K, aligned, indexed = case
    return form != 'start' and (form[0] == 1 or r in (1, 63) or r > R_LONG)


# the row population of a step case, by packed row
GENERIC, INACTIVE, SAME, FIRST, LAST, A2ONLY, TIE_HOLD, TIE_FAIL, CLAMP = range(9)
POPULATION = {0: INACTIVE, 1: SAME, 2: FIRST, 3: LAST, 4: A2ONLY, 5: TIE_HOLD, 6: TIE_FAIL, 7: CLAMP, 8: INACTIVE}


def categories(r, zi):
    """GENERIC: an arbitrary old pair.  INACTIVE: active = 0 on entry.  SAME: the old pair is the new one in every factor (it
    freezes at tol = 0 too).  FIRST / LAST: only factor 0 / K - 1 of a1 moved.  A2ONLY (ZI): only one factor of a2 moved.
    TIE_HOLD / TIE_FAIL: factor K - 1 of the old a1 is the double at which |new - old| <= tol * old holds with EQUALITY, and
    the double below it, where it fails; every other factor holds.  LAST rows carry the row maximum of E[log U] in factor K - 1
    as well.  CLAMP: every new shape is 1e-15.  Neighbouring packed rows
    -- up to eight of them share a wave -- are of different kinds."""
    cat = np.full(r, GENERIC)
    if r >= 63:
        m = np.arange(r) % 16
        for k, v in POPULATION.items():
            cat[m == k] = v
        if not zi:
            cat[cat == A2ONLY] = GENERIC
    elif r == 3:
        cat[1], cat[2] = SAME, INACTIVE
    return cat


def _slab_rows_of(p, r, nslab, row0):
    """Rows of the packed R buffer that hold the packed rows p."""
    rows = [p]
    for s in range(1, nslab):
        q = p[p >= row0]
        rows.append(s * (r - row0) + q)
    return np.concatenate(rows)


def _seed_mu(rng, r, inactive_p):
    mu = (rng.integers(-32, 33, size=r) / 8.0).astype(np.float32)
    if inactive_p.size > 1:
        mu[inactive_p[0]] = np.nan              # a frozen NaN row: in none of the statistics
        mu[inactive_p[1]] = -256.0              # beyond STAT_MAX: in the minimum alone
    return mu


def case_inputs(case):
    """(c, before) of a case, deterministic in the case: the inputs of the call and what every buffer it may write holds."""
    zi, form, r, K, aligned, indexed = case
    start = form == 'start'
    Kp = gr.kpad(K)
    rng = np.random.default_rng([r, K, int(zi), int(indexed), sum(map(ord, case_id(case)))])
    perm = rng.permutation(r).astype(np.int32)
    c = dict(zi=zi, start=start, r=r, K=K, Kp=Kp, aligned=aligned, alias=aliased(case), nslab=1, slab_row0=0, tol=0.0, it=IT,
             alpha1=None, alpha2=None, a2_row=None, rate=None, Z=None, F=None, R=None, row_index=perm if indexed else None)
    o = perm.astype(np.int64) if indexed else np.arange(r)
    active = np.ones(r, dtype=np.uint8)
    froze_at = (1000 + np.arange(r)).astype(np.int32)
    a2 = None
    if start:
        a1, a2l = gr.ladder_pair(r, K)
        a1 = a1.copy()
        a1[r - 1, :] = 1e-15                             # a row at the clamp: every E[log U] is near -1e15, stored near 0
        if zi:
            a2 = a2l.copy()
            a2[min(5, r - 2), K // 2] = np.nan           # a NaN rate: a NaN row, mu = NaN, Elog stored unshifted
        else:
            c['a2_row'] = np.array(gr.A2_LADDER)[np.arange(K) % len(gr.A2_LADDER)]
        off = np.arange(r) % 4 == 2                      # rows that are inactive: not written
        off[[r - 1, min(5, r - 2)]] = False
        active[off] = 0
    else:
        nslab, row0 = form
        c.update(nslab=nslab, slab_row0=row0, tol=TOL if r >= 63 else 0.0)
        d = gr.dyadic_plain(rng, r, K)
        fin = gr.dyadic_finalize(rng, r, K, Kp, nslab, row0)
        alpha1, Z, F, R = d['prior1'], d['Z'], fin['F'], fin['R']
        j = int(rng.integers(2048, 6144))
        alpha1[K - 1] = 4095.0 * j / 2.0 ** 24           # = 65 * (63 j / 2^24), in [0.5, 1.5): the tie pair below is exact
        cat = categories(r, zi)
        tie = np.flatnonzero((cat == TIE_HOLD) | (cat == TIE_FAIL))
        clamp = np.flatnonzero(cat == CLAMP)
        R[_slab_rows_of(tie, r, nslab, row0), K - 1] = 0.0
        Z[o[tie], K - 1] = 0.0                           # a1_new[K - 1] = alpha1[K - 1] exactly
        R[_slab_rows_of(clamp, r, nslab, row0), :] = 0.0
        Z[o[clamp], :] = -16.0                           # alpha1 - 16 < 0: every shape clamps
        # LAST rows: factor K - 1 also holds the row MAXIMUM of E[log U] -- a1_new >= 62.75 + 15 there against a rate below 1.5
        # (psi - log >= 3.9), a1_new = alpha1 < 1.5 in every other factor (psi - log <= 0.04 + 0.7)
        last = np.flatnonzero(cat == LAST)
        rows = _slab_rows_of(last, r, nslab, row0)
        R[rows, :K - 1], R[rows, K - 1] = 0.0, 63.0
        F[last, K - 1] = 255.0 / 256.0
        Z[o[last], :K - 1], Z[o[last], K - 1] = 0.0, 15.0
        d['rate_vec'][K - 1] = 0.0
        c.update(alpha1=alpha1, Z=Z, F=F, R=R)
        n1 = gr.clamp(alpha1[None, :] + gr.finalize_ref(Z, F, R, K, nslab, row0, c['row_index'])[o].astype(np.float64))
        old1 = rng.gamma(2.0, 20.0, size=(r, K)) + 1e-3
        held = np.isin(cat, (SAME, FIRST, LAST, A2ONLY, TIE_HOLD, TIE_FAIL))
        old1[held] = n1[held]
        old1[cat == FIRST, 0] = 2.0 * n1[cat == FIRST, 0]
        old1[cat == LAST, K - 1] = 2.0 * n1[cat == LAST, K - 1]
        hold = n1[tie, K - 1] / 65.0 * 64.0
        assert (n1[tie, K - 1] == alpha1[K - 1]).all() and (n1[tie, K - 1] - hold == TOL * hold).all()
        fail = np.nextafter(hold, 0.0)
        assert not moved_ref(n1[tie, K - 1], hold, TOL).any() and moved_ref(n1[tie, K - 1], fail, TOL).all()
        old1[tie, K - 1] = np.where(cat[tie] == TIE_HOLD, hold, fail)
        old1[clamp] = 1.0
        assert (n1[clamp] == 1e-15).all()
        a1 = np.empty((r, K))
        a1[o] = old1
        if zi:
            c['alpha2'] = d['prior2']
            c['rate'] = gr.dyadic_zi(rng, r, K)['rate_mat']
            c['rate'][o[last], K - 1] = 0.0
            n2 = gr.clamp(c['alpha2'][None, :] + c['rate'][o])
            old2 = rng.gamma(2.0, 20.0, size=(r, K)) + 1e-3
            old2[held] = n2[held]
            only = np.flatnonzero(cat == A2ONLY)
            old2[only, (only // 16) % K] *= 2.0
            a2 = np.empty((r, K))
            a2[o] = old2
        else:
            c['a2_row'] = gr.clamp(d['prior2'] + d['rate_vec'])
        active[o[cat == INACTIVE]] = 0
    before = dict(a1=a1, a2=a2, U_hat=np.full((r, K), SENTINEL) if zi else None,
                  Elog=np.full((r, K), SENTINEL, dtype=np.float32),
                  FUn=c['F'].copy() if c['alias'] else np.full((r, Kp), SENTINEL, dtype=np.float32),
                  mu=_seed_mu(rng, r, np.flatnonzero(active[o] == 0)), upart=np.full((blocks(r), 4), SENTINEL, dtype=np.float32),
                  active=active, froze_at=froze_at, n_active=N_ACTIVE0)
    return c, before


def second_call(c, got):
    """(c, before) of a second call on the buffers the first one left: it + 1, the same R; Z moved by 64 in one factor of
    every third row (the finalize step stays exact: multiples of 2^-8 below 2^9).  A row the first call wrote and Z leaves alone
    meets its own a1 again and freezes; a moved one is written again and counted again.  The F buffer is given its first contents
    again where FUn is that buffer (the first call wrote FUn over it; the row pass that would have formed R from it is not part
    of the call)."""
    r, K = c['r'], c['K']
    Z = c['Z'].copy()
    rows = np.arange(0, r, 3)
    Z[rows, rows % K] += np.float32(64.0)
    before = {k: (None if v is None else np.array(v, copy=True)) for k, v in got.items()}
    before['n_active'] = int(got['n_active'])
    if c['alias']:
        before['FUn'] = c['F'].copy()
    return dict(c, Z=Z, it=c['it'] + 1), before
