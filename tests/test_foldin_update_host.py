# -*- coding: utf-8 -*-
"""The float64 reference of the fold-in update (tests/foldin_update_reference.py) checked on its own: that the case table
reaches every instantiation of foldin_launch / foldin_launch_lpr in every form, that blocks() is
oriana_foldin_update_blocks, that the dyadic inputs keep the finalize step exact, that a faithful float32 evaluation of the
kernel's arithmetic keeps every bound while eleven wrong restatements each fail the comparison the GPU test makes, that one
reference step is the model's map (transform_reference.T64, zi_foldin_reference.T64), and the argument errors of both
entries, which return before any launch.  No GPU."""
import ctypes

import numpy as np
import pytest
import scipy.special

import foldin_update_reference as fr
import gamma_update_reference as gr

EINVAL, EKRANGE = -1, -2

# Every instantiation the launch switches of csrc/updates.hip list, per ZI: foldin_launch_lpr<VEC, ZI> over LPR 8 .. 64 for
# VEC 4, 2, 1 (NC = 1), and the element instantiation <1, 64, 4> of foldin_launch.
INSTANTIATIONS = [(zi, vec, lpr, 1) for zi in (False, True) for vec in (4, 2, 1) for lpr in (8, 16, 32, 64)] + \
                 [(False, 1, 64, 4), (True, 1, 64, 4)]

SMALL = [c for c in fr.CASES if c[2] <= fr.R_LONG]


def _form(case):
    f = case[1]
    return f if isinstance(f, str) else (f[0], 'half' if f[1] else 0)


def test_the_cases_reach_every_instantiation():
    reached = {}
    for case in fr.CASES:
        zi, form, r, K, aligned, indexed = case
        assert gr.kpad(K) != 0, case
        reached.setdefault((zi,) + fr.instantiation(zi, K, aligned), []).append(case)
    assert set(reached) == set(INSTANTIATIONS) and len(set(INSTANTIATIONS)) == 26
    for inst in INSTANTIATIONS:
        cases = reached[inst]
        # r = 1 has no second half: its (3, 0) is not counted as a form of the long matrix
        forms = {_form(c) for c in cases if c[2] > 1}
        assert {'start', (1, 0), (3, 0), (1, 'half'), (3, 'half')} <= forms, inst
        steps = [c for c in cases if c[1] != 'start']
        assert {c[5] for c in steps} == {False, True}, inst
        assert {c[5] for c in cases if c[1] == 'start'} >= {True}, inst
        assert {fr.aliased(c) for c in steps} == {False, True}, inst
        full = [c for c in steps if c[2] >= 63]
        assert full and {c[5] for c in full} == {False, True}, inst
        for c in full:
            want = set(fr.POPULATION.values()) | {fr.GENERIC}
            assert set(fr.categories(c[2], c[0]).tolist()) == (want if c[0] else want - {fr.A2ONLY}), c
    # the table of the issue: K -> LPR, aligned; what the unaligned cases fall to
    for vec, lprs in ((4, [8, 8, 16, 16, 32, 32, 64]), (2, [8, 8, 16, 16, 32, 32, 64, 64]), (1, [8, 8, 16, 16, 32, 32, 64, 64])):
        assert [fr.instantiation(False, K) for K in gr.VEC_K[vec]] == [(vec, l, 1) for l in lprs]
    assert all(fr.instantiation(True, K) == (1, 64, 4) for K in fr.K_ODD_WIDE)
    assert fr.instantiation(False, 100) == (4, 32, 1) and fr.instantiation(False, 100, False) == (1, 64, 4)
    assert fr.instantiation(False, 64) == (4, 16, 1) and fr.instantiation(False, 64, False) == (1, 64, 1)
    # the rows per work-group: the floor, a value between, the cap with more than 2048 groups; five groups at r = 515
    assert fr.foldin_rpb(515) == 128 and fr.blocks(515) == 5 and 515 - 4 * 128 == 3
    assert fr.foldin_rpb(fr.R_MID[0]) == 160 and fr.foldin_rpb(fr.R_CAP[0]) == 512 and fr.blocks(fr.R_CAP[0]) > 2048
    assert {(c[2], c[3]) for c in fr.CASES if c[2] > fr.R_LONG} == {fr.R_MID, fr.R_CAP}
    assert {c[0] for c in fr.CASES if (c[2], c[3]) == fr.R_CAP} == {False, True}
    assert len(set(fr.CASES)) == len(fr.CASES)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from oriana_amd import _lib
    return _lib.load()


def test_blocks_is_the_entrys(lib):
    for r in (-1, 0, 1, 127, 128, 129, 515, 2048 * 129 + 5, 2048 * 512 + 77):
        assert fr.blocks(r) == int(lib.oriana_foldin_update_blocks(r)), r


@pytest.mark.parametrize('case', [c for c in SMALL if c[1] != 'start'], ids=fr.case_id)
def test_dyadic_inputs_make_the_finalize_step_exact(case):
    """Both calls of a case: float32 (a product, then a sum) and float64 (rounded once) are the same bits."""
    c, before = fr.case_inputs(case)
    for Z in (c['Z'], fr.second_call(c, before)[0]['Z']):
        args = (Z, c['F'], c['R'], c['K'], c['nslab'], c['slab_row0'], c['row_index'])
        z32, z64 = gr.finalize_ref(*args, dtype=np.float32), gr.finalize_ref(*args, dtype=np.float64)
        assert z32.dtype == np.float32 and np.array_equal(z32, z64)
        z = z64.astype(np.float64) * 256
        assert np.array_equal(z, np.round(z)) and float(np.abs(z64).max()) < 512
    assert c['F'].shape == (c['r'], c['Kp']) and c['R'].shape == (gr.slab_rows(c['r'], c['nslab'], c['slab_row0']), c['Kp'])


# ---- the kernel's arithmetic in NumPy float32 -----------------------------------------------------------------------------------
def _kernel_f32(c, before, wrong=(), log_ulp=0):
    """What a faithful kernel leaves in the buffers: the float64 pair and predicate as the kernel forms them, psi and the
    logarithm rounded to float32 (the logarithm moved by further ulps on request), subtracted, shifted and exponentiated as
    k_foldin_update does.  `wrong` names deliberate mistakes (test_the_comparison_rejects_wrong_restatements)."""
    zi, K, r, start, tol = c['zi'], c['K'], c['r'], c['start'], c['tol']
    W = set(wrong)
    o = np.arange(r) if c['row_index'] is None else np.asarray(c['row_index'], dtype=np.int64)
    got = {k: (None if v is None else np.array(v, copy=True)) for k, v in before.items()}
    was = before['active'][o] != 0
    old1 = before['a1'][o]
    n2 = before['a2'][o] if zi else np.broadcast_to(c['a2_row'][None, :], (r, K))
    if start:
        n1, moved = old1, np.ones(r, dtype=bool)
    else:
        nslab = c['nslab'] - (1 if 'last slab dropped' in W else 0)
        row0 = 0 if 'slab_row0 ignored' in W else c['slab_row0']
        R = c['R']
        if 'slab_row0 ignored' in W:                   # (every slab read as r whole rows: rows the buffer does not have)
            R = np.vstack([R, np.random.default_rng(1).integers(0, 64, size=(3 * r, c['Kp'])).astype(np.float32)])
        src = o if 'row_index on F and R' in W else np.arange(r)
        rr = R[src, :K].copy()
        for s in range(1, nslab):
            m = src >= row0
            rr[m] = rr[m] + R[s * (r - row0) + src[m], :K]
        z = c['F'][src, :K] * rr + c['Z'][o]
        assert z.dtype == np.float32
        n1 = gr.clamp(c['alpha1'][None, :] + z.astype(np.float64))

        def mv(new, old):
            d = np.abs(new - old)
            hold = (d < tol * old) if '< for <=' in W else (d <= tol * old)
            return (~hold)[:, :K - 1 if 'OR stops before the last factor' in W else K].any(axis=1)
        moved = mv(n1, old1)
        if zi:
            n2 = gr.clamp(c['alpha2'][None, :] + c['rate'][o])
            if 'ZI freezes on a1 alone' not in W:
                moved = moved | mv(n2, before['a2'][o])
    write, freeze = was & moved, was & ~moved
    with np.errstate(all='ignore'):
        psi = scipy.special.digamma(n1.astype(np.float32).astype(np.float64)).astype(np.float32)
        lg = np.log(n2.astype(np.float32).astype(np.float64)).astype(np.float32)
        for _ in range(log_ulp):
            lg = np.nextafter(lg, np.float32(np.inf))
        el = psi - lg
        assert el.dtype == np.float32
        bad = np.isnan(el).any(axis=1)
        mx = np.fmax.reduce(el[:, :K - 1] if 'shift over K - 1 factors' in W and K > 1 else el, axis=1)
        fu = np.exp(el.astype(np.float64) - mx.astype(np.float64)[:, None]).astype(np.float32)
        els = np.where(bad[:, None], el, el - mx[:, None])
        if 'shift omitted' in W:
            els = el
    if not start:
        got['a1'][o[write]] = n1[write]
        if 'frozen row written' in W:
            got['a1'][o[freeze]] = n1[freeze]
        if zi:
            got['a2'][o[write]] = n2[write]
        got['active'][o[freeze]] = 0
        got['froze_at'][o[freeze]] = c['it']
        got['n_active'] = int(write.sum()) + (0 if 'n_active stored' in W else int(before['n_active']))
    if zi:
        with np.errstate(all='ignore'):
            got['U_hat'][o[write]] = (n1 / n2)[write]
    got['Elog'][o[write]] = els[write]
    got['FUn'][write, :K] = fu[write]
    got['mu'][write] = np.where(bad[write], np.float32(np.nan), np.float32(0.0))
    mu = got['mu'].copy()
    if 'inactive mu left out' in W:
        mu[~was] = np.nan
    got['upart'] = fr.upart_ref(mu, r)
    return got


@pytest.mark.parametrize('case', SMALL, ids=fr.case_id)
def test_a_faithful_float32_evaluation_keeps_every_bound(case):
    c, before = fr.case_inputs(case)
    ref = fr.foldin_ref(c, before)
    got = _kernel_f32(c, before)
    out = fr.check(c, before, ref, got)
    assert max(out.values()) <= 1.0
    fr.check(c, before, ref, _kernel_f32(c, before, log_ulp=1))
    # what the case is there for
    cat = fr.categories(c['r'], c['zi'])
    if c['start']:
        assert not ref['freeze'].any() and ref['n_active'] == fr.N_ACTIVE0 and np.array_equal(ref['froze_at'], before['froze_at'])
        assert ref['write'][ref['orow'] == c['r'] - 1].all() and (ref['nanrow'] & ref['write']).sum() == (1 if c['zi'] else 0)
        if c['r'] >= 63:
            assert (~ref['write']).sum() > 100 and np.isnan(ref['mu']).sum() == 1 + int(c['zi'])
    elif c['r'] >= 63:
        want = {fr.INACTIVE: (False, False), fr.SAME: (False, True), fr.FIRST: (True, False), fr.LAST: (True, False),
                fr.A2ONLY: (True, False), fr.TIE_HOLD: (False, True), fr.TIE_FAIL: (True, False), fr.CLAMP: (True, False)}
        for k, (w, f) in want.items():
            assert (ref['write'][cat == k] == w).all() and (ref['freeze'][cat == k] == f).all(), k
        assert ref['n_active'] == fr.N_ACTIVE0 + int(ref['write'].sum()) > fr.N_ACTIVE0
        assert (ref['a1'][ref['orow'][cat == fr.CLAMP]] == 1e-15).all()
        assert (ref['Elog_ref'][cat == fr.LAST].argmax(axis=1) == c['K'] - 1).all()
        # the second call: rows that met their own a1 again freeze, the moved ones are written and counted again
        c2, b2 = fr.second_call(c, got)
        ref2 = fr.foldin_ref(c2, b2)
        fr.check(c2, b2, ref2, _kernel_f32(c2, b2))
        assert ref2['freeze'].sum() > 0 and ref2['write'].sum() > 0 and not (ref2['write'] & ~ref['write']).any()
        assert (ref2['froze_at'][ref2['orow'][ref2['freeze']]] == fr.IT + 1).all()
        assert ref2['n_active'] == ref['n_active'] + int(ref2['write'].sum())
    elif c['r'] == 3:
        assert ref['write'].tolist() == [True, False, False] and ref['freeze'].tolist() == [False, True, False]


WRONG = ['< for <=', 'OR stops before the last factor', 'shift omitted', 'shift over K - 1 factors', 'last slab dropped',
         'slab_row0 ignored', 'row_index on F and R', 'frozen row written', 'inactive mu left out', 'n_active stored',
         'ZI freezes on a1 alone']


@pytest.mark.parametrize('wrong', WRONG)
@pytest.mark.parametrize('K', [50, 33, 101])
def test_the_comparison_rejects_wrong_restatements(wrong, K):
    """Each mistake, made in the float32 evaluation and fed through foldin_update_reference.check, fails an assertion -- at a K
    of two factors per lane, of one, and of the element instantiation."""
    indexed = wrong == 'row_index on F and R'
    case = (wrong == 'ZI freezes on a1 alone', (3, 0 if indexed else fr.R_LONG // 2), fr.R_LONG, K, True, indexed)
    assert case in fr.CASES
    c, before = fr.case_inputs(case)
    ref = fr.foldin_ref(c, before)
    fr.check(c, before, ref, _kernel_f32(c, before))
    with pytest.raises(AssertionError):
        fr.check(c, before, ref, _kernel_f32(c, before, wrong=[wrong]))
    if wrong == '< for <=':
        # ... and it is the tie rows that catch it: without them the mistake passes
        cat = fr.categories(c['r'], c['zi'])
        b = dict(before, active=before['active'].copy())
        b['active'][ref['orow'][cat == fr.TIE_HOLD]] = 0
        fr.check(c, b, fr.foldin_ref(c, b), _kernel_f32(c, b, wrong=[wrong]))


# ---- one reference step is the model's map -----------------------------------------------------------------------------------------
def _step_inputs(zi, K, a1, a2, alpha1, alpha2, Z, rate):
    r, Kp = a1.shape[0], gr.kpad(K)
    c = dict(zi=zi, start=False, r=r, K=K, Kp=Kp, aligned=True, alias=False, nslab=1, slab_row0=0, tol=0.0, it=0, alpha1=alpha1,
             alpha2=alpha2 if zi else None, a2_row=None if zi else a2, rate=rate, Z=Z.astype(np.float32),
             F=np.zeros((r, Kp), dtype=np.float32), R=np.zeros((r, Kp), dtype=np.float32), row_index=None)
    before = dict(a1=a1.copy(), a2=a2.copy() if zi else None, U_hat=np.zeros((r, K)) if zi else None,
                  Elog=np.zeros((r, K), dtype=np.float32), FUn=np.zeros((r, Kp), dtype=np.float32), mu=np.zeros(r, dtype=np.float32),
                  upart=np.zeros((fr.blocks(r), 4), dtype=np.float32), active=np.ones(r, dtype=np.uint8),
                  froze_at=np.zeros(r, dtype=np.int32), n_active=0)
    return c, before


def test_one_reference_step_is_transform_references_map():
    """Z = float32 of the responsibility sums of transform_reference, F = R = 0: a1 of foldin_ref is T64 to the float32
    rounding of Z (2^-24 |Z|, and the float64 roundings of forming Z = T64 - alpha1 and adding alpha1 again)."""
    import transform_reference as tr
    rng = np.random.default_rng(11)
    n, m, K = 37, 29, 5
    X = rng.poisson(1.5, size=(n, m)).astype(np.float64)
    lv = rng.normal(-1.0, 1.0, size=(m, K)).astype(np.float32)
    alpha1, a2_row, a1 = rng.random(K) + 0.5, rng.random(K) * 20 + 1.0, rng.gamma(1.0, 1.0, size=(n, K))
    T = tr.T64(X, lv, alpha1, a2_row, a1)
    Z = T - alpha1[None, :]
    c, before = _step_inputs(False, K, a1, a2_row, alpha1, None, Z, None)
    ref = fr.foldin_ref(c, before)
    assert ref['write'].all() and ref['n_active'] == n
    assert (np.abs(ref['a1'] - T) <= gr.U32 * np.abs(Z) + 4 * gr.U64 * T).all()
    assert (np.abs(ref['a1'] - T) > 0).any()


def test_one_reference_step_is_zi_foldin_references_map():
    import zi_foldin_reference as zf
    rng = np.random.default_rng(12)
    n, m, K = 37, 29, 5
    X = (rng.poisson(1.5, size=(n, m)) * (rng.random((n, m)) < 0.7)).astype(np.float64)
    lv = rng.normal(-1.0, 1.0, size=(m, K)).astype(np.float32)
    V, pi_d = rng.gamma(1.0, 1.0, size=(m, K)), rng.uniform(0.3, 0.95, size=m)
    alpha1, alpha2 = rng.random(K) + 0.5, rng.random(K) + 0.5
    a1, a2 = rng.gamma(1.0, 1.0, size=(n, K)), rng.gamma(2.0, 3.0, size=(n, K))
    T1, T2 = zf.T64(X, lv, V, pi_d, alpha1, alpha2, a1, a2)
    Z = zf.responsibilities_sum(X, zf.elog_u(a1, a2), lv)
    rate = zf._dot(zf.dropout_f32(X, V, pi_d, a1 / a2).astype(np.float64), V)
    c, before = _step_inputs(True, K, a1, a2, alpha1, alpha2, Z, rate)
    ref = fr.foldin_ref(c, before)
    assert ref['write'].all() and ref['n_active'] == n
    assert (np.abs(ref['a1'] - T1) <= gr.U32 * np.abs(Z) + gr.U64 * T1).all()
    assert np.array_equal(ref['a2'], T2)                     # the same float64 addition and clamp


# ---- ORIANA_EINVAL / ORIANA_EKRANGE of both entries: before any launch -----------------------------------------------------------
def test_argument_errors_without_a_launch(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    plain = dict(a1=p, Elog=p, active=p, froze_at=p, n_active=p, alpha1=p, a2_row=p, Z=p, F=p, R=p, nslab=1, slab_row0=0, row_index=None,
                 r=4, K=4, tol=1e-4, it=0, FU_next=p, mu_out=p, upart=p)
    zi = dict(a1=p, a2=p, U_hat=p, Elog=p, active=p, froze_at=p, n_active=p, alpha1=p, alpha2=p, rate=p, Z=p, F=p, R=p, nslab=1,
              slab_row0=0, row_index=None, r=4, K=4, tol=1e-4, it=0, FU_next=p, mu_out=p, upart=p)
    for f, ok in ((lib.oriana_foldin_update, plain), (lib.oriana_foldin_update_zi, zi)):
        def rc(**kw):
            return f(*dict(ok, **kw).values(), None)
        for kw in (dict(r=-1), dict(K=0), dict(K=-3), dict(nslab=0), dict(nslab=65536), dict(slab_row0=-1), dict(it=-1), dict(it=1 << 31),
                   dict(tol=float('nan')), dict(tol=-1e-9)):
            assert rc(**kw) == EINVAL, kw
        assert rc(K=257) == EKRANGE
        assert rc(r=0) == 0 and rc(r=0, a1=None, Elog=None, active=None) == 0
        always = [k for k in ok if k in ('a1', 'a2', 'U_hat', 'Elog', 'active', 'a2_row', 'FU_next', 'mu_out', 'upart')]
        step = [k for k in ok if k in ('Z', 'F', 'alpha1', 'alpha2', 'rate', 'froze_at')]
        assert len(always) == (7 if ok is plain else 8) and len(step) == (4 if ok is plain else 6)
        start = dict(R=None, Z=None, F=None, alpha1=None, froze_at=None, n_active=None)
        if ok is zi:
            start.update(alpha2=None, rate=None)
        for k in always:
            assert rc(**{k: None}) == EINVAL, k                           # the step form
            assert rc(**dict(start, **{k: None})) == EINVAL, k            # the start form
        for k in step:
            assert rc(**{k: None}) == EINVAL, k                           # R given: the step form needs each of them
