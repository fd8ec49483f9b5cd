# -*- coding: utf-8 -*-
"""The Gamma shape/rate update (k_gamma_update<FIN, NT>, k_gamma_update_vec<FIN, VEC, LPR>) and the M-step (k_mstep_gamma,
k_mstep_gamma_pair) of csrc/updates.hip against the float64 statement of tests/gamma_update_reference.py, once per
instantiation of the launch switches and per form of the call (gamma_update_reference.CASES): Z, a1 and a2 bit for bit on
inputs that make every float32 operation exact, E within an ulp, E[log .] inside the bound derived there element by element,
the column sums as ADDED into what the buffers held, the PREP outputs from the stored E[log .], and nothing written outside
the outputs.  GPU only."""
import numpy as np
import pytest
import torch

import gamma_update_reference as gr

pytestmark = pytest.mark.gpu

SENTINEL = -7777.25          # (exact in float32; no output of any case takes this value)
GUARD_ROWS = 3
EKRANGE = -2

WORST = {}                   # output -> largest error / bound seen (printed when the module is done: run with -s)


@pytest.fixture(scope='module', autouse=True)
def _report():
    assert torch.cuda.is_available()
    yield
    for key in sorted(WORST):
        print('largest error / bound, %s: %.4g (%s)' % ((key,) + WORST[key]))


def _note(key, value, tag=''):
    value = float(value)
    if value >= WORST.get(key, (-1.0, ''))[0]:
        WORST[key] = (value, tag)
    return value


class Buf:
    """A device matrix inside a larger allocation filled with SENTINEL: `guard` elements follow it, and an unaligned one
    starts 8 bytes into the allocation."""

    def __init__(self, shape, dtype, aligned=True, guard=0, host=None):
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape))
        off = 0 if aligned else 8 // torch.empty(0, dtype=dtype).element_size()
        self.flat = torch.full((off + n + guard,), SENTINEL, dtype=dtype, device='cuda')
        self.t = self.flat[off:off + n].view(shape)
        self.guard = self.flat[off + n:]
        self.head = self.flat[:off]
        if host is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(host)).view(shape))
        assert self.t.data_ptr() % 16 == (0 if aligned else 8)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def np(self):
        return self.t.cpu().numpy()

    def untouched(self):
        return bool((self.guard == SENTINEL).all()) and bool((self.head == SENTINEL).all())


def _up(host, dtype, aligned=True):
    return None if host is None else Buf(np.shape(host), dtype, aligned, host=np.asarray(host))


def _p(buf):
    return None if buf is None else buf.ptr


def _same(got, want):
    """bit for bit, a NaN matching a NaN"""
    return np.array_equal(got, want, equal_nan=True)


def _launch(case, d, Kp, lazy=False):
    """One call of the entry the case names, on fresh buffers.  Returns (rc, buffers)."""
    from oriana_amd import _lib
    from oriana_amd._lib import stream_ptr
    lib = _lib.load()
    entry, form, r, K, aligned, prep = case
    f64, f32 = torch.float64, torch.float32
    rng = np.random.default_rng(K + 7 * r)
    b = {}
    stored = form == 'stored'
    b['a1'] = Buf((r, K), f64, aligned, GUARD_ROWS * K, host=d['a1'] if stored else None)
    b['El'] = Buf((r, K), f32, aligned, GUARD_ROWS * K)
    if lazy:
        b['a2row'] = Buf((K,), f64, aligned, 4)
    else:
        b['a2'] = Buf((r, K), f64, aligned, GUARD_ROWS * K, host=d['a2'] if stored else None)
        b['E'] = Buf((r, K), f64, aligned, GUARD_ROWS * K)
    if form != 'specials':
        b['start'] = rng.standard_normal((2, K)) * 3.0          # the kernel ADDS: the sums start from something
        b['sums'] = Buf((2, K), f64, True, 4, host=b['start'])
        sE, sL = b['sums'].t[0].data_ptr(), b['sums'].t[1].data_ptr()
    else:
        sE = sL = None
    nblk = gr.prep_blocks(r, K) if prep else 0
    if prep:
        assert nblk == int(lib.oriana_gamma_update_prep_blocks(r, K)) and nblk > 0
        b['FUn'] = Buf((r, Kp), f32, aligned, GUARD_ROWS * Kp)
        b['mu'] = Buf((r,), f32, True, 8)
        b['up'] = Buf((nblk, 4), f32, True, 8)
    pp = (_p(b.get('FUn')), _p(b.get('mu')), _p(b.get('up')))
    p1, p2 = _up(d.get('prior1'), f64), _up(d.get('prior2'), f64)
    rv = _up(d.get('rate_vec'), f64)
    b['Z'] = None if stored else Buf((r, K), f32, aligned, GUARD_ROWS * K, host=d['Z'])
    st = stream_ptr()
    if entry == 'plain':
        zm, rm, rmul = _up(d.get('zmul'), f32, aligned), _up(d.get('rate_mat'), f64, aligned), _up(d.get('rmul'), f32, aligned)
        args = (b['a1'].ptr, b['a2'].ptr, b['E'].ptr, b['El'].ptr, sE, sL, _p(p1), _p(p2), _p(b['Z']), _p(zm), _p(rv), _p(rm), _p(rmul),
                r, K)
        if prep:
            rc = lib.oriana_gamma_update_prep(*args, *pp, st)
        else:
            rc = lib.oriana_gamma_update(*args, st)
    else:
        F, R = _up(d['F'], f32, aligned), _up(d['R'], f32, aligned)
        ri = _up(d['row_index'], torch.int32)
        tail = (_p(p1), _p(p2), b['Z'].ptr, F.ptr, R.ptr, d['nslab'], d['slab_row0'], ri.ptr, rv.ptr, r, K, *pp, st)
        if lazy:
            rc = lib.oriana_gamma_update_finalize_lazy(b['a1'].ptr, b['a2row'].ptr, b['El'].ptr, sE, sL, *tail)
        else:
            rc = lib.oriana_gamma_update_finalize_prep(b['a1'].ptr, b['a2'].ptr, b['E'].ptr, b['El'].ptr, sE, sL, *tail)
    torch.cuda.synchronize()
    return rc, b


def _check_sums(tag, b, ref, El):
    got = b['sums'].np()
    for i, (name, x) in enumerate((('sum E', ref['E']), ('sum Elog', El.astype(np.float64)))):
        want = gr.colsum_total(b['start'][i], x)
        tol = gr.colsum_tol(b['start'][i], x)
        fin = np.isfinite(want)
        assert _same(got[i][~fin], want[~fin]), (tag, name)
        if fin.any():
            assert _note(name, (np.abs(got[i][fin] - want[fin]) / tol[fin]).max(), tag) <= 1.0, (tag, name)
    assert b['sums'].untouched()


def _check_prep(tag, case, d, b, El, Kp):
    entry, form, r, K, aligned, prep = case
    packed = El[d['row_index']] if entry == 'fin' else El
    mu, fu, stats = gr.prep_ref(packed)
    assert _same(b['mu'].np(), mu), tag
    FUn = b['FUn'].np()
    got = FUn[:, :K]
    with np.errstate(all='ignore'):
        want = fu.astype(np.float32)
        ulp = np.spacing(np.abs(want))
        err = np.abs(got.astype(np.float64) - fu)
    bad = np.isnan(fu)
    assert np.array_equal(np.isnan(got), bad), tag
    assert _note('FU_next (float32 ulps)', (err[~bad] / ulp[~bad].astype(np.float64)).max(), tag) <= 1.0, tag
    assert (FUn[:, K:] == SENTINEL).all(), tag                   # the padding columns are not the kernel's to write
    up = b['up'].np().astype(np.float64)
    assert up[:, 2].sum() == stats['count'] and np.float32(up[:, 3].min()) == stats['min'], tag
    if form == 'stored':
        assert stats['min'] < -gr.STAT_MAX and stats['count'] == r - 2 and np.isnan(mu).sum() == 1
    n = max(stats['count'], 1)
    # float32 sums of n terms in some order: (n - 1) roundings of 2^-24 each on at most sum |x|; a square adds one
    assert abs(up[:, 0].sum() - stats['sum']) <= (n - 1) * gr.U32 * stats['sum_abs'], tag
    assert abs(up[:, 1].sum() - stats['sumsq']) <= n * gr.U32 * stats['sumsq'], tag
    assert b['FUn'].untouched() and b['mu'].untouched() and b['up'].untouched(), tag


@pytest.mark.parametrize('case', gr.CASES, ids=gr.case_id)
def test_gamma_update_against_float64(case):
    entry, form, r, K, aligned, prep = case
    tag = gr.case_id(case)
    d, Kp = gr.case_inputs(case)
    ref = gr.gamma_update_ref(**d)
    rc, b = _launch(case, d, Kp)
    assert rc == 0, tag
    # shapes, rates and the completed Z: bit for bit
    a1, a2, E, El = b['a1'].np(), b['a2'].np(), b['E'].np(), b['El'].np()
    if ref['Z_out'] is not None:
        assert _same(b['Z'].np(), ref['Z_out']), tag
        assert b['Z'].untouched()
    assert _same(a1, ref['a1']), tag
    assert _same(a2, ref['a2']), tag
    # E within an ulp of a1 / a2
    fin = np.isfinite(ref['E'])
    assert _same(E[~fin], ref['E'][~fin]), tag
    assert _note('E (float64 ulps)', (np.abs(E[fin] - ref['E'][fin]) / np.spacing(np.abs(ref['E'][fin]))).max(), tag) <= 1.0, tag
    # E[log .] inside its bound, element by element; what is not finite in the reference, in place
    ratio = gr.elog_ratio(El, ref)
    assert _note('Elog', ratio.max(), tag) <= 1.0, (tag, np.unravel_index(int(ratio.argmax()), ratio.shape))
    if form == 'specials':
        assert (~np.isfinite(ref['Elog_ref'])).sum() >= 3 and (ref['a1'] == 1e-15).sum() >= 3
    else:
        _check_sums(tag, b, ref, El)
    for k in ('a1', 'a2', 'E', 'El'):
        assert b[k].untouched(), (tag, k)
    if prep:
        _check_prep(tag, case, d, b, El, Kp)
    if entry != 'fin':
        return
    # the lazy entry: no a2 and no E matrix, the K rates once; ORIANA_EKRANGE exactly where the launch rule says
    rc, lz = _launch(case, d, Kp, lazy=True)
    if not gr.lazy_runs(r, K, aligned, prep):
        assert rc == EKRANGE, tag
        assert (lz['a1'].flat == SENTINEL).all() and (lz['El'].flat == SENTINEL).all() and (lz['a2row'].flat == SENTINEL).all()
        return
    assert rc == 0, tag
    assert _same(lz['a2row'].np(), ref['a2'][0]) and lz['a2row'].untouched(), tag
    assert _same(lz['a1'].np(), a1) and _same(lz['El'].np(), El) and _same(lz['Z'].np(), ref['Z_out']), tag
    _check_sums(tag + ' lazy', lz, ref, El)
    assert lz['a1'].untouched() and lz['El'].untouched() and lz['Z'].untouched(), tag
    if prep:
        _check_prep(tag + ' lazy', case, d, lz, El, Kp)


# ---- the M-step --------------------------------------------------------------------------------------------------------------
Y_LADDER = [-1e15, -2e15, -1e4, -50.0, -2.5, -2.23, -2.21, -1.0, 0.0, 1.0, 5.0, 20.0]     # log p2 + mean log: both sides of -2.22


def _mstep_inputs(K, count, seed):
    """Priors and column sums whose y = log p2 + f32(sumL / count) walks Y_LADDER; column 0 holds clamped shapes (mean log
    -1e15: the float32 nearest to it lies above, the new shape does not clamp), column 1 a mean of -2e15 (it does, to
    1e-15 exactly); one column carries no mass (sum E = 0: the rate is DBL_MAX)."""
    rng = np.random.default_rng(seed)
    p2 = rng.random(K) + 0.5
    p2[:2] = 1e-3
    y = np.array(Y_LADDER)[np.arange(K) % len(Y_LADDER)] * (1.0 + 0.01 * (np.arange(K) // len(Y_LADDER)))
    sumL = (y - np.log(p2)) * count
    sumE = (rng.random(K) * 3.0 + 0.01) * count
    sumE[min(3, K - 1)] = 0.0
    return rng.random(K) + 0.5, p2, sumE, sumL


def _check_mstep(tag, got1, got2, p2, sumE, sumL, count):
    want1, want2 = gr.mstep_ref(None, p2, sumE, sumL, count)
    for name, got, want in (('M-step shape', got1, want1), ('M-step rate', got2, want2)):
        pinned = ~np.isfinite(want) | (want == 1e-15) | (want == gr.DBL_MAX)
        assert _same(got[pinned], want[pinned]), (tag, name)
        rel = np.abs(got[~pinned] - want[~pinned]) / np.abs(want[~pinned])
        if rel.size:
            assert _note(name + ' (of rtol 1e-9)', rel.max() / 1e-9, tag) <= 1.0, (tag, name)
    return want1, want2


@pytest.mark.parametrize('K', [1, 64, 65, 100, 129, 512])
def test_mstep_against_float64(K):
    from oriana_amd._lib import call, stream_ptr
    f64 = torch.float64
    for count in (1e6, 1.0):
        p1, p2, sumE, sumL = _mstep_inputs(K, count, K)
        b1, b2 = Buf((K,), f64, True, 4, host=p1), Buf((K,), f64, True, 4, host=p2)
        cE, cL = _up(sumE, f64), _up(sumL, f64)
        call('oriana_mstep_gamma', b1.ptr, b2.ptr, cE.ptr, cL.ptr, count, K, stream_ptr())
        torch.cuda.synchronize()
        w1, w2 = _check_mstep('single K=%d count=%g' % (K, count), b1.np(), b2.np(), p2, sumE, sumL, count)
        assert b1.untouched() and b2.untouched()
        assert _same(cE.np(), sumE) and _same(cL.np(), sumL)
        if K > 3:
            assert w2[3] == gr.DBL_MAX
        if K > 1:
            assert w1[1] == 1e-15 and 1e-15 < w1[0] < 1.0000001e-15


@pytest.mark.parametrize('keep', [False, True])
@pytest.mark.parametrize('K', [1, 64, 65, 100, 129, 512])
def test_mstep_pair_against_float64(K, keep):
    from oriana_amd._lib import call, stream_ptr
    f64 = torch.float64
    cu, cv = 1e6, 1.0                                            # the two sides: a million cells, a single gene
    u = _mstep_inputs(K, cu, 2 * K)
    v = _mstep_inputs(K, cv, 2 * K + 1)
    bu = [Buf((K,), f64, True, 4, host=x) for x in u]
    bv = [Buf((K,), f64, True, 4, host=x) for x in v]
    kv = Buf((2 * K,), f64, True, 4)
    call('oriana_mstep_gamma_pair', bu[0].ptr, bu[1].ptr, bu[2].ptr, bu[3].ptr, cu, bv[0].ptr, bv[1].ptr, bv[2].ptr, bv[3].ptr, cv,
         kv.ptr if keep else None, K, stream_ptr())
    torch.cuda.synchronize()
    _check_mstep('pair u K=%d' % K, bu[0].np(), bu[1].np(), u[1], u[2], u[3], cu)
    _check_mstep('pair v K=%d' % K, bv[0].np(), bv[1].np(), v[1], v[2], v[3], cv)
    for b, h in ((bu[2], u[2]), (bu[3], u[3]), (bv[2], v[2]), (bv[3], v[3])):
        assert _same(b.np(), h) and b.untouched()
    assert all(b.untouched() for b in bu[:2] + bv[:2])
    if keep:
        assert _same(kv.np(), np.concatenate([v[2], v[3]])) and kv.untouched()
    else:
        assert (kv.flat == SENTINEL).all()
