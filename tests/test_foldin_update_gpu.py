# -*- coding: utf-8 -*-
"""oriana_foldin_update and oriana_foldin_update_zi (csrc/updates.hip: k_foldin_update<VEC, LPR, NC, ZI>) called directly,
against the float64 statement of tests/foldin_update_reference.py, once per instantiation of the launch switch and per form of
the call (foldin_update_reference.CASES): the pair, the flags, the counter, mu and the partial statistics bit for bit, U_hat
within an ulp, the stored E[log U] and FUn inside the bounds derived there element by element, every row that is frozen,
freezing or inactive exactly as it was, and nothing written in padding columns or outside the buffers.  Every case with
r >= 63 makes a second call on what the first one left.  GPU only.

The thresholds are the derived bounds (ratio <= 1).  Seen on an MI355X, largest over the cases of an instantiation: stored
E[log U] 0.54 .. 0.75 of its bound (the largest at ZI <4, 32>), FUn 0.96 .. 0.98 (the bound is one float32
rounding and little more), U_hat 0 ulp; no instantiation stands out."""
import numpy as np
import pytest
import torch

import foldin_update_reference as fr
from test_gamma_update_gpu import GUARD_ROWS, SENTINEL, Buf

pytestmark = pytest.mark.gpu

assert SENTINEL == fr.SENTINEL
IFILL = {torch.uint8: 0x5A, torch.int32: -77}

WORST = {}                   # (output, instantiation) -> largest error / bound seen (printed when the module is done: run with -s)


@pytest.fixture(scope='module', autouse=True)
def _report():
    assert torch.cuda.is_available()
    yield
    for key in sorted(WORST):
        print('largest error / bound, %s %s<VEC %d, LPR %d, NC %d>: %.4g (%s)' % ((key[0], 'zi' if key[1] else 'plain') + key[2:] + WORST[key]))


class Shifted(Buf):
    """A Buf that starts `shift` bytes into its allocation (4: a float32 matrix that is element-aligned and no more)."""

    def __init__(self, shape, dtype, shift, guard=0, host=None):
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape))
        off = shift // torch.empty(0, dtype=dtype).element_size()
        self.flat = torch.full((off + n + guard,), SENTINEL, dtype=dtype, device='cuda')
        self.t = self.flat[off:off + n].view(shape)
        self.guard = self.flat[off + n:]
        self.head = self.flat[:off]
        if host is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(host)).view(shape))
        assert self.t.data_ptr() % 16 == shift


class IBuf:
    """An integer vector with 16 guard elements behind it."""

    def __init__(self, host, dtype):
        host = np.atleast_1d(np.asarray(host))
        n = host.shape[0]
        self.fill = IFILL[dtype]
        self.flat = torch.full((n + 16,), self.fill, dtype=dtype, device='cuda')
        self.t = self.flat[:n]
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(host)).to(dtype))
        self.ptr = self.t.data_ptr()

    def np(self):
        return self.t.cpu().numpy()

    def untouched(self):
        return bool((self.flat[self.t.shape[0]:] == self.fill).all())


def _buffers(c, before):
    """Every operand of the call on the device; what the entry may write sits between guard words and holds `before`."""
    f64, f32 = torch.float64, torch.float32
    r, K, Kp, al = c['r'], c['K'], c['Kp'], c['aligned']
    b = {}

    def mat(host, dtype, cols, aligned=al):
        return None if host is None else Buf(np.shape(host), dtype, aligned, GUARD_ROWS * cols, host=host)
    b['a1'] = mat(before['a1'], f64, K)
    b['a2'], b['U_hat'], b['rate'] = mat(before['a2'], f64, K), mat(before['U_hat'], f64, K), mat(c['rate'], f64, K)
    # unaligned: a1 (and the ZI matrices) 8 bytes off, Elog 4, F / FUn / R / Z 8
    b['Elog'] = mat(before['Elog'], f32, K) if al else Shifted((r, K), f32, 4, GUARD_ROWS * K, host=before['Elog'])
    b['Z'], b['R'] = mat(c['Z'], f32, K), mat(c['R'], f32, Kp)
    b['F'] = mat(c['F'], f32, Kp)
    b['FUn'] = b['F'] if c['alias'] else mat(before['FUn'], f32, Kp)
    b['mu'] = Buf((r,), f32, True, 8, host=before['mu'])
    b['upart'] = Buf(before['upart'].shape, f32, True, 8, host=before['upart'])
    b['active'], b['froze_at'] = IBuf(before['active'], torch.uint8), IBuf(before['froze_at'], torch.int32)
    b['n_active'] = IBuf([before['n_active']], torch.int32)
    for k in ('alpha1', 'alpha2', 'a2_row'):
        b[k] = None if c[k] is None else Buf((K,), f64, True, 4, host=c[k])
    b['row_index'] = None if c['row_index'] is None else IBuf(c['row_index'], torch.int32)
    return b


def _p(buf):
    return None if buf is None else buf.ptr


def _call(c, b):
    """One call of the entry; returns what the buffers hold afterwards."""
    from oriana_amd import _lib
    from oriana_amd._lib import stream_ptr
    lib = _lib.load()
    assert fr.blocks(c['r']) == int(lib.oriana_foldin_update_blocks(c['r'])) == b['upart'].t.shape[0]
    tail = (_p(b['Z']), _p(b['F']), _p(b['R']), c['nslab'], c['slab_row0'], _p(b['row_index']), c['r'], c['K'], c['tol'], c['it'],
            b['FUn'].ptr, b['mu'].ptr, b['upart'].ptr, stream_ptr())
    if c['zi']:
        rc = lib.oriana_foldin_update_zi(b['a1'].ptr, b['a2'].ptr, b['U_hat'].ptr, b['Elog'].ptr, b['active'].ptr, b['froze_at'].ptr,
                                         b['n_active'].ptr, _p(b['alpha1']), _p(b['alpha2']), _p(b['rate']), *tail)
    else:
        rc = lib.oriana_foldin_update(b['a1'].ptr, b['Elog'].ptr, b['active'].ptr, b['froze_at'].ptr, b['n_active'].ptr,
                                      _p(b['alpha1']), b['a2_row'].ptr, *tail)
    torch.cuda.synchronize()
    assert rc == 0
    got = {k: (None if b[k] is None else b[k].np()) for k in ('a1', 'a2', 'U_hat', 'Elog', 'FUn', 'mu', 'upart', 'active', 'froze_at')}
    got['n_active'] = int(b['n_active'].np()[0])
    return got


def _untouched(tag, c, b, inputs):
    """Guard words of every buffer, and the inputs the entry only reads."""
    for k, buf in b.items():
        if buf is not None:
            assert buf.untouched(), (tag, k)
    for k, host in inputs.items():
        if host is not None and not (k == 'F' and c['alias']):
            assert fr.same(b[k].np(), host), (tag, k)


def _check(tag, case, c, before, got):
    ref = fr.foldin_ref(c, before)
    out = fr.check(c, before, ref, got)
    inst = (c['zi'],) + fr.instantiation(c['zi'], c['K'], c['aligned'])
    for k, v in out.items():
        print('%s: %s %.4g of its bound' % (tag, k, v))
        if v >= WORST.get((k,) + inst, (-1.0, ''))[0]:
            WORST[(k,) + inst] = (v, tag)
    return ref


@pytest.mark.parametrize('case', fr.CASES, ids=fr.case_id)
def test_foldin_update_against_float64(case):
    tag = fr.case_id(case)
    c, before = fr.case_inputs(case)
    b = _buffers(c, before)
    inputs = {k: c[k] for k in ('Z', 'F', 'R', 'rate', 'alpha1', 'alpha2', 'a2_row', 'row_index')}
    got = _call(c, b)
    ref = _check(tag, case, c, before, got)
    _untouched(tag, c, b, inputs)
    if c['start']:
        assert got['n_active'] == fr.N_ACTIVE0 and ref['write'].any()
    if c['start'] or c['r'] < 63:
        return
    # the second call, on what the first one left: the rows that met their own pair again freeze now, the counter adds again
    c2, before2 = fr.second_call(c, got)
    b['Z'].t.copy_(torch.from_numpy(c2['Z']))
    if c['alias']:
        b['F'].t.copy_(torch.from_numpy(c['F']))
    got2 = _call(c2, b)
    ref2 = _check(tag + ' again', case, c2, before2, got2)
    _untouched(tag + ' again', c2, b, dict(inputs, Z=c2['Z']))
    assert ref2['freeze'].any() and ref2['write'].any() and got2['n_active'] == got['n_active'] + int(ref2['write'].sum())
