# -*- coding: utf-8 -*-
"""CPU-only checks of tests/dense_pass_reference.py: the yardstick of tests/test_dense_pass_gpu.py is sharp, the complete
bf16 x 3 evaluation lies inside helpers.zlog_bound at every padded width, and an evaluation that loses one of its six cross
products lies outside it."""
import json

import numpy as np
import pytest

import dense_pass_reference as dr
from helpers import err_colrel, ZLOG_REF_MAX, ZLOG_REF_MAX_SLOW, zlog_bound


def test_splits_are_exact_truncations():
    rng = np.random.default_rng(1)
    x = (rng.normal(size=4096) * np.exp(rng.normal(size=4096) * 8)).astype(np.float32)
    x[:4] = [0.0, 1.0, -1.0, np.float32(1) + np.float32(2.0 ** -23)]
    hi, mid, lo = dr.split3(x)
    for p in (hi, mid, lo):
        assert not (p.view(np.uint32) & np.uint32(0xFFFF)).any()          # each part is a bf16
    assert np.array_equal(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64), x.astype(np.float64))
    assert (np.abs(hi) <= np.abs(x)).all() and (np.abs(mid) <= np.abs(x) * 2.0 ** -7).all() and (np.abs(lo) <= np.abs(x) * 2.0 ** -14).all()
    assert set(dr.SIX) | {(1, 2), (2, 1), (2, 2)} == {(a, b) for a in range(3) for b in range(3)}


def test_case_geometry():
    c = dr.pin_case(20)
    assert c['X'].shape == (300, 160) and c['lu'].shape == (300, 20) and c['lv'].shape == (160, 20)
    assert ((c['X'] != 0).sum(0) >= 0.1 * 300).all()                       # every gene dense at dense_density = 0.1
    assert c['X'].max() < 65536                                            # the dense block stores uint16
    assert not c['X'].flags.writeable and not c['exact'][0].flags.writeable
    assert dr.pin_case(20) is c
    s = dr.pin_case(20, 'sparse')
    assert not s['St'][dr.DEAD_GENE].any() and s['St'].any(1).sum() == 159
    assert not s['exact'][1][dr.DEAD_GENE].any() and not s['ref'][2][dr.DEAD_GENE].any()
    q = dr.pin_case(20, 'zi-quirk')
    assert np.array_equal(q['dq'], q['D'][:, :20]) and (q['D'][q['X'] != 0] == 1).all()
    t = dr.pin_case(41, 'gap', False, 160, 40)
    assert t['X'].shape == (300, 200) and ((t['X'][:, 160:] != 0).sum(0) < 0.1 * 300).all()
    assert len(dr.WIDTHS) == len(set(dr.KPADS)) == 12


@pytest.mark.parametrize('K', dr.WIDTHS)
def test_six_products_inside_and_mutants_outside_the_bound(K):
    """At every padded width, on the plain nest: the reference's float32 nest is a sharp yardstick, the complete six-product
    evaluation is inside zlog_bound(d_ref) on Z_i and on Z_j, and each mutant -- mid x mid missing, both lo terms missing, one lo
    term missing -- is outside it on both."""
    c = dr.pin_case(K)
    fig = dict(K=K, kpad=dr.KPADS[dr.WIDTHS.index(K)])
    fails = []
    evals = {'six products': dr.six_product_eval(c)}
    evals.update({name: dr.six_product_eval(c, drop) for name, drop in dr.MUTANTS.items()})
    for o, name in enumerate(('Z_i', 'Z_j')):
        exact = c['exact'][o]
        assert np.isfinite(exact).all()
        d_ref = err_colrel(c['ref'][o], exact)
        bound = zlog_bound(d_ref)
        fig[name] = dict(ref=d_ref, bound=bound)
        if not d_ref < ZLOG_REF_MAX:
            fails.append('%s: the reference nest is %.3e from exact' % (name, d_ref))
        for what, out in evals.items():
            d = err_colrel(out[o], exact)
            fig[name][what] = dict(dist=d, over_bound=d / bound)
            if (what == 'six products') != (d <= bound):
                fails.append('%s %s: %.3e against the bound %.3e' % (name, what, d, bound))
    print('DENSE_PIN_HOST ' + json.dumps(fig))
    assert not fails, fails


@pytest.mark.parametrize('K', dr.WIDTHS)
@pytest.mark.parametrize('nest,slow', [('gap', True), ('sparse', False), ('zi-quirk', False)])
def test_reference_float32_nest_is_a_sharp_yardstick(K, nest, slow):
    """The other cases the GPU tests judge by a multiple of the reference's own distance: that distance stays small."""
    c = dr.pin_case(K, nest, slow)
    lim = ZLOG_REF_MAX_SLOW if slow else ZLOG_REF_MAX
    for name, ref, exact in zip(('Z_i', 'Z_j', 'Z_log'), c['ref'], c['exact']):
        assert np.isfinite(exact).all()
        assert err_colrel(ref, exact) < lim, name
