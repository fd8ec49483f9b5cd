# -*- coding: utf-8 -*-
"""CPU-only checks of tests/sliced_pass_reference.py: the constructed counts hold the cases tests/test_sliced_pass_gpu.py is
about, the float64 nest over the non-zeros agrees with cavi_oracle.zq_exact, the reference's float32 nest is a sharp yardstick
on every case the GPU module judges, and a float32 evaluation that loses the last record of one slice, or takes one padding
slot for an entry, lies outside helpers.zlog_bound -- for every slice of every tile."""
import json

import numpy as np
import pytest

import sliced_pass_reference as sr
from helpers import err_colrel, ZLOG_REF_MAX, zlog_bound

TILE = sr.TILE


def _base_cases(L, blocks, first, last):
    """The cases of test_trim_last_iteration_gpu.test_constructed_counts_hold_the_cases in the blocks `blocks`: the tiles
    `first` hold the remainder pairs, the tile `last` the empty slices."""
    for rb in blocks:
        pairs, same, diff = set(), 0, 0
        for cb in first:
            for w in range(8):
                l0, l1 = int(L[rb, cb, 2 * w]), int(L[rb, cb, 2 * w + 1])
                assert l0 > 0 and l1 > 0
                pairs.add((l0 % 4, l1 % 4))
                same += ((l0 + 3) // 4 == (l1 + 3) // 4); diff += ((l0 + 3) // 4 != (l1 + 3) // 4)
        assert pairs == {(a, b) for a in range(4) for b in range(4)}
        assert same > 0 and diff > 0
        assert {int(v) % 4 for cb in first for v in L[rb, cb]} == {0, 1, 2, 3}
        end = L[rb, last]
        assert any(end[2 * w] == 0 and end[2 * w + 1] > 0 for w in range(8))
        assert any(end[2 * w] > 0 and end[2 * w + 1] == 0 for w in range(8))
        assert any(end[2 * w] == 0 and end[2 * w + 1] == 0 for w in range(8))


@pytest.mark.parametrize('side', ['rows', 'cols'])
def test_small_problem_holds_the_cases(side):
    """3 x 4 tiles on the side under test: the cases of build_rows in the tiles it made, and in the added tile every iteration count
    0 .. 6 plus the 64-iteration slice, placed as every wave-to-slice mapping needs it."""
    X = sr.problem('small', side)
    assert X.shape == ((552, 805) if side == 'rows' else (808, 549)) and not X.flags.writeable
    assert sr.problem('small', side) is X
    Xs = sr.sliced_view('small', side)
    L = sr.slice_lengths('small', side)
    assert L.shape == (3, 4, 16)                                          # ragged last block (40 rows) and last tile (37 columns)
    ex = sr.extra_tile_index('small', side)
    assert ex == 2
    _base_cases(L, (0, 1), (0, 1), 3)
    assert (Xs[2 * TILE:, :TILE] != 0).sum() == 1                         # single-entry tile
    assert (Xs[2 * TILE:, TILE:2 * TILE] != 0).sum() == 0                 # tile with no entry
    assert (Xs[2 * TILE:, 3 * TILE:] != 0).sum() > 1                      # partial both ways
    it = sr.slice_iterations('small', side)
    assert int(it[:, [0, 1, 3]].max()) <= 4                               # (what build_rows reaches on its own)
    for rb in (0, 1):
        assert [int(v) for v in L[rb, ex]] == sr.EXTRA_LENGTHS[rb]
        assert set(range(7)) <= {int(v) for v in it[rb, ex]}              # 0 .. 6 iterations in ONE tile: around the depths 2, 3, 4
        deep = [s for s in range(16) if L[rb, ex, s] == sr.DEEP]
        assert len(deep) == 1 and it[rb, ex, deep[0]] == 64
        d = deep[0]
        r0 = rb * TILE + d * 16
        assert ((Xs[r0:r0 + 16, ex * TILE:(ex + 1) * TILE] != 0).sum(1) == TILE).sum() == 1     # one row with every column of the tile
        for width in (2, 4, 8, 16):       # a wave of the two-lane kernels, of the one-lane kernels / a group at G = 16, at G = 8, G = 4
            others = [int(L[rb, ex, s]) for s in range(d // width * width, d // width * width + width) if s != d]
            assert max(others) <= (sr.SHORT if width <= 4 else 24) and min(others) == 0, (width, others)
        assert any(0 < v <= sr.SHORT for v in (int(L[rb, ex, s]) for s in range(d // 4 * 4, d // 4 * 4 + 4) if s != d))
    # the deep slice is the first of its wave in one block and the second in the other
    assert {[s for s in range(16) if L[rb, ex, s] == sr.DEEP][0] % 2 for rb in (0, 1)} == {0, 1}
    assert [int(v) for v in L[2, ex, :3]] == sr.EXTRA_LENGTHS[2][:3] and not L[2, ex, 3:].any()


@pytest.mark.parametrize('side', ['rows', 'cols'])
def test_band_problem_holds_the_cases(side):
    """11 row blocks x 3 gene tiles: the construction of build_rows at that height (rows), its transpose at that width (cols)."""
    X = sr.problem('band', side)
    assert X.shape == (sr.BAND_ROWS, 549) and (X.shape[0] + TILE - 1) // TILE == 11 and X.shape[0] % TILE == 40
    Xs = sr.sliced_view('band', side)
    L = sr.slice_lengths('band', side)
    if side == 'rows':
        assert L.shape == (11, 3, 16)
        _base_cases(L, range(10), (0, 1), 2)
        assert (Xs[10 * TILE:, :TILE] != 0).sum() == 1 and (Xs[10 * TILE:, TILE:2 * TILE] != 0).sum() == 0
        assert (Xs[10 * TILE:, 2 * TILE:] != 0).sum() > 1
    else:
        assert L.shape == (3, 11, 16)
        _base_cases(L, (0, 1), (0, 1), 10)
        assert all((L[rb, 2:10] > 0).all() for rb in (0, 1))              # (longer slices further along: 4 i + a, a up to 20)
        assert (Xs[2 * TILE:, :TILE] != 0).sum() == 1 and (Xs[2 * TILE:, TILE:2 * TILE] != 0).sum() == 0
        assert (Xs[2 * TILE:, 10 * TILE:] != 0).sum() > 1


def test_widths_and_case_list():
    assert len(sr.WIDTHS) == len(set(sr.KPADS)) == 18
    assert set(sr.FAMILY_WIDTHS) | set(sr.WEIGHT_WIDTHS) | set(sr.BAND_WIDTHS) <= set(sr.WIDTHS)
    keys = sr.case_keys()
    assert len(keys) == len(set(keys)) == 2 * 2 * 18 + 2 * 2 * 6 + 2 * 7
    c = sr.inputs('small', 'rows', 20, 'sparse+weighted')
    assert c['lu'].dtype == c['lv'].dtype == c['X'].dtype == np.float32 and not c['lu'].flags.writeable
    assert 0.25 <= c['D'].min() and c['D'].max() <= 1.0
    assert set(np.unique(c['St'])) == {0.0, 1.0} and np.array_equal(c['St'], (c['Sh'] > np.float32(0.3)).astype(np.float32))
    assert sr.inputs('small', 'rows', 20, 'plain')['D'] is None and sr.inputs('small', 'rows', 20, 'plain')['St'] is None


@pytest.mark.parametrize('form', sr.FORMS)
@pytest.mark.parametrize('K', [13, 50])
@pytest.mark.parametrize('side', ['rows', 'cols'])
def test_nonzero_nest_agrees_with_zq_exact(side, K, form):
    """The float64 nest over the non-zeros against the dense float64 evaluation of the same statements: 1e-13 on every output."""
    from oracle import cavi_oracle as co
    a = sr.inputs('small', side, K, form)
    got = sr.exact_nz(a['lu'], a['lv'], a['X'], a['St'], a['Sh'], a['D'])
    ref = co.zq_exact(a['lu'], a['lv'], a['X'], S_tilde=a['St'], S_hat=a['Sh'], D_hat=a['D'], quirk=False)
    for name, g, r in zip(('Z_i', 'Z_j', 'Z_log'), got, ref):
        assert np.isfinite(r).all()
        assert err_colrel(g, r) < 1e-13, name


def test_zero_skipping_nest_is_the_same_nest():
    """The band problem's float32 yardstick (zq_gap_nz) is the full nest bit for bit."""
    from oracle import cavi_oracle as co
    c = sr.case('band', 'cols', 20, 'plain')
    n, m = c['X'].shape
    full = [np.empty((n, 20), np.float32), np.empty((m, 20), np.float32)]
    co.zq_gap(full[0], full[1], c['lu'], c['lv'], c['X'])
    assert full[0].tobytes() == c['ref'][0].tobytes() and full[1].tobytes() == c['ref'][1].tobytes()


@pytest.mark.parametrize('name,side,K,form', sr.case_keys(), ids=lambda v: str(v))
def test_reference_float32_nest_is_a_sharp_yardstick(name, side, K, form):
    """Every case the GPU module judges by a multiple of the reference's own distance: that distance stays under ZLOG_REF_MAX,
    the deep rows of the added tile included."""
    c = sr.case(name, side, K, form)
    fig = dict(problem=name, side=side, K=K, form=form)
    for o, (ref, exact) in zip(('Z_i', 'Z_j', 'Z_log'), zip(c['ref'], c['exact'])):
        assert np.isfinite(exact).all()
        if ref is not None:
            d = err_colrel(ref, exact)
            fig[o] = dict(ref=d, bound=zlog_bound(d))
            assert d < ZLOG_REF_MAX, o
    print('SLICED_PIN_REF ' + json.dumps(fig))
    assert (c['ref'][2] is None) == (form == 'plain')


@pytest.mark.parametrize('side', ['rows', 'cols'])
def test_lost_record_and_taken_padding_slot_are_outside_the_bound(side):
    """K = 20, plain nest, small problem.  The float32 evaluation in slot order is inside zlog_bound of the reference's distance on
    both outputs; with the record in the last occupied slot of ONE slice skipped, or with ONE padding slot read as an entry of
    image row 0 with x = 1, it is outside on both -- for every slice of every tile."""
    c = sr.case('small', side, 20, 'plain')
    ev = sr.f32_slot_eval(c, side)
    # (Zi / Zj of the evaluation follow the side under test: for 'cols' its rows are the genes)
    order = (0, 1) if side == 'rows' else (1, 0)
    exact = [c['exact'][o] for o in order]
    bound = [zlog_bound(err_colrel(c['ref'][o], c['exact'][o])) for o in order]
    stream = ev['stream']
    live = stream[5] >= 0
    assert int(live.sum()) == int((c['X'] != 0).sum()) and len(stream[0]) % 64 == 0
    assert len(set(zip(stream[4][live], stream[5][live]))) == int(live.sum())          # every entry in exactly one slot
    base = [err_colrel(ev['Zi'], exact[0]), err_colrel(ev['Zj'], exact[1])]
    assert base[0] <= bound[0] and base[1] <= bound[1], (base, bound)
    muts = sr.mutants(ev)
    L = sr.slice_lengths('small', side)
    assert len(muts) == int((L > 0).sum())                                  # one per slice that has a slot
    worst = dict(lost=[np.inf, np.inf], taken=[np.inf, np.inf])
    ntaken = 0
    for where, lost, taken in muts:
        for what, mut in (('lost', lost), ('taken', taken)):
            if mut is None:
                continue
            ntaken += what == 'taken'
            Zi, Zj = sr.apply_mutant(ev, mut)
            d = [err_colrel(Zi, exact[0]), err_colrel(Zj, exact[1])]
            for o in (0, 1):
                worst[what][o] = min(worst[what][o], d[o] / bound[o])
                assert d[o] > bound[o], (what, where, mut, o, d[o], bound[o])
    assert ntaken >= len(muts) - 2                                           # (a slice of 16 full-width rows has no padding slot)
    names = [('Z_i', 'Z_j')[o] for o in order]
    print('SLICED_PIN_HOST ' + json.dumps(dict(side=side, K=20, slices=len(muts),
                                                 complete_over_bound={z: base[o] / bound[o] for o, z in enumerate(names)},
                                                 least_mutant_over_bound={what: {z: w[o] for o, z in enumerate(names)} for what, w in worst.items()})))
