# -*- coding: utf-8 -*-
"""The sliced row and column passes (csrc/passes_*.h, dispatched in csrc/passes.hip) against the float64 loop nest, per kernel
family and launch form, on counts constructed for the slice edges: every remainder of a slice's longest row, 0 .. 6 and 64
iterations per slice in one tile, empty slices and waves, ragged blocks and tiles (tests/sliced_pass_reference.py).  One K per
configuration of the dispatcher (18); on the row side one work-group walking every gene tile of its row block, a whole-grid
split, the split last round and the planner's own split; on the column side the planned work list, a list cut for many
items, one item per column block, the deterministic partials and the band grid of a call without a work list.  The bound is
helpers.zlog_bound, a multiple of the reference's own float32 distance measured on the same inputs
(tests/test_sliced_pass_host.py: an evaluation that loses one record of one slice, or takes one padding slot for an entry, is
outside it at every slice).  GPU only."""
import json

import numpy as np
import pytest
import torch

import sliced_pass_reference as sr
from helpers import err_colrel, zlog_bound, ZLOG_REF_MAX

pytestmark = pytest.mark.gpu
TILE = sr.TILE


@pytest.fixture(scope='module')
def eng():
    from oriana_amd import engine
    assert torch.cuda.is_available()
    return engine


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def host(t):
    return None if t is None else t.cpu().numpy()


# ---- the dispatcher's rule, restated -------------------------------------------------------------------
# These are restatements, not observations: the C ABI does not say which kernel template a launch took.  Each mirrors one place,
# and has to be read against it again whenever that place changes:
#   row_family   csrc/passes.hip  row_family(KCfg, V)   (V = 0 for 'plain'; weights, row-side s or a second image otherwise)
#   two_lane     csrc/passes.hip  takes_row_items(Fam)  (and the ORIANA_EINVAL of launch_row_pass for a split last round)
#   col_family   csrc/passes.hip  col_family(KCfg, Col::plain); Col::partials differs at Kp <= 20 only (generic), Col::dual
#                                 is k_col_pass2<DUAL> up to Kp = 64 and no kernel above
#   dual (run_pin)  engine._zq_cols: col_pass_dual is tried whenever Z_log is asked for and dq is None -- the weighted form
#                   included, not the sparse forms only -- and engine.col_pass_dual declines in the deterministic mode
#   per_item (run_pin)  csrc/passes.hip launch_col_pass, SPLIT = WaveGeo<G>::SPLIT (csrc/passes_generic.h)
#   band_grid    csrc/passes.hip  band_grid() and the two calls of it in launch_col_pass
# What IS observed beside them: oriana_kpad, oriana_col_block_tiles, the return codes of oriana_row_pass_general and
# oriana_col_pass_dual, ws.s_rs, ws.rows_nslab, ws.row_split, the work lists, and (run_pin) which of engine.col_pass_dual /
# engine.col_pass the nest called, with what list, and what the dual entry answered.
def kpad_of(K):
    return sr.KPADS[sr.WIDTHS.index(K)]


def row_family(K, form):
    kp = kpad_of(K)
    if 36 <= kp <= 64:
        return 'k64'
    if kp <= 32:
        return 'narrow' if form == 'plain' else 'generic'
    return 'k100' if kp in (96, 100) else 'generic'


def col_family(K):
    kp = kpad_of(K)
    return 'narrow' if kp <= 20 else 'k64' if 36 <= kp <= 64 else 'generic' if kp >= 128 else 'col2'


def two_lane(K):
    return 36 <= kpad_of(K) <= 64 or kpad_of(K) in (96, 100)


def band_grid(nrb, col_groups, target, min_band):
    """csrc/passes.hip band_grid: (bands, row blocks per band)."""
    nb = max(1, min(-(-target // col_groups), -(-nrb // min_band), 65535))
    per = -(-nrb // nb)
    return -(-nrb // per), per


def row_tiles(ws, ct):
    """Gene tiles per row-side work item (one per row block for the one-lane and G-lane kernels' grid.y index), from the split the
    workspace hands the row pass (struct oriana_row_split)."""
    sp, ncb = ws.row_split, ct.ncb
    if sp.edge[0] < 0:
        cut = [p * ncb // sp.parts for p in range(sp.parts + 1)]
    else:
        cut = [int(sp.edge[p]) for p in range(sp.parts + 1)]
    parts = [cut[p + 1] - cut[p] for p in range(sp.parts)]
    return [ncb] * int(sp.nfull) + parts * (ct.nrb - int(sp.nfull))


def col_items(ct, width):
    """The work list the column pass gets for this width: items, and items per column block."""
    w = ct.col_work_width(width)
    if w is None:
        return None
    w = host(w)
    nblk = -(-ct.ncb // width)
    assert ((0 <= w[:, 0]) & (w[:, 0] < nblk) & (0 <= w[:, 1]) & (w[:, 1] < w[:, 2]) & (w[:, 2] <= ct.nrb)).all()
    for b in range(nblk):                                  # the items of a column block cover every row block once
        cover = np.zeros(ct.nrb, int)
        for _, r0, r1 in w[w[:, 0] == b]:
            cover[r0:r1] += 1
        assert (cover == 1).all(), (b, w.tolist())
    return dict(width=width, items=len(w), per_block=[int((w[:, 0] == b).sum()) for b in range(nblk)],
                row_blocks=sorted({int(r1 - r0) for _, r0, r1 in w}))


ROW_FORMS = {'whole': lambda ct: (ct.nrb, 1, [0, ct.ncb]),        # one group per row block walks all gene tiles
             'even-2': lambda ct: (0, 2, None),                   # whole-grid split
             'last-round': lambda ct: (1, 2, [0, 2, ct.ncb]),     # row block 0 whole, the others in two gene ranges
             'planned': lambda ct: None}
COL_FORMS = ('planned', 'many-items', 'one-item', 'partials')


def run_pin(eng, c, row_form='planned', col_form='planned', clear_work=False):
    """engine.zq on a case in the given launch forms: outputs on the host, workspace, layout, the launch form as a dict."""
    from oriana_amd import _lib
    lib = _lib.load()
    K, form = c['K'], c['form']
    n, m = c['X'].shape
    ct = eng.CountTiles.from_dense(np.array(c['X']), 'cuda', side=dev(c['D']), sort_cols=False)
    assert ct.col_perm is None and ct.row_perm is None and ct.dense is None
    assert (ct.nrb, ct.ncb) == (-(-n // TILE), -(-m // TILE))
    ws = eng.ZWorkspace(ct, K)
    assert ws.Kp == kpad_of(K) == int(lib.oriana_kpad(K))
    split = ROW_FORMS[row_form](ct)
    if split is not None:
        ws.set_row_split(*split)
    width = int(lib.oriana_col_block_tiles(K))
    assert width == (2 if col_family(K) in ('k64', 'col2') else 1)
    # one walk, two images (a work list of single tiles) wherever the log sums are asked for and two images fit: every form but
    # 'plain', the weighted one included; not in the deterministic mode (engine._zq_cols, engine.col_pass_dual)
    dual = c['ref'][2] is not None and ws.Kp <= 64 and col_form != 'partials'
    widths = [1] if dual else [width]                                       # the list(s) this call's column passes read
    if col_form == 'many-items':
        for w in widths:
            ct._col_work[w] = ct._build_col_work(target_items=24, width=w)
    elif col_form == 'one-item':
        for w in widths:
            nblk = -(-ct.ncb // w)
            ct._col_work[w] = torch.tensor([[b, 0, ct.nrb] for b in range(nblk)], dtype=torch.int32, device='cuda')
    if clear_work:
        for w in widths:
            ct._col_work[w] = None                                          # engine.col_pass then passes work = NULL: the band grid
        assert ct.col_work_for(K) is None
    plain = form == 'plain'
    o = [torch.empty(n, K, device='cuda'), torch.empty(m, K, device='cuda'), None if plain else torch.empty(m, K, device='cuda')]
    # what the nest calls on the column side: the dual entry's answer, and every column pass with its list and mode
    seen, real_dual, real_col = [], eng.col_pass_dual, eng.col_pass

    def spy_dual(ct_, *a, **k):
        ok = real_dual(ct_, *a, **k)
        seen.append('dual:' + ('ran' if ok else 'declined'))
        return ok

    def spy_col(ct_, s_cs, G, C, K_, C_ptr=None, what='zj'):
        w_ = ct_.col_work_for(K_)
        seen.append('col_pass:%s:%s' % (what, 'bands' if w_ is None else 'partials' if eng.DETERMINISTIC else 'list'))
        return real_col(ct_, s_cs, G, C, K_, C_ptr=C_ptr, what=what)
    eng.set_deterministic(col_form == 'partials')
    eng.col_pass_dual, eng.col_pass = spy_dual, spy_col
    try:
        eng.zq(ws, o[0], o[1], o[2], dev(c['lu']), dev(c['lv']), S_tilde=dev(c['St']), S_hat=dev(c['Sh']),
               w_nz=ct.side_nz if c['D'] is not None else None)
        torch.cuda.synchronize()
    finally:
        eng.col_pass_dual, eng.col_pass = real_dual, real_col
        eng.set_deterministic(False)
    how = 'bands' if clear_work else 'partials' if col_form == 'partials' else 'list'
    if dual:
        assert seen == ['dual:ran'], seen
    elif plain:
        assert seen == ['col_pass:zj:' + how], seen
    else:                                                                   # two passes of the same family: the sums, the log sums
        assert seen == ['dual:declined', 'col_pass:zj:' + how, 'col_pass:log:' + how], seen
    # the column kernel of this call: one walk over two images (k_col_pass2<DUAL>) for every form with log sums up to Kp = 64; the
    # partials of Kp <= 20 come from the G-lane kernel (the one-lane kernel writes none); else the family of the plain form
    col_kernel = 'col2-dual' if dual else 'generic' if (col_form == 'partials' and col_family(K) == 'narrow') else col_family(K)
    row_kernel = row_family(K, form) + ('+row_spmm' if 'sparse' in form and ws.Kp > 64 else '')
    f = dict(kpad=ws.Kp, row_family=row_kernel, col_family=col_kernel, row_form=row_form, col_form=col_form,
             row_tiles=row_tiles(ws, ct), rows_nslab=ws.rows_nslab, col_calls=seen,
             launch_form='observed; the bands restated from band_grid' if clear_work else 'observed')
    if clear_work:
        narrow = col_family(K) == 'narrow'
        per_item = 1 if col_family(K) != 'generic' else 2 if ws.Kp <= 224 else 4                 # (WaveGeo<G>::SPLIT: 2 at G = 8, 4 at G = 16)
        groups = -(-ct.ncb // width) * per_item
        nb, per = band_grid(ct.nrb, groups, 2048 if narrow else 1024, 4 if narrow else 8)
        f['col'] = dict(bands=[min(per, ct.nrb - b * per) for b in range(nb)], col_groups=groups)
    else:
        f['col'] = [col_items(ct, w) for w in widths]
    if 'sparse' in form:
        # two images fit up to Kp = 64: the S_hat-weighted row sums come out of the row pass; beyond, s goes to row-side slots and
        # k_row_spmm follows
        assert (ws.s_rs is None) == (ws.Kp <= 64)
        f['sparse_rows'] = 'two-image' if ws.s_rs is None else 's_rs + k_row_spmm'
    return [host(t) for t in o], ws, ct, f


def judge(group, c, out, f, extra=None):
    """Every output no further from the float64 nest than zlog_bound of the reference's own distance; prints the figures."""
    fig = dict(group=group, problem=c['name'], side=c['side'], K=c['K'], form=c['form'])
    fig.update(f)
    fig.update(extra or {})
    fails = []
    for name, got, ref, exact in zip(('Z_i', 'Z_j', 'Z_log'), out, c['ref'], c['exact']):
        if ref is None:
            assert got is None
            continue
        d_hip, d_ref = err_colrel(got, exact), err_colrel(ref, exact)
        fig[name] = dict(hip=d_hip, ref=d_ref, ratio=d_hip / d_ref, over_bound=d_hip / zlog_bound(d_ref))
        if not d_ref < ZLOG_REF_MAX:
            fails.append('%s: the reference nest is %.3e from exact' % (name, d_ref))
        if not d_hip <= zlog_bound(d_ref):
            fails.append('%s: HIP is %.3e from exact, the reference arithmetic %.3e' % (name, d_hip, d_ref))
    print('SLICED_PIN ' + json.dumps(fig))
    assert not fails, fails


def conserved(c, out):
    """sum_k Z_i[i, k] = sum_j x_ij, sum_k Z_j[j, k] = sum_i x_ij: the tolerances of test_trim_last_iteration_gpu.py."""
    np.testing.assert_allclose(out[0].sum(1), c['X'].sum(1), rtol=2e-5, atol=1e-3)
    np.testing.assert_allclose(out[1].sum(1), c['X'].sum(0), rtol=2e-5, atol=1e-3)


def check(eng, group, c, row_form='planned', col_form='planned', clear_work=False):
    out, ws, ct, f = run_pin(eng, c, row_form, col_form, clear_work)
    assert int(ws.tile_flag.sum().item()) == 0                    # everything on the fast path: the kernels' own sums are judged
    judge(group, c, out, f)
    if c['form'] == 'plain':
        conserved(c, out)
    return out, ws, ct, f


# ---- 0. the dispatcher's table ------------------------------------------------------------------------------------------------
def test_dispatch_table(eng):
    """oriana_kpad and oriana_col_block_tiles over the 18 widths; oriana_col_pass_dual answers 0 up to Kp = 64 and
    ORIANA_EKRANGE (-2) above, where two images of 256 factor rows no longer fit in LDS."""
    from oriana_amd import _lib
    from oriana_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    assert tuple(int(lib.oriana_kpad(K)) for K in sr.WIDTHS) == sr.KPADS == (16, 20, 32, 36, 48, 52, 64, 68, 80, 84, 96, 100, 112, 128,
                                                                              160, 192, 224, 256)
    assert [int(lib.oriana_col_block_tiles(K)) for K in sr.WIDTHS] == [1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1]
    ct = eng.CountTiles.from_dense(np.array(sr.problem('small', 'rows')), 'cuda', sort_cols=False)
    w = ct.col_work_width(1)
    for K in sr.WIDTHS:
        ws = eng.ZWorkspace(ct, K)                                # (s = 0 everywhere: the pass adds nothing)
        C1, C2 = torch.zeros_like(ws.C), torch.zeros_like(ws.C)
        rc = lib.oriana_col_pass_dual(ct.sparse_struct, ptr(ws.s_cs), ptr(ws.FU), ptr(ws.FU), ptr(C1), ptr(C2), K, ptr(w), w.shape[0],
                                      stream_ptr())
        torch.cuda.synchronize()
        assert rc == (0 if ws.Kp <= 64 else -2), (K, rc)
        assert not C1.any() and not C2.any()


# ---- 1. every width: one group per row block, and the planner's split ---------------------------------------------------------
@pytest.mark.parametrize('row_form', ['whole', 'planned'])
@pytest.mark.parametrize('form', ['plain', 'sparse'])
@pytest.mark.parametrize('K', sr.WIDTHS)
@pytest.mark.parametrize('side', ['rows', 'cols'])
def test_every_width(eng, side, K, form, row_form):
    c = sr.case('small', side, K, form)
    out, ws, ct, f = check(eng, 'width:' + row_form, c, row_form)
    if row_form == 'whole':
        assert f['row_tiles'] == [ct.ncb] * ct.nrb and ct.ncb >= 3           # the image hand-over between tiles, the next one in flight
    else:
        assert len(f['row_tiles']) > ct.nrb                                  # 3 or 4 row blocks are far from filling the chip: split
    assert any(max(i['per_block']) > 1 for i in f['col'])                    # per-gene sums combined across work items


# ---- 2. the other launch forms, one width per family --------------------------------------------------------------------------
@pytest.mark.parametrize('row_form', ['even-2', 'last-round'])
@pytest.mark.parametrize('form', ['plain', 'sparse'])
@pytest.mark.parametrize('K', sr.FAMILY_WIDTHS)
@pytest.mark.parametrize('side', ['rows', 'cols'])
def test_row_side_splits(eng, side, K, form, row_form):
    """The whole-grid split in two gene ranges (every family) and the split last round with explicit edges (the two-lane
    families: k64, k100; the others answer ORIANA_EINVAL)."""
    from oriana_amd._lib import OrianaHipError
    c = sr.case('small', side, K, form)
    if row_form == 'last-round' and not two_lane(K):
        with pytest.raises(OrianaHipError, match='oriana_row_pass_general failed with code -1'):
            run_pin(eng, c, row_form)
        torch.cuda.synchronize()
        return
    out, ws, ct, f = check(eng, 'row-split:' + row_form, c, row_form)
    ncb = ct.ncb
    if row_form == 'even-2':
        assert f['row_tiles'] == [ncb // 2, ncb - ncb // 2] * ct.nrb
    else:
        assert f['row_tiles'] == [ncb] + [2, ncb - 2] * (ct.nrb - 1)
    if 'sparse' not in form or ws.Kp <= 64:
        assert f['rows_nslab'] == 2                                          # two slabs of R, added by the finalize


@pytest.mark.parametrize('col_form', ['many-items', 'one-item', 'partials'])
@pytest.mark.parametrize('form', ['plain', 'sparse'])
@pytest.mark.parametrize('K', sr.FAMILY_WIDTHS)
@pytest.mark.parametrize('side', ['rows', 'cols'])
def test_column_side_lists(eng, side, K, form, col_form):
    """A work list cut for 24 items (several items per column block: atomics across items), one item per column block walking every
    row block (the next row block's image and stream in flight), and the deterministic per-item partials -- twice, bit for bit."""
    c = sr.case('small', side, K, form)
    out, ws, ct, f = check(eng, 'col-list:' + col_form, c, 'planned', col_form)
    for i in f['col']:
        if col_form == 'one-item':
            assert i['per_block'] == [1] * len(i['per_block']) and i['row_blocks'] == [ct.nrb]
        else:
            assert max(i['per_block']) > 1
    if col_form == 'partials':
        again = run_pin(eng, c, 'planned', col_form)[0]
        for x, y in zip(out, again):
            assert (x is None and y is None) or x.tobytes() == y.tobytes()


# ---- 3. per-entry weights -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row_form', ['whole', 'planned'])
@pytest.mark.parametrize('form', ['weighted', 'sparse+weighted'])
@pytest.mark.parametrize('K', sr.WEIGHT_WIDTHS)
@pytest.mark.parametrize('side', ['rows', 'cols'])
def test_weights(eng, side, K, form, row_form):
    """D_hat at the stored entries (prefetch depth 2 on the G-lane row kernels; the weighted s in its own column-side slots)."""
    c = sr.case('small', side, K, form)
    out, ws, ct, f = check(eng, 'weights:' + row_form, c, row_form)
    assert ws.sw_cs is not None and len(out) == 3 and out[2] is not None
    # the log sums ride on the per-gene sums wherever two images fit, with or without S: k_col_pass2<DUAL> over single tiles
    if ws.Kp <= 64:
        assert f['col_family'] == 'col2-dual' and f['col_calls'] == ['dual:ran'] and [i['width'] for i in f['col']] == [1]
    else:
        assert f['col_family'] == col_family(K) and [i['width'] for i in f['col']] == [1 if ws.Kp >= 128 else 2]
    if row_form == 'whole':
        assert f['row_tiles'] == [ct.ncb] * ct.nrb


# ---- 4. the band grid: a column pass without a work list -----------------------------------------------------------------------
def expected_bands(K):
    return [4, 4, 3] if col_family(K) == 'narrow' else [6, 5]


@pytest.mark.parametrize('K', sr.BAND_WIDTHS)
@pytest.mark.parametrize('side', ['rows', 'cols'])
def test_band_grid(eng, side, K):
    """11 row blocks, work = NULL: launch_col_pass cuts row bands itself -- at least two, the last one ragged."""
    c = sr.case('band', side, K, 'plain')
    out, ws, ct, f = check(eng, 'band-grid', c, 'planned', 'planned', clear_work=True)
    assert ct.nrb == 11 and ct.ncb == 3
    assert f['col']['bands'] == expected_bands(K) and len(f['col']['bands']) >= 2 and f['col']['bands'][-1] < f['col']['bands'][0], f


@pytest.mark.parametrize('K', [20, 100])
@pytest.mark.parametrize('side', ['rows', 'cols'])
def test_band_grid_stateless(eng, side, K):
    """The consumer of the band grid: oriana_zq_gap_f32 packs X per call and runs the nest with no split and no work lists
    (csrc/stateless.hip).  The entry exposes neither: the launch form printed here is what that statement implies, an
    expectation, and is marked so."""
    c = sr.case('band', side, K, 'plain')
    n, m = c['X'].shape
    o = [torch.empty(n, K, device='cuda'), torch.empty(m, K, device='cuda')]
    eng.zq_gap_stateless(o[0], o[1], dev(c['lu']), dev(c['lv']), dev(c['X']))
    torch.cuda.synchronize()
    out = [host(t) for t in o] + [None]
    nrb, ncb = -(-n // TILE), -(-m // TILE)
    narrow = col_family(K) == 'narrow'
    groups = -(-ncb // (1 if narrow else 2))
    nb, per = band_grid(nrb, groups, 2048 if narrow else 1024, 4 if narrow else 8)
    bands = [min(per, nrb - b * per) for b in range(nb)]
    assert bands == expected_bands(K)
    judge('band-grid:stateless', c, out, dict(kpad=kpad_of(K), row_family=row_family(K, 'plain'), col_family=col_family(K), row_form='whole',
                                              col_form='bands', row_tiles=[ncb] * nrb, col=dict(bands=bands, col_groups=groups),
                                              launch_form='expected'))
    conserved(c, out)
