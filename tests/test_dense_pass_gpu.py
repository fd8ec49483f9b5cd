# -*- coding: utf-8 -*-
"""The dense-gene passes (csrc/dense_pass.hip: k_dn_row, k_dn_col, the slow path behind them) against the float64 loop nest,
at every padded width of the factor matrices and in the launch forms where one work-group walks several tiles: the ring of three
image buffers wraps, the gene side leaves the matrix core after eight cell tiles, a wave's flag word carries several tiles.
Cases and yardsticks: tests/dense_pass_reference.py; the bound is helpers.zlog_bound, a multiple of the reference's own float32
distance measured on the same inputs (tests/test_dense_pass_host.py: an evaluation that loses one of the six cross products is
outside it at every width).  GPU only."""
import json

import numpy as np
import pytest
import torch

import dense_pass_reference as dr
from helpers import err_colrel, zlog_bound, ZLOG_REF_MAX, ZLOG_REF_MAX_SLOW

pytestmark = pytest.mark.gpu

# LDS-DMA instructions per wave and cell tile of the gene-side kernel (cell image pieces / 512 + the four of the s tile): the
# count its vector-memory waits are written for, per padded width
NCOPY = {16: 5, 20: 5, 32: 5, 36: 5, 48: 6, 52: 6, 64: 6, 68: 6, 80: 7, 84: 7, 96: 7, 100: 7}
TWO_LANE = [K for K in dr.WIDTHS if 33 <= K <= 64 or 85 <= K <= 100]      # the sliced row pass splits single row blocks
TAIL_SPARSE_GENES = 260          # two sliced gene tiles (256 + 4): a two-part split needs two


@pytest.fixture(scope='module')
def eng():
    from oriana_amd import engine
    assert torch.cuda.is_available()
    return engine


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def host(t):
    return t.cpu().numpy()


def launch_form(ws, ct, K):
    """What the two launches do with the workspace's splits (include/oriana_hip.h: even ranges of gene tiles per row-side group,
    of cell tiles per gene-side group, eight gene tiles per gene-side group)."""
    from oriana_amd import _lib
    lib = _lib.load()
    ngt, nct = ct.gd // 32, (ct.n + 31) // 32
    per_g = -(-ngt // min(ws.dn_gene_splits, ngt))
    per_c = -(-nct // min(ws.dn_cell_splits, nct))
    pv, pu = int(lib.oriana_dense_image_pieces(K, 0)), int(lib.oriana_dense_image_pieces(K, 1))
    assert pv % 512 == 0 and pu % 512 == 0 and pv > pu > 0               # whole LDS-DMA rounds of the eight waves
    groups = -(-ngt // 8)
    return dict(row_tiles=[min(per_g, ngt - g) for g in range(0, ngt, per_g)], col_tiles=[min(per_c, nct - c) for c in range(0, nct, per_c)],
                col_groups=groups, idle_waves=8 * groups - ngt, ncopy=pu // 512 + 4, kpad=int(lib.oriana_kpad(K)))


def run_pin(eng, c, splits, row_split=None):
    """engine.zq on a pin case with the dense kernels' splits set by hand: outputs on the host, workspace, layout, launch form."""
    n, mt, K = dr.PIN_N, c['m'], c['K']
    ct = eng.CountTiles.from_dense(np.array(c['X']), 'cuda', dense_density=0.1)
    assert ct.gd == c['gd'] and ct.ms == mt - c['gd']
    ws = eng.ZWorkspace(ct, K)
    planned = (ws.dn_gene_splits, ws.dn_cell_splits)
    ws.dn_gene_splits, ws.dn_cell_splits = splits
    if row_split is not None:
        ws.set_row_split(*row_split)
    o = [torch.empty(n, K, device='cuda'), torch.empty(mt, K, device='cuda'), torch.empty(mt, K, device='cuda')]
    if c['nest'] == 'gap':
        o = o[:2]
        eng.zq_gap(ws, o[0], o[1], dev(c['lu']), dev(c['lv']))
    else:
        eng.zq(ws, o[0], o[1], o[2], dev(c['lu']), dev(c['lv']), S_tilde=dev(c['St']), S_hat=dev(c['Sh']), dq=dev(c['dq']))
    torch.cuda.synchronize()
    form = launch_form(ws, ct, K)
    assert form['kpad'] == dr.KPADS[dr.WIDTHS.index(K)] and form['ncopy'] == NCOPY[form['kpad']], form
    return [host(t) for t in o], ws, ct, form, planned


def flags(ws, ct):
    """The slow-path flags as [cell tile][gene tile]."""
    d = ct.dense
    return host(ws.dn_flag)[:d.nct * d.ngt].reshape(d.nct, d.ngt)


def judge(group, c, out, form, splits, extra=None):
    """Every output no further from the float64 nest than zlog_bound of the reference's own distance; prints the figures."""
    fig = dict(group=group, K=c['K'], kpad=form['kpad'], nest=c['nest'], slow=c['slow'], m=c['m'], gd=c['gd'], splits=list(splits),
               row_tiles=form['row_tiles'], col_tiles=form['col_tiles'])
    fig.update(extra or {})
    fails = []
    lim = ZLOG_REF_MAX_SLOW if c['slow'] else ZLOG_REF_MAX
    for name, got, ref, exact in zip(('Z_i', 'Z_j', 'Z_log'), out, c['ref'], c['exact']):
        d_hip, d_ref = err_colrel(got, exact), err_colrel(ref, exact)
        fig[name] = dict(hip=d_hip, ref=d_ref, ratio=d_hip / d_ref, over_bound=d_hip / zlog_bound(d_ref))
        if not d_ref < lim:
            fails.append('%s: the reference nest is %.3e from exact' % (name, d_ref))
        if not d_hip <= zlog_bound(d_ref):
            fails.append('%s: HIP is %.3e from exact, the reference arithmetic %.3e' % (name, d_hip, d_ref))
    print('DENSE_PIN ' + json.dumps(fig))
    assert not fails, fails


def conserved(c, out):
    """sum_k Z_i[i, k] = sum_j x_ij, sum_k Z_j[j, k] = sum_i x_ij (every responsibility vector sums to 1): the tolerances of
    test_dense_gpu.py."""
    assert np.allclose(out[0].sum(1), c['X'].sum(1), rtol=2e-6)
    assert np.allclose(out[1].sum(1), c['X'].sum(0), rtol=2e-5, atol=1e-3)


def test_padded_widths():
    from oriana_amd import _lib
    lib = _lib.load()
    assert tuple(int(lib.oriana_kpad(K)) for K in dr.WIDTHS) == dr.KPADS == (16, 20, 32, 36, 48, 52, 64, 68, 80, 84, 96, 100)
    assert all(int(lib.oriana_dense_supported(K)) == 1 for K in dr.WIDTHS)


# ---- 1. launch forms ----------------------------------------------------------------------------------------------------------
FORMS = {'unsplit': ((1, 1), [5], [10]),                     # the row loop walks 5 tiles (the ring wraps); one flush + 2 on the gene side
         'split-2x3': ((2, 3), [3, 2], [4, 4, 2]),           # gene ranges through the atomic output
         'planned': (None, [1] * 5, [1] * 10)}               # one tile per work-group: what the planner picks at this size


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('K', dr.WIDTHS)
def test_launch_forms(eng, K, form):
    """The plain nest on the fast path in the three launch forms, every padded width: no entry flagged, both outputs inside the
    bound, the responsibilities conserved."""
    c = dr.pin_case(K)
    ngt, nct = dr.PIN_M // 32, (dr.PIN_N + 31) // 32
    splits, row_tiles, col_tiles = FORMS[form]
    splits = splits or (ngt, nct)
    out, ws, ct, f, planned = run_pin(eng, c, splits)
    assert ct.gd == dr.PIN_M and ct.ms == 0
    assert f['row_tiles'] == row_tiles and f['col_tiles'] == col_tiles and f['col_groups'] == 1 and f['idle_waves'] == 3, f
    if form == 'planned':
        assert planned == splits, planned
    assert int(ws.dn_flag.sum().item()) == 0                  # the fast kernels are the ones being judged
    judge('launch-form:' + form, c, out, f, splits, dict(planned=list(planned)))
    conserved(c, out)


# ---- 2. the sparse and zi-quirk nests, unsplit ----------------------------------------------------------------------------------
@pytest.mark.parametrize('nest', ['sparse', 'zi-quirk'])
@pytest.mark.parametrize('K', dr.WIDTHS)
def test_nests_unsplit(eng, K, nest):
    """sparse: den against the masked FV image, R against the second image FV * S_hat, both gene-side products (sum s FU and the
    centred sum s FU E[log U]) over the same s; zi-quirk: the gene-side factor FU * dq.  Z_i, Z_j and Z_log are judged."""
    c = dr.pin_case(K, nest)
    out, ws, ct, f, _ = run_pin(eng, c, (1, 1))
    assert ct.gd == dr.PIN_M and f['row_tiles'] == [5] and f['col_tiles'] == [10], f
    fl = flags(ws, ct)
    if nest == 'sparse':
        cp = host(ct.col_perm)
        dead_tile = int(np.flatnonzero(cp[:ct.gd] == dr.DEAD_GENE)[0]) // 32
        assert fl[:, dead_tile].all() and not np.delete(fl, dead_tile, axis=1).any()     # only the dead gene's tiles leave the fast path
        assert not out[1][dr.DEAD_GENE].any() and not out[2][dr.DEAD_GENE].any()
    else:
        assert not fl.any()
    assert len(out) == 3
    judge('nest:' + nest, c, out, f, (1, 1))


# ---- 3. the slow path across the tiles of one wave -----------------------------------------------------------------------------
@pytest.mark.parametrize('K', dr.WIDTHS)
def test_slow_path_across_tiles(eng, K):
    """One cell at lu - 80: its cell tile is flagged in all five gene tiles -- five bits of one wave's flag word, written after
    the loop -- and the exact slow path fills them in."""
    c = dr.pin_case(K, 'gap', True)
    out, ws, ct, f, _ = run_pin(eng, c, (1, 1))
    assert ct.gd == dr.PIN_M and f['row_tiles'] == [5] and f['col_tiles'] == [10], f
    fl = flags(ws, ct)
    assert int(fl.sum()) > 0
    rp = host(ct.row_perm) if ct.row_perm is not None else np.arange(dr.PIN_N)
    slow_tile = int(np.flatnonzero(rp == dr.SLOW_CELL)[0]) // 32
    assert fl[slow_tile].all() and not np.delete(fl, slow_tile, axis=0).any()
    judge('slow-path', c, out, f, (1, 1), dict(flagged=int(fl.sum())))
    conserved(c, out)


# ---- 4. two gene-side work-groups ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [100, 33])
def test_two_gene_side_groups(eng, K):
    """m = 288: nine gene tiles, the second gene-side group has one live wave and seven clamped to the last tile."""
    c = dr.pin_case(K, 'gap', False, 288)
    out, ws, ct, f, _ = run_pin(eng, c, (1, 1))
    assert ct.gd == 288 and f['row_tiles'] == [9] and f['col_tiles'] == [10] and f['col_groups'] == 2 and f['idle_waves'] == 7, f
    assert int(ws.dn_flag.sum().item()) == 0
    judge('two-gene-groups', c, out, f, (1, 1))
    conserved(c, out)


# ---- 5. the split last round -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', TWO_LANE)
def test_split_last_round(eng, K):
    """The tail_parts path of oriana_dense_row_pass_tail: the second 256-cell block (44 cells) in two gene-tile ranges, each adding
    into its own slab of R beside the sliced row pass's parts.  The 160 dense genes and 260 genes at density 0.05 (two sliced
    gene tiles: the sliced row pass takes no more parts than it has gene tiles)."""
    c = dr.pin_case(K, 'gap', False, dr.PIN_M, TAIL_SPARSE_GENES)
    n, mt = dr.PIN_N, c['m']
    ct = eng.CountTiles.from_dense(np.array(c['X']), 'cuda', dense_density=0.1)
    assert ct.gd == dr.PIN_M and ct.ms == TAIL_SPARSE_GENES and ct.nrb == 2 and ct.ncb == 2
    ws = eng.ZWorkspace(ct, K)
    ws.dn_gene_splits, ws.dn_cell_splits = 1, 1
    ws.set_row_split(1, 2, None)
    assert ws.dense_tail(2) == (1, 2)
    o = [torch.empty(n, K, device='cuda'), torch.empty(mt, K, device='cuda')]
    eng.zq_gap(ws, o[0], o[1], dev(c['lu']), dev(c['lv']))
    torch.cuda.synchronize()
    assert ws.rows_nslab == 2 and ws.dense_tail(ws.rows_nslab) == (1, 2)
    f = launch_form(ws, ct, K)
    assert f['row_tiles'] == [5] and f['col_tiles'] == [10] and f['ncopy'] == NCOPY[f['kpad']], f
    assert int(ws.dn_flag.sum().item()) == 0 and int(ws.tile_flag.sum().item()) == 0
    out = [host(t) for t in o]
    judge('split-last-round', c, out, f, (1, 1), dict(row_split=[1, 2], tail_row_tiles=[2, 3]))
    conserved(c, out)
