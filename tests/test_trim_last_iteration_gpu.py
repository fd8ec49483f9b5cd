# -*- coding: utf-8 -*-
"""The sliced passes do not issue the all-padding steps of a slice's final iteration (csrc/passes_k100.h): constructed
counts that put every remainder of the longest row / column (mod 4) in front of the row kernel k_row_pass_k100 and the
two-tile column kernel k_col_pass2, through the C ABI, against the C oracle nest (oracle/zq_kernels.c) at the tolerance
tests/test_kernels_gpu.py uses for the same entries.

Layout of a constructed matrix (no gene or cell ordering: packed position = position in X), 256 x 256 tiles:
  * row blocks 0, 1 x gene tiles 0, 1: the two 16-row slices of wave w hold longest rows of 4 i0 + a and 4 i1 + b entries;
    (a, b) runs over all 16 pairs of {0..3}^2 across the 8 waves of the two tiles, (i0, i1) are equal for some waves and
    different for others (the wave then runs max(i0, i1) iterations and the shorter slice is dead in the last ones);
  * the partial last gene tile: a wave with one empty slice (either half), a wave with two empty slices, one-entry rows;
  * the partial last row block: a single-entry tile, a tile with no entry, a tile that is partial both ways.
The transposed construction gives the column slices (one wave each, both tiles of a pair) the same cases."""
import functools

import numpy as np
import pytest
import torch

from helpers import err_colrel

RTOL = 1e-5          # tests/test_kernels_gpu.py: RTOL of the same entries against the same oracle
TILE = 256
N_ROWS, N_COLS = 2 * TILE + 40, 2 * TILE + 37


def _slice_lengths(rb, cb, last_rb, last_cb):
    """Longest row of each of the 16 slices of tile (rb, cb)."""
    if rb == last_rb:
        if cb == 0:
            return None                                   # single-entry tile (placed by the caller)
        if cb == 1:
            return [0] * 16                               # tile with no entry
        return [6, 3, 2] + [0] * 13                       # partial both ways
    if cb == last_cb:                                     # empty slices beside live ones, an empty wave, one-entry rows
        return [0, 5, 7, 0, 0, 0, 1, 1, 2, 9, 4, 3, 8, 8, 1, 0]
    lens = []
    for w in range(8):
        a, b = divmod(8 * cb + w, 4)
        i0, i1 = 1 + (w + rb) % 3, 1 + 2 * ((w + rb) % 2)
        lens += [4 * i0 + a, 4 * i1 + b]
    return lens


def build_rows(nr, nc, seed):
    """(nr, nc) counts whose ROW slices hold the cases of the module docstring."""
    rng = np.random.default_rng(seed)
    X = np.zeros((nr, nc), np.int64)
    nrb, ncb = (nr + TILE - 1) // TILE, (nc + TILE - 1) // TILE
    for rb in range(nrb):
        for cb in range(ncb):
            width = min(TILE, nc - cb * TILE)
            lens = _slice_lengths(rb, cb, nrb - 1, ncb - 1)
            if lens is None:
                X[rb * TILE + 8, cb * TILE + 3] = 5
                continue
            for sl, L in enumerate(lens):
                rows = [r for r in range(rb * TILE + sl * 16, rb * TILE + sl * 16 + 16) if r < nr]
                if not rows or L == 0:
                    continue
                L = min(L, width)
                longest = rows[(sl * 5) % len(rows)]
                for r in rows:
                    k = L if r == longest else int(rng.integers(0, L + 1))
                    cols = cb * TILE + rng.choice(width, size=k, replace=False)
                    X[r, cols] = rng.poisson(3.0, size=k) + 1
    return X


@functools.lru_cache(maxsize=None)
def problem(side):
    """side 'rows': the cases sit in the row slices (row kernel); 'cols': in the column slices (column kernel)."""
    X = build_rows(N_ROWS, N_COLS, 1) if side == 'rows' else np.ascontiguousarray(build_rows(N_COLS, N_ROWS, 2).T)
    assert X.shape == (N_ROWS, N_COLS)
    return X


def longest_per_slice(X):
    """[row block][gene tile][slice] longest row of the slice inside the tile."""
    n, m = X.shape
    nrb, ncb = (n + TILE - 1) // TILE, (m + TILE - 1) // TILE
    nz = np.zeros((nrb * TILE, ncb * TILE), bool)
    nz[:n, :m] = X != 0
    cnt = nz.reshape(nrb, TILE, ncb, TILE).sum(3)                      # [rb][row][cb]
    return cnt.reshape(nrb, 16, 16, ncb).max(2).transpose(0, 2, 1)    # [rb][cb][slice]


def test_constructed_counts_hold_the_cases():
    """CPU: the construction really contains what the module docstring lists, on the row side and (transposed) on the column
    side."""
    for side in ('rows', 'cols'):
        X = problem(side)
        L = longest_per_slice(X if side == 'rows' else np.ascontiguousarray(X.T))
        nrb, ncb = L.shape[:2]
        assert (nrb, ncb) == (3, 3)
        for rb in (0, 1):                                 # (the split row blocks of the last-round test hold them too)
            pairs, same, diff = set(), 0, 0
            for cb in (0, 1):
                for w in range(8):
                    l0, l1 = int(L[rb, cb, 2 * w]), int(L[rb, cb, 2 * w + 1])
                    assert l0 > 0 and l1 > 0
                    pairs.add((l0 % 4, l1 % 4))
                    same += ((l0 + 3) // 4 == (l1 + 3) // 4); diff += ((l0 + 3) // 4 != (l1 + 3) // 4)
            assert pairs == {(a, b) for a in range(4) for b in range(4)}
            assert same > 0 and diff > 0
            assert {int(v) % 4 for v in L[rb, 0]} | {int(v) % 4 for v in L[rb, 1]} == {0, 1, 2, 3}
            last = L[rb, 2]
            assert any(last[2 * w] == 0 and last[2 * w + 1] > 0 for w in range(8))
            assert any(last[2 * w] > 0 and last[2 * w + 1] == 0 for w in range(8))
            assert any(last[2 * w] == 0 and last[2 * w + 1] == 0 for w in range(8))
        Xs = X if side == 'rows' else X.T
        assert (Xs[2 * TILE:, :TILE] != 0).sum() == 1     # single-entry tile
        assert (Xs[2 * TILE:, TILE:2 * TILE] != 0).sum() == 0      # tile with no entry
        assert (Xs[2 * TILE:, 2 * TILE:] != 0).sum() > 1  # partial last row block x partial last gene tile


@functools.lru_cache(maxsize=None)
def _inputs(side, K, form):
    X = problem(side)
    n, m = X.shape
    rng = np.random.default_rng(K + len(form))
    a = dict(X=X, lu=rng.normal(size=(n, K)).astype(np.float32), lv=rng.normal(size=(m, K)).astype(np.float32),
             D=None, St=None, Sh=None)
    if 'weighted' in form:
        a['D'] = (0.25 + 0.75 * rng.random((n, m))).astype(np.float32)
    if 'srow' in form:
        ps = rng.random((m, K))
        a['St'] = (ps > 0.3).astype(np.float32); a['Sh'] = ps.astype(np.float32)
    return a


@functools.lru_cache(maxsize=None)
def _oracle(side, K, form):
    from oracle import cavi_oracle as co
    a = _inputs(side, K, form)
    n, K = a['lu'].shape
    m = a['lv'].shape[0]
    Xf = np.ascontiguousarray(a['X'].astype(np.float32))
    r = [np.empty((n, K), np.float32), np.empty((m, K), np.float32), np.empty((m, K), np.float32)]
    if a['St'] is not None and a['D'] is not None:
        co.zq_sparse_zigap(r[0], r[1], r[2], a['lu'], a['lv'], a['St'], a['Sh'], a['D'], Xf)
    elif a['St'] is not None:
        co.zq_sparse_gap(r[0], r[1], r[2], a['lu'], a['lv'], a['St'], a['Sh'], Xf)
    elif a['D'] is not None:
        co.zq_zigap(r[0], r[1], r[2], a['lu'], a['lv'], a['D'], Xf, quirk=False)
    else:
        co.zq_gap(r[0], r[1], a['lu'], a['lv'], Xf)
        r[2] = None
    return r


FORMS = ['plain', 'weighted', 'srow', 'srow+weighted']     # the four variants of the row kernel (weights, row-side s)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('K', [100, 96])
@pytest.mark.parametrize('side', ['rows', 'cols'])
def test_oracle_alone_within_tolerance(side, K, form):
    """CPU: the float32 oracle nest itself is within the tolerance of the float64 evaluation of the same statements on every
    constructed problem, so the tolerance is a fair one to ask of the kernels there."""
    from oracle import cavi_oracle as co
    a = _inputs(side, K, form)
    ref = _oracle(side, K, form)
    exact = co.zq_exact(a['lu'], a['lv'], a['X'], S_tilde=a['St'], S_hat=a['Sh'], D_hat=a['D'], quirk=False)
    for name, got, ex in zip(('Z_i', 'Z_j', 'Z_log'), ref, exact):
        if got is not None:
            e = err_colrel(got, ex)
            print('%s %s K=%d %s: oracle vs float64 %.3e' % (side, form, K, name, e))
            assert e < RTOL, name


def _run(eng, a, K, split=None, deterministic=False):
    """The loop nest on the GPU through the C ABI (engine.zq: oriana_row_pass_general, oriana_fixup, oriana_col_pass[_det])."""
    X = a['X']
    n, m = X.shape
    c = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()
    ct = eng.CountTiles.from_dense(X, 'cuda', side=c(a['D']), sort_cols=False)
    assert ct.col_perm is None and ct.row_perm is None and ct.dense is None
    ws = eng.ZWorkspace(ct, K)
    if split is not None:
        ws.set_row_split(*split)
    plain = a['D'] is None and a['St'] is None
    Zi = torch.empty(n, K, device='cuda'); Zj = torch.empty(m, K, device='cuda')
    Zl = None if plain else torch.empty(m, K, device='cuda')
    eng.set_deterministic(deterministic)
    try:
        eng.zq(ws, Zi, Zj, Zl, c(a['lu']), c(a['lv']), S_tilde=c(a['St']), S_hat=c(a['Sh']),
               w_nz=ct.side_nz if a['D'] is not None else None)
        torch.cuda.synchronize()
    finally:
        eng.set_deterministic(False)
    return [Zi.cpu().numpy(), Zj.cpu().numpy(), None if Zl is None else Zl.cpu().numpy()], ws


@pytest.fixture(scope='module')
def eng():
    from oriana_amd import engine
    assert torch.cuda.is_available()
    return engine


# the plan's own split; every row block whole; the last round split: row blocks 1, 2 cut into the gene-tile ranges [0, 2), [2, 3)
SPLITS = {'planned': None, 'whole': (3, 1, [0, 3]), 'last_round': (1, 2, [0, 2, 3])}


@pytest.mark.gpu
@pytest.mark.parametrize('split', sorted(SPLITS))
@pytest.mark.parametrize('deterministic', [False, True], ids=['atomics', 'partials'])
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('K', [100, 96])
@pytest.mark.parametrize('side', ['rows', 'cols'])
def test_trimmed_passes_match_the_oracle(eng, side, K, form, deterministic, split):
    a = _inputs(side, K, form)
    got, ws = _run(eng, a, K, split=SPLITS[split], deterministic=deterministic)
    assert eng._lib.load().oriana_col_block_tiles(K) == 2           # the two-tile column kernel
    assert int(ws.tile_flag.sum().item()) == 0                      # everything on the fast path: the kernels' own sums
    ref = _oracle(side, K, form)
    for name, g, r in zip(('Z_i', 'Z_j', 'Z_log'), got, ref):
        if r is not None:
            e = err_colrel(g, r)
            print('%s K=%d %s %s %s %s: %.3e' % (side, K, form, 'partials' if deterministic else 'atomics', split, name, e))
            assert e < RTOL, name
    if form == 'plain':                                             # responsibilities sum to the counts
        np.testing.assert_allclose(got[0].sum(1), a['X'].sum(1), rtol=2e-5, atol=1e-3)
        np.testing.assert_allclose(got[1].sum(1), a['X'].sum(0), rtol=2e-5, atol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('K', [100, 96])
@pytest.mark.parametrize('side', ['rows', 'cols'])
def test_deterministic_runs_are_bit_identical(eng, side, K, form, monkeypatch):
    """The same constructed problem twice under ORIANA_DETERMINISTIC=1 (engine.DETERMINISTIC is what the variable sets):
    identical bits in every output."""
    monkeypatch.setenv('ORIANA_DETERMINISTIC', '1')
    a = _inputs(side, K, form)
    first, _ = _run(eng, a, K, split=SPLITS['last_round'], deterministic=True)
    second, _ = _run(eng, a, K, split=SPLITS['last_round'], deterministic=True)
    for x, y in zip(first, second):
        if x is not None:
            assert x.tobytes() == y.tobytes()
