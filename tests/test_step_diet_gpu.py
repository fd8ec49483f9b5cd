# -*- coding: utf-8 -*-
"""The per-step bookkeeping of the sliced K = 85..100 passes (csrc/passes_k100.h, "step diet"): the row kernel
k_row_pass_k100 forms s without a test of x, records the den test as a wave mask and writes the NaN of a slow entry after
the iteration, off the hot path; both kernels form a read's address in one instruction.  One small pCMF problem that
takes every path of the change, through the C ABI, against the C oracle nest (oracle/zq_kernels.c) at the tolerance
tests/test_kernels_gpu.py asks of the same kernels.

The counts (600 x 700, 3 x 3 tiles of 256 x 256, no gene or cell ordering: packed position = position in X):
  * density 0.1; row 10 and gene 20 are empty; tile (row block 1, gene tile 1) holds no entry at all;
  * row block 0 is full, row block 2 holds 88 rows (rows beyond n: den == 0 in every step of their lanes), the last gene
    tile is partial;
  * row 0 holds 60 entries in gene tile 0, so the two slices of wave 0 differ by at least two iterations;
  * the longest rows of the slices cover every remainder mod 4.
The stored s is not compared entry by entry (the oracle does not return it): Z_j is the column pass over exactly that s, and
after the slow path no stored s may be a NaN.  No record field changed, so there is no pack-time layout to check."""
import functools

import numpy as np
import pytest
import torch

from helpers import err_colrel

RTOL = 1e-5          # tests/test_kernels_gpu.py: RTOL of the same entries against the same oracle
TILE = 256
N, M = 600, 700
KS = [85, 96, 100]
SLOW_ROWS = [3] + list(range(TILE + 32, TILE + 48))     # one cell of row block 0; ALL of slice 2 of row block 1: den tiny in every slot


@functools.lru_cache(maxsize=None)
def counts():
    rng = np.random.default_rng(11)
    X = (rng.random((N, M)) < 0.1) * rng.integers(1, 40, size=(N, M))
    X[10, :] = 0
    X[:, 20] = 0
    X[TILE:2 * TILE, TILE:2 * TILE] = 0
    X[0, :60] = rng.integers(1, 40, size=60)
    X[0, 20] = 0
    return np.ascontiguousarray(X.astype(np.int64))


def longest_per_slice(X):
    """[row block][gene tile][slice] longest row of the slice inside the tile."""
    n, m = X.shape
    nrb, ncb = (n + TILE - 1) // TILE, (m + TILE - 1) // TILE
    nz = np.zeros((nrb * TILE, ncb * TILE), bool)
    nz[:n, :m] = X != 0
    cnt = nz.reshape(nrb, TILE, ncb, TILE).sum(3)
    return cnt.reshape(nrb, 16, 16, ncb).max(2).transpose(0, 2, 1)


def test_counts_hold_the_cases():
    """CPU: the construction contains what the module docstring lists."""
    X = counts()
    assert X.shape == (N, M) and 0.08 < (X != 0).mean() < 0.12
    assert not X[10].any() and not X[:, 20].any() and not X[TILE:2 * TILE, TILE:2 * TILE].any()
    L = longest_per_slice(X)
    assert L.shape == (3, 3, 16)
    assert {int(v) % 4 for v in L.ravel()} == {0, 1, 2, 3}
    it = (L + 3) // 4
    assert it[0, 0, 0] - it[0, 0, 1] >= 2                  # wave 0 of tile (0, 0): slices two iterations apart
    assert (L[1, 1] == 0).all() and (L[2, :, 6:] == 0).all() and (L[2, :, :5] > 0).all()


@functools.lru_cache(maxsize=None)
def inputs(K, form, slow):
    X = counts()
    rng = np.random.default_rng(100 + K)
    a = dict(X=X, lu=rng.normal(size=(N, K)).astype(np.float32), lv=rng.normal(size=(M, K)).astype(np.float32),
             D=None, St=None, Sh=None)
    if slow:
        a['lu'][SLOW_ROWS] -= np.float32(80.0)             # (as tests/test_kernels_gpu.py puts a cell on the exact slow path)
    if 'weighted' in form:
        a['D'] = (0.25 + 0.75 * rng.random((N, M))).astype(np.float32)
    if 'srow' in form:
        ps = rng.random((M, K))
        a['St'] = (ps > 0.3).astype(np.float32); a['Sh'] = ps.astype(np.float32)
    return a


@functools.lru_cache(maxsize=None)
def oracle(K, form, slow):
    from oracle import cavi_oracle as co
    a = inputs(K, form, slow)
    Xf = np.ascontiguousarray(a['X'].astype(np.float32))
    r = [np.empty((N, K), np.float32), np.empty((M, K), np.float32), np.empty((M, K), np.float32)]
    if a['St'] is not None and a['D'] is not None:
        co.zq_sparse_zigap(r[0], r[1], r[2], a['lu'], a['lv'], a['St'], a['Sh'], a['D'], Xf)
    elif a['St'] is not None:
        co.zq_sparse_gap(r[0], r[1], r[2], a['lu'], a['lv'], a['St'], a['Sh'], Xf)
    elif a['D'] is not None:
        co.zq_zigap(r[0], r[1], r[2], a['lu'], a['lv'], a['D'], Xf, quirk=False)
    else:
        co.zq_gap_nz(r[0], r[1], a['lu'], a['lv'], Xf)
        r[2] = None
    return r


@pytest.fixture(scope='module')
def eng():
    from oriana_amd import engine
    assert torch.cuda.is_available()
    return engine


def run(eng, a, K):
    """The loop nest on the GPU through the C ABI (engine.zq: row pass, slow path, column pass)."""
    c = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()
    ct = eng.CountTiles.from_dense(a['X'], 'cuda', side=c(a['D']), sort_cols=False)
    assert ct.col_perm is None and ct.row_perm is None and ct.dense is None
    ws = eng.ZWorkspace(ct, K)
    plain = a['D'] is None and a['St'] is None
    Zi = torch.empty(N, K, device='cuda'); Zj = torch.empty(M, K, device='cuda')
    Zl = None if plain else torch.empty(M, K, device='cuda')
    eng.zq(ws, Zi, Zj, Zl, c(a['lu']), c(a['lv']), S_tilde=c(a['St']), S_hat=c(a['Sh']),
           w_nz=ct.side_nz if a['D'] is not None else None)
    torch.cuda.synchronize()
    return [Zi.cpu().numpy(), Zj.cpu().numpy(), None if Zl is None else Zl.cpu().numpy()], ws, ct


def check(got, ref, what):
    for name, g, r in zip(('Z_i', 'Z_j', 'Z_log'), got, ref):
        if r is not None:
            e = err_colrel(g, r)
            print('%s %s: %.3e' % (what, name, e))
            assert np.isfinite(g).all(), name
            assert e < RTOL, name


@pytest.mark.gpu
@pytest.mark.parametrize('K', KS)
def test_plain_nest_matches_the_oracle_and_conserves_the_counts(eng, K):
    a = inputs(K, 'plain', False)
    got, ws, ct = run(eng, a, K)
    assert int(ws.tile_flag.sum().item()) == 0                      # everything on the fast path
    check(got, oracle(K, 'plain', False), 'K=%d plain' % K)
    assert bool(torch.isfinite(ws.s_cs).all())
    np.testing.assert_allclose(got[0].sum(1), a['X'].sum(1), rtol=2e-5, atol=1e-3)     # responsibilities sum to the counts
    np.testing.assert_allclose(got[1].sum(1), a['X'].sum(0), rtol=2e-5, atol=1e-3)
    assert not got[0][10].any() and not got[1][20].any()            # the empty row, the empty gene


@pytest.mark.gpu
@pytest.mark.parametrize('form', ['weighted', 'srow', 'srow+weighted'])
def test_weighted_and_row_side_variants_match_the_oracle(eng, form):
    a = inputs(100, form, False)
    got, ws, ct = run(eng, a, 100)
    check(got, oracle(100, form, False), 'K=100 ' + form)


@pytest.mark.gpu
@pytest.mark.parametrize('K,form', [(85, 'plain'), (96, 'plain'), (100, 'plain'), (100, 'weighted'), (100, 'srow')])
def test_slow_entries_flag_their_tiles_and_are_repaired(eng, K, form):
    """Cell 3 and the sixteen cells of one slice of row block 1 sit 80 below the rest: den < den_min at each of their entries
    AND at each padding slot of that slice (every lane of its half wave fails the den test in every step).  Flagged: exactly
    the tiles in which one of those cells has an entry (not the empty tile of row block 1, not row block 2, whose rows beyond
    n have den == 0); after the slow path the outputs are the oracle's and no NaN is left in s or Z_j."""
    a = inputs(K, form, True)
    got, ws, ct = run(eng, a, K)
    nz = a['X'] != 0
    expect = np.zeros((ct.nrb, ct.ncb), bool)
    for r in SLOW_ROWS:
        for cb in range(ct.ncb):
            expect[r // TILE, cb] |= bool(nz[r, cb * TILE:(cb + 1) * TILE].any())
    assert expect[0].all() and expect[1, 0] and not expect[1, 1] and expect[1, 2] and not expect[2].any()
    flags = ws.tile_flag[:ct.nrb * ct.ncb].cpu().numpy().reshape(ct.nrb, ct.ncb) != 0
    print('K=%d %s flags' % (K, form), flags.astype(int).tolist())
    assert (flags == expect).all(), flags
    check(got, oracle(K, form, True), 'K=%d %s slow' % (K, form))
    assert bool(torch.isfinite(ws.s_cs).all())
    if form == 'plain':
        np.testing.assert_allclose(got[1].sum(1), a['X'].sum(0), rtol=2e-5, atol=1e-3)
