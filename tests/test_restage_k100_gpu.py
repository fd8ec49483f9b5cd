# -*- coding: utf-8 -*-
"""The restaging of the sliced K = 85 .. 100 row kernel (csrc/passes_k100.h, k100::Stage: three address classes per thread, an
unpredicated full-tile path, a per-element path for the ragged tile) moves data only: k_row_pass_k100, and k_col_pass2 behind
it (k100::StageEach), must give the bits they gave before it.

Shapes: the smallest at which staging can go wrong, 256 x 256 tiles, sliced layout only, no gene or cell ordering (packed
position = position in X): genes 256 (one full tile), 257 (full + one gene), 511, 2 * 256 + 37; cells 256, 257, 2 * 256 + 40;
K = 96 (no tail chunk), 97 and 100 (tail chunk), 85 (Kp = 96 with padding).  Every gene count meets every K; the cell counts
rotate, so both ragged directions meet (257 x 257, 552 x 549, ...).  Beside them one HYBRID case (32 dense genes: the sliced
kernels' FV / C base is advanced by the dense rows) and one with a FORCED row split (row blocks 1, 2 cut into the gene-tile
ranges [0, 2), [2, 3): part work-groups start at gene tile 2).
Inputs: log-factors drawn as a shuffled grid, so every entry of FU / FV is distinct (a misplaced chunk or row cannot cancel);
every row has a count in every gene tile it meets and every gene one in every row block.
Checks: Z_i, Z_j through the C ABI (engine.zq) against the C oracle nest at the tolerance tests/test_kernels_gpu.py and
tests/test_trim_last_iteration_gpu.py use for the same entries -- a CPU test shows the oracle itself is inside it on exactly
these inputs --, and BITWISE against arrays recorded on an MI355X from the parent commit 74b4ffb (before the change) by
tools/record_restage_goldens.py (tests/golden/restage_k100/<case>.npz): Z_i of both modes, Z_j of the deterministic mode
(engine.set_deterministic: the float atomics of the default mode add in any order; in the hybrid case the rows of the sliced
genes, the dense genes' rows being the dense-gene kernels' atomics in either mode)."""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, err_colrel

RTOL = 1e-5          # tests/test_kernels_gpu.py, tests/test_trim_last_iteration_gpu.py: the same entries, the same oracle
TILE = 256
GENES = [256, 257, 511, 2 * TILE + 37]
CELLS = [256, 257, 2 * TILE + 40]
KS = [96, 97, 100, 85]
DENSE = 32

# name -> (cells, genes, K, dense genes, row split (nfull, parts, edges) or None = every row block whole)
CASES = {}
for _gi, _m in enumerate(GENES):
    for _ki, _K in enumerate(KS):
        CASES['n%d_m%d_K%d' % (CELLS[(_gi + _ki) % 3], _m, _K)] = (CELLS[(_gi + _ki) % 3], _m, _K, 0, None)
CASES['hybrid_n257_m%d_K100' % (DENSE + 293)] = (257, DENSE + 293, 100, DENSE, None)       # sliced genes: 256 + 37
CASES['split_n552_m549_K100'] = (552, 549, 100, 0, (1, 2, [0, 2, 3]))
CASES['split_n552_m549_K96'] = (552, 549, 96, 0, (1, 2, [0, 2, 3]))
GOLDEN_DIR = os.path.join(GOLDEN, 'restage_k100')


def build_counts(n, m, dense, seed):
    """(n, m) counts, about 4 % non-zero, plus one count per (row, gene tile) and per (gene, row block); the first `dense` genes
    are expressed in every cell."""
    rng = np.random.default_rng(seed)
    X = ((rng.poisson(3.0, size=(n, m)) + 1) * (rng.random((n, m)) < 0.04)).astype(np.int64)
    ms = m - dense                                                   # the sliced genes [dense, m): tiles count from `dense`
    for cb in range((ms + TILE - 1) // TILE):
        c0 = dense + cb * TILE
        w = min(TILE, m - c0)
        X[np.arange(n), c0 + (np.arange(n) * 7 + cb) % w] += 1 + (np.arange(n) % 3)
    for rb in range((n + TILE - 1) // TILE):
        r0 = rb * TILE
        h = min(TILE, n - r0)
        X[r0 + (np.arange(m) * 5 + rb) % h, np.arange(m)] += 1 + (np.arange(m) % 2)
    if dense:
        X[:, :dense] = rng.poisson(4.0, size=(n, dense)) + 1
    return X


def distinct_grid(rng, rows, K):
    """(rows, K) float32 in [-1.5, 1.5]: a shuffled grid, every value once."""
    v = np.linspace(-1.5, 1.5, rows * K).astype(np.float32)
    return np.ascontiguousarray(rng.permutation(v).reshape(rows, K))


@functools.lru_cache(maxsize=None)
def inputs(name):
    n, m, K, dense, _ = CASES[name]
    seed = sorted(CASES).index(name)
    rng = np.random.default_rng(1000 + seed)
    return dict(X=build_counts(n, m, dense, seed), lu=distinct_grid(rng, n, K), lv=distinct_grid(rng, m, K))


@functools.lru_cache(maxsize=None)
def oracle(name):
    from oracle import cavi_oracle as co
    a = inputs(name)
    n, K = a['lu'].shape
    m = a['lv'].shape[0]
    r = [np.empty((n, K), np.float32), np.empty((m, K), np.float32)]
    co.zq_gap(r[0], r[1], a['lu'], a['lv'], np.ascontiguousarray(a['X'].astype(np.float32)))
    return r


def test_cases_cover_the_shapes():
    """CPU: every gene count meets every K, every cell count occurs, both ragged directions meet; the inputs are what the
    module docstring says."""
    plain = [c for c in CASES.values() if not c[3] and c[4] is None]
    assert {(c[1], c[2]) for c in plain} == {(m, K) for m in GENES for K in KS}
    assert {c[0] for c in plain} == set(CELLS)
    assert any(c[0] % TILE and c[1] % TILE for c in plain)
    assert any(c[3] == DENSE for c in CASES.values()) and any(c[4] is not None for c in CASES.values())
    for name, (n, m, K, dense, _) in CASES.items():
        a = inputs(name)
        X = a['X']
        assert X.shape == (n, m) and a['lu'].shape == (n, K) and a['lv'].shape == (m, K)
        for f in (a['lu'], a['lv']):                                  # distinct, and still distinct as factors exp(. - max)
            assert np.unique(f).size == f.size
            assert np.unique(np.exp(f - f.max()).astype(np.float32)).size == f.size
        for c0 in range(dense, m, TILE):
            assert ((X[:, c0:c0 + TILE] != 0).sum(1) > 0).all(), name
        for r0 in range(0, n, TILE):
            assert ((X[r0:r0 + TILE] != 0).sum(0) > 0).all(), name
        if dense:
            assert (X[:, :dense] != 0).all() and ((X[:, dense:] != 0).mean(0) < 0.5).all()


@pytest.mark.parametrize('name', sorted(CASES))
def test_oracle_alone_within_tolerance(name):
    """CPU: the float32 oracle nest itself is within the tolerance of the float64 evaluation of the same statements on exactly
    these inputs, so the tolerance is a fair one to ask of the kernels there."""
    from oracle import cavi_oracle as co
    a = inputs(name)
    exact = co.zq_exact(a['lu'], a['lv'], a['X'], quirk=False)
    for what, got, ex in zip(('Z_i', 'Z_j'), oracle(name), exact):
        e = err_colrel(got, ex)
        print('%s %s: oracle vs float64 %.3e' % (name, what, e))
        assert e < RTOL, what


def run(eng, name, deterministic):
    """[Z_i, Z_j] of the loop nest on the GPU through the C ABI (engine.zq: oriana_row_pass_general, oriana_fixup,
    oriana_col_pass[_det]; the dense-gene entries beside them in the hybrid case), and the workspace."""
    n, m, K, dense, split = CASES[name]
    a = inputs(name)
    c = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    ct = eng.CountTiles.from_dense(a['X'], 'cuda', sort_cols=False, dense_density=0.9 if dense else None)
    assert ct.row_perm is None and ct.gd == dense and (ct.dense is not None) == bool(dense)
    assert dense or ct.col_perm is None
    if dense:                  # the packed genes [0, dense) are the caller's first `dense` genes: rows [dense:] of Z_j are the sliced genes'
        assert sorted(ct.col_perm[:dense].cpu().tolist()) == list(range(dense))
    ws = eng.ZWorkspace(ct, K)
    ws.set_row_split(*(split if split is not None else (ct.nrb, 1, [0, ct.ncb])))
    Zi = torch.empty(n, K, device='cuda'); Zj = torch.empty(m, K, device='cuda')
    eng.set_deterministic(deterministic)
    try:
        eng.zq(ws, Zi, Zj, None, c(a['lu']), c(a['lv']))
        torch.cuda.synchronize()
    finally:
        eng.set_deterministic(False)
    return [Zi.cpu().numpy(), Zj.cpu().numpy()], ws


@pytest.fixture(scope='module')
def eng():
    from oriana_amd import engine
    assert torch.cuda.is_available()
    return engine


@pytest.mark.gpu
@pytest.mark.parametrize('deterministic', [False, True], ids=['atomics', 'partials'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_restaged_passes_keep_their_bits(eng, name, deterministic):
    K, dense = CASES[name][2:4]
    got, ws = run(eng, name, deterministic)
    assert eng._lib.load().oriana_col_block_tiles(K) == 2            # the two-tile column kernel
    assert int(ws.tile_flag.sum().item()) == 0                       # everything on the fast path: the kernels' own sums
    for what, g, r in zip(('Z_i', 'Z_j'), got, oracle(name)):
        e = err_colrel(g, r)
        print('%s %s %s: %.3e' % (name, 'partials' if deterministic else 'atomics', what, e))
        assert e < RTOL, what
    gold = np.load(os.path.join(GOLDEN_DIR, name + '.npz'))
    assert got[0].tobytes() == gold['Z_i'].tobytes(), 'Z_i differs from the parent commit\'s bits'
    if deterministic:
        # (the sliced genes' rows: those of the dense genes are the dense-gene kernels' float atomics in either mode)
        assert got[1][dense:].tobytes() == gold['Z_j_det'].tobytes(), 'Z_j (deterministic mode) differs from the parent commit\'s bits'
