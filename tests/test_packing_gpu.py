# -*- coding: utf-8 -*-
"""Every route into the packed count layout, bit for bit against tests/packing_reference.py (a NumPy restatement of
include/oriana_hip.h and DESIGN.md section 3): the chunked route of CountTiles.from_dense (row chunks past the first: rb0,
the dense block's first cell tile, the per-chunk cell order, the side matrix), SciPy inputs in every format (and that they are
only read), the second grid launch of the packers (more than 65535 row blocks in one chunk) and the two untested shapes of
the resident C handle (ldx > m; CSR that is not canonical); the steps every host shares (oriana_pack_offsets,
oriana_plan_inputs) against NumPy and from_chunks against from_dense (one builder).  Everything is exact but the comparisons with the oracle's
loop nest, which use helpers.RTOL.  GPU only."""
import ctypes

import numpy as np
import pytest
import torch

import helpers
import packing_reference as pr
from helpers import err_colrel

pytestmark = pytest.mark.gpu

TILE = 256


@pytest.fixture(scope='module')
def eng():
    from oriana_amd import engine
    assert torch.cuda.is_available()
    return engine


def _layout(ct):
    """Everything the kernels read of a CountTiles, as host arrays."""
    h = ct.host_arrays()
    out = dict(rec=h['rec'].view(np.int64), ridx=h['ridx'], rslice=h['rslice'], cslice=h['cslice'], roff=h['roff'], coff=h['coff'],
               tile_nnz=ct.tile_nnz.cpu().numpy(),
               scalars=np.array([ct.n, ct.m, ct.nrb, ct.ncb, ct.nnz, ct.nnz_sparse, ct.rslots, ct.cslots, ct.gd], dtype=np.int64),
               col_perm=ct.col_perm.cpu().numpy() if ct.col_perm is not None else np.zeros(0, np.int32),
               row_perm=ct.row_perm.cpu().numpy() if ct.row_perm is not None else np.zeros(0, np.int32),
               dense=ct.dense.x.cpu().numpy() if ct.dense is not None else np.zeros(0, np.uint16))
    if ct.side_nz is not None:
        out['side_nz'] = ct.side_nz.cpu().numpy().view(np.uint32)
    return out


def _assert_same_layout(a, b, what=''):
    la, lb = _layout(a), _layout(b)
    assert la.keys() == lb.keys(), what
    for k in la:
        assert la[k].dtype == lb[k].dtype and la[k].shape == lb[k].shape and np.array_equal(la[k], lb[k]), (what, k)


def _assert_reference_layout(ct, X, dense_density, chunk_rows, sort_rows, D=None):
    """ct against the reference layout of X (the array handed to the packer), byte for byte."""
    X32 = np.asarray(X).astype(np.float32)
    n, m = X32.shape
    cp, gd = pr.expected_gene_order(X, dense_density)
    rp = pr.expected_row_perm(X32, chunk_rows) if sort_rows else None
    L = pr.expected_layout(X32, cp, rp, gd)
    got = _layout(ct)
    assert ct.gd == gd and np.array_equal(got['col_perm'], cp) and got['col_perm'].dtype == np.int32
    if sort_rows:
        assert got['row_perm'].dtype == np.int32 and np.array_equal(got['row_perm'], rp)
    else:
        assert ct.row_perm is None
    assert (ct.nrb, ct.ncb) == (L['nrb'], L['ncb'])
    assert ct.nnz == int(np.count_nonzero(X32)) and ct.nnz_sparse == L['nnz_sparse']
    assert ct.rslots == L['rslots'] and ct.cslots == L['cslots']
    for k in ('tile_nnz', 'rslice', 'cslice', 'roff', 'coff', 'ridx'):
        assert got[k].dtype == L[k].dtype and got[k].shape == L[k].shape and np.array_equal(got[k], L[k]), k
    # the records as 8-byte words: value, column-side slot, column AND the pad byte; padding slots are all-zero bytes
    assert np.array_equal(got['rec'], L['rec'].view(np.int64))
    if gd:
        assert np.array_equal(got['dense'], pr.expected_dense_block(X32, cp, rp, gd))
    else:
        assert ct.dense is None
    assert np.array_equal(pr.decode(ct), X32)
    if D is not None:
        want = np.zeros(max(L['rslots'], 1), dtype=np.float32)
        want[L['entry_slot']] = D[L['entry_cell'], L['entry_gene']]
        assert np.array_equal(got['side_nz'], want.view(np.uint32))             # D at every record, +0 at every other slot
    else:
        assert ct.side_nz is None
    return L


# ---- A. the chunked route of from_dense -----------------------------------------------------------------------------------
SPECIAL = dict(zero=1, full=2, wide=3, frac=4)      # genes: never expressed / expressed in every cell / a count of 70000 / a non-integer count


def _counts_a(n, m, dtype, hybrid):
    """Counts as _rand_counts (test_kernels_gpu.py) / _counts (test_dense_gpu.py): Poisson + 1 under a per-gene density,
    a few large outliers; an all-zero row block (n >= 512), an all-zero gene and a gene expressed in every other cell.
    Hybrid cases: enough genes above the density threshold, among them one with a count of 70000 and (floating-point
    input) one with a non-integer count, which must stay on the sliced side."""
    rng = np.random.default_rng(1000 * n + m)
    dens = np.clip(rng.beta(1.0, 3.0, size=m), 0.02, 1.0)
    if hybrid:
        dens[:min(m, 48)] = np.linspace(1.0, 0.35, min(m, 48))
    X = rng.poisson(3.0, size=(n, m)).astype(np.int64) + 1
    small = np.dtype(dtype) == np.uint8
    X[rng.random((n, m)) < 0.005] = 200 if small else 50000
    X *= rng.random((n, m)) < dens[None, :]
    X[:, SPECIAL['zero']] = 0
    X[:, SPECIAL['full']] = np.maximum(X[:, SPECIAL['full']], 1)
    if not small:
        X[:, SPECIAL['wide']] = 70000 * (rng.random(n) < 0.9)
    X = X.astype(np.float64)
    if np.dtype(dtype).kind == 'f':
        X[:, SPECIAL['frac']] = 2.5 * (rng.random(n) < 0.9)
    if n >= 2 * TILE:
        X[TILE:2 * TILE] = 0
    return np.ascontiguousarray(X.astype(dtype))


SHAPES_A = [(1000, 300), (513, 257), (256, 40), (257, 5)]
# (dtype, sort_rows, dense_density, side): every dtype, both row orders and the side matrix on the sliced layout; every dtype
# and both row orders on the hybrid one (which carries no side matrix)
OPTIONS_A = [(np.float32, False, None, False), (np.int64, True, None, False), (np.int32, False, None, True),
             (np.float64, True, None, True), (np.uint8, False, None, False),
             (np.float32, True, 0.2, False), (np.int64, False, 0.2, False), (np.int32, True, 0.2, False),
             (np.float64, False, 0.2, False), (np.uint8, True, 0.2, False)]


@pytest.mark.parametrize('dtype,sort_rows,dd,with_side', OPTIONS_A,
                         ids=lambda v: getattr(v, '__name__', None) or repr(v))
@pytest.mark.parametrize('n,m', SHAPES_A)
def test_from_dense_chunked_equals_reference_layout(eng, n, m, dtype, sort_rows, dd, with_side):
    X = _counts_a(n, m, dtype, hybrid=bool(dd))
    D = np.random.default_rng(n + m).random((n, m)).astype(np.float32) if with_side else None
    side = torch.from_numpy(D).cuda() if with_side else None
    whole = (n + TILE - 1) // TILE * TILE
    kw = dict(sort_rows=sort_rows, dense_density=dd, side=side)
    ct_chunks = eng.CountTiles.from_dense(X, 'cuda', chunk_bytes=1, **kw)          # 256-row chunks
    ct_one = eng.CountTiles.from_dense(X, 'cuda', **kw)
    _assert_reference_layout(ct_chunks, X, dd, TILE, sort_rows, D)
    _assert_reference_layout(ct_one, X, dd, whole, sort_rows, D)
    if dd and m >= 40:
        assert ct_chunks.gd >= 32
        dense_genes = ct_chunks.col_perm.cpu().numpy()[:ct_chunks.gd]
        if np.dtype(dtype) != np.uint8:
            assert (X[:, SPECIAL['wide']] != 0).mean() >= dd and SPECIAL['wide'] not in dense_genes
        if np.dtype(dtype).kind == 'f':
            assert (X[:, SPECIAL['frac']] != 0).mean() >= dd and SPECIAL['frac'] not in dense_genes
    if sort_rows:
        depth = (X != 0).sum(1)
        rp = ct_chunks.row_perm.cpu().numpy()
        for r0 in range(0, n, TILE):
            r1 = min(n, r0 + TILE)
            assert np.array_equal(rp[r0:r1], r0 + np.argsort(-depth[r0:r1], kind='stable'))
    else:
        _assert_same_layout(ct_chunks, ct_one)


@pytest.mark.parametrize('dtype,sort_rows,dd', [(np.int64, True, None), (np.float32, False, 0.2)], ids=['sliced', 'hybrid'])
def test_passes_follow_a_chunked_layout(eng, dtype, sort_rows, dd):
    """One responsibility pass over a layout packed in four chunks, as test_zq_gap_random judges it: the passes follow
    roff / coff (and the dense block's cell tiles) across the chunk boundaries."""
    from oracle import cavi_oracle as co
    n, m, K = 1000, 300, 20
    X = _counts_a(n, m, dtype, hybrid=bool(dd))
    rng = np.random.default_rng(5)
    lu = (rng.normal(size=(n, K)) * 2.0).astype(np.float32)
    lv = (rng.normal(size=(m, K)) * 2.0 + 1.0).astype(np.float32)
    ct = eng.CountTiles.from_dense(X, 'cuda', chunk_bytes=1, sort_rows=sort_rows, dense_density=dd)
    assert (ct.gd >= 32) == bool(dd)
    ws = eng.ZWorkspace(ct, K)
    Zi = torch.empty(n, K, dtype=torch.float32, device='cuda')
    Zj = torch.empty(m, K, dtype=torch.float32, device='cuda')
    eng.zq_gap(ws, Zi, Zj, torch.from_numpy(lu).cuda(), torch.from_numpy(lv).cuda())
    torch.cuda.synchronize()
    Zi, Zj = Zi.cpu().numpy(), Zj.cpu().numpy()
    rZi = np.empty((n, K), np.float32); rZj = np.empty((m, K), np.float32)
    co.zq_gap(rZi, rZj, lu, lv, np.ascontiguousarray(X.astype(np.float32)))
    print('err_colrel Z_i %.3e Z_j %.3e' % (err_colrel(Zi, rZi), err_colrel(Zj, rZj)))
    assert err_colrel(Zi, rZi) < helpers.RTOL
    assert err_colrel(Zj, rZj) < helpers.RTOL
    np.testing.assert_allclose(Zi.sum(1), X.sum(1), rtol=2e-5, atol=1e-3)
    np.testing.assert_allclose(Zj.sum(1), X.sum(0), rtol=2e-5, atol=1e-3)


# ---- B. SciPy inputs -------------------------------------------------------------------------------------------------------
N_B, M_B = 700, 300


def _dense_b():
    rng = np.random.default_rng(23)
    dens = np.full(M_B, 0.13)
    dens[:40] = np.linspace(1.0, 0.6, 40)                         # enough genes above the hybrid threshold
    X = (rng.poisson(3.0, size=(N_B, M_B)) + 1) * (rng.random((N_B, M_B)) < dens[None, :])
    X[300:560] = 0                                                # an empty row block
    return X.astype(np.float32)


def _triplets_with_duplicates(X, rng):
    """(row, col, value) in random order: entries >= 2 split into two that add up to them, plus explicit zeros on empty
    places (also one that shares its place with a real entry)."""
    r, c = np.nonzero(X)
    v = X[r, c].astype(np.float32)
    split = (v >= 2) & (rng.random(v.size) < 0.3)
    zr, zc = np.nonzero(X == 0)
    pick = rng.choice(zr.size, size=500, replace=False)
    rows = np.concatenate([r, r[split], zr[pick], r[:50]])
    cols = np.concatenate([c, c[split], zc[pick], c[:50]])
    vals = np.concatenate([np.where(split, v - 1, v), np.ones(int(split.sum()), np.float32), np.zeros(500 + 50, np.float32)])
    o = rng.permutation(rows.size)
    return rows[o], cols[o], vals[o]


def _raw_csr(rows, cols, vals, shape):
    """CSR straight from triplets, nothing summed or sorted inside the rows."""
    import scipy.sparse as sp
    o = np.argsort(rows, kind='stable')
    indptr = np.zeros(shape[0] + 1, dtype=np.int32)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=shape[0]))
    return sp.csr_matrix((vals[o], cols[o].astype(np.int32), indptr), shape=shape)


def _variants_b():
    import scipy.sparse as sp
    Xd = _dense_b()
    rng = np.random.default_rng(7)
    A = sp.csr_matrix(Xd)
    out = {'csr': A}
    r, c = np.nonzero(Xd)
    o = rng.permutation(r.size)
    out['csr_shuffled'] = _raw_csr(r[o], c[o], Xd[r[o], c[o]], Xd.shape)
    tr = _triplets_with_duplicates(Xd, rng)
    out['csr_duplicates_zeros'] = _raw_csr(*tr, Xd.shape)
    out['csc'] = sp.csc_matrix(Xd)
    out['coo_duplicates'] = sp.coo_matrix((tr[2], (tr[0], tr[1])), shape=Xd.shape)
    A64 = A.copy()
    A64.indptr, A64.indices = A64.indptr.astype(np.int64), A64.indices.astype(np.int64)
    out['csr_int64_indices'] = A64
    out['csr_int32_data'] = sp.csr_matrix((A.data.astype(np.int32), A.indices.copy(), A.indptr.copy()), shape=Xd.shape)
    out['csr_float64_data'] = sp.csr_matrix((A.data.astype(np.float64), A.indices.copy(), A.indptr.copy()), shape=Xd.shape)
    out['all_zero'] = sp.csr_matrix(Xd.shape, dtype=np.float32)
    assert out['csr'].has_canonical_format and not out['csr_shuffled'].has_sorted_indices
    assert not out['csr_duplicates_zeros'].has_canonical_format and out['csr_duplicates_zeros'].nnz > A.nnz + 500
    assert A64.indices.dtype == np.int64 and A64.indptr.dtype == np.int64
    for k, B in out.items():
        assert np.array_equal(np.asarray(B.todense()).astype(np.float32), Xd if k != 'all_zero' else 0 * Xd), k
    return out


VARIANTS_B = ['csr', 'csr_shuffled', 'csr_duplicates_zeros', 'csc', 'coo_duplicates', 'csr_int64_indices', 'csr_int32_data',
              'csr_float64_data', 'all_zero']


@pytest.fixture(scope='module')
def sparse_b(eng):
    """The variants and, per dense_density, the layout from_dense gives for the same counts (packed once)."""
    variants = _variants_b()
    dense = {}
    for name in ('csr', 'all_zero'):
        Xd = np.asarray(variants[name].todense()).astype(np.float32)
        for dd in (None, 0.2):
            dense[name, dd] = (Xd, eng.CountTiles.from_dense(Xd, 'cuda', dense_density=dd))
    assert dense['csr', 0.2][1].gd >= 32
    return variants, dense


def _arrays(A):
    names = ('row', 'col', 'data') if A.format == 'coo' else ('indptr', 'indices', 'data')
    return [getattr(A, k) for k in names]


class _Untouched:
    """The caller's sparse matrix before and after: the same array objects, byte for byte, and the same nnz."""

    def __init__(self, A):
        self.A, self.arrays, self.nnz = A, _arrays(A), A.nnz
        self.copies = [a.copy() for a in self.arrays]

    def check(self, what=''):
        now = _arrays(self.A)
        for a, b, c in zip(now, self.arrays, self.copies):
            assert a is b and a.dtype == c.dtype and a.shape == c.shape and a.tobytes() == c.tobytes(), what
        assert self.A.nnz == self.nnz, what


@pytest.mark.parametrize('dd', [None, 0.2], ids=['sliced', 'hybrid'])
@pytest.mark.parametrize('chunk_rows', [256, 8192])
@pytest.mark.parametrize('name', VARIANTS_B)
def test_from_scipy_equals_from_dense(eng, sparse_b, name, chunk_rows, dd):
    variants, dense = sparse_b
    A = variants[name]
    Xd, ct_d = dense['all_zero' if name == 'all_zero' else 'csr', dd]
    keep = _Untouched(A)
    ct = eng.CountTiles.from_scipy(A, 'cuda', chunk_rows=chunk_rows, dense_density=dd)
    keep.check(name)
    _assert_same_layout(ct, ct_d, name)
    assert ct.nnz == int(np.count_nonzero(Xd.astype(np.float32)))
    assert np.array_equal(pr.decode(ct), Xd)


@pytest.mark.parametrize('name', ['csr', 'csr_shuffled', 'csr_duplicates_zeros', 'coo_duplicates'])
def test_models_only_read_a_sparse_input(eng, sparse_b, name):
    """CountMatrix(A) keeps A itself when A is CSR, and GaP packs what it is given: neither may rewrite the user's matrix."""
    import oriana_amd.models as M
    from oriana_amd.singlecell import CountMatrix
    variants, dense = sparse_b
    A = variants[name]
    Xd, ct_d = dense['csr', None]
    rng = np.random.default_rng(3)
    a1 = rng.gamma(1.0, 1.0, size=(N_B, 5)); b1 = rng.gamma(1.0, 1.0, size=(M_B, 5))
    keep = _Untouched(A)
    ct = CountMatrix(A).to_tiles('cuda')
    keep.check('CountMatrix.to_tiles')
    _assert_same_layout(ct, ct_d)
    g = M.GaP(A, k=5, init=(a1, b1))
    keep.check('GaP(A)')
    _assert_same_layout(g.counts, ct_d)
    g = M.GaP(CountMatrix(A), k=5, init=(a1, b1))
    keep.check('GaP(CountMatrix(A))')
    _assert_same_layout(g.counts, ct_d)


def test_from_scipy_copies_only_what_it_must(eng, sparse_b, monkeypatch):
    """A CSR matrix in canonical format is packed from its own arrays; one that is not, from a copy."""
    import scipy.sparse as sp
    variants, _ = sparse_b
    copied = []
    orig = sp.csr_matrix.copy
    monkeypatch.setattr(sp.csr_matrix, 'copy', lambda self: (copied.append(self.nnz), orig(self))[1])
    eng.CountTiles.from_scipy(variants['csr'], 'cuda')
    eng.CountTiles.from_scipy(variants['csr_int64_indices'], 'cuda')
    assert copied == []
    eng.CountTiles.from_scipy(variants['csr_duplicates_zeros'], 'cuda')
    assert copied == [variants['csr_duplicates_zeros'].nnz]


# ---- C. more than 65535 row blocks in one chunk: the packers' second grid launch ---------------------------------------------
def test_second_grid_launch_of_the_packers(eng):
    """gridDim.y ends at 65535: a chunk of 65537 row blocks takes two launches of the counting and of the filling kernel,
    the second with pointers, row count, first row block and side matrix advanced by 65535 blocks.  One non-zero per 64
    rows, the 300 rows of the second launch dense."""
    nfirst = 65535
    n, m = nfirst * TILE + 300, 3
    rng = np.random.default_rng(65535)
    X = np.zeros((n, m), dtype=np.int32)
    rows = np.flatnonzero(rng.random(n) < 1.0 / 64)
    X[rows, rng.integers(0, m, size=rows.size)] = rng.integers(1, 100, size=rows.size)
    X[(nfirst - 1) * TILE + 5, 1] = 7                              # the last row block of the first launch holds entries
    X[nfirst * TILE:] = rng.integers(1, 50, size=(300, m))        # row blocks 65535 and 65536: the second launch
    assert X[(nfirst - 1) * TILE:nfirst * TILE].any() and X[nfirst * TILE:(nfirst + 1) * TILE].all() and X[(nfirst + 1) * TILE:].all()
    D = rng.random((n, m), dtype=np.float32)
    ct = eng.CountTiles.from_dense(X, 'cuda', side=torch.from_numpy(D).cuda())
    assert ct.nrb == nfirst + 2 and ct.ncb == 1 and ct.row_perm is None
    assert ct.nnz == int(np.count_nonzero(X))
    Y, slot, cell, gene = pr.decode(ct, with_entries=True)
    assert np.array_equal(Y[nfirst * TILE:], X[nfirst * TILE:].astype(np.float32))          # the rows of the second launch
    assert np.array_equal(Y, X.astype(np.float32))
    assert int((cell >= nfirst * TILE).sum()) == 300 * m
    side_nz = ct.side_nz.cpu().numpy()
    assert side_nz.shape == (ct.rslots,)
    want = np.zeros(ct.rslots, dtype=np.float32)
    want[slot] = D[cell, gene]
    second = cell >= nfirst * TILE
    assert np.array_equal(side_nz[slot[second]], D[cell[second], gene[second]])
    assert np.array_equal(side_nz.view(np.uint32), want.view(np.uint32))


# ---- D. the resident handle ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from oriana_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


def _data_d(seed, n, m, K):
    rng = np.random.default_rng(seed)
    dens = rng.beta(1.0, 3.0, size=m)
    dens[:40] = np.linspace(1.0, 0.5, 40)
    X = ((rng.poisson(3.0, size=(n, m)) + 1) * (rng.random((n, m)) < dens[None, :])).astype(np.float32)
    lu = rng.normal(size=(n, K)).astype(np.float32)
    lv = rng.normal(size=(m, K)).astype(np.float32)
    rZi = np.empty((n, K), np.float32); rZj = np.empty((m, K), np.float32)
    from oracle import cavi_oracle as co
    co.zq_gap(rZi, rZj, lu, lv, X)
    return rng, X, lu, lv, rZi, rZj


def _info_and_pass(lib, h, lu, lv, n, m, K):
    from oriana_amd._lib import ptr, stream_ptr
    assert h.value
    info = (ctypes.c_int64 * 13)()
    assert lib.oriana_counts_info(h, info, 13) == 0
    Zi, Zj = torch.full((n, K), 7.0, device='cuda'), torch.full((m, K), 7.0, device='cuda')
    lud, lvd = torch.from_numpy(lu).cuda(), torch.from_numpy(lv).cuda()
    assert lib.oriana_zq_gap_resident(h, ptr(Zi), ptr(Zj), ptr(lud), ptr(lvd), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert lib.oriana_counts_destroy(h) == 0
    return list(info), Zi.cpu().numpy(), Zj.cpu().numpy()


@pytest.mark.parametrize('dd', [0.0, 0.2], ids=['sliced', 'hybrid'])
def test_resident_dense_with_padded_rows(lib, dd):
    """ldx = m + 7: the padding columns (1e30) are never read."""
    from oriana_amd._lib import ptr, stream_ptr
    n, m, K = 600, 270, 20
    _, X, lu, lv, rZi, rZj = _data_d(41, n, m, K)
    Xpad = np.full((n, m + 7), 1e30, dtype=np.float32)
    Xpad[:, :m] = X
    res = []
    for arr in (X, Xpad):
        Xd = torch.from_numpy(arr).cuda()
        h = ctypes.c_void_p(None)
        assert lib.oriana_counts_create_dense_f32(ctypes.addressof(h), ptr(Xd), n, m, arr.shape[1], K, dd, stream_ptr()) == 0
        res.append(_info_and_pass(lib, h, lu, lv, n, m, K))
    assert res[0][0][4] == int(np.count_nonzero(X)) and (res[0][0][5] >= 32) == (dd > 0)
    assert res[1][0] == res[0][0]
    for info, Zi, Zj in res:
        print('err_colrel Z_i %.3e Z_j %.3e' % (err_colrel(Zi, rZi), err_colrel(Zj, rZj)))
        assert err_colrel(Zi, rZi) < helpers.RTOL and err_colrel(Zj, rZj) < helpers.RTOL


@pytest.mark.parametrize('dd', [0.0, 0.2], ids=['sliced', 'hybrid'])
@pytest.mark.parametrize('form', ['shuffled_zeros', 'duplicates'])
def test_resident_csr_that_is_not_canonical(lib, form, dd):
    """oriana_counts_create_csr reads any CSR: indices in any order inside a row, explicit zeros that are no entries, and
    duplicate column indices of a row that ADD UP (include/oriana_hip.h) -- the same handle and the same sums as from the
    canonical form."""
    import scipy.sparse as sp
    from oriana_amd._lib import stream_ptr
    n, m, K = 600, 270, 20
    rng, X, lu, lv, rZi, rZj = _data_d(43, n, m, K)
    r, c = np.nonzero(X)
    v = X[r, c]
    if form == 'shuffled_zeros':
        zr, zc = np.nonzero(X == 0)
        pick = rng.choice(zr.size, size=400, replace=False)
        rows, cols, vals = np.concatenate([r, zr[pick]]), np.concatenate([c, zc[pick]]), np.concatenate([v, np.zeros(400, np.float32)])
    else:
        split = v >= 2                                            # v = (v - 1) + 1: exact in float32, whatever the order
        rows, cols = np.concatenate([r, r[split]]), np.concatenate([c, c[split]])
        vals = np.concatenate([np.where(split, v - 1, v), np.ones(int(split.sum()), np.float32)])
    o = rng.permutation(rows.size)
    B = _raw_csr(rows[o], cols[o], vals[o].astype(np.float32), X.shape)
    assert not B.has_canonical_format and B.nnz > int(np.count_nonzero(X))
    res = []
    for A in (sp.csr_matrix(X), B):
        indptr = np.ascontiguousarray(A.indptr.astype(np.int64))
        indices = np.ascontiguousarray(A.indices.astype(np.int32))
        data = np.ascontiguousarray(A.data.astype(np.float32))
        h = ctypes.c_void_p(None)
        assert lib.oriana_counts_create_csr(ctypes.addressof(h), indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, n, m, K,
                                            dd, stream_ptr()) == 0
        res.append(_info_and_pass(lib, h, lu, lv, n, m, K))
    assert res[0][0][4] == int(np.count_nonzero(X)) and (res[0][0][5] >= 32) == (dd > 0)
    assert res[1][0] == res[0][0]
    print('err_colrel against the canonical form: Z_i %.3e Z_j %.3e' % (err_colrel(res[1][1], res[0][1]), err_colrel(res[1][2], res[0][2])))
    assert err_colrel(res[1][1], res[0][1]) < helpers.RTOL and err_colrel(res[1][2], res[0][2]) < helpers.RTOL
    for info, Zi, Zj in res:
        assert err_colrel(Zi, rZi) < helpers.RTOL and err_colrel(Zj, rZj) < helpers.RTOL


# ---- E. the steps every host shares: the scan, the planners' inputs, the one builder ------------------------------------------
def _offsets(lib, rs, cs):
    """oriana_pack_offsets on device copies of the int32 counts -> (roff, coff, totals) on the host."""
    from oriana_amd._lib import ptr, stream_ptr
    nt = int(rs.size)
    drs, dcs = (torch.from_numpy(np.concatenate([a, np.zeros(1, np.int32)])).cuda() for a in (rs, cs))      # (never empty)
    roff = torch.full((nt + 1,), -1, dtype=torch.int64, device='cuda')
    coff = torch.full((nt + 1,), -1, dtype=torch.int64, device='cuda')
    tot = np.full(2, -1, dtype=np.int64)
    assert lib.oriana_pack_offsets(ptr(roff), ptr(coff), ptr(drs), ptr(dcs), nt, tot.ctypes.data, stream_ptr()) == 0
    return roff.cpu().numpy(), coff.cpu().numpy(), tot                  # (the entry has synchronised: tot is final here)


def _assert_offsets(lib, rs, cs):
    roff, coff, tot = _offsets(lib, rs, cs)
    for off, cnt, total in ((roff, rs, tot[0]), (coff, cs, tot[1])):
        want = np.concatenate([np.zeros(1, np.int64), np.cumsum(cnt.astype(np.int64))])
        assert off.dtype == np.int64 and np.array_equal(off, want)
        assert off[-1] == total == int(cnt.astype(np.int64).sum())


@pytest.mark.parametrize('nt', [0, 1, 63, 64, 1023, 1024, 1025, 3 * 1024 + 7])
def test_pack_offsets_equal_cumsum(lib, nt):
    """The wave boundary (64), the work-group carry (1024) and an empty table."""
    rng = np.random.default_rng(nt)
    _assert_offsets(lib, rng.integers(0, 70000, size=nt).astype(np.int32), rng.integers(0, 70000, size=nt).astype(np.int32))


def test_pack_offsets_carry_past_32_bits(lib):
    nt = 3 * 1024 + 7
    big = np.full(nt, 1 << 21, dtype=np.int32)
    assert nt * (1 << 21) > 1 << 32
    _assert_offsets(lib, big, big + 64)


def _plan_inputs(lib, rs, cslice, nrb, ncb, want_cost=True, want_iters=True):
    from oriana_amd._lib import ptr, stream_ptr
    cost = np.full(ncb, np.nan) if want_cost else None
    iters = np.full(nrb * ncb, -1, dtype=np.int32) if want_iters else None
    assert lib.oriana_plan_inputs(ptr(rs) if want_cost else None, ptr(cslice) if want_iters else None, nrb, ncb,
                                  cost.ctypes.data if want_cost else None, iters.ctypes.data if want_iters else None,
                                  stream_ptr()) == 0
    return cost, iters


@pytest.fixture(scope='module')
def packed_e(eng):
    """(n, m, dense_density) -> (CountTiles, its tile_rslots as they were before finish() dropped them), packed once."""
    out = {}
    orig = eng.CountTiles.finish
    saved = []

    def finish(self):
        saved.append(self.tile_rslots.clone())
        return orig(self)
    eng.CountTiles.finish = finish
    try:
        for n, m, dd in [(513, 257, None), (257, 5, None), (1000, 300, 0.2)]:
            ct = eng.CountTiles.from_dense(_counts_a(n, m, np.float32, hybrid=bool(dd)), 'cuda', dense_density=dd)
            out[n, m, dd] = (ct, saved.pop())
            assert not saved and (ct.gd >= 32) == bool(dd)
    finally:
        eng.CountTiles.finish = orig
    return out


@pytest.mark.parametrize('n,m,dd', [(513, 257, None), (257, 5, None), (1000, 300, 0.2)], ids=['513x257', '257x5', '1000x300-hybrid'])
def test_plan_inputs_equal_numpy(lib, packed_e, n, m, dd):
    """Both planner inputs from a packed layout's own tables, exactly: the longest column slice per tile as integers, the
    gene-tile cost as the bit pattern of the doubles -- against sum / nrb / 1024 + 2 and against the expression the Python
    host used before it called this entry (float64 mean / (16 * 64) + 2.0): the row split cannot have moved."""
    ct, rs = packed_e[n, m, dd]
    nrb, ncb, nt = ct.nrb, ct.ncb, ct.nrb * ct.ncb
    assert nt > 0 and ncb == (m - ct.gd + TILE - 1) // TILE
    h = ct.host_arrays()
    cost, iters = _plan_inputs(lib, rs, ct.cslice, nrb, ncb)
    cs = h['cslice'][:nt].astype(np.int64)
    want_iters = ((cs[:, 1:] - cs[:, :-1]) // 64).max(axis=1).astype(np.int32)
    assert iters.dtype == np.int32 and np.array_equal(iters, want_iters) and want_iters.max() > 0
    rsh = rs.cpu().numpy()[:nt].reshape(nrb, ncb)
    assert np.array_equal(rsh.sum(axis=1, dtype=np.int64), np.diff(h['roff'])[:nt].reshape(nrb, ncb).sum(axis=1))     # the layout's own
    want_cost = rsh.sum(axis=0, dtype=np.float64) / float(nrb) / 1024.0 + 2.0
    parent = rsh.astype(np.float64).mean(axis=0) / (16 * 64) + 2.0
    assert cost.dtype == np.float64 and np.array_equal(cost.view(np.int64), want_cost.view(np.int64))
    assert np.array_equal(cost.view(np.int64), parent.view(np.int64))
    assert np.array_equal(ct.gene_tile_cost.view(np.int64), cost.view(np.int64))         # what finish() handed to the row plan


@pytest.mark.parametrize('which', ['no_cost', 'no_iters'])
def test_plan_inputs_either_output_may_be_null(lib, packed_e, which):
    """A NULL output (its device table is then NULL too) leaves the other one as it is with both."""
    ct, rs = packed_e[513, 257, None]
    cost, iters = _plan_inputs(lib, rs, ct.cslice, ct.nrb, ct.ncb)
    c1, i1 = _plan_inputs(lib, rs, ct.cslice, ct.nrb, ct.ncb, want_cost=which != 'no_cost', want_iters=which != 'no_iters')
    if which == 'no_cost':
        assert c1 is None and np.array_equal(i1, iters)
    else:
        assert i1 is None and np.array_equal(c1.view(np.int64), cost.view(np.int64))


@pytest.mark.parametrize('sort_rows,dd', [(True, None), (False, 0.2)], ids=['sliced_sort_rows', 'hybrid'])
def test_from_chunks_equals_from_dense(eng, sort_rows, dd):
    """One builder: a generator of 256-row chunks and the dense matrix cut into 256-row chunks give the same layout, the
    per-chunk cell order included."""
    n, m = 1000, 300
    X = _counts_a(n, m, np.float32, hybrid=bool(dd))
    Xd = torch.from_numpy(X).cuda()
    ct_c = eng.CountTiles.from_chunks(n, m, lambda r0, r1: Xd[r0:r1], 256, 'cuda', sort_rows=sort_rows, dense_density=dd)
    ct_d = eng.CountTiles.from_dense(X, 'cuda', chunk_bytes=1, sort_rows=sort_rows, dense_density=dd)
    assert (ct_c.gd >= 32) == bool(dd) and (ct_c.row_perm is not None) == sort_rows
    _assert_same_layout(ct_c, ct_d)
