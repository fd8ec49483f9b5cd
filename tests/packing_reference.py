# -*- coding: utf-8 -*-
"""The packed count layout restated in plain NumPy, for tests/test_packing_gpu.py.

Written from include/oriana_hip.h (struct oriana_counts, oriana_rowrec, struct oriana_dense, oriana_plan_gene_order) and
DESIGN.md section 3, "Data layout in HBM" -- not from the packing kernels:

  * X is cut into 256 x 256 tiles, row-block-major.  The 256 rows of a tile form 16 slices of 16 rows; a slice is a run of
    iterations of 64 slots = 16 rows x 4 consecutive records of that row, so the k-th entry of row r (increasing column
    order) sits at  slice start + (k // 4) * 64 + (r % 16) * 4 + k % 4,  and a slice is as long as its longest row needs:
    ceil(longest / 4) * 64 slots.  Every slot without an entry is all-zero bytes.
  * The column side is the same with rows and columns exchanged: one byte per slot, the row inside the tile; 64 more
    slots per tile after its 16 slices (the write-only dummies).  A record names its column-side slot (cdst) and its column
    inside the tile.
  * roff / coff are the running sums of the tiles' slot counts.
  * A hybrid layout keeps the first gd packed genes as uint16 counts in 32 x 32 blocks (register order of the row kernel:
    engine.DenseBlock.to_dense documents it); the sliced layout then covers the packed genes [gd, m).

Everything here is exact: the tests compare bytes."""
import numpy as np

TILE = 256
REC = np.dtype([('x', '<f4'), ('cdst', '<u2'), ('col', 'u1'), ('pad', 'u1')])


def expected_gene_order(X, dense_density=None):
    """(col_perm int32 [m], gd): genes by decreasing non-zero count, ties in the caller's order; with a density, the genes
    expressed in at least that share of the cells whose counts are all integers in [0, 65535) first, cut to a multiple
    of 32 (oriana_plan_gene_order)."""
    X = np.asarray(X)
    n, m = X.shape
    col_nnz = (X != 0).sum(0).astype(np.int64)
    order = np.argsort(-col_nnz, kind='stable')
    if not dense_density:
        return order.astype(np.int32), 0
    Xf = X.astype(np.float64)
    bad = ((Xf < 0) | (Xf >= 65535) | (Xf != np.floor(Xf))).sum(0)
    ok = (col_nnz.astype(np.float64) >= float(dense_density) * max(n, 1)) & (bad == 0) & (col_nnz > 0)
    cand = order[ok[order]]
    gd = (len(cand) // 32) * 32
    if gd == 0:
        return order.astype(np.int32), 0
    keep = np.ones(m, dtype=bool)
    keep[cand[:gd]] = False
    return np.concatenate([cand[:gd], order[keep[order]]]).astype(np.int32), gd


def expected_row_perm(X, chunk_rows):
    """sort_rows: inside every packing chunk the cells by decreasing non-zero count, ties in the caller's order."""
    depth = (np.asarray(X) != 0).sum(1)
    n = depth.shape[0]
    out = np.empty(n, dtype=np.int32)
    for r0 in range(0, n, chunk_rows):
        r1 = min(n, r0 + chunk_rows)
        out[r0:r1] = r0 + np.argsort(-depth[r0:r1], kind='stable')
    return out


def _packed(X32, col_perm, row_perm):
    Xp = np.asarray(X32, dtype=np.float32)
    if row_perm is not None:
        Xp = Xp[np.asarray(row_perm, dtype=np.int64)]
    if col_perm is not None:
        Xp = Xp[:, np.asarray(col_perm, dtype=np.int64)]
    return Xp


def _slices(cnt):
    """cnt (nt, 256) entries per row (column) of every tile -> (nt, 17) slot offsets of the 16 slices."""
    longest = cnt.reshape(-1, 16, 16).max(axis=2)
    length = (longest + 3) // 4 * 64
    out = np.zeros((cnt.shape[0], 17), dtype=np.int64)
    out[:, 1:] = np.cumsum(length, axis=1)
    return out


def expected_layout(X32, col_perm=None, row_perm=None, gd=0):
    """The sliced layout of the packed genes [gd, m) of the dense float32 matrix X32 (caller's order) under the two
    orderings.  Returns a dict: nrb, ncb, tile_nnz, rslice, cslice (uint32 (max(nt, 1), 17)), roff, coff (int64 [nt + 1]),
    rslots, cslots, nnz_sparse, rec (REC [max(rslots, 1)]), ridx (uint8 [max(cslots, 1)]), and for the side matrix:
    entry_slot (row-side slot of every entry), entry_cell / entry_gene (its place in the CALLER's matrix)."""
    X32 = np.asarray(X32, dtype=np.float32)
    n, m = X32.shape
    ms = m - gd
    S = _packed(X32, col_perm, row_perm)[:, gd:]
    nrb, ncb = (n + TILE - 1) // TILE, (ms + TILE - 1) // TILE
    nt = nrb * ncb
    P = np.zeros((nrb * TILE, ncb * TILE), dtype=np.float32)
    P[:n, :ms] = S
    T = P.reshape(nrb, TILE, ncb, TILE).transpose(0, 2, 1, 3).reshape(nt, TILE, TILE)      # [tile][row][column]
    nz = T != 0
    rslice, cslice = _slices(nz.sum(axis=2)), _slices(nz.sum(axis=1))
    roff, coff = np.zeros(nt + 1, dtype=np.int64), np.zeros(nt + 1, dtype=np.int64)
    roff[1:] = np.cumsum(rslice[:, 16])
    coff[1:] = np.cumsum(cslice[:, 16] + 64)
    rslots, cslots = int(roff[-1]), int(coff[-1])
    t, r, c = np.nonzero(nz)                                        # ordered by tile, row, column
    krow = (np.cumsum(nz, axis=2) - 1)[t, r, c]                      # rank of the entry in its row / in its column
    kcol = (np.cumsum(nz, axis=1) - 1)[t, r, c]
    rslot = rslice[t, r >> 4] + (krow >> 2) * 64 + (r & 15) * 4 + (krow & 3)
    cslot = cslice[t, c >> 4] + (kcol >> 2) * 64 + (c & 15) * 4 + (kcol & 3)
    rec = np.zeros(max(rslots, 1), dtype=REC)
    ridx = np.zeros(max(cslots, 1), dtype=np.uint8)
    rec['x'][roff[t] + rslot] = T[t, r, c]
    rec['cdst'][roff[t] + rslot] = cslot
    rec['col'][roff[t] + rslot] = c
    ridx[coff[t] + cslot] = r
    prow, pcol = (t // max(ncb, 1)) * TILE + r, gd + (t % max(ncb, 1)) * TILE + c
    cell = prow if row_perm is None else np.asarray(row_perm, dtype=np.int64)[prow]
    gene = pcol if col_perm is None else np.asarray(col_perm, dtype=np.int64)[pcol]
    u32 = lambda a: np.ascontiguousarray(a if nt else np.zeros((1, 17)), dtype=np.uint32)
    return dict(nrb=nrb, ncb=ncb, tile_nnz=nz.sum(axis=(1, 2)).astype(np.int32) if nt else np.zeros(1, np.int32),
                rslice=u32(rslice), cslice=u32(cslice), roff=roff, coff=coff, rslots=rslots, cslots=cslots,
                nnz_sparse=int(nz.sum()), rec=rec, ridx=ridx, entry_slot=roff[t] + rslot, entry_cell=cell, entry_gene=gene)


# register order of the dense block: gene g of a 32-gene tile is element v of half h (lanes 32 h .. 32 h + 31),
# g = 8 (v >> 2) + 4 h + (v & 3)
_G = np.arange(32)
_V, _H = 4 * (_G >> 3) + (_G & 3), (_G >> 2) & 1
_LANE = 32 * _H[None, :] + np.arange(32)[:, None]                   # [cell][gene] -> lane


def expected_dense_block(X32, col_perm, row_perm, gd):
    """uint16 image of DenseBlock.x: [cell tile of 32][gene tile of 32][v // 8][lane][v % 8], whole 256-row blocks
    allocated, zeros beyond the last cell."""
    X32 = np.asarray(X32, dtype=np.float32)
    n = X32.shape[0]
    ngt, nct = gd // 32, (n + TILE - 1) // TILE * 8
    B = np.zeros((nct * 32, gd), dtype=np.uint16)
    B[:n] = _packed(X32, col_perm, row_perm)[:, :gd].astype(np.uint16)
    out = np.zeros((nct, ngt, 2, 64, 8), dtype=np.uint16)
    out[:, :, (_V >> 3)[None, :], _LANE, (_V & 7)[None, :]] = B.reshape(nct, 32, ngt, 32).transpose(0, 2, 1, 3)
    return out.reshape(-1)


def decode_dense_block(x, n, gd):
    """(n, gd) float32, packed gene order, from the uint16 image."""
    ngt = gd // 32
    x5 = np.asarray(x).reshape(-1, ngt, 2, 64, 8)
    B = x5[:, :, (_V >> 3)[None, :], _LANE, (_V & 7)[None, :]]      # [cell tile][gene tile][cell][gene]
    return B.transpose(0, 2, 1, 3).reshape(-1, gd)[:n].astype(np.float32)


def entries(h, nrb, ncb):
    """Every stored entry of host_arrays() `h`, from the row side: (row-side slot, packed row, packed column of the sliced
    part, value); checks on the way that the column side names the same entry (AssertionError otherwise).  Vectorised over
    the stored entries: no loop over tiles."""
    nt = nrb * ncb
    rec = h['rec']
    slot = np.flatnonzero(rec['x'] != 0)
    if nt == 0 or slot.size == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, np.zeros(0, dtype=np.float32)
    roff, coff = h['roff'].astype(np.int64), h['coff'].astype(np.int64)
    rs, cs = h['rslice'][:nt].astype(np.int64), h['cslice'][:nt].astype(np.int64)
    assert slot[-1] < roff[-1]
    start = (roff[:nt, None] + rs[:, :16]).reshape(-1)              # first slot of every (tile, slice): non-decreasing
    seg = np.searchsorted(start, slot, side='right') - 1
    t, sl = seg >> 4, seg & 15
    assert (slot < roff[t] + rs[t, sl + 1]).all()
    row = sl * 16 + (((slot - start[seg]) & 63) >> 2)
    col = rec['col'][slot].astype(np.int64)
    cd = rec['cdst'][slot].astype(np.int64)
    # the column side: the slot belongs to the entry's column, inside its slice, and names the entry's row
    base = cs[t, col >> 4]
    assert (cd >= base).all() and (cd < cs[t, (col >> 4) + 1]).all() and ((((cd - base) & 63) >> 2) == (col & 15)).all()
    assert np.array_equal(h['ridx'][coff[t] + cd].astype(np.int64), row)
    assert np.unique(coff[t] + cd).size == slot.size
    return slot, (t // ncb) * TILE + row, (t % ncb) * TILE + col, rec['x'][slot]


def decode(ct, with_entries=False):
    """The dense float32 matrix, caller's order, from ct.host_arrays() (and the dense block of a hybrid layout).
    with_entries: also (row-side slot, cell, gene) of every sliced entry, in the caller's numbering."""
    h = ct.host_arrays()
    slot, prow, pcol, x = entries(h, ct.nrb, ct.ncb)
    assert slot.size == ct.nnz_sparse
    if slot.size:
        assert prow.max() < ct.n and pcol.max() < ct.ms
    Xp = np.zeros((ct.n, ct.m), dtype=np.float32)
    Xp[prow, ct.gd + pcol] = x
    if ct.dense is not None:
        Xp[:, :ct.gd] = decode_dense_block(ct.dense.x.cpu().numpy(), ct.n, ct.gd)
    rp = ct.row_perm.cpu().numpy().astype(np.int64) if ct.row_perm is not None else None
    cp = ct.col_perm.cpu().numpy().astype(np.int64) if ct.col_perm is not None else None
    X = Xp
    if rp is not None:
        X = np.empty_like(Xp)
        X[rp] = Xp
    if cp is not None:
        out = np.empty_like(X)
        out[:, cp] = X
        X = out
    if not with_entries:
        return X
    cell = prow if rp is None else rp[prow]
    gene = ct.gd + pcol if cp is None else cp[ct.gd + pcol]
    return X, slot, cell, gene
