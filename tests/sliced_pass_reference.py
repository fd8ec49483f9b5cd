# -*- coding: utf-8 -*-
"""The sliced row and column passes (csrc/passes_*.h, dispatched in csrc/passes.hip) restated for tests/test_sliced_pass_gpu.py
and tests/test_sliced_pass_host.py.  Host only; every case is computed once and its arrays are read-only.

Written from include/oriana_hip.h (oriana_counts: 256 x 256 tiles, 16 slices of 16 rows per tile, 64 slots -- four records per
row -- per iteration of a slice, the slice as long as its longest row) and from the statements the kernels' file comments cite
(gap.py:67-80, zigap.py:79-95, sparse_gap.py:81-97, sparse_zigap.py:100-116) -- not from the kernels.

Counts (no gene or cell ordering: packed position = position in X):
  * small('rows'): tests/test_trim_last_iteration_gpu.build_rows at its own size (3 x 3 tiles, ragged last row block and gene
    tile: every remainder mod 4 of a slice's longest row, waves whose slices need different iteration counts, empty slices
    beside live ones, an empty wave, a single-entry tile, a tile with no entry, a tile partial both ways) with one more
    full-width gene tile put in front of the ragged one: 3 x 4 tiles.  build_rows reaches 1 .. 4 iterations per slice; the
    added tile holds, in each full row block, slices of 0, 1, 2, 3, 4, 5 and 6 iterations (on both sides of every prefetch depth
    in use: 2, 3 and 4 iterations) and one slice whose longest row has all 256 entries of the tile (64 iterations), with
    empty and one-iteration slices around it in the aligned group of four slices (a wave of the one-lane kernels), in its pair
    (a wave of the two-lane kernels) and in the 16, 8 or 4 slices of a work-group of the G-lane kernels (WaveGeo<G>: one slice
    per wave, or per two or four waves).
  * small('cols'): the same construction transposed (4 x 3 tiles): the column slices hold the cases.
  * band('rows') / band('cols'): build_rows at 11 row blocks (n = 10 * 256 + 40) x the same 3 gene tiles, and the transposed
    construction of that shape: enough row blocks for the band grid of the column pass without a work list (two bands of
    6 + 5 row blocks; 4 + 4 + 3 for the one-lane kernel).

Yardsticks: exact_nz(), the float64 loop nest over the non-zero counts only (COO, np.add.at: no n x m x K intermediate), which
agrees with cavi_oracle.zq_exact to 1e-13 (tests/test_sliced_pass_host.py), and the reference's own float32 nests
(oracle/zq_kernels.c).  slot_stream() / f32_slot_eval() restate the slot order of the packed layout for the two mutants the
bound of the GPU tests has to tell apart from a complete evaluation: a record lost at the end of a slice, a padding slot taken
for an entry."""
import functools

import numpy as np

from test_trim_last_iteration_gpu import build_rows, longest_per_slice, N_ROWS, N_COLS, TILE   # noqa: F401 (re-exported)

# one K per configuration of the dispatcher (csrc/passes.hip pick_cfg: 18), padded where the class allows it
WIDTHS = (13, 20, 29, 33, 45, 50, 61, 66, 77, 84, 93, 100, 105, 120, 150, 190, 200, 250)
KPADS = (16, 20, 32, 36, 48, 52, 64, 68, 80, 84, 96, 100, 112, 128, 160, 192, 224, 256)
FORMS = ('plain', 'weighted', 'sparse', 'sparse+weighted')
FAMILY_WIDTHS = (20, 29, 50, 84, 100, 150, 250)       # one per kernel family: narrow, narrow / k_col_pass2, k64, G = 4, k100, G = 8, G = 16
WEIGHT_WIDTHS = (20, 50, 84, 100, 150, 250)           # one per row family of the weights column
# one per column family: narrow, k_col_pass2 (Kp = 32 and the duplicated image of Kp = 100), k64, generic with a whole image
# (Kp = 128) and with sub-tiles of it (Kp = 160: two of 128 rows; Kp = 256)
BAND_WIDTHS = (20, 29, 50, 100, 120, 150, 250)
BAND_ROWS = 10 * TILE + 40
DEEP = TILE                      # entries of the longest row of the deep slice: every column of the tile
SHORT = 4                        # a "short" slice: one iteration

# longest row per slice of the added tile, per row block (the ragged last one has 40 rows: slices 0, 1 and half of 2).
# Iterations = ceil(length / 4): block 0 holds 64, 0, 1, 0 | 0, 1, 2, 3 | 4, 5, 6, 6 | 3, 0, 5, 1 (deep slice first in its
# wave), block 1 holds 2, 3, 0, 6 | 4, 0, 5, 2 | 1, 3, 4, 0 | 0, 64, 1, 0 (deep slice second in its pair and in its four).
EXTRA_LENGTHS = ([DEEP, 0, 3, 0, 0, 2, 7, 12, 13, 18, 24, 21, 9, 0, 17, 1],
                 [5, 11, 0, 23, 16, 0, 20, 6, 1, 10, 15, 0, 0, DEEP, 2, 0],
                 [22, 0, 5] + [0] * 13)
# entries of the other 15 rows of a deep slice: at most this many (a draw, like every other row of the construction)
DEEP_OTHER_ROWS = 64


def extra_tile(nr, seed):
    """(nr, 256) counts of the added gene tile: EXTRA_LENGTHS per row block, rows filled the way build_rows fills them."""
    rng = np.random.default_rng(seed)
    T = np.zeros((nr, TILE), np.int64)
    nrb = (nr + TILE - 1) // TILE
    assert nrb == len(EXTRA_LENGTHS)
    for rb in range(nrb):
        for sl, L in enumerate(EXTRA_LENGTHS[rb]):
            rows = [r for r in range(rb * TILE + sl * 16, rb * TILE + sl * 16 + 16) if r < nr]
            if not rows or L == 0:
                continue
            longest = rows[(sl * 5) % len(rows)]
            for r in rows:
                k = L if r == longest else int(rng.integers(0, min(L, DEEP_OTHER_ROWS) + 1))
                cols = rng.choice(TILE, size=k, replace=False)
                T[r, cols] = rng.poisson(3.0, size=k) + 1
    return T


def _rows_construction(nr, nc, seed, extra):
    X = build_rows(nr, nc, seed)
    if extra:
        full = (nc // TILE) * TILE                # the added tile goes in front of the ragged last gene tile
        X = np.concatenate([X[:, :full], extra_tile(nr, seed + 100), X[:, full:]], axis=1)
    return X


@functools.lru_cache(maxsize=None)
def problem(name, side):
    """name 'small' / 'band', side 'rows' (the cases sit in the row slices) / 'cols' (in the column slices).  int64, read-only."""
    if name == 'small':
        X = _rows_construction(N_ROWS, N_COLS, 1, True) if side == 'rows' else _rows_construction(N_COLS, N_ROWS, 2, True).T
    else:
        X = build_rows(BAND_ROWS, N_COLS, 3) if side == 'rows' else build_rows(N_COLS, BAND_ROWS, 4).T
    X = np.ascontiguousarray(X)
    X.setflags(write=False)
    return X


def sliced_view(name, side):
    """The counts with the side under test as rows: X for 'rows', X^T for 'cols'."""
    X = problem(name, side)
    return X if side == 'rows' else np.ascontiguousarray(X.T)


def slice_lengths(name, side):
    """[block][tile][slice] longest row (column, for 'cols') of the slice inside the tile, on the side under test."""
    return longest_per_slice(sliced_view(name, side))


def slice_iterations(name, side):
    """[block][tile][slice] iterations of 64 slots the slice takes: four records per row and iteration."""
    return (slice_lengths(name, side) + 3) // 4


def extra_tile_index(name, side):
    """Index of the added tile along the tile axis of slice_lengths (the last full-width one), or None."""
    return None if name != 'small' else slice_lengths(name, side).shape[1] - 2


# ---- inputs and yardsticks ----------------------------------------------------------------------------------------------------
def exact_nz(lu, lv, X, St=None, Sh=None, D=None):
    """The four loop nests in float64 from the float32 inputs, over the non-zero counts only: (Z_i, Z_j, Z_log) as
    cavi_oracle.zq_exact(quirk=False) defines them, without its n x m x K intermediates."""
    n, K = lu.shape
    m = lv.shape[0]
    i, j = np.nonzero(X)
    x = np.asarray(X)[i, j].astype(np.float64)
    ls = np.asarray(lu, np.float64)[i] + np.asarray(lv, np.float64)[j]
    with np.errstate(all='ignore'):
        e = np.exp(ls)
        if St is not None:
            e = e * np.asarray(St, np.float64)[j]
        den = e.sum(1)
        den = np.where(den > 0, den, 1.0)
        r = x[:, None] * e / den[:, None]
        wi = r if D is None else np.asarray(D, np.float64)[i, j][:, None] * r
        Zi, Zj, Zl = np.zeros((n, K)), np.zeros((m, K)), np.zeros((m, K))
        np.add.at(Zi, i, wi if Sh is None else wi * np.asarray(Sh, np.float64)[j])
        np.add.at(Zj, j, wi)
        np.add.at(Zl, j, wi * np.where(r == 0, 0.0, ls))
    return Zi, Zj, Zl


def _freeze(c):
    for v in list(c.values()) + list(c.get('exact', ())) + list(c.get('ref', ())):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def inputs(name, side, K, form):
    """dict(X float32, lu, lv N(0, 1) float32, D in 0.25 .. 1 or None, St = (p > 0.3), Sh = p or None)."""
    assert form in FORMS
    X = problem(name, side)
    n, m = X.shape
    rng = np.random.default_rng(7000 + K + 1000 * FORMS.index(form) + (500 if side == 'cols' else 0))
    c = dict(X=np.ascontiguousarray(X.astype(np.float32)), lu=rng.normal(size=(n, K)).astype(np.float32),
             lv=rng.normal(size=(m, K)).astype(np.float32), D=None, St=None, Sh=None, K=K, form=form, side=side, name=name)
    if 'weighted' in form:
        c['D'] = (0.25 + 0.75 * rng.random((n, m))).astype(np.float32)
    if 'sparse' in form:
        ps = rng.random((m, K))
        c['St'] = (ps > 0.3).astype(np.float32)
        c['Sh'] = ps.astype(np.float32)
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def case(name, side, K, form):
    """inputs() plus exact = exact_nz (float64) and ref = the reference's float32 nest of the form: (Z_i, Z_j, Z_log), Z_log
    None for 'plain'.  The small problem takes the C oracle's full nests; the band problem (plain only) the zero-skipping
    nest zq_gap_nz, bit-identical while every exponential is finite (tests/test_sliced_pass_host.py checks that here)."""
    from oracle import cavi_oracle as co
    c = dict(inputs(name, side, K, form))
    X, lu, lv = c['X'], c['lu'], c['lv']
    n, m = X.shape
    r = [np.empty((n, K), np.float32), np.empty((m, K), np.float32), np.empty((m, K), np.float32)]
    if form == 'plain':
        (co.zq_gap_nz if name == 'band' else co.zq_gap)(r[0], r[1], lu, lv, X)
        r[2] = None
    else:
        assert name == 'small'
        if form == 'weighted':
            co.zq_zigap(r[0], r[1], r[2], lu, lv, c['D'], X, quirk=False)
        elif form == 'sparse':
            co.zq_sparse_gap(r[0], r[1], r[2], lu, lv, c['St'], c['Sh'], X)
        else:
            co.zq_sparse_zigap(r[0], r[1], r[2], lu, lv, c['St'], c['Sh'], c['D'], X)
    c['ref'] = tuple(r)
    c['exact'] = exact_nz(lu, lv, X, c['St'], c['Sh'], c['D'])
    return _freeze(c)


def case_keys():
    """Every (problem, side, K, form) tests/test_sliced_pass_gpu.py judges."""
    keys = [('small', side, K, form) for side in ('rows', 'cols') for form in ('plain', 'sparse') for K in WIDTHS]
    keys += [('small', side, K, form) for side in ('rows', 'cols') for form in ('weighted', 'sparse+weighted') for K in WEIGHT_WIDTHS]
    keys += [('band', side, K, 'plain') for side in ('rows', 'cols') for K in BAND_WIDTHS]
    return keys


# ---- the slot order of the packed layout, and the two mutants ----------------------------------------------------------------
def slot_stream(Xs):
    """The row-side slots of `Xs` (the side under test as rows) in stream order: tile by tile (block, then tile), slice by slice,
    iteration by iteration, 16 rows x 4 records per iteration, a row's entries by increasing column.  Returns int64 arrays
    (block, tile, slice, it, row, col): col = -1 marks a padding slot (a row beyond its last entry or beyond the matrix)."""
    n, m = Xs.shape
    nrb, ncb = (n + TILE - 1) // TILE, (m + TILE - 1) // TILE
    out = []
    for rb in range(nrb):
        for cb in range(ncb):
            sub = Xs[rb * TILE:(rb + 1) * TILE, cb * TILE:(cb + 1) * TILE] != 0
            for sl in range(16):
                rows = sub[sl * 16:sl * 16 + 16]
                if not rows.any():
                    continue
                ents = [np.flatnonzero(r) for r in rows]
                niter = (max(len(e) for e in ents) + 3) // 4
                cols = np.full((niter * 4, 16), -1, np.int64)            # [entry index][row of the slice]
                for g, e in enumerate(ents):
                    cols[:len(e), g] = e + cb * TILE
                cols = cols.reshape(niter, 4, 16).transpose(0, 2, 1)     # [it][row][record]
                it, g, _ = np.indices(cols.shape)
                k = cols.size
                out.append(np.stack([np.full(k, rb), np.full(k, cb), np.full(k, sl), it.ravel(),
                                     rb * TILE + sl * 16 + g.ravel(), cols.ravel()]))
    s = np.concatenate(out, axis=1)
    return tuple(s)


def f32_slot_eval(c, side):
    """The plain nest in float32 the way the file comment of csrc/passes.hip states it, in slot order:
        FU = exp(lu - rowmax), FV = exp(lv - rowmax);  den = <FU_i, FV_j>;  s = x / den;  R_i += s FV_j;  C_j += s FU_i
    every sum float32, one addition per slot.  Returns dict(Zi, Zj float32 in the orientation of the side under test's
    matrix `Xs`, FA, FB, R, C, stream, Xs): what the mutants below patch."""
    assert c['form'] == 'plain'
    f32 = np.float32
    Xs = c['X'] if side == 'rows' else np.ascontiguousarray(c['X'].T)
    la, lb = (c['lu'], c['lv']) if side == 'rows' else (c['lv'], c['lu'])
    FA = np.exp(la - la.max(1, keepdims=True)).astype(f32)
    FB = np.exp(lb - lb.max(1, keepdims=True)).astype(f32)
    st = slot_stream(Xs)
    live = st[5] >= 0
    i, j = st[4][live], st[5][live]
    s = (Xs[i, j] / np.einsum('ek,ek->e', FA[i], FB[j], dtype=f32)).astype(f32)
    R, C = np.zeros(FA.shape, f32), np.zeros(FB.shape, f32)
    np.add.at(R, i, s[:, None] * FB[j])
    np.add.at(C, j, s[:, None] * FA[i])
    return dict(Zi=FA * R, Zj=FB * C, FA=FA, FB=FB, R=R, C=C, stream=st, Xs=Xs)


def mutants(ev):
    """For every slice that has slots: ((block, tile, slice), lost, taken).  `lost` = (i, j, -1): the record in the last occupied
    slot of the slice is skipped; `taken` = (i, j, +1): the first padding slot of the slice that belongs to a row of the matrix is
    treated as an entry of image row 0 (the tile's first column) with x = 1 -- None where the slice has no such slot."""
    rb, cb, sl, it, row, col = ev['stream']
    n = ev['Xs'].shape[0]
    key = (rb * 1000 + cb) * 16 + sl
    out = []
    for k in np.unique(key):
        idx = np.flatnonzero(key == k)
        occ = idx[col[idx] >= 0]
        last = occ[-1]
        pad = idx[(col[idx] < 0) & (row[idx] < n)]
        taken = (int(row[pad[0]]), int(cb[pad[0]]) * TILE, +1) if len(pad) else None
        out.append(((int(rb[last]), int(cb[last]), int(sl[last])), (int(row[last]), int(col[last]), -1), taken))
    return out


def apply_mutant(ev, mut):
    """(Zi, Zj) float32 of f32_slot_eval with one record removed (sign -1, x = the count) or added (sign +1, x = 1)."""
    f32 = np.float32
    i, j, sign = mut
    x = ev['Xs'][i, j] if sign < 0 else f32(1)
    s = f32(x) / np.dot(ev['FA'][i], ev['FB'][j])
    Zi, Zj = ev['Zi'].copy(), ev['Zj'].copy()
    Zi[i] = ev['FA'][i] * (ev['R'][i] + f32(sign) * s * ev['FB'][j])
    Zj[j] = ev['FB'][j] * (ev['C'][j] + f32(sign) * s * ev['FA'][i])
    return Zi, Zj
