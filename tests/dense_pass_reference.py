# -*- coding: utf-8 -*-
"""The dense-gene share of the responsibility pass (csrc/dense_pass.hip) restated for tests/test_dense_pass_gpu.py and
tests/test_dense_pass_host.py.

Written from include/oriana_hip.h (oriana_factor_prep, oriana_dense_images, oriana_dense_row_pass_tail, oriana_dense_col_pass,
oriana_finalize) and from the statements the file comment of dense_pass.hip cites (gap.py:67-80, sparse_gap.py:88-97,
zigap.py:94-95) -- not from the kernels.

Two parts:
  * pin_case(): the inputs of the float64 pins of the dense passes, one per padded width of the factor matrices, with the
    float64 value (cavi_oracle.zq_exact) and the reference's own float32 loop nest on the same inputs, computed once per case
    and shared;
  * six_product_eval(): the arithmetic the file comment promises -- every float32 operand split by truncation into three
    bf16 parts, six of the nine cross products, float32 wherever a value is kept between two products -- with a switch that
    drops cross products: what the bound of the GPU tests has to tell apart from the complete evaluation."""
import functools

import numpy as np

PIN_N, PIN_M = 300, 160          # two 256-cell blocks (the second holds 44 cells: tile 9 has 12, tiles 10-15 are padding); five gene tiles
PIN_DENSITY = 0.6
# one K per padded width oriana_kpad knows up to 100 (16 KC + 4 TAIL: the twelve (KC, TAIL) instantiations of k_dn_row / k_dn_col)
WIDTHS = (13, 20, 29, 33, 41, 50, 61, 68, 77, 84, 90, 100)
KPADS = (16, 20, 32, 36, 48, 52, 64, 68, 80, 84, 96, 100)
NESTS = ('gap', 'sparse', 'zi-quirk')
DEAD_GENE = 5
SLOW_CELL = 3
# the seed of a width's case; an entry here replaces 4000 + K (a width whose mutants do not all leave the bound on the CPU
# gets another draw, never another bound: tests/test_dense_pass_host.py)
SEEDS = {}

# the cross products (part of A, part of B) the evaluation keeps, 0 = hi, 1 = mid, 2 = lo; (1, 2), (2, 1), (2, 2) are below
# the float32 rounding of the sum
SIX = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
MUTANTS = {'no mid x mid': ((1, 1),), 'no lo terms': ((2, 0), (0, 2)), 'one lo term missing': ((2, 0),)}


def counts(rng, n, m, dens, maxv=3000):
    """The counts of test_dense_gpu._counts: Poisson(40) + 1, 2 % of the entries at `maxv`, thinned per gene."""
    X = rng.poisson(40.0, size=(n, m)).astype(np.int64) + 1
    X[rng.random((n, m)) < 0.02] = maxv
    X *= (rng.random((n, m)) < dens[None, :])
    return X


@functools.lru_cache(maxsize=None)
def pin_case(K, nest='gap', slow=False, m=PIN_M, sparse_genes=0):
    """dict(X, lu, lv, St, Sh, D, dq, K, nest, slow, m, gd, exact=(Z_i, Z_j, Z_log) float64, ref=(...) the reference's float32
    nest of `nest` -- two outputs for 'gap', three otherwise).  n = 300; `m` genes of density 0.6 (all dense at
    dense_density = 0.1), then `sparse_genes` genes of density 0.05 (under 10 % each: they stay on the sliced side).  lu = 1.5 N, lv = 1.5 N - 1;
    slow: one cell at lu - 80.  Computed once; callers must not write into the arrays."""
    from oracle import cavi_oracle as co
    assert nest in NESTS
    n = PIN_N
    mt = m + sparse_genes
    rng = np.random.default_rng(SEEDS.get(K, 4000 + K))
    dens = np.concatenate([np.full(m, PIN_DENSITY), np.full(sparse_genes, 0.05)])
    X = counts(rng, n, mt, dens).astype(np.float32)
    for j in range(m, mt):                        # (a draw of 30 non-zero counts would make the gene dense: keep 27 at most)
        X[np.flatnonzero(X[:, j])[27:], j] = 0
    lu = (rng.normal(size=(n, K)) * 1.5).astype(np.float32)
    lv = (rng.normal(size=(mt, K)) * 1.5 - 1.0).astype(np.float32)
    if slow:
        lu[SLOW_CELL] -= 80.0
    c = dict(X=X, lu=lu, lv=lv, St=None, Sh=None, D=None, dq=None, K=K, nest=nest, slow=slow, m=mt, gd=m)
    if nest == 'sparse':
        ps = rng.random((mt, K))
        c['St'] = (ps > 0.3).astype(np.float32)
        c['Sh'] = ps.astype(np.float32)
        c['St'][DEAD_GENE] = 0.0                  # a gene with every factor switched off
    if nest == 'zi-quirk':
        D = rng.random((n, mt)).astype(np.float32)
        D[X != 0] = 1.0                           # what the models hold (zigap.py:135)
        c['D'] = D
        c['dq'] = np.ascontiguousarray(D[:, :K])  # zigap.py:94 reads D_hat[i, k]
    r = [np.empty((n, K), np.float32), np.empty((mt, K), np.float32), np.empty((mt, K), np.float32)]
    with np.errstate(all='ignore'):
        if nest == 'gap':
            co.zq_gap(r[0], r[1], lu, lv, X)
            r = r[:2]
        elif nest == 'sparse':
            co.zq_sparse_gap(r[0], r[1], r[2], lu, lv, c['St'], c['Sh'], X)
        else:
            co.zq_zigap(r[0], r[1], r[2], lu, lv, c['D'], X, quirk=True)
        c['exact'] = co.zq_exact(lu, lv, X, c['St'], c['Sh'], c['D'], quirk=(nest == 'zi-quirk'))
    c['ref'] = tuple(r)
    for v in list(c.values()) + list(c['exact']) + list(c['ref']):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---- the bf16 x 3 evaluation ----------------------------------------------------------------------------------------------
def split3(x):
    """float32 -> (hi, mid, lo), each a float32 whose low 16 bits are zero (a bf16), by truncation: hi + mid + lo == x exactly
    (8 + 8 + 8 mantissa bits) wherever lo stays a normal number."""
    x = np.ascontiguousarray(x, np.float32)
    top = np.uint32(0xFFFF0000)
    hi = (x.view(np.uint32) & top).view(np.float32)
    r = x - hi                                    # exact
    mid = (r.view(np.uint32) & top).view(np.float32)
    r2 = r - mid                                  # exact
    lo = (r2.view(np.uint32) & top).view(np.float32)
    return hi, mid, lo


def _product(A, B, keep):
    """sum over the kept (part of A, part of B) pairs of A_part @ B_part^T: the products exact (bf16 x bf16), the sum in float64."""
    a = [p.astype(np.float64) for p in split3(A)]
    b = [p.astype(np.float64) for p in split3(B)]
    out = np.zeros((A.shape[0], B.shape[0]))
    for pa, pb in keep:
        out += a[pa] @ b[pb].T
    return out


def _tiled(A, B, keep, km, rows_per_flush):
    """C[j, k] = sum_i A[i, j] B[i, k], i in chunks of `rows_per_flush`: a chunk's sum on the matrix core (the kept cross
    products for the factors k < km, plain float32 FMAs -- here: float64 -- for the tail factors k >= km), rounded to float32 when
    it leaves, the chunks added in float32."""
    f32 = np.float32
    out = np.zeros((A.shape[1], B.shape[1]), f32)
    for i0 in range(0, A.shape[0], rows_per_flush):
        a, b = A[i0:i0 + rows_per_flush], B[i0:i0 + rows_per_flush]
        part = np.empty(out.shape)
        part[:, :km] = _product(np.ascontiguousarray(a.T), np.ascontiguousarray(b[:, :km].T), keep)
        part[:, km:] = a.T.astype(np.float64) @ b[:, km:].astype(np.float64)
        out = (out + part.astype(f32)).astype(f32)
    return out


def six_product_eval(case, drop=()):
    """(Z_i, Z_j) float32 of the plain nest as dense_pass.hip's file comment states it:
        FU = exp(lu - rowmax), FV = exp(lv - rowmax)                  float32 (oriana_factor_prep)
        den = FV FU^T                                                 the first 16 (Kp / 16) factors as six cross products of the
                                                                      bf16 parts, the last Kp % 16 in float32; a float32 value
        s = x / den                                                   float32
        R += S FV per tile of 32 genes, C += S^T FU per 256 cells     six cross products on the tile, float32 between tiles
        Z_i = FU R, Z_j = FV C                                        one float32 product (oriana_finalize)
    `drop`: cross products (part of A, part of B) left out of all three products."""
    assert case['nest'] == 'gap' and not case['slow']
    f32 = np.float32
    keep = tuple(p for p in SIX if p not in set(drop))
    lu, lv, X, K = case['lu'], case['lv'], case['X'], case['K']
    kp = KPADS[WIDTHS.index(K)] if K in WIDTHS else None
    km = K if kp is None or kp % 16 == 0 else kp - 4         # factors on the matrix core (zero padding adds exact zeros)
    FU = np.exp(lu - lu.max(1, keepdims=True)).astype(f32)
    FV = np.exp(lv - lv.max(1, keepdims=True)).astype(f32)
    den = _product(FV[:, :km], FU[:, :km], keep) + FV[:, km:].astype(np.float64) @ FU[:, km:].astype(np.float64).T
    den = den.astype(f32)                                    # [gene, cell]
    s = np.where(X != 0, X / den.T, 0).astype(f32)           # [cell, gene]
    R = _tiled(np.ascontiguousarray(s.T), FV, keep, km, 32)  # sum over genes, 32 at a time
    C = _tiled(s, FU, keep, km, 256)                         # sum over cells, 256 at a time
    return (FU * R).astype(f32), (FV * C).astype(f32)
