# -*- coding: utf-8 -*-
"""The case table of the three held-out ZI entries -- oriana_zi_foldin_rate, oriana_zi_gene_rate, oriana_zi_cell_bound (csrc/
dense_f32.hip, csrc/dense_zi.hip) -- and the NumPy recipe of their inputs.  Plain data: tests/test_zi_heldout_cases_host.py holds
the table to the dispatch rule (oriana_zi_dispatch) and to the loop bounds, tests/test_zi_heldout_forms_gpu.py makes the calls.

Inputs (inputs(K, n, m), deterministic per (K, n, m), read-only):
    V ~ Gamma(2, 0.5) (m, K);  U ~ Gamma(1, 1) (n, K), scaled so that the mean of Lambda = U V^T is 1;
    pi_d ~ U(0.05, 0.95) with gene PI_ZERO at 0 and gene PI_ONE at 1;
    X ~ Poisson(0.4) with gene ZERO_GENE all zero and (n > 1) cell ZERO_CELL all zero.
Two thirds of the entries then have 0.01 < d < 0.99 (at the body shape 64 to 67 % for every K used here): the sigmoid, not its
two ends, decides the result.  MIDDLE_MIN is the condition tests/test_zi_foldin_gpu.py puts on its own case.

Body shape: N_BODY = 300 cells -- a partial last tile of 32 cells, a partial work-group of 128 (dense_f32.hip) and of 256 cells
(dense_zi.hip) -- by M_REAL = 291 genes, handed to the entries either with one inert gene (V row 0, pi_d 0) as M_ALIGNED = 292 =
9 x 32 + 4, or as they are (m % 4 != 0: the tiles family does not apply): ten gene tiles, the last one of 4 or 3 genes.  The
rate kernels cut one gene range at this size, so it passes the flush at 256 genes and goes on.  The gene count is small on purpose:
a DV row is a sum of 291 terms d_ij V_jk, one wrong d_ij moves it by about 1e-2 relative, a thousand times the bound."""
import functools

import numpy as np

N_BODY, M_REAL, M_ALIGNED = 300, 291, 292
PI_ZERO, PI_ONE, ZERO_GENE, ZERO_CELL = 0, 1, 2, 11
MIDDLE_MIN = 0.2
F32, BF16X3 = 0, 1                    # ORIANA_MATRIX_F32, ORIANA_MATRIX_BF16X3
UPDATE = 0                            # op of oriana_zi_dispatch: the D update and its rate-only twin
TILES, B16, F32_FAMILY = 1, 2, 3      # family of oriana_zi_dispatch

# ---- the factor-loop forms of k_dropout_sweep and k_gene_rate ------------------------------------------------------------------
# With KS = ceil(K / 2) steps of the float32 matrix instruction (two factors each; an odd K ends in a zero-padded factor):
#   'short'  KS < 4            one step at a time
#   'empty'  4 <= KS < 8       prologue and epilogue, the pipelined body runs zero times
#   'body'   KS >= 8           the body runs (KS - 4) // 4 times
# and the epilogue takes rem = KS % 4 steps beyond its full turn of four.  NT = ceil(oriana_kpad(K) / 32) factor tiles of the
# second product.  K: (NT, form, KS, rem) -- held to the loop bounds by the host test.
K_FORMS_TABLE = {
    1: (1, 'short', 1, None),         # NT = 1 at its narrowest; the short loop at one end; odd
    6: (1, 'short', 3, None),         # the short loop at its other end
    7: (1, 'empty', 4, 0),            # the first K that takes the pipelined form; odd
    13: (1, 'empty', 7, 3),           # rem = 3 without a body; odd
    30: (1, 'body', 15, 3),           # rem = 3 behind a running body; Kp = 32: NT = 1 at (nearly) its widest
    33: (2, 'body', 17, 1),           # NT = 2 at its narrowest; odd
    64: (2, 'body', 32, 0),           # NT = 2 at its widest
    65: (3, 'body', 33, 1),           # NT = 3 at its narrowest; odd
    78: (3, 'body', 39, 3),
    84: (3, 'body', 42, 2),
    96: (3, 'body', 48, 0),           # NT = 3 at its widest
    97: (4, 'body', 49, 1),           # NT = 4 at its narrowest; odd
    126: (4, 'body', 63, 3),
    128: (4, 'body', 64, 0),          # NT = 4 at its widest, the last K the entries serve
}
K_FORMS = tuple(K_FORMS_TABLE)
assert K_FORMS == (1, 6, 7, 13, 30, 33, 64, 65, 78, 84, 96, 97, 126, 128)
# what the K above must cover between them: (form, KS) for the short loop's ends, (form, rem) for the others
LOOP_FORMS = (('short', 1), ('short', 3), ('empty', 0), ('empty', 3), ('body', 0), ('body', 1), ('body', 2), ('body', 3))

# ---- oriana_zi_foldin_rate: (K, arithmetic, m, with_tiles) at N_BODY cells --------------------------------------------------------
# m is the gene count the entry is given (M_ALIGNED: one inert gene; M_REAL: none); with_tiles: the per-lane flags of
# oriana_nzmask_tiles are passed.  The tiles family runs when both hold; otherwise the entry goes on to the next candidate.
RATE_CASES = tuple(
    # k_zi_row<KC, TAIL, true>: <3,0> <3,1> <4,0> <4,1> <5,0> <5,1> <6,0> <6,1> at the widest K of each, and two that are narrower
    [(K, BF16X3, M_ALIGNED, True) for K in (48, 52, 64, 68, 80, 84, 96, 100, 53, 97)] +
    # k_dropout_sweep_b16<NT, KC, true> as the first candidate: <1,1> (Kp = 16), <1,2> (Kp = 20, 32), <2,3> (Kp = 36)
    [(K, BF16X3, M_ALIGNED, True) for K in (13, 16, 20, 30, 32, 33, 36)] +
    # ... by the fallback from tiles: <2,3> (Kp = 48), <2,4> (Kp = 52, 64; reachable in no other way)
    [(K, BF16X3, M_REAL, True) for K in (48, 52, 64)] + [(K, BF16X3, M_ALIGNED, False) for K in (48, 64)] +
    # k_dropout_sweep<NT, true> by the fallback from tiles (NT = 3: Kp = 68 .. 96; NT = 4: Kp = 100) ...
    [(K, BF16X3, M_REAL, True) for K in (68, 84, 96, 100)] + [(K, BF16X3, M_ALIGNED, False) for K in (80, 100)] +
    # ... as the first candidate of bf16 x 3 (Kp = 112, 128), whatever the gene count
    [(101, BF16X3, M_ALIGNED, True), (112, BF16X3, M_REAL, True), (128, BF16X3, M_ALIGNED, True)] +
    # ... and under ORIANA_MATRIX_F32 in every loop form; the flags and the alignment of m play no part there
    [(K, F32, M_ALIGNED, True) for K in K_FORMS] + [(30, F32, M_REAL, False), (78, F32, M_REAL, True), (126, F32, M_ALIGNED, False)])

# Edge shapes, one instantiation per family: (K, arithmetic, n, m, with_tiles), every gene real (m is also the number of genes
# of the inputs).  One cell; a cell tile and one cell; one piece of four genes (tiles) and three genes (the fallback of the same
# K); 256 genes: the flush at 256 genes falls on the last tile.
RATE_EDGE_CASES = tuple((K, a, n, m, True)
                        for K, a in ((52, BF16X3), (20, BF16X3), (30, F32))
                        for n, m in ((1, M_ALIGNED), (33, M_ALIGNED), (N_BODY, 4), (N_BODY, 3), (N_BODY, 256)))

# inactive cells of the body shape: a whole work-group of 256 cells (two of 128); one of 128 cells inside an otherwise active 256;
# scattered cells, the ends of tiles and groups among them
def inactive_patterns(n=N_BODY):
    """{name: active flags [n] uint8}; fewer patterns where n is too small for them."""
    pats = {}
    if n > 256:
        pats['group-of-256'] = np.ones(n, dtype=np.uint8)
        pats['group-of-256'][:256] = 0
        pats['group-of-128'] = np.ones(n, dtype=np.uint8)
        pats['group-of-128'][128:256] = 0
    if n > 1:
        pats['scattered'] = np.ones(n, dtype=np.uint8)
        pats['scattered'][[i for i in (0, 31, 32, 127, 128, 200, 255, 256, 257, 290, n - 1) if i < n]] = 0
    return pats

# ---- oriana_zi_gene_rate -----------------------------------------------------------------------------------------------------
# Long batches, one per NT: 32 x 4096 + 32 x 33 cells cut into GENE_RATE_RANGES = 32 ranges of 4160 cells -- a range leaves the
# matrix core every 256 cells, spills to float64 after 4096 and goes on for two tiles more (the second and last spill adds to
# the partial); the last range (3168 cells) spills once.  36 genes: a full strip, a strip of four, two empty waves.
GENE_RATE_RANGES = 32
LONG_N, LONG_M = 32 * 4096 + 32 * 33, 36
GENE_RATE_LONG_KS = (20, 50, 80, 128)
# one batch whose ranges (288 cells) pass the flush at 256 cells and no spill
MID_N, MID_M, MID_K = 9216, 36, 33
# edge shapes of the other two entries at one K: (n, m), every gene real.  oriana_zi_gene_rate is specified for gene counts that
# are multiples of 4 only: it takes those.
GENE_EDGE_K = 30
EDGE_SHAPES = ((1, M_ALIGNED), (33, M_ALIGNED), (N_BODY, 4), (N_BODY, 3), (N_BODY, 256))
GENE_RATE_EDGE_SHAPES = tuple(s for s in EDGE_SHAPES if s[1] % 4 == 0)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def inputs(K, n=N_BODY, m=M_REAL):
    """(X (n, m), U (n, K), V (m, K), pi_d [m]) float64, made once per (K, n, m); U, V and pi_d read-only (X goes through
    torch.from_numpy in the packer: left writable, never written)."""
    return _inputs(int(K), int(n), int(m))


@functools.lru_cache(maxsize=None)
def _inputs(K, n, m):
    assert m >= 3 and n >= 1 and K >= 1
    rng = np.random.default_rng([K, n, m])
    V = rng.gamma(2.0, 0.5, size=(m, K))
    U = rng.gamma(1.0, 1.0, size=(n, K))
    U /= float(V.sum(axis=0) @ U.sum(axis=0)) / (n * m)           # mean of U V^T, without forming it
    pi_d = rng.uniform(0.05, 0.95, size=m)
    pi_d[PI_ZERO], pi_d[PI_ONE] = 0.0, 1.0
    X = rng.poisson(0.4, size=(n, m)).astype(np.float64)
    X[:, ZERO_GENE] = 0
    if n > 1:
        X[min(ZERO_CELL, n - 1)] = 0
    return (X,) + _frozen(U, V, pi_d)


def middle_fraction(d):
    """The share of the dropout posteriors that the sigmoid decides."""
    return float(((d > 0.01) & (d < 0.99)).mean())
