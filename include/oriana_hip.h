/*
 * oriana_hip.h -- C ABI of the MI355X (gfx950) CAVI engine for probabilistic count matrix
 * factorisation.  This is the drop-in boundary for the hot path of AntoinePassemiers/Oriana:
 * every entry point names the reference interface it replaces (paths relative to the reference
 * repository root).  Plain pointers and sizes only; all pointers are DEVICE pointers unless a
 * parameter is documented as host.  Calls are asynchronous on `stream` (a hipStream_t passed as
 * void*; NULL = the default stream).  Return value: 0 on success, a negative code otherwise
 * (-1000 - hipError_t for HIP errors, ORIANA_E* for argument errors); nothing is thrown.
 * The library keeps no global state; all scratch memory is supplied by the caller.
 *
 * Layouts
 *   - "dense (r, K) f32/f64": C-contiguous, exactly the reference's ndarray layout
 *     (oriana/parameters.py:8-32 holds float64 buffers; the kernels take float32, gap.py:67).
 *   - "factor matrix (r, Kp) f32": K padded with zeros to Kp = oriana_kpad(K); row-major.
 *   - oriana_counts: the count matrix X (constant across sweeps, oriana/models/gap.py:29-32)
 *     repacked once into 256 x 256 tiles that keep only the non-zero counts; see DESIGN.md.
 */
#ifndef ORIANA_HIP_H
#define ORIANA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORIANA_TILE 256

#define ORIANA_EINVAL   (-1)   /* bad argument (NULL pointer, negative size, K out of range) */
#define ORIANA_EKRANGE  (-2)   /* K larger than the largest compiled configuration */
#define ORIANA_EQUIRK   (-3)   /* reference_quirks needs K <= m (zigap.py:94 reads D_hat[i, k]) */
#define ORIANA_EUNIT    (-4)   /* a hybrid resident handle serves the ZI nests under oriana_counts_declare_unit_dropout only */

/* 8-byte record of one slot of the row-side stream.  x == 0 marks a padding slot. */
typedef struct {
    float    x;     /* the count, as float32 (gap.py:94 casts X to float32); 0 = padding */
    uint16_t cdst;  /* slot of this entry inside the tile's column-side region */
    uint8_t  col;   /* column inside the tile */
    uint8_t  pad;
} oriana_rowrec;

/* Tiled, sliced non-zero layout of one row shard of X (built once by oriana_pack_*).
 *
 * X is cut into 256 x 256 tiles (row-block-major).  Inside a tile the non-zeros are stored twice:
 *   - row side: the tile's 256 rows form 16 slices of 16 rows.  A slice is a sequence of
 *     "iterations" of 64 slots = 16 rows x 4 consecutive records of that row (slot = iteration*64 +
 *     row_in_slice*4 + u); a row's records are in increasing column order; rows shorter than the
 *     longest row of the slice are padded (x = 0).  One wave-wide 512-byte load fetches an iteration.
 *   - column side: the same with 16-column slices; slot = iteration*64 + col_in_slice*4 + u holds
 *     the tile row index (ridx) and, in the per-sweep array `s`, the scalar s_ij of that entry;
 *     a column's entries are in increasing row order.  The last 64 slots of a tile's column-side
 *     region are write-only dummies (target of the padding lanes' stores).
 * All arrays live in device memory and are owned by the caller (the Python host allocates them as
 * torch tensors; rowrec and ridx must be zero-filled before oriana_pack_fill). */
typedef struct {
    int64_t n, m;                 /* rows (cells) in this shard, columns (genes) */
    int64_t nrb, ncb;             /* ceil(n / 256), ceil(m / 256) */
    int64_t nnz;                  /* non-zero entries */
    int64_t rslots, cslots;       /* total slots of the row-side / column-side streams */
    const int64_t       *roff;       /* [nrb*ncb + 1] first row-side slot of tile (rb, cb), rb-major */
    const int64_t       *coff;       /* [nrb*ncb + 1] first column-side slot of the tile */
    const uint32_t      *rslice;     /* [nrb*ncb][17] slot offsets of the 16-row slices inside the tile */
    const uint32_t      *cslice;     /* [nrb*ncb][17] slot offsets of the 16-column slices inside the tile */
    const oriana_rowrec *rowrec;     /* [rslots] */
    const uint8_t       *ridx;       /* [cslots] row inside the tile */
    /* Optional internal orderings (NULL = identity): packed column c holds gene col_perm[c], packed
     * row r holds cell row_perm[r].  Sorting genes (and cells) by their non-zero count puts
     * entries of similar density in the same tile, which shortens the padding of the slices.
     * All dense inputs / outputs of the API stay in the caller's order: the permutation is applied
     * by oriana_factor_prep (gather), oriana_finalize (scatter) and oriana_fixup. */
    const int32_t       *col_perm;   /* [m] */
    const int32_t       *row_perm;   /* [n] */
} oriana_counts;

/* Kp for a given K (0 if K is out of range). */
int64_t oriana_kpad(int64_t K);
/* Column tiles (of 256 genes) one work-group of oriana_col_pass covers for this K: the "column block" of a work
 * item indexes groups of this many adjacent tiles (2 for K <= 116, where one image of the row block serves two
 * tiles; 1 for the wider K; 0 if K is out of range). */
int64_t oriana_col_block_tiles(int64_t K);
/* Library / build identification ("oriana_hip gfx950 <version>"). */
const char *oriana_version(void);

/* ---- packing the count matrix (replaces `self.X[:].astype(np.float32)`, gap.py:94) --------
 * Two passes over dense row chunks (a chunk starts at a multiple of 256 rows):
 *   1. oriana_pack_count   -> per-tile nnz / slot counts and the slice offsets
 *   2. oriana_pack_offsets -> roff, coff and the two slot totals; (caller) zero-filled rowrec, ridx of those sizes
 *   3. oriana_pack_fill    -> rowrec / ridx (/ side_nz)
 * X is dense (rows, m) with leading dimension ldx (elements), float32 or (xdtype = 1) int64 /
 * (xdtype = 2) int32 / (xdtype = 3) float64.  rb0 = first row block of the chunk.
 */
int oriana_pack_count(const void *X, int xdtype, int64_t rows, int64_t m, int64_t ldx,
                      int64_t rb0, int64_t ncb,
                      int32_t *tile_nnz,      /* [nrb*ncb] */
                      int32_t *tile_rslots,   /* [nrb*ncb] */
                      int32_t *tile_cslots,   /* [nrb*ncb] (includes the 64 dummy slots) */
                      uint32_t *rslice,       /* [nrb*ncb][17] */
                      uint32_t *cslice,       /* [nrb*ncb][17] */
                      void *stream);
int oriana_pack_fill(const void *X, int xdtype, int64_t rows, int64_t m, int64_t ldx,
                     int64_t rb0, int64_t ncb, const int64_t *roff, const int64_t *coff,
                     const uint32_t *rslice, const uint32_t *cslice,
                     oriana_rowrec *rowrec, uint8_t *ridx,
                     /* optional: gather a dense (rows, m) f32 side matrix (D_hat) at the non-zeros,
                      * row-side slot order */
                     const float *side, int64_t ldside, float *side_nz,
                     void *stream);
/* Step 2, the one scan of every host (csrc/pack_nest.h, engine.py).  DEVICE: tile_rslots, tile_cslots [nt] (in; may be NULL
 * when nt == 0), roff, coff [nt + 1] (out).  HOST: totals [2] (out) = {roff[nt], coff[nt]}, the row-side and column-side slots
 * that size the record arrays.  SYNCHRONISES the stream. */
int oriana_pack_offsets(int64_t *roff, int64_t *coff, const int32_t *tile_rslots, const int32_t *tile_cslots, int64_t nt,
                        int64_t *totals, void *stream);

/* ---- factor preparation ---------------------------------------------------------------------
 * From E[log U] (gamma.py:52-61 output, dense (r, K) f32) build the factor matrix
 *   F[i, k] = exp(l[i, k] - mu[i]) * (mask ? mask[i, k] : 1),   mu[i] = max_k l[i, k],
 * the shift being undone analytically (softmax is shift invariant, gap.py:74-78).  Rows whose
 * shift is too large for the shifted form to reproduce the reference's float32 behaviour are
 * zero-filled: every entry that touches them fails the den test and is evaluated by the exact slow
 * path (oriana_fixup).
 */
int oriana_factor_prep(float *F, float *mu, const float *logF, const float *mask,
                       const int32_t *row_index,   /* F row i is built from logF row row_index[i] (NULL: i) */
                       int64_t r, int64_t K, void *stream);
/* Both sides at once, with the validity test CENTRED on the two sides' typical shifts: only the sums
 * lu[i,k] + lv[j,k] enter the loop nests (gap.py:74), and the iterations drift along the scale indeterminacy
 * (U c, V / c) -- a row takes the shifted form iff its shift lies within A_side of the mean shift of its side, A_u + A_v
 * chosen (and shared in proportion to the sides' spreads) so that every sum of two accepted shifts keeps the
 * reference's own float32 denominator normal.  Same F as
 * oriana_factor_prep wherever both accept a row.  maskV: S_tilde of the sparse models or NULL; scratch:
 * oriana_prep_scratch_bytes() bytes of device memory, ZEROED once before the first call (per-group partial sums of the
 * row maxima, added up in a fixed order by the last group to finish: no float atomics, nothing to clear between
 * calls, safe inside a captured graph). */
int oriana_factor_prep_pair(float *FU, float *FV, const float *logU, const float *logV, const float *maskV,
                            const int32_t *row_index_u, const int32_t *row_index_v,
                            int64_t n, int64_t m, int64_t K, float *scratch, void *stream);
/* The same with a list of buffers that the second launch zero-fills on the side (the outputs and scratch the passes of
 * a sweep accumulate into -- Z_i, Z_j, C, tile_flag, the float64 column sums): on a small matrix (configs[1]) the fill
 * kernels were a seventh of the sweep.  Each entry: a 4-byte aligned pointer and a byte count that is a multiple of 4
 * (0 = unused).  clr may be NULL. */
#define ORIANA_CLEAR_MAX 8
typedef struct oriana_clear_list {
    void   *ptr[ORIANA_CLEAR_MAX];
    int64_t bytes[ORIANA_CLEAR_MAX];
} oriana_clear_list;
int oriana_factor_prep_pair_clear(float *FU, float *FV, const float *logU, const float *logV, const float *maskV,
                                  const int32_t *row_index_u, const int32_t *row_index_v,
                                  int64_t n, int64_t m, int64_t K, float *scratch, const oriana_clear_list *clr,
                                  void *stream);
/* [r5] The cell side prepared by the Gamma update that produced E[log U] (oriana_gamma_update_prep /
 * oriana_gamma_update_finalize_prep below: FU holds exp(E[log U] - row maximum) of every row, mu_u [n] the row maxima (NaN: the
 * row holds a NaN), upart [4 * nupart] the per-group partial statistics of the maxima): this call combines the statistics,
 * prepares the gene side from logV, overwrites the cell rows the centred validity test rejects, and zero-fills `clr` -- the
 * 2 x 4 K n bytes of reading E[log U] twice (statistics, preparation) and the second write of FU disappear from the sweep
 * (0.9 ms of 2.9 ms outside the passes at 1M x 30k, K = 100).  Same F and same statistics as oriana_factor_prep_pair up to the
 * summation order of the partials. */
int oriana_factor_prep_pair_fused(float *FU, const float *mu_u, const float *upart, int64_t nupart, float *FV,
                                  const float *logV, const float *maskV, const int32_t *row_index_v,
                                  int64_t n, int64_t m, int64_t K, float *scratch, const oriana_clear_list *clr, void *stream);
int64_t oriana_prep_scratch_bytes(void);   /* includes 4096 bytes for the log-sum centres at oriana_prep_center_offset() */
int64_t oriana_prep_center_offset(void);

/* ---- the responsibility pass ----------------------------------------------------------------
 * Replaces the loop nests  GaP.compute_Z_q_expectations        (oriana/models/gap.py:67-80)
 *                          ZIGaP.compute_Z_q_expectations      (oriana/models/zigap.py:79-95)
 *                          SparseGaP.compute_Z_q_expectations  (oriana/models/sparse_gap.py:81-97)
 *                          SparseZIGaP.compute_Z_q_expectations(oriana/models/sparse_zigap.py:100-116)
 * in three kernels over the tiled non-zeros:
 *   oriana_row_pass : s_ij = x_ij / sum_k FU[i,k] FVden[j,k]   and   R[i,:] = sum_j w_ij s_ij FVacc[j,:]
 *   oriana_col_pass : C[j,:] (+)= sum_i s_ij G[i,:]
 *   oriana_fixup    : entries the shifted form cannot represent (NaN sentinel in s) are evaluated
 *                     exactly as the reference does (expf of the sum, den > 0 guard) and added
 *                     with atomics to the dense outputs.
 */
int oriana_row_pass(const oriana_counts *cm,
                    const float *FU,        /* (n, Kp) */
                    const float *FV,        /* (m, Kp) */
                    const float *w_nz,      /* [rslots] per-entry weight (D_hat at the non-zeros) or NULL = 1 */
                    float *R,               /* (n, Kp) out -- left untouched when s_rs is given (the pass then only produces s) */
                    float *s_cs,            /* [cslots] out: s_ij (unweighted), column-side slots; padding slots must hold 0 */
                    float *sw_cs,           /* [cslots] out: w_ij s_ij (required iff w_nz) */
                    float *s_rs,            /* [rslots] out: s_ij, row-side slots, or NULL */
                    int32_t *tile_flag,     /* [nrb*ncb] out: 1 if the tile holds slow-path entries (zero it first) */
                    int64_t K, void *stream);

/* The plain row pass (w_nz = NULL, no row-side copy of s) with the gene tiles of every row block split over
 * `gene_splits` work-groups: a row block is one work-group, so a matrix of 10,000 cells (configs[1]) ran the pass on 40
 * of the 256 CUs.  R is then (gene_splits, n, Kp): every group stores the row sums of its gene range in its own slab
 * (no atomics, nothing to clear); oriana_finalize_slabs / oriana_gamma_update_finalize add the slabs up.  The split that
 * fills the chip: oriana_row_pass_plan below (a short matrix: every row block; a long one: the row blocks of the last round).
 * Forwards to oriana_row_pass_general (as oriana_row_pass does: the arguments are validated there). */
int oriana_row_pass_split(const oriana_counts *cm, const float *FU, const float *FV, float *R, float *s_cs,
                          int32_t *tile_flag, int64_t K, int64_t gene_splits, void *stream);

/* [r4] Which work-groups of the row pass share a row block.  The two-lane kernels (33 <= Kp <= 64, 85 <= K <= 100) run one
 * 512-thread group per CU, so the pass advances in ROUNDS of 256 row blocks and the last, partly filled round costs a whole
 * one (measured at 1M x 30k, K = 100: 3840 / 3907 / 4096 row blocks = 33.9 / 35.8 / 36.2 ms).  The row blocks [0, nfull) --
 * the full rounds -- are one work-group each (all gene tiles, row sums in slab 0 of R); every row block from nfull on is
 * `parts` work-groups: part p takes the gene tiles [edge[p], edge[p+1]) and stores its row sums in slab p, so the last round
 * is made of shorter groups.  nfull = 0 is the split of oriana_row_pass_split (short matrices); nfull = nrb, parts = 1 no
 * split at all.  R = (parts, n, Kp); the rows below 256 * nfull have slab 0 only (oriana_finalize_slabs_from). */
typedef struct oriana_row_split {
    int32_t nfull;
    int32_t parts;          /* 1 .. 8 */
    int32_t edge[9];        /* edge[0] = 0 <= ... <= edge[parts] = ncb */
} oriana_row_split;

/* The split that fills the chip for this matrix and K.
 * tile_cost: HOST array of ncb relative costs of the gene tiles (the ranges are cut at equal-cost points; genes are packed
 * by decreasing density, so equal tile counts are not equal work) or NULL = equal.  ORIANA_ROW_SPLIT_ROUNDS=off: only the
 * short-matrix rule. */
int oriana_row_pass_plan(const oriana_counts *cm, int64_t K, const double *tile_cost, oriana_row_split *out);

/* [r5] The same for a given number of compute units (oriana_row_pass_plan uses oriana_device_cus()): host code only, no
 * device call -- the plan of a 128-, 256- or 304-CU part can be formed (and tested) anywhere. */
int oriana_row_pass_plan_cus(const oriana_counts *cm, int64_t K, const double *tile_cost, int64_t cus, oriana_row_split *out);
/* Compute units of the device the calling thread has selected (hipDeviceAttributeMultiprocessorCount, cached per device;
 * the environment's ORIANA_CUS overrides; 256 where no device is visible): the "rounds of the chip" every plan counts in. */
int64_t oriana_device_cus(void);

/* [r4] Every variant of the row pass behind one entry, under a split (NULL = none); s_rs given: R untouched.  FV2 given (s_rs
 * must be NULL): the row pass of the sparse models with the S_hat-weighted sums folded in (sparse_gap.py:88-95) -- the dot
 * product runs against FV (= exp-shifted E[log V] masked by S_tilde), the accumulation against FV2 (= FV * S_hat), both staged
 * side by side in LDS, so R[i,:] = sum_j w_ij s_ij FV2[j,:] comes out of this pass and oriana_row_spmm is not needed;
 * ORIANA_EKRANGE when the two images of 256 factor rows do not fit (Kp > 64): run the pass with s_rs, then oriana_row_spmm.
 * Kernels other than the two-lane ones take nfull = 0 only (ORIANA_EINVAL otherwise) and cut their ranges evenly. */
int oriana_row_pass_general(const oriana_counts *cm, const float *FU, const float *FV, const float *FV2,
                            const float *w_nz, float *R, float *s_cs, float *sw_cs, float *s_rs, int32_t *tile_flag,
                            int64_t K, const oriana_row_split *split,
                            const float *den_min,   /* device: the den threshold (scratch of oriana_factor_prep_pair +
                                                       oriana_prep_den_threshold_offset()); NULL = the constant 1e-10 */
                            void *stream);
/* [r4] The den threshold of the shifted form: s = x / den' is trusted when den' >= threshold, below it the entry takes the
 * exact slow path (oriana_fixup).  The guarantee behind it is that the reference's own float32 den = exp(mu_i + mv_j) den'
 * is a normal number with room to spare (>= 3e-30); with the smallest sum mu_i + mv_j of the factor matrices at hand
 * (row statistics of oriana_factor_prep_pair) the threshold is 3e-30 exp(-sum_lo) in [1e-25, 1e-10] instead of the
 * worst-case constant 1e-10 -- ZI-pCMF drifts along U c, V / c and after 25 sweeps at configs[2] a third of the tiles
 * held entries between the two.  ORIANA_DEN_THRESHOLD=fixed keeps the constant. */
int64_t oriana_prep_den_threshold_offset(void);

/* R[i,:] = sum_j w_ij s_ij FV[j,:] with s given in row-side slots (sparse models: S_hat-weighted sums). */
int oriana_row_spmm(const oriana_counts *cm, const float *s_rs, const float *w_nz,
                    const float *FV, float *R, int64_t K, void *stream);
/* The same product for a fold-in of the sparse models, where most cells are frozen after a few iterations: `active` [n]
 * bytes in the CALLER's row order (cm->row_perm maps the packed rows onto it).  A work-group none of whose rows (256, 128 or
 * 64 consecutive packed rows, by K) is active returns at once and leaves its rows of R as they are; the rows of every other
 * group, active or not, are computed exactly as oriana_row_spmm computes them (bit for bit).  active == NULL is oriana_row_spmm. */
int oriana_row_spmm_active(const oriana_counts *cm, const float *s_rs, const float *w_nz,
                           const float *FV, float *R, const uint8_t *active, int64_t K, void *stream);

int oriana_col_pass(const oriana_counts *cm, const float *s_cs,
                    const float *G,         /* (n, Kp) */
                    float *C,               /* (m, Kp) accumulated with atomics: zero it first */
                    int64_t K,
                    /* optional work list [nwork][3] = (column block, first row block, end row block):
                     * one workgroup per item; a column block is oriana_col_block_tiles(K) adjacent column
                     * tiles; items should carry similar slot counts (genes differ widely in density).
                     * NULL / 0: uniform row bands. */
                    const int32_t *work, int64_t nwork,
                    void *stream);

/* Two products over ONE walk of the column-side stream: C1 += s G1 and C2 += s G2 (the sparse models' per-gene sums
 * and log sums, sparse_gap.py:96-97), both images of a row block side by side in LDS.  `work`: items
 * (column TILE, first row block, end row block) -- one tile per item, whatever oriana_col_block_tiles(K) says.
 * Returns ORIANA_EKRANGE when two images do not fit (Kp > 64): call oriana_col_pass twice then. */
int oriana_col_pass_dual(const oriana_counts *cm, const float *s_cs, const float *G1, const float *G2, float *C1,
                         float *C2, int64_t K, const int32_t *work, int64_t nwork, void *stream);
/* [r6] Analysis entry, not on the path of a sweep: the same sums with float64 accumulators in a fixed order and one rounding to
 * float32 at the end (C += f32(sum_i s_ij G_i)): the most a compensated accumulation of the float32 kernels could reach
 * (tools/parity_report.py: ORIANA_COL_F64=1 routes the per-gene sums of the sparse models' log sums through it). */
int oriana_col_pass_f64acc(const oriana_counts *cm, const float *s_cs, const float *G, float *C, int64_t K, void *stream);
/* Deterministic debug mode of the column pass (no counterpart in the reference, which is
 * single-threaded): every work item stores its accumulators in its own slab of `scratch`
 * (oriana_col_pass_det_scratch_bytes(K, nwork) bytes) instead of adding them to C with float atomics, and a
 * second kernel adds the slabs of each column block to C in work-item order.  Two runs give bit-identical C;
 * the default path differs from it only by the order of the float32 additions.  Needs a work list. */
int64_t oriana_col_pass_det_scratch_bytes(int64_t K, int64_t nwork);
int oriana_col_pass_det(const oriana_counts *cm, const float *s_cs, const float *G, float *C, int64_t K,
                        const int32_t *work, int64_t nwork, float *scratch, void *stream);

/* ---- the densest genes on the matrix cores (hybrid layout) --------------------------------------------------
 * Same loop nest (oriana/models/gap.py:67-80), other evaluation: the first `gd` PACKED genes (the densest ones, a
 * multiple of 32; the host picks them from a density threshold) are kept as a dense uint16 block instead of the
 * sliced non-zero layout; the oriana_counts of a hybrid layout then covers the packed genes [gd, m) only (its
 * col_perm, FV and C pointers are the full arrays advanced by gd rows).  Their share of the pass,
 *     den = FU FV^T,  s = x / den,  R += S FV,  C += S^T FU,
 * runs as matrix products on the bf16 matrix cores in float32-EQUIVALENT arithmetic: every float32 operand enters as
 * its exact three-way bf16 split (24 bits), six cross products per term, float32 accumulation, no sum longer than one
 * tile on the matrix core (csrc/dense_pass.hip; DESIGN.md section 7 has the measured error).  Entries whose
 * denominator fails the test of the sparse side get the same NaN sentinel and the same exact slow path.
 * Counts must be integers in [0, 65535) for a gene to be eligible (the host checks). */
typedef struct {
    int64_t n;             /* cells of this shard */
    int64_t gd;            /* dense genes = packed columns [0, gd), multiple of 32 */
    int64_t nct;           /* allocated cell tiles of 32 rows: 8 * ceil(n / 256) */
    const uint16_t *x;     /* [nct][gd / 32][1024] counts, register order of the row kernel (dense_pass.hip) */
} oriana_dense;

/* 1 if the dense evaluation is compiled for this K (K <= 100). */
int oriana_dense_supported(int64_t K);
/* 16-byte pieces of one 32-row tile's operand image; side 0 = gene side (FV), 1 = cell side (FU). */
int64_t oriana_dense_image_pieces(int64_t K, int side);
/* Pack `rows` rows (a multiple of 32 unless they are the last ones) of the already column-permuted dense chunk X
 * (columns [0, gd), leading dimension ldx, dtypes as oriana_pack_count) into cell tiles ct_first.. of xd. */
int oriana_dense_pack(const void *X, int xdtype, int64_t rows, int64_t gd, int64_t ldx, int64_t ct_first,
                      uint16_t *xd, void *stream);
/* Split operand images of a padded (rows, Kp) factor matrix, one per tile of 32 rows: img holds
 * ceil(rows / 32) * oriana_dense_image_pieces(K, side) * 16 bytes. */
int oriana_dense_images(void *img, const float *F, int64_t rows, int64_t K, int side, void *stream);
/* Row side: S (nct * gd/32 * 1024 floats, out) and R[i,:] += sum_j s_ij FV[j,:] over the dense genes (R must hold the
 * sparse genes' sums or zeros; added with atomics when gene_splits > 1).  flag: [nct][gd / 32] out (every entry written:
 * 1 where the tile of s holds sentinels).  [r4] tail_parts > 1: the 256-cell blocks from tail_nfull on are split into
 * tail_parts even gene-tile ranges, part p ADDING into slab p of R = (tail_parts, n, Kp) (struct oriana_row_split: the same rows
 * as the sliced row pass of a hybrid layout splits; gene_splits must be 1 then).  tail_parts <= 1: no such split. */
int oriana_dense_row_pass_tail(const oriana_dense *d, const float *FU, const void *imgV, float *R, float *S,
                          int32_t *flag, int64_t K, int64_t gene_splits, int64_t tail_nfull, int64_t tail_parts,
                               const float *den_min /* as oriana_row_pass_general */, void *stream);
/* Gene side: C[j,:] += sum_i s_ij FU[i,:] for the dense genes (atomics: zero C first), imgU = the cell-side images. */
int oriana_dense_col_pass(const oriana_dense *d, const void *imgU, const float *S, float *C, int64_t K,
                          int64_t cell_splits, void *stream);
/* Exact slow path for the flagged tiles of every nest (adds to the dense outputs Z_hat_i, Z_hat_j; clears the sentinels in S):
 * Z_log (zigap.py:95, sparse_gap.py:97; may be NULL), the D_hat[i, k] weight of zigap.py:94 on the gene side (Z_hat_j[j, k] +=
 * dq[i, k] r_ijk; dq: (n, K) float32, caller's cell order; may be NULL), the masks of the sparse models (S_tilde, S_hat: both or
 * neither; (m, K) float32, caller's gene order).  zj_packed != 0: Z_hat_j is indexed by the PACKED gene index (the row-sharded
 * pCMF sweep exchanges the per-gene sums in packed order). */
int oriana_dense_fixup_variant(const oriana_dense *d, const int32_t *flag, float *S, const float *logU, const float *logV,
                               const int32_t *row_perm, const int32_t *col_perm, float *Z_hat_i, float *Z_hat_j,
                               float *Z_log, const float *dq, const float *S_tilde, const float *S_hat, int64_t K,
                               int zj_packed, void *stream);
/* oriana_dense_images with the second image (the operand of the accumulation R += S F2 and its tail pieces) taken from F2:
 * the sparse models accumulate against FV * S_hat while den runs against the masked FV (sparse_gap.py:88-95). */
int oriana_dense_images2(void *img, const float *F, const float *F2, int64_t rows, int64_t K, int side, void *stream);
/* D_hat[i, j] = value at every non-zero count of the dense genes (zigap.py:77, 135); D_hat: (n, ld) float32, caller's
 * cell / gene order. */
int oriana_dense_fix_nz(const oriana_dense *d, float *D_hat, int64_t ld, const int32_t *row_perm, const int32_t *col_perm,
                        double value, void *stream);

/* Count statistics / deviance sums of the dense genes (the share of oriana_count_stats and oriana_metric_nnz that the
 * sliced layout of a hybrid matrix does not cover): colsum, colnnz (caller's gene order), out2 += {sum (x log x - x),
 * sum x^2}; with U, V (dense float64 (n, K), (m, K)): out4 += {sum Lambda, sum x log Lambda, sum Lambda^2,
 * sum x Lambda} over the non-zero counts, Lambda = U V^T in float64.  Any output may be NULL. */
int oriana_dense_metric(const oriana_dense *d, const double *U, const double *V, const int32_t *row_perm,
                        const int32_t *col_perm, double *colsum, double *colnnz, double *out2, double *out4,
                        int64_t K, void *stream);

/* Z[o,k] = (accumulate ? Z[o,k] : 0) + F[i,k] * R[i,k] (* mul[o,k] if mul), o = row_index ? row_index[i] : i
 * -- dense (r, K) out from padded (r, Kp) in. */
int oriana_finalize(float *Z, const float *F, const float *R, const float *mul, const int32_t *row_index,
                    int64_t r, int64_t K, int accumulate, void *stream);

/* Z[o,k] += F[i,k] * (R[0][i,k] + ... + R[nslab-1][i,k]) -- R = (nslab, r, Kp) as oriana_row_pass_split leaves it. */
int oriana_finalize_slabs(float *Z, const float *F, const float *R, int64_t nslab, const int32_t *row_index,
                          int64_t r, int64_t K, void *stream);
/* [r4] the same where only the rows from slab_row0 on have more than slab 0 (oriana_row_split: slab_row0 = 256 * nfull). */
int oriana_finalize_slabs_from(float *Z, const float *F, const float *R, int64_t nslab, int64_t slab_row0, const int32_t *row_index,
                          int64_t r, int64_t K, void *stream);

/* Slow path (exact reference arithmetic) for the entries flagged by oriana_row_pass.
 * variant bit 0: S_tilde / S_hat present (sparse models); bit 1: D_hat weights (w_nz);
 * bit 2: reference quirk zigap.py:94 (dq = D_hat[:, :K] dense (n, K)).
 * Adds into Zi (n, K), Zj (m, K), Zlog (m, K) (any may be NULL) and rewrites the sentinels in
 * s_cs / sw_cs / s_rs as 0. */
int oriana_fixup(const oriana_counts *cm, const int32_t *tile_flag,
                 float *s_cs, float *sw_cs, float *s_rs,
                 const float *logU, const float *logV,
                 const float *S_tilde, const float *S_hat,
                 const float *w_nz, const float *dq,
                 float *Zi, float *Zj, float *Zlog,
                 int64_t K, int variant, void *stream);

/* ---- deviance / Frobenius metrics (base.py:58-87 with loglikelihood_X, sparse_zigap.py:44-51) --------
 * The metrics split into sums over the stored (non-zero) entries, sums over the zero entries and closed
 * forms of column sums (oriana_amd/models/base.py:_metric_terms spells the algebra out).
 *   oriana_factor_cast_f32 : F (r, Kp) f32 = float32(E[row_index[i], :] (* mul)) -- with these factors
 *                            oriana_row_pass leaves s_ij = x_ij / Lambda_ij in s_rs
 *   oriana_metric_nnz      : out4 += { sum Lambda, sum x log Lambda, sum Lambda^2, sum x Lambda } over the stored
 *                            entries (Lambda = x / s; entries with the NaN sentinel are recomputed in f64)
 *   oriana_count_stats     : constants of X: per-gene sums and non-zero counts, sum (x log x - x), sum x^2
 *   oriana_dropout_metric  : out2 += { sum log(pi_j exp(-Lambda_ij) + 1 - pi_j), sum Lambda_ij^2 } over the
 *                            entries with X == 0 and round(D_hat) == 1 (the mask of base.py:60-61, 67);
 *                            Lambda = U V^T on the f64 matrix cores, never stored
 */
int oriana_factor_cast_f32(float *F, const double *E, const float *mul, const int32_t *row_index,
                           int64_t r, int64_t K, void *stream);
int oriana_metric_nnz(const oriana_counts *cm, const float *s_rs, const double *U, const double *V,
                      int64_t K, double *out4, void *stream);
int oriana_count_stats(const oriana_counts *cm, double *colsum, double *colnnz, double *out2, void *stream);
int oriana_dropout_metric(double *out2, const float *D_hat, const double *U, const double *V, const double *pi_d,
                          const uint32_t *nzmask, int64_t n, int64_t m, int64_t K, void *stream);

/* ---- the deviance along a prefix of the factors (oriana_amd/models/base.py: deviance_path) ----------------------
 * Lambda^(k)_ij = sum_{l < k} U_il V_jl over the first k columns of the factors handed in (the caller has put the columns
 * into its factor order).  ends: int32 device array of n_ends prefix lengths, strictly increasing, within 1..K (an end
 * above K is read as K).  out: (n_ends, 2) float64, out[e] += { sum Lambda^(ends[e]), sum x log Lambda^(ends[e]) } over the
 * non-zero counts (float64 atomics per work-group; the caller zeroes it).  A prefix whose rate is exactly 0 at a non-zero
 * count gives -inf in out[e, 1] for that e.
 *   oriana_metric_nnz_prefix   : the stored entries of the sliced layout, walked once.  FU (n, Kp), FV (m, Kp): float32
 *                                images of oriana_factor_cast_f32 in packed row / gene order (hybrid layout: FV advanced to
 *                                the packed gene gd); the running sum is float32 and a value below 1e-10, zero, NaN or
 *                                infinite at an end is replaced by the float64 sum of U (n, K), V (m, K) (caller's row /
 *                                gene order, found through row_perm / col_perm as in oriana_metric_nnz).  K <= 256.
 *   oriana_dense_metric_prefix : the non-zero counts of the dense genes of a hybrid layout, float64 throughout
 *                                (K <= 1024, as oriana_dense_metric).
 * Both return ORIANA_EINVAL on a missing pointer, K <= 0 or n_ends outside 0..K, and 0 without a launch for an empty
 * problem (no stored entry, no dense gene, n_ends == 0). */
int oriana_metric_nnz_prefix(const oriana_counts *cm, const float *FU, const float *FV, const double *U, const double *V,
                             int64_t K, const int32_t *ends, int64_t n_ends, double *out, void *stream);
int oriana_dense_metric_prefix(const oriana_dense *d, const double *U, const double *V, const int32_t *row_perm,
                               const int32_t *col_perm, int64_t K, const int32_t *ends, int64_t n_ends, double *out,
                               void *stream);

/* ---- the deviance per gene and per cell (oriana_amd/models/base.py: gene_deviance, cell_deviance) -----------------
 * The sums of the metrics kept along one axis.  gene_out: (m, 3) float64 in the caller's gene order, cell_out: (n, 5) float64
 * in the caller's row order; every entry ADDS into them with float64 atomics (the caller zeroes them; reruns agree to the
 * order of the additions), and a NULL output skips that axis (both NULL: ORIANA_EINVAL).
 *   gene_out[j] += { sum Lambda, sum x log Lambda, sum (x log x - x) } over the non-zero counts of gene j
 *   cell_out[i] += the same three over the non-zero counts of cell i, then { sum gene_const[j][0],
 *                  sum (gene_const[j][1] + x gene_const[j][2]) }; gene_const: (m, 3) float64 in the caller's gene order,
 *                  needed with cell_out only; the row of a gene without a non-zero count is never used
 *   oriana_metric_nnz_axes     : the stored entries of the sliced layout, Lambda as oriana_metric_nnz takes it (x / s from
 *                                the row pass, the float64 sum of U, V for the NaN sentinel and for 0).  K <= 256
 *                                (ORIANA_EKRANGE above).
 *   oriana_dense_metric_axes   : the non-zero counts of the dense genes of a hybrid layout, float64 throughout (K <= 1024).
 *   oriana_dropout_metric_axes : gene_out (m,) and cell_out (n,) += log(pi_j exp(-Lambda_ij) + 1 - pi_j) over the entries
 *                                with X == 0 and D_hat > 0.5 -- the term of oriana_dropout_metric per axis, on the f64
 *                                matrix cores; m is the padded gene count of D_hat's rows.  ORIANA_EKRANGE for K > 256.
 * All three return ORIANA_EINVAL on a missing pointer or K <= 0 before any HIP call, and 0 without a launch for an empty
 * problem. */
int oriana_metric_nnz_axes(const oriana_counts *cm, const float *s_rs, const double *U, const double *V, int64_t K,
                           const double *gene_const, double *gene_out, double *cell_out, void *stream);
int oriana_dense_metric_axes(const oriana_dense *d, const double *U, const double *V, const int32_t *row_perm,
                             const int32_t *col_perm, int64_t K, const double *gene_const, double *gene_out,
                             double *cell_out, void *stream);
int oriana_dropout_metric_axes(double *gene_out, double *cell_out, const float *D_hat, const double *U, const double *V,
                               const double *pi_d, const uint32_t *nzmask, int64_t n, int64_t m, int64_t K, void *stream);

/* ---- the variational bound of pCMF (oriana_amd/models/gap.py: elbo; no counterpart in the reference) --------
 * With q(Z) at its optimum for the current q(U) q(V), Gamma(shape, rate) throughout:
 *   ELBO = sum_{x != 0} [x log den - lgamma(x + 1)] - sum_k (sum_i U_hat_ik)(sum_j V_hat_jk) - KL_U - KL_V,
 *   log den_ij = log sum_k exp(E[log U]_ik + E[log V]_jk)   (the float32 expectations the next sweep reads).
 *   oriana_elbo_nnz   : out2 += { sum x log den, sum lgamma(x + 1) } over the stored entries of the sliced layout.
 *                       log den = mu_u[i] + mu_v[j] + log(x / s): s_rs from oriana_row_pass over the shifted factors
 *                       F = exp(l - mu) of oriana_factor_prep, mu_u [n], mu_v [m] its row maxima (packed order, NaN for a
 *                       rejected row).  An entry whose s is the NaN sentinel or 0 is a float64 log-sum-exp over the K
 *                       factors from logU (n, K), logV (m, K) (caller's order, float32) inside the kernel -- NOT the
 *                       exp-of-the-sum arithmetic of oriana_fixup: the bound stays finite where den underflows.
 *   oriana_dense_elbo : the same two sums over the non-zero counts of the dense genes of a hybrid layout, every
 *                       log den a float64 log-sum-exp (K <= 256).
 *   oriana_gamma_kl   : out[0] += sum_{i,k} KL(Gamma(s1_ik, s2_ik) || Gamma(p1_k, p2_k)) over an (r, K) side, float64:
 *                       (s1 - p1) psi(s1) - lgamma(s1) + lgamma(p1) + p1 (log s2 - log p2) + s1 (p2 - s2) / s2.
 *                       s2_is_row != 0: s2 is a K-vector broadcast over the rows (pCMF's cell-side rate,
 *                       oriana_gamma_update_finalize_lazy); else dense (r, K).  Shapes at the clamp (1e-15) give finite values.
 */
int oriana_elbo_nnz(const oriana_counts *cm, const float *s_rs, const float *mu_u, const float *mu_v,
                    const float *logU, const float *logV, int64_t K, double *out2, void *stream);
int oriana_dense_elbo(const oriana_dense *d, const float *logU, const float *logV, const int32_t *row_perm,
                      const int32_t *col_perm, double *out2, int64_t K, void *stream);
int oriana_gamma_kl(double *out, const double *s1, const double *s2, int s2_is_row, const double *p1, const double *p2,
                    int64_t r, int64_t K, void *stream);

/* ---- the bound per cell (oriana_amd/models/gap.py: score_samples; engine.cell_bounds) ------------------------
 * A cell's share of the bound above: sum_j [x_ij log den_ij - lgamma(x_ij + 1)] - sum_k U_hat_ik sum_j V_hat_jk - KL_i.
 *   oriana_cell_bound_nnz : out2 (n, 2) float64, caller's row order, = { sum_j x_ij log den_ij, sum_j lgamma(x_ij + 1) } per
 *                           cell over the stored entries of the sliced layout; arguments and per-entry arithmetic of
 *                           oriana_elbo_nnz (float64 log-sum-exp fall-back included).  One work-group per row block walks
 *                           its gene tiles in order: a cell's entries are added in a fixed order and every cell's pair is
 *                           WRITTEN (0, 0 for a cell without entries) -- no atomics, out2 need not be zeroed, reruns are
 *                           bit-identical.
 *   oriana_gamma_kl_rows  : out[i] = sum_k KL(Gamma(s1_ik, s2_ik) || Gamma(p1_k, p2_k)), the pieces and arguments of
 *                           oriana_gamma_kl, one value WRITTEN per row, summed in a fixed order.
 * Both check their arguments before any HIP call: ORIANA_EINVAL on a missing pointer or K <= 0, 0 on an empty input. */
int oriana_cell_bound_nnz(const oriana_counts *cm, const float *s_rs, const float *mu_u, const float *mu_v,
                          const float *logU, const float *logV, int64_t K, double *out2, void *stream);
int oriana_gamma_kl_rows(double *out, const double *s1, const double *s2, int s2_is_row, const double *p1, const double *p2,
                         int64_t r, int64_t K, void *stream);

/* ---- stateless drop-ins with the reference's exact signatures (outputs first) ------------------
 * One entry per loop nest, arguments in the reference's order, all matrices dense C-contiguous f32
 * on the device: X, D_hat (n, m); log_U_hat and the row-side output (n, K); log_V_hat, S_tilde, S_hat
 * and the gene-side outputs (m, K).  The callee zero-fills the outputs (gap.py:69-70).  `ws` is
 * caller-provided scratch of at least oriana_zq_workspace_bytes() bytes (256-byte aligned); these
 * entry points pack X on every call, as the reference re-casts X on every call (gap.py:94), and
 * synchronise the stream once (the slot totals size the record arrays).  The model classes use the
 * resident oriana_counts instead.
 *   oriana_zq_gap_f32          GaP.compute_Z_q_expectations          oriana/models/gap.py:67-80
 *   oriana_zq_zigap_f32        ZIGaP.compute_Z_q_expectations        oriana/models/zigap.py:79-95
 *                              reference_quirks != 0 keeps the D_hat[i, k] index of zigap.py:94
 *                              (needs K <= m); 0 weights the per-gene sums with D_hat[i, j]
 *   oriana_zq_sparse_gap_f32   SparseGaP.compute_Z_q_expectations    oriana/models/sparse_gap.py:81-97
 *   oriana_zq_sparse_zigap_f32 SparseZIGaP.compute_Z_q_expectations  oriana/models/sparse_zigap.py:100-116
 */
int64_t oriana_zq_workspace_bytes(int64_t n, int64_t m, int64_t K, int64_t nnz_bound);
int oriana_zq_gap_f32(float *Z_hat_i, float *Z_hat_j,
                      const float *log_U_hat, const float *log_V_hat, const float *X,
                      int64_t n, int64_t m, int64_t K, void *ws, int64_t ws_bytes, void *stream);
int oriana_zq_zigap_f32(float *DZ_hat_i, float *DZ_hat_j, float *DZ_exp_logsum_hat,
                        const float *log_U_hat, const float *log_V_hat, const float *D_hat, const float *X,
                        int64_t n, int64_t m, int64_t K, int reference_quirks,
                        void *ws, int64_t ws_bytes, void *stream);
int oriana_zq_sparse_gap_f32(float *SZ_hat_i, float *Z_hat_j, float *Z_exp_logsum_hat,
                             const float *log_U_hat, const float *log_V_hat,
                             const float *S_tilde, const float *S_hat, const float *X,
                             int64_t n, int64_t m, int64_t K, void *ws, int64_t ws_bytes, void *stream);
int oriana_zq_sparse_zigap_f32(float *DSZ_hat, float *DZ_hat, float *DZ_exp_logsum_hat,
                               const float *log_U_hat, const float *log_V_hat,
                               const float *S_tilde, const float *S_hat, const float *D_hat, const float *X,
                               int64_t n, int64_t m, int64_t K, void *ws, int64_t ws_bytes, void *stream);

/* ---- Gamma / Bernoulli updates and the M-step --------------------------------------------------
 * oriana_gamma_update: one side (U or V) of update_variational_parameters
 *   (gap.py:96-110, zigap.py:114-128, sparse_gap.py:117-132, sparse_zigap.py:137-152) fused with
 *   Gamma.mean / Gamma.meanlog (nodes/probabilistic/gamma.py:37-61):
 *     a1 = max(1e-15, nan_to_num(prior1[k] + zmul[i,k] * Z[i,k]))
 *     a2 = max(1e-15, nan_to_num(prior2[k] + rmul[i,k] * (rate_mat ? rate_mat[i,k] : rate_vec[k])))
 *     E = a1 / a2 (f64);  Elog = f32(digamma(f32(a1))) - logf(f32(a2))
 *   and the column sums sum_i E[i,k], sum_i Elog[i,k] (f64, ADDED into colsum_E / colsum_Elog:
 *   zero them first; they feed the M-step means, gap.py:120-122, and the other side's rate).
 *   Z may be NULL (initialisation: a1/a2 are taken as they are, only expectations are produced).
 */
int oriana_gamma_update(double *a1, double *a2, double *E, float *Elog,
                        double *colsum_E, double *colsum_Elog,
                        const double *prior1, const double *prior2,
                        const float *Z, const float *zmul,
                        const double *rate_vec, const double *rate_mat, const float *rmul,
                        int64_t r, int64_t K, void *stream);

/* The same update with the last step of the responsibility pass folded in (pCMF, gap.py:79-80 + 96-110): rows are walked
 * in PACKED order p, Z[o,k] += F[p,k] * sum_s R[s][p,k] with o = row_index ? row_index[p] : p (what oriana_finalize_slabs
 * does; R = (nslab, r, Kp); Z stays a complete output) and a1 = prior1 + Z, a2 = prior2 + rate_vec at once -- one launch
 * and one pass over Z less per side. */
int oriana_gamma_update_finalize(double *a1, double *a2, double *E, float *Elog,
                                 double *colsum_E, double *colsum_Elog,
                                 const double *prior1, const double *prior2,
                                 float *Z, const float *F, const float *R, int64_t nslab, const int32_t *row_index,
                                 const double *rate_vec, int64_t r, int64_t K, void *stream);
/* [r5] Both updates with the cell-side half of the NEXT sweep's factor preparation folded in (FU_next != NULL; see
 * oriana_factor_prep_pair_fused): FU_next (r, Kp) float32, zero-filled once by the caller (padding columns are never written),
 * gets exp(Elog - row maximum) in the packed row order of F / R (finalize form) or in the caller's row order (plain form: only
 * for counts without a row permutation); mu_out [r]; upart [4 * oriana_gamma_update_prep_blocks(r, K)].  The blocks query
 * returns 0 when no vector kernel serves this K (odd K above 64, K above 256): the caller then keeps the separate preparation.
 * FU_next = NULL: exactly oriana_gamma_update / oriana_gamma_update_finalize (the latter with slab_row0: only the rows from
 * slab_row0 on have more than slab 0, as oriana_finalize_slabs_from). */
int64_t oriana_gamma_update_prep_blocks(int64_t r, int64_t K);
int oriana_gamma_update_prep(double *a1, double *a2, double *E, float *Elog,
                             double *colsum_E, double *colsum_Elog,
                             const double *prior1, const double *prior2,
                             const float *Z, const float *zmul,
                             const double *rate_vec, const double *rate_mat, const float *rmul,
                             int64_t r, int64_t K, float *FU_next, float *mu_out, float *upart, void *stream);
int oriana_gamma_update_finalize_prep(double *a1, double *a2, double *E, float *Elog,
                                 double *colsum_E, double *colsum_Elog,
                                 const double *prior1, const double *prior2,
                                 float *Z, const float *F, const float *R, int64_t nslab, int64_t slab_row0, const int32_t *row_index,
                                 const double *rate_vec, int64_t r, int64_t K, float *FU_next, float *mu_out, float *upart,
                                 void *stream);
/* [r6] The finalize form for pCMF's cell side WITHOUT the two (r, K) float64 matrices no kernel of a sweep reads:
 *   gap.py:98   a2[i, :] = max(1e-15, alpha2 + sum_j V_hat)   -- the same K numbers in every row: written ONCE, to a2_row[K];
 *   gap.py:101  U_hat = a1 / a2 (Gamma._mean, gamma.py:37-46)  -- not stored; its column sums go to colsum_E as before.
 * The launch moves 3.2 instead of 4.8 GB at configs[3].  The caller materialises a2 / U_hat on access (oriana_amd/models/gap.py:
 * a float64 broadcast and a float64 division, bit-identical to what the kernel would have stored).  Everything else as
 * oriana_gamma_update_finalize_prep.  ORIANA_EKRANGE when no vector kernel serves this K / these pointers (odd K above 64,
 * K above 256, a pointer that is not 16-byte aligned): take oriana_gamma_update_finalize_prep. */
int oriana_gamma_update_finalize_lazy(double *a1, double *a2_row, float *Elog,
                                 double *colsum_E, double *colsum_Elog,
                                 const double *prior1, const double *prior2,
                                 float *Z, const float *F, const float *R, int64_t nslab, int64_t slab_row0, const int32_t *row_index,
                                 const double *rate_vec, int64_t r, int64_t K, float *FU_next, float *mu_out, float *upart,
                                 void *stream);

/* The GLOBAL step of a streaming fit (oriana_amd/models/gap.py: partial_fit; stochastic variational inference, no counterpart
 * in the reference): the gene side of oriana_gamma_update with the batch's estimate BLENDED into the shapes and rates the model
 * holds, one launch.  Z (m, K) float32 = sum_{i in batch} x_ij r_ijk at the batch's converged cell side, sum_u [K] float64 =
 * sum_{i in batch} E[U_ik], scale = n_total / n_batch, rho in [0, 1] the step size:
 *   b1 = max(1e-15, nan_to_num((1 - rho) * b1 + rho * (beta1[k] + scale * Z[j,k])))
 *   b2 = max(1e-15, nan_to_num((1 - rho) * b2 + rho * (beta2[k] + scale * sum_u[k])))          (b1, b2 (m, K) float64, in place)
 *   E = b1 / b2 (f64);  Elog = f32(digamma(f32(b1))) - logf(f32(b2));  colsum_E / colsum_Elog [K] += their column sums (f64;
 *   zero them first, either may be NULL) -- the arithmetic of oriana_gamma_update on a stored pair, element for element.
 * The convex form makes rho = 0 leave b1, b2 bit for bit and rho = 1 give the batch estimate bit for bit (at scale = 1:
 * every output of oriana_gamma_update with rate_vec = sum_u); (1 - rho) is formed once, in float64, on the host.  Each value
 * takes three float64 roundings, by explicit FMAs -- fma(scale, stat, prior), rho * that, fma(1 - rho, b, it) --, so every
 * kernel configuration below gives the same bits.
 * F == NULL: Z is complete and only read.  F != NULL: the finalize form, as oriana_gamma_update_finalize -- rows are walked in
 * the PACKED gene order p of the batch's tiles, Z[o,k] += F[p,k] * sum_s R[s][p,k] with o = row_index ? row_index[p] : p
 * (R = (nslab, m, Kp), F (m, Kp); Z is completed in place) and blended at once: the batch's column pass runs without its
 * finalize launch.  Every K with oriana_kpad(K) != 0 and any pointer alignment is served (odd K above 64 and buffers that are
 * not 16-byte aligned by an element-per-lane kernel); ORIANA_EKRANGE for K above 256, ORIANA_EINVAL for rho outside [0, 1] or
 * a scale that is negative or not finite. */
int oriana_svi_gene_update(double *b1, double *b2, double *E, float *Elog,
                           double *colsum_E, double *colsum_Elog,
                           const double *beta1, const double *beta2,
                           float *Z, const float *F, const float *R, int64_t nslab, const int32_t *row_index,
                           const double *sum_u, double scale, double rho,
                           int64_t m, int64_t K, void *stream);
/* oriana_svi_gene_update with the rate statistic as an (m, K) float64 matrix in the caller's gene order (ZI-pCMF: a gene's rate
 * reads the dropout posterior of its own zeros, oriana_zi_gene_rate):
 *   b2 = max(1e-15, nan_to_num((1 - rho) * b2 + rho * (beta2[k] + scale * rate[j,k])))
 * -- one flag through the same kernels, the same three FMAs per value: a matrix whose every row is sum_u gives the bits of the
 * vector entry.  Everything else as above. */
int oriana_svi_gene_update_mat(double *b1, double *b2, double *E, float *Elog,
                               double *colsum_E, double *colsum_Elog,
                               const double *beta1, const double *beta2,
                               float *Z, const float *F, const float *R, int64_t nslab, const int32_t *row_index,
                               const double *rate, double scale, double rho,
                               int64_t m, int64_t K, void *stream);

/* The step between two row passes of a FOLD-IN (oriana_amd/models/gap.py: transform; no counterpart in the reference): pCMF's
 * cell-side update for cells the model was not fitted on, the gene side frozen -- per cell a fixed-point iteration of
 *   a1 <- max(1e-15, alpha1 + Z_i),  Z_i = Z + F * sum_slabs R  (as oriana_gamma_update_finalize_lazy: packed rows, nslab, slab_row0,
 *   row_index),  E[log U] = f32(psi(f32(a1))) - logf(f32(a2_row))   (a2_row [K] = alpha2 + sum_j V_hat: constant over the iteration),
 *   stored MINUS its row maximum (mu_out = 0): the softmax over the factors does not see the shift, and the float32 exponentials
 *   of the slow path then do not underflow for a cell whose shapes sit near the clamp.
 * Per row: a cell with active[o] != 0 whose update satisfies |a1_new - a1| <= tol * a1 in every factor FREEZES: active[o] = 0,
 * froze_at[o] = it, and neither its a1, its Elog nor its row of FU_next is written by this or any later call.  Every other active
 * cell gets a1 (float64), Elog (float32) and the PREP outputs of oriana_gamma_update_finalize_prep: FU_next (r, Kp), mu_out [r],
 * upart [4 * oriana_foldin_update_blocks(r)] (the statistics cover all rows: a frozen row enters with the mu_out it stored last).
 * *n_active += the cells still active after the call (one atomic per work-group; the caller zeroes it).  No (r, K) float64
 * matrix but a1 is touched, no column sums are formed, Z is not written back.  FU_next may be F itself (in place).
 * R == NULL: the START -- a1 is taken as it is, every active cell gets Elog, FU_next, mu_out from it; Z, F, alpha1, froze_at,
 * n_active are not read.  Every K with oriana_kpad(K) != 0 and any pointer alignment is served (odd K above 64 and unaligned
 * buffers by an element-per-lane instantiation); ORIANA_EKRANGE only where no row pass exists (K above 256). */
int64_t oriana_foldin_update_blocks(int64_t r);
int oriana_foldin_update(double *a1, float *Elog, uint8_t *active, int32_t *froze_at, int32_t *n_active,
                         const double *alpha1, const double *a2_row, const float *Z, const float *F, const float *R,
                         int64_t nslab, int64_t slab_row0, const int32_t *row_index, int64_t r, int64_t K, double tol,
                         int64_t it, float *FU_next, float *mu_out, float *upart, void *stream);

/* The same step for a fold-in into a ZERO-INFLATED model (oriana_amd/models/zigap.py: fold_in), where the rate is a matrix: a
 * cell carries the pair (a1, a2), each (r, K) float64 in the caller's row order, and one call applies
 *   a1' = max(1e-15, nan_to_num(alpha1 + Z_i)),   a2' = max(1e-15, nan_to_num(alpha2 + rate[o]))
 * with rate (r, K) = sum_j d_ij V_hat_jk formed by oriana_zi_foldin_rate from the U_hat of the pair that enters.  A cell FREEZES
 * when |a1' - a1| <= tol * a1 AND |a2' - a2| <= tol * a2 hold in every factor; a frozen cell is never written again.  Every
 * other active cell gets a1, a2, U_hat = a1' / a2' (r, K float64), Elog = f32(psi(f32(a1'))) - logf(f32(a2')) minus its row
 * maximum, and the prep outputs FU_next / mu_out / upart, exactly as oriana_foldin_update.  R == NULL: the START -- the pair is
 * taken as it is; U_hat, Elog, FU_next, mu_out are written from it.  The same K and alignment coverage as oriana_foldin_update
 * (a2, rate and U_hat join the buffers whose 16-byte alignment selects the vector instantiations). */
int oriana_foldin_update_zi(double *a1, double *a2, double *U_hat, float *Elog, uint8_t *active, int32_t *froze_at,
                            int32_t *n_active, const double *alpha1, const double *alpha2, const double *rate,
                            const float *Z, const float *F, const float *R, int64_t nslab, int64_t slab_row0,
                            const int32_t *row_index, int64_t r, int64_t K, double tol, int64_t it, float *FU_next,
                            float *mu_out, float *upart, void *stream);

/* M-step for one Gamma node (gap.py:117-129; utils.py:39-51):
 *   p1 = max(1e-15, nan_to_num(inverse_digamma(log(p2) + f32(colsum_Elog / count))))
 *   p2 = max(1e-15, nan_to_num(p1 / (colsum_E / count)))            (K-vectors, f64, in place) */
int oriana_mstep_gamma(double *p1, double *p2, const double *colsum_E, const double *colsum_Elog,
                       double count, int64_t K, void *stream);

/* Both Gamma nodes in one launch.  keep_v (2K values or NULL): copy of the V side's column sums {sum E, sum Elog} --
 * a sweep that accumulates them in scratch (cleared with the other scratch of the sweep) keeps them here for the next
 * sweep's cell-side rate, sum_j V_hat (gap.py:98). */
int oriana_mstep_gamma_pair(double *p1u, double *p2u, const double *colsum_E_u, const double *colsum_Elog_u, double count_u,
                            double *p1v, double *p2v, const double *colsum_E_v, const double *colsum_Elog_v, double count_v,
                            double *keep_v, int64_t K, void *stream);

/* Column sums of a dense (r, K) f64 matrix, optionally times an f32 (r, K) multiplier, added
 * into out[K] (zero it first) -- `V_hat.sum(axis=0)`, gap.py:98. */
int oriana_colsum_f64(double *out, const double *A, const float *mul, int64_t r, int64_t K, void *stream);

/* ---- zero-inflated / sparse model pieces -------------------------------------------------------
 * D_q update (zigap.py:130-136, sparse_zigap.py:163-169), in three steps:
 *   oriana_dropout_update : p_d = sigmoid(logit(pi_d)[None, :] - Lambda), columns with pi_d <= 0 -> 1e-10,
 *                           pi_d >= 1 -> 1 - 1e-10; D_hat = float32(p_d).  Lambda = U_hat V_hat^T, dense
 *                           (rows, m) f64, may alias p_d.
 *   oriana_dropout_fix_nz_ld : p_d[X != 0] = value (1 - 1e-10; 1.0 at initialisation, zigap.py:77) and D_hat,
 *                           from the tiled layout.
 *   oriana_colsum_wide_f64: out[j] += sum_i A[i, j]  (pi_d = mean(p_d, axis=0), zigap.py:158).
 */
int oriana_dropout_update(double *p_d, float *D_hat, const double *Lambda, const double *pi_d,
                          /* optional: bit mask of X != 0 (oriana_nzmask_f32 layout) -> the override
                           * p_d[X != 0] = 1 - 1e-10 is applied in the same pass */
                          const uint32_t *nzmask,
                          /* optional: colsum[j] += sum_i p_d[i, j] (zero it first) */
                          double *colsum,
                          int64_t rows, int64_t m, void *stream);
/* mask[(i / 32) * m + j] bit (i % 32) = (D[i, j] != 0); ceil(rows / 32) * m words. */
int oriana_nzmask_f32(uint32_t *mask, const float *D, int64_t rows, int64_t m, void *stream);
/* The same update with Lambda = U_hat V_hat^T formed on the matrix cores inside the kernel (f64 MFMA),
 * so that Lambda never goes through HBM: U (n, K), V (m, K) f64 row-major, K <= 256.  p_d and D_hat
 * are optional outputs (NULL: not stored) -- the models keep only D_hat resident and evaluate p_d on
 * access from a snapshot of (U, V, pi_d). */
int oriana_dropout_update_fused(double *p_d, float *D_hat, const double *U, const double *V, const double *pi_d,
                                const uint32_t *nzmask, double *colsum, int64_t n, int64_t m, int64_t K,
                                void *stream);
/* Rate terms of the ZI Gamma updates on the matrix cores, D_hat (n, m) f32 read in place and promoted
 * to f64 as np.dot does:  trans = 0: out[n, K] += D_hat W[m, K]   (zigap.py:116, np.dot(D_hat, V_hat))
 *                         trans = 1: out[m, K] += D_hat^T W[n, K] (zigap.py:124, np.dot(D_hat.T, U_hat))
 * `out` must be initialised (zeros for a plain product).  K <= 256. */
int oriana_dense_times_factor(double *out, const float *D, const double *W, int64_t n, int64_t m, int64_t K,
                              int trans, void *stream);
/* The dense work of one ZI SWEEP on the float32 matrix cores (csrc/dense_f32.hip), K <= 128 (else ORIANA_EKRANGE:
 * use the float64 entries above).  Long sums leave the matrix core every 256 terms and end in float64; measured
 * against the float64 entries: D_hat within 2 float32 ulp, rate terms within 3e-7 relative.
 *
 * oriana_dropout_sweep_fused: D_hat[n, m] = f32(sigmoid(logit(pi_d) - U V^T)) with the overrides of zigap.py:130-136
 * (nzmask optional as above), colsum[j] += sum_i p_d[i, j] (optional, zero it first), and -- V_next / DV_next both
 * given or both NULL -- DV_next[n, K] += D_hat V_next[m, K] from the tile of D_hat still in registers: with V_next the
 * factor the NEXT sweep's cell update multiplies (zigap.py:116: the V_hat just updated; sparse_zigap.py:138:
 * S_hat * Vprime_hat) that sweep has no pass over D_hat left on the cell side.  DV_next must be zeroed first.
 * scratch: oriana_dropout_sweep_scratch_floats(m, K) floats of device scratch (logit(pi_d), float32 copies of V and
 * V_next), 16-byte aligned, contents undefined on entry and exit: every piece of it that a kernel reads has been written by
 * the same call (tests/test_scratch_contract_gpu.py).  arithmetic: how the float32 products are evaluated --
 *   ORIANA_MATRIX_F32     v_mfma_f32_32x32x2_f32 (a chain of single-rounding float32 FMAs);
 *   ORIANA_MATRIX_BF16X3  each float32 operand split into three bf16, six cross products on the bf16 matrix cores,
 *                         float32 accumulation (K <= 100 when the gene count is a multiple of 4, K <= 64 otherwise;
 *                         larger K silently take the float32 instruction; csrc/dense_f32.hip, csrc/dense_zi.hip): the same
 *                         error as the float32 chain on sums of <= 512 terms (which is all the kernel forms before it
 *                         leaves the matrix core), 2.7 x its rate. */
#define ORIANA_MATRIX_F32     0
#define ORIANA_MATRIX_BF16X3  1
int oriana_dropout_sweep_fused(float *D_hat, const double *U, const double *V, const double *pi_d,
                               const uint32_t *nzmask, double *colsum, const double *V_next, double *DV_next,
                               float *scratch, int arithmetic, int64_t n, int64_t m, int64_t K, void *stream);
int64_t oriana_dropout_sweep_scratch_floats(int64_t m, int64_t K);
/* [r6] The same sweep with the non-zero mask ALSO as per-lane flags for the K = 33 .. 100 bf16 x 3 kernel (csrc/dense_zi.hip,
 * dn::k_zi_row): every lane of a wave reads the 16 flags of the 16 values it holds with one 2-byte LDS read per tile and
 * applies the override p_d[X != 0] = 1 - 1e-10 (zigap.py:135) with two instructions per entry (bit-field extract, bit-field
 * insert) where the gene-major words of oriana_nzmask_f32 took three plus eight LDS reads per tile.
 * nztiles: oriana_nzmask_tiles_words(n, m) uint32 words (16-byte aligned), built ONCE per count matrix by oriana_nzmask_tiles
 * from the oriana_nzmask_f32 layout: per (cell tile of 32, gene tile of 32) 64 x 16 bits, bit v of entry l =
 * (X[32 ct + l % 32, 32 gt + 8 (v / 4) + 4 (l / 32) + v % 4] != 0); cell tiles padded to a multiple of 8.
 * nztiles == NULL (= oriana_dropout_sweep_fused): that kernel does not apply; K <= 64 takes the bf16 kernels of
 * csrc/dense_f32.hip, larger K the float32 matrix instruction. */
int oriana_dropout_sweep_fused_tiles(float *D_hat, const double *U, const double *V, const double *pi_d,
                                     const uint32_t *nzmask, const uint32_t *nztiles, double *colsum, const double *V_next,
                                     double *DV_next, float *scratch, int arithmetic, int64_t n, int64_t m, int64_t K,
                                     void *stream);
int64_t oriana_nzmask_tiles_words(int64_t n, int64_t m);
int oriana_nzmask_tiles(uint32_t *tiles, const uint32_t *nzmask, int64_t n, int64_t m, void *stream);
/* The oriana_nzmask_f32 layout straight from packed counts, in the caller's row and gene order (cm->row_perm, cm->col_perm):
 * mask[(i / 32) * ld + j] bit (i % 32) |= (x_ij != 0), ld >= cm->m.  The mask must be ZEROED first (ceil(cm->n / 32) * ld words);
 * no (n, m) float matrix exists at any point.  With oriana_nzmask_tiles: both mask forms of a query. */
int oriana_nzmask_counts(uint32_t *mask, const oriana_counts *cm, int64_t ld, void *stream);
/* The cell-side rate of a fold-in into a ZI model: DV[i, :] += sum_j d_ij V[j, :]  (DV (n, K) float64, zeroed by the caller) with
 *   d_ij = 1 where x_ij != 0;  1e-10 / 1 where pi_d_j <= 0 / >= 1;  f32(sigmoid(logit(pi_d_j) - U_i . V_j)) elsewhere
 * -- the D_hat of oriana_dropout_sweep_fused_tiles, formed tile by tile in registers and NEVER stored: no D_hat, no column sums.
 * K <= 128 (else ORIANA_EKRANGE); the kernel family that serves a K is the one that entry runs for it (the same rule and the
 * same preconditions, minus the D_hat pointer), compiled without the store and the column-sum path.  nzmask (required) and
 * nztiles (optional, as above) describe the cells at hand; scratch: oriana_dropout_sweep_scratch_floats(m, K) floats, 16-byte
 * aligned, contents undefined on entry and exit.  active [n] bytes or NULL (= every cell): a work-group whose cells are all
 * inactive returns at once; rows of U and DV that belong to inactive cells are neither read nor written. */
int oriana_zi_foldin_rate(double *DV, const double *U, const double *V, const double *pi_d, const uint32_t *nzmask,
                          const uint32_t *nztiles, const uint8_t *active, float *scratch, int arithmetic, int64_t n, int64_t m,
                          int64_t K, void *stream);
/* Which kernel serves a dense ZI product of width K: the answer of the dispatch chain the entries themselves run (csrc/
 * dense_tiles.h, zi_candidate), without a launch -- no device is needed.  op 0: the D update (oriana_dropout_sweep_fused_tiles)
 * and its rate-only twin (oriana_zi_foldin_rate); op 1: D_hat^T W (oriana_dense_t_times_factor_f32).  tiles_ok: the run-time
 * preconditions of the csrc/dense_zi.hip family hold (a gene count that is a multiple of 4, 16-byte aligned pointers, and for
 * op 0 the per-lane flags of oriana_nzmask_tiles; for op 1 a scratch).  Returns (family << 16) | (a << 8) | b >= 0 with
 *   family 1  csrc/dense_zi.hip, k_zi_row / k_zi_col<KC = a, TAIL = b>;
 *   family 2  the bf16 x 3 kernels of csrc/dense_f32.hip, k_dropout_sweep_b16<NT = a, KC = b> / k_dt_times_factor_b16<NT = a>;
 *   family 3  the float32 matrix instruction, k_dropout_sweep<NT = a> / k_dt_times_factor_f32<NT = a, GQ = b>;
 * ORIANA_EKRANGE for K > 128, ORIANA_EINVAL for K <= 0, another op or another arithmetic, as the entries. */
int oriana_zi_dispatch(int op, int64_t K, int arithmetic, int tiles_ok);
/* The dropout term of a held-out cell's bound under a ZI model with the gene side frozen (ZIGaP.fold_in_score_samples,
 * engine.zi_cell_bounds), the dropout posterior collapsed at its optimum and never stored:
 *   out[i] = sum_{j < m_real, x_ij != 0} z_ij + sum_{j < m_real, x_ij == 0} softplus(z_ij),   z_ij = logit(pi~_j) - U_i . V_j,
 *   pi~_j = min(max(pi_d_j, 1e-10), 1 - 1e-10)   (the two override values of zigap.py:133-134: every logit is finite).
 * The caller adds the cell-independent sum_j log(1 - pi~_j).  U (n, K), V (m, K), pi_d [m] float64; nzmask in the
 * oriana_nzmask_f32 layout with ld = m (oriana_nzmask_counts).  m counts the inert padding genes [m_real, m) (V row 0, pi_d 0)
 * too: they are left out of the sums.  K <= 128 (else ORIANA_EKRANGE): the float32 matrix instruction's kernel of the D update
 * (csrc/dense_f32.hip, k_dropout_sweep) with this epilogue in place of the sigmoid, softplus as max(z, 0) + log1p(exp(-|z|)).
 * Per tile of 32 genes a cell's values are added in float32, the tiles in float64; the gene axis is cut into S ranges (a
 * function of n, m and the device's compute units), every range WRITES its partial to scratch and a second launch adds the S
 * partials in order: no atomics, out [n] need not be zeroed, every out[i] is written, reruns are bit-identical.
 * scratch: oriana_zi_cell_bound_scratch_doubles(n, m, K) = S n + 32 ceil(m / 64) doubles (the partials, then the float32 logits).
 * ORIANA_EINVAL on a missing pointer, K <= 0 or m_real outside [0, m]; 0 for n == 0 before any HIP call. */
int64_t oriana_zi_cell_bound_scratch_doubles(int64_t n, int64_t m, int64_t K);
int oriana_zi_cell_bound(double *out, const double *U, const double *V, const double *pi_d, const uint32_t *nzmask,
                         double *scratch, int64_t n, int64_t m, int64_t m_real, int64_t K, void *stream);
/* The gene-side rate statistic of a batch folded into a ZI model (ZIGaP.fold_in_fit, heldout.zi_gene_rate), the
 * dropout posterior formed tile by tile and never stored:
 *   G[j, k] = sum_{i < n} d_ij U[i, k]   (m, K) float64,      dsum[j] = sum_{i < n} d_ij   [m] float64,
 *   d_ij = 1 where x_ij != 0; 1e-10 / 1 in the columns with pi_d <= 0 / >= 1; else f32(sigmoid(logit(pi_d_j) - U_i . V_j))
 * -- the d of oriana_zi_foldin_rate (k_logit_f32's +-inf flags, not the clamped logits of the bound).  U (n, K), V (m, K),
 * pi_d [m] float64; nzmask in the oriana_nzmask_f32 layout with ld = m (oriana_nzmask_counts); m a multiple of 4 with inert
 * padding genes (V row 0, pi_d 0), whose rows of G and dsum the caller drops.  K <= 128 (else ORIANA_EKRANGE): the float32 matrix
 * instruction (csrc/dense_f32.hip, k_gene_rate -- the transposed twin of k_dropout_sweep).  Sums leave the matrix core every 256
 * cells and float32 every 4096; a gene's d are added 16 at a time in float32, then in float64, and in a column with pi_d <= 0
 * dsum is nnz_j + 1e-10 (n - nnz_j) in float64.  The cell axis is cut into S = oriana_zi_gene_rate_ranges(n, m, K) <= 32 ranges
 * that start on multiples of 32 (S ceil(m / 128) stays within two work-groups per compute unit, so the partials never exceed
 * 256 rows of K doubles per compute unit whatever n and m);
 * every range WRITES its partial to scratch and a second launch adds the S partials in order: no atomics, G and dsum need not
 * be zeroed, every element is written, reruns are bit-identical.
 * scratch: oriana_zi_gene_rate_scratch_doubles(n, m, K) = S (m K + m) + 32 ceil(m / 64) doubles.
 * ORIANA_EINVAL on a missing pointer or K <= 0; n == 0 writes zeros; 0 for m == 0 before any HIP call. */
int64_t oriana_zi_gene_rate_ranges(int64_t n, int64_t m, int64_t K);
int64_t oriana_zi_gene_rate_scratch_doubles(int64_t n, int64_t m, int64_t K);
int oriana_zi_gene_rate(double *G, double *dsum, const double *U, const double *V, const double *pi_d, const uint32_t *nzmask,
                        double *scratch, int64_t n, int64_t m, int64_t K, void *stream);
/* out[m, K] += D_hat^T W[n, K] (zigap.py:124), D_hat streamed once; `out` must be initialised.  arithmetic as above;
 * scratch: oriana_dense_t_scratch_floats(n, K) floats (16-byte aligned; the bf16 operand images of W; contents undefined on
 * entry and exit), may be NULL with ORIANA_MATRIX_F32. */
int oriana_dense_t_times_factor_f32(double *out, const float *D, const double *W, float *scratch, int arithmetic,
                                    int64_t n, int64_t m, int64_t K, void *stream);
int64_t oriana_dense_t_scratch_floats(int64_t n, int64_t K);
/* ld: the leading dimension of p_d / D_hat (the sliced part of a hybrid layout: cm->m counts its own genes only); either output
 * may be NULL */
int oriana_dropout_fix_nz_ld(const oriana_counts *cm, double *p_d, float *D_hat, double value, int64_t ld, void *stream);
int oriana_colsum_wide_f64(double *out, const double *A, int64_t rows, int64_t m, void *stream);
/* the same for a float32 matrix (D_hat, while p_d == D_hat exactly: zigap.py:77) */
int oriana_colsum_wide_f32(double *out, const float *A, int64_t rows, int64_t m, void *stream);
/* dq[i, k] = D[i, k], k < K: the columns the reference's zigap.py:94 reads (D_hat[i, k]). */
int oriana_take_cols_f32(float *out, const float *D, int64_t rows, int64_t m, int64_t K, void *stream);

/* S_q update (sparse_gap.py:134-141, sparse_zigap.py:154-161):
 *   p_s = nan_to_num(sigmoid(logit(pi_s)[:, None] - (-Zlog + nan_to_num(c * Vprime_hat)))),
 *   c = c_vec[k] (sum_i U_hat) or c_mat[j, k] (D_hat^T U_hat); rows with pi_s <= 0 / >= 1 overridden;
 *   S_hat = float32(p_s).  oriana_threshold_f32: S_tilde = (p_s > tau) (sparse_gap.py:113).
 *   oriana_rowmean_f64: pi_s = mean(p_s, axis=1) (sparse_gap.py:165). */
int oriana_sparsity_update(double *p_s, float *S_hat, const double *pi_s, const float *Zlog,
                           const double *c_vec, const double *c_mat, const double *Vprime_hat,
                           int64_t m, int64_t K, void *stream);
int oriana_threshold_f32(float *out, const double *p, double tau, int64_t len, void *stream);
int oriana_rowmean_f64(double *out, const double *A, int64_t r, int64_t K, void *stream);

/* out = A * B element-wise, f64 x f32 -> f64 (V_hat = S_hat * Vprime_hat, sparse_gap.py:118). */
int oriana_mul_f64_f32(double *out, const double *A, const float *B, int64_t len, void *stream);

/* Fout[i, :] = Fin[i, :] * mul[row_index ? row_index[i] : i, :]  (padded factor times a dense (., K) f32
 * matrix: S_hat-, D_hat[:, :K]- or E[log U]-weighted factors for the extra sums of the ZI / sparse loop
 * nests).  zero_guard: entries with Fin == 0 stay 0 whatever mul holds. */
int oriana_scale_factor(float *Fout, const float *Fin, const float *mul, const int32_t *row_index,
                        int64_t r, int64_t K, int zero_guard, void *stream);
/* The log sums sum_i r_ijk (lu_ik + lv_jk) (zigap.py:95, sparse_gap.py:97) as two column sums around a per-factor
 * centre a_k = mean of E[log U]_ik over the contributing cells (without it the two sums are each |lu| times larger than
 * their total once the sweeps have drifted, and the sparsity posterior amplifies the lost float32 digits):
 *   oriana_log_center            acc[0..K) = sum w logF, acc[K..2K) = sum w over the entries that carry weight (F > 1e-20,
 *                                finite log); w = W[., k] (dense (r, K) f32 in the caller's row order: the cell's Z_hat_i) or 1;
 *                                acc is zeroed here
 *   oriana_scale_factor_centered Fout = Fin * (mul - a_k), 0 where Fin == 0             (acc NULL: a = 0)
 *   oriana_finalize_zlog         Zlog[o, k] += FV[j, k] * (C2[j, k] + (logV[o, k] + a_k) * C[j, k]), o = row_index ? row_index[j] : j,
 *                                combined in float64 */
int oriana_log_center(double *acc, const float *F, const float *logF, const float *W, const int32_t *row_index,
                      int64_t r, int64_t K, void *stream);
int oriana_scale_factor_centered(float *Fout, const float *Fin, const float *mul, const double *acc,
                                 const int32_t *row_index, int64_t r, int64_t K, void *stream);
int oriana_finalize_zlog(float *Zlog, const float *FV, const float *C2, const float *C, const float *logV,
                         const double *acc, const int32_t *row_index, int64_t r, int64_t K, void *stream);

/* Element-wise special functions on f64 vectors (oriana/utils.py:9-15, 31-51) -- used by tests
 * and by the host mirror of oriana.utils. */
int oriana_digamma_f64(double *y, const double *x, int64_t len, void *stream);
int oriana_trigamma_f64(double *y, const double *x, int64_t len, void *stream);
int oriana_inverse_digamma_f64(double *y, const double *x, int64_t len, void *stream);
int oriana_sigmoid_f64(double *y, const double *x, int64_t len, void *stream);
int oriana_logit_f64(double *y, const double *x, int64_t len, void *stream);

/* ---- [r5] planning of the resident layout as plain C (host arrays in and out, no device) -------------------------------
 * What the kernels of a sweep depend on beyond the packed records.  engine.py (the Python host) and the resident handle below
 * both call these; tests/test_plan.py checks them on the CPU against a NumPy restatement.
 *
 * oriana_plan_gene_order: the internal gene order.  Genes in decreasing order of their non-zero count (col_nnz, summed over
 * all row shards; ties in the caller's order).  dense_density > 0 (hybrid layout): the genes expressed in at least that share
 * of the n_total cells whose counts all fit a uint16 block (bad[j] == 0: no negative, >= 65535 or non-integer entry; bad may be
 * NULL) come first, cut to a multiple of 32 (*gd), unless they hold less than min_share of the non-zeros (then *gd = 0). */
int oriana_plan_gene_order(const int64_t *col_nnz, const int64_t *bad, int64_t m, int64_t n_total,
                           double dense_density, double min_share, int32_t *order /* out [m] */, int64_t *gd /* out */);
/* oriana_plan_col_work: the work list of oriana_col_pass -- items (column block, first row block, end row block) of about
 * equal cost, ordered by row band (concurrent items stage the same factor rows).  tile_iters [nrb * ncb]: longest column-side
 * slice of each tile in iterations of 64 slots; width = oriana_col_block_tiles(K); cost of a row block of a column block =
 * 1.45 * (longest slice over its tiles; sum_price != 0: their sum) + 3.2 (staging 256 factor rows; microseconds on MI355X).
 * target_items = 0: 25-50 tiles per item, 9 to 36 items per CU; rounds != 0: re-cut so that the count lands just below a
 * multiple of `cus` (one 1024-thread group per CU: a partly filled last round costs a whole one).  items: out [cap][3],
 * cap >= oriana_plan_col_work_capacity(nrb, ncb, width). */
int64_t oriana_plan_col_work_capacity(int64_t nrb, int64_t ncb, int64_t width);
int oriana_plan_col_work(const int32_t *tile_iters, int64_t nrb, int64_t ncb, int64_t width, int64_t cus,
                         int64_t target_items, int rounds, int sum_price, int32_t *items, int64_t cap, int64_t *n_items);
/* oriana_plan_inputs: what the two planners read of a packed layout, formed in one place for every host.  DEVICE (in):
 * tile_rslots [nrb * ncb] as oriana_pack_count left it, cslice [nrb * ncb][17].  HOST (out, either may be NULL, its device
 * input is then not read): gene_tile_cost [ncb], the tile_cost of oriana_row_pass_plan = mean over the row blocks of
 * tile_rslots / 1024 (iterations of a 16-row slice) + 2.0 (staging the tile's 256 factor rows, in iterations); tile_iters
 * [nrb * ncb], the input of oriana_plan_col_work.  SYNCHRONISES the stream. */
int oriana_plan_inputs(const int32_t *tile_rslots, const uint32_t *cslice, int64_t nrb, int64_t ncb,
                       double *gene_tile_cost, int32_t *tile_iters, void *stream);
/* Splits of the dense-gene kernels of a hybrid layout: gene ranges of oriana_dense_row_pass_tail (at most two work-groups per CU)
 * and cell ranges of oriana_dense_col_pass (four per CU, a multiple of 8 cell tiles). */
int oriana_plan_dense_splits(int64_t n, int64_t gd, int64_t cus, int64_t *gene_splits, int64_t *cell_splits);

/* ---- [r5] resident handle: the count matrix packed ONCE for a host that is not Python --------------------------------------
 * The reference calls its loop nest once per step() with the same X (oriana/models/gap.py:89-94, zigap.py:105-112,
 * sparse_gap.py:107-115, sparse_zigap.py:126-135) and re-casts X every time; the stateless entries above repack X per call.
 * A handle owns (hipMalloc) the packed layout -- gene order, sliced records, the dense uint16 block of a hybrid layout
 * (dense_density > 0 and oriana_dense_supported(K); <= 0: sliced only), the column work list, the row split, the scratch of a
 * call -- built by the planning functions above for oriana_device_cus() compute units.  X: dense (n, ldx) float32 on the
 * DEVICE, or CSR on the HOST (indptr [n + 1], indices, data; expanded on the device in row chunks of at most 512 MB, so
 * neither side ever holds the dense matrix).  The CSR arrays need not be canonical: the column indices of a row may come in
 * any order, an entry whose value is 0 is no entry, and entries of one row that name the same column ADD UP (SciPy's
 * meaning of duplicates, float32 sums; never last-writer-wins); an index outside [0, m) or a decreasing indptr is
 * ORIANA_EINVAL before anything is launched.  Only columns [0, m) of a dense X with ldx > m are read.
 * The create calls synchronise the stream; the zq
 * calls are asynchronous on it, take DEVICE matrices in the reference's argument order (outputs first, zero-filled by the
 * callee, 2-D C-contiguous float32) and must not run concurrently on one handle. */
typedef struct oriana_resident oriana_resident;
int oriana_counts_create_dense_f32(oriana_resident **out, const float *X, int64_t n, int64_t m, int64_t ldx, int64_t K,
                                   double dense_density, void *stream);
int oriana_counts_create_csr(oriana_resident **out, const int64_t *indptr, const int32_t *indices, const float *data,
                             int64_t n, int64_t m, int64_t K, double dense_density, void *stream);
int oriana_counts_destroy(oriana_resident *h);
/* info[0..12] = {n, m, K, Kp, non-zeros, dense genes, row-side slots, column-side slots, resident bytes, column work items,
 * row-split parts, first split row block, compute units planned for} */
int oriana_counts_info(const oriana_resident *h, int64_t *info, int64_t len);
/* GaP.compute_Z_q_expectations (gap.py:67-80) on the resident layout, sliced or hybrid. */
int oriana_zq_gap_resident(oriana_resident *h, float *Z_hat_i, float *Z_hat_j, const float *log_U_hat, const float *log_V_hat,
                           void *stream);
/* The three twins (zigap.py:79-95, sparse_gap.py:81-97, sparse_zigap.py:100-116) on the resident layout.
 *
 * [r6] oriana_counts_declare_unit_dropout(h, 1): the caller declares that every D_hat it will pass is exactly 1 wherever the
 * count is non-zero -- which holds for every D_hat the reference's own models produce (zigap.py:135 / sparse_zigap.py:168 set
 * p_d[X != 0] = 1 - 1e-10, Bernoulli.mean casts to float32: bernoulli.py:45; the initial p_d = (X > 0): zigap.py:77).  The
 * nests then run exactly as oriana_amd's model classes run them: sliced OR hybrid handle, no gather of D_hat (it is read for
 * the D_hat[i, k] weights of zigap.py:94 only), and for Kp <= 64 the fused kernels -- the S_hat-weighted row sums out of the
 * two-image row pass, both per-gene sums out of one dual column pass (Kp > 64: den-only row pass + second row product + two
 * column passes).  oriana_zq_sparse_gap_resident has no D_hat and always runs this way.
 * Without the declaration (the default) D_hat may hold anything: it is gathered at the stored entries on every call and the
 * weighted four-kernel form runs, on a SLICED handle only (ORIANA_EUNIT for a hybrid one: the dense-gene kernels carry no
 * per-entry weights).
 * The third output (the log sums) may be NULL: the reference's ZIGaP never reads it (zigap.py:105-112) and the model classes
 * skip it; the sparse models need it (sparse_gap.py:135). */
int oriana_counts_declare_unit_dropout(oriana_resident *h, int on);
int oriana_zq_zigap_resident(oriana_resident *h, float *DZ_hat_i, float *DZ_hat_j, float *DZ_exp_logsum_hat,
                             const float *log_U_hat, const float *log_V_hat, const float *D_hat, int reference_quirks, void *stream);
int oriana_zq_sparse_gap_resident(oriana_resident *h, float *SZ_hat_i, float *Z_hat_j, float *Z_exp_logsum_hat,
                                  const float *log_U_hat, const float *log_V_hat, const float *S_tilde, const float *S_hat, void *stream);
int oriana_zq_sparse_zigap_resident(oriana_resident *h, float *DSZ_hat, float *DZ_hat, float *DZ_exp_logsum_hat,
                                    const float *log_U_hat, const float *log_V_hat, const float *S_tilde, const float *S_hat,
                                    const float *D_hat, void *stream);

/* ---- k-means on the cell factors (csrc/kmeans.hip) ------------------------------------------------------------
 * The reference's pipeline ends in sklearn.cluster.KMeans(n_clusters, n_init=100) on np.log(U) (experiments/clustering.py).
 * One Lloyd half-step of R independent restarts over the same rows Y (n, d) float32, row stride ldy >= d:
 *   d2(i, c) = sum_k (y_ik - c_rck)^2 in float32 (the direct difference form, k ascending), label = the arg-min over c (the
 *   smallest index wins an exact tie); sums[r, c, :] = the sum of the rows labelled c, counts[r, c] their exact number,
 *   inertia[r] = sum_i d2(i, label).  labels (n) or NULL receives the labels of restart label_restart only, mind (R, n) or NULL
 *   the minimum distances.  A row tile is read once per group of oriana_kmeans_group(d, C) restarts; no (n, C) array exists.
 * Deterministic: no float atomics; two calls with the same inputs and the same `blocks` (work-groups along the rows; 0: sized
 * from the device) agree bit for bit, and a restart's outputs do not depend on the other restarts of the call.  The sums add
 * at most oriana_kmeans_partial_rows() rows in float32 before the partial sum is promoted to float64.
 * scratch: oriana_kmeans_scratch_bytes(n, d, C, R, blocks) bytes, 16-byte aligned, contents undefined on entry and exit.
 * All arguments are validated before any HIP call: n < 0, d < 1, C < 1, R < 1, ldy < d, blocks < 0 -> ORIANA_EINVAL;
 * C > oriana_kmeans_max_centers(d) -> ORIANA_EKRANGE; a NULL required pointer -> ORIANA_EINVAL.  n = 0: zeroed outputs. */
int oriana_kmeans_step(const float *Y, int64_t n, int64_t d, int64_t ldy, const float *centers, int64_t C, int64_t R,
                       double *sums, int64_t *counts, double *inertia, int32_t *labels, int64_t label_restart, float *mind,
                       void *scratch, int64_t blocks, void *stream);
/* The largest C served at feature width d: 8192 / pad4(d) for d <= 256, 0 for any other d. */
int64_t oriana_kmeans_max_centers(int64_t d);
/* Restarts that share one read of a row tile (the waves of a work-group): 4, or 2 where the partial sums of 4 exceed the LDS;
 * 0 for an unsupported (d, C). */
int64_t oriana_kmeans_group(int64_t d, int64_t C);
/* Bytes of scratch of a step (negative: the argument error the step would return). */
int64_t oriana_kmeans_scratch_bytes(int64_t n, int64_t d, int64_t C, int64_t R, int64_t blocks);
/* The largest number of rows added in float32 before a partial sum is promoted to float64. */
int64_t oriana_kmeans_partial_rows(void);
/* Rows of a tile (the unit `blocks` divides). */
int64_t oriana_kmeans_tile_rows(void);

/* ---- exact k nearest neighbours of the cells (csrc/knn.hip) --------------------------------------------------
 * For every query row of Q (nq, d) float32, row stride ldq >= d, the k nearest of the candidate rows Y (n, d) float32, row
 * stride ldy >= d, by brute force; no distance matrix exists.  Query row i has the global index q0 + i, candidate row j the
 * global index y0 + j; the indices written are global and int32 (y0 + n <= 2^31 - 1).
 *   the pair   f(q, c) = sum_j (q_j - c_j)^2 in float32: one sequential fmaf chain over j ascending that starts from 0, every
 *              difference rounded once -- the chain of oriana_kmeans_step.  Zero padding of the features adds fmaf(0, 0, acc)
 *              and is exact.  f(q, c) == f(c, q) bit for bit (the chain is symmetric under negation of the differences).
 *   the row    the k candidates smallest under the total order (f, global candidate index), both ascending, in that order:
 *              idx (nq, k) int32 and d2 (nq, k) float32, row-major.  With exclude_self the candidate whose global index equals
 *              the query's is skipped -- that one row only: other bit-identical rows stay eligible and come back with f = 0.
 *              Where fewer than k candidates exist the tail is idx = -1, d2 = +inf.  A pair whose f overflows float32 counts
 *              as absent.
 *   merge = 1  the incoming idx / d2 rows are valid rows of the same form made from OTHER candidates; the k best of the union
 *              are left in place.
 * Partition independence: the value of a pair does not depend on how the work is tiled, and a row is the k smallest of a set
 * under a total order, so the outputs are the same bit for bit for any `blocks` (ranges the candidates are cut into inside a
 * call; 0: sized from the device), for any split of the candidates over merging calls in any order, and for any split of the
 * queries over calls with the matching q0.  No atomics: every list has one writer and a fixed order.
 * scratch: oriana_knn_scratch_bytes_for(nq, n, d, k, blocks, Y, ldy) bytes (oriana_knn_scratch_bytes(..) is never less),
 * 16-byte aligned, contents undefined on entry and exit.
 * All arguments are validated before any HIP call: a negative size, index base or `blocks`, d < 1, k < 1, ldq < d, ldy < d,
 * nq or y0 + n beyond 2^31 - 1, n beyond 2^31 - 9 -> ORIANA_EINVAL; d > 256 or k > oriana_knn_max_neighbors(d) -> ORIANA_EKRANGE; a NULL idx, d2
 * or scratch, a NULL Q with nq > 0 or Y with n > 0, a scratch that is not 16-byte aligned -> ORIANA_EINVAL.  nq = 0 is a
 * no-op; n = 0 without merge writes the padding values, with merge nothing. */
int oriana_knn(const float *Q, int64_t nq, int64_t ldq, int64_t q0, const float *Y, int64_t n, int64_t ldy, int64_t y0,
               int64_t d, int64_t k, int exclude_self, int merge, int32_t *idx, float *d2, void *scratch, int64_t blocks,
               void *stream);
/* The largest k served at feature width d, from the LDS of a work-group (the query tile and the lists of four waves):
 * (160 KiB - 260 pad4(d)) / 2048 for d <= 256 (47 at d = 256, 67 at d = 100), 0 for any other d. */
int64_t oriana_knn_max_neighbors(int64_t d);
/* Bytes of scratch that serve a call with any Y (negative: the argument error the call would return): a padded image of the
 * candidates (n pad4(d) floats), the partial lists (8 k bytes per query, wave and range) and a copy of the incoming rows. */
int64_t oriana_knn_scratch_bytes(int64_t nq, int64_t n, int64_t d, int64_t k, int64_t blocks);
/* Bytes of scratch of the call with this Y and ldy: no image where Y itself serves as one (d and ldy multiples of four, Y
 * 16-byte aligned; Y is not dereferenced). */
int64_t oriana_knn_scratch_bytes_for(int64_t nq, int64_t n, int64_t d, int64_t k, int64_t blocks, const float *Y, int64_t ldy);
/* Queries of a tile (one work-group along the queries). */
int64_t oriana_knn_tile_rows(void);
/* Waves of a work-group at (d, k): 8 where the lists of eight waves fit the LDS beside the query tile, else 4 (ORIANA_KNN_WAVES=4
 * in the environment: always 4, for tuning runs; no result depends on it); 0 for an unsupported (d, k). */
int64_t oriana_knn_waves(int64_t d, int64_t k);
/* Ranges the candidates of a call are cut into (at most 64 / oriana_knn_waves(d, k), at least one 8-candidate step per wave);
 * negative: the argument error. */
int64_t oriana_knn_splits(int64_t nq, int64_t n, int64_t d, int64_t k, int64_t blocks);

/* ---- per-cluster sums of distances: the silhouette of a clustering of the cells (csrc/silhouette.hip) --------
 * For every query row of Q (nq, d) float32, row stride ldq >= d, and every cluster c: the sum of the Euclidean distances to the
 * candidate rows of cluster c.  The candidates Y (n, d) float32, row stride ldy >= d, lie GROUPED BY CLUSTER: cluster c owns
 * the rows [offsets[c], offsets[c + 1]).  No distance matrix exists.
 *   the pair   f(q, c) of oriana_knn: sum_j (q_j - c_j)^2 in float32 as one sequential fmaf chain over j ascending that starts
 *              from 0, every difference rounded once, zero padding exact; f of a row with itself or with a bit-identical row
 *              is exactly 0.  The distance is sqrtf(f), the correctly rounded float32 square root (the library is built
 *              without any fast-math flag).
 *   the sum    every distance is converted to float64 and added in float64; no float32 partial sum exists.  No atomics: every
 *              sum has one writer.  Inside a launch the order of addition is fixed by the plan (a function of the sizes, the
 *              offsets and `blocks`), so the same call twice gives the same bits.  Bits are NOT promised across different
 *              partitions of the work (`blocks`, candidates in several accumulating calls, queries in several calls); the
 *              terms are the same bit for bit, so two partitions differ by the float64 summation order only.
 *   the output sums[c * lds + q], device, float64, cluster-major, lds >= nq.  accumulate = 0 overwrites all C x nq entries (a
 *              cluster without rows becomes 0), accumulate = 1 adds the call's sums to what is there.  Entries of a row of
 *              `sums` beyond nq are never touched.
 * offsets: HOST memory, C + 1 ascending entries, offsets[0] = 0, offsets[C] = n; it may be freed when the call returns (the
 * call waits for the stream once, after the copy of its small work table and before its launches).
 * `blocks`: ranges the candidates as a whole are cut into (0: sized from the device, two work-groups per CU); a cluster is cut
 * where it exceeds one range, at most 32,767 ranges.
 * scratch: oriana_cluster_distance_sums_scratch_bytes_for(..) bytes, 16-byte aligned, contents undefined on entry and exit.
 * All arguments are validated before any HIP call: a negative size or `blocks`, d < 1, ldq < d, ldy < d, lds < nq, nq beyond
 * 2^31 - 1, n beyond 2^31 - 9 (the step counter is 32-bit) -> ORIANA_EINVAL; d > 256 or C beyond
 * oriana_cluster_distance_sums_max_clusters() -> ORIANA_EKRANGE; a NULL offsets or scratch, a NULL sums with nq, C > 0, Q with
 * nq > 0 or Y with n > 0, a scratch that is not 16-byte aligned, offsets that do not start at 0, descend or do not end at n ->
 * ORIANA_EINVAL.  nq = 0 or C = 0 is a no-op. */
int oriana_cluster_distance_sums(const float *Q, int64_t nq, int64_t ldq, const float *Y, int64_t n, int64_t ldy, int64_t d,
                                 const int64_t *offsets, int64_t C, double *sums, int64_t lds, int accumulate, void *scratch,
                                 int64_t blocks, void *stream);
/* Bytes of scratch of a call with this Y and ldy, an upper bound for every valid offsets (negative: the argument error the call
 * would return): a padded image of the candidates (n pad4(d) floats; none where Y itself serves: d and ldy multiples of four, Y
 * 16-byte aligned; Y is not dereferenced), the work table, and 512 bytes per query tile and work item (at most min(C, n) +
 * ranges items). */
int64_t oriana_cluster_distance_sums_scratch_bytes_for(int64_t nq, int64_t n, int64_t d, int64_t C, int64_t blocks, const float *Y,
                                                       int64_t ldy);
/* The largest C served (32,768: the work items of a call are one extent of its grid). */
int64_t oriana_cluster_distance_sums_max_clusters(void);

/* ---- per-cell totals and per-cluster gene moments of the counts (oriana_amd/models/base.py: cell_totals,
 * cluster_gene_stats, marker_genes; no counterpart in the reference) --------------------------------------------------------
 * Sums over the NON-ZERO counts of both layouts of a model's matrix: cm is the sliced layout (of a hybrid matrix: its packed
 * genes [gd, m), as every entry above takes it), dn the dense block of a hybrid layout or NULL, row_perm / col_perm the FULL
 * orderings the dense block is read through (NULL = identity; the sliced layout carries its own).  Counts are read as stored
 * (float32 records, uint16 block); every sum is float64 and ADDS into its output with float64 atomics (the caller zeroes it;
 * reruns agree to the order of the additions -- exactly, while every partial sum is an integer below 2^53).
 *   oriana_cell_totals : totals[i] += sum_j x_ij, (n,) in the caller's row order.
 *   oriana_group_stats : labels (n,) int32 in the caller's row order, each in [0, C) (a label outside is never counted and never
 *                        addresses memory); scale (n,) float64 in the caller's row order or NULL.  Per non-zero count x of cell
 *                        i and gene j: y = x (scale == NULL) or (double)x * scale[i]; with log1p_flag y = log1p(y) in float64;
 *                        out[0, c, j] += 1, out[1, c, j] += y, out[2, c, j] += y * y with c = labels[i].  out: (3, C, m_all)
 *                        float64, caller's gene order, m_all = cm->m + (dn ? dn->gd : 0).
 *   oriana_group_stats_max_groups : the largest C (1024).
 * ORIANA_EINVAL for a NULL cm / labels / out / totals, a negative size, a dense block whose gd is no multiple of 32 or whose
 * cells are not cm's, or C < 1; ORIANA_EKRANGE for C above the limit; both before any HIP call.  0 without a launch for a
 * layout without a stored count. */
int oriana_cell_totals(const oriana_counts *cm, const oriana_dense *dn, const int32_t *row_perm, const int32_t *col_perm,
                       double *totals, void *stream);
int oriana_group_stats(const oriana_counts *cm, const oriana_dense *dn, const int32_t *row_perm, const int32_t *col_perm,
                       const int32_t *labels, const double *scale, int log1p_flag, int64_t C, double *out, void *stream);
int64_t oriana_group_stats_max_groups(void);

/* ---- gene-set scores: the transformed counts times a weight matrix (csrc/groupstats.hip, oriana_amd/models/base.py:
 * gene_scores, score_genes; no counterpart in the reference) ----------------------------------------------------
 * cm, dn, row_perm, col_perm, scale, log1p_flag: exactly as oriana_group_stats takes them.  W (m_all, S) float64, row-major, in
 * the caller's gene order, m_all = cm->m + (dn ? dn->gd : 0); out (n, S) float64, row-major, in the caller's row order.
 *   out[i, s] = sum over the stored counts x of cell i, gene j, of W[j, s] * y,  y as oriana_group_stats forms it,
 * every term one acc = fma(W[j, s], y, acc) in float64.  out is WRITTEN (the caller need not zero it): every element of the
 * (n, S) array, exactly 0 in every column for a cell without a stored count; nothing outside it.  W and out need 8-byte
 * alignment only.  No scratch.
 * The order of the additions is a fixed function of the two layouts and of S -- per cell: each of the 4 lanes of the sliced
 * kernel that hold the row over its slots in tile and slot order, the 4 lanes by a butterfly; then the dense block's 8 threads
 * of the cell, each over its genes in tile order, in thread order -- with no floating-point atomic anywhere and one writer per
 * element and launch: the same call gives the same bits on every run, whatever the grid does.
 *   oriana_gene_scores_max_sets  : the largest S (1024).
 *   oriana_gene_scores_set_chunk : the sets one work-group carries (8); the chunks of a larger S are one extent of the grid, the
 *                                  last one may be partial.
 * ORIANA_EINVAL for a NULL cm / W / out, S < 1, a layout oriana_group_stats refuses, or a grid beyond 2^31 - 1; ORIANA_EKRANGE
 * for S above the limit; all before any HIP call.  0 without a launch for n = 0. */
int oriana_gene_scores(const oriana_counts *cm, const oriana_dense *dn, const int32_t *row_perm, const int32_t *col_perm,
                       const double *scale, int log1p_flag, const double *W, int64_t S, double *out, void *stream);
int64_t oriana_gene_scores_max_sets(void);
int64_t oriana_gene_scores_set_chunk(void);

/* ---- tie-aware rank sums of the stored counts per (cluster, gene) (csrc/ranksum.hip, oriana_amd/models/base.py:
 * cluster_rank_sums, marker_genes(method='wilcoxon'); no counterpart in the reference) ---------------------------
 * cm, dn, row_perm, col_perm, labels, scale: as oriana_group_stats takes them (col_perm the FULL ordering or NULL; the outputs
 * go through it).  One call serves one PANEL: the genes [g0, g1) of the packed order, 0 <= g0 <= g1 <= m_all = cm->m + gd, either
 * inside the dense block (g0, g1 multiples of 32, g1 <= gd) or inside the sliced part (g0 - gd a multiple of 256; g1 - gd too
 * unless g1 = m_all).
 *   the key    of a stored count x of cell i: the bit pattern of the float64 v = (double)x * scale[i], ONE IEEE product
 *              (scale == NULL: v = x).  Precondition: scale[i] > 0 and finite for every cell with a stored count, so v > 0 and the
 *              unsigned 64-bit patterns order as the values do.  Two entries tie exactly when their patterns are equal.
 *   outputs    per gene j of the panel (caller's gene order), over its stored counts sorted by key, positions 1-based, a tie
 *              run occupying the positions [p, q] (t = q - p + 1 records):
 *                cnt[c, j]  = stored counts of the cells with labels[i] == c
 *                pos2[c, j] = sum over those entries of (p + q) of the entry's run: twice the sum of their average positions
 *                ties[j]    = sum over the runs of t^3 - t
 *              (C, m_all), (C, m_all), (m_all,) int64.  All C rows of the panel's columns and its ties are WRITTEN with plain
 *              stores (a gene belongs to one work-group); nothing outside the panel's columns is touched.  Every term is an
 *              integer: the same bits on every run, for every capacity that holds the panel and every lds_cap.  A cell whose
 *              label lies outside [0, C) is ranked like any other, adds to no cluster and never addresses memory through its label.
 *   scratch    oriana_rank_sums_scratch_bytes_for(capacity_records, g1 - g0) bytes, 16-byte aligned, contents undefined on entry
 *              and exit: per gene counts, offsets and cursors, then two buffers of capacity_records {key, label} records.  If
 *              the panel holds more stored counts than capacity_records, overflow[0] is set to 1, nothing is written outside
 *              the scratch and the outputs are left as they were; otherwise overflow is not written (the caller zeroes it).
 *   lds_cap    the longest segment (a gene's stored counts) one work-group sorts inside LDS; longer ones are cut into runs of
 *              the largest power of two <= lds_cap, sorted in LDS and merged pairwise through global memory.  0 = the default,
 *              oriana_rank_sums_lds_cap() = 4096, which is also the largest value.
 * ORIANA_EINVAL for a NULL cm / labels / output / overflow / scratch, a negative size, C < 1, a layout oriana_group_stats
 * refuses, a misaligned scratch, lds_cap outside [0, oriana_rank_sums_lds_cap()], a panel that is not tile-aligned or straddles
 * the two layouts; ORIANA_EKRANGE for C above oriana_rank_sums_max_groups() = 1024 or n >= 2^21 (sum (t^3 - t) <= n^3 < 2^63);
 * all before any HIP call.  0 without a launch for an empty panel or n = 0. */
int64_t oriana_rank_sums_max_groups(void);
int64_t oriana_rank_sums_lds_cap(void);
/* (negative: ORIANA_EINVAL for a negative argument) */
int64_t oriana_rank_sums_scratch_bytes_for(int64_t records, int64_t genes);
int oriana_rank_sums(const oriana_counts *cm, const oriana_dense *dn, const int32_t *row_perm, const int32_t *col_perm,
                     const int32_t *labels, const double *scale, int64_t C, int64_t g0, int64_t g1, void *scratch,
                     int64_t capacity_records, int64_t lds_cap, int64_t *pos2, int64_t *cnt, int64_t *ties, int32_t *overflow,
                     void *stream);

/* ---- the exact t-SNE layout of the cells (csrc/tsne.hip, oriana_amd/cluster.py: tsne) --------------------------
 * oriana_tsne_affinities : conditional neighbour probabilities at a perplexity.  sq_distances (n, k) float32 contiguous, what
 *   oriana_knn wrote: every row ascending and padded with +inf.  Per row, over its m finite entries, p_j = exp(-beta (d_j - d_0))
 *   / sum with the beta at which the entropy H = -sum p log p equals log(perplexity), all in float64.  The search is
 *   deterministic: from beta = 1 the value is doubled (halved) while no upper (lower) bracket exists, then bisected; it stops at
 *   |H - log perplexity| <= 1e-9 or after oriana_tsne_affinity_steps() = 200 evaluations of H.  p (n, k) float32 (exactly 0 at
 *   the padded slots) and beta (n) float64 are written.  A row whose finite entries are all equal gets the uniform distribution
 *   and a finite beta; a row without finite entries p = 0 and beta = 1.  Whether a row holds enough finite entries for the
 *   perplexity is the caller's check.  n < 0, k < 1, a perplexity that is not in [1, inf), a NULL pointer with n > 0 ->
 *   ORIANA_EINVAL; n = 0 is a no-op.
 * oriana_tsne_attract : P (n, n) as CSR (row_ptr (n + 1) int64, cols int32 within [0, n) -- an entry outside is skipped and
 *   addresses nothing --, vals float32), Y (n, 2) float32 contiguous, 8-byte aligned.  In float64, with D = 1 + |y_i - y_j|^2:
 *   attr[i] = sum_j P_ij (y_i - y_j) / D, (n, 2); klrow[i] = sum_j P_ij (log P_ij + log D) over the entries with P_ij > 0.  One
 *   wave per row: lane l takes the row's entries l, l + 64, .. in order and the 64 partial sums are added in one fixed shape, so
 *   a row's bits depend on the row alone.  n < 0 or beyond 2^31 - 1, a NULL row_ptr / Y / attr / klrow with n > 0, a misaligned
 *   Y -> ORIANA_EINVAL; n = 0 is a no-op.
 * oriana_tsne_repulse : queries Q (nq, 2) and candidates Y (n, 2), float32 contiguous, 8-byte aligned.  rep[i] = sum_j w_ij^2
 *   (q_i - y_j), (nq, 2) float64, and zrow[i] = sum_j w_ij, (nq) float64, over ALL candidates (nothing is excluded).
 *   the pair   one float32 sequence: dx = qx - yx and dy = qy - yy, each rounded once; s = fmaf(dy, dy, fmaf(dx, dx, 1));
 *              w = the hardware reciprocal of s (v_rcp_f32, 1 ulp); w2 = w * w; the terms w, w2 * dx, w2 * dy, the last two
 *              entering their sums by fmaf (the products are not rounded on their own).  A pair of bit-identical points
 *              gives w = 1 exactly and force terms of exactly 0.
 *   the sum    every w is converted to float64 and added in float64 (Z loses nothing to the n exact self pairs the caller
 *              subtracts).  The candidates are taken in steps of 8; the force terms of one step are added in float32 in
 *              candidate order starting from 0, each step's two sums are converted to float64 and everything beyond is added in
 *              float64.  No atomics:
 *              every sum has one writer.  Inside a launch the order is fixed by the plan (a function of nq, n and `blocks`), so
 *              the same call twice gives the same bits.  Bits are NOT promised across different partitions of the candidates:
 *              `blocks` cuts at whole steps, so the step sums are the same bit for bit and only the float64 summation order
 *              differs; so it is for accumulating calls whose candidate chunks are multiples of 8, while other chunk sizes
 *              move candidates between steps (the float32 order inside a step differs too).  A partition of the QUERIES
 *              changes nothing.
 *   accumulate = 0 overwrites rep and zrow of the nq queries (n = 0: zeros), 1 adds the call's sums to what is there.
 *   `blocks`: ranges the candidates are cut into (0: sized from the device, two work-groups per CU; at most 32,767 and at most
 *   one per step).  scratch: oriana_tsne_repulse_scratch_bytes_for(nq, n, blocks) bytes (1,536 per query tile and range), 16-byte
 *   aligned, contents undefined on entry and exit.
 *   A negative size or `blocks`, nq beyond 2^31 - 1, n beyond 2^31 - 9 (the step counter is 32-bit), a NULL scratch, a NULL Q /
 *   rep / zrow with nq > 0, a NULL Y with n > 0, a misaligned scratch, Q or Y -> ORIANA_EINVAL, all before any HIP call.  nq = 0
 *   is a no-op. */
int oriana_tsne_affinities(const float *sq_distances, int64_t n, int64_t k, double perplexity, float *p, double *beta, void *stream);
int64_t oriana_tsne_affinity_steps(void);
int oriana_tsne_attract(const int64_t *row_ptr, const int32_t *cols, const float *vals, const float *Y, int64_t n, double *attr,
                        double *klrow, void *stream);
int oriana_tsne_repulse(const float *Q, int64_t nq, const float *Y, int64_t n, double *rep, double *zrow, int accumulate,
                        void *scratch, int64_t blocks, void *stream);
/* Bytes of scratch of such a call (negative: the argument error the call would return). */
int64_t oriana_tsne_repulse_scratch_bytes_for(int64_t nq, int64_t n, int64_t blocks);

/* ---- communities on the neighbour graph (csrc/community.hip, oriana_amd/cluster.py: snn_graph, louvain; no
 * counterpart in the reference) --------------------------------------------------------------------------------------------------
 * A graph is symmetric CSR: row_ptr (n + 1) int64, cols int32 ascending inside a row, weights int64 >= 0.
 * oriana_snn_weights : indices (n, k) int32 contiguous as oriana_knn wrote it.  Nc(i) = the entries of row i inside [0, n) other
 *   than i (no entry twice: the caller's check), and i itself.  For every stored entry e of row i with column j,
 *   weights[e] = |Nc(i) & Nc(j)|, an integer whatever the enumeration; a column outside [0, n) gets 0 and addresses nothing.  n < 0
 *   or beyond 2^31 - 1, k < 1 or beyond oriana_knn_max_neighbors(1), a NULL indices / row_ptr with n > 0 -> ORIANA_EINVAL before
 *   any HIP call; n = 0 is a no-op.
 * oriana_louvain_sweep : ONE synchronous local-moving sweep of Louvain's method.  deg[i] = the sum of the weights of row i (a self
 *   entry, present at aggregated levels, included), two_m = sum deg with two_m^2 < 2^63; the state is comm (n) int32 within
 *   [0, n), tot[c] = sum of deg over community c (int64), size[c] = its nodes (int32).  For node i with a = comm[i] the
 *   candidates are a and comm[j] of every stored j != i;
 *     k_ic = sum of w_ij over j != i with comm[j] = c (the self entry never counts; k_ia may be 0)
 *     tot'_c = tot[c] - [c = a] deg_i
 *     g(c) = __dsub_rn((double)(two_m * k_ic), __dmul_rn(resolution, (double)(deg_i * tot'_c)))
 *   both integer products exact in int64, each converted once, the product and the difference rounded once each.  c* = the
 *   candidate of the largest g, ties to the smallest id; i moves to c* iff c* != a and g(c*) > g(a); where size[a] = 1 and
 *   size[c*] = 1 the move is taken only when c* < a.  Every decision reads the OLD comm, tot and size: comm_new (n) and moved[0],
 *   the number of nodes with comm_new != comm, are all that is written, and they are the same bits for every `blocks`,
 *   row_cap and scratch that holds the tables.  An entry of comm or cols outside [0, n) addresses nothing.
 *   row_cap   rows of at most row_cap entries are served by one wave with a table in LDS; 0 = oriana_louvain_row_cap() = 128,
 *             which is also the largest value.  The longer rows are the caller's list: long_rows (n_long) int32, exactly the
 *             rows with more than row_cap entries, and long_off (n_long + 1) int64, where the table of long row q starts in the
 *             scratch, in slots; the table of a row of len entries has T(len) = max(64, the least power of two >= 2 len) slots,
 *             and long_off[n_long] is their sum.  A listed row that is not long, or whose table would leave the scratch, is
 *             skipped.
 *   scratch   scratch_bytes bytes, at least 16, 16-byte aligned, contents undefined on entry and exit: a 16-byte header, then 16
 *             bytes per slot; oriana_louvain_sweep_scratch_bytes_for(long_off[n_long]) bytes hold every table.  If they do not
 *             fit, overflow[0] is set to 1 and nothing else is written outside the scratch; otherwise overflow is not written
 *             (the caller zeroes it).
 *   `blocks`  work-groups of each launch (0: sized from the device).
 * ORIANA_EINVAL before any HIP call for n < 0 or beyond 2^31 - 1, two_m < 0 or two_m^2 >= 2^63, a resolution that is not finite
 * and positive, row_cap outside [0, oriana_louvain_row_cap()], negative blocks or n_long, n_long > n, scratch_bytes < 16, a NULL
 * or misaligned scratch, a NULL moved / overflow, with n > 0 a NULL row_ptr / deg / comm / tot / size / comm_new, with n_long > 0
 * a NULL long_rows / long_off. */
int oriana_snn_weights(const int32_t *indices, int64_t n, int64_t k, const int64_t *row_ptr, const int32_t *cols, int64_t *weights,
                       void *stream);
int64_t oriana_louvain_row_cap(void);
/* (negative: ORIANA_EINVAL for a negative argument) */
int64_t oriana_louvain_sweep_scratch_bytes_for(int64_t long_slots);
int oriana_louvain_sweep(int64_t n, const int64_t *row_ptr, const int32_t *cols, const int64_t *weights, const int64_t *deg,
                         int64_t two_m, double resolution, const int32_t *comm, const int64_t *tot, const int32_t *size,
                         int64_t row_cap, const int32_t *long_rows, const int64_t *long_off, int64_t n_long, void *scratch,
                         int64_t scratch_bytes, int32_t *comm_new, int64_t *moved, int32_t *overflow, int64_t blocks, void *stream);

/* ---- diffusion maps on the neighbour graph (csrc/diffusion.hip, oriana_amd/cluster.py: diffusion_graph, diffusion_map; DESIGN.md
 * 5p; no counterpart in the reference) -------------------------------------------------------------------------------------------
 * All float64, no float atomics: every result is the same bits for every `blocks` (0: sized from the device), for whatever a
 * scratch held, and on repetition.
 * oriana_csr_spmv_f64 : y = A x, A in CSR (row_ptr (n + 1) int64, cols int32, vals float64; x and y hold n entries).  A row is
 *   served by an aligned group of 16 lanes: lane l adds the entries l, l + 16, ... of the row as one ascending fma chain starting
 *   from 0, then the 16 sums are added by lane ^ 1, lane ^ 2 and the two mirrors inside the group.  An entry whose column lies
 *   outside [0, n) addresses nothing and adds nothing.  n < 0 or beyond 2^31 - 1, negative blocks, with n > 0 a NULL row_ptr / x /
 *   y -> ORIANA_EINVAL before any HIP call; n = 0 is a no-op.
 * A basis Q holds its columns contiguously: column c starts at Q + c * ldq, ldq >= n and even, Q 16-byte aligned.
 * oriana_basis_orthogonalize_f64 : classical Gram-Schmidt of w (n, 16-byte aligned) against the first j columns of Q, `passes`
 *   (1 or 2) times: c = Q^T w, w <- w - Q c, h <- h + c (h holds j entries and is ADDED to: the caller zeroes it for a new w);
 *   then beta2[0] = ||w||^2.  Sums over rows run over tiles of oriana_basis_tile_rows() rows (a function of nothing): inside a tile
 *   each lane adds its rows as an ascending fma chain and the wave's lanes are added in a fixed order; the tiles are added in
 *   ascending order.  The subtraction is one fma per column, columns ascending.  Q is read twice per pass.
 *   scratch: oriana_basis_orthogonalize_scratch_bytes_for(n, j) bytes, 16-byte aligned, contents undefined on entry and exit,
 *   nothing written outside it; a scratch_bytes below that size -> ORIANA_EINVAL.
 * oriana_basis_append_f64 : column j of Q (j >= 0) = w / sqrt(beta2[0]), the root and the quotients correctly rounded; beta2 is
 *   read on the device.
 * oriana_basis_combine_f64 : out = Q S for S (j, m) row-major; out holds its m columns like a basis (ldo >= n and even, 16-byte
 *   aligned); out[r, c] = an fma chain over k = 0 .. j - 1 ascending, starting from 0.  m = 0 is a no-op.
 * ORIANA_EINVAL before any HIP call for a negative size or `blocks`, n beyond 2^38, j < 1 (append: j < 0) or j / m beyond 2^20,
 * ldq < n, ldo < n or either odd, passes outside {1, 2}, and with n > 0 a NULL or misaligned Q / w / out / scratch and a NULL h /
 * beta2 / S.  n = 0 is a no-op. */
int oriana_csr_spmv_f64(int64_t n, const int64_t *row_ptr, const int32_t *cols, const double *vals, const double *x, double *y,
                        int64_t blocks, void *stream);
int64_t oriana_basis_tile_rows(void);
/* (negative: ORIANA_EINVAL for sizes the call would refuse) */
int64_t oriana_basis_orthogonalize_scratch_bytes_for(int64_t n, int64_t j);
int oriana_basis_orthogonalize_f64(int64_t n, const double *Q, int64_t ldq, int64_t j, double *w, double *h, double *beta2,
                                   int64_t passes, void *scratch, int64_t scratch_bytes, int64_t blocks, void *stream);
int oriana_basis_append_f64(int64_t n, double *Q, int64_t ldq, int64_t j, const double *w, const double *beta2, void *stream);
int oriana_basis_combine_f64(int64_t n, const double *Q, int64_t ldq, int64_t j, const double *S, int64_t m, double *out,
                             int64_t ldo, int64_t blocks, void *stream);

/* ---- Harmony batch correction of the cell features (csrc/harmony.hip, oriana_amd/cluster.py: harmony; no counterpart
 * in the reference) ----------------------------------------------------------------------------------------------------------------
 * Rows are float32 with a row stride >= d and unit column stride; batch (n) int32 within [0, B) (a value outside addresses nothing:
 * the row then belongs to no batch); R (n, K) float32 contiguous; K <= oriana_harmony_max_clusters(d), B <=
 * oriana_harmony_max_batches(), d <= 256, else ORIANA_EKRANGE.  No float atomics: for a given `blocks` (0: sized from the device)
 * every output is the same bits on repetition and for whatever the scratch held.  scratch: the entry's *_scratch_bytes(n, d, K, B,
 * blocks) bytes, 16-byte aligned, contents undefined on entry and exit.  ORIANA_EINVAL before any HIP call for a negative size or
 * `blocks`, d, K or B < 1, a row stride < d, n beyond 2^31 - 65, a NULL or misaligned scratch, a NULL required pointer.
 * oriana_harmony_assign : for the n rows at Z (a row range of the caller's matrix; batch and R point at the same first row)
 *   THE PAIR, all float32, one rounding per step, c = float32(-inv_sigma * log2(e)):
 *     dot_k  = fl(acc + cmp) after a compensated chain over the features ascending from 0 (y: centers (K, d) float32): per
 *              feature p = fl(z_f y_kf), ep = fmaf(z_f, y_kf, -p), s = fl(acc + p), bb = fl(s - acc),
 *              es = fl(fl(acc - fl(s - bb)) + fl(p - bb)), acc = s, cmp = fl(cmp + fl(ep + es))
 *     dist_k = fmaf(-2, dot_k, 2);  m = min_k dist_k
 *     e_k    = exp2(fl(fl(dist_k - m) * c)) * P[k, batch]     (exp2: v_exp_f32, 1 ulp; P (K, B) float32, positive)
 *     s      = e_0 + e_1 + ... ascending;  R_k = e_k * fl(1 / s)                  (1 / s correctly rounded)
 *   A row's R depends on nothing but the row, the centres, P and c.  Also, in float64 and in a fixed order given `blocks`:
 *   O_blk[k, b] = sum over the range's rows of batch b of R_k; sums[0] = sum R_k dist_k; sums[1] = sum R_k logf(R_k) over
 *   R_k > 0 (each product exact in float64).  inv_sigma must be finite and positive.  n = 0: O_blk and sums are zeroed.
 * oriana_harmony_moments : S[k, b, :] = sum_{batch_i = b} R_ik x_i (K, B, d) and O[k, b] = sum_{batch_i = b} R_ik, float64.  The rows
 *   of one batch inside a tile of 64 rows are taken in ascending order, oriana_harmony_partial_rows() at a time: those as one float32
 *   fmaf chain from 0, the chains' values then in float64, groups ascending, tiles ascending inside a range, ranges ascending.  One
 *   writer per partial sum.  n = 0: zeroed.
 * oriana_harmony_correct : Zcorr[i, f] = z_if - s, s = the fmaf chain over k ascending from 0 of R_ik * W[k, batch_i, f] (W (K, B, d)
 *   float32); Zcos[i, :] = Zcorr[i, :] / sqrt(a), a = the fmaf chain over f ascending of Zcorr_if^2 (root and quotient correctly
 *   rounded); a = 0 writes a zero row.  Zcorr and Zcos are (n, d) contiguous.  n = 0 is a no-op. */
int64_t oriana_harmony_max_clusters(int64_t d);      /* 0: d is not served */
int64_t oriana_harmony_max_batches(void);
int64_t oriana_harmony_partial_rows(void);
/* (negative: the argument error the call would return) */
int64_t oriana_harmony_assign_scratch_bytes(int64_t n, int64_t d, int64_t K, int64_t B, int64_t blocks);
int64_t oriana_harmony_moments_scratch_bytes(int64_t n, int64_t d, int64_t K, int64_t B, int64_t blocks);
int64_t oriana_harmony_correct_scratch_bytes(int64_t n, int64_t d, int64_t K, int64_t B, int64_t blocks);
int oriana_harmony_assign(const float *Z, int64_t n, int64_t d, int64_t ldz, const int32_t *batch, const float *centers, int64_t K,
                          const float *P, int64_t B, double inv_sigma, float *R, double *O_blk, double *sums, void *scratch,
                          int64_t blocks, void *stream);
int oriana_harmony_moments(const float *X, int64_t n, int64_t d, int64_t ldx, const float *R, int64_t K, const int32_t *batch,
                           int64_t B, double *S, double *O, void *scratch, int64_t blocks, void *stream);
int oriana_harmony_correct(const float *Z, int64_t n, int64_t d, int64_t ldz, const float *R, int64_t K, const int32_t *batch,
                           const float *W, int64_t B, float *Zcorr, float *Zcos, void *scratch, int64_t blocks, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ORIANA_HIP_H */
