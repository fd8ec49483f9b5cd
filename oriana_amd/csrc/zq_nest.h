// zq_nest.h -- the launch sequence of one loop nest (gap.py:67-80, zigap.py:79-95, sparse_gap.py:81-97, sparse_zigap.py:100-116),
// written ONCE for the C entries that run a whole nest: the resident handle (resident.hip) and the stateless drop-ins
// (stateless.hip).  An entry validates, provides the buffers its variant needs, fills a ZqView and calls zq_run:
//     preparation (+ clear list) -> row pass -> slow path -> [second row product] -> dense genes -> finalize rows
//     -> per-gene sums -> finalize genes -> log sums.
// engine.zq (oriana_amd/engine.py) is the ONE Python copy of this sequence, in the same order, for the model classes: it
// interleaves their timers, the cell-side update, the sharded exchange and the deterministic mode.
#pragma once
#include "common.h"
#include <string.h>

namespace oriana {

#define ORIANA_TRY(expr) do { const int _rc = (expr); if (_rc) return _rc; } while (0)

// Everything a nest touches.  Pointers are NULL where the variant has none.
struct ZqView {
    const oriana_counts *cm = nullptr;          // the sliced genes [gd, m)
    const oriana_dense *dn = nullptr;           // the dense genes [0, gd) of a hybrid layout
    int64_t n = 0, m = 0, K = 0, Kp = 0, gd = 0;
    float *FU = nullptr, *FV = nullptr, *R = nullptr, *C = nullptr, *s_cs = nullptr, *prep = nullptr;
    int32_t *tile_flag = nullptr;
    // the ZI / sparse nests.  GQ (FU * dq) may be G2 itself unless two_image, which keeps both alive at once.
    float *F2 = nullptr, *G2 = nullptr, *C2 = nullptr, *dq = nullptr, *GQ = nullptr, *s_rs = nullptr, *sw_cs = nullptr;
    const float *w_nz = nullptr;                // D_hat at the stored entries (general weights; needs sw_cs)
    float *dn_S = nullptr;
    int32_t *dn_flag = nullptr;
    void *dn_imgV = nullptr, *dn_imgU = nullptr;
    int64_t dn_gene_splits = 1, dn_cell_splits = 1;
    const oriana_row_split *split = nullptr;    // NULL: none (R is one slab)
    const int32_t *col_perm = nullptr, *col_work = nullptr, *col_work1 = nullptr;
    int64_t n_col_work = 0, n_col_work1 = 0;
    bool dynamic_den = false;                   // the den threshold of the preparation (false: the constant 1e-10)
    bool clear_outputs = false;                 // Z_i, Z_j, Z_log join the clear list (false: the caller has zeroed them)
    // The two-image kernels where they fit (Kp <= 64): the sparse nests' S_hat-weighted row sums out of the row pass, both
    // per-gene sums out of one dual column pass.  Their second operands (F2, G2) are then prepared ahead of the pass.
    bool two_image = false;
};

static inline const float *zq_den_min(const float *prep) {
    return reinterpret_cast<const float *>(reinterpret_cast<const char *>(prep) + oriana_prep_den_threshold_offset());
}
static inline double *zq_center(float *prep) {
    return reinterpret_cast<double *>(reinterpret_cast<char *>(prep) + oriana_prep_center_offset());
}
// rows of R: slabs 1.. of a last-round split hold the rows of the split row blocks only
static inline int64_t zq_r_rows(int64_t n, const oriana_row_split *sp) {
    return sp ? n + (int64_t)(sp->parts - 1) * (n - (int64_t)sp->nfull * TILE) : n;
}
// the dense row kernel follows a last-round split of the sliced row pass (its blocks from nfull on in `parts` gene ranges,
// adding into the slabs of R) when R has those slabs in this call and the dense genes have no split of their own
static inline bool zq_dense_tail(const ZqView &v, int64_t nslab) {
    const oriana_row_split *sp = v.split;
    return sp && sp->nfull > 0 && sp->parts > 1 && sp->parts == nslab && v.dn_gene_splits == 1 && sp->parts <= v.gd / 32;
}
// what the preparation's second launch zero-fills on the side
static inline oriana_clear_list zq_clear_list(const ZqView &v, float *Zi, float *Zj, float *Zlog, bool have_sliced) {
    oriana_clear_list cl;
    memset(&cl, 0, sizeof(cl));
    int e = 0;
    auto add = [&](void *p, int64_t bytes) { cl.ptr[e] = p; cl.bytes[e++] = bytes; };
    const int64_t nt = v.cm->nrb * v.cm->ncb;
    if (v.clear_outputs) { add(Zi, (int64_t)sizeof(float) * v.n * v.K); add(Zj, (int64_t)sizeof(float) * v.m * v.K); }
    add(v.C, (int64_t)sizeof(float) * v.m * v.Kp);
    add(v.tile_flag, (int64_t)sizeof(int32_t) * (nt > 0 ? nt : 1));
    if (Zlog && v.clear_outputs) add(Zlog, (int64_t)sizeof(float) * v.m * v.K);
    if (Zlog) add(v.C2, (int64_t)sizeof(float) * v.m * v.Kp);
    if (!have_sliced) add(v.R, (int64_t)sizeof(float) * zq_r_rows(v.n, v.split) * v.Kp);      // (no row pass overwrites it)
    return cl;
}

// One nest.  S_tilde / S_hat: both or neither (the sparse models); Zlog may be NULL (the log sums are skipped); v.w_nz: the
// per-gene sums and log sums are D_hat[i, j]-weighted; v.dq: zigap.py:94, Z_j weighted by D_hat[i, k] on the plain s --
// dq_src given: v.dq is taken from its first K columns here.
static int zq_run(const ZqView &v, float *Zi, float *Zj, float *Zlog, const float *lu, const float *lv, const float *S_tilde,
                  const float *S_hat, const float *dq_src, void *stream) {
    const int64_t n = v.n, m = v.m, K = v.K, gd = v.gd, goff = gd * v.Kp;
    const oriana_counts *cm = v.cm;
    const bool sparse = S_hat != nullptr, have_sliced = m > gd || gd == 0;
    const float *w_nz = v.w_nz, *den_min = v.dynamic_den ? zq_den_min(v.prep) : nullptr;
    float *sw_cs = w_nz ? v.sw_cs : nullptr, *dq = v.dq;
    if (gd > 0 && (w_nz || !v.two_image)) return ORIANA_EINVAL;     // (the dense-gene kernels carry no per-entry weights)
    const oriana_clear_list cl = zq_clear_list(v, Zi, Zj, Zlog, have_sliced);
    ORIANA_TRY(oriana_factor_prep_pair_clear(v.FU, v.FV, lu, lv, S_tilde, nullptr, v.col_perm, n, m, K, v.prep, &cl, stream));
    if (dq && dq_src) ORIANA_TRY(oriana_take_cols_f32(dq, dq_src, n, m, K, stream));
    auto scale_f2 = [&]() { return oriana_scale_factor(v.F2, v.FV, S_hat, v.col_perm, m, K, 0, stream); };
    if (sparse && v.two_image) ORIANA_TRY(scale_f2());
    const int variant = (sparse ? 1 : 0) | (w_nz ? 2 : 0) | (dq ? 4 : 0);
    const int64_t slab_row0 = v.split ? (int64_t)v.split->nfull * TILE : 0;
    int64_t nslab = 1;
    if (have_sliced) {
        bool fused = false;
        if (sparse && v.two_image) {
            const int rc = oriana_row_pass_general(cm, v.FU, v.FV + goff, v.F2 + goff, w_nz, v.R, v.s_cs, sw_cs, nullptr, v.tile_flag, K,
                                                   v.split, den_min, stream);
            if (rc != 0 && rc != ORIANA_EKRANGE) return rc;
            fused = rc == 0;
        }
        float *s_rs = (sparse && !fused) ? v.s_rs : nullptr;
        if (sparse && !fused && !s_rs) return ORIANA_EINVAL;
        if (!fused)
            ORIANA_TRY(oriana_row_pass_general(cm, v.FU, v.FV + goff, nullptr, w_nz, v.R, v.s_cs, sw_cs, s_rs, v.tile_flag, K, v.split,
                                               den_min, stream));
        if (!s_rs && v.split) nslab = v.split->parts;       // (with s_rs the pass leaves R alone: the second row product writes one slab)
        ORIANA_TRY(oriana_fixup(cm, v.tile_flag, v.s_cs, sw_cs, s_rs, lu, lv, S_tilde, S_hat, w_nz, dq, Zi, Zj, Zlog, K, variant, stream));
        if (s_rs) {
            // S_hat-weighted row sums (sparse_gap.py:95): a second row product with FV * S_hat
            if (!v.two_image) ORIANA_TRY(scale_f2());
            ORIANA_TRY(oriana_row_spmm(cm, s_rs, w_nz, v.F2 + goff, v.R, K, stream));
        }
    }
    if (gd > 0) {
        ORIANA_TRY(oriana_dense_images2(v.dn_imgV, v.FV, sparse ? v.F2 : nullptr, gd, K, 0, stream));
        const bool tail = zq_dense_tail(v, nslab);
        ORIANA_TRY(oriana_dense_row_pass_tail(v.dn, v.FU, v.dn_imgV, v.R, v.dn_S, v.dn_flag, K, v.dn_gene_splits, tail ? v.split->nfull : 0,
                                              tail ? v.split->parts : 1, den_min, stream));
        ORIANA_TRY(oriana_dense_fixup_variant(v.dn, v.dn_flag, v.dn_S, lu, lv, nullptr, v.col_perm, Zi, Zj, Zlog, dq, S_tilde, S_hat, K, 0,
                                              stream));
    }
    ORIANA_TRY(oriana_finalize_slabs_from(Zi, v.FU, v.R, nslab, slab_row0, nullptr, n, K, stream));
    // ---- per-gene sums: D_hat[i, j]-weighted (sw), or -- zigap.py:94 -- weighted by D_hat[i, k] on the plain s
    double *center = zq_center(v.prep);
    auto center_g2 = [&]() -> int {     // sum_i r_ijk (lu_ik + lv_jk) = FV (sum_i s FU lu) + FV lv (sum_i s FU), lu centred
        ORIANA_TRY(oriana_log_center(center, v.FU, lu, Zi, nullptr, n, K, stream));
        return oriana_scale_factor_centered(v.G2, v.FU, lu, center, nullptr, n, K, stream);
    };
    auto cols = [&](const float *s, const float *G, float *Cm) -> int {
        if (have_sliced) ORIANA_TRY(oriana_col_pass(cm, s, G, Cm + goff, K, v.col_work, v.n_col_work, stream));
        return 0;
    };
    auto dense_cols = [&](const float *G, float *Cm) -> int {
        if (gd == 0) return 0;
        ORIANA_TRY(oriana_dense_images(v.dn_imgU, G, n, K, 1, stream));
        return oriana_dense_col_pass(v.dn, v.dn_imgU, v.dn_S, Cm, K, v.dn_cell_splits, stream);
    };
    const float *s_log = sw_cs ? sw_cs : v.s_cs, *s_j = s_log, *G = v.FU;
    auto dual = [&](bool *done) -> int {      // C += s FU and C2 += s G2 from one walk over the stream, where two images fit
        *done = false;
        if (!v.two_image || !v.col_work1 || !have_sliced) return 0;
        const int rc = oriana_col_pass_dual(cm, s_log, v.FU, v.G2, v.C + goff, v.C2 + goff, K, v.col_work1, v.n_col_work1, stream);
        if (rc != 0 && rc != ORIANA_EKRANGE) return rc;
        *done = rc == 0;
        return 0;
    };
    if (Zlog && v.two_image) ORIANA_TRY(center_g2());
    if (dq) { ORIANA_TRY(oriana_scale_factor(v.GQ, v.FU, dq, nullptr, n, K, 0, stream)); G = v.GQ; s_j = v.s_cs; }
    bool dual_done = false;
    if (Zlog && !dq) ORIANA_TRY(dual(&dual_done));
    if (!dual_done) ORIANA_TRY(cols(s_j, G, v.C));
    ORIANA_TRY(dense_cols(G, v.C));
    ORIANA_TRY(oriana_finalize(Zj, v.FV, v.C, nullptr, v.col_perm, m, K, 1, stream));
    if (!Zlog) return 0;
    if (dq) {                                 // the log sums use the plain column sums (zigap.py:95), Z_j the D_hat[i, k]-weighted ones
        ORIANA_HIP_CHECK(hipMemsetAsync(v.C, 0, sizeof(float) * m * v.Kp, (hipStream_t)stream));
        ORIANA_TRY(dual(&dual_done));
        if (!dual_done) ORIANA_TRY(cols(s_log, v.FU, v.C));
        ORIANA_TRY(dense_cols(v.FU, v.C));
    }
    if (!v.two_image) ORIANA_TRY(center_g2());
    if (!dual_done) ORIANA_TRY(cols(s_log, v.G2, v.C2));
    ORIANA_TRY(dense_cols(v.G2, v.C2));
    return oriana_finalize_zlog(Zlog, v.FV, v.C2, v.C, lv, center, v.col_perm, m, K, stream);
}

}  // namespace oriana
