// passes.hip -- the responsibility pass of CAVI for pCMF-type models on gfx950.
//
// Replaces the four numba loop nests (oriana/models/gap.py:67-80, zigap.py:79-95,
// sparse_gap.py:81-97, sparse_zigap.py:100-116).  With FU = exp(E[log U] - rowshift) and
// FV = exp(E[log V] - rowshift) (oriana_factor_prep), for every non-zero count x_ij
//     den_ij = sum_k FU[i,k] FV[j,k]            s_ij = x_ij / den_ij
//     Z_i[i,k] = FU[i,k] * sum_j s_ij FV[j,k]    (row pass, register accumulators)
//     Z_j[j,k] = FV[j,k] * sum_i s_ij FU[i,k]    (column pass, register accumulators)
// which is r_ijk = x_ij e_k / sum_k e_k, e_k = exp(lu_ik + lv_jk), summed over j and over i, with
// the shifts cancelling in the ratio.  Zero counts contribute nothing (gap.py:78) and are never
// touched: X lives in HBM as 256 x 256 tiles of sliced non-zero records (pack.hip).
//
// Mapping (wave64): a group of G lanes owns one row (row pass) or one column (column pass) for
// the whole kernel and keeps its K-vector and its accumulator in registers, 4*T4 floats per lane
// (Kp = 4*G*T4).  The other side's K-vectors are staged through LDS, 256 rows at a time, and
// read with ds_read_b128.  A wave streams its slice of the tile 64 slots (one 512-byte load) per
// iteration and walks the four records of each quad with DPP broadcasts; the inner loops have no
// data-dependent branch.  No MFMA: the work is a sampled dot product per non-zero plus two scaled
// vector adds over the sparse support of X, not a dense contraction.
#include "launch.h"
#include <string.h>
#include <stdlib.h>

// (the ablation switches of rounds 1-4 -- no barriers, no scattered s stores, masked padding slots, rotation variants, staging
//  once, staggered waves -- are archived as tools/experiments/passes_ablation_switches_r4.diff)

#include "passes_prep.h"
#include "passes_generic.h"
#include "passes_k100.h"
#include "passes_k64.h"
#include "passes_narrow.h"

namespace oriana {

// ------------------------------------------------------------------------------------------
// dispatch on K:  Kp = 4 * G * T4 (+ G * TAIL)
// ------------------------------------------------------------------------------------------
struct KCfg {
    int G, T4, TAIL;
    constexpr int kp() const { return 4 * G * T4 + G * TAIL; }
};
// Kp = 16 t (+4): the smallest padded width that holds K.  The tail (one extra float per lane)
// keeps K = 20, 50, 100 ... free of padding work.
static inline bool pick_cfg(int64_t K, KCfg *c) {
    if (K <= 0) return false;
    for (int t = 1; t <= 7; ++t) {
        if (K <= 16 * t) { *c = {4, t, 0}; return true; }
        if (t <= 6 && K <= 16 * t + 4) { *c = {4, t, 1}; return true; }
    }
    if (K <= 128) { *c = {8, 4, 0}; return true; }
    if (K <= 160) { *c = {8, 5, 0}; return true; }
    if (K <= 192) { *c = {8, 6, 0}; return true; }
    if (K <= 224) { *c = {8, 7, 0}; return true; }
    if (K <= 256) { *c = {16, 4, 0}; return true; }
    return false;
}

// run-time configuration -> template arguments: the 18 configurations pick_cfg can return, by Kp / 4
#define ORIANA_FOR_CFG(cfg, CALL)                                                                                         \
    switch ((cfg).kp() / 4) {                                                                                             \
    case 4: CALL(4, 1, 0);   case 5: CALL(4, 1, 1);   case 8: CALL(4, 2, 0);   case 9: CALL(4, 2, 1);                     \
    case 12: CALL(4, 3, 0);  case 13: CALL(4, 3, 1);  case 16: CALL(4, 4, 0);  case 17: CALL(4, 4, 1);                    \
    case 20: CALL(4, 5, 0);  case 21: CALL(4, 5, 1);  case 24: CALL(4, 6, 0);  case 25: CALL(4, 6, 1);                    \
    case 28: CALL(4, 7, 0);  case 32: CALL(8, 4, 0);  case 40: CALL(8, 5, 0);  case 48: CALL(8, 6, 0);                    \
    case 56: CALL(8, 7, 0);  case 64: CALL(16, 4, 0);                                                                     \
    default: return ORIANA_EKRANGE;                                                                                       \
    }

// ------------------------------------------------------------------------------------------
// Which kernel family serves which configuration.  These functions are the whole rule: the launchers below name a kernel
// template only under `if constexpr` on their answers (what is compiled is what can be launched), the planning entries
// (oriana_row_pass_plan_cus, oriana_col_block_tiles) ask them too, and DESIGN.md section 0 shows them as a table per model.
// (rounds 1-4 selected older generations with ORIANA_PASS_IMPL=r1|r2|r3 for A/B runs: gone; the git history has them)
// ------------------------------------------------------------------------------------------
enum class Fam {
    none,       // no kernel: the entry answers ORIANA_EKRANGE ("not this form's case") and the caller takes its other form
    narrow,     // passes_narrow.h: one lane per row / gene
    k64,        // passes_k64.h: two lanes per row / gene, rows zero-padded to 64 floats
    k100,       // passes_k100.h, k_row_pass_k100: two lanes per row, duplicated chunk groups
    col2,       // passes_k100.h, k_col_pass2: four lanes per gene; two column tiles per image, or (DUAL) two images of one tile
    generic     // passes_generic.h: G lanes per row / gene
};
// row-pass variant = the VAR argument of the row kernels (bits 0 and 2 exclude each other: oriana_row_pass_general)
constexpr int V_SROW = 1, V_WEIGHTS = 2, V_IMAGE2 = 4;
enum class Col { plain, partials, dual };       // C += s G;  the same into per-item slabs (Cpart);  two products from one walk

// one staged image of 256 factor rows for the generic kernels (rows padded to 256 bytes; column sub-tiles above 160 KB)
static constexpr size_t lds_bytes(KCfg c) { return (size_t)(TILE / pick_nsub(c.kp())) * lds_stride_floats(c.kp()) * sizeof(float); }

static constexpr Fam row_family(KCfg c, int V) {
    const int kp = c.kp();
    if (kp >= 36 && kp <= 64) return Fam::k64;                   // every variant; a second image is a second 64 KB
    if (V & V_IMAGE2)                                            // two images side by side, whole tiles: Kp <= 32 of what is left
        return (pick_nsub(kp) == 1 && 2 * lds_bytes(c) <= (size_t)LDS_BUDGET) ? Fam::generic : Fam::none;      // (Kp > 64: one image is 128 KB)
    if (kp <= 32 && V == 0) return Fam::narrow;                  // the plain variant only
    if (kp == 96 || kp == 100) return Fam::k100;
    return Fam::generic;      // Kp <= 32 with weights / row-side s, Kp = 68, 80, 84, 112 .. 256
}
// The two-lane families run one 512-thread work-group per work item: a whole row block, or one gene range of a split one
// (k100::row_item: any oriana_row_split, the last-round form with explicit edges included).  The others take a grid of
// (work-groups of the row blocks, parts): whole-grid splits only, cut evenly by the kernel.
static constexpr bool takes_row_items(Fam f) { return f == Fam::k64 || f == Fam::k100; }
static constexpr int row_groups_per_block(Fam f, int G) { return f == Fam::generic ? TILE / (16 * (64 / G)) : 1; }

static constexpr Fam col_family(KCfg c, Col mode) {
    const int kp = c.kp();
    if (mode == Col::dual)                                       // two plain images of a four-lane configuration: Kp <= 64
        return (c.G == 4 && c.T4 != 6 && 2 * lds_bytes(c) <= (size_t)LDS_BUDGET) ? Fam::col2 : Fam::none;
    // (33 <= Kp <= 64: the two-lane dual kernel k64::k_col_pass_k64<KP4, true> measured 11.3 ms against 10.9 ms for the four-lane
    //  one at configs[4] -- with two images per step the walk is bound by the LDS return port either way; it is not dispatched)
    // (narrow up to Kp = 20 only: at Kp = 32 the two-tile kernel measured 26.0 us against 28.3 at 10,000 x 2,000)
    if (kp <= 20) return mode == Col::plain ? Fam::narrow : Fam::generic;      // (the narrow kernel writes no partials)
    if (c.G != 4) return Fam::generic;                           // Kp >= 128
    return (kp >= 36 && kp <= 64) ? Fam::k64 : Fam::col2;
}
// column tiles per work item (and per grid.x index) of the plain and the partials form; a dual item is one tile
static constexpr int col_tiles_per_item(KCfg c) {
    const Fam f = col_family(c, Col::plain);
    return (f == Fam::k64 || f == Fam::col2) ? 2 : 1;
}

// ORIANA_DEN_THRESHOLD=fixed: the row kernels keep the constant DEN_MIN (round 3's rule; A/B runs)
static bool den_threshold_dynamic() {
    static const bool fixed = [] { const char *e = getenv("ORIANA_DEN_THRESHOLD"); return e && !strcmp(e, "fixed"); }();
    return !fixed;
}

template <int G, int T4, int TAIL, int V>
static int launch_row_pass(const oriana_counts *cm, const float *FU, const float *FV, const float *w_nz, float *R,
                           float *s_cs, float *sw_cs, float *s_rs, int32_t *tile_flag, hipStream_t s,
                           const float *FV2, const oriana_row_split &sp, const float *den_min) {
    constexpr KCfg c{G, T4, TAIL};
    constexpr Fam F = row_family(c, V);
    constexpr int KP = c.kp();
    // one item per full row block, then the parts of the split ones
    const int64_t items = (int64_t)sp.nfull + (cm->nrb - sp.nfull) * sp.parts;
    if (items > 0x7fffffffLL) return ORIANA_EINVAL;
    if constexpr (F == Fam::none) {
        return ORIANA_EKRANGE;
    } else if constexpr (F == Fam::k64) {
        return launch(k64::k_row_pass_k64<KP / 4, V>, dim3((unsigned)items), dim3(512), (size_t)k64::IMG4 * 16 * ((V & V_IMAGE2) ? 2 : 1), s,
                      *cm, FU, FV, w_nz, R, s_cs, sw_cs, s_rs, tile_flag, FV2, sp, den_min);
    } else if constexpr (F == Fam::k100) {
        return launch(k100::k_row_pass_k100<TAIL, V>, dim3((unsigned)items), dim3(512), (size_t)k100::image_bytes(TAIL), s,
                      *cm, FU, FV, w_nz, R, s_cs, sw_cs, s_rs, tile_flag, sp, den_min);
    } else {
        static_assert(!takes_row_items(F) && row_groups_per_block(F, G) == (F == Fam::generic ? WaveGeo<G>::SPLIT : 1), "");
        if (!(sp.nfull == 0 || sp.parts == 1)) return ORIANA_EINVAL;
        const dim3 grid((unsigned)(cm->nrb * row_groups_per_block(F, G)), (unsigned)sp.parts);
        if constexpr (F == Fam::narrow)
            return launch(narrow::k_row_pass_narrow<KP>, grid, dim3(256), narrow::Geo<KP>::bytes(), s, *cm, FU, FV, R, s_cs, tile_flag, den_min);
        else
            return launch(k_row_pass<G, T4, TAIL, V>, grid, dim3(1024), lds_bytes(c) * ((V & V_IMAGE2) ? 2 : 1), s,
                          *cm, FU, FV, w_nz, R, s_cs, sw_cs, s_rs, tile_flag, FV2, den_min);
    }
}

template <int G, int T4, int TAIL>
static int launch_row_spmm(const oriana_counts *cm, const float *s_rs, const float *w_nz, const float *FV,
                           float *R, hipStream_t s) {
    return with_variant<0, 1>(w_nz ? 1 : 0, [&](auto HASW) {
        return launch(k_row_spmm<G, T4, TAIL, decltype(HASW)::value != 0>, dim3((unsigned)(cm->nrb * WaveGeo<G>::SPLIT)), dim3(1024),
                      lds_bytes(KCfg{G, T4, TAIL}), s, *cm, s_rs, w_nz, FV, R, (const uint8_t *)nullptr);
    });
}

// the same grid with the skipping mode compiled in (active != NULL)
template <int G, int T4, int TAIL>
static int launch_row_spmm_active(const oriana_counts *cm, const float *s_rs, const float *w_nz, const float *FV,
                                  float *R, const uint8_t *active, hipStream_t s) {
    return with_variant<0, 1>(w_nz ? 1 : 0, [&](auto HASW) {
        return launch(k_row_spmm<G, T4, TAIL, decltype(HASW)::value != 0, true>, dim3((unsigned)(cm->nrb * WaveGeo<G>::SPLIT)),
                      dim3(1024), lds_bytes(KCfg{G, T4, TAIL}), s, *cm, s_rs, w_nz, FV, R, active);
    });
}

// Grid of the column pass without a work list: (col_groups, row bands), enough bands to fill the chip (~target work-groups)
// without shrinking a band below min_band row blocks.
struct Bands { int64_t nb, per; };
static Bands band_grid(const oriana_counts *cm, int64_t col_groups, int64_t target, int64_t min_band) {
    int64_t nb = (target + col_groups - 1) / col_groups;
    const int64_t maxb = (cm->nrb + min_band - 1) / min_band;
    if (nb > maxb) nb = maxb;
    if (nb < 1) nb = 1;
    if (nb > 65535) nb = 65535;
    const int64_t per = (cm->nrb + nb - 1) / nb;
    return {(cm->nrb + per - 1) / per, per};
}

// work items (work != NULL: nwork triples of width col_tiles_per_item, or width 1 for the dual form) or a band grid
template <int G, int T4, int TAIL, Col MODE>
static int launch_col_pass(const oriana_counts *cm, const float *s_cs, const float *Gm, float *C, const int32_t *work,
                           int64_t nwork, float *Cpart, const float *Gm2, float *C2, hipStream_t s) {
    constexpr KCfg c{G, T4, TAIL};
    constexpr Fam F = col_family(c, MODE);
    if constexpr (F == Fam::none) {
        return ORIANA_EKRANGE;
    } else {
        static_assert(MODE == Col::dual || col_tiles_per_item(c) == ((F == Fam::k64 || F == Fam::col2) ? 2 : 1), "plain and partials share work lists");
        if (work && nwork <= 0) return 0;
        constexpr int KP = c.kp();
        constexpr int SPLIT = F == Fam::generic ? WaveGeo<G>::SPLIT : 1;        // work-groups per item
        dim3 grid((unsigned)(nwork * SPLIT));
        int64_t per = 0;
        if (!work) {
            const int64_t col_groups = (cm->ncb + col_tiles_per_item(c) - 1) / col_tiles_per_item(c) * SPLIT;
            const Bands b = F == Fam::narrow ? band_grid(cm, col_groups, 2048, 4) : band_grid(cm, col_groups, 1024, 8);
            grid = dim3((unsigned)col_groups, (unsigned)b.nb);
            per = b.per;
        }
        if constexpr (F == Fam::narrow) {
            return launch(narrow::k_col_pass_narrow<KP>, grid, dim3(256), narrow::Geo<KP>::bytes(), s, *cm, s_cs, Gm, C, work, per);
        } else if constexpr (F == Fam::k64) {
            return launch(k64::k_col_pass_k64<KP / 4, false>, grid, dim3(1024), (size_t)k64::IMG4 * 16, s,
                          *cm, s_cs, Gm, C, work, per, Cpart, nullptr, nullptr);
        } else if constexpr (F == Fam::col2) {
            constexpr bool DUAL = MODE == Col::dual;
            static_assert(!DUAL || 2 * ColImage<T4, TAIL>::bytes() <= (size_t)LDS_BUDGET, "");
            return launch(k_col_pass2<T4, TAIL, DUAL>, grid, dim3(1024), ColImage<T4, TAIL>::bytes() * (DUAL ? 2 : 1), s,
                          *cm, s_cs, Gm, C, work, per, Cpart, Gm2, C2);
        } else {
            return launch(k_col_pass<G, T4, TAIL>, grid, dim3(1024), lds_bytes(c), s, *cm, s_cs, Gm, C, work, per, Cpart);
        }
    }
}

}  // namespace oriana

using namespace oriana;

extern "C" int64_t oriana_kpad(int64_t K) {
    KCfg c;
    if (!pick_cfg(K, &c)) return 0;
    return c.kp();
}

extern "C" const char *oriana_version(void) { return "oriana_hip gfx950 0.5"; }

extern "C" int64_t oriana_col_block_tiles(int64_t K) {
    KCfg c;
    if (!pick_cfg(K, &c)) return 0;
    return col_tiles_per_item(c);
}

static bool counts_ok(const oriana_counts *cm) {
    if (!cm || cm->n < 0 || cm->m < 0) return false;
    if (cm->nrb != (cm->n + TILE - 1) / TILE || cm->ncb != (cm->m + TILE - 1) / TILE) return false;
    if (cm->nrb * cm->ncb > 0 && (!cm->roff || !cm->coff || !cm->rslice || !cm->cslice)) return false;
    if (cm->rslots > 0 && !cm->rowrec) return false;
    if (cm->cslots > 0 && !cm->ridx) return false;
    return true;
}

extern "C" int oriana_factor_prep(float *F, float *mu, const float *logF, const float *mask,
                                  const int32_t *row_index, int64_t r, int64_t K, void *stream) {
    const int64_t Kp = oriana_kpad(K);
    if (r < 0 || K <= 0) return ORIANA_EINVAL;
    if (Kp == 0) return ORIANA_EKRANGE;
    if (r == 0) return 0;
    if (!F || !logF) return ORIANA_EINVAL;
    hipLaunchKernelGGL(k_factor_prep, dim3((unsigned)((r + 3) / 4)), dim3(256), 0, (hipStream_t)stream, F, mu,
                       logF, mask, row_index, r, (int)K, (int)Kp);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t oriana_prep_center_offset(void) { return ((int64_t)sizeof(float) * (STATS_PART0 + 4 * 2 * STATS_MAX_BLOCKS) + 7) / 8 * 8; }
extern "C" int64_t oriana_prep_den_threshold_offset(void) { return 7 * (int64_t)sizeof(float); }
extern "C" int64_t oriana_prep_scratch_bytes(void) { return oriana_prep_center_offset() + 4096; }

static int factor_prep_pair_impl(float *FU, float *FV, const float *logU, const float *logV, const float *maskV,
                                 const int32_t *row_index_u, const int32_t *row_index_v, int64_t n, int64_t m,
                                 int64_t K, float *scratch, const oriana_clear_list *clr, const float *mu_u,
                                 const float *upart, int64_t nupart, void *stream) {
    const int64_t Kp = oriana_kpad(K);
    const bool fused = mu_u != nullptr;
    if (n < 0 || m < 0 || K <= 0) return ORIANA_EINVAL;
    if (Kp == 0) return ORIANA_EKRANGE;
    oriana_clear_list cl;
    memset(&cl, 0, sizeof(cl));
    int64_t clear_bytes = 0;
    if (clr) {
        cl = *clr;
        for (int e = 0; e < ORIANA_CLEAR_MAX; ++e) {
            if (cl.bytes[e] < 0 || (cl.bytes[e] & 3) || (cl.bytes[e] > 0 && (!cl.ptr[e] || ((uintptr_t)cl.ptr[e] & 3)))) return ORIANA_EINVAL;
            clear_bytes += cl.bytes[e];
        }
    }
    if (n == 0 && m == 0 && clear_bytes == 0) return 0;
    if ((n > 0 && (!FU || (!fused && !logU))) || (m > 0 && (!FV || !logV)) || !scratch) return ORIANA_EINVAL;
    if (fused && (!upart || nupart <= 0 || nupart > 0x7fffffffLL || n <= 0)) return ORIANA_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    // (one work-group per 64 rows, at most STATS_MAX_BLOCKS per side: every group ends with an agent-scope
    //  release / acquire pair, which on a small matrix costs more than the rows it covers)
    const int lane_rows = K <= 32 ? 1 : 0;
    const int64_t rows_per_group = lane_rows ? 256 : 64;
    auto capped = [&](int64_t r) { const int64_t b = (r + rows_per_group - 1) / rows_per_group; return (int)(b < STATS_MAX_BLOCKS ? b : STATS_MAX_BLOCKS); };
    const int sbu = fused ? 0 : capped(n);
    const int sbv = (fused && m == 0) ? 1 : capped(m);      // (fused: some group has to combine the cell side's partials)
    if (sbu + sbv > 0)
        hipLaunchKernelGGL(k_row_stats, dim3((unsigned)(sbu + sbv)), dim3(256), 0, s, scratch, logU, n, logV, maskV, m, (int)K, sbu,
                           lane_rows, den_threshold_dynamic() ? 1 : 0, fused ? upart : (const float *)nullptr, (int)nupart);
    const int64_t nbu = fused ? (n + 255) / 256 : (n + 3) / 4, nbv = (m + 3) / 4;
    // zero-fill groups: 16 KB each, at most 4096
    int64_t ncl = (clear_bytes + 16383) / 16384;
    if (ncl > 4096) ncl = 4096;
    if (nbu + nbv + ncl > 0x7fffffffLL) return ORIANA_EINVAL;
    hipLaunchKernelGGL(k_factor_prep_pair, dim3((unsigned)(nbu + nbv + ncl)), dim3(256), 0, s, FU, FV, logU, logV, maskV,
                       row_index_u, row_index_v, n, m, (int)K, (int)Kp, (int)nbu, (int)nbv, (const float *)scratch, cl, mu_u);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_factor_prep_pair_clear(float *FU, float *FV, const float *logU, const float *logV, const float *maskV,
                                             const int32_t *row_index_u, const int32_t *row_index_v, int64_t n, int64_t m,
                                             int64_t K, float *scratch, const oriana_clear_list *clr, void *stream) {
    return factor_prep_pair_impl(FU, FV, logU, logV, maskV, row_index_u, row_index_v, n, m, K, scratch, clr, nullptr, nullptr, 0, stream);
}

extern "C" int oriana_factor_prep_pair_fused(float *FU, const float *mu_u, const float *upart, int64_t nupart, float *FV,
                                             const float *logV, const float *maskV, const int32_t *row_index_v, int64_t n,
                                             int64_t m, int64_t K, float *scratch, const oriana_clear_list *clr, void *stream) {
    if (!mu_u) return ORIANA_EINVAL;
    return factor_prep_pair_impl(FU, FV, nullptr, logV, maskV, nullptr, row_index_v, n, m, K, scratch, clr, mu_u, upart, nupart, stream);
}

extern "C" int oriana_factor_prep_pair(float *FU, float *FV, const float *logU, const float *logV, const float *maskV,
                                       const int32_t *row_index_u, const int32_t *row_index_v, int64_t n, int64_t m,
                                       int64_t K, float *scratch, void *stream) {
    return oriana_factor_prep_pair_clear(FU, FV, logU, logV, maskV, row_index_u, row_index_v, n, m, K, scratch, nullptr, stream);
}

static oriana_row_split no_split(const oriana_counts *cm) {
    oriana_row_split sp = {};
    sp.nfull = (int32_t)cm->nrb; sp.parts = 1; sp.edge[0] = 0; sp.edge[1] = (int32_t)cm->ncb;
    return sp;
}
// oriana_row_pass_split: every row block in gene_splits even ranges (a count split_ok rejects stays rejected as parts = 0)
static oriana_row_split even_split(int64_t gene_splits) {
    oriana_row_split sp = {};
    sp.nfull = 0; sp.parts = (gene_splits < 1 || gene_splits > 65535) ? 0 : (int32_t)gene_splits; sp.edge[0] = -1;
    return sp;
}
static bool split_ok(const oriana_counts *cm, const oriana_row_split &sp) {
    if (sp.nfull < 0 || sp.nfull > cm->nrb || sp.parts < 1 || sp.parts > 65535) return false;
    if (cm->ncb > 0 && sp.parts > cm->ncb) return false;
    if (sp.edge[0] < 0) return true;
    if (sp.parts > 8 || sp.edge[0] != 0 || sp.edge[sp.parts] != cm->ncb) return false;
    for (int e = 0; e < sp.parts; ++e)
        if (sp.edge[e + 1] < sp.edge[e]) return false;
    return true;
}

extern "C" int oriana_row_pass(const oriana_counts *cm, const float *FU, const float *FV, const float *w_nz,
                               float *R, float *s_cs, float *sw_cs, float *s_rs, int32_t *tile_flag, int64_t K,
                               void *stream) {
    return oriana_row_pass_general(cm, FU, FV, nullptr, w_nz, R, s_cs, sw_cs, s_rs, tile_flag, K, nullptr, nullptr, stream);
}

// Gene-tile split of the plain row pass for short matrices: a row block is one work-group (two or four for K > 112), so a
// matrix of 10,000 cells runs the pass on 40 of the 256 CUs; splitting each row block's gene tiles over several groups
// fills the chip; each group of a row block stores its row sums in its own slab of R, which the consumer adds up
// (atomics on R cost 1.2 us per split at 10,000 x 20: more than the tile a split saves).
extern "C" int oriana_row_pass_plan_cus(const oriana_counts *cm, int64_t K, const double *tile_cost, int64_t cus, oriana_row_split *out) {
    if (cus <= 0) return ORIANA_EINVAL;
    if (!cm || !out || cm->nrb < 0 || cm->nrb > 0x7fffffffLL || cm->ncb > 0x7fffffffLL) return ORIANA_EINVAL;
    *out = no_split(cm);
    KCfg cfg;
    if (!pick_cfg(K, &cfg) || cm->nrb <= 0 || cm->ncb <= 1) return 0;
    const Fam fam = row_family(cfg, 0);             // (the plan is the plain variant's; the two-lane families serve every variant)
    const bool two_lane = takes_row_items(fam);
    const int64_t groups = cm->nrb * row_groups_per_block(fam, cfg.G);
    int64_t nfull = 0, parts = 1;
    if (groups < cus) {
        // short matrices: two work-groups per CU at most, evenly sized ranges (measured at 10,000 x 2,000, K = 20:
        // 77 / 42 / 25 / 24 us for 1 / 2 / 4 / 8 groups per row block; 8 is the better sweep)
        parts = 2 * cus / groups;
    } else if (two_lane) {
        // One 512-thread group per CU (the image and the registers leave room for one): the pass advances in rounds of `cus`
        // (256 on the MI355X the figures are from) row blocks and a partly filled last round costs a whole one (1M x 30k, K = 100: 3840 / 3907 / 4096 row blocks =
        // 33.9 / 35.8 / 36.2 ms; 391 row blocks -- configs[2] -- run as two rounds).  The row blocks of the last round are
        // split into p gene ranges each: ceil(tail * p / 256) / p rounds instead of one, + 1 % per extra range; a finer
        // split has to earn 3 %.
        const int64_t tail = cm->nrb % cus;
        if (tail == 0) return 0;
        double best = 1.0;
        int64_t bp = 1;
        for (int64_t p2 = 2; p2 <= 8 && p2 <= cm->ncb; ++p2) {
            const double c = (double)((tail * p2 + cus - 1) / cus) / (double)p2 + 0.01 * (double)(p2 - 1);
            if (c < 0.97 * best) { best = c; bp = p2; }
        }
        if (bp == 1) return 0;
        nfull = cm->nrb - tail; parts = bp;
    } else {
        return 0;
    }
    if (parts > cm->ncb) parts = cm->ncb;
    if (parts <= 1) return 0;
    {   // whole tiles per range: fewer parts if the tiles do not go round
        const int64_t per = (cm->ncb + parts - 1) / parts;
        parts = (cm->ncb + per - 1) / per;
    }
    out->nfull = (int32_t)nfull; out->parts = (int32_t)parts;
    if (!two_lane || parts > 8) { out->edge[0] = -1; return 0; }       // evenly cut (gridDim.y kernels / many short ranges)
    // equal-cost cut points (genes are packed by decreasing density: the first tiles are the long ones)
    double total = 0.0;
    for (int64_t c = 0; c < cm->ncb; ++c) total += tile_cost ? (tile_cost[c] > 0.0 ? tile_cost[c] : 0.0) : 1.0;
    if (!(total > 0.0)) { out->edge[0] = -1; return 0; }
    out->edge[0] = 0;
    double cum = 0.0;
    int64_t c = 0;
    for (int64_t e = 1; e < parts; ++e) {
        const double want = total * (double)e / (double)parts;
        while (c < cm->ncb) {
            const double w = tile_cost ? (tile_cost[c] > 0.0 ? tile_cost[c] : 0.0) : 1.0;
            if (cum + 0.5 * w > want) break;
            cum += w; ++c;
        }
        // every range keeps at least one tile
        const int64_t lo = out->edge[e - 1] + 1, hi = cm->ncb - (parts - e);
        int64_t edge = c < lo ? lo : (c > hi ? hi : c);
        while (c < edge) { cum += tile_cost ? (tile_cost[c] > 0.0 ? tile_cost[c] : 0.0) : 1.0; ++c; }
        out->edge[e] = (int32_t)edge;
    }
    out->edge[parts] = (int32_t)cm->ncb;
    return 0;
}

// [r5] ... for the device the calling thread has selected (oriana_device_cus: multiProcessorCount, not a literal 256)
extern "C" int oriana_row_pass_plan(const oriana_counts *cm, int64_t K, const double *tile_cost, oriana_row_split *out) {
    return oriana_row_pass_plan_cus(cm, K, tile_cost, oriana_device_cus(), out);
}

extern "C" int oriana_row_pass_split(const oriana_counts *cm, const float *FU, const float *FV, float *R, float *s_cs,
                                     int32_t *tile_flag, int64_t K, int64_t gene_splits, void *stream) {
    const oriana_row_split sp = even_split(gene_splits);
    return oriana_row_pass_general(cm, FU, FV, nullptr, nullptr, R, s_cs, nullptr, nullptr, tile_flag, K, &sp, nullptr, stream);
}

// The row pass in full generality: the plain pass, or (FV2 given) the sparse models' two-image form, with the gene tiles of a
// row block split over work-groups (split; NULL = none), each storing its row sums in its own slab of R.  The one place the
// arguments of a row pass are validated: oriana_row_pass and oriana_row_pass_split forward here.
extern "C" int oriana_row_pass_general(const oriana_counts *cm, const float *FU, const float *FV, const float *FV2,
                                       const float *w_nz, float *R, float *s_cs, float *sw_cs, float *s_rs,
                                       int32_t *tile_flag, int64_t K, const oriana_row_split *split, const float *den_min,
                                       void *stream) {
    if (!counts_ok(cm) || K <= 0) return ORIANA_EINVAL;
    KCfg cfg;
    if (!pick_cfg(K, &cfg)) return ORIANA_EKRANGE;
    if (cm->n == 0) return 0;
    if (!FU || !R || (cm->m > 0 && !FV) || (cm->m > 0 && (!s_cs || !tile_flag))) return ORIANA_EINVAL;
    if ((w_nz != nullptr) != (sw_cs != nullptr) || (FV2 && s_rs)) return ORIANA_EINVAL;
    const oriana_row_split sp = split ? *split : no_split(cm);
    if (!split_ok(cm, sp)) return ORIANA_EINVAL;
    if (cm->m == 0) FV2 = nullptr;
    hipStream_t s = (hipStream_t)stream;
    const int var = (s_rs ? V_SROW : 0) | (w_nz ? V_WEIGHTS : 0) | (FV2 ? V_IMAGE2 : 0);
#define CALL(G, T, L)                                                                                                      \
    return with_variant<0, 1, 2, 3, 4, 6>(var, [&](auto V) {                                                               \
        return launch_row_pass<G, T, L, decltype(V)::value>(cm, FU, FV, w_nz, R, s_cs, sw_cs, s_rs, tile_flag, s, FV2, sp, den_min); \
    })
    ORIANA_FOR_CFG(cfg, CALL);
#undef CALL
}

extern "C" int oriana_row_spmm(const oriana_counts *cm, const float *s_rs, const float *w_nz, const float *FV,
                               float *R, int64_t K, void *stream) {
    if (!counts_ok(cm) || K <= 0) return ORIANA_EINVAL;
    KCfg cfg;
    if (!pick_cfg(K, &cfg)) return ORIANA_EKRANGE;
    if (cm->n == 0) return 0;
    if (!R || (cm->m > 0 && !FV) || (cm->rslots > 0 && !s_rs)) return ORIANA_EINVAL;
    hipStream_t s = (hipStream_t)stream;
#define CALL(G, T, L) return launch_row_spmm<G, T, L>(cm, s_rs, w_nz, FV, R, s)
    ORIANA_FOR_CFG(cfg, CALL);
#undef CALL
}

extern "C" int oriana_row_spmm_active(const oriana_counts *cm, const float *s_rs, const float *w_nz, const float *FV,
                                      float *R, const uint8_t *active, int64_t K, void *stream) {
    if (!active) return oriana_row_spmm(cm, s_rs, w_nz, FV, R, K, stream);
    if (!counts_ok(cm) || K <= 0) return ORIANA_EINVAL;
    KCfg cfg;
    if (!pick_cfg(K, &cfg)) return ORIANA_EKRANGE;
    if (cm->n == 0) return 0;
    if (!R || (cm->m > 0 && !FV) || (cm->rslots > 0 && !s_rs)) return ORIANA_EINVAL;
    hipStream_t s = (hipStream_t)stream;
#define CALL(G, T, L) return launch_row_spmm_active<G, T, L>(cm, s_rs, w_nz, FV, R, active, s)
    ORIANA_FOR_CFG(cfg, CALL);
#undef CALL
}

extern "C" int oriana_col_pass(const oriana_counts *cm, const float *s_cs, const float *Gm, float *C, int64_t K,
                               const int32_t *work, int64_t nwork, void *stream) {
    if (!counts_ok(cm) || K <= 0) return ORIANA_EINVAL;
    KCfg cfg;
    if (!pick_cfg(K, &cfg)) return ORIANA_EKRANGE;
    if (cm->n == 0 || cm->m == 0) return 0;
    if (!Gm || !C || !s_cs) return ORIANA_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (nwork < 0 || (work == nullptr && nwork != 0)) return ORIANA_EINVAL;
#define CALL(G, T, L) return launch_col_pass<G, T, L, Col::plain>(cm, s_cs, Gm, C, work, nwork, nullptr, nullptr, nullptr, s)
    ORIANA_FOR_CFG(cfg, CALL);
#undef CALL
}

// [r6] ANALYSIS entry (tools/parity_report.py): the column pass with float64 accumulators in a fixed
// order -- one thread per gene and group of 8 factors walks the gene's slots through every row block -- and ONE rounding to
// float32 at the end: C += f32(sum_i s_ij G_i).  What a compensated (Kahan / two-float) accumulation of the float32 kernels
// could reach at most; no kernel of a sweep calls it.
__global__ __launch_bounds__(256) void k_col_pass_f64acc(oriana_counts cm, const float *__restrict__ s_cs,
                                                         const float *__restrict__ Gm, float *__restrict__ C, int K, int Kp) {
    const int c = threadIdx.x, sl = c >> 4;
    const int64_t cb = blockIdx.x, col = cb * TILE + c;
    const int k0 = blockIdx.y * 8;
    if (col >= cm.m) return;
    double acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0;
    for (int64_t rb = 0; rb < cm.nrb; ++rb) {
        const int64_t t = rb * cm.ncb + cb;
        const uint32_t s0 = cm.cslice[t * 17 + sl], s1 = cm.cslice[t * 17 + sl + 1];
        const int ni = (int)((s1 - s0) >> 6);
        const int64_t base = cm.coff[t] + s0 + (c & 15) * 4;
        for (int it = 0; it < ni; ++it)
            for (int r = 0; r < 4; ++r) {
                const float sv = s_cs[base + (int64_t)it * 64 + r];
                if (sv == 0.f) continue;
                const int64_t row = rb * TILE + cm.ridx[base + (int64_t)it * 64 + r];
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (k0 + e < K) acc[e] += (double)sv * (double)Gm[row * Kp + k0 + e];
            }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (k0 + e < K) C[col * Kp + k0 + e] += (float)acc[e];
}

extern "C" int oriana_col_pass_f64acc(const oriana_counts *cm, const float *s_cs, const float *Gm, float *C, int64_t K,
                                      void *stream) {
    if (!counts_ok(cm) || K <= 0) return ORIANA_EINVAL;
    const int64_t Kp = oriana_kpad(K);
    if (Kp == 0) return ORIANA_EKRANGE;
    if (cm->n == 0 || cm->m == 0) return 0;
    if (!Gm || !C || !s_cs) return ORIANA_EINVAL;
    hipLaunchKernelGGL(k_col_pass_f64acc, dim3((unsigned)cm->ncb, (unsigned)((K + 7) / 8)), dim3(256), 0, (hipStream_t)stream, *cm,
                       s_cs, Gm, C, (int)K, (int)Kp);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

// two images, one column tile per work item (work list of width 1)
extern "C" int oriana_col_pass_dual(const oriana_counts *cm, const float *s_cs, const float *G1, const float *G2,
                                    float *C1, float *C2, int64_t K, const int32_t *work, int64_t nwork, void *stream) {
    if (!counts_ok(cm) || K <= 0) return ORIANA_EINVAL;
    KCfg cfg;
    if (!pick_cfg(K, &cfg)) return ORIANA_EKRANGE;
    if (cm->n == 0 || cm->m == 0) return 0;
    if (!G1 || !G2 || !C1 || !C2 || !s_cs || !work || nwork < 0) return ORIANA_EINVAL;
    hipStream_t s = (hipStream_t)stream;
#define CALL(G, T, L) return launch_col_pass<G, T, L, Col::dual>(cm, s_cs, G1, C1, work, nwork, nullptr, G2, C2, s)
    ORIANA_FOR_CFG(cfg, CALL);
#undef CALL
}

static int col_pass_partials(const oriana_counts *cm, const float *s_cs, const float *Gm, float *C, int64_t K,
                             const int32_t *work, int64_t nwork, float *scratch, hipStream_t s) {
    KCfg cfg;
    if (!pick_cfg(K, &cfg)) return ORIANA_EKRANGE;
#define CALL(G, T, L) return launch_col_pass<G, T, L, Col::partials>(cm, s_cs, Gm, C, work, nwork, scratch, nullptr, nullptr, s)
    ORIANA_FOR_CFG(cfg, CALL);
#undef CALL
}

extern "C" int64_t oriana_col_pass_det_scratch_bytes(int64_t K, int64_t nwork) {
    const int64_t Kp = oriana_kpad(K), w = oriana_col_block_tiles(K);
    if (Kp == 0 || nwork < 0) return 0;
    return nwork * w * TILE * Kp * (int64_t)sizeof(float);
}

extern "C" int oriana_col_pass_det(const oriana_counts *cm, const float *s_cs, const float *Gm, float *C, int64_t K,
                                   const int32_t *work, int64_t nwork, float *scratch, void *stream) {
    if (!counts_ok(cm) || K <= 0) return ORIANA_EINVAL;
    if (cm->n == 0 || cm->m == 0 || nwork == 0) return 0;
    if (!Gm || !C || !s_cs || !work || nwork < 0 || !scratch) return ORIANA_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    // every (item, column, factor) slot of the scratch is written by exactly one lane of the item that owns it, except
    // the columns past m and the padding lanes of partial column blocks: clear it first
    ORIANA_HIP_CHECK(hipMemsetAsync(scratch, 0, (size_t)oriana_col_pass_det_scratch_bytes(K, nwork), s));
    int rc = col_pass_partials(cm, s_cs, Gm, C, K, work, nwork, scratch, s);
    if (rc) return rc;
    const int64_t w = oriana_col_block_tiles(K);
    const int64_t nblk = (cm->ncb + w - 1) / w;
    hipLaunchKernelGGL(k_col_reduce, dim3((unsigned)nblk), dim3(256), 0, s, C, scratch, work, nwork, cm->m,
                       (int)oriana_kpad(K), (int)w);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_finalize(float *Z, const float *F, const float *R, const float *mul,
                               const int32_t *row_index, int64_t r, int64_t K, int accumulate, void *stream) {
    const int64_t Kp = oriana_kpad(K);
    if (r < 0 || K <= 0) return ORIANA_EINVAL;
    if (Kp == 0) return ORIANA_EKRANGE;
    if (r == 0) return 0;
    if (!Z || !F || !R) return ORIANA_EINVAL;
    const int64_t tot = r * K;
    hipLaunchKernelGGL(k_finalize, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Z, F, R,
                       mul, row_index, r, (int)K, (int)Kp, accumulate, 1, (int64_t)0);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_finalize_slabs_from(float *Z, const float *F, const float *R, int64_t nslab, int64_t slab_row0,
                                          const int32_t *row_index, int64_t r, int64_t K, void *stream) {
    const int64_t Kp = oriana_kpad(K);
    if (r < 0 || K <= 0 || nslab < 1 || nslab > 65535 || slab_row0 < 0) return ORIANA_EINVAL;
    if (Kp == 0) return ORIANA_EKRANGE;
    if (r == 0) return 0;
    if (!Z || !F || !R) return ORIANA_EINVAL;
    const int64_t tot = r * K;
    hipLaunchKernelGGL(k_finalize, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Z, F, R,
                       (const float *)nullptr, row_index, r, (int)K, (int)Kp, 1, (int)nslab, slab_row0);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_finalize_slabs(float *Z, const float *F, const float *R, int64_t nslab, const int32_t *row_index,
                                     int64_t r, int64_t K, void *stream) {
    return oriana_finalize_slabs_from(Z, F, R, nslab, 0, row_index, r, K, stream);
}

extern "C" int oriana_fixup(const oriana_counts *cm, const int32_t *tile_flag, float *s_cs, float *sw_cs,
                            float *s_rs, const float *logU, const float *logV, const float *S_tilde,
                            const float *S_hat, const float *w_nz, const float *dq, float *Zi, float *Zj,
                            float *Zlog, int64_t K, int variant, void *stream) {
    if (!counts_ok(cm) || K <= 0) return ORIANA_EINVAL;
    const int64_t nt = cm->nrb * cm->ncb;
    if (nt == 0 || cm->nnz == 0) return 0;
    if (!tile_flag || !s_cs || !logU || !logV) return ORIANA_EINVAL;
    const int quirk = ((variant & 4) ? 1 : 0) | ((variant & 8) ? 2 : 0);       // bit 1: Z_hat_j indexed by the packed gene
    // (K <= number of genes is the caller's to check: cm->m of the sliced part of a hybrid layout counts its own genes only)
    if ((quirk & 1) && !dq) return ORIANA_EQUIRK;
    const int per = (int)(nt / 2048 < 1 ? 1 : (nt / 2048 > 64 ? 64 : nt / 2048));       // tiles per work-group (k_fixup)
    hipLaunchKernelGGL(k_fixup, dim3((unsigned)((nt + per - 1) / per)), dim3(256), 0, (hipStream_t)stream, *cm, tile_flag, s_cs,
                       sw_cs, s_rs, logU, logV, S_tilde, S_hat, w_nz, dq, Zi, Zj, Zlog, (int)K, quirk, nt, per);
    ORIANA_LAUNCH_CHECK();
    return 0;
}
