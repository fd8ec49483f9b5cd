// stateless.hip -- drop-ins with the reference's exact kernel signatures (outputs first, inputs
// after, dense float32 matrices, callee zero-fills, gap.py:67-80 and twins).  X is repacked on
// every call, as the reference re-casts X on every call (gap.py:94); the model classes keep the
// packed layout resident instead and call the passes directly.
#include "pack_nest.h"

namespace oriana {

struct WsLayout {
    int64_t nt, Kp;
    size_t tile_nnz, tile_rslots, tile_cslots, roff, coff, rslice, cslice, tile_flag, totals, rowrec, ridx, s_cs,
        FU, FV, R, C, w_nz, sw_cs, s_rs, F2, G2, C2, dq, prep, total;
};

static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// rslot_cap / cslot_cap: capacities of the row-side / column-side slot arrays
static WsLayout ws_layout(int64_t n, int64_t m, int64_t K, int64_t rslot_cap, int64_t cslot_cap) {
    WsLayout L;
    const int64_t nrb = (n + TILE - 1) / TILE, ncb = (m + TILE - 1) / TILE;
    L.nt = nrb * ncb;
    L.Kp = oriana_kpad(K);
    size_t o = 0;
    const int64_t nt1 = L.nt > 0 ? L.nt : 1;
    const int64_t rs1 = rslot_cap > 0 ? rslot_cap : 1, cs1 = cslot_cap > 0 ? cslot_cap : 1;
    const int64_t n1 = n > 0 ? n : 1, m1 = m > 0 ? m : 1;
    L.tile_nnz = o;    o = align256(o + sizeof(int32_t) * nt1);
    L.tile_rslots = o; o = align256(o + sizeof(int32_t) * nt1);
    L.tile_cslots = o; o = align256(o + sizeof(int32_t) * nt1);
    L.roff = o;        o = align256(o + sizeof(int64_t) * (nt1 + 1));
    L.coff = o;        o = align256(o + sizeof(int64_t) * (nt1 + 1));
    L.rslice = o;      o = align256(o + sizeof(uint32_t) * nt1 * 17);
    L.cslice = o;      o = align256(o + sizeof(uint32_t) * nt1 * 17);
    L.tile_flag = o;   o = align256(o + sizeof(int32_t) * nt1);
    L.totals = o;      o = align256(o + sizeof(int64_t) * 4);
    L.rowrec = o;      o = align256(o + sizeof(oriana_rowrec) * rs1);
    L.ridx = o;        o = align256(o + cs1);
    L.s_cs = o;        o = align256(o + sizeof(float) * cs1);
    L.FU = o;          o = align256(o + sizeof(float) * n1 * L.Kp);
    L.FV = o;          o = align256(o + sizeof(float) * m1 * L.Kp);
    L.R = o;           o = align256(o + sizeof(float) * n1 * L.Kp);
    L.C = o;           o = align256(o + sizeof(float) * m1 * L.Kp);
    // extras of the ZI / sparse loop nests (always laid out: one workspace size serves the four entries)
    L.w_nz = o;        o = align256(o + sizeof(float) * rs1);
    L.sw_cs = o;       o = align256(o + sizeof(float) * cs1);
    L.s_rs = o;        o = align256(o + sizeof(float) * rs1);
    L.F2 = o;          o = align256(o + sizeof(float) * m1 * L.Kp);
    L.G2 = o;          o = align256(o + sizeof(float) * n1 * L.Kp);
    L.C2 = o;          o = align256(o + sizeof(float) * m1 * L.Kp);
    L.dq = o;          o = align256(o + sizeof(float) * n1 * (K > 0 ? K : 1));
    L.prep = o;        o = align256(o + (size_t)oriana_prep_scratch_bytes());
    L.total = o;
    return L;
}

// Slot capacities that are always sufficient for `nnz_bound` non-zeros: a slice iteration holds 64
// slots and is opened by at least one record, and each tile carries 64 dummy slots.
static inline int64_t slot_bound(int64_t nnz_bound) { return 64 * nnz_bound; }

}  // namespace oriana

using namespace oriana;

extern "C" int64_t oriana_zq_workspace_bytes(int64_t n, int64_t m, int64_t K, int64_t nnz_bound) {
    if (n < 0 || m < 0 || nnz_bound < 0 || oriana_kpad(K) == 0) return 0;
    const int64_t nt = ((n + TILE - 1) / TILE) * ((m + TILE - 1) / TILE);
    // worst case: every record alone in its slice iteration; capped by the dense tile capacity
    int64_t cap = slot_bound(nnz_bound);
    const int64_t dense = nt * 65536;
    if (cap > dense) cap = dense;
    return (int64_t)ws_layout(n, m, K, cap, cap + 64 * nt).total;
}

// The four loop nests on dense inputs.  Zlog / S_tilde / S_hat / D_hat may be NULL (absent in that
// variant); quirk = zigap.py:94 (per-gene sums weighted by D_hat[i, k]).  Packs X, then runs the nest (zq_nest.h).
static int zq_dense(float *Zi, float *Zj, float *Zlog, const float *log_U_hat, const float *log_V_hat,
                    const float *S_tilde, const float *S_hat, const float *D_hat, int quirk, const float *X,
                    int64_t n, int64_t m, int64_t K, void *ws, int64_t ws_bytes, void *stream) {
    if (n < 0 || m < 0 || K <= 0) return ORIANA_EINVAL;
    if (oriana_kpad(K) == 0) return ORIANA_EKRANGE;
    if ((S_tilde == nullptr) != (S_hat == nullptr)) return ORIANA_EINVAL;
    if (quirk && (!D_hat || K > m)) return ORIANA_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (n > 0 && (!Zi || !log_U_hat)) return ORIANA_EINVAL;
    if (m > 0 && (!Zj || !log_V_hat)) return ORIANA_EINVAL;
    // callee zero-fills the outputs (gap.py:69-70, zigap.py:82-84)
    if (n > 0) ORIANA_HIP_CHECK(hipMemsetAsync(Zi, 0, sizeof(float) * n * K, s));
    if (m > 0) ORIANA_HIP_CHECK(hipMemsetAsync(Zj, 0, sizeof(float) * m * K, s));
    if (m > 0 && Zlog) ORIANA_HIP_CHECK(hipMemsetAsync(Zlog, 0, sizeof(float) * m * K, s));
    if (n == 0 || m == 0) return 0;
    if (!X || !ws || ((uintptr_t)ws & 255)) return ORIANA_EINVAL;
    const bool sparse = S_hat != nullptr, weighted = D_hat != nullptr;
    // fixed-size part first: counts, offsets, slice tables
    const WsLayout L0 = ws_layout(n, m, K, 0, 0);
    if ((size_t)ws_bytes < L0.total) return ORIANA_EINVAL;
    char *b = (char *)ws;
    const PackTables t{(int32_t *)(b + L0.tile_nnz), (int32_t *)(b + L0.tile_rslots), (int32_t *)(b + L0.tile_cslots), (int64_t *)(b + L0.roff),
                       (int64_t *)(b + L0.coff), (uint32_t *)(b + L0.rslice), (uint32_t *)(b + L0.cslice)};
    // X packed as one chunk in the caller's gene order; the slot totals place the record arrays and what follows them in the workspace
    WsLayout L = L0;
    ZqView v;
    auto chunk = [&](int64_t, int64_t, bool, const float **Xc, int64_t *ld) -> int { *Xc = X; *ld = m; return 0; };
    auto place = [&](int64_t rslots, int64_t cslots, oriana_rowrec **rowrec, uint8_t **ridx, float **side_nz) -> int {
        L = ws_layout(n, m, K, rslots, cslots);
        if (L.total > (size_t)ws_bytes) return ORIANA_EINVAL;
        const int64_t rs1 = rslots > 0 ? rslots : 1, cs1 = cslots > 0 ? cslots : 1;
        *rowrec = (oriana_rowrec *)(b + L.rowrec); *ridx = (uint8_t *)(b + L.ridx);
        v.s_cs = (float *)(b + L.s_cs);
        // padding slots: x == 0 records, row index 0, s == 0
        ORIANA_HIP_CHECK(hipMemsetAsync(*rowrec, 0, sizeof(oriana_rowrec) * rs1, s));
        ORIANA_HIP_CHECK(hipMemsetAsync(*ridx, 0, cs1, s));
        ORIANA_HIP_CHECK(hipMemsetAsync(v.s_cs, 0, sizeof(float) * cs1, s));
        if (weighted) {
            v.w_nz = *side_nz = (float *)(b + L.w_nz); v.sw_cs = (float *)(b + L.sw_cs);
            ORIANA_HIP_CHECK(hipMemsetAsync(*side_nz, 0, sizeof(float) * rs1, s));
            ORIANA_HIP_CHECK(hipMemsetAsync(v.sw_cs, 0, sizeof(float) * cs1, s));
        }
        if (sparse) {
            v.s_rs = (float *)(b + L.s_rs);
            ORIANA_HIP_CHECK(hipMemsetAsync(v.s_rs, 0, sizeof(float) * rs1, s));
        }
        return 0;
    };
    oriana_counts cm;
    ORIANA_TRY(pack_sliced(&cm, n, m, n, t, nullptr, D_hat, m, 1, chunk, place, s));
    // the nest over the workspace: no dense block, no split, no work lists, no two-image kernels, the fixed den threshold;
    // the outputs are zeroed above, C / tile_flag / C2 by the preparation's clear list
    v.cm = &cm; v.n = n; v.m = m; v.K = K; v.Kp = L.Kp;
    v.FU = (float *)(b + L.FU); v.FV = (float *)(b + L.FV); v.R = (float *)(b + L.R); v.C = (float *)(b + L.C);
    v.prep = (float *)(b + L.prep); v.tile_flag = (int32_t *)(b + L0.tile_flag);
    v.F2 = (float *)(b + L.F2); v.G2 = v.GQ = (float *)(b + L.G2); v.C2 = (float *)(b + L.C2);
    if (quirk) {
        v.dq = (float *)(b + L.dq);
        ORIANA_TRY(oriana_take_cols_f32(v.dq, D_hat, n, m, K, stream));
    }
    ORIANA_HIP_CHECK(hipMemsetAsync(v.prep, 0, 8 * sizeof(float), s));            // the arrival counter
    return zq_run(v, Zi, Zj, Zlog, log_U_hat, log_V_hat, S_tilde, S_hat, nullptr, stream);
}

extern "C" int oriana_zq_gap_f32(float *Z_hat_i, float *Z_hat_j, const float *log_U_hat, const float *log_V_hat,
                                 const float *X, int64_t n, int64_t m, int64_t K, void *ws, int64_t ws_bytes,
                                 void *stream) {
    return zq_dense(Z_hat_i, Z_hat_j, nullptr, log_U_hat, log_V_hat, nullptr, nullptr, nullptr, 0, X, n, m, K, ws,
                    ws_bytes, stream);
}

extern "C" int oriana_zq_zigap_f32(float *DZ_hat_i, float *DZ_hat_j, float *DZ_exp_logsum_hat, const float *log_U_hat,
                                   const float *log_V_hat, const float *D_hat, const float *X, int64_t n, int64_t m,
                                   int64_t K, int reference_quirks, void *ws, int64_t ws_bytes, void *stream) {
    if (!D_hat && n > 0 && m > 0) return ORIANA_EINVAL;
    if (!DZ_exp_logsum_hat && m > 0) return ORIANA_EINVAL;
    return zq_dense(DZ_hat_i, DZ_hat_j, DZ_exp_logsum_hat, log_U_hat, log_V_hat, nullptr, nullptr, D_hat,
                    reference_quirks ? 1 : 0, X, n, m, K, ws, ws_bytes, stream);
}

extern "C" int oriana_zq_sparse_gap_f32(float *SZ_hat_i, float *Z_hat_j, float *Z_exp_logsum_hat,
                                        const float *log_U_hat, const float *log_V_hat, const float *S_tilde,
                                        const float *S_hat, const float *X, int64_t n, int64_t m, int64_t K, void *ws,
                                        int64_t ws_bytes, void *stream) {
    if ((!S_tilde || !S_hat || !Z_exp_logsum_hat) && m > 0) return ORIANA_EINVAL;
    return zq_dense(SZ_hat_i, Z_hat_j, Z_exp_logsum_hat, log_U_hat, log_V_hat, S_tilde, S_hat, nullptr, 0, X, n, m, K,
                    ws, ws_bytes, stream);
}

extern "C" int oriana_zq_sparse_zigap_f32(float *DSZ_hat, float *DZ_hat, float *DZ_exp_logsum_hat,
                                          const float *log_U_hat, const float *log_V_hat, const float *S_tilde,
                                          const float *S_hat, const float *D_hat, const float *X, int64_t n, int64_t m,
                                          int64_t K, void *ws, int64_t ws_bytes, void *stream) {
    if ((!S_tilde || !S_hat || !DZ_exp_logsum_hat) && m > 0) return ORIANA_EINVAL;
    if (!D_hat && n > 0 && m > 0) return ORIANA_EINVAL;
    return zq_dense(DSZ_hat, DZ_hat, DZ_exp_logsum_hat, log_U_hat, log_V_hat, S_tilde, S_hat, D_hat, 0, X, n, m, K, ws,
                    ws_bytes, stream);
}
