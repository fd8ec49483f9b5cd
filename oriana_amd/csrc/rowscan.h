// rowscan.h -- what the four geometry passes on the cell features share (kmeans.hip, knn.hip, silhouette.hip, tsne.hip; DESIGN.md
// sections 5i, 5j, 5k, 5m): a work-group owns a tile of 64 rows, lane = row, and its waves take 8-candidate steps of a candidate
// range in turn.
//   the tile     feature-major in LDS, [pad4(d)][65], zero padding features and a zero column 64: zero_tile, stage_tile
//   the image    the candidates as float32 rows that start 16-byte aligned and hold pad4(d) floats, so that a step's 8 candidates x 4
//                features are wave-uniform scalar loads: Y itself where direct_image() holds, else a padded copy (row_image; the
//                one pad kernel of the library sits in knn.hip)
//   THE PAIR     f = sum_j (q_j - c_j)^2 as one fmaf chain over the features ascending from 0 (include/oriana_hip.h states it):
//                chain8, on the row pointers pick_rows8 chose
//   the ranges   enough for two work-groups per CU given the tiles (two_per_cu); every caller adds its own clamps
//   the sums     the float64 sums of a tile's ranges are added in range order (add_ranges): no atomics, one writer, one fixed order.
//                (Before that a scan kernel adds the lane sums of its W waves through LDS in wave order 0 .. W - 1; that text
//                stays in k_sil_scan and k_tsne_repulse: called through a template here it changed the address arithmetic of
//                both kernels, by one to three instructions outside control flow, and gave k_sil_scan a third parked SGPR.)
// Step counters and candidate numbers are 32-bit on purpose: with 64-bit ones the compiler no longer proves the row addresses
// uniform and falls back to vector loads (5j).
#pragma once
#include "launch.h"

namespace oriana {

constexpr int RS_ROWS = 64;               // rows of a tile (one per lane)
constexpr int RS_LD = 65;                 // floats between two features of the LDS tile; column 64 holds 0
constexpr int RS_CH = 8;                  // candidates per step
constexpr int64_t RS_MAX_D = 256;         // features served

inline int64_t pad4(int64_t d) { return (d + 3) / 4 * 4; }
inline int64_t pad16(int64_t b) { return (b + 15) / 16 * 16; }
// Y itself serves as the candidate image where every row starts 16-byte aligned and holds whole groups of four features
inline bool direct_image(const float *Y, int64_t ldy, int64_t d) { return d % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)Y & 15) == 0; }
// ranges per tile (or work-groups per group of restarts): `blocks`, or enough for two work-groups per CU
inline int64_t two_per_cu(int64_t blocks, int64_t tiles) {
    return blocks > 0 ? blocks : (2 * oriana_device_cus() + tiles - 1) / (tiles > 0 ? tiles : 1);
}
// queries and candidates are ints in the kernels, and so is the last step's c0 + 7
inline bool rows_fit_int(int64_t nq, int64_t n) { return nq <= 0x7fffffffLL && n <= 0x7fffffffLL - RS_CH; }

// the (n, d) rows of Y as an image: Y itself, or a pad4(d) copy that the pad kernel writes to `scratch` on stream st
struct RowImage {
    const float4 *rows;
    int64_t ld4;                          // float4 between two rows
};
int row_image(const float *Y, int64_t n, int64_t ldy, int64_t d, void *scratch, hipStream_t st, RowImage *out);

// ---- the tile; a work-group of W waves, barriers are the caller's -----------------------------------------------------------
template <int W>
__device__ __forceinline__ void zero_tile(float *tile, int dp) {
    for (int e = (int)threadIdx.x; e < dp * RS_LD; e += 64 * W) tile[e] = 0.0f;      // the padding features, column 64
}

// rows row0 .. row0 + 63 of Q (nq, d): wave w takes rows w, w + W, ..; lanes over the features; 64 / W loads in flight
template <int W>
__device__ __forceinline__ void stage_tile(float *tile, const float *Q, int64_t nq, int d, int64_t ldq, int64_t row0,
                                           int w, int lane) {
    const int nrow = nq - row0 < RS_ROWS ? (int)(nq - row0) : RS_ROWS;
    for (int kk = lane; kk < d; kk += 64) {
        float v[RS_ROWS / W];
        #pragma unroll
        for (int u = 0; u < RS_ROWS / W; ++u) {
            const int i = w + u * W;
            v[u] = i < nrow ? Q[(row0 + i) * ldq + kk] : 0.0f;
        }
        #pragma unroll
        for (int u = 0; u < RS_ROWS / W; ++u) tile[kk * RS_LD + w + u * W] = v[u];
    }
}

// ---- the pair ------------------------------------------------------------------------------------------------------------------
// the rows of the step at candidate c0 of a range that ends at `end` (int or int64_t, as the caller holds it): a step's tail
// re-reads the last row
template <typename End>
__device__ __forceinline__ void pick_rows8(const float4 *(&row)[RS_CH], const float4 *img, int64_t ld4, int c0, End end) {
    #pragma unroll
    for (int j = 0; j < RS_CH; ++j) {
        const int64_t c = c0 + j < end ? c0 + j : end - 1;
        row[j] = img + c * ld4;
    }
}

// acc[j] = f(the lane's row of the tile, row[j]) over dq groups of four features; tl = tile + lane
__device__ __forceinline__ void chain8(float (&acc)[RS_CH], const float *tl, int dq, const float4 *(&row)[RS_CH]) {
    #pragma unroll
    for (int j = 0; j < RS_CH; ++j) acc[j] = 0.0f;
    for (int q = 0; q < dq; ++q) {
        const float y0 = tl[(4 * q + 0) * RS_LD], y1 = tl[(4 * q + 1) * RS_LD];
        const float y2 = tl[(4 * q + 2) * RS_LD], y3 = tl[(4 * q + 3) * RS_LD];
        #pragma unroll
        for (int j = 0; j < RS_CH; ++j) {
            const float4 cv = row[j][q];
            const float e0 = y0 - cv.x, e1 = y1 - cv.y, e2 = y2 - cv.z, e3 = y3 - cv.w;
            acc[j] = fmaf(e0, e0, acc[j]);
            acc[j] = fmaf(e1, e1, acc[j]);
            acc[j] = fmaf(e2, e2, acc[j]);
            acc[j] = fmaf(e3, e3, acc[j]);
        }
    }
}

// ---- the float64 sums ----------------------------------------------------------------------------------------------------------
// s = the ranges [i0, i1) of tile blockIdx.x for this lane, in range order; nranges: the ranges of a tile in part
template <int NC>
__device__ __forceinline__ void add_ranges(double (&s)[NC], const double *part, int nranges, int i0, int i1, int lane) {
    const double *p = part + (int64_t)blockIdx.x * nranges * (NC * RS_ROWS) + lane;
    #pragma unroll
    for (int c = 0; c < NC; ++c) s[c] = 0.0;
    for (int i = i0; i < i1; ++i) {
        #pragma unroll
        for (int c = 0; c < NC; ++c) s[c] += p[(int64_t)i * (NC * RS_ROWS) + c * RS_ROWS];
    }
}

}  // namespace oriana
