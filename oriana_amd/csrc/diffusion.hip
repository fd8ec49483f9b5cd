// diffusion.hip -- the float64 kernels of the diffusion map on the neighbour graph of oriana_knn (oriana_amd/cluster.py:
// diffusion_graph, diffusion_map; models/base.py: cell_diffusion, cell_pseudotime; no counterpart in the reference).
//
//   oriana_csr_spmv_f64             y = A x for a CSR matrix.  A row is served by an aligned group of 16 lanes, four rows per wave:
//                                   lane l of the group takes the entries l, l + 16, ... of the row as ONE ascending fma chain, then
//                                   the 16 partial sums are added by four DPP steps inside the row of 16 lanes.  Which lane adds
//                                   which entry depends on the row alone.
//   oriana_basis_orthogonalize_f64  classical Gram-Schmidt of w against the j columns of Q, once or twice: c = Q^T w, w -= Q c,
//                                   h += c, and ||w||^2 at the end.  Every sum over rows runs over tiles of BT_ROWS rows: a tile
//                                   writes one partial per column into the scratch (k_basis_dot: the w tile in registers, a wave
//                                   streams its columns with 16-byte loads and ends each with one wave sum), k_basis_reduce adds
//                                   the tiles in ascending order, k_basis_sub walks the columns in ascending order with each thread
//                                   owning four rows.  Q is read twice per pass.
//   oriana_basis_append_f64         Q[:, j] = w / sqrt(beta2), beta2 read on the device.
//   oriana_basis_combine_f64        out = Q S, an ascending fma chain over the j columns per output element.
// No float atomics anywhere; no result depends on `blocks`, on what the scratch held or on how often a call is repeated.
#include "launch.h"

namespace oriana {
namespace {

constexpr int BT_ROWS = 1024;                  // oriana_basis_tile_rows(): the rows of one partial sum
constexpr int BT_NT = 256;                     // threads of a work-group of the basis kernels (four waves)
constexpr int BT_WAVES = BT_NT / 64;
constexpr int BT_DOT_PIECES = BT_ROWS / 128;   // 16-byte pieces of a column tile per lane where one WAVE reads the tile: 8
constexpr int BT_SUB_PIECES = BT_ROWS / (2 * BT_NT);     // ... per thread where the WORK-GROUP reads the tile: 2
constexpr int CM_COLS = 8;                     // output columns of oriana_basis_combine_f64 per walk over Q
constexpr int SPMV_NT = 256;                   // 16 groups of 16 lanes: 16 rows per work-group
constexpr int64_t BASIS_MAX_N = 1LL << 38, BASIS_MAX_J = 1LL << 20;

// rows r and r + 1 of a column (r even, p = the address of row r, 16-byte aligned); a row at or beyond n reads as 0 and is not
// touched
template <bool FULL>
__device__ __forceinline__ double2 ld_rows(const double *p, int64_t r, int64_t n) {
    if (FULL || r + 1 < n) return *reinterpret_cast<const double2 *>(p);
    double2 v;
    v.x = r < n ? p[0] : 0.0;
    v.y = 0.0;
    return v;
}
template <bool FULL>
__device__ __forceinline__ void st_rows(double *p, int64_t r, int64_t n, double2 v) {
    if (FULL || r + 1 < n) *reinterpret_cast<double2 *>(p) = v;
    else if (r < n) p[0] = v.x;
}

// sum over the aligned group of 16 lanes, in every lane of the group: xor 1, xor 2, then the two mirrors (lanes that already hold
// equal quad sums, so the mirror adds what xor 4 and xor 8 would)
__device__ __forceinline__ double group16_sum_f64(double v) {
    v += dpp_f64<0xB1>(v);
    v += dpp_f64<0x4E>(v);
    v += dpp_f64<0x141>(v);
    v += dpp_f64<0x140>(v);
    return v;
}

// ---- y = A x -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SPMV_NT)
k_csr_spmv(int64_t n, const int64_t *__restrict__ rp, const int32_t *__restrict__ cols, const double *__restrict__ vals,
           const double *__restrict__ x, double *__restrict__ y) {
    const int l = (int)threadIdx.x & 15, g = (int)threadIdx.x >> 4;
    const int64_t groups = (n + 15) / 16;
    for (int64_t b = blockIdx.x; b < groups; b += gridDim.x) {
        const int64_t i = b * 16 + g;
        double acc = 0.0;
        if (i < n) {
            const int64_t e1 = rp[i + 1];
            for (int64_t e = rp[i] + l; e < e1; e += 16) {
                const int64_t c = cols[e];
                if (c >= 0 && c < n) acc = fma(vals[e], x[c], acc);            // (a column outside the matrix addresses nothing)
            }
        }
        acc = group16_sum_f64(acc);
        if (i < n && l == 0) y[i] = acc;
    }
}

// ---- c = Q^T w per tile --------------------------------------------------------------------------------------------------------
template <bool FULL>
__device__ __forceinline__ void dot_tile(int64_t n, const double *__restrict__ Q, int64_t ldq, int64_t j, const double *__restrict__ w,
                                         double *__restrict__ part, int64_t t) {
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int64_t r0 = t * BT_ROWS + 2 * lane;
    double2 wr[BT_DOT_PIECES];
#pragma unroll
    for (int k = 0; k < BT_DOT_PIECES; ++k) wr[k] = ld_rows<FULL>(w + r0 + 128 * k, r0 + 128 * k, n);
    int64_t c = wv;
    for (; c + BT_WAVES < j; c += 2 * BT_WAVES) {                              // two columns of this wave at a time
        const double *qa = Q + c * ldq + r0, *qb = qa + BT_WAVES * ldq;
        double2 a[BT_DOT_PIECES], b[BT_DOT_PIECES];
#pragma unroll
        for (int k = 0; k < BT_DOT_PIECES; ++k) {
            a[k] = ld_rows<FULL>(qa + 128 * k, r0 + 128 * k, n);
            b[k] = ld_rows<FULL>(qb + 128 * k, r0 + 128 * k, n);
        }
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int k = 0; k < BT_DOT_PIECES; ++k) {
            sa = fma(a[k].x, wr[k].x, sa); sa = fma(a[k].y, wr[k].y, sa);
            sb = fma(b[k].x, wr[k].x, sb); sb = fma(b[k].y, wr[k].y, sb);
        }
        sa = wave_sum_f64(sa);
        sb = wave_sum_f64(sb);
        if (lane == 0) { part[t * j + c] = sa; part[t * j + c + BT_WAVES] = sb; }
    }
    if (c < j) {                                                               // (wave-uniform) the odd last column of this wave
        const double *qa = Q + c * ldq + r0;
        double sa = 0.0;
#pragma unroll
        for (int k = 0; k < BT_DOT_PIECES; ++k) {
            const double2 a = ld_rows<FULL>(qa + 128 * k, r0 + 128 * k, n);
            sa = fma(a.x, wr[k].x, sa); sa = fma(a.y, wr[k].y, sa);
        }
        sa = wave_sum_f64(sa);
        if (lane == 0) part[t * j + c] = sa;
    }
}

__global__ void __launch_bounds__(BT_NT)
k_basis_dot(int64_t n, const double *__restrict__ Q, int64_t ldq, int64_t j, const double *__restrict__ w, double *__restrict__ part,
            int64_t tiles) {
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        if ((t + 1) * BT_ROWS <= n) dot_tile<true>(n, Q, ldq, j, w, part, t);
        else dot_tile<false>(n, Q, ldq, j, w, part, t);
    }
}

// c[col] = the partials of the tiles in ascending order; h[col] += c[col]
__global__ void __launch_bounds__(64)
k_basis_reduce(const double *__restrict__ part, int64_t tiles, int64_t j, double *__restrict__ cvec, double *__restrict__ h) {
    const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (c >= j) return;
    double s = 0.0;
#pragma unroll 16
    for (int64_t t = 0; t < tiles; ++t) s += part[t * j + c];
    cvec[c] = s;
    h[c] += s;
}

// ---- w -= Q c per tile, and the tile's share of ||w||^2 after the last pass ----------------------------------------------------
template <bool FULL, bool LAST>
__device__ __forceinline__ void sub_tile(int64_t n, const double *__restrict__ Q, int64_t ldq, int64_t j, double *__restrict__ w,
                                         const double *__restrict__ cvec, double *__restrict__ npart, int64_t t, double *s_w) {
    const int tid = (int)threadIdx.x;
    const int64_t r0 = t * BT_ROWS + 2 * tid;
    double2 a[BT_SUB_PIECES];
#pragma unroll
    for (int k = 0; k < BT_SUB_PIECES; ++k) a[k] = ld_rows<FULL>(w + r0 + 2 * BT_NT * k, r0 + 2 * BT_NT * k, n);
    const double *q = Q + r0;
#pragma unroll 8
    for (int64_t c = 0; c < j; ++c) {
        const double m = -cvec[c];
#pragma unroll
        for (int k = 0; k < BT_SUB_PIECES; ++k) {
            const double2 v = ld_rows<FULL>(q + c * ldq + 2 * BT_NT * k, r0 + 2 * BT_NT * k, n);
            a[k].x = fma(m, v.x, a[k].x);
            a[k].y = fma(m, v.y, a[k].y);
        }
    }
#pragma unroll
    for (int k = 0; k < BT_SUB_PIECES; ++k) st_rows<FULL>(w + r0 + 2 * BT_NT * k, r0 + 2 * BT_NT * k, n, a[k]);
    if (LAST) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < BT_SUB_PIECES; ++k) { s = fma(a[k].x, a[k].x, s); s = fma(a[k].y, a[k].y, s); }      // (rows beyond n hold 0)
        s = wave_sum_f64(s);
        __syncthreads();                                                       // (the last tile's sums have been read)
        if ((tid & 63) == 0) s_w[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) npart[t] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
    }
}

template <bool LAST>
__global__ void __launch_bounds__(BT_NT)
k_basis_sub(int64_t n, const double *__restrict__ Q, int64_t ldq, int64_t j, double *__restrict__ w, const double *__restrict__ cvec,
            double *__restrict__ npart, int64_t tiles) {
    __shared__ double s_w[BT_WAVES];
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        if ((t + 1) * BT_ROWS <= n) sub_tile<true, LAST>(n, Q, ldq, j, w, cvec, npart, t, s_w);
        else sub_tile<false, LAST>(n, Q, ldq, j, w, cvec, npart, t, s_w);
    }
}

// beta2 = the tiles' shares in ascending order
__global__ void k_basis_norm(const double *__restrict__ npart, int64_t tiles, double *__restrict__ beta2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
#pragma unroll 16
    for (int64_t t = 0; t < tiles; ++t) s += npart[t];
    beta2[0] = s;
}

// ---- Q[:, j] = w / sqrt(beta2) -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BT_NT)
k_basis_append(int64_t n, double *__restrict__ qcol, const double *__restrict__ w, const double *__restrict__ beta2) {
    const int64_t r = ((int64_t)blockIdx.x * BT_NT + threadIdx.x) * 2;
    if (r >= n) return;
    const double s = __dsqrt_rn(beta2[0]);
    double2 v = ld_rows<false>(w + r, r, n);
    v.x = __ddiv_rn(v.x, s);
    v.y = __ddiv_rn(v.y, s);
    st_rows<false>(qcol + r, r, n, v);
}

// ---- out = Q S -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BT_NT)
k_basis_combine(int64_t n, const double *__restrict__ Q, int64_t ldq, int64_t j, const double *__restrict__ S, int64_t m,
                double *__restrict__ out, int64_t ldo) {
    const int64_t chunks = (n + 2 * BT_NT - 1) / (2 * BT_NT);
    for (int64_t b = blockIdx.x; b < chunks; b += gridDim.x) {
        const int64_t r = (b * BT_NT + threadIdx.x) * 2;
        for (int64_t c0 = 0; c0 < m; c0 += CM_COLS) {
            const int nc = m - c0 < CM_COLS ? (int)(m - c0) : CM_COLS;         // (uniform)
            double2 acc[CM_COLS];
#pragma unroll
            for (int u = 0; u < CM_COLS; ++u) acc[u] = make_double2(0.0, 0.0);
            for (int64_t k = 0; k < j; ++k) {
                const double2 v = ld_rows<false>(Q + k * ldq + r, r, n);
                const double *s = S + k * m + c0;
#pragma unroll
                for (int u = 0; u < CM_COLS; ++u)
                    if (u < nc) { acc[u].x = fma(s[u], v.x, acc[u].x); acc[u].y = fma(s[u], v.y, acc[u].y); }
            }
#pragma unroll
            for (int u = 0; u < CM_COLS; ++u)
                if (u < nc) st_rows<false>(out + (c0 + u) * ldo + r, r, n, acc[u]);
        }
    }
}

__host__ int64_t basis_tiles(int64_t n) { return (n + BT_ROWS - 1) / BT_ROWS; }
__host__ bool basis_dims_ok(int64_t n, int64_t ld, int64_t j) {
    return n >= 0 && n <= BASIS_MAX_N && j >= 1 && j <= BASIS_MAX_J && ld >= n && (ld & 1) == 0;
}
__host__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace oriana

using namespace oriana;

extern "C" int oriana_csr_spmv_f64(int64_t n, const int64_t *row_ptr, const int32_t *cols, const double *vals, const double *x,
                                   double *y, int64_t blocks, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || n > 0x7fffffffLL || blocks < 0) return ORIANA_EINVAL;
    if (n == 0) return 0;
    if (!row_ptr || !x || !y) return ORIANA_EINVAL;                // (cols and vals may be NULL for a matrix without entries)
    const int64_t groups = (n + 15) / 16;
    int64_t nb = blocks > 0 ? blocks : 16 * oriana_device_cus();
    if (nb > groups) nb = groups;
    if (nb < 1) nb = 1;
    return launch(k_csr_spmv, dim3((unsigned)nb), dim3(SPMV_NT), 0, stream, n, row_ptr, cols, vals, x, y);
}

extern "C" int64_t oriana_basis_tile_rows(void) { return BT_ROWS; }

extern "C" int64_t oriana_basis_orthogonalize_scratch_bytes_for(int64_t n, int64_t j) {
    if (n < 0 || n > BASIS_MAX_N || j < 1 || j > BASIS_MAX_J) return ORIANA_EINVAL;
    const int64_t tiles = basis_tiles(n);
    return ((tiles * j + j + tiles) * 8 + 15) / 16 * 16;
}

extern "C" int oriana_basis_orthogonalize_f64(int64_t n, const double *Q, int64_t ldq, int64_t j, double *w, double *h, double *beta2,
                                              int64_t passes, void *scratch, int64_t scratch_bytes, int64_t blocks, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!basis_dims_ok(n, ldq, j) || (passes != 1 && passes != 2) || blocks < 0 || scratch_bytes < 0) return ORIANA_EINVAL;
    if (scratch_bytes < oriana_basis_orthogonalize_scratch_bytes_for(n, j)) return ORIANA_EINVAL;
    if (n == 0) return 0;
    if (!Q || !w || !h || !beta2 || !scratch) return ORIANA_EINVAL;
    if (!aligned16(Q) || !aligned16(w) || !aligned16(scratch)) return ORIANA_EINVAL;
    const int64_t tiles = basis_tiles(n);
    double *part = static_cast<double *>(scratch), *cvec = part + tiles * j, *npart = cvec + j;
    int64_t nb = blocks > 0 ? blocks : 4 * oriana_device_cus();
    if (nb > tiles) nb = tiles;
    const unsigned nr = (unsigned)((j + 63) / 64);
    for (int64_t p = 0; p < passes; ++p) {
        int rc = launch(k_basis_dot, dim3((unsigned)nb), dim3(BT_NT), 0, stream, n, Q, ldq, j, w, part, tiles);
        if (rc) return rc;
        rc = launch(k_basis_reduce, dim3(nr), dim3(64), 0, stream, part, tiles, j, cvec, h);
        if (rc) return rc;
        if (p + 1 < passes) rc = launch(k_basis_sub<false>, dim3((unsigned)nb), dim3(BT_NT), 0, stream, n, Q, ldq, j, w, cvec, npart, tiles);
        else rc = launch(k_basis_sub<true>, dim3((unsigned)nb), dim3(BT_NT), 0, stream, n, Q, ldq, j, w, cvec, npart, tiles);
        if (rc) return rc;
    }
    return launch(k_basis_norm, dim3(1), dim3(1), 0, stream, npart, tiles, beta2);
}

extern "C" int oriana_basis_append_f64(int64_t n, double *Q, int64_t ldq, int64_t j, const double *w, const double *beta2,
                                       void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || n > BASIS_MAX_N || j < 0 || j > BASIS_MAX_J || ldq < n || (ldq & 1)) return ORIANA_EINVAL;
    if (n == 0) return 0;
    if (!Q || !w || !beta2 || !aligned16(Q) || !aligned16(w)) return ORIANA_EINVAL;
    const int64_t nb = (n + 2 * BT_NT - 1) / (2 * BT_NT);
    return launch(k_basis_append, dim3((unsigned)nb), dim3(BT_NT), 0, stream, n, Q + j * ldq, w, beta2);
}

extern "C" int oriana_basis_combine_f64(int64_t n, const double *Q, int64_t ldq, int64_t j, const double *S, int64_t m, double *out,
                                        int64_t ldo, int64_t blocks, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!basis_dims_ok(n, ldq, j) || m < 0 || m > BASIS_MAX_J || ldo < n || (ldo & 1) || blocks < 0) return ORIANA_EINVAL;
    if (n == 0 || m == 0) return 0;
    if (!Q || !S || !out || !aligned16(Q) || !aligned16(out)) return ORIANA_EINVAL;
    const int64_t chunks = (n + 2 * BT_NT - 1) / (2 * BT_NT);
    int64_t nb = blocks > 0 ? blocks : 8 * oriana_device_cus();
    if (nb > chunks) nb = chunks;
    return launch(k_basis_combine, dim3((unsigned)nb), dim3(BT_NT), 0, stream, n, Q, ldq, j, S, m, out, ldo);
}
