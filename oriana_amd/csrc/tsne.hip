// tsne.hip -- the three device passes of the exact t-SNE layout of the cells (cluster.tsne).
//
// k_tsne_affinities  lane = row of the (n, k) squared distances of oriana_knn: the beta of p_j ~ exp(-beta (d_j - d_0)) whose entropy
//                    is log(perplexity), by doubling / halving while one side is unbounded and then bisection, in float64.
// k_tsne_attract     one wave per CSR row of the joint P: the lanes stride over the row's entries with float64 partial sums that
//                    wave_sum_f64 adds in one fixed shape, so a row's bits do not depend on the launch it is part of.
// k_tsne_repulse     the hot path, the scan of k_sil_scan at d = 2: a work-group of four waves owns one 64-query tile (lane = query:
//                    two registers, no LDS tile) and one candidate range; the waves take the range's 8-candidate steps in turn
//                    (wave w: steps w, w + 4, ..); the 16 floats of a step are wave-uniform and come through scalar loads.
//                    The pair is ONE float32 sequence (tsne_pair below).  Every w is converted to float64 and added to the lane's
//                    float64 sum (the driver subtracts the n self pairs from Z: a float32 partial sum next to an exact 1 would
//                    cost Z its digits where Z << n); the two force terms of a step's candidates are added in float32 in
//                    candidate order, and the step's two sums are converted and added to the lane's float64
//                    running sums.  At the end the four sums of a query are added through LDS in wave order and written as
//                    float64 per (tile, range, component, lane).
// k_tsne_reduce      lane = query: the ranges are added in range order (rowscan.h: add_ranges) and written (or, with accumulate,
//                    added) to rep / zrow.
// No atomics; every output has one writer and a fixed order inside a launch.  From rowscan.h come also the tile and step sizes,
// the two-work-groups-per-CU rule of the ranges and the limit on the row counts; there is no LDS tile and no d-long chain here.
#include "rowscan.h"

namespace oriana {
namespace {

constexpr int TS_W = 4;                   // waves of a work-group
constexpr int64_t TS_MAX_SPLIT = 32767;   // ranges the candidates are cut into (the y extent of the grid)
constexpr int TS_STEPS = 200;             // evaluations of the entropy per row, at most
constexpr double TS_HTOL = 1e-9;          // |H - log perplexity| at which the search of a row stops

// ---- affinities --------------------------------------------------------------------------------------------------------------
// S = sum_j exp(-beta e_j), E = sum_j e_j exp(-beta e_j) over the m finite entries, e_j = d_j - d_0 >= 0 (so S >= 1: no underflow of
// the sum); H = log S + beta E / S
__global__ void __launch_bounds__(64)
k_tsne_affinities(const float *__restrict__ d2, int64_t n, int k, double logperp, float *__restrict__ p, double *__restrict__ beta_out) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float *row = d2 + i * k;
    float *out = p + i * k;
    int m = 0;
    while (m < k && row[m] < INFINITY) ++m;                       // (ascending, padded with +inf: the finite entries lead)
    for (int j = m; j < k; ++j) out[j] = 0.0f;
    if (m == 0) { beta_out[i] = 1.0; return; }
    const double d0 = (double)row[0];
    double beta = 1.0, lo = 0.0, hi = INFINITY;
    bool has_lo = false;
    for (int it = 0; it < TS_STEPS; ++it) {
        double S = 0.0, E = 0.0;
        for (int j = 0; j < m; ++j) {
            const double e = (double)row[j] - d0;
            const double w = exp(-beta * e);
            S += w;
            E += e * w;
        }
        const double diff = log(S) + beta * E / S - logperp;
        if (fabs(diff) <= TS_HTOL) break;
        if (diff > 0.0) {                                          // too flat: a larger beta
            lo = beta; has_lo = true;
            beta = hi == INFINITY ? beta * 2.0 : 0.5 * (beta + hi);
        } else {
            hi = beta;
            beta = has_lo ? 0.5 * (beta + lo) : beta * 0.5;
        }
    }
    double S = 0.0;
    for (int j = 0; j < m; ++j) S += exp(-beta * ((double)row[j] - d0));
    for (int j = 0; j < m; ++j) out[j] = (float)(exp(-beta * ((double)row[j] - d0)) / S);
    beta_out[i] = beta;
}

// ---- the attractive term -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * TS_W)
k_tsne_attract(const int64_t *__restrict__ rp, const int32_t *__restrict__ col, const float *__restrict__ val,
               const float2 *__restrict__ Y, int64_t n, double *__restrict__ attr, double *__restrict__ klrow) {
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int64_t i = (int64_t)blockIdx.x * TS_W + w;              // (wave-uniform: all 64 lanes reach the reduction)
    if (i >= n) return;
    const int64_t a = rp[i], b = rp[i + 1];
    const float2 yi = Y[i];
    double sx = 0.0, sy = 0.0, sk = 0.0;
    for (int64_t e = a + lane; e < b; e += 64) {
        const int64_t j = col[e];
        if (j < 0 || j >= n) continue;                             // (a column outside the matrix addresses nothing)
        const double P = (double)val[e];
        const float2 yj = Y[j];
        const double dx = (double)yi.x - (double)yj.x, dy = (double)yi.y - (double)yj.y;
        const double D = fma(dy, dy, fma(dx, dx, 1.0));
        const double pw = P / D;
        sx = fma(pw, dx, sx);
        sy = fma(pw, dy, sy);
        if (P > 0.0) sk = fma(P, log(P) + log(D), sk);
    }
    sx = wave_sum_f64(sx);
    sy = wave_sum_f64(sy);
    sk = wave_sum_f64(sk);
    if (lane == 0) {
        attr[2 * i] = sx;
        attr[2 * i + 1] = sy;
        klrow[i] = sk;
    }
}

// ---- the repulsive term ------------------------------------------------------------------------------------------------------
// THE PAIR, one fixed float32 sequence (include/oriana_hip.h states it; tests/tsne_reference.py bounds it):
//   dx = qx - yx, dy = qy - yy            each rounded once
//   s  = fmaf(dy, dy, fmaf(dx, dx, 1))    >= 1
//   w  = v_rcp_f32(s)                     the hardware reciprocal, 1 ulp (no correction sequence: DESIGN.md 5m)
//   w2 = w * w
// then sz = sz + (double)w in float64, and ax = fmaf(w2, dx, ax), ay = fmaf(w2, dy, ay) in float32 over the candidates of one step,
// in candidate order from 0 (the products are not rounded on their own: written as fmaf so that no contraction setting decides
// it).  Bit-identical points: dx = dy = 0, s = 1, w = 1 exactly, and the force terms are exactly 0.
__device__ __forceinline__ void tsne_pair(float qx, float qy, float yx, float yy, float &ax, float &ay, double &sz) {
    const float dx = qx - yx, dy = qy - yy;
    const float s = fmaf(dy, dy, fmaf(dx, dx, 1.0f));
    const float w = __builtin_amdgcn_rcpf(s);
    const float w2 = w * w;
    sz += (double)w;
    ax = fmaf(w2, dx, ax);
    ay = fmaf(w2, dy, ay);
}

struct TsPlan {
    int64_t ntiles, nranges, sp;          // sp: steps per range
    int64_t total;                        // bytes of the scratch: [tile][range][3][64] float64
};

TsPlan ts_plan(int64_t nq, int64_t n, int64_t blocks) {
    TsPlan p;
    p.ntiles = (nq + RS_ROWS - 1) / RS_ROWS;
    const int64_t steps = (n + RS_CH - 1) / RS_CH;
    int64_t t = two_per_cu(blocks, p.ntiles);
    if (t > TS_MAX_SPLIT) t = TS_MAX_SPLIT;
    if (t > steps) t = steps;
    if (t < 1) t = 1;
    p.sp = steps > 0 ? (steps + t - 1) / t : 1;
    p.nranges = steps > 0 ? (steps + p.sp - 1) / p.sp : 0;       // (no range is empty)
    p.total = p.ntiles * p.nranges * 3 * RS_ROWS * 8;
    return p;
}

// part: [tile][range][3][64] float64; range r owns the candidates [r sp 8, min((r + 1) sp 8, n))
__global__ void __launch_bounds__(64 * TS_W)
k_tsne_repulse(const float2 *__restrict__ Q, int64_t nq, const float2 *__restrict__ Y, int n, int sp, double *__restrict__ part) {
    __shared__ double red[TS_W * 3 * RS_ROWS];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int64_t q = (int64_t)blockIdx.x * RS_ROWS + lane;
    const float2 qv = Q[q < nq ? q : nq - 1];                      // (a lane beyond the queries repeats the last one; never written)
    const float qx = qv.x, qy = qv.y;

    // (rows are ints: n <= 2^31 - 9, so r0 + st * 8 + 7 stays an int)
    const int64_t first = (int64_t)blockIdx.y * sp * RS_CH, last = first + (int64_t)sp * RS_CH;
    const int r0 = (int)first, r1 = (int)(last < n ? last : n);
    const int nst = (r1 - r0 + RS_CH - 1) / RS_CH;
    double sx = 0.0, sy = 0.0, sz = 0.0;

    for (int st = w; st < nst; st += TS_W) {
        const int c0 = r0 + st * RS_CH;
        float ax = 0.0f, ay = 0.0f;
        if (c0 + RS_CH <= r1) {                                    // (wave-uniform) a whole step: 16 consecutive floats
            const float2 *c = Y + c0;
            float2 v[RS_CH];
            #pragma unroll
            for (int j = 0; j < RS_CH; ++j) v[j] = c[j];
            #pragma unroll
            for (int j = 0; j < RS_CH; ++j) tsne_pair(qx, qy, v[j].x, v[j].y, ax, ay, sz);
        } else {                                                   // the range's tail re-reads the last point, masked
            #pragma unroll
            for (int j = 0; j < RS_CH; ++j) {
                const float2 v = Y[c0 + j < r1 ? c0 + j : r1 - 1];
                if (c0 + j < r1) tsne_pair(qx, qy, v.x, v.y, ax, ay, sz);
            }
        }
        sx += (double)ax;
        sy += (double)ay;
    }

    // ---- the four sums of a query in wave order
    red[(w * 3 + 0) * RS_ROWS + lane] = sx;
    red[(w * 3 + 1) * RS_ROWS + lane] = sy;
    red[(w * 3 + 2) * RS_ROWS + lane] = sz;
    __syncthreads();
    if (w == 0) {
        double *out = part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * (3 * RS_ROWS) + lane;
        #pragma unroll
        for (int c = 0; c < 3; ++c) {
            double s = red[c * RS_ROWS + lane];
            #pragma unroll
            for (int v = 1; v < TS_W; ++v) s += red[(v * 3 + c) * RS_ROWS + lane];
            out[c * RS_ROWS] = s;
        }
    }
}

__global__ void __launch_bounds__(64)
k_tsne_reduce(double *__restrict__ rep, double *__restrict__ zrow, int64_t nq, const double *__restrict__ part, int nranges,
              int accumulate) {
    const int lane = (int)threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * RS_ROWS + lane;
    if (q >= nq) return;
    double s[3];
    add_ranges(s, part, nranges, 0, nranges, lane);
    if (accumulate) {
        s[0] += rep[2 * q];
        s[1] += rep[2 * q + 1];
        s[2] += zrow[q];
    }
    rep[2 * q] = s[0];
    rep[2 * q + 1] = s[1];
    zrow[q] = s[2];
}

int ts_check_sizes(int64_t nq, int64_t n, int64_t blocks) {
    if (nq < 0 || n < 0 || blocks < 0) return ORIANA_EINVAL;
    if (!rows_fit_int(nq, n)) return ORIANA_EINVAL;
    return 0;
}

}  // namespace
}  // namespace oriana

using namespace oriana;

extern "C" int64_t oriana_tsne_affinity_steps(void) { return TS_STEPS; }

extern "C" int oriana_tsne_affinities(const float *sq_distances, int64_t n, int64_t k, double perplexity, float *p, double *beta,
                                      void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || k < 1 || !(perplexity >= 1.0) || !(perplexity < INFINITY)) return ORIANA_EINVAL;
    if (k > 0x7fffffffLL) return ORIANA_EKRANGE;
    if (n == 0) return 0;
    if (!sq_distances || !p || !beta) return ORIANA_EINVAL;
    return launch(k_tsne_affinities, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, sq_distances, n, (int)k, log(perplexity), p,
                  beta);
}

extern "C" int oriana_tsne_attract(const int64_t *row_ptr, const int32_t *cols, const float *vals, const float *Y, int64_t n,
                                   double *attr, double *klrow, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || n > 0x7fffffffLL) return ORIANA_EINVAL;
    if (n == 0) return 0;
    if (!row_ptr || !Y || !attr || !klrow) return ORIANA_EINVAL;   // (cols and vals may be NULL for a matrix without entries)
    if ((uintptr_t)Y & 7) return ORIANA_EINVAL;
    return launch(k_tsne_attract, dim3((unsigned)((n + TS_W - 1) / TS_W)), dim3(64 * TS_W), 0, stream, row_ptr, cols, vals,
                  reinterpret_cast<const float2 *>(Y), n, attr, klrow);
}

extern "C" int64_t oriana_tsne_repulse_scratch_bytes_for(int64_t nq, int64_t n, int64_t blocks) {
    const int rc = ts_check_sizes(nq, n, blocks);
    if (rc) return rc;
    const int64_t b = ts_plan(nq, n, blocks).total;
    return b > 16 ? b : 16;
}

extern "C" int oriana_tsne_repulse(const float *Q, int64_t nq, const float *Y, int64_t n, double *rep, double *zrow, int accumulate,
                                   void *scratch, int64_t blocks, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ts_check_sizes(nq, n, blocks);
    if (rc) return rc;
    if (!scratch || (nq > 0 && (!Q || !rep || !zrow)) || (n > 0 && !Y)) return ORIANA_EINVAL;
    if (((uintptr_t)scratch & 15) || ((uintptr_t)Q & 7) || ((uintptr_t)Y & 7)) return ORIANA_EINVAL;
    if (nq == 0) return 0;
    const TsPlan p = ts_plan(nq, n, blocks);
    double *part = static_cast<double *>(scratch);
    if (p.nranges > 0) {
        rc = launch(k_tsne_repulse, dim3((unsigned)p.ntiles, (unsigned)p.nranges), dim3(64 * TS_W), 0, stream,
                    reinterpret_cast<const float2 *>(Q), nq, reinterpret_cast<const float2 *>(Y), (int)n, (int)p.sp, part);
        if (rc) return rc;
    }
    return launch(k_tsne_reduce, dim3((unsigned)p.ntiles), dim3(64), 0, stream, rep, zrow, nq, part, (int)p.nranges,
                  accumulate ? 1 : 0);
}
