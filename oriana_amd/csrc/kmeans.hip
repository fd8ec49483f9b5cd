// kmeans.hip -- one Lloyd half-step of R independent k-means restarts over the same rows (oriana_kmeans_step): labels, per-cluster
// sums and counts, inertia, the minimum distance.  DESIGN.md section 5i.
//
// A work-group owns a contiguous range of 64-row tiles and a group of G restarts, one restart per wave.  The tile is staged in
// LDS once for the group, in the layout of rowscan.h (feature-major [k][65], column 64 stays zero); the staging loop is this
// file's own, because the waves of the group are a run-time number here.
//   assign      lane = row.  The centres of the wave's restart are wave-uniform: they come through scalar loads from a padded
//               float32 image ((R, Cp, dp), dp = pad4(d), Cp = C rounded up to 8; written by k_kmeans_pad), 8 centres x 4
//               features per step; d2 = sum_k (y_k - c_k)^2 by sequential fma over k ascending, the arg-min by a strict < over c
//               ascending (the smallest index wins a tie).  The chain is the text of rowscan.h's chain8, kept here as a copy:
//               called through the header, with row pointers cen + (c0 + j) dq, this kernel parked 38 SGPRs in VGPR lanes
//               instead of 10.
//   accumulate  lane = feature.  For every cluster c the rows labelled c (a ballot) are added in ascending row order in a register,
//               the tile's sum then goes into the wave's own (C, dp) float32 partial in LDS: no atomics, a fixed order.  After
//               KM_FLUSH tiles the partial is promoted into the work-group's float64 partial in global memory.
// k_kmeans_reduce adds the work-groups' partials in ascending order.  Nothing depends on which waves share a work-group, so a
// restart's outputs are the same bit for bit alone or inside any batch, for a given number of work-groups along the rows.
#include "rowscan.h"

namespace oriana {
namespace {

constexpr int KM_G = 4;                   // restarts (waves) of a work-group; 2 where the partials of 4 do not fit
constexpr int KM_FLUSH = 4;               // tiles between two promotions of the float32 partials to float64
constexpr int64_t KM_LDS = 160 * 1024;    // LDS of a CU
constexpr int64_t KM_MAX_CD = 8192;       // C * pad4(d) served

inline int64_t km_lds_bytes(int64_t dp, int64_t C, int64_t G) { return 4 * (dp * RS_LD + G * C * dp + G * C); }
inline int64_t km_group(int64_t dp, int64_t C) { return km_lds_bytes(dp, C, KM_G) <= KM_LDS ? KM_G : 2; }

struct KmPlan {
    int64_t dp, Cp, G, groups, ntiles, bx, tpb;
    int64_t off_psums, off_pinert, off_pcounts, total;      // bytes into the scratch (the padded centres sit at 0)
};

// sizes in range (d, C, R >= 1, n >= 0, C within oriana_kmeans_max_centers(d))
KmPlan km_plan(int64_t n, int64_t d, int64_t C, int64_t R, int64_t blocks) {
    KmPlan p;
    p.dp = pad4(d);
    p.Cp = (C + RS_CH - 1) / RS_CH * RS_CH;
    p.G = km_group(p.dp, C);
    p.groups = (R + p.G - 1) / p.G;
    p.ntiles = (n + RS_ROWS - 1) / RS_ROWS;
    int64_t bx = two_per_cu(blocks, p.groups);
    if (bx > p.ntiles) bx = p.ntiles;
    if (bx < 1) bx = 1;
    p.bx = bx;
    p.tpb = (p.ntiles + bx - 1) / bx;
    p.off_psums = R * p.Cp * p.dp * 4;                      // (dp is a multiple of 4: a multiple of 16 bytes)
    p.off_pinert = p.off_psums + bx * R * C * p.dp * 8;
    p.off_pcounts = p.off_pinert + bx * R * 8;
    p.total = p.off_pcounts + bx * R * C * 8;
    return p;
}

// promote a wave's float32 partial (LDS) into its float64 partial (global; `first`: not written yet) and clear it; lane e % 64 owns
// element e in every call; eight loads in flight
__device__ __forceinline__ void km_promote(float *part, double *__restrict__ gp, int CD, int lane, bool first) {
    for (int e0 = lane; e0 < CD; e0 += 64 * 8) {
        double g[8];
        #pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + 64 * u;
            g[u] = (!first && e < CD) ? gp[e] : 0.0;
        }
        #pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + 64 * u;
            if (e < CD) {
                gp[e] = g[u] + (double)part[e];
                part[e] = 0.0f;
            }
        }
    }
}

// the centres (R, C, d) as (R, Cp, dp) float32, zero where padded
__global__ void __launch_bounds__(256) k_kmeans_pad(float *__restrict__ cpad, const float *__restrict__ centers, int C, int d, int Cp,
                                                    int dp, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int k = (int)(e % dp);
    const int64_t rc = e / dp;
    const int c = (int)(rc % Cp);
    const int64_t r = rc / Cp;
    cpad[e] = (c < C && k < d) ? centers[(r * C + c) * d + k] : 0.0f;
}

__global__ void __launch_bounds__(256)
k_kmeans_step(const float *__restrict__ Y, int64_t n, int d, int64_t ldy, const float *__restrict__ cpad, int C, int Cp, int dp, int R,
              double *__restrict__ psums, int64_t *__restrict__ pcounts, double *__restrict__ pinert, int32_t *__restrict__ labels,
              int label_restart, float *__restrict__ mind, int64_t tpb, int64_t ntiles) {
    extern __shared__ float lds[];
    const int G = (int)(blockDim.x >> 6);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int CD = C * dp;
    float *tile = lds;
    float *part = lds + dp * RS_LD + w * CD;
    int *cnt = reinterpret_cast<int *>(lds + dp * RS_LD + G * CD) + w * C;
    const int r = (int)blockIdx.y * G + w;
    const bool live = r < R;                                          // (wave-uniform)

    for (int e = (int)threadIdx.x; e < dp * RS_LD; e += (int)blockDim.x) tile[e] = 0.0f;      // the padding features, column 64
    if (live) {
        for (int e = lane; e < CD; e += 64) part[e] = 0.0f;
        for (int e = lane; e < C; e += 64) cnt[e] = 0;
    }
    __syncthreads();

    const int64_t t0 = (int64_t)blockIdx.x * tpb;
    const int64_t t1 = t0 + tpb < ntiles ? t0 + tpb : ntiles;
    double *gp = psums + ((int64_t)blockIdx.x * R + (live ? r : 0)) * CD;
    const float4 *cen = reinterpret_cast<const float4 *>(cpad + (int64_t)(live ? r : 0) * Cp * dp);
    const int dq = dp >> 2;
    double inert = 0.0;
    bool first = true;
    int pending = 0;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t row0 = t * RS_ROWS;
        const int nrow = n - row0 < RS_ROWS ? (int)(n - row0) : RS_ROWS;
        // ---- stage the tile: wave w takes rows w, w + G, ..; lanes over the features; eight loads in flight
        for (int kk = lane; kk < d; kk += 64) {
            for (int ib = 0; ib < RS_ROWS / G; ib += 16) {          // (RS_ROWS / G is 16 or 32)
                float v[16];
                #pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int i = w + (ib + u) * G;
                    v[u] = i < nrow ? Y[(row0 + i) * ldy + kk] : 0.0f;
                }
                #pragma unroll
                for (int u = 0; u < 16; ++u) tile[kk * RS_LD + w + (ib + u) * G] = v[u];
            }
        }
        __syncthreads();
        if (live) {
            // ---- assign: lane = row
            float best = INFINITY;
            int lab = 0;
            const float *tl = tile + lane;
            for (int c0 = 0; c0 < C; c0 += RS_CH) {
                float acc[RS_CH];
                #pragma unroll
                for (int j = 0; j < RS_CH; ++j) acc[j] = 0.0f;
                for (int q = 0; q < dq; ++q) {
                    const float y0 = tl[(4 * q + 0) * RS_LD], y1 = tl[(4 * q + 1) * RS_LD];
                    const float y2 = tl[(4 * q + 2) * RS_LD], y3 = tl[(4 * q + 3) * RS_LD];
                    #pragma unroll
                    for (int j = 0; j < RS_CH; ++j) {
                        const float4 cv = cen[(c0 + j) * dq + q];
                        const float e0 = y0 - cv.x, e1 = y1 - cv.y, e2 = y2 - cv.z, e3 = y3 - cv.w;
                        acc[j] = fmaf(e0, e0, acc[j]);
                        acc[j] = fmaf(e1, e1, acc[j]);
                        acc[j] = fmaf(e2, e2, acc[j]);
                        acc[j] = fmaf(e3, e3, acc[j]);
                    }
                }
                #pragma unroll
                for (int j = 0; j < RS_CH; ++j)
                    if (c0 + j < C && acc[j] < best) { best = acc[j]; lab = c0 + j; }
            }
            const bool valid = lane < nrow;
            if (valid) {
                if (mind) mind[(int64_t)r * n + row0 + lane] = best;
                if (labels && r == label_restart) labels[row0 + lane] = lab;
                inert += (double)best;
            }
            // ---- accumulate: lane = feature; the rows of a cluster in ascending order, four LDS reads in flight
            for (int c = 0; c < C; ++c) {
                const unsigned long long mask = __ballot(valid && lab == c);
                if (!mask) continue;
                if (lane == 0) cnt[c] += __popcll(mask);
                for (int kb = 0; kb < dp; kb += 64) {
                    const bool on = kb + lane < dp;
                    const float *tk = tile + (on ? kb + lane : 0) * RS_LD;
                    float a = 0.0f;
                    unsigned long long m = mask;
                    while (m) {
                        const int i0 = __builtin_ctzll(m); m &= m - 1;
                        const int i1 = m ? __builtin_ctzll(m) : RS_ROWS; m &= m - 1;      // (column 64: + 0)
                        const int i2 = m ? __builtin_ctzll(m) : RS_ROWS; m &= m - 1;
                        const int i3 = m ? __builtin_ctzll(m) : RS_ROWS; m &= m - 1;
                        const float v0 = tk[i0], v1 = tk[i1], v2 = tk[i2], v3 = tk[i3];
                        a += v0; a += v1; a += v2; a += v3;
                    }
                    if (on) part[c * dp + kb + lane] += a;
                }
            }
            if (++pending == KM_FLUSH) {
                km_promote(part, gp, CD, lane, first);
                first = false;
                pending = 0;
            }
        }
        __syncthreads();
    }
    if (live) {
        if (pending || first) km_promote(part, gp, CD, lane, first);
        for (int e = lane; e < C; e += 64) pcounts[((int64_t)blockIdx.x * R + r) * C + e] = cnt[e];
        for (int o = 32; o > 0; o >>= 1) inert += __shfl_xor(inert, o, 64);
        if (lane == 0) pinert[(int64_t)blockIdx.x * R + r] = inert;
    }
}

// the work-groups' partials in ascending order: sums (R, C, d), then counts (R, C), then the inertia (R)
__global__ void __launch_bounds__(256)
k_kmeans_reduce(double *__restrict__ sums, int64_t *__restrict__ counts, double *__restrict__ inertia, const double *__restrict__ psums,
                const int64_t *__restrict__ pcounts, const double *__restrict__ pinert, int64_t bx, int64_t R, int C, int d, int dp) {
    int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t ns = R * C * d, nc = R * C;
    if (e < ns) {
        const int k = (int)(e % d);
        const int64_t rc = e / d;
        double s = 0.0;
        for (int64_t b = 0; b < bx; ++b) s += psums[(b * R * C + rc) * dp + k];
        sums[e] = s;
        return;
    }
    e -= ns;
    if (e < nc) {
        int64_t s = 0;
        for (int64_t b = 0; b < bx; ++b) s += pcounts[b * nc + e];
        counts[e] = s;
        return;
    }
    e -= nc;
    if (e < R) {
        double s = 0.0;
        for (int64_t b = 0; b < bx; ++b) s += pinert[b * R + e];
        inertia[e] = s;
    }
}

}  // namespace
}  // namespace oriana

using namespace oriana;

extern "C" int64_t oriana_kmeans_max_centers(int64_t d) {
    if (d < 1 || d > RS_MAX_D) return 0;
    return KM_MAX_CD / pad4(d);
}

extern "C" int64_t oriana_kmeans_group(int64_t d, int64_t C) {
    if (d < 1 || C < 1 || C > oriana_kmeans_max_centers(d)) return 0;
    return km_group(pad4(d), C);
}

extern "C" int64_t oriana_kmeans_partial_rows(void) { return (int64_t)KM_FLUSH * RS_ROWS; }

extern "C" int64_t oriana_kmeans_tile_rows(void) { return RS_ROWS; }

extern "C" int64_t oriana_kmeans_scratch_bytes(int64_t n, int64_t d, int64_t C, int64_t R, int64_t blocks) {
    if (n < 0 || d < 1 || C < 1 || R < 1 || blocks < 0) return ORIANA_EINVAL;
    if (C > oriana_kmeans_max_centers(d)) return ORIANA_EKRANGE;
    return km_plan(n, d, C, R, blocks).total;
}

extern "C" int oriana_kmeans_step(const float *Y, int64_t n, int64_t d, int64_t ldy, const float *centers, int64_t C, int64_t R,
                                  double *sums, int64_t *counts, double *inertia, int32_t *labels, int64_t label_restart, float *mind,
                                  void *scratch, int64_t blocks, void *stream) {
    if (n < 0 || d < 1 || C < 1 || R < 1 || ldy < d || blocks < 0) return ORIANA_EINVAL;
    if (C > oriana_kmeans_max_centers(d)) return ORIANA_EKRANGE;
    if (!centers || !sums || !counts || !inertia || !scratch || (n > 0 && !Y)) return ORIANA_EINVAL;
    if (labels && (label_restart < 0 || label_restart >= R)) return ORIANA_EINVAL;
    if (((uintptr_t)scratch & 15) || R > 0x7fffffffLL / (C * pad4(d) + 8)) return ORIANA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        ORIANA_HIP_CHECK(hipMemsetAsync(sums, 0, (size_t)(R * C * d) * 8, st));
        ORIANA_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)(R * C) * 8, st));
        ORIANA_HIP_CHECK(hipMemsetAsync(inertia, 0, (size_t)R * 8, st));
        return 0;
    }
    const KmPlan p = km_plan(n, d, C, R, blocks);
    if (p.groups > 65535 || p.bx > 0x7fffffffLL) return ORIANA_EINVAL;
    char *base = static_cast<char *>(scratch);
    float *cpad = reinterpret_cast<float *>(base);
    double *psums = reinterpret_cast<double *>(base + p.off_psums);
    double *pinert = reinterpret_cast<double *>(base + p.off_pinert);
    int64_t *pcounts = reinterpret_cast<int64_t *>(base + p.off_pcounts);
    const int64_t npad = R * p.Cp * p.dp;
    int rc = launch(k_kmeans_pad, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, st, cpad, centers, (int)C, (int)d, (int)p.Cp,
                    (int)p.dp, npad);
    if (rc) return rc;
    rc = launch(k_kmeans_step, dim3((unsigned)p.bx, (unsigned)p.groups), dim3((unsigned)(64 * p.G)), (size_t)km_lds_bytes(p.dp, C, p.G),
                st, Y, n, (int)d, ldy, cpad, (int)C, (int)p.Cp, (int)p.dp, (int)R, psums, pcounts, pinert, labels, (int)label_restart,
                mind, p.tpb, p.ntiles);
    if (rc) return rc;
    const int64_t nout = R * C * d + R * C + R;
    return launch(k_kmeans_reduce, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, sums, counts, inertia, psums, pcounts, pinert,
                  p.bx, R, (int)C, (int)d, (int)p.dp);
}
