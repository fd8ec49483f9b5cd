// harmony.hip -- the three passes of Harmony batch correction on the cell features (oriana_harmony_assign, oriana_harmony_moments,
// oriana_harmony_correct): soft assignments under a per-batch penalty, the per-cluster per-batch moments, the corrected rows.
// DESIGN.md section 5r.
//
// Every work-group is ONE wave: nothing below depends on which waves share a work-group, and a barrier is a fence only.
//   assign    a work-group owns a contiguous range of 64-row tiles.  The tile is staged in LDS in the layout of rowscan.h
//             (feature-major [k][65]).  lane = row: the centres are wave-uniform, scalar loads from a zero-padded image ((Kp, dp),
//             written by k_harmony_pad), 8 centres x 4 features per step, the dot products compensated (hm_dot2); THE PAIR (include/oriana_hip.h states it) leaves dist in
//             LDS ([K][65]), then e_k, their sum and R in two more walks over k.  lane = cluster: the rows of one batch (a ballot)
//             are added in ascending row order in float64 into the work-group's own (K, B) image in LDS; lane = cluster again
//             writes the rows of R coalesced.  No atomics; k_harmony_assign_reduce adds the work-groups' partials in ascending order.
//   moments   a work-group owns a range of tiles, one batch, HM_KC clusters and 64 of the d + 1 columns (column d is the constant
//             1: its sum is O).  lane = column; the rows of the batch in ascending order, four in flight, the responsibilities
//             wave-uniform; the four rows in flight in float32, then promoted into float64 registers (with a whole tile's rows
//             in float32 the centres carried sqrt(T) roundings each: DESIGN.md 5r, end to end).  One writer per partial;
//             k_harmony_moments_reduce adds the ranges in ascending order.
//   correct   a work-group owns a range of tiles and one batch, whose (K, dp) image of W it stages in LDS once.  lane = feature for
//             the fmaf chain over k (four rows share a read of W), lane = row for the norm's chain over the features.
#include "rowscan.h"

// THE PAIR and the chains below are fixed float32 sequences: every fused multiply-add is written as fmaf and nothing else may
// fuse, so THIS FILE IS COMPILED WITH -ffp-contract=off (_build.EXTRA_FLAGS).  __fmul_rn, __fadd_rn and __fsub_rn are plain
// operators in this toolchain, and under hipcc's default (fast) the compiler contracted the sum of the compensated chain, p - bb
// and the sum over k into fused multiply-adds; `#pragma clang fp contract(off)` at file scope changed nothing in the device code.
namespace oriana {
namespace {

constexpr int64_t HM_LDS = 160 * 1024;    // LDS of a CU
constexpr int HM_MAX_B = 64;              // batches served: the limit on K below leaves room for (K, HM_MAX_B) float32 + float64
constexpr int HM_KC = 16;                 // moments: clusters of a work-group
constexpr int HM_STAGE = 16;              // assign: loads of a lane in flight while a tile is staged
constexpr int HM_CK = 4;                  // correct: clusters per step (4 rows x HM_CK responsibilities in SGPRs)
constexpr int HM_T = 4;                   // moments: rows added in float32 before the promotion to float64 (the rows in flight)

inline int64_t hm_assign_lds(int64_t dp, int64_t K, int64_t B) { return 4 * (dp * RS_LD + K * RS_LD + K * B) + 8 * K * B; }
inline int64_t hm_correct_lds(int64_t dp, int64_t K) { return 4 * (dp * RS_LD + K * dp + RS_ROWS); }
inline int64_t hm_max_clusters(int64_t d) {
    const int64_t dp = pad4(d);
    const int64_t a = (HM_LDS - 4 * dp * RS_LD) / (4 * RS_LD + 12 * HM_MAX_B);
    const int64_t c = (HM_LDS - 4 * dp * RS_LD - 4 * RS_ROWS) / (4 * dp);
    return a < c ? a : c;
}

// ranges of tiles: `blocks`, or enough for `per_cu` single-wave work-groups per CU given `groups` work-groups per range
struct HmRanges { int64_t ntiles, bx, tpb; };
inline HmRanges hm_ranges(int64_t n, int64_t blocks, int64_t groups, int64_t per_cu) {
    HmRanges r;
    r.ntiles = (n + RS_ROWS - 1) / RS_ROWS;
    int64_t bx = blocks > 0 ? blocks : (per_cu * oriana_device_cus() + groups - 1) / groups;
    if (bx > r.ntiles) bx = r.ntiles;
    if (bx < 1) bx = 1;
    r.tpb = (r.ntiles + bx - 1) / bx;
    if (r.tpb < 1) r.tpb = 1;                       // (n = 0)
    r.bx = (r.ntiles + r.tpb - 1) / r.tpb;          // (no range without a tile)
    if (r.bx < 1) r.bx = 1;
    return r;
}
inline int64_t up16(int64_t b) { return (b + 15) / 16 * 16; }

// src (rows, d) contiguous as (rowsp, dp) float32, zero where padded; `perm_B` > 0: src is (rows, perm_B, d), dst (perm_B, rows, dp)
__global__ void __launch_bounds__(256) k_harmony_pad(float *__restrict__ dst, const float *__restrict__ src, int rows, int d, int rowsp,
                                                     int dp, int perm_B, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int f = (int)(e % dp);
    const int64_t r = e / dp;
    if (perm_B > 0) {
        const int k = (int)(r % rows);
        const int64_t b = r / rows;
        dst[e] = f < d ? src[((int64_t)k * perm_B + b) * d + f] : 0.0f;
    } else {
        dst[e] = (r < rows && f < d) ? src[r * d + f] : 0.0f;
    }
    (void)rowsp;
}

// one feature of the compensated dot product of THE PAIR: acc takes the rounded product by a rounded addition, cmp what the two
// roundings lost -- the product's by fmaf, the addition's by the six operations of the error-free sum (no ordering of |acc| and
// |p| is assumed).  A plain fmaf chain loses up to d u sum |z y| of the dot product; at 1 / sigma = 10 that alone moved R by 6e-07
// where rounding the stored state moves it by 2e-07 (end to end).
__device__ __forceinline__ void hm_dot2(float &acc, float &cmp, float z, float y) {
    const float p = __fmul_rn(z, y);
    const float ep = fmaf(z, y, -p);
    const float s = __fadd_rn(acc, p);
    const float bb = __fsub_rn(s, acc);
    const float es = __fadd_rn(__fsub_rn(acc, __fsub_rn(s, bb)), __fsub_rn(p, bb));
    acc = s;
    cmp = __fadd_rn(cmp, __fadd_rn(ep, es));
}

// e_k of THE PAIR from dist_k, the row's minimum, cexp = float32(-log2(e) / sigma) and P_kb: three roundings and the instruction's own
__device__ __forceinline__ float hm_ek(float dist, float m, float cexp, float p) {
    const float a = __fsub_rn(dist, m);
    const float t = __fmul_rn(a, cexp);
    return __fmul_rn(__builtin_amdgcn_exp2f(t), p);
}

__global__ void __launch_bounds__(64)
k_harmony_assign(const float *__restrict__ Z, int64_t n, int d, int64_t ldz, const int32_t *__restrict__ batch,
                 const float *__restrict__ cpad, int K, const float *__restrict__ P, int B, float cexp, float *__restrict__ R,
                 double *__restrict__ pO, double *__restrict__ psum, int tpb) {
    extern __shared__ double hm_lds[];
    const int dp = (d + 3) & ~3;
    const int ntiles = (int)((n + RS_ROWS - 1) / RS_ROWS);
    const int lane = (int)threadIdx.x;
    const int KB = K * B;
    double *oacc = hm_lds;                                          // (K, B) float64: this work-group's O
    float *tile = reinterpret_cast<float *>(oacc + KB);             // [dp][65]
    float *D = tile + dp * RS_LD;                                   // [K][65]: dist, then R
    float *Ps = D + K * RS_LD;                                      // (K, B)
    for (int e = lane; e < KB; e += 64) { oacc[e] = 0.0; Ps[e] = P[e]; }
    zero_tile<1>(tile, dp);
    __syncthreads();

    const int t0 = (int)blockIdx.x * tpb;
    const int t1 = t0 + tpb < ntiles ? t0 + tpb : ntiles;
    const float4 *cen = reinterpret_cast<const float4 *>(cpad);
    const int dq = dp >> 2;
    double sd = 0.0, se = 0.0;

    for (int t = t0; t < t1; ++t) {
        const int64_t row0 = (int64_t)t * RS_ROWS;
        const int nrow = n - row0 < RS_ROWS ? (int)(n - row0) : RS_ROWS;
        // stage the tile, lanes over the tile's elements in row-major order: per-lane addresses, HM_STAGE loads in flight.  (The
        // staging loop is this file's own: stage_tile<1> keeps the addresses of all 64 rows in SGPRs across the feature loop, which
        // parked 535 of them in VGPR lanes here.)  Rows past nrow keep what an earlier tile left: finite, and never used.
        const int tot = nrow * d;
        #pragma unroll 1
        for (int e0 = lane; e0 < tot; e0 += 64 * HM_STAGE) {
            float v[HM_STAGE];
            int at[HM_STAGE];
            #pragma unroll
            for (int u = 0; u < HM_STAGE; ++u) {
                const int e = e0 + 64 * u < tot ? e0 + 64 * u : tot - 1;      // (a tail stores the last element again: no predicates)
                const int i = e / d, f = e - i * d;
                at[u] = f * RS_LD + i;
                v[u] = Z[(row0 + i) * ldz + f];
            }
            #pragma unroll
            for (int u = 0; u < HM_STAGE; ++u) tile[at[u]] = v[u];
        }
        const bool valid = lane < nrow;
        const int b = valid ? batch[row0 + lane] : -1;
        const int bc = b < 0 ? 0 : (b < B ? b : B - 1);           // (a batch out of range never indexes anything)
        __syncthreads();
        // ---- dist: lane = row
        const float *tl = tile + lane;
        float *Dl = D + lane;
        float m = INFINITY;
        for (int c0 = 0; c0 < K; c0 += RS_CH) {
            float acc[RS_CH], cmp[RS_CH];
            #pragma unroll
            for (int j = 0; j < RS_CH; ++j) { acc[j] = 0.0f; cmp[j] = 0.0f; }
            for (int q = 0; q < dq; ++q) {
                const float y0 = tl[(4 * q + 0) * RS_LD], y1 = tl[(4 * q + 1) * RS_LD];
                const float y2 = tl[(4 * q + 2) * RS_LD], y3 = tl[(4 * q + 3) * RS_LD];
                #pragma unroll
                for (int j = 0; j < RS_CH; ++j) {
                    const float4 cv = cen[(c0 + j) * dq + q];
                    hm_dot2(acc[j], cmp[j], y0, cv.x);
                    hm_dot2(acc[j], cmp[j], y1, cv.y);
                    hm_dot2(acc[j], cmp[j], y2, cv.z);
                    hm_dot2(acc[j], cmp[j], y3, cv.w);
                }
            }
            #pragma unroll
            for (int j = 0; j < RS_CH; ++j)
                if (c0 + j < K) {
                    const float dist = fmaf(-2.0f, __fadd_rn(acc[j], cmp[j]), 2.0f);
                    Dl[(c0 + j) * RS_LD] = dist;
                    m = fminf(m, dist);
                }
        }
        // ---- e_k and their sum over k ascending, then R = e_k * (1 / sum)
        float s = 0.0f;
        #pragma unroll 1
        for (int k = 0; k < K; ++k) s = __fadd_rn(s, hm_ek(Dl[k * RS_LD], m, cexp, Ps[k * B + bc]));
        const float inv = 1.0f / s;
        double rd = 0.0, re = 0.0;
        #pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const float dist = Dl[k * RS_LD];
            const float r = __fmul_rn(hm_ek(dist, m, cexp, Ps[k * B + bc]), inv);
            Dl[k * RS_LD] = r;
            rd += (double)r * (double)dist;
            if (r > 0.0f) re += (double)r * (double)logf(r);
        }
        if (valid) { sd += rd; se += re; }
        __syncthreads();
        // ---- O: lane = cluster; the rows of a batch in ascending order, four LDS reads in flight
        for (int bb = 0; bb < B; ++bb) {
            const unsigned long long mask = __ballot(valid && b == bb);
            if (!mask) continue;
            for (int kb = 0; kb < K; kb += 64) {
                const bool on = kb + lane < K;
                const float *dk = D + (on ? kb + lane : 0) * RS_LD;
                double a = 0.0;
                unsigned long long mm = mask;
                while (mm) {
                    const int i0 = __builtin_ctzll(mm); mm &= mm - 1;
                    const bool h1 = mm != 0; const int i1 = h1 ? __builtin_ctzll(mm) : i0; mm &= mm - 1;
                    const bool h2 = mm != 0; const int i2 = h2 ? __builtin_ctzll(mm) : i0; mm &= mm - 1;
                    const bool h3 = mm != 0; const int i3 = h3 ? __builtin_ctzll(mm) : i0; mm &= mm - 1;
                    const float v0 = dk[i0], v1 = dk[i1], v2 = dk[i2], v3 = dk[i3];
                    a += (double)v0;
                    a += h1 ? (double)v1 : 0.0;
                    a += h2 ? (double)v2 : 0.0;
                    a += h3 ? (double)v3 : 0.0;
                }
                if (on) oacc[(kb + lane) * B + bb] += a;
            }
        }
        // ---- the rows of R, lanes over the clusters
        #pragma unroll 1
        for (int i = 0; i < nrow; ++i) {
            float *Ri = R + (row0 + i) * K;
            for (int kb = 0; kb < K; kb += 64)
                if (kb + lane < K) Ri[kb + lane] = D[(kb + lane) * RS_LD + i];
        }
        __syncthreads();
    }
    for (int e = lane; e < KB; e += 64) pO[(int64_t)blockIdx.x * KB + e] = oacc[e];
    sd = wave_sum_f64(sd);
    se = wave_sum_f64(se);
    if (lane == 0) {
        psum[(int64_t)blockIdx.x * 2 + 0] = sd;
        psum[(int64_t)blockIdx.x * 2 + 1] = se;
    }
}

// the work-groups' partials in ascending order: O_blk (K, B), then the two sums
__global__ void __launch_bounds__(256)
k_harmony_assign_reduce(double *__restrict__ O, double *__restrict__ sums, const double *__restrict__ pO, const double *__restrict__ psum,
                        int64_t bx, int64_t KB) {
    int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < KB) {
        double s = 0.0;
        for (int64_t x = 0; x < bx; ++x) s += pO[x * KB + e];
        O[e] = s;
        return;
    }
    e -= KB;
    if (e < 2) {
        double s = 0.0;
        for (int64_t x = 0; x < bx; ++x) s += psum[x * 2 + e];
        sums[e] = s;
    }
}

__global__ void __launch_bounds__(64)
k_harmony_moments(const float *__restrict__ X, int64_t n, int d, int64_t ldx, const float *__restrict__ R, int K,
                  const int32_t *__restrict__ batch, int B, double *__restrict__ part, int64_t tpb, int64_t ntiles, int nfb) {
    const int lane = (int)threadIdx.x;
    const int fb = (int)blockIdx.y % nfb, kc = (int)blockIdx.y / nfb;
    const int b = (int)blockIdx.z;
    const int f = fb * 64 + lane;
    const int k0 = kc * HM_KC;
    const bool isx = f < d, isone = f == d;
    int kk[HM_KC];
    #pragma unroll
    for (int j = 0; j < HM_KC; ++j) kk[j] = k0 + j < K ? k0 + j : K - 1;      // (a tail re-reads the last cluster; never stored)
    double dacc[HM_KC];
    #pragma unroll
    for (int j = 0; j < HM_KC; ++j) dacc[j] = 0.0;

    const int64_t t0 = (int64_t)blockIdx.x * tpb;
    const int64_t t1 = t0 + tpb < ntiles ? t0 + tpb : ntiles;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t row0 = t * RS_ROWS;
        const int nrow = n - row0 < RS_ROWS ? (int)(n - row0) : RS_ROWS;
        const int bv = lane < nrow ? batch[row0 + lane] : -1;
        unsigned long long mm = __ballot(bv == b);
        if (!mm) continue;
        while (mm) {
            float acc[HM_KC];
            #pragma unroll
            for (int j = 0; j < HM_KC; ++j) acc[j] = 0.0f;
            int iu[4] = {0, 0, 0, 0};
            bool hu[4];
            #pragma unroll
            for (int u = 0; u < 4; ++u) {
                hu[u] = mm != 0;
                iu[u] = hu[u] ? __builtin_ctzll(mm) : iu[0];
                mm &= mm - 1;
            }
            float x[4];
            #pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float v = isx ? X[(row0 + iu[u]) * ldx + f] : 0.0f;
                x[u] = hu[u] ? (isone ? 1.0f : v) : 0.0f;
            }
            #pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float *rr = R + (row0 + iu[u]) * K;
                #pragma unroll
                for (int j = 0; j < HM_KC; ++j) acc[j] = fmaf(rr[kk[j]], x[u], acc[j]);
            }
            #pragma unroll
            for (int j = 0; j < HM_KC; ++j) dacc[j] += (double)acc[j];
        }
    }
    if (f <= d) {
        #pragma unroll
        for (int j = 0; j < HM_KC; ++j)
            if (k0 + j < K) part[((((int64_t)blockIdx.x * K + k0 + j) * B + b) * (d + 1)) + f] = dacc[j];
    }
}

// the ranges' partials in ascending order: S (K, B, d) and O (K, B) from (bx, K, B, d + 1)
__global__ void __launch_bounds__(256)
k_harmony_moments_reduce(double *__restrict__ S, double *__restrict__ O, const double *__restrict__ part, int64_t bx, int64_t KB, int d) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t tot = KB * (d + 1);
    if (e >= tot) return;
    double s = 0.0;
    for (int64_t x = 0; x < bx; ++x) s += part[x * tot + e];
    const int f = (int)(e % (d + 1));
    const int64_t kb = e / (d + 1);
    if (f < d) S[kb * d + f] = s;
    else O[kb] = s;
}

__global__ void __launch_bounds__(64)
k_harmony_correct(const float *__restrict__ Z, int64_t n, int d, int64_t ldz, const float *__restrict__ R, int K,
                  const int32_t *__restrict__ batch, const float *__restrict__ wpad, float *__restrict__ Zcorr, float *__restrict__ Zcos,
                  int dp, int64_t tpb, int64_t ntiles) {
    extern __shared__ float hc_lds[];
    const int lane = (int)threadIdx.x;
    const int b = (int)blockIdx.y;
    float *Wb = hc_lds;                         // [K][dp]: W[:, b, :], zero where padded
    float *tile = Wb + K * dp;                  // [dp][65]: the corrected rows of this batch
    float *nrm = tile + dp * RS_LD;             // [64]
    {
        const float4 *src = reinterpret_cast<const float4 *>(wpad + (int64_t)b * K * dp);
        float4 *dst = reinterpret_cast<float4 *>(Wb);
        for (int e = lane; e < (K * dp) >> 2; e += 64) dst[e] = src[e];
    }
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * tpb;
    const int64_t t1 = t0 + tpb < ntiles ? t0 + tpb : ntiles;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t row0 = t * RS_ROWS;
        const int nrow = n - row0 < RS_ROWS ? (int)(n - row0) : RS_ROWS;
        const int bv = lane < nrow ? batch[row0 + lane] : -1;
        const unsigned long long mask = __ballot(bv == b);
        if (!mask) continue;
        // ---- z - sum_k R W: lane = feature, four rows share a read of W
        for (int f0 = 0; f0 < d; f0 += 64) {
            const int f = f0 + lane;
            const bool on = f < d;
            const float *wf = Wb + (on ? f : 0);
            unsigned long long mm = mask;
            while (mm) {
                int iu[4] = {0, 0, 0, 0};
                bool hu[4];
                #pragma unroll
                for (int u = 0; u < 4; ++u) {
                    hu[u] = mm != 0;
                    iu[u] = hu[u] ? __builtin_ctzll(mm) : iu[0];
                    mm &= mm - 1;
                }
                float z[4], s[4];
                #pragma unroll
                for (int u = 0; u < 4; ++u) {
                    z[u] = on ? Z[(row0 + iu[u]) * ldz + f] : 0.0f;
                    s[u] = 0.0f;
                }
                for (int k0 = 0; k0 < K; k0 += HM_CK) {
                    float r[4][HM_CK];
                    #pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float *rr = R + (row0 + iu[u]) * K;
                        #pragma unroll
                        for (int j = 0; j < HM_CK; ++j) {
                            const float v = rr[k0 + j < K ? k0 + j : K - 1];
                            r[u][j] = k0 + j < K ? v : 0.0f;
                        }
                    }
                    #pragma unroll
                    for (int j = 0; j < HM_CK; ++j) {
                        const float w = wf[(k0 + j < K ? k0 + j : K - 1) * dp];
                        #pragma unroll
                        for (int u = 0; u < 4; ++u) s[u] = fmaf(r[u][j], w, s[u]);
                    }
                }
                #pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (hu[u] && on) {
                        const float zc = z[u] - s[u];
                        Zcorr[(row0 + iu[u]) * d + f] = zc;
                        tile[f * RS_LD + iu[u]] = zc;
                    }
            }
        }
        __syncthreads();
        // ---- the norm: lane = row, one chain over the features
        if ((mask >> lane) & 1ull) {
            float a = 0.0f;
            for (int f = 0; f < d; ++f) {
                const float v = tile[f * RS_LD + lane];
                a = fmaf(v, v, a);
            }
            nrm[lane] = sqrtf(a);
        }
        __syncthreads();
        for (int f0 = 0; f0 < d; f0 += 64) {
            const int f = f0 + lane;
            if (f >= d) continue;
            unsigned long long mm = mask;
            while (mm) {
                const int i = __builtin_ctzll(mm); mm &= mm - 1;
                const float nr = nrm[i];
                Zcos[(row0 + i) * d + f] = nr > 0.0f ? tile[f * RS_LD + i] / nr : 0.0f;
            }
        }
        __syncthreads();
    }
}

struct HmAssignPlan { int64_t dp, Kp, off_pO, off_psum, total; HmRanges r; };
HmAssignPlan hm_assign_plan(int64_t n, int64_t d, int64_t K, int64_t B, int64_t blocks) {
    HmAssignPlan p;
    p.dp = pad4(d);
    p.Kp = (K + RS_CH - 1) / RS_CH * RS_CH;
    p.r = hm_ranges(n, blocks, 1, 4);
    p.off_pO = p.Kp * p.dp * 4;                         // (a multiple of 16 bytes)
    p.off_psum = p.off_pO + p.r.bx * K * B * 8;
    p.total = up16(p.off_psum + p.r.bx * 2 * 8);
    return p;
}

struct HmMomentsPlan { int64_t nfb, nkc, total; HmRanges r; };
HmMomentsPlan hm_moments_plan(int64_t n, int64_t d, int64_t K, int64_t B, int64_t blocks) {
    HmMomentsPlan p;
    p.nfb = (d + 1 + 63) / 64;
    p.nkc = (K + HM_KC - 1) / HM_KC;
    p.r = hm_ranges(n, blocks, p.nfb * p.nkc * B, 16);
    p.total = up16(p.r.bx * K * B * (d + 1) * 8);
    return p;
}

inline int hm_check_sizes(int64_t n, int64_t d, int64_t K, int64_t B, int64_t blocks) {
    if (n < 0 || d < 1 || K < 1 || B < 1 || blocks < 0) return ORIANA_EINVAL;
    if (d > RS_MAX_D || B > HM_MAX_B || K > hm_max_clusters(d)) return ORIANA_EKRANGE;
    if (n > 0x7fffffffLL - RS_ROWS) return ORIANA_EINVAL;
    return 0;
}

}  // namespace
}  // namespace oriana

using namespace oriana;

extern "C" int64_t oriana_harmony_max_clusters(int64_t d) {
    if (d < 1 || d > RS_MAX_D) return 0;
    return hm_max_clusters(d);
}

extern "C" int64_t oriana_harmony_max_batches(void) { return HM_MAX_B; }

extern "C" int64_t oriana_harmony_partial_rows(void) { return HM_T; }

extern "C" int64_t oriana_harmony_assign_scratch_bytes(int64_t n, int64_t d, int64_t K, int64_t B, int64_t blocks) {
    const int rc = hm_check_sizes(n, d, K, B, blocks);
    if (rc) return rc;
    return hm_assign_plan(n, d, K, B, blocks).total;
}

extern "C" int64_t oriana_harmony_moments_scratch_bytes(int64_t n, int64_t d, int64_t K, int64_t B, int64_t blocks) {
    const int rc = hm_check_sizes(n, d, K, B, blocks);
    if (rc) return rc;
    return hm_moments_plan(n, d, K, B, blocks).total;
}

extern "C" int64_t oriana_harmony_correct_scratch_bytes(int64_t n, int64_t d, int64_t K, int64_t B, int64_t blocks) {
    const int rc = hm_check_sizes(n, d, K, B, blocks);
    if (rc) return rc;
    return B * K * pad4(d) * 4;
}

extern "C" int oriana_harmony_assign(const float *Z, int64_t n, int64_t d, int64_t ldz, const int32_t *batch, const float *centers,
                                     int64_t K, const float *P, int64_t B, double inv_sigma, float *R, double *O_blk, double *sums,
                                     void *scratch, int64_t blocks, void *stream) {
    int rc = hm_check_sizes(n, d, K, B, blocks);
    if (rc) return rc;
    if (ldz < d || !(inv_sigma > 0.0) || !(inv_sigma < 1e30)) return ORIANA_EINVAL;
    if (!centers || !P || !O_blk || !sums || !scratch || (n > 0 && (!Z || !batch || !R))) return ORIANA_EINVAL;
    if ((uintptr_t)scratch & 15) return ORIANA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        ORIANA_HIP_CHECK(hipMemsetAsync(O_blk, 0, (size_t)(K * B) * 8, st));
        ORIANA_HIP_CHECK(hipMemsetAsync(sums, 0, 16, st));
        return 0;
    }
    const HmAssignPlan p = hm_assign_plan(n, d, K, B, blocks);
    char *base = static_cast<char *>(scratch);
    float *cpad = reinterpret_cast<float *>(base);
    double *pO = reinterpret_cast<double *>(base + p.off_pO);
    double *psum = reinterpret_cast<double *>(base + p.off_psum);
    const int64_t npad = p.Kp * p.dp;
    rc = launch(k_harmony_pad, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, st, cpad, centers, (int)K, (int)d, (int)p.Kp, (int)p.dp,
                0, npad);
    if (rc) return rc;
    const float cexp = (float)(-inv_sigma * 1.4426950408889634);
    rc = launch(k_harmony_assign, dim3((unsigned)p.r.bx), dim3(64), (size_t)hm_assign_lds(p.dp, K, B), st, Z, n, (int)d, ldz, batch, cpad,
                (int)K, P, (int)B, cexp, R, pO, psum, (int)p.r.tpb);
    if (rc) return rc;
    const int64_t nout = K * B + 2;
    return launch(k_harmony_assign_reduce, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, O_blk, sums, pO, psum, p.r.bx, K * B);
}

extern "C" int oriana_harmony_moments(const float *X, int64_t n, int64_t d, int64_t ldx, const float *R, int64_t K, const int32_t *batch,
                                      int64_t B, double *S, double *O, void *scratch, int64_t blocks, void *stream) {
    int rc = hm_check_sizes(n, d, K, B, blocks);
    if (rc) return rc;
    if (ldx < d) return ORIANA_EINVAL;
    if (!S || !O || !scratch || (n > 0 && (!X || !R || !batch))) return ORIANA_EINVAL;
    if ((uintptr_t)scratch & 15) return ORIANA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        ORIANA_HIP_CHECK(hipMemsetAsync(S, 0, (size_t)(K * B * d) * 8, st));
        ORIANA_HIP_CHECK(hipMemsetAsync(O, 0, (size_t)(K * B) * 8, st));
        return 0;
    }
    const HmMomentsPlan p = hm_moments_plan(n, d, K, B, blocks);
    if (p.nfb * p.nkc > 65535) return ORIANA_EINVAL;
    double *part = static_cast<double *>(scratch);
    rc = launch(k_harmony_moments, dim3((unsigned)p.r.bx, (unsigned)(p.nfb * p.nkc), (unsigned)B), dim3(64), 0, st, X, n, (int)d, ldx, R,
                (int)K, batch, (int)B, part, p.r.tpb, p.r.ntiles, (int)p.nfb);
    if (rc) return rc;
    const int64_t nout = K * B * (d + 1);
    return launch(k_harmony_moments_reduce, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, S, O, part, p.r.bx, K * B, (int)d);
}

extern "C" int oriana_harmony_correct(const float *Z, int64_t n, int64_t d, int64_t ldz, const float *R, int64_t K, const int32_t *batch,
                                      const float *W, int64_t B, float *Zcorr, float *Zcos, void *scratch, int64_t blocks, void *stream) {
    int rc = hm_check_sizes(n, d, K, B, blocks);
    if (rc) return rc;
    if (ldz < d) return ORIANA_EINVAL;
    if (!W || !scratch || (n > 0 && (!Z || !R || !batch || !Zcorr || !Zcos))) return ORIANA_EINVAL;
    if ((uintptr_t)scratch & 15) return ORIANA_EINVAL;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t dp = pad4(d);
    const HmRanges r = hm_ranges(n, blocks, B, 4);
    float *wpad = static_cast<float *>(scratch);
    const int64_t npad = B * K * dp;
    rc = launch(k_harmony_pad, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, st, wpad, W, (int)K, (int)d, (int)K, (int)dp, (int)B, npad);
    if (rc) return rc;
    return launch(k_harmony_correct, dim3((unsigned)r.bx, (unsigned)B), dim3(64), (size_t)hm_correct_lds(dp, K), st, Z, n, (int)d, ldz, R,
                  (int)K, batch, wpad, Zcorr, Zcos, (int)dp, r.tpb, r.ntiles);
}
