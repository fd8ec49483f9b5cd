// updates.hip -- Gamma shape/rate updates, Gamma expectations and the M-step on gfx950.
//
// Replaces the (n + m) * K NumPy statements of update_variational_parameters /
// update_prior_hyper_parameters (oriana/models/gap.py:96-129 and the three twins) together with
// Gamma.mean / Gamma.meanlog (oriana/nodes/probabilistic/gamma.py:37-61) and the special functions
// of oriana/utils.py.  All of it is float64 element-wise work plus column sums: HBM-bound,
// fused so that each parameter matrix is written once and Z is read once.
#include "common.h"

namespace oriana {

// blockDim = (KT, RY): thread (tx, ty) handles columns tx, tx + KT, ... of rows ty, ty + RY, ...
// inside the block's row strip.  Column sums are carried per thread in f64, reduced over ty in
// LDS and added to the global K-vectors with one f64 atomic per column per block.
constexpr int GU_ROWS_PER_BLOCK = 512;        // upper bound; rows_per_block() picks fewer for short matrices
constexpr int GU_MAXCOLS_PER_THREAD = 4;     // K <= 4 * 128

// FIN: the last step of the responsibility pass (oriana_finalize: Z[o] += F[p] * R[p], o = row_index[p]) is folded in:
// the rows are walked in PACKED order p, Z is completed in place (it stays a full output) and used at once.
// NT: threads per work-group.  Every group ends with 2K float64 atomics on the SAME 2K addresses, which the memory
// side serialises (measured: 26 ns per group; a row of a thread is 0.8 us of dependent loads): a short matrix takes few,
// large groups (1024 threads, 79 of them at 10,000 rows: 17.6 -> ~10 us), a long one many small groups.
template <bool FIN, int NT>
__global__ __launch_bounds__(NT) void k_gamma_update(double *__restrict__ a1, double *__restrict__ a2,
                                                      double *__restrict__ E, float *__restrict__ Elog,
                                                      double *__restrict__ colsum_E, double *__restrict__ colsum_Elog,
                                                      const double *__restrict__ prior1, const double *__restrict__ prior2,
                                                      const float *__restrict__ Z_in, const float *__restrict__ zmul,
                                                      const double *__restrict__ rate_vec,
                                                      const double *__restrict__ rate_mat,
                                                      const float *__restrict__ rmul, int64_t r, int K, int rpb,
                                                      float *__restrict__ Zfin, const float *__restrict__ F,
                                                      const float *__restrict__ Rs, const int32_t *__restrict__ row_index,
                                                      int Kp, int nslab, int64_t slab_row0) {
    const float *Z = FIN ? Zfin : Z_in;
    __shared__ double red[2][NT];
    const int KT = blockDim.x, RY = blockDim.y;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * rpb;
    const int64_t r1 = (r0 + rpb < r) ? r0 + rpb : r;
    double sE[GU_MAXCOLS_PER_THREAD], sL[GU_MAXCOLS_PER_THREAD];
    #pragma unroll
    for (int c = 0; c < GU_MAXCOLS_PER_THREAD; ++c) { sE[c] = 0.0; sL[c] = 0.0; }

    for (int64_t row = r0 + ty; row < r1; row += RY) {
        const int64_t orow = (FIN && row_index) ? (int64_t)row_index[row] : row;
        #pragma unroll
        for (int c = 0; c < GU_MAXCOLS_PER_THREAD; ++c) {
            const int k = tx + c * KT;
            if (k < K) {
                const int64_t idx = orow * K + k;
                double s1, s2;
                if (FIN) {
                    float rr = Rs[row * Kp + k];
                    const int ns = row >= slab_row0 ? nslab : 1;
                    for (int sl = 1; sl < ns; ++sl) rr += Rs[((int64_t)sl * (r - slab_row0) + row) * Kp + k];
                    const float zf = fmaf(F[row * Kp + k], rr, Zfin[idx]) + 0.0f;                  // k_finalize (accumulate)
                    Zfin[idx] = zf;
                    s1 = clamp_eps(prior1[k] + (double)zf);
                    s2 = clamp_eps(prior2[k] + rate_vec[k]);
                    a1[idx] = s1;
                    a2[idx] = s2;
                } else if (Z) {
                    double z = (double)Z[idx];
                    if (zmul) z = (double)(zmul[idx] * Z[idx]);          // f32 product, as S_hat * Z_hat_j
                    s1 = clamp_eps(prior1[k] + z);
                    double rt = rate_mat ? rate_mat[idx] : rate_vec[k];
                    if (rmul) rt = (double)rmul[idx] * rt;
                    s2 = clamp_eps(prior2[k] + rt);
                    a1[idx] = s1;
                    a2[idx] = s2;
                } else {
                    s1 = a1[idx];
                    s2 = a2[idx];
                }
                const double e = s1 / s2;                                // gamma.py:37-46
                const float el = gamma_meanlog_f32(s1, s2);              // gamma.py:52-61
                E[idx] = e;
                Elog[idx] = el;
                sE[c] += e;
                sL[c] += (double)el;
            }
        }
    }
    // reduce over ty: inside a wave first (KT <= 32: lanes l, l + KT, ... hold the same column), then over the waves
    // through LDS -- at most NT / 64 terms per column for the thread that issues the atomics
    const int flat = ty * KT + tx, lane = flat & 63, wv = flat >> 6, NW = NT / 64;
    const int kw = KT < 64 ? KT : 64;                  // distinct columns inside a wave
    #pragma unroll
    for (int c = 0; c < GU_MAXCOLS_PER_THREAD; ++c) {
        if (c * KT >= K) break;                        // (uniform: no thread holds a column of this round)
        const int k = tx + c * KT;
        double vE = sE[c], vL = sL[c];
        for (int off = kw; off < 64; off <<= 1) { vE += __shfl_xor(vE, off); vL += __shfl_xor(vL, off); }
        __syncthreads();
        if (lane < kw) {
            // column of this lane inside the round: tx for KT <= 64; for KT = 128 a wave covers half of the columns
            red[0][wv * kw + lane] = vE;
            red[1][wv * kw + lane] = vL;
        }
        __syncthreads();
        if (ty == 0 && k < K) {
            double tE = 0.0, tL = 0.0;
            if (KT <= 64) {
                for (int w = 0; w < NW; ++w) { tE += red[0][w * kw + tx]; tL += red[1][w * kw + tx]; }
            } else {
                // KT = 128: rows of threads span two waves; wave 2y + (tx >> 6) holds columns (tx & 63) of row y
                for (int w = (tx >> 6); w < NW; w += 2) { tE += red[0][w * kw + (tx & 63)]; tL += red[1][w * kw + (tx & 63)]; }
            }
            if (colsum_E) atomicAdd(&colsum_E[k], tE);
            if (colsum_Elog) atomicAdd(&colsum_Elog[k], tL);
        }
    }
}

// ------------------------------------------------------------------------------------------
// [r5] The same update, VEC consecutive factors per lane and LPR lanes per row (a power of two >= K / VEC; 64 / LPR rows
// per wave and iteration): every access is a 4 * VEC (float32) or 8 * VEC (float64) byte piece per lane, the pieces of a row
// contiguous -- round 4's kernel gave each lane ONE element per row (512- and 288-byte wave stores at K = 100 that
// straddle the 128-byte lines: 2.3 TB/s for 4.4 GB).  Needs K % VEC == 0 (row starts stay aligned).
//
// PREP outputs (FUn != NULL), the cell-side half of the NEXT sweep's factor preparation: the row's K values of E[log .] are in
// the row's LPR lanes anyway, so the row maximum, F = exp(E[log .] - max) and the per-group partial statistics of the maxima
// (k_row_stats) cost no extra read: FUn (r, Kp) gets the row in the arithmetic of factor_prep_row (padding columns are never
// written: the buffer is zero-filled once), mu_out[r] the maximum (NaN if the row holds a NaN), upart[4 b ..] = {sum, sum of
// squares, count, min} of group b's maxima.  The validity test needs the statistics of ALL rows, i.e. the end of this
// launch: the next sweep's preparation applies it to mu_out and overwrites the rejected rows (k_factor_prep_pair, fix mode).
struct GuVecArgs {
    double *a1, *a2, *E;
    float *Elog;
    double *colsum_E, *colsum_Elog;
    const double *prior1, *prior2;
    const float *Z_in, *zmul;
    const double *rate_vec, *rate_mat;
    const float *rmul;
    int64_t r;
    int K, rpb;
    float *Zfin;
    const float *F, *Rs;
    const int32_t *row_index;
    int Kp, nslab;
    int64_t slab_row0;
    float *FUn, *mu_out, *upart;
    double *a2row;      // [r6] FIN, a2 == NULL: the K rate values every row shares (gap.py:98: alpha2 + sum_j V_hat), written once
};

template <int VEC> struct VecF;
template <> struct VecF<1> { typedef float T; };
template <> struct VecF<2> { typedef float T __attribute__((ext_vector_type(2))); };
template <> struct VecF<4> { typedef float T __attribute__((ext_vector_type(4))); };
typedef double d2 __attribute__((ext_vector_type(2)));

template <int VEC>
__device__ __forceinline__ void ld_f32(float (&o)[VEC], const float *p) {
    typedef typename VecF<VEC>::T V;
    const V v = *reinterpret_cast<const V *>(p);
    if constexpr (VEC == 1) o[0] = v;
    else { _Pragma("unroll") for (int i = 0; i < VEC; ++i) o[i] = v[i]; }
}
template <int VEC>
__device__ __forceinline__ void st_f32(float *p, const float (&o)[VEC]) {
    typedef typename VecF<VEC>::T V;
    V v;
    if constexpr (VEC == 1) v = o[0];
    else { _Pragma("unroll") for (int i = 0; i < VEC; ++i) v[i] = o[i]; }
    *reinterpret_cast<V *>(p) = v;
}
template <int VEC>
__device__ __forceinline__ void ld_f64(double (&o)[VEC], const double *p) {
    if constexpr (VEC == 1) o[0] = *p;
    else { _Pragma("unroll") for (int i = 0; i < VEC; i += 2) { const d2 v = *reinterpret_cast<const d2 *>(p + i); o[i] = v[0]; o[i + 1] = v[1]; } }
}
template <int VEC>
__device__ __forceinline__ void st_f64(double *p, const double (&o)[VEC]) {
    if constexpr (VEC == 1) *p = o[0];
    else { _Pragma("unroll") for (int i = 0; i < VEC; i += 2) { d2 v; v[0] = o[i]; v[1] = o[i + 1]; *reinterpret_cast<d2 *>(p + i) = v; } }
}

// gamma_meanlog_f32 with logf(f32(a2)) given (the pCMF cell / gene side: a2 is one value per factor)
__device__ __forceinline__ float gamma_meanlog_f32_lg(double a1, float lg) {
    const float a1f = (float)a1;
    float psi;
    if (a1f > 0.0f && a1f < INFINITY) psi = (float)digamma_pos_for_f32((double)a1f);
    else psi = (float)digamma_f64((double)a1f);
    return psi - lg;
}

template <bool FIN, int VEC, int LPR>
__global__ __launch_bounds__(256) void k_gamma_update_vec(const GuVecArgs A) {
    constexpr int RPW = 64 / LPR, NW = 4, NCOL = LPR * VEC;
    __shared__ double red[2][NW][NCOL];
    __shared__ float sred[4][NW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int cg = lane & (LPR - 1), sr = lane / LPR;
    const int k0 = cg * VEC, K = A.K, Kp = A.Kp;
    const bool act = k0 < K;
    const int64_t r = A.r;
    const int64_t r0 = (int64_t)blockIdx.x * A.rpb;
    const int64_t r1 = (r0 + A.rpb < r) ? r0 + A.rpb : r;
    const bool prep = A.FUn != nullptr;
    const bool upd = FIN || A.Z_in != nullptr;
    double p1[VEC], p2[VEC], rv[VEC], s2c[VEC], sE[VEC], sL[VEC];
    float lg2c[VEC];
    #pragma unroll
    for (int v = 0; v < VEC; ++v) {
        p1[v] = (act && upd) ? A.prior1[k0 + v] : 1.0;
        p2[v] = (act && upd) ? A.prior2[k0 + v] : 1.0;
        rv[v] = (act && A.rate_vec) ? A.rate_vec[k0 + v] : 0.0;
        s2c[v] = clamp_eps(p2[v] + rv[v]);
        lg2c[v] = logf((float)s2c[v]);
        sE[v] = 0.0; sL[v] = 0.0;
    }
    float st_sum = 0.f, st_sq = 0.f, st_cnt = 0.f, st_min = INFINITY;
    for (int64_t rb = r0 + w * RPW; rb < r1; rb += NW * RPW) {
        const int64_t row = rb + sr;
        const bool in = act && row < r1;
        float el[VEC];
        #pragma unroll
        for (int v = 0; v < VEC; ++v) el[v] = -INFINITY;
        if (in) {
            const int64_t orow = (FIN && A.row_index) ? (int64_t)A.row_index[row] : row;
            const int64_t idx = orow * K + k0;
            double s1[VEC], s2[VEC], e[VEC];
            if (FIN) {
                float rr[VEC], f[VEC], z[VEC];
                ld_f32<VEC>(rr, A.Rs + row * Kp + k0);
                ld_f32<VEC>(f, A.F + row * Kp + k0);
                ld_f32<VEC>(z, A.Zfin + idx);
                const int ns = row >= A.slab_row0 ? A.nslab : 1;
                for (int sl = 1; sl < ns; ++sl) {
                    float r2[VEC];
                    ld_f32<VEC>(r2, A.Rs + ((int64_t)sl * (r - A.slab_row0) + row) * Kp + k0);
                    #pragma unroll
                    for (int v = 0; v < VEC; ++v) rr[v] += r2[v];
                }
                #pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    z[v] = fmaf(f[v], rr[v], z[v]) + 0.0f;                                  // k_finalize (accumulate)
                    s1[v] = clamp_eps(p1[v] + (double)z[v]);
                    s2[v] = s2c[v];
                }
                st_f32<VEC>(A.Zfin + idx, z);
                st_f64<VEC>(A.a1 + idx, s1);
                if (A.a2) st_f64<VEC>(A.a2 + idx, s2);
                #pragma unroll
                for (int v = 0; v < VEC; ++v)
                    el[v] = gamma_meanlog_f32_lg(s1[v], lg2c[v]);
            } else if (A.Z_in) {
                float z[VEC];
                ld_f32<VEC>(z, A.Z_in + idx);
                if (A.zmul) {
                    float zm[VEC];
                    ld_f32<VEC>(zm, A.zmul + idx);
                    #pragma unroll
                    for (int v = 0; v < VEC; ++v) z[v] = zm[v] * z[v];                        // f32 product, as S_hat * Z_hat_j
                }
                double rt[VEC];
                if (A.rate_mat) ld_f64<VEC>(rt, A.rate_mat + idx);
                else { _Pragma("unroll") for (int v = 0; v < VEC; ++v) rt[v] = rv[v]; }
                if (A.rmul) {
                    float rm[VEC];
                    ld_f32<VEC>(rm, A.rmul + idx);
                    #pragma unroll
                    for (int v = 0; v < VEC; ++v) rt[v] = (double)rm[v] * rt[v];
                }
                #pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    s1[v] = clamp_eps(p1[v] + (double)z[v]);
                    s2[v] = clamp_eps(p2[v] + rt[v]);
                }
                st_f64<VEC>(A.a1 + idx, s1);
                st_f64<VEC>(A.a2 + idx, s2);
                #pragma unroll
                for (int v = 0; v < VEC; ++v) el[v] = gamma_meanlog_f32(s1[v], s2[v]);
            } else {
                ld_f64<VEC>(s1, A.a1 + idx);
                ld_f64<VEC>(s2, A.a2 + idx);
                #pragma unroll
                for (int v = 0; v < VEC; ++v) el[v] = gamma_meanlog_f32(s1[v], s2[v]);
            }
            #pragma unroll
            for (int v = 0; v < VEC; ++v) {
                e[v] = s1[v] / s2[v];                                                       // gamma.py:37-46
                sE[v] += e[v];
                sL[v] += (double)el[v];
            }
            if (A.E) st_f64<VEC>(A.E + idx, e);
            st_f32<VEC>(A.Elog + idx, el);
        }
        if (prep) {
            // (wave-uniform: every lane takes part in the row's reduction; lanes beyond K or beyond the last row hold -inf)
            float mx = -INFINITY;
            bool bad = false;
            #pragma unroll
            for (int v = 0; v < VEC; ++v) { if (el[v] != el[v]) bad = true; mx = fmaxf(mx, el[v]); }
            static_assert(LPR >= 8, "lanes_max / lanes_or reduce over groups of at least 8 lanes");
            mx = lanes_max<LPR>(mx);                           // (DPP / permlane swaps: ten ds_bpermute per row pair before)
            const int badi = (int)lanes_or<LPR>(bad ? 1u : 0u);
            if (in) {
                float fu[VEC];
                #pragma unroll
                for (int v = 0; v < VEC; ++v)
                    fu[v] = (float)exp((double)el[v] - (double)mx);
                st_f32<VEC>(A.FUn + row * Kp + k0, fu);
                if (cg == 0) {
                    A.mu_out[row] = badi ? NAN : mx;
                    if (!badi) {
                        if (fabsf(mx) <= STAT_MAX) { st_sum += mx; st_sq += mx * mx; st_cnt += 1.f; }          // as k_row_stats
                        st_min = fminf(st_min, mx);
                    }
                }
            }
        }
    }
    // column sums: lanes holding the same factors inside the wave, then the four waves through LDS
    #pragma unroll
    for (int v = 0; v < VEC; ++v) {
        double vE = sE[v], vL = sL[v];
        #pragma unroll
        for (int o = LPR; o < 64; o <<= 1) { vE += __shfl_xor(vE, o, 64); vL += __shfl_xor(vL, o, 64); }
        if (sr == 0) { red[0][w][k0 + v] = vE; red[1][w][k0 + v] = vL; }
    }
    if (prep) {
        st_sum = wave_sum(st_sum); st_sq = wave_sum(st_sq); st_cnt = wave_sum(st_cnt); st_min = -wave_max(-st_min);
        if (lane == 0) { sred[0][w] = st_sum; sred[1][w] = st_sq; sred[2][w] = st_cnt; sred[3][w] = st_min; }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) {
        const double tE = ((red[0][0][k] + red[0][1][k]) + red[0][2][k]) + red[0][3][k];
        const double tL = ((red[1][0][k] + red[1][1][k]) + red[1][2][k]) + red[1][3][k];
        if (A.colsum_E) atomicAdd(&A.colsum_E[k], tE);
        if (A.colsum_Elog) atomicAdd(&A.colsum_Elog[k], tL);
    }
    if (FIN && A.a2row && blockIdx.x == 0 && w == 0 && sr == 0 && act) st_f64<VEC>(A.a2row + k0, s2c);
    if (prep && threadIdx.x == 0) {
        float *pp = A.upart + 4 * (size_t)blockIdx.x;
        pp[0] = ((sred[0][0] + sred[0][1]) + sred[0][2]) + sred[0][3];
        pp[1] = ((sred[1][0] + sred[1][1]) + sred[1][2]) + sred[1][3];
        pp[2] = ((sred[2][0] + sred[2][1]) + sred[2][2]) + sred[2][3];
        pp[3] = fminf(fminf(sred[3][0], sred[3][1]), fminf(sred[3][2], sred[3][3]));
    }
}

// ------------------------------------------------------------------------------------------
// The step between two row passes of a FOLD-IN (models/gap.py transform: new cells against a frozen gene side): the cell
// side of k_gamma_update_vec<FIN> with everything a fold-in has no use for left out -- no a2 / U_hat stores, no column sums,
// Z is read (the slow path's additions) and not written back -- and a per-cell convergence test in their place.  Per row, in
// packed order (o = row_index[p]):
//   a1_new = max(1e-15, alpha1 + Z[o] + F[p] * sum_slabs R[p]);   still = exists k: !(|a1_new - a1| <= tol * a1)
//   active[o] && !still : the cell FREEZES -- active[o] = 0, froze_at[o] = it; nothing else of the row is written, now or later
//   active[o] && still  : a1[o] = a1_new, Elog[o] = f32(psi(f32(a1_new))) - logf(f32(a2_row)) (gamma_meanlog_f32_lg: the cast
//                         of the sweep) MINUS ITS ROW MAXIMUM, and the PREP outputs of k_gamma_update_vec: FUn[p], mu[p] (= 0),
//                         the statistics partials.
// The row maximum: the responsibilities are a softmax over the factors, which a shift of the cell's whole row leaves as it is.
// A sweep stores E[log U] unshifted (the M-step reads it) and its slow path restates the reference's float32 exp(lu + lv), which
// underflows to r = 0 for a cell whose every E[log U] is below ~-100 (a shape near the clamp: psi(1e-15) = -1e15) -- such a
// cell would never leave alpha1.  Nothing but the next row phase reads a fold-in's E[log U], so it is stored with maximum 0:
// FUn = exp(E[log U] - max) is the same numbers, every row passes the validity test, and the slow path's exponentials of
// the factors that carry the cell's mass are of order exp(lv).
// The statistics of the validity test cover ALL rows: a frozen row enters with the maximum it stored last (mu[p] is read back).
// FUn may be the buffer F points to (every lane reads its own elements of a row before it writes them; no other kernel reads
// F meanwhile -- a fold-in has no column pass).  n_active += the rows still active: one atomic per work-group.
// R == NULL is the START: a1 is taken as it is and every active row gets Elog, FUn and mu from it (no test, no counter).
// NC pieces of VEC factors per lane, LPR lanes per row: NC = 1 are the configurations of gu_vec_cfg; <1, 64, 4> -- a wave per
// row, element accesses -- serves the K and the pointers those leave out (odd K above 64, unaligned buffers).
struct FoldinArgs {
    double *a1;
    float *Elog;
    uint8_t *active;
    int32_t *froze_at, *n_active;
    const double *alpha1, *a2_row;
    const float *Z, *F, *R;
    const int32_t *row_index;
    float *FUn, *mu, *upart;
    int64_t r, slab_row0;
    int K, Kp, nslab, rpb, it;
    double tol;
    // ZI (the zero-inflated fold-in, oriana_foldin_update_zi): the rate is a MATRIX -- a2 (r, K) read and written, rate (r, K) =
    // sum_j d_ij V_hat_jk of the pair that enters the iteration, alpha2 [K], U_hat (r, K) = a1 / a2 out; all in the caller's
    // row order, like a1.  a2_row is not read.
    double *a2;
    const double *rate, *alpha2;
    double *U_hat;
};

// ZI: a2_new = max(1e-15, alpha2 + rate[o]), a cell freezes when BOTH |a1_new - a1| <= tol * a1 and |a2_new - a2| <= tol * a2
// hold in every factor, E[log U] takes logf(f32(a2_new)) of the cell's own rate, and a cell still active also gets a2[o] and
// U_hat[o] = a1_new / a2_new (the operand of the next oriana_zi_foldin_rate).  The start form writes U_hat from the pair as given.
template <int VEC, int LPR, int NC, bool ZI = false>
__global__ __launch_bounds__(256) void k_foldin_update(const FoldinArgs A) {
    constexpr int RPW = 64 / LPR, NW = 4;
    static_assert(LPR >= 8, "lanes_max / lanes_or reduce over groups of at least 8 lanes");
    __shared__ float sred[5][NW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int cg = lane & (LPR - 1), sr = lane / LPR;
    const int K = A.K, Kp = A.Kp;
    const int64_t r = A.r;
    const int64_t r0 = (int64_t)blockIdx.x * A.rpb;
    const int64_t r1 = (r0 + A.rpb < r) ? r0 + A.rpb : r;
    const bool start = A.R == nullptr;
    // the K-vectors, once per work-group: this lane's factors of alpha1 and of log a2
    double p1[NC][VEC], p2[ZI ? NC : 1][VEC];
    float lg[NC][VEC];
    #pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int k0 = (cg + c * LPR) * VEC;
        #pragma unroll
        for (int v = 0; v < VEC; ++v) {
            p1[c][v] = (k0 < K && !start) ? A.alpha1[k0 + v] : 1.0;
            if constexpr (ZI) { p2[c][v] = (k0 < K && !start) ? A.alpha2[k0 + v] : 1.0; lg[c][v] = 0.0f; }
            else lg[c][v] = k0 < K ? logf((float)A.a2_row[k0 + v]) : 0.0f;
        }
    }
    float st_sum = 0.f, st_sq = 0.f, st_cnt = 0.f, st_min = INFINITY, n_still = 0.f;
    for (int64_t rb = r0 + w * RPW; rb < r1; rb += NW * RPW) {
        const int64_t row = rb + sr;
        const bool inr = row < r1;
        const int64_t orow = inr ? (A.row_index ? (int64_t)A.row_index[row] : row) : 0;
        const bool was = inr && A.active[orow] != 0;
        double s1[NC][VEC], s2[ZI ? NC : 1][VEC];
        float el[NC][VEC];
        bool moved = false;
        #pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int k0 = (cg + c * LPR) * VEC;
            #pragma unroll
            for (int v = 0; v < VEC; ++v) { el[c][v] = -INFINITY; s1[c][v] = 1.0; }
            if constexpr (ZI) { _Pragma("unroll") for (int v = 0; v < VEC; ++v) s2[c][v] = 1.0; }
            if (was && k0 < K) {
                double old[VEC];
                ld_f64<VEC>(old, A.a1 + orow * K + k0);
                if constexpr (ZI) {
                    double old2[VEC];
                    ld_f64<VEC>(old2, A.a2 + orow * K + k0);
                    if (start) {
                        #pragma unroll
                        for (int v = 0; v < VEC; ++v) s2[c][v] = old2[v];
                    } else {
                        double rt[VEC];
                        ld_f64<VEC>(rt, A.rate + orow * K + k0);
                        #pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            s2[c][v] = clamp_eps(p2[c][v] + rt[v]);
                            if (!(fabs(s2[c][v] - old2[v]) <= A.tol * old2[v])) moved = true;
                        }
                    }
                    #pragma unroll
                    for (int v = 0; v < VEC; ++v) lg[c][v] = logf((float)s2[c][v]);
                }
                if (start) {
                    #pragma unroll
                    for (int v = 0; v < VEC; ++v) s1[c][v] = old[v];
                    moved = true;
                } else {
                    float rr[VEC], f[VEC], z[VEC];
                    ld_f32<VEC>(rr, A.R + row * Kp + k0);
                    ld_f32<VEC>(f, A.F + row * Kp + k0);
                    ld_f32<VEC>(z, A.Z + orow * K + k0);
                    const int ns = row >= A.slab_row0 ? A.nslab : 1;
                    for (int sl = 1; sl < ns; ++sl) {
                        float r2[VEC];
                        ld_f32<VEC>(r2, A.R + ((int64_t)sl * (r - A.slab_row0) + row) * Kp + k0);
                        #pragma unroll
                        for (int v = 0; v < VEC; ++v) rr[v] += r2[v];
                    }
                    #pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const float zf = fmaf(f[v], rr[v], z[v]) + 0.0f;                        // k_finalize (accumulate)
                        s1[c][v] = clamp_eps(p1[c][v] + (double)zf);
                        if (!(fabs(s1[c][v] - old[v]) <= A.tol * old[v])) moved = true;
                    }
                }
                #pragma unroll
                for (int v = 0; v < VEC; ++v) el[c][v] = gamma_meanlog_f32_lg(s1[c][v], lg[c][v]);
            }
        }
        // (wave-uniform from here: every lane takes part in its row's reductions; lanes beyond K, of a frozen row or beyond
        //  the last row hold -inf)
        const bool write = was && lanes_or<LPR>(moved ? 1u : 0u) != 0u;
        float mx = -INFINITY;
        bool bad = false;
        #pragma unroll
        for (int c = 0; c < NC; ++c) {
            #pragma unroll
            for (int v = 0; v < VEC; ++v) { if (el[c][v] != el[c][v]) bad = true; mx = fmaxf(mx, el[c][v]); }
        }
        mx = lanes_max<LPR>(mx);
        const int badi = (int)lanes_or<LPR>(bad ? 1u : 0u);
        if (write) {
            #pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int k0 = (cg + c * LPR) * VEC;
                if (k0 < K) {
                    float fu[VEC];
                    #pragma unroll
                    for (int v = 0; v < VEC; ++v) fu[v] = (float)exp((double)el[c][v] - (double)mx);
                    // (E[log U] goes out MINUS its row maximum, see above; a row with a NaN as it is)
                    float els[VEC];
                    #pragma unroll
                    for (int v = 0; v < VEC; ++v) els[v] = badi ? el[c][v] : el[c][v] - mx;
                    if (!start) st_f64<VEC>(A.a1 + orow * K + k0, s1[c]);
                    if constexpr (ZI) {
                        double e[VEC];
                        #pragma unroll
                        for (int v = 0; v < VEC; ++v) e[v] = s1[c][v] / s2[c][v];                   // gamma.py:37-46
                        if (!start) st_f64<VEC>(A.a2 + orow * K + k0, s2[c]);
                        st_f64<VEC>(A.U_hat + orow * K + k0, e);
                    }
                    st_f32<VEC>(A.Elog + orow * K + k0, els);
                    st_f32<VEC>(A.FUn + row * Kp + k0, fu);
                }
            }
        }
        if (inr && cg == 0) {
            float m1;
            if (write) {
                m1 = badi ? NAN : 0.0f;                             // (the maximum of what was stored)
                A.mu[row] = m1;
                n_still += 1.f;
            } else {
                m1 = A.mu[row];                                     // a frozen row: the maximum of its last update
                if (was) { A.active[orow] = 0; A.froze_at[orow] = A.it; }
            }
            if (m1 == m1) {
                if (fabsf(m1) <= STAT_MAX) { st_sum += m1; st_sq += m1 * m1; st_cnt += 1.f; }                  // as k_row_stats
                st_min = fminf(st_min, m1);
            }
        }
    }
    st_sum = wave_sum(st_sum); st_sq = wave_sum(st_sq); st_cnt = wave_sum(st_cnt); st_min = -wave_max(-st_min);
    n_still = wave_sum(n_still);
    if (lane == 0) { sred[0][w] = st_sum; sred[1][w] = st_sq; sred[2][w] = st_cnt; sred[3][w] = st_min; sred[4][w] = n_still; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float *pp = A.upart + 4 * (size_t)blockIdx.x;
        pp[0] = ((sred[0][0] + sred[0][1]) + sred[0][2]) + sred[0][3];
        pp[1] = ((sred[1][0] + sred[1][1]) + sred[1][2]) + sred[1][3];
        pp[2] = ((sred[2][0] + sred[2][1]) + sred[2][2]) + sred[2][3];
        pp[3] = fminf(fminf(sred[3][0], sred[3][1]), fminf(sred[3][2], sred[3][3]));
        const int left = (int)(((sred[4][0] + sred[4][1]) + sred[4][2]) + sred[4][3]);       // (<= 512 rows: exact in float32)
        if (A.n_active && left > 0) atomicAdd(A.n_active, left);
    }
}

// ------------------------------------------------------------------------------------------
// The GLOBAL step of a streaming fit (models/gap.py partial_fit; stochastic variational inference, Hoffman et al. 2013): the
// gene side of k_gamma_update / k_gamma_update_vec with the shapes and rates BLENDED into what the model holds instead of
// replaced -- per gene j (FIN: per packed gene p, o = row_index[p], Z[o] += F[p] * sum_slabs R[p] first, as k_finalize) --
//   b1 = max(1e-15, nan_to_num(omr * b1 + rho * (beta1_k + scale * Z[j,k])))        omr = 1 - rho, formed once on the host
//   b2 = max(1e-15, nan_to_num(omr * b2 + rho * (beta2_k + scale * sum_u[k])))
// then E = b1 / b2, Elog = gamma_meanlog_f32(b1, b2) and their column sums exactly as the Z == NULL form of k_gamma_update
// forms them from a stored pair.  The convex form: rho = 0 multiplies the old value by 1 and adds 0 (b stays bit for bit),
// rho = 1 multiplies it by 0 (the batch estimate bit for bit, the pair of k_gamma_update at scale = 1).  b2 is a matrix: a loaded state need not hold the same rate in every gene.
struct SviArgs {
    double *b1, *b2, *E;
    float *Elog;
    double *colsum_E, *colsum_Elog;
    const double *beta1, *beta2;
    float *Z;
    const float *F, *R;
    const int32_t *row_index;
    const double *sum_u;
    double scale, rho, omr;
    int64_t r;
    int K, Kp, nslab, rpb;
    int su_mat;                   // sum_u is an (r, K) matrix in the caller's gene order (oriana_svi_gene_update_mat), not a K-vector
};

// (explicit FMAs, three roundings per value -- prior + scale * stat, rho * that, omr * old + it: every instantiation below
//  then forms the same bits, whatever the compiler would have contracted)
__device__ __forceinline__ double svi_target(double prior, double scale, double stat) { return fma(scale, stat, prior); }
__device__ __forceinline__ double svi_blend(double old, double target, double rho, double omr) {
    return clamp_eps(fma(omr, old, rho * target));
}

// the element-per-lane form: the mapping and the reduction of k_gamma_update<FIN, 256>
template <bool FIN>
__global__ __launch_bounds__(256) void k_svi_gene_update(const SviArgs A) {
    constexpr int NT = 256;
    __shared__ double red[2][NT];
    const int KT = blockDim.x, RY = blockDim.y, K = A.K, Kp = A.Kp;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int64_t r = A.r;
    const int64_t r0 = (int64_t)blockIdx.x * A.rpb;
    const int64_t r1 = (r0 + A.rpb < r) ? r0 + A.rpb : r;
    double p1[GU_MAXCOLS_PER_THREAD], t2[GU_MAXCOLS_PER_THREAD], sE[GU_MAXCOLS_PER_THREAD], sL[GU_MAXCOLS_PER_THREAD];
    #pragma unroll
    for (int c = 0; c < GU_MAXCOLS_PER_THREAD; ++c) {
        const int k = tx + c * KT;
        p1[c] = k < K ? A.beta1[k] : 1.0;
        // (su_mat: the prior, the target is formed per element below)
        t2[c] = k < K ? (A.su_mat ? A.beta2[k] : svi_target(A.beta2[k], A.scale, A.sum_u[k])) : 1.0;
        sE[c] = 0.0; sL[c] = 0.0;
    }
    for (int64_t row = r0 + ty; row < r1; row += RY) {
        const int64_t orow = (FIN && A.row_index) ? (int64_t)A.row_index[row] : row;
        #pragma unroll
        for (int c = 0; c < GU_MAXCOLS_PER_THREAD; ++c) {
            const int k = tx + c * KT;
            if (k < K) {
                const int64_t idx = orow * K + k;
                float z = A.Z[idx];
                if (FIN) {
                    float rr = A.R[row * Kp + k];
                    for (int sl = 1; sl < A.nslab; ++sl) rr += A.R[((int64_t)sl * r + row) * Kp + k];
                    z = fmaf(A.F[row * Kp + k], rr, z) + 0.0f;                                     // k_finalize (accumulate)
                    A.Z[idx] = z;
                }
                const double s1 = svi_blend(A.b1[idx], svi_target(p1[c], A.scale, (double)z), A.rho, A.omr);
                const double s2 = svi_blend(A.b2[idx], A.su_mat ? svi_target(t2[c], A.scale, A.sum_u[idx]) : t2[c], A.rho, A.omr);
                A.b1[idx] = s1;
                A.b2[idx] = s2;
                const double e = s1 / s2;                                // gamma.py:37-46
                const float el = gamma_meanlog_f32(s1, s2);              // gamma.py:52-61
                A.E[idx] = e;
                A.Elog[idx] = el;
                sE[c] += e;
                sL[c] += (double)el;
            }
        }
    }
    const int flat = ty * KT + tx, lane = flat & 63, wv = flat >> 6, NW = NT / 64;
    const int kw = KT < 64 ? KT : 64;                  // distinct columns inside a wave
    #pragma unroll
    for (int c = 0; c < GU_MAXCOLS_PER_THREAD; ++c) {
        if (c * KT >= K) break;                        // (uniform: no thread holds a column of this round)
        const int k = tx + c * KT;
        double vE = sE[c], vL = sL[c];
        for (int off = kw; off < 64; off <<= 1) { vE += __shfl_xor(vE, off); vL += __shfl_xor(vL, off); }
        __syncthreads();
        if (lane < kw) {
            red[0][wv * kw + lane] = vE;
            red[1][wv * kw + lane] = vL;
        }
        __syncthreads();
        if (ty == 0 && k < K) {
            double tE = 0.0, tL = 0.0;
            if (KT <= 64) {
                for (int w = 0; w < NW; ++w) { tE += red[0][w * kw + tx]; tL += red[1][w * kw + tx]; }
            } else {
                // KT = 128: rows of threads span two waves; wave 2y + (tx >> 6) holds columns (tx & 63) of row y
                for (int w = (tx >> 6); w < NW; w += 2) { tE += red[0][w * kw + (tx & 63)]; tL += red[1][w * kw + (tx & 63)]; }
            }
            if (A.colsum_E) atomicAdd(&A.colsum_E[k], tE);
            if (A.colsum_Elog) atomicAdd(&A.colsum_Elog[k], tL);
        }
    }
}

// VEC consecutive factors per lane, LPR lanes per row: the mapping and the reduction of k_gamma_update_vec
template <bool FIN, int VEC, int LPR>
__global__ __launch_bounds__(256) void k_svi_gene_update_vec(const SviArgs A) {
    constexpr int RPW = 64 / LPR, NW = 4, NCOL = LPR * VEC;
    __shared__ double red[2][NW][NCOL];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int cg = lane & (LPR - 1), sr = lane / LPR;
    const int k0 = cg * VEC, K = A.K, Kp = A.Kp;
    const bool act = k0 < K;
    const int64_t r = A.r;
    const int64_t r0 = (int64_t)blockIdx.x * A.rpb;
    const int64_t r1 = (r0 + A.rpb < r) ? r0 + A.rpb : r;
    double p1[VEC], t2[VEC], sE[VEC], sL[VEC];
    #pragma unroll
    for (int v = 0; v < VEC; ++v) {
        p1[v] = act ? A.beta1[k0 + v] : 1.0;
        t2[v] = act ? (A.su_mat ? A.beta2[k0 + v] : svi_target(A.beta2[k0 + v], A.scale, A.sum_u[k0 + v])) : 1.0;      // (su_mat: the prior)
        sE[v] = 0.0; sL[v] = 0.0;
    }
    for (int64_t rb = r0 + w * RPW; rb < r1; rb += NW * RPW) {
        const int64_t row = rb + sr;
        if (act && row < r1) {
            const int64_t orow = (FIN && A.row_index) ? (int64_t)A.row_index[row] : row;
            const int64_t idx = orow * K + k0;
            float z[VEC], el[VEC];
            double s1[VEC], s2[VEC], e[VEC];
            ld_f32<VEC>(z, A.Z + idx);
            if (FIN) {
                float rr[VEC], f[VEC];
                ld_f32<VEC>(rr, A.R + row * Kp + k0);
                ld_f32<VEC>(f, A.F + row * Kp + k0);
                for (int sl = 1; sl < A.nslab; ++sl) {
                    float r2[VEC];
                    ld_f32<VEC>(r2, A.R + ((int64_t)sl * r + row) * Kp + k0);
                    #pragma unroll
                    for (int v = 0; v < VEC; ++v) rr[v] += r2[v];
                }
                #pragma unroll
                for (int v = 0; v < VEC; ++v) z[v] = fmaf(f[v], rr[v], z[v]) + 0.0f;                 // k_finalize (accumulate)
                st_f32<VEC>(A.Z + idx, z);
            }
            double tg[VEC];
            ld_f64<VEC>(s1, A.b1 + idx);
            ld_f64<VEC>(s2, A.b2 + idx);
            if (A.su_mat) ld_f64<VEC>(tg, A.sum_u + idx);
            #pragma unroll
            for (int v = 0; v < VEC; ++v) {
                s1[v] = svi_blend(s1[v], svi_target(p1[v], A.scale, (double)z[v]), A.rho, A.omr);
                s2[v] = svi_blend(s2[v], A.su_mat ? svi_target(t2[v], A.scale, tg[v]) : t2[v], A.rho, A.omr);
                e[v] = s1[v] / s2[v];                                                       // gamma.py:37-46
                el[v] = gamma_meanlog_f32(s1[v], s2[v]);                                    // gamma.py:52-61
                sE[v] += e[v];
                sL[v] += (double)el[v];
            }
            st_f64<VEC>(A.b1 + idx, s1);
            st_f64<VEC>(A.b2 + idx, s2);
            st_f64<VEC>(A.E + idx, e);
            st_f32<VEC>(A.Elog + idx, el);
        }
    }
    // column sums: lanes holding the same factors inside the wave, then the four waves through LDS
    #pragma unroll
    for (int v = 0; v < VEC; ++v) {
        double vE = sE[v], vL = sL[v];
        #pragma unroll
        for (int o = LPR; o < 64; o <<= 1) { vE += __shfl_xor(vE, o, 64); vL += __shfl_xor(vL, o, 64); }
        if (sr == 0) { red[0][w][k0 + v] = vE; red[1][w][k0 + v] = vL; }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) {
        const double tE = ((red[0][0][k] + red[0][1][k]) + red[0][2][k]) + red[0][3][k];
        const double tL = ((red[1][0][k] + red[1][1][k]) + red[1][2][k]) + red[1][3][k];
        if (A.colsum_E) atomicAdd(&A.colsum_E[k], tE);
        if (A.colsum_Elog) atomicAdd(&A.colsum_Elog[k], tL);
    }
}

__global__ __launch_bounds__(256) void k_colsum_f64(double *__restrict__ out, const double *__restrict__ A,
                                                    const float *__restrict__ mul, int64_t r, int K, int rpb) {
    __shared__ double red[256];
    const int KT = blockDim.x, RY = blockDim.y;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * rpb;
    const int64_t r1 = (r0 + rpb < r) ? r0 + rpb : r;
    for (int c = 0; c < GU_MAXCOLS_PER_THREAD; ++c) {
        const int k = tx + c * KT;
        double s = 0.0;
        if (k < K) {
            for (int64_t row = r0 + ty; row < r1; row += RY) {
                double v = A[row * K + k];
                if (mul) v *= (double)mul[row * K + k];
                s += v;
            }
        }
        __syncthreads();
        red[ty * KT + tx] = s;
        __syncthreads();
        if (ty == 0 && k < K) {
            double t = 0.0;
            for (int y = 0; y < RY; ++y) t += red[y * KT + tx];
            atomicAdd(&out[k], t);
        }
    }
}

// gap.py:117-129: one thread per factor
__global__ void k_mstep_gamma(double *__restrict__ p1, double *__restrict__ p2, const double *__restrict__ colsum_E,
                              const double *__restrict__ colsum_Elog, double count, int K) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    // np.mean over a float32 matrix returns float32 (gap.py:120)
    const float mean_log = (float)(colsum_Elog[k] / count);
    const double y = log(p2[k]) + (double)mean_log;
    const double n1 = clamp_eps(inverse_digamma_f64(y));
    const double mean_e = colsum_E[k] / count;
    const double n2 = clamp_eps(n1 / mean_e);
    p1[k] = n1;
    p2[k] = n2;
}

// both Gamma nodes in one launch (block 0: U side, block 1: V side).  keep_v: the V side's column sums were accumulated
// in colsum_v (scratch of the sweep) and are copied to keep_v (2K values: sums of E, then of Elog), where the next
// sweep's cell-side update reads sum_j V_hat.
__global__ void k_mstep_gamma_pair(double *__restrict__ p1u, double *__restrict__ p2u, const double *__restrict__ cEu,
                                   const double *__restrict__ cLu, double count_u, double *__restrict__ p1v,
                                   double *__restrict__ p2v, const double *__restrict__ cEv,
                                   const double *__restrict__ cLv, double count_v, double *__restrict__ keep_v, int K) {
    const bool vs = blockIdx.x == 1;
    double *p1 = vs ? p1v : p1u, *p2 = vs ? p2v : p2u;
    const double *cE = vs ? cEv : cEu, *cL = vs ? cLv : cLu;
    const double count = vs ? count_v : count_u;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const double se = cE[k], sl = cL[k];
        const float mean_log = (float)(sl / count);
        const double y = log(p2[k]) + (double)mean_log;
        const double n1 = clamp_eps(inverse_digamma_f64(y));
        const double n2 = clamp_eps(n1 / (se / count));
        p1[k] = n1;
        p2[k] = n2;
        if (vs && keep_v) { keep_v[k] = se; keep_v[K + k] = sl; }
    }
}

// lgamma for x > 0.  Below 2^-27 (the shapes clamped to 1e-15, gap.py:55) the series -log x - gamma x, whose next term
// (pi^2 / 12 x^2) is below 1e-17: no dependence on how the library treats arguments next to the pole.
__device__ __forceinline__ double lgamma_pos(double x) {
    if (x < 7.450580596923828e-09) return -log(x) - 0.5772156649015329 * x;
    return lgamma(x);
}

// The per-factor constants of the Kullback-Leibler kernels, the launch's dynamic LDS (5 K doubles), [K] each: p1 | p2 |
// lgamma(p1) - p1 log p2 | s2 (vector form, s2_row != 0) | its log.  The 256 threads fill it; the caller's barrier follows.
extern __shared__ double kc[];
__device__ __forceinline__ void gamma_kl_fill(const double *s2, int s2_row, const double *p1, const double *p2, int K) {
    for (int k = threadIdx.x; k < K; k += 256) {
        const double a = p1[k], b = p2[k];
        kc[k] = a;
        kc[K + k] = b;
        kc[2 * K + k] = lgamma_pos(a) - a * log(b);
        kc[3 * K + k] = s2_row ? s2[k] : 0.0;
        kc[4 * K + k] = s2_row ? log(s2[k]) : 0.0;
    }
}

// KL(Gamma(s1_e, s2) || Gamma(p1_k, p2_k)) of element e, factor k, shape / rate, float64, five pieces in this order:
//   (s1 - p1) psi(s1) - lgamma(s1) + lgamma(p1) + p1 (log s2 - log p2) + s1 (p2 - s2) / s2
__device__ __forceinline__ double gamma_kl_term(const double *s1, const double *s2, int s2_row, int64_t e, int k, int K) {
    const double a = s1[e];
    const double b = s2_row ? kc[3 * K + k] : s2[e];
    const double lb = s2_row ? kc[4 * K + k] : log(b);
    const double pa = kc[k], pb = kc[K + k];
    return (a - pa) * digamma_f64(a) - lgamma_pos(a) + kc[2 * K + k] + pa * lb + a * (pb - b) / b;
}

// out[0] += sum_{i,k} KL(Gamma(s1_ik, s2_ik) || Gamma(p1_k, p2_k)) (gamma_kl_term).
// s2_row != 0: s2 is a K-vector, the same rate in every row (pCMF's cell side, oriana_gamma_update_finalize_lazy).
// Grid-stride over the r K elements; the per-factor constants in LDS (5 K doubles); one atomic per work-group.
__global__ __launch_bounds__(256) void k_gamma_kl(double *__restrict__ out, const double *__restrict__ s1,
                                                  const double *__restrict__ s2, int s2_row, const double *__restrict__ p1,
                                                  const double *__restrict__ p2, int64_t r, int K) {
    __shared__ double red[4];
    gamma_kl_fill(s2, s2_row, p1, p2, K);
    __syncthreads();
    const int64_t tot = r * K;
    double acc = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (int64_t)gridDim.x * 256) {
        const int k = (int)(e % K);
        acc += gamma_kl_term(s1, s2, s2_row, e, k, K);
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

// out[i] = sum_k KL(Gamma(s1_ik, s2_ik) || Gamma(p1_k, p2_k)): k_gamma_kl per row instead of in total (models/gap.py:
// score_samples) -- gamma_kl_term per element over the cache of gamma_kl_fill.  `lpr` lanes (a power of two, 4 .. 64) share a
// row: a lane adds its factors k = c, c + lpr, .. in that order, a butterfly over the lane group combines them (both partners
// form the same sum) and the group's first lane WRITES the row's value: a fixed order, no atomics, nothing to zero first.
__global__ __launch_bounds__(256) void k_gamma_kl_rows(double *__restrict__ out, const double *__restrict__ s1,
                                                       const double *__restrict__ s2, int s2_row, const double *__restrict__ p1,
                                                       const double *__restrict__ p2, int64_t r, int K, int lpr) {
    gamma_kl_fill(s2, s2_row, p1, p2, K);
    __syncthreads();
    const int rpb = 256 / lpr, c = threadIdx.x & (lpr - 1);
    // (g0 is uniform over the work-group: every lane takes part in every butterfly, the groups beyond r with 0)
    for (int64_t g0 = (int64_t)blockIdx.x * rpb; g0 < r; g0 += (int64_t)gridDim.x * rpb) {
        const int64_t i = g0 + threadIdx.x / lpr;
        double acc = 0.0;
        if (i < r) {
            for (int k = c; k < K; k += lpr) {
                acc += gamma_kl_term(s1, s2, s2_row, i * K + k, k, K);
            }
        }
        for (int o = lpr >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (c == 0 && i < r) out[i] = acc;
    }
}

enum { OP_DIGAMMA = 0, OP_TRIGAMMA, OP_INVDIGAMMA, OP_SIGMOID, OP_LOGIT };
template <int OP>
__global__ void k_map_f64(double *__restrict__ y, const double *__restrict__ x, int64_t len) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const double v = x[i];
    double o;
    if (OP == OP_DIGAMMA) o = digamma_f64(v);
    else if (OP == OP_TRIGAMMA) o = trigamma_f64(v);
    else if (OP == OP_INVDIGAMMA) o = inverse_digamma_f64(v);
    else if (OP == OP_SIGMOID) o = sigmoid_f64(v);
    else o = logit_f64(v);
    y[i] = o;
}

template <int OP>
static int launch_map(double *y, const double *x, int64_t len, void *stream) {
    if (len < 0) return ORIANA_EINVAL;
    if (len == 0) return 0;
    if (!y || !x) return ORIANA_EINVAL;
    hipLaunchKernelGGL(k_map_f64<OP>, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, x, len);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

// Rows per block: enough blocks to fill the chip (>= ~8 per CU) even for a short matrix -- at 512 rows
// per block the gene side (30,000 rows) ran on 59 of the 256 CUs and one rank's share of the cell side
// (125,000 rows) on 245, a single 4-wave block each: 0.34 ms per call instead of ~0.1.
static inline int rows_per_block(int64_t r, int ry) {
    int64_t rpb = (r + 2047) / 2048;
    rpb = (rpb + ry - 1) / ry * ry;
    if (rpb < 4 * ry) rpb = 4 * ry;
    if (rpb > GU_ROWS_PER_BLOCK) rpb = GU_ROWS_PER_BLOCK;
    return (int)rpb;
}

static inline void pick_block(int64_t K, dim3 *block, int threads = 256) {
    int kt = 1;
    while (kt < K && kt < 128) kt <<= 1;
    *block = dim3(kt, threads / kt);
}

// short matrices: 1024-thread groups, four rows per thread (see k_gamma_update)
static inline bool gu_large_groups(int64_t r) {
    // (inside a configs[1] sweep: 10,000 rows 19.3 us with 1024-thread groups against 22.4 with 256; 2,000 rows 13.8 against 9.6)
    return r > 4096 && r <= 32768;
}


// ---- dispatch of k_gamma_update_vec -------------------------------------------------------------------------------
static inline bool aligned_to(const void *p, uintptr_t a) { return p == nullptr || ((uintptr_t)p & (a - 1)) == 0; }

// VEC and LPR for this K (false: the element-per-lane kernel serves it)
static inline bool gu_vec_cfg(int64_t K, bool wide_ok, int *vec, int *lpr) {
    int v;
    if (wide_ok && K % 4 == 0 && K <= 256) v = 4;
    else if (wide_ok && K % 2 == 0 && K <= 128) v = 2;
    else if (K <= 64) v = 1;
    else return false;
    int l = 8;
    while (l * v < K) l <<= 1;
    *vec = v; *lpr = l;
    return true;
}

static inline int gu_vec_rpb(int64_t r, int lpr) {
    const int ry = 4 * (64 / lpr);
    return rows_per_block(r, ry);
}

template <bool FIN, int VEC>
static void gu_vec_launch_lpr(const GuVecArgs &a, int lpr, int64_t nblk, hipStream_t s) {
    const dim3 g((unsigned)nblk), b(256);
    switch (lpr) {
    case 8: hipLaunchKernelGGL((k_gamma_update_vec<FIN, VEC, 8>), g, b, 0, s, a); break;
    case 16: hipLaunchKernelGGL((k_gamma_update_vec<FIN, VEC, 16>), g, b, 0, s, a); break;
    case 32: hipLaunchKernelGGL((k_gamma_update_vec<FIN, VEC, 32>), g, b, 0, s, a); break;
    default: hipLaunchKernelGGL((k_gamma_update_vec<FIN, VEC, 64>), g, b, 0, s, a); break;
    }
}

// true: launched (a.rpb is set here); false: no vector configuration for this K / these pointers
template <bool FIN>
static bool gu_vec_launch(GuVecArgs a, hipStream_t s) {
    const bool wide_ok = aligned_to(a.a1, 16) && aligned_to(a.a2, 16) && aligned_to(a.E, 16) && aligned_to(a.Elog, 16) &&
                         aligned_to(a.Z_in, 16) && aligned_to(a.zmul, 16) && aligned_to(a.rate_mat, 16) && aligned_to(a.rmul, 16) &&
                         aligned_to(a.Zfin, 16) && aligned_to(a.F, 16) && aligned_to(a.Rs, 16) && aligned_to(a.FUn, 16) &&
                         aligned_to(a.a2row, 16);
    int vec, lpr;
    if (!gu_vec_cfg(a.K, wide_ok, &vec, &lpr)) return false;
    if (a.FUn) {
        // The caller sized `upart` with oriana_gamma_update_prep_blocks, which assumes the aligned (wide) configuration: a
        // pointer that is not 16-byte aligned would drop to a narrower VEC, a smaller rows-per-block and MORE blocks than
        // upart has room for.  Refuse instead (the entry returns ORIANA_EINVAL).
        int v2, l2;
        if (!gu_vec_cfg(a.K, true, &v2, &l2) || v2 != vec || l2 != lpr) return false;
    }
    a.rpb = gu_vec_rpb(a.r, lpr);
    const int64_t nblk = (a.r + a.rpb - 1) / a.rpb;
    if (vec == 4) gu_vec_launch_lpr<FIN, 4>(a, lpr, nblk, s);
    else if (vec == 2) gu_vec_launch_lpr<FIN, 2>(a, lpr, nblk, s);
    else gu_vec_launch_lpr<FIN, 1>(a, lpr, nblk, s);
    return true;
}

// Short matrices are latency-bound (a sweep of configs[1] is a dozen launches of microseconds): there a thread's serial
// chain is what counts, and one element per lane (k_gamma_update, large groups) is the shorter one -- measured at 2,000 x 20:
// 10.3 us against 15.0 us, at 10,000 x 20: 15.7 against 17.4 (profiles/r05_perf_gamma*.txt).  The vector kernel takes over from
// 2^20 elements on (30,000 x 100: 46 against 60 us), and whenever its PREP outputs are asked for.
static inline bool gu_small(int64_t r, int64_t K) { return r * K < (int64_t)1 << 20; }

// the element-per-lane kernel on the arguments of the vector one
template <bool FIN>
static int gu_scalar_launch(const GuVecArgs &a, hipStream_t s) {
    constexpr int BIG = FIN ? 1024 : 512;            // (the general form needs more than the 128 VGPRs of a 1024-thread group)
    dim3 block;
    const bool big = gu_large_groups(a.r);
    pick_block(a.K, &block, big ? BIG : 256);
    const int rpb = big ? 4 * (int)block.y : rows_per_block(a.r, (int)block.y);
    const dim3 grid((unsigned)((a.r + rpb - 1) / rpb));
    const int Kp = FIN ? a.Kp : 0;
#define ORIANA_GU(NT) hipLaunchKernelGGL((k_gamma_update<FIN, NT>), grid, block, 0, s, a.a1, a.a2, a.E, a.Elog, a.colsum_E, a.colsum_Elog,    \
                                         a.prior1, a.prior2, a.Z_in, a.zmul, a.rate_vec, a.rate_mat, a.rmul, a.r, a.K, rpb, a.Zfin, a.F, a.Rs, \
                                         a.row_index, Kp, a.nslab, a.slab_row0)
    if (big) ORIANA_GU(BIG);
    else ORIANA_GU(256);
#undef ORIANA_GU
    ORIANA_LAUNCH_CHECK();
    return 0;
}

}  // namespace oriana

using namespace oriana;

extern "C" int64_t oriana_gamma_update_prep_blocks(int64_t r, int64_t K) {
    int vec, lpr;
    if (r <= 0 || K <= 0 || !gu_vec_cfg(K, true, &vec, &lpr)) return 0;
    const int rpb = gu_vec_rpb(r, lpr);
    return (r + rpb - 1) / rpb;
}

extern "C" int oriana_gamma_update_prep(double *a1, double *a2, double *E, float *Elog, double *colsum_E,
                                        double *colsum_Elog, const double *prior1, const double *prior2, const float *Z,
                                        const float *zmul, const double *rate_vec, const double *rate_mat,
                                        const float *rmul, int64_t r, int64_t K, float *FU_next, float *mu_out, float *upart,
                                        void *stream) {
    if (r < 0 || K <= 0) return ORIANA_EINVAL;
    if (K > 128 * GU_MAXCOLS_PER_THREAD) return ORIANA_EKRANGE;
    if (r == 0) return 0;
    if (!a1 || !a2 || !E || !Elog) return ORIANA_EINVAL;
    if (Z && (!prior1 || !prior2 || (!rate_vec && !rate_mat))) return ORIANA_EINVAL;
    if (FU_next && (!mu_out || !upart || oriana_kpad(K) == 0)) return ORIANA_EINVAL;
    const GuVecArgs a = {a1, a2, E, Elog, colsum_E, colsum_Elog, prior1, prior2, Z, zmul, rate_vec, rate_mat, rmul, r, (int)K, 0,
                         nullptr, nullptr, nullptr, nullptr, (int)oriana_kpad(K), 1, 0, FU_next, mu_out, upart, nullptr};
    if ((FU_next || !gu_small(r, K)) && gu_vec_launch<false>(a, (hipStream_t)stream)) { ORIANA_LAUNCH_CHECK(); return 0; }
    if (FU_next) return ORIANA_EINVAL;                 // (callers ask oriana_gamma_update_prep_blocks first)
    return gu_scalar_launch<false>(a, (hipStream_t)stream);
}

extern "C" int oriana_gamma_update(double *a1, double *a2, double *E, float *Elog, double *colsum_E,
                                   double *colsum_Elog, const double *prior1, const double *prior2, const float *Z,
                                   const float *zmul, const double *rate_vec, const double *rate_mat,
                                   const float *rmul, int64_t r, int64_t K, void *stream) {
    return oriana_gamma_update_prep(a1, a2, E, Elog, colsum_E, colsum_Elog, prior1, prior2, Z, zmul, rate_vec, rate_mat, rmul, r, K,
                                    nullptr, nullptr, nullptr, stream);
}

extern "C" int oriana_gamma_update_finalize_prep(double *a1, double *a2, double *E, float *Elog, double *colsum_E,
                                            double *colsum_Elog, const double *prior1, const double *prior2, float *Z,
                                            const float *F, const float *R, int64_t nslab, int64_t slab_row0, const int32_t *row_index,
                                            const double *rate_vec, int64_t r, int64_t K, float *FU_next, float *mu_out,
                                            float *upart, void *stream) {
    if (r < 0 || K <= 0 || nslab < 1 || nslab > 65535 || slab_row0 < 0) return ORIANA_EINVAL;
    const int64_t Kp = oriana_kpad(K);
    if (K > 128 * GU_MAXCOLS_PER_THREAD || Kp == 0) return ORIANA_EKRANGE;
    if (r == 0) return 0;
    if (!a1 || !a2 || !E || !Elog || !Z || !F || !R || !prior1 || !prior2 || !rate_vec) return ORIANA_EINVAL;
    if (FU_next && (!mu_out || !upart)) return ORIANA_EINVAL;
    const GuVecArgs a = {a1, a2, E, Elog, colsum_E, colsum_Elog, prior1, prior2, nullptr, nullptr, rate_vec, nullptr, nullptr, r, (int)K, 0,
                         Z, F, R, row_index, (int)Kp, (int)nslab, slab_row0, FU_next, mu_out, upart, nullptr};
    if ((FU_next || !gu_small(r, K)) && gu_vec_launch<true>(a, (hipStream_t)stream)) { ORIANA_LAUNCH_CHECK(); return 0; }
    if (FU_next) return ORIANA_EINVAL;
    return gu_scalar_launch<true>(a, (hipStream_t)stream);
}

// [r6] pCMF's cell side without the two matrices nobody reads inside a sweep (gap.py:98, 101): a2 is the same K numbers in
// every row (alpha2 + sum_j V_hat) -- they go to a2_row[K] once -- and U_hat = a1 / a2 is not stored (its column sums still
// are summed here).  1.6 of the 4.8 GB the launch moves at configs[3].  The caller (models/gap.py) evaluates both on access.
// ORIANA_EKRANGE: no vector configuration for this K / these pointers -- the caller takes oriana_gamma_update_finalize_prep.
extern "C" int oriana_gamma_update_finalize_lazy(double *a1, double *a2_row, float *Elog, double *colsum_E, double *colsum_Elog,
                                                 const double *prior1, const double *prior2, float *Z, const float *F,
                                                 const float *R, int64_t nslab, int64_t slab_row0, const int32_t *row_index,
                                                 const double *rate_vec, int64_t r, int64_t K, float *FU_next, float *mu_out,
                                                 float *upart, void *stream) {
    if (r < 0 || K <= 0 || nslab < 1 || nslab > 65535 || slab_row0 < 0) return ORIANA_EINVAL;
    const int64_t Kp = oriana_kpad(K);
    if (K > 128 * GU_MAXCOLS_PER_THREAD || Kp == 0) return ORIANA_EKRANGE;
    if (!a1 || !a2_row || !Elog || !Z || !F || !R || !prior1 || !prior2 || !rate_vec) return ORIANA_EINVAL;
    if (FU_next && (!mu_out || !upart)) return ORIANA_EINVAL;
    if (r == 0) return ORIANA_EKRANGE;                 // (nothing would write a2_row)
    if (!FU_next && gu_small(r, K)) return ORIANA_EKRANGE;     // (launch-bound sizes: the scalar kernel)
    GuVecArgs a = {a1, nullptr, nullptr, Elog, colsum_E, colsum_Elog, prior1, prior2, nullptr, nullptr, rate_vec, nullptr, nullptr, r, (int)K, 0,
                   Z, F, R, row_index, (int)Kp, (int)nslab, slab_row0, FU_next, mu_out, upart, a2_row};
    if (!gu_vec_launch<true>(a, (hipStream_t)stream)) return ORIANA_EKRANGE;
    ORIANA_LAUNCH_CHECK();
    return 0;
}

// rows per work-group of k_foldin_update: a function of r alone (every configuration walks whole multiples of its rows per
// iteration, 4 .. 32), so that the caller can size `upart` before it knows which configuration its pointers get
static inline int foldin_rpb(int64_t r) { return rows_per_block(r, 32); }

extern "C" int64_t oriana_foldin_update_blocks(int64_t r) {
    if (r <= 0) return 0;
    const int rpb = foldin_rpb(r);
    return (r + rpb - 1) / rpb;
}

template <int VEC, bool ZI>
static void foldin_launch_lpr(const FoldinArgs &a, int lpr, int64_t nblk, hipStream_t s) {
    const dim3 g((unsigned)nblk), b(256);
    switch (lpr) {
    case 8: hipLaunchKernelGGL((k_foldin_update<VEC, 8, 1, ZI>), g, b, 0, s, a); break;
    case 16: hipLaunchKernelGGL((k_foldin_update<VEC, 16, 1, ZI>), g, b, 0, s, a); break;
    case 32: hipLaunchKernelGGL((k_foldin_update<VEC, 32, 1, ZI>), g, b, 0, s, a); break;
    default: hipLaunchKernelGGL((k_foldin_update<VEC, 64, 1, ZI>), g, b, 0, s, a); break;
    }
}

// the configuration for this K and these pointers (gu_vec_cfg; the element-per-lane instantiation for what it leaves out)
template <bool ZI>
static void foldin_launch(const FoldinArgs &a, bool wide_ok, hipStream_t s) {
    const int64_t nblk = (a.r + a.rpb - 1) / a.rpb;
    int vec, lpr;
    if (!gu_vec_cfg(a.K, wide_ok, &vec, &lpr)) hipLaunchKernelGGL((k_foldin_update<1, 64, 4, ZI>), dim3((unsigned)nblk), dim3(256), 0, s, a);
    else if (vec == 4) foldin_launch_lpr<4, ZI>(a, lpr, nblk, s);
    else if (vec == 2) foldin_launch_lpr<2, ZI>(a, lpr, nblk, s);
    else foldin_launch_lpr<1, ZI>(a, lpr, nblk, s);
}

extern "C" int oriana_foldin_update(double *a1, float *Elog, uint8_t *active, int32_t *froze_at, int32_t *n_active,
                                    const double *alpha1, const double *a2_row, const float *Z, const float *F, const float *R,
                                    int64_t nslab, int64_t slab_row0, const int32_t *row_index, int64_t r, int64_t K, double tol,
                                    int64_t it, float *FU_next, float *mu_out, float *upart, void *stream) {
    if (r < 0 || K <= 0 || nslab < 1 || nslab > 65535 || slab_row0 < 0 || it < 0 || it > 0x7fffffffLL || !(tol >= 0.0)) return ORIANA_EINVAL;
    const int64_t Kp = oriana_kpad(K);
    if (Kp == 0) return ORIANA_EKRANGE;                // (no row pass serves this K: there is no F / R layout to read)
    if (r == 0) return 0;
    if (!a1 || !Elog || !active || !a2_row || !FU_next || !mu_out || !upart) return ORIANA_EINVAL;
    if (R && (!Z || !F || !alpha1 || !froze_at)) return ORIANA_EINVAL;
    FoldinArgs a = {a1, Elog, active, froze_at, R ? n_active : nullptr, alpha1, a2_row, Z, F, R, row_index, FU_next, mu_out, upart,
                    r, slab_row0, (int)K, (int)Kp, (int)nslab, foldin_rpb(r), (int)it, tol, nullptr, nullptr, nullptr, nullptr};
    const bool wide_ok = aligned_to(a1, 16) && aligned_to(Elog, 16) && aligned_to(Z, 16) && aligned_to(F, 16) && aligned_to(R, 16) &&
                         aligned_to(FU_next, 16);
    foldin_launch<false>(a, wide_ok, (hipStream_t)stream);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_foldin_update_zi(double *a1, double *a2, double *U_hat, float *Elog, uint8_t *active, int32_t *froze_at,
                                       int32_t *n_active, const double *alpha1, const double *alpha2, const double *rate,
                                       const float *Z, const float *F, const float *R, int64_t nslab, int64_t slab_row0,
                                       const int32_t *row_index, int64_t r, int64_t K, double tol, int64_t it, float *FU_next,
                                       float *mu_out, float *upart, void *stream) {
    if (r < 0 || K <= 0 || nslab < 1 || nslab > 65535 || slab_row0 < 0 || it < 0 || it > 0x7fffffffLL || !(tol >= 0.0)) return ORIANA_EINVAL;
    const int64_t Kp = oriana_kpad(K);
    if (Kp == 0) return ORIANA_EKRANGE;
    if (r == 0) return 0;
    if (!a1 || !a2 || !U_hat || !Elog || !active || !FU_next || !mu_out || !upart) return ORIANA_EINVAL;
    if (R && (!Z || !F || !alpha1 || !alpha2 || !rate || !froze_at)) return ORIANA_EINVAL;
    FoldinArgs a = {a1, Elog, active, froze_at, R ? n_active : nullptr, alpha1, nullptr, Z, F, R, row_index, FU_next, mu_out, upart,
                    r, slab_row0, (int)K, (int)Kp, (int)nslab, foldin_rpb(r), (int)it, tol, a2, rate, alpha2, U_hat};
    const bool wide_ok = aligned_to(a1, 16) && aligned_to(a2, 16) && aligned_to(U_hat, 16) && aligned_to(rate, 16) && aligned_to(Elog, 16) &&
                         aligned_to(Z, 16) && aligned_to(F, 16) && aligned_to(R, 16) && aligned_to(FU_next, 16);
    foldin_launch<true>(a, wide_ok, (hipStream_t)stream);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_gamma_update_finalize(double *a1, double *a2, double *E, float *Elog, double *colsum_E,
                                            double *colsum_Elog, const double *prior1, const double *prior2, float *Z,
                                            const float *F, const float *R, int64_t nslab, const int32_t *row_index,
                                            const double *rate_vec, int64_t r, int64_t K, void *stream) {
    return oriana_gamma_update_finalize_prep(a1, a2, E, Elog, colsum_E, colsum_Elog, prior1, prior2, Z, F, R, nslab, 0, row_index,
                                             rate_vec, r, K, nullptr, nullptr, nullptr, stream);
}

template <bool FIN, int VEC>
static void svi_vec_launch_lpr(const SviArgs &a, int lpr, int64_t nblk, hipStream_t s) {
    const dim3 g((unsigned)nblk), b(256);
    switch (lpr) {
    case 8: hipLaunchKernelGGL((k_svi_gene_update_vec<FIN, VEC, 8>), g, b, 0, s, a); break;
    case 16: hipLaunchKernelGGL((k_svi_gene_update_vec<FIN, VEC, 16>), g, b, 0, s, a); break;
    case 32: hipLaunchKernelGGL((k_svi_gene_update_vec<FIN, VEC, 32>), g, b, 0, s, a); break;
    default: hipLaunchKernelGGL((k_svi_gene_update_vec<FIN, VEC, 64>), g, b, 0, s, a); break;
    }
}

// the configuration of gu_vec_cfg for this K and these pointers; the element-per-lane kernel for what it leaves out (odd K
// above 64, buffers that are not 16-byte aligned at a K above 64).  No gu_small rule: a call sits behind a whole fold-in.
template <bool FIN>
static void svi_launch(SviArgs a, hipStream_t s) {
    const bool wide_ok = aligned_to(a.b1, 16) && aligned_to(a.b2, 16) && aligned_to(a.E, 16) && aligned_to(a.Elog, 16) &&
                         aligned_to(a.Z, 16) && aligned_to(a.F, 16) && aligned_to(a.R, 16) && (!a.su_mat || aligned_to(a.sum_u, 16));
    int vec, lpr;
    if (gu_vec_cfg(a.K, wide_ok, &vec, &lpr)) {
        a.rpb = gu_vec_rpb(a.r, lpr);
        const int64_t nblk = (a.r + a.rpb - 1) / a.rpb;
        if (vec == 4) svi_vec_launch_lpr<FIN, 4>(a, lpr, nblk, s);
        else if (vec == 2) svi_vec_launch_lpr<FIN, 2>(a, lpr, nblk, s);
        else svi_vec_launch_lpr<FIN, 1>(a, lpr, nblk, s);
        return;
    }
    dim3 block;
    pick_block(a.K, &block, 256);
    a.rpb = rows_per_block(a.r, (int)block.y);
    hipLaunchKernelGGL((k_svi_gene_update<FIN>), dim3((unsigned)((a.r + a.rpb - 1) / a.rpb)), block, 0, s, a);
}

// one entry behind both forms of the rate statistic: a K-vector every gene shares (pCMF) or an (m, K) matrix (ZI-pCMF)
static int svi_gene_update(double *b1, double *b2, double *E, float *Elog, double *colsum_E, double *colsum_Elog, const double *beta1,
                           const double *beta2, float *Z, const float *F, const float *R, int64_t nslab, const int32_t *row_index,
                           const double *sum_u, int su_mat, double scale, double rho, int64_t m, int64_t K, void *stream) {
    if (m < 0 || K <= 0 || !(rho >= 0.0 && rho <= 1.0) || !(scale >= 0.0 && scale < INFINITY)) return ORIANA_EINVAL;
    if (F && (nslab < 1 || nslab > 65535)) return ORIANA_EINVAL;
    const int64_t Kp = oriana_kpad(K);
    if (Kp == 0) return ORIANA_EKRANGE;
    if (m == 0) return 0;
    if (!b1 || !b2 || !E || !Elog || !beta1 || !beta2 || !Z || !sum_u || (F && !R)) return ORIANA_EINVAL;
    const SviArgs a = {b1, b2, E, Elog, colsum_E, colsum_Elog, beta1, beta2, Z, F, F ? R : nullptr, F ? row_index : nullptr, sum_u,
                       scale, rho, 1.0 - rho, m, (int)K, (int)Kp, F ? (int)nslab : 1, 0, su_mat};
    if (F) svi_launch<true>(a, (hipStream_t)stream);
    else svi_launch<false>(a, (hipStream_t)stream);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_svi_gene_update(double *b1, double *b2, double *E, float *Elog, double *colsum_E, double *colsum_Elog,
                                      const double *beta1, const double *beta2, float *Z, const float *F, const float *R,
                                      int64_t nslab, const int32_t *row_index, const double *sum_u, double scale, double rho,
                                      int64_t m, int64_t K, void *stream) {
    return svi_gene_update(b1, b2, E, Elog, colsum_E, colsum_Elog, beta1, beta2, Z, F, R, nslab, row_index, sum_u, 0, scale, rho, m, K,
                           stream);
}

// the rate statistic as an (m, K) float64 matrix in the caller's gene order (ZIGaP.fold_in_fit: G_jk = sum_i d_ij U_hat_ik)
extern "C" int oriana_svi_gene_update_mat(double *b1, double *b2, double *E, float *Elog, double *colsum_E, double *colsum_Elog,
                                          const double *beta1, const double *beta2, float *Z, const float *F, const float *R,
                                          int64_t nslab, const int32_t *row_index, const double *rate, double scale, double rho,
                                          int64_t m, int64_t K, void *stream) {
    return svi_gene_update(b1, b2, E, Elog, colsum_E, colsum_Elog, beta1, beta2, Z, F, R, nslab, row_index, rate, 1, scale, rho, m, K,
                           stream);
}

extern "C" int oriana_colsum_f64(double *out, const double *A, const float *mul, int64_t r, int64_t K, void *stream) {
    if (r < 0 || K <= 0) return ORIANA_EINVAL;
    if (K > 128 * GU_MAXCOLS_PER_THREAD) return ORIANA_EKRANGE;
    if (r == 0) return 0;
    if (!out || !A) return ORIANA_EINVAL;
    dim3 block;
    pick_block(K, &block);
    const int rpb = rows_per_block(r, (int)block.y);
    const int64_t nblk = (r + rpb - 1) / rpb;
    hipLaunchKernelGGL(k_colsum_f64, dim3((unsigned)nblk), block, 0, (hipStream_t)stream, out, A, mul, r, (int)K, rpb);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_mstep_gamma(double *p1, double *p2, const double *colsum_E, const double *colsum_Elog,
                                  double count, int64_t K, void *stream) {
    if (K <= 0 || !(count > 0)) return ORIANA_EINVAL;
    if (!p1 || !p2 || !colsum_E || !colsum_Elog) return ORIANA_EINVAL;
    hipLaunchKernelGGL(k_mstep_gamma, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, (hipStream_t)stream, p1, p2,
                       colsum_E, colsum_Elog, count, (int)K);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_mstep_gamma_pair(double *p1u, double *p2u, const double *colsum_E_u, const double *colsum_Elog_u,
                                       double count_u, double *p1v, double *p2v, const double *colsum_E_v,
                                       const double *colsum_Elog_v, double count_v, double *keep_v, int64_t K,
                                       void *stream) {
    if (K <= 0 || !(count_u > 0) || !(count_v > 0)) return ORIANA_EINVAL;
    if (!p1u || !p2u || !colsum_E_u || !colsum_Elog_u || !p1v || !p2v || !colsum_E_v || !colsum_Elog_v) return ORIANA_EINVAL;
    hipLaunchKernelGGL(k_mstep_gamma_pair, dim3(2), dim3(K <= 64 ? 64 : 128), 0, (hipStream_t)stream, p1u, p2u, colsum_E_u,
                       colsum_Elog_u, count_u, p1v, p2v, colsum_E_v, colsum_Elog_v, count_v, keep_v, (int)K);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_digamma_f64(double *y, const double *x, int64_t len, void *s) { return launch_map<OP_DIGAMMA>(y, x, len, s); }
extern "C" int oriana_trigamma_f64(double *y, const double *x, int64_t len, void *s) { return launch_map<OP_TRIGAMMA>(y, x, len, s); }
extern "C" int oriana_inverse_digamma_f64(double *y, const double *x, int64_t len, void *s) { return launch_map<OP_INVDIGAMMA>(y, x, len, s); }
extern "C" int oriana_sigmoid_f64(double *y, const double *x, int64_t len, void *s) { return launch_map<OP_SIGMOID>(y, x, len, s); }
extern "C" int oriana_logit_f64(double *y, const double *x, int64_t len, void *s) { return launch_map<OP_LOGIT>(y, x, len, s); }

extern "C" int oriana_gamma_kl(double *out, const double *s1, const double *s2, int s2_is_row, const double *p1,
                               const double *p2, int64_t r, int64_t K, void *stream) {
    if (r < 0 || K <= 0 || K > 1024) return ORIANA_EINVAL;
    if (r == 0) return 0;
    if (!out || !s1 || !s2 || !p1 || !p2) return ORIANA_EINVAL;
    const int64_t tot = r * K;
    int64_t nblk = (tot + 1023) / 1024;            // four elements per lane, at most eight work-groups per CU
    const int64_t cap = 8 * oriana_device_cus();
    if (nblk > cap) nblk = cap;
    if (nblk < 1) nblk = 1;
    hipLaunchKernelGGL(k_gamma_kl, dim3((unsigned)nblk), dim3(256), (size_t)5 * K * sizeof(double), (hipStream_t)stream, out, s1,
                       s2, s2_is_row ? 1 : 0, p1, p2, r, (int)K);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_gamma_kl_rows(double *out, const double *s1, const double *s2, int s2_is_row, const double *p1,
                                    const double *p2, int64_t r, int64_t K, void *stream) {
    if (r < 0 || K <= 0 || K > 1024) return ORIANA_EINVAL;
    if (r == 0) return 0;
    if (!out || !s1 || !s2 || !p1 || !p2) return ORIANA_EINVAL;
    int lpr = 4;                                   // the smallest lane group that covers K, a wave at the most
    while (lpr < 64 && lpr < K) lpr *= 2;
    const int64_t rpb = 256 / lpr;
    int64_t nblk = (r + rpb - 1) / rpb;
    const int64_t cap = 8 * oriana_device_cus();   // (at most eight work-groups per CU, as oriana_gamma_kl)
    if (nblk > cap) nblk = cap;
    if (nblk < 1) nblk = 1;
    hipLaunchKernelGGL(k_gamma_kl_rows, dim3((unsigned)nblk), dim3(256), (size_t)5 * K * sizeof(double), (hipStream_t)stream, out,
                       s1, s2, s2_is_row ? 1 : 0, p1, p2, r, (int)K, lpr);
    ORIANA_LAUNCH_CHECK();
    return 0;
}
