// metrics.hip -- the sparse-side sums of the deviance / Frobenius metrics (reference
// oriana/models/base.py:58-87 with loglikelihood_X, sparse_zigap.py:44-51).  Lambda_ij = <U_hat_i, V_j>
// at the stored (non-zero) entries comes from the responsibility kernels themselves: with
// FU = float32(U_hat), FV = float32(V) the row pass leaves s_ij = x_ij / Lambda_ij in the row-side
// slots; everything that depends on the zero entries is either a closed form of column sums or
// the MODE 1 epilogue of k_dropout_fused (dense_mfma.hip).
#include "common.h"

namespace oriana {

// F[i, k] = float32(E[row_index ? row_index[i] : i, k] * (mul ? mul[same row, k] : 1)), padded to Kp
__global__ __launch_bounds__(256) void k_factor_cast(float *__restrict__ F, const double *__restrict__ E,
                                                     const float *__restrict__ mul,
                                                     const int32_t *__restrict__ row_index, int64_t r, int K, int Kp) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= r * Kp) return;
    const int64_t i = idx / Kp;
    const int k = (int)(idx - i * Kp);
    float v = 0.f;
    if (k < K) {
        const int64_t src = row_index ? (int64_t)row_index[i] : i;
        double e = E[src * K + k];
        if (mul) e *= (double)mul[src * K + k];
        v = (float)e;
    }
    F[idx] = v;
}

__device__ __forceinline__ double block_sum(double v, double *sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < nw; ++i) t += sh[i];
    return t;
}

// constants of X: colsum[gene] += sum_i x_ij, colnnz[gene] += #{i: x_ij != 0} (caller's gene order),
// out[0] += sum (x log x - x), out[1] += sum x^2, over the stored entries.  One work-group per tile.
__global__ __launch_bounds__(256) void k_count_stats(oriana_counts cm, double *__restrict__ colsum,
                                                     double *__restrict__ colnnz, double *__restrict__ out) {
    __shared__ double cs[TILE];
    __shared__ int cn[TILE];
    __shared__ double sh[4];
    const int64_t t = blockIdx.x;
    const int64_t cb = t % cm.ncb;
    cs[threadIdx.x] = 0.0;
    cn[threadIdx.x] = 0;
    __syncthreads();
    const int64_t rbase = cm.roff[t];
    const uint32_t s_end = cm.rslice[t * 17 + 16];
    double a0 = 0.0, a1 = 0.0;
    for (uint32_t slot = threadIdx.x; slot < s_end; slot += 256) {
        const oriana_rowrec rec = cm.rowrec[rbase + slot];
        if (rec.x == 0.f) continue;
        const double x = (double)rec.x;
        a0 += x * log(x) - x;
        a1 += x * x;
        // (float64: a column's sum over one tile's 256 rows leaves float32's exact range once counts reach ~2^16 --
        //  17 counts of 10^6 already round -- and counts of 65535 and above always live in this sliced layout)
        atomicAdd(&cs[rec.col], x);
        atomicAdd(&cn[rec.col], 1);
    }
    __syncthreads();
    const int64_t jp = cb * TILE + threadIdx.x;
    if (jp < cm.m && cn[threadIdx.x] != 0) {
        const int64_t j = cm.col_perm ? (int64_t)cm.col_perm[jp] : jp;
        atomicAdd(&colsum[j], cs[threadIdx.x]);
        atomicAdd(&colnnz[j], (double)cn[threadIdx.x]);
    }
    a0 = block_sum(a0, sh);
    a1 = block_sum(a1, sh);
    if (threadIdx.x == 0) { atomicAdd(&out[0], a0); atomicAdd(&out[1], a1); }
}

// out[0] += sum Lambda, out[1] += sum x log Lambda, out[2] += sum Lambda^2, out[3] += sum x Lambda over the
// stored entries, Lambda = x / s (s from the row pass).  Entries the row pass could not evaluate (NaN
// sentinel: Lambda < 1e-10) are recomputed from the float64 factors.
__global__ __launch_bounds__(256) void k_metric_nnz(oriana_counts cm, const float *__restrict__ s_rs,
                                                    const double *__restrict__ U, const double *__restrict__ V,
                                                    int K, double *__restrict__ out) {
    __shared__ double sh[4];
    const int64_t t = blockIdx.x;
    const int64_t rb = t / cm.ncb, cb = t - rb * cm.ncb;
    const int64_t rbase = cm.roff[t];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int sl = 0; sl < 16; ++sl) {
        const uint32_t s0 = cm.rslice[t * 17 + sl], s1 = cm.rslice[t * 17 + sl + 1];
        for (uint32_t slot = s0 + threadIdx.x; slot < s1; slot += 256) {
            const oriana_rowrec rec = cm.rowrec[rbase + slot];
            if (rec.x == 0.f) continue;
            const float s = s_rs[rbase + slot];
            const double x = (double)rec.x;
            double lam;
            if (s == s && s != 0.f) {
                lam = x / (double)s;
            } else {
                const int64_t ip = rb * TILE + sl * 16 + (int)(((slot - s0) & 63u) >> 2);
                const int64_t jp = cb * TILE + rec.col;
                const int64_t i = cm.row_perm ? (int64_t)cm.row_perm[ip] : ip;
                const int64_t j = cm.col_perm ? (int64_t)cm.col_perm[jp] : jp;
                lam = 0.0;
                for (int k = 0; k < K; ++k) lam += U[i * K + k] * V[j * K + k];
            }
            a0 += lam;
            a1 += x * log(lam);
            a2 += lam * lam;
            a3 += x * lam;
        }
    }
    a0 = block_sum(a0, sh);
    a1 = block_sum(a1, sh);
    a2 = block_sum(a2, sh);
    a3 = block_sum(a3, sh);
    if (threadIdx.x == 0) {
        atomicAdd(&out[0], a0); atomicAdd(&out[1], a1); atomicAdd(&out[2], a2); atomicAdd(&out[3], a3);
    }
}

// The sums of k_metric_nnz kept per gene and per cell (models/base.py: gene_deviance, cell_deviance).  One work-group per tile
// as k_metric_nnz, the rate by the same rule (Lambda = x / s from the row pass, the float64 sum of U, V for the NaN sentinel
// and for 0), so the per-axis values and the scalar metrics see the same rate.
//   gene_out (m, 3), caller's gene order: += { sum Lambda, sum x log Lambda, sum (x log x - x) } over the gene's stored entries
//   cell_out (n, 5), caller's row order : += the same three over the cell's stored entries, then { sum gconst[j][0],
//                                          sum (gconst[j][1] + x gconst[j][2]) }, gconst (m, 3) in the caller's gene order
// A NULL output skips that axis.  Per tile the partial sums live in LDS: a gene table as k_count_stats keeps (LDS float64
// atomics, one per entry and term) and a row table fed as k_cell_bound_nnz feeds its own -- a thread striding by 256 stays with
// one row per slice (slice lengths are multiples of 64), adds its entries in registers, the 4 lanes of the row are combined by a
// butterfly and one lane adds the result for the (wave, slice) into the row table.  What leaves the work-group is one float64
// atomic per term and touched (tile, gene) or (tile, row): the outputs are sums of atomics, reruns agree to the order of the
// additions (the dense block and the dropout term add into the same arrays the same way).  24 KiB of LDS.
__global__ __launch_bounds__(256) void k_metric_nnz_axes(oriana_counts cm, const float *__restrict__ s_rs,
                                                         const double *__restrict__ U, const double *__restrict__ V, int K,
                                                         const double *__restrict__ gconst, double *__restrict__ gene_out,
                                                         double *__restrict__ cell_out) {
    __shared__ double gs[TILE][3];
    __shared__ double gc[TILE][3];
    __shared__ double rs[TILE][5];
    __shared__ int gn[TILE], rn[TILE];
    const int tid = threadIdx.x, rl = (tid & 63) >> 2;
    const int64_t t = blockIdx.x;
    const int64_t rb = t / cm.ncb, cb = t - rb * cm.ncb;
    const int64_t rbase = cm.roff[t];
    {
        const int64_t jp = cb * TILE + tid;
        const bool ok = cell_out && jp < cm.m;
        const int64_t j = ok ? (cm.col_perm ? (int64_t)cm.col_perm[jp] : jp) : 0;
#pragma unroll
        for (int q = 0; q < 3; ++q) { gs[tid][q] = 0.0; gc[tid][q] = ok ? gconst[3 * j + q] : 0.0; }
#pragma unroll
        for (int q = 0; q < 5; ++q) rs[tid][q] = 0.0;
        gn[tid] = 0;
        rn[tid] = 0;
    }
    __syncthreads();
    for (int sl = 0; sl < 16; ++sl) {
        const uint32_t s0 = cm.rslice[t * 17 + sl], s1 = cm.rslice[t * 17 + sl + 1];
        if (s0 == s1) continue;                                  // (uniform over the work-group)
        const int r = sl * 16 + rl;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
        int cnt = 0;
        for (uint32_t slot = s0 + tid; slot < s1; slot += 256) {
            const oriana_rowrec rec = cm.rowrec[rbase + slot];
            if (rec.x == 0.f) continue;
            const float s = s_rs[rbase + slot];
            const double x = (double)rec.x;
            const int c = rec.col;
            double lam;
            if (s == s && s != 0.f) {
                lam = x / (double)s;
            } else {
                const int64_t ip = rb * TILE + r, jp = cb * TILE + c;
                const int64_t i = cm.row_perm ? (int64_t)cm.row_perm[ip] : ip;
                const int64_t j = cm.col_perm ? (int64_t)cm.col_perm[jp] : jp;
                lam = 0.0;
                for (int k = 0; k < K; ++k) lam += U[i * K + k] * V[j * K + k];
            }
            const double xl = x * log(lam), xx = x * log(x) - x;
            if (gene_out) {
                atomicAdd(&gs[c][0], lam);
                atomicAdd(&gs[c][1], xl);
                atomicAdd(&gs[c][2], xx);
                gn[c] = 1;
            }
            if (cell_out) {
                a0 += lam; a1 += xl; a2 += xx;
                a3 += gc[c][0];
                a4 += gc[c][1] + x * gc[c][2];
                cnt = 1;
            }
        }
        if (cell_out) {
            // (a slice's length is a multiple of 64: the lanes of a wave leave the loop together)
            a0 += __shfl_xor(a0, 1, 64); a0 += __shfl_xor(a0, 2, 64);
            a1 += __shfl_xor(a1, 1, 64); a1 += __shfl_xor(a1, 2, 64);
            a2 += __shfl_xor(a2, 1, 64); a2 += __shfl_xor(a2, 2, 64);
            a3 += __shfl_xor(a3, 1, 64); a3 += __shfl_xor(a3, 2, 64);
            a4 += __shfl_xor(a4, 1, 64); a4 += __shfl_xor(a4, 2, 64);
            cnt |= __shfl_xor(cnt, 1, 64); cnt |= __shfl_xor(cnt, 2, 64);
            if ((tid & 3) == 0 && cnt) {
                atomicAdd(&rs[r][0], a0); atomicAdd(&rs[r][1], a1); atomicAdd(&rs[r][2], a2);
                atomicAdd(&rs[r][3], a3); atomicAdd(&rs[r][4], a4);
                rn[r] = 1;
            }
        }
    }
    __syncthreads();
    const int64_t jp = cb * TILE + tid, ip = rb * TILE + tid;
    if (gene_out && gn[tid] && jp < cm.m) {
        const int64_t j = cm.col_perm ? (int64_t)cm.col_perm[jp] : jp;
#pragma unroll
        for (int q = 0; q < 3; ++q) atomicAdd(&gene_out[3 * j + q], gs[tid][q]);
    }
    if (cell_out && rn[tid] && ip < cm.n) {
        const int64_t i = cm.row_perm ? (int64_t)cm.row_perm[ip] : ip;
#pragma unroll
        for (int q = 0; q < 5; ++q) atomicAdd(&cell_out[5 * i + q], rs[tid][q]);
    }
}

constexpr int PREFIX_MAX_ENDS = 256;      // K <= 256 in the sliced layout (oriana_kpad), one end per factor at most

// The deviance sums of every prefix of the factors (models/base.py: deviance_path): with Lambda^(k)_ij = sum_{l < k} FU[ip, l]
// FV[jp, l] the running float32 sum over the factor images (packed row / gene order, row stride Kp, columns already in the
// caller's factor order), out[e, 0] += sum Lambda^(ends[e]), out[e, 1] += sum x log Lambda^(ends[e]) over the stored entries.
// One work-group per tile and one lane per stored entry, as k_metric_nnz; a lane walks the factors ONCE and stops at each end.
// A running sum that is not a trusted float32 value there (below 1e-10 -- the row pass's threshold --, zero, NaN or infinite)
// is replaced by the float64 sum of U, V (caller's row / gene order through row_perm / col_perm, columns in the same factor
// order), itself a running sum that is advanced only when asked for: the fall-back costs one more walk, not one per end.
// Accumulators: a lane cannot hold 2 x 100+ float64 sums in registers, so nothing is accumulated per lane.  At each end the
// wave adds its 64 lanes' two terms (wave_sum_f64, common.h: DPP and permlane swaps, no LDS) and lane 0 adds the pair into the wave's own row of an LDS table
// part[wave][end][2] (16 KiB), which no other wave touches: no barrier inside the walk.  The table is summed over the four
// waves at the end and goes out as one float64 atomic per (end, term) and work-group.  Slice lengths are multiples of 64
// (pack.hip: k_pack_fill), and the slot loop is written so that the lanes of a wave run it together whatever the length:
// the cross-lane sums always see all 64 lanes (a padding slot or a lane past the end contributes 0).
__global__ __launch_bounds__(256) void k_metric_nnz_prefix(oriana_counts cm, const float *__restrict__ FU,
                                                           const float *__restrict__ FV, const double *__restrict__ U,
                                                           const double *__restrict__ V, int K, int Kp,
                                                           const int32_t *__restrict__ ends, int E,
                                                           double *__restrict__ out) {
    __shared__ double part[4][PREFIX_MAX_ENDS][2];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    for (int e = tid; e < 4 * E; e += 256) { part[e / E][e % E][0] = 0.0; part[e / E][e % E][1] = 0.0; }
    __syncthreads();
    const int64_t t = blockIdx.x;
    const int64_t rb = t / cm.ncb, cb = t - rb * cm.ncb;
    const int64_t rbase = cm.roff[t];
    for (int sl = 0; sl < 16; ++sl) {
        const uint32_t s0 = cm.rslice[t * 17 + sl], s1 = cm.rslice[t * 17 + sl + 1];
        for (uint32_t wbase = s0 + (uint32_t)(w * 64); wbase < s1; wbase += 256) {      // (uniform over the wave)
            const uint32_t slot = wbase + (uint32_t)lane;
            double x = 0.0;
            int64_t ip = 0, jp = 0;
            if (slot < s1) {
                const oriana_rowrec rec = cm.rowrec[rbase + slot];
                x = (double)rec.x;
                ip = rb * TILE + sl * 16 + (int)(((slot - s0) & 63u) >> 2);
                jp = cb * TILE + rec.col;
            }
            const bool live = x != 0.0 && ip < cm.n && jp < cm.m;
            if (!live) { ip = 0; jp = 0; }                                // (a row every lane may read)
            if (__ballot(live) == 0ull) continue;                        // (uniform: a wave of padding)
            const float *__restrict__ fu = FU + ip * Kp;
            const float *__restrict__ fv = FV + jp * Kp;
            const int64_t i = cm.row_perm ? (int64_t)cm.row_perm[ip] : ip;
            const int64_t j = cm.col_perm ? (int64_t)cm.col_perm[jp] : jp;
            const double *__restrict__ u = U + i * K;
            const double *__restrict__ v = V + j * K;
            float acc = 0.f;
            double dacc = 0.0;
            int dl = 0, e = 0;
            int end = min((int)ends[0], K);
            // four factors per 16-byte load (Kp is a multiple of 4 and the images hold zeros from K on); an end is met when the
            // number of factors added equals it (ends that do not increase are never met: their sums stay 0)
            for (int c = 0; 4 * c < K && e < E; ++c) {
                const float4 a4 = reinterpret_cast<const float4 *>(fu)[c], b4 = reinterpret_cast<const float4 *>(fv)[c];
                const float pa[4] = {a4.x, a4.y, a4.z, a4.w}, pb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc = fmaf(pa[q], pb[q], acc);
                    if (4 * c + q + 1 != end) continue;                  // (uniform over the wave)
                    double a0 = 0.0, a1 = 0.0;
                    if (live) {
                        double lam = (double)acc;
                        if (!(acc >= DEN_MIN && acc < INFINITY)) {
                            for (; dl < end; ++dl) dacc += u[dl] * v[dl];
                            lam = dacc;
                        }
                        a0 = lam;
                        a1 = x * log(lam);
                    }
                    a0 = wave_sum_f64(a0);
                    a1 = wave_sum_f64(a1);
                    if (lane == 0) { part[w][e][0] += a0; part[w][e][1] += a1; }
                    ++e;
                    end = e < E ? min((int)ends[e], K) : -1;
                }
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < 2 * E; e += 256) {
        const int q = e & 1, ee = e >> 1;
        const double s = ((part[0][ee][q] + part[1][ee][q]) + part[2][ee][q]) + part[3][ee][q];
        if (s != 0.0) atomicAdd(&out[e], s);
    }
}

// One stored entry of the data term, count x != 0 at the packed position (ip, jp), s its row-pass value: a0 += x log den,
// a1 += lgamma(x + 1).  log den_ij = mu_u[i] + mu_v[j] + log(x / s); what the shifted form could not represent (NaN sentinel or
// 0 in s, a rejected row's NaN maximum) is a float64 log-sum-exp over the K factors.  THE arithmetic of k_elbo_nnz and
// k_cell_bound_nnz: the sum over the cells of the second is the first up to the order of additions.
__device__ __forceinline__ void bound_entry(const oriana_counts &cm, const float s, const double x, const int64_t ip,
                                            const int64_t jp, const float *mu_u, const float *mu_v, const float *logU,
                                            const float *logV, int K, double &a0, double &a1) {
    if (ip >= cm.n || jp >= cm.m) return;                    // (no stored entry lies there: mu_u, mu_v end at n, m)
    double ld = NAN;
    if (s > 0.f && s < INFINITY) ld = (double)mu_u[ip] + (double)mu_v[jp] + log(x / (double)s);
    if (!(fabs(ld) < INFINITY)) {
        const int64_t i = cm.row_perm ? (int64_t)cm.row_perm[ip] : ip;
        const int64_t j = cm.col_perm ? (int64_t)cm.col_perm[jp] : jp;
        ld = logsumexp_f64(logU + i * K, logV + j * K, K);
    }
    a0 += x * ld;
    a1 += lgamma(x + 1.0);
}

// out[0] += sum x log den, out[1] += sum lgamma(x + 1) over the stored entries: the data term of the variational bound
// (models/gap.py: elbo).  log den_ij = log sum_k exp(lu_ik + lv_jk) = mu_u[i] + mu_v[j] + log(x / s), s from the row pass
// over the shifted factors exp(l - mu) of oriana_factor_prep (mu_u, mu_v: its row maxima, packed order); per entry
// bound_entry: the bound lives in the log domain and stays finite where den itself underflows.
__global__ __launch_bounds__(256) void k_elbo_nnz(oriana_counts cm, const float *__restrict__ s_rs,
                                                  const float *__restrict__ mu_u, const float *__restrict__ mu_v,
                                                  const float *__restrict__ logU, const float *__restrict__ logV,
                                                  int K, double *__restrict__ out) {
    __shared__ double sh[4];
    const int64_t t = blockIdx.x;
    const int64_t rb = t / cm.ncb, cb = t - rb * cm.ncb;
    const int64_t rbase = cm.roff[t];
    double a0 = 0.0, a1 = 0.0;
    for (int sl = 0; sl < 16; ++sl) {
        const uint32_t s0 = cm.rslice[t * 17 + sl], s1 = cm.rslice[t * 17 + sl + 1];
        for (uint32_t slot = s0 + threadIdx.x; slot < s1; slot += 256) {
            const oriana_rowrec rec = cm.rowrec[rbase + slot];
            if (rec.x == 0.f) continue;
            bound_entry(cm, s_rs[rbase + slot], (double)rec.x, rb * TILE + sl * 16 + (int)(((slot - s0) & 63u) >> 2),
                        cb * TILE + rec.col, mu_u, mu_v, logU, logV, K, a0, a1);
        }
    }
    a0 = block_sum(a0, sh);
    a1 = block_sum(a1, sh);
    if (threadIdx.x == 0) { atomicAdd(&out[0], a0); atomicAdd(&out[1], a1); }
}

// out[i] = { sum_j x_ij log den_ij, sum_j lgamma(x_ij + 1) } over the stored entries of cell i (caller's row order): the two
// sums of k_elbo_nnz per cell (models/gap.py: score_samples), entry for entry by bound_entry.  One work-group owns a
// row block and walks its gene tiles in order.  Slot s0 + t of a slice belongs to row sl * 16 + ((t & 63) >> 2) and slice
// lengths are multiples of 64 (pack.hip: k_pack_fill, slice_offsets), so a thread striding by 256 stays with ONE row per
// slice: a row's entries are spread over 4 lanes x 4 waves.  The work-group is four such groups of 256 threads, group g taking
// the slices sl = g, g + 4, .. of every tile (a row belongs to one group: 16 waves per CU where one group alone leaves the
// float64 log / lgamma chains of a single wave per SIMD exposed).  Each thread adds its entries of a (tile, slice) in slot
// order, the 4 lanes of a row are combined by a butterfly (both partners form the same sum) and the (wave, row) partial in
// LDS, which that lane group alone touches, takes the result: tile after tile, a fixed order.  The 4 waves are added at the
// end and every row of the block is WRITTEN (0 for a cell without entries): no atomics, nothing to zero first, reruns are
// bit-identical.  (The lane reduction runs per slice, not once at the end: sixteen per-slice accumulators in registers need
// the slice loop unrolled, sixteen copies of the lgamma / log / log-sum-exp bodies.)
__global__ __launch_bounds__(1024) void k_cell_bound_nnz(oriana_counts cm, const float *__restrict__ s_rs,
                                                         const float *__restrict__ mu_u, const float *__restrict__ mu_v,
                                                         const float *__restrict__ logU, const float *__restrict__ logV,
                                                         int K, double *__restrict__ out) {
    __shared__ double sh[2][4][TILE];
    const int tid = threadIdx.x & 255, grp = threadIdx.x >> 8, w = tid >> 6, rl = (tid & 63) >> 2;
    const int64_t rb = blockIdx.x;
    sh[0][grp][tid] = 0.0;
    sh[1][grp][tid] = 0.0;
    __syncthreads();
    for (int64_t cb = 0; cb < cm.ncb; ++cb) {
        const int64_t t = rb * cm.ncb + cb;
        const int64_t rbase = cm.roff[t];
        for (int sl = grp; sl < 16; sl += 4) {
            const uint32_t s0 = cm.rslice[t * 17 + sl], s1 = cm.rslice[t * 17 + sl + 1];
            if (s0 == s1) continue;                              // (uniform over the group)
            const int r = sl * 16 + rl;
            const int64_t ip = rb * TILE + r;
            double a0 = 0.0, a1 = 0.0;
            for (uint32_t slot = s0 + tid; slot < s1; slot += 256) {
                const oriana_rowrec rec = cm.rowrec[rbase + slot];
                if (rec.x == 0.f) continue;
                bound_entry(cm, s_rs[rbase + slot], (double)rec.x, ip, cb * TILE + rec.col, mu_u, mu_v, logU, logV, K, a0, a1);
            }
            // (a slice's length is a multiple of 64: the lanes of a wave leave the loop together)
            a0 += __shfl_xor(a0, 1, 64); a0 += __shfl_xor(a0, 2, 64);
            a1 += __shfl_xor(a1, 1, 64); a1 += __shfl_xor(a1, 2, 64);
            if ((tid & 3) == 0) { sh[0][w][r] += a0; sh[1][w][r] += a1; }
        }
    }
    __syncthreads();
    const int64_t ip = rb * TILE + tid;
    if (grp == 0 && ip < cm.n) {
        const int64_t i = cm.row_perm ? (int64_t)cm.row_perm[ip] : ip;
        out[2 * i] = ((sh[0][0][tid] + sh[0][1][tid]) + sh[0][2][tid]) + sh[0][3][tid];
        out[2 * i + 1] = ((sh[1][0][tid] + sh[1][1][tid]) + sh[1][2][tid]) + sh[1][3][tid];
    }
}

}  // namespace oriana

using namespace oriana;

extern "C" int oriana_factor_cast_f32(float *F, const double *E, const float *mul, const int32_t *row_index,
                                      int64_t r, int64_t K, void *stream) {
    const int64_t Kp = oriana_kpad(K);
    if (r < 0 || Kp == 0) return Kp == 0 ? ORIANA_EKRANGE : ORIANA_EINVAL;
    if (r == 0) return 0;
    if (!F || !E) return ORIANA_EINVAL;
    const int64_t tot = r * Kp;
    hipLaunchKernelGGL(k_factor_cast, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, F, E, mul,
                       row_index, r, (int)K, (int)Kp);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_count_stats(const oriana_counts *cm, double *colsum, double *colnnz, double *out2,
                                  void *stream) {
    if (!cm || !colsum || !colnnz || !out2) return ORIANA_EINVAL;
    const int64_t nt = cm->nrb * cm->ncb;
    if (nt == 0 || cm->rslots == 0) return 0;
    if (nt > 0x7fffffffLL) return ORIANA_EINVAL;
    hipLaunchKernelGGL(k_count_stats, dim3((unsigned)nt), dim3(256), 0, (hipStream_t)stream, *cm, colsum, colnnz, out2);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_metric_nnz(const oriana_counts *cm, const float *s_rs, const double *U, const double *V,
                                 int64_t K, double *out4, void *stream) {
    if (!cm || !s_rs || !U || !V || !out4 || K <= 0) return ORIANA_EINVAL;
    const int64_t nt = cm->nrb * cm->ncb;
    if (nt == 0 || cm->rslots == 0) return 0;
    if (nt > 0x7fffffffLL) return ORIANA_EINVAL;
    hipLaunchKernelGGL(k_metric_nnz, dim3((unsigned)nt), dim3(256), 0, (hipStream_t)stream, *cm, s_rs, U, V, (int)K,
                       out4);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_metric_nnz_axes(const oriana_counts *cm, const float *s_rs, const double *U, const double *V,
                                      int64_t K, const double *gene_const, double *gene_out, double *cell_out,
                                      void *stream) {
    if (!cm || !s_rs || !U || !V || K <= 0 || (!gene_out && !cell_out) || (cell_out && !gene_const)) return ORIANA_EINVAL;
    if (oriana_kpad(K) == 0) return ORIANA_EKRANGE;
    const int64_t nt = cm->nrb * cm->ncb;
    if (nt == 0 || cm->rslots == 0) return 0;
    if (nt > 0x7fffffffLL) return ORIANA_EINVAL;
    hipLaunchKernelGGL(k_metric_nnz_axes, dim3((unsigned)nt), dim3(256), 0, (hipStream_t)stream, *cm, s_rs, U, V, (int)K,
                       gene_const, gene_out, cell_out);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_metric_nnz_prefix(const oriana_counts *cm, const float *FU, const float *FV, const double *U,
                                        const double *V, int64_t K, const int32_t *ends, int64_t n_ends, double *out,
                                        void *stream) {
    const int64_t Kp = oriana_kpad(K);
    if (!cm || !FU || !FV || !U || !V || !out || K <= 0 || n_ends < 0 || n_ends > K) return ORIANA_EINVAL;
    if (Kp == 0 || n_ends > PREFIX_MAX_ENDS) return ORIANA_EKRANGE;
    const int64_t nt = cm->nrb * cm->ncb;
    if (n_ends == 0 || nt == 0 || cm->rslots == 0) return 0;
    if (!ends || nt > 0x7fffffffLL) return ORIANA_EINVAL;
    hipLaunchKernelGGL(k_metric_nnz_prefix, dim3((unsigned)nt), dim3(256), 0, (hipStream_t)stream, *cm, FU, FV, U, V, (int)K,
                       (int)Kp, ends, (int)n_ends, out);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_elbo_nnz(const oriana_counts *cm, const float *s_rs, const float *mu_u, const float *mu_v,
                               const float *logU, const float *logV, int64_t K, double *out2, void *stream) {
    if (!cm || !s_rs || !mu_u || !mu_v || !logU || !logV || !out2 || K <= 0) return ORIANA_EINVAL;
    const int64_t nt = cm->nrb * cm->ncb;
    if (nt == 0 || cm->rslots == 0) return 0;
    if (nt > 0x7fffffffLL) return ORIANA_EINVAL;
    hipLaunchKernelGGL(k_elbo_nnz, dim3((unsigned)nt), dim3(256), 0, (hipStream_t)stream, *cm, s_rs, mu_u, mu_v, logU, logV,
                       (int)K, out2);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_cell_bound_nnz(const oriana_counts *cm, const float *s_rs, const float *mu_u, const float *mu_v,
                                     const float *logU, const float *logV, int64_t K, double *out2, void *stream) {
    if (!cm || !s_rs || !mu_u || !mu_v || !logU || !logV || !out2 || K <= 0) return ORIANA_EINVAL;
    if (cm->nrb == 0 || cm->n == 0) return 0;
    if (cm->nrb < 0 || cm->nrb > 0x7fffffffLL || cm->ncb < 0) return ORIANA_EINVAL;
    // (a layout without a stored entry is still launched: every cell's pair is written, here as 0)
    hipLaunchKernelGGL(k_cell_bound_nnz, dim3((unsigned)cm->nrb), dim3(1024), 0, (hipStream_t)stream, *cm, s_rs, mu_u, mu_v, logU,
                       logV, (int)K, out2);
    ORIANA_LAUNCH_CHECK();
    return 0;
}
