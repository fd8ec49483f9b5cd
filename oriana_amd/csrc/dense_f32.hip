// dense_f32.hip -- the dense (n x m) work of a zero-inflated SWEEP in float32 arithmetic on the matrix cores, with
// every long sum carried on in float64.  Two evaluations of the same float32 products (`arithmetic`):
//   ORIANA_MATRIX_BF16X3  three-way bf16 splits of each operand, six cross products on v_mfma_f32_32x32x16_bf16 (K <= 64)
//   ORIANA_MATRIX_F32     v_mfma_f32_32x32x2_f32 (2x the float64 rate; K <= 128)
//
//   oriana_dropout_sweep_fused   D_hat = f32(sigmoid(logit(pi_d) - U_hat V_hat^T)) with the overrides of zigap.py:130-136,
//                                the column sums of p_d, AND the product D_hat V_next of the NEXT sweep's cell-side
//                                rates (zigap.py:116) from the tile of D_hat still in registers -- one 4 n m byte write,
//                                no read of D_hat.
//   oriana_dense_t_times_factor_f32   out[m, K] += D_hat^T W[n, K]  (zigap.py:124), D_hat streamed once.
//   oriana_zi_cell_bound         the dropout term of a held-out cell's bound: the sweep kernel's Lambda^T = V U^T with the epilogue
//                                z or softplus(z), z = logit(pi~) - Lambda, summed per cell in a fixed order (float32 instruction, K <= 128).
//   oriana_zi_gene_rate          the gene-side rate statistic of a folded-in batch (ZIGaP.fold_in_fit): G = d^T U_hat and the column sums
//                                of d, d the dropout posterior of the fold-in, never stored -- the sweep kernel transposed (genes resident,
//                                cell tiles walked: Lambda = U V^T), partials per cell range WRITTEN and combined in order (float32
//                                instruction, K <= 128; the sums leave float32 every 4096 cells).
//
// Numerics.  v_mfma_f32_32x32x2_f32 is a chain of single-rounding FMAs in k order, round-to-nearest-even
// (tools/ubench/mfma_f32.hip: bit-identical to a host fmaf() chain): a sum of T positive terms carries an unbiased
// relative error of ~ 1.5e-8 sqrt(T) (measured 1.2e-7 / 3.5e-7 / 9.5e-7 rms at T = 64 / 512 / 4096).  Lambda
// (K <= 128 terms) is used as is; the long sums (over genes / cells) leave the matrix core every 256 terms, are added
// up per work-group in float32 registers (<= 20 partial sums of independent error) and across work-groups in float64
// (atomics), so the rate terms carry ~ 1e-7, an order below the 1e-6 the float32 responsibility passes leave
// (DESIGN section 7).
// The exact float64 kernels of dense_mfma.hip stay: they evaluate p_d itself when a caller asks for it, the metrics,
// and the rate term of a sweep that cannot use the fused product (first sweep, state written from outside).
//
// Fragment map of v_mfma_f32_32x32x2_f32: A[m = lane & 31][k = lane >> 5], B[k = lane >> 5][n = lane & 31],
// D reg v: [m = 8 (v / 4) + 4 (lane >> 5) + v % 4][n = lane & 31].
#include "dense_tiles.h"               // tile types, bf16 x 3 splits, the six-product macro, acc_row, TS, pick_splits: used from there
// (the ablation switches behind the measurements of DESIGN_HISTORY.md -- ORIANA_ABL32_NOSTORE / _NOSIG / _NOTRANS -- are
// archived as a patch: tools/experiments/dense_f32_mfma_ablation_switches_r2.diff)

namespace oriana {

// the tile pieces of dense_tiles.h (the bf16 x 3 kernels below use its splits and its six-product macro ORIANA_DN_MF6)
using dn::f16v;
using dn::f4v;
using dn::bf8;
using dn::u4v;
using dn::mfma_b16;
using dn::split2;
using dn::split8;
using dn::acc_row;
using dn::TS;

__device__ __forceinline__ f16v mfma32(float a, float b, f16v c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// Scheduling fence for vector-memory instructions only (everything else may cross): keeps a prefetch where it was
// written -- left alone, the scheduler sinks such loads down to their first use, i.e. turns them into plain loads.
#define ORIANA_VMEM_FENCE() __builtin_amdgcn_sched_barrier(0x38F)

// LDS carve-up of k_dropout_sweep (floats)
struct SweepLds {
    int us, vt, v2, mt, tb, cs, dm, total;
    int v2s;                      // row stride of the [gene][k] image
    __host__ __device__ SweepLds(int KP2, int NT) {
        v2s = NT * 32 + 8;        // 4 rows apart = 32 banks apart: the two lane halves never collide
        int o = 0;
        us = o; o += 4 * KP2 * 32;           // [wave][k][32 cells]
        vt = o; o += 2 * KP2 * 32;           // [buf][k][32 genes]
        v2 = o; o += 2 * 32 * v2s;           // [buf][32 genes][k]
        mt = o; o += 2 * 4 * 32 * 2;         // [buf][wave][32 genes] {logit(pi_d) (+-inf: overrides), non-zero bits
                                             //  of the wave's 32 cells}
        tb = o; o += 4 * 32 * TS;            // [wave][32 cells][32 genes] transpose buffer
        cs = o; o += 2 * 4 * 32;             // [parity][wave][32 genes] column partial sums
        dm = o; o += 32;                     // where the staging writes of k >= KP2 land (no branch per element)
        total = o;
    }
};

// Work-group: 4 waves = 4 strips of 32 cells, one range of genes walked in tiles of 32.  Per tile and wave:
//   Lambda^T[gene, cell] = V U^T on the matrix core (A = V tile from LDS, B = the wave's U strip from LDS) -- the
//   TRANSPOSED product, so that the accumulator registers, after the sigmoid, are already laid out as the A operand
//   of the second product  DV[cell, k] += D[cell, gene] V_next[gene, k]  (register v of lane half h = gene
//   8 (v / 4) + 4 h + v % 4: the reduction simply visits the genes in that order);
//   D_hat goes to HBM through a 32 x 32 transpose in LDS (128-byte runs per cell row); the same read-back yields
//   the tile's column sums.
// RATE (oriana_zi_foldin_rate): DV alone -- the transpose, the D_hat store and the column sums are compiled out; a work-group
// none of whose 128 cells is active returns at its top, U_hat rows of inactive cells are not read, their DV rows not written.
// BOUND (oriana_zi_cell_bound): no second product either -- the epilogue of a tile is g(z) = z at a non-zero count, softplus(z)
// at a zero, z = lgit - Lambda, with `lgit` the CLAMPED image of k_logit_clamped_f32 (finite; -inf marks a gene that is left out).
// All 16 accumulator registers of a lane belong to one cell (c = lane & 31; the lane halves hold different genes of it): their
// float32 sum joins a float64 running sum per tile, the halves meet in one cross-lane step at the end, and the work-group WRITES
// its range's partial to partial[blockIdx.y * n + cell] (the `colsum` argument) -- no atomics; k_cell_bound_combine adds the
// ranges in order.
template <int NT, bool RATE = false, bool BOUND = false>
__global__ __launch_bounds__(256, (NT <= 2) ? 2 : 1) void k_dropout_sweep(float *__restrict__ D_hat, const double *__restrict__ U,
                                                       const double *__restrict__ V, const float *__restrict__ lgit,
                                                       const uint32_t *__restrict__ nzmask, double *__restrict__ colsum,
                                                       const double *__restrict__ Vn, double *__restrict__ DV,
                                                       int64_t n, int64_t m, int K, int KP2, int64_t j_per_split,
                                                       const uint8_t *__restrict__ active) {
    extern __shared__ float lds[];
    constexpr bool STORE = !RATE && !BOUND;                      // D_hat and the column sums leave the kernel
    const SweepLds L(KP2, NT);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int64_t i0w = (int64_t)blockIdx.x * 128 + w * 32;
    const int64_t jb = (int64_t)blockIdx.y * j_per_split;
    const int64_t je = (jb + j_per_split < m) ? jb + j_per_split : m;
    const int KS = KP2 >> 1;
    float *Us = lds + L.us + w * KP2 * 32;
    float *T = lds + L.tb + w * 32 * TS;
    if constexpr (RATE) {
        if (!dn::any_active<128>(active, (int64_t)blockIdx.x * 128, n, lane)) return;     // (work-group uniform)
    }

    // the wave's strip of U_hat, [k][cell]
    for (int e = lane; e < KP2 * 32; e += 64) {
        const int cell = e / KP2, kk = e - cell * KP2;            // consecutive lanes: consecutive k of one cell
        const int64_t i = i0w + cell;
        Us[kk * 32 + cell] = ((RATE ? dn::cell_active(active, i, n) : i < n) && kk < K) ? (float)U[i * K + kk] : 0.f;
    }

    // Staging of one gene tile, 8 threads per gene.  The vector-memory counter of gfx9 retires loads, stores and
    // atomics in ONE order: a wait for a load also waits for every older store.  So the loads of tile t + 1 are issued
    // at the top of tile t and consumed (LDS stores) right BEFORE tile t's D_hat stores are issued -- what is older
    // than them by then (the stores and atomics of tile t - 1) has had a whole tile to drain.
    const int sg = tid >> 3, sk = tid & 7;
    constexpr int NU = NT * 4;                                   // 8 * NU = NT * 32 >= KP2
    const bool same_v = (Vn == V);
    double sreg[NU], nreg[NU];
    uint32_t mkreg = 0;
    // (addresses are clamped into range and the padding is zeroed when the values are consumed: straight-line
    //  loads, no register is written under a branch)
    bool sok = false;
    auto stage_load = [&](int64_t j0) {
        const int64_t j = j0 + sg;
        sok = j < je;
        const int64_t jc = sok ? j : je - 1;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int kk = sk + 8 * u;
            sreg[u] = V[jc * K + (kk < K ? kk : K - 1)];
        }
        if (!BOUND && Vn && !same_v) {
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int kk = sk + 8 * u;
                nreg[u] = Vn[jc * K + (kk < K ? kk : K - 1)];
            }
        }
    };
    auto stage_store = [&](int buf) {
        float *vt = lds + L.vt + buf * KP2 * 32;
        float *v2 = lds + L.v2 + buf * 32 * L.v2s;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int kk = sk + 8 * u;
            const bool ok = sok && kk < K;
            (kk < KP2 ? vt + kk * 32 : lds + L.dm)[sg] = ok ? (float)sreg[u] : 0.f;
            if (!BOUND && Vn) v2[sg * L.v2s + kk] = ok ? (float)(same_v ? sreg[u] : nreg[u]) : 0.f;
        }
    };
    // per gene and wave: {logit(pi_d), the mask word of the wave's 32 cells}; threads 0..127, one (wave, gene) each
    const int mw = (tid >> 5) & 3;
    const int64_t mrow = ((int64_t)blockIdx.x * 128 + mw * 32) >> 5;
    const bool mrow_ok = nzmask && (int64_t)blockIdx.x * 128 + mw * 32 < n;
    float lgreg = 0.f;
    auto meta_load = [&](int64_t j0) {
        if (tid < 128) {
            const int64_t jj = j0 + (tid & 31);
            const int64_t jc = jj < je ? jj : je - 1;
            lgreg = lgit[jc];
            mkreg = mrow_ok ? nzmask[mrow * m + jc] : 0u;
        }
    };
    auto meta_store = [&](int buf) {
        if (tid < 128) {
            float2 pr;
            pr.x = lgreg;
            pr.y = __uint_as_float(mkreg);
            *reinterpret_cast<float2 *>(lds + L.mt + ((buf * 4 + mw) * 32 + (tid & 31)) * 2) = pr;
        }
    };

    f16v dv[NT], dvs[NT];                                       // matrix-core accumulators; their sums every 256 genes
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int v = 0; v < 16; ++v) { dv[nt][v] = 0.f; dvs[nt][v] = 0.f; }
    }
    const bool rowok = i0w + c < n;
    const bool vec_ok = (m & 3) == 0;
    double bsum = 0.0;                                           // BOUND: the cell's running sum over this lane half's genes

    if (jb < je) {
        stage_load(jb);
        meta_load(jb);
        stage_store(0);
        meta_store(0);
    }
    __syncthreads();
    int buf = 0, par = 0, since_flush = 0;
    // column sums of the tile before (partials of the 4 waves in LDS): atomics issued AFTER the tile's loads
    auto colsum_flush = [&](int64_t jt, int parity) {
        if (colsum && w == 0 && lane < 32 && jt + lane < je) {
            const float *cs = lds + L.cs + parity * 4 * 32 + lane;
            atomicAdd(&colsum[jt + lane], (double)cs[0] + (double)cs[32] + (double)cs[64] + (double)cs[96]);
        }
    };
    for (int64_t j0 = jb; j0 < je; j0 += 32) {
        const bool more = j0 + 32 < je;
        { const int64_t jn = more ? j0 + 32 : j0; stage_load(jn); meta_load(jn); }   // (the last tile again: unused)
        if constexpr (STORE) { if (j0 > jb) colsum_flush(j0 - 32, par ^ 1); }
        ORIANA_VMEM_FENCE();
        // ---- Lambda^T = V U^T: four steps per turn, the operands of the next turn requested before the matrix
        // instructions of this one (an LDS round trip is longer than one 16-pass instruction)
        const float *vt = lds + L.vt + buf * KP2 * 32;
        f16v l0;
#pragma unroll
        for (int v = 0; v < 16; ++v) l0[v] = 0.f;
        {
            const float *pa = vt + h * 32 + c, *pb = Us + h * 32 + c;
            float a[4], b[4], an[4], bn[4];
            int s = 0;
            if (KS >= 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) { a[u] = pa[64 * u]; b[u] = pb[64 * u]; }
                for (; s + 8 <= KS; s += 4) {
                    pa += 256; pb += 256;
#pragma unroll
                    for (int u = 0; u < 4; ++u) { an[u] = pa[64 * u]; bn[u] = pb[64 * u]; }
#pragma unroll
                    for (int u = 0; u < 4; ++u) l0 = mfma32(a[u], b[u], l0);
#pragma unroll
                    for (int u = 0; u < 4; ++u) { a[u] = an[u]; b[u] = bn[u]; }
                }
                pa += 256; pb += 256;
                // the remainder's operands, then the last full turn
                const int rem = KS - s - 4;
#pragma unroll
                for (int u = 0; u < 3; ++u) { const int o = (u < rem) ? 64 * u : 0; an[u] = pa[o]; bn[u] = pb[o]; }
#pragma unroll
                for (int u = 0; u < 4; ++u) l0 = mfma32(a[u], b[u], l0);
#pragma unroll
                for (int u = 0; u < 3; ++u) if (u < rem) l0 = mfma32(an[u], bn[u], l0);
            } else {
                for (; s < KS; ++s) l0 = mfma32(pa[64 * s], pb[64 * s], l0);
            }
        }
        // ---- sigmoid, overrides
        const int jrem = (je - j0 < 32) ? (int)(je - j0) : 32;
        const float2 *mts = reinterpret_cast<const float2 *>(lds + L.mt) + (buf * 4 + w) * 32;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const float2 mt = mts[acc_row(v, h)];
            if ((v & 3) == 0) __builtin_amdgcn_sched_barrier(0);     // four entries at a time: bounded register use
            const float x = mt.x - l0[v];
            if constexpr (BOUND) {
                // softplus, safe at both ends: exp of a non-positive number, log1p of a number in [0, 1]
                float g = fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x)));
                if ((__float_as_uint(mt.y) >> c) & 1u) g = x;    // X != 0: log pi - Lambda
                if (mt.x == -INFINITY) g = 0.0f;                 // a gene that is left out (inert padding)
                l0[v] = g;
                continue;
            }
            float p = __builtin_amdgcn_rcpf(1.0f + __expf(-x));
            if (mt.x == -INFINITY) p = 1e-10f;                   // pi_d <= 0                         zigap.py:133
            if ((__float_as_uint(mt.y) >> c) & 1u) p = 1.0f;     // X != 0: f32(1 - 1e-10) == 1       zigap.py:135
            l0[v] = p;
        }
        if (!(jrem == 32 && i0w + 32 <= n)) {                    // (uniform) padding never reaches a sum
#pragma unroll
            for (int v = 0; v < 16; ++v) if (!rowok || acc_row(v, h) >= jrem) l0[v] = 0.f;
        }
        if constexpr (STORE) {
#pragma unroll
            for (int v = 0; v < 16; ++v) T[c * TS + acc_row(v, h)] = l0[v];
        }
        if constexpr (BOUND) {                                   // 16 genes of the cell in float32, then the float64 carry
            float t = l0[0];
#pragma unroll
            for (int v = 1; v < 16; ++v) t += l0[v];
            bsum += (double)t;
        }
        __builtin_amdgcn_wave_barrier();
        stage_store(buf ^ 1);
        meta_store(buf ^ 1);
        ORIANA_VMEM_FENCE();
        // ---- D_hat rows out, column sums of the tile
        if constexpr (STORE) {
            const int gq = (lane & 7) * 4;
            const bool full = vec_ok && jrem == 32;              // uniform: whole 16-byte pieces
            f4v csum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = (lane >> 3) + 8 * q;
                const f4v t = *reinterpret_cast<const f4v *>(T + r * TS + gq);
                csum += t;
                const int64_t i = i0w + r;
                if (D_hat && i < n) {
                    float *dst = D_hat + i * m + j0 + gq;
                    if (full) *reinterpret_cast<f4v *>(dst) = t;
                    else {
                        if (gq + 0 < jrem) dst[0] = t.x;
                        if (gq + 1 < jrem) dst[1] = t.y;
                        if (gq + 2 < jrem) dst[2] = t.z;
                        if (gq + 3 < jrem) dst[3] = t.w;
                    }
                }
            }
            if (colsum) {
                csum.x = sum_mod8(csum.x); csum.y = sum_mod8(csum.y); csum.z = sum_mod8(csum.z); csum.w = sum_mod8(csum.w);
                if (lane < 8) *reinterpret_cast<f4v *>(lds + L.cs + (par * 4 + w) * 32 + gq) = csum;
            }
        }
        // ---- DV += D V_next
        if (!BOUND && Vn) {
            const float *v2 = lds + L.v2 + buf * 32 * L.v2s + c;
            float bc[NT], bn[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bc[nt] = v2[acc_row(0, h) * L.v2s + nt * 32];
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int gn = acc_row(v < 15 ? v + 1 : 15, h);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bn[nt] = v2[gn * L.v2s + nt * 32];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) dv[nt] = mfma32(l0[v], bc[nt], dv[nt]);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bc[nt] = bn[nt];
                __builtin_amdgcn_sched_barrier(0);
            }
            if (++since_flush == 8) {                            // 256 genes: leave the matrix core
                since_flush = 0;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int v = 0; v < 16; ++v) { dvs[nt][v] += dv[nt][v]; dv[nt][v] = 0.f; }
            }
        }
        __syncthreads();
        buf ^= 1;
        par ^= 1;
    }
    if constexpr (STORE) { if (jb < je) colsum_flush(jb + ((je - jb - 1) / 32) * 32, par ^ 1); }
    if constexpr (BOUND) {
        bsum += __shfl_xor(bsum, 32);                            // the other half of the cell's genes
        if (h == 0 && rowok) colsum[(int64_t)blockIdx.y * n + i0w + c] = bsum;
    }
    if (!BOUND && Vn && DV) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int64_t i = i0w + acc_row(v, h);
                const int k = nt * 32 + c;
                if ((RATE ? dn::cell_active(active, i, n) : i < n) && k < K)
                    atomicAdd(&DV[i * K + k], (double)dvs[nt][v] + (double)dv[nt][v]);
            }
    }
}

// out[j, k] += sum_i D[i, j] W[i, k]: a wave owns 32 * GQ genes (lane c: genes jw + GQ c ... + GQ - 1, one vector
// load per row) and NT * 32 factors; the 4 waves of a group share the rows [ib, ie) and the W chunks staged in LDS.
// A = D^T (m index = gene slot), B = W chunk; per row pair GQ * NT matrix instructions.
template <int NT, int GQ>
__global__ __launch_bounds__(256, (NT < 4) ? 2 : 1) void k_dt_times_factor_f32(double *__restrict__ out, const float *__restrict__ D,
                                                             const double *__restrict__ W, int64_t n, int64_t m, int K,
                                                             int64_t i_per_split) {
    constexpr int WS = (NT & 1) ? NT * 32 : NT * 32 + 32;       // rows one apart = 32 banks apart
    constexpr int RC = (NT > 2) ? 32 : 64;                       // rows per staged chunk
    __shared__ float Ws[2][RC * WS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int64_t jw = ((int64_t)blockIdx.x * 4 + w) * (32 * GQ);
    const int64_t ib = (int64_t)blockIdx.y * i_per_split;
    const int64_t ie = (ib + i_per_split < n) ? ib + i_per_split : n;
    const bool vec_ok = (m % GQ) == 0;
    const int64_t j = jw + GQ * c;

    f16v acc[GQ][NT], accs[GQ][NT];                             // matrix-core accumulators; their sums every 256 rows
#pragma unroll
    for (int q = 0; q < GQ; ++q)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int v = 0; v < 16; ++v) { acc[q][nt][v] = 0.f; accs[q][nt][v] = 0.f; }

    // W chunk staging, a quarter (PF row pairs = 16 rows) at a time: 16 threads per row, loads issued ahead of the
    // matrix instructions of a group and stored to LDS after them
    constexpr int PF = 8;                                        // row pairs per group, and in flight
    constexpr int NW = NT * 2;                                   // 16 * NW = NT * 32 factors
    const int sr = tid >> 4, sk = tid & 15;
    double wreg[NW];
    // (clamped addresses, padding zeroed when the values are stored: straight-line loads that the compiler leaves where
    //  they are issued -- a load under a branch drags its conversion, and with it the wait, up to the load)
    bool wok = false;
    auto stage_load = [&](int64_t i0, int grp) {
        const int64_t i = i0 + grp * 2 * PF + sr;
        wok = i < ie;
        const double *src = W + (wok ? i : ie - 1) * K;
#pragma unroll
        for (int u = 0; u < NW; ++u) {
            const int kk = sk + 16 * u;
            wreg[u] = src[kk < K ? kk : K - 1];
        }
    };
    auto stage_store = [&](int buf, int grp) {
        const int r = grp * 2 * PF + sr;
#pragma unroll
        for (int u = 0; u < NW; ++u)                             // (a product, not a select: the load stays unconditional)
            Ws[buf][r * WS + sk + 16 * u] = (float)wreg[u] * ((wok && sk + 16 * u < K) ? 1.f : 0.f);
    };
    struct Frag { float d[GQ]; };
    auto load_d = [&](Frag &f, int64_t i) {
#pragma unroll
        for (int q = 0; q < GQ; ++q) f.d[q] = 0.f;
        if (i < ie && j < m) {
            const float *src = D + i * m + j;
            if (GQ == 4 && vec_ok && j + 4 <= m) {
                const float4 t = *reinterpret_cast<const float4 *>(src);
                f.d[0] = t.x; f.d[1 % GQ] = t.y; f.d[2 % GQ] = t.z; f.d[3 % GQ] = t.w;
            } else if (GQ == 2 && vec_ok && j + 2 <= m) {
                const float2 t = *reinterpret_cast<const float2 *>(src);
                f.d[0] = t.x; f.d[1 % GQ] = t.y;
            } else {
#pragma unroll
                for (int q = 0; q < GQ; ++q) if (j + q < m) f.d[q] = src[q];
            }
        }
    };

    // ring of RING row pairs: the slot a matrix instruction has just consumed is refilled with the pair RING steps ahead
    constexpr int RING = 2 * PF;
    constexpr int NG = RC / (2 * PF);                            // staging groups (PF row pairs) per chunk
    static_assert(RC / 2 % RING == 0, "a chunk is a whole number of ring turns");
    Frag ring[RING];
    if (ib < ie) {
#pragma unroll
        for (int g = 0; g < NG; ++g) { stage_load(ib, g); stage_store(0, g); }
#pragma unroll
        for (int p = 0; p < RING; ++p) load_d(ring[p], ib + 2 * p + h);
    }
    __syncthreads();
    int buf = 0, chunks = 0;
    // interior of the matrix (every row the ring will ask for exists, the wave's genes are whole vectors): one
    // vector load from a running pointer per row pair, nothing else
    typedef float dvec __attribute__((ext_vector_type(GQ == 1 ? 2 : GQ)));   // (GQ == 1 takes the scalar branch)
    const bool wave_fast = vec_ok && jw + 32 * GQ <= m;
    // One step = one row pair: the B operands of the NEXT step are requested, the matrix instructions of this step
    // issued, the ring slot refilled -- and a full scheduling fence: the order below is the schedule (left to itself
    // the scheduler sinks the prefetches down to their uses, i.e. exposes every latency they were written to hide).
    auto chunk = [&](auto fast_tag, int64_t i0, bool more) {
        constexpr bool FAST = decltype(fast_tag)::value;
        const float *dp = D + (i0 + 2 * RING + h) * m + j;       // (dereferenced on the fast path only)
        const int64_t dstep = 2 * m;
        float bc[NT], bn[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bc[nt] = Ws[buf][h * WS + c + nt * 32];
#pragma unroll 1
        for (int t = 0; t < RC / 2 / RING; ++t) {
#pragma unroll
            for (int gg = 0; gg < 2; ++gg) {
                const int g = 2 * t + gg, s0 = g * PF;
                stage_load(more ? i0 + RC : i0, g);              // (unconditional; the last chunk is staged again, unread)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int p = 0; p < PF; ++p) {
                    const int sn = (s0 + p + 1 < RC / 2) ? s0 + p + 1 : RC / 2 - 1;
                    const float *wrow = &Ws[buf][(2 * sn + h) * WS + c];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bn[nt] = wrow[nt * 32];
                    __builtin_amdgcn_sched_barrier(0);
                    Frag &f = ring[gg * PF + p];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int q = 0; q < GQ; ++q) acc[q][nt] = mfma32(f.d[q], bc[nt], acc[q][nt]);
                    if (FAST) {
                        if (GQ == 1) f.d[0] = *dp;
                        else {
                            const dvec tv = *reinterpret_cast<const dvec *>(dp);
#pragma unroll
                            for (int q = 0; q < GQ; ++q) f.d[q] = tv[q];
                        }
                        dp += dstep;
                    } else {
                        load_d(f, i0 + 2 * (s0 + p + RING) + h);
                    }
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bc[nt] = bn[nt];
                    __builtin_amdgcn_sched_barrier(0);
                }
                stage_store(buf ^ 1, g);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    for (int64_t i0 = ib; i0 < ie; i0 += RC) {
        const bool more = i0 + RC < ie;
        if (wave_fast && i0 + RC + 2 * RING <= ie) chunk(std::true_type{}, i0, more);
        else chunk(std::false_type{}, i0, more);
        if (++chunks == 256 / RC) {                              // 256 rows: leave the matrix core
            chunks = 0;
#pragma unroll
            for (int q = 0; q < GQ; ++q)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int v = 0; v < 16; ++v) { accs[q][nt][v] += acc[q][nt][v]; acc[q][nt][v] = 0.f; }
        }
        __syncthreads();
        buf ^= 1;
    }
#pragma unroll
    for (int q = 0; q < GQ; ++q)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int64_t jj = jw + GQ * acc_row(v, h) + q;
                const int k = nt * 32 + c;
                if (jj < m && k < K) atomicAdd(&out[jj * K + k], (double)accs[q][nt][v] + (double)acc[q][nt][v]);
            }
}

// ------------------------------------------------------------------------------------------------------------------
// The same sweep kernel with every float32 product evaluated on the bf16 matrix cores: x = hi + mid + lo (three bf16,
// 24 bits, split by truncation so that the remainders are exact) and six of the nine cross products
// (hi hi, hi mid, mid hi, mid mid, hi lo, lo hi; the three dropped ones are below 2^-24 of the product), accumulated in
// float32 by v_mfma_f32_32x32x16_bf16.  tools/ubench/mfma_bf16x3.hip: the error of a sum of <= 512 positive terms is
// that of the float32 FMA chain (2.9e-7 rms at 512), at 2.7 x the rate of v_mfma_f32_32x32x2_f32 after the six-fold
// overhead.  K <= 64.  Fragment map of v_mfma_f32_32x32x16_bf16: A[m = lane & 31][k = 8 (lane >> 5) + e],
// B[k = 8 (lane >> 5) + e][n = lane & 31], e = 0..7 the eight bf16 (four dwords) of the lane; D as for the float32
// 32 x 32 instructions.  The splits (split2, split8), mfma_b16 and the macro of the six products are dense_tiles.h's.

// LDS carve-up of k_dropout_sweep_b16 (bytes): operand images are [..][split][lane] x 16 bytes
struct B16Lds {
    int vt, v2, mt, tb, cs, total;
    __host__ __device__ B16Lds(int KC, int NT) {
        int o = 0;
        vt = o; o += 2 * KC * 3 * 64 * 16;           // [buf][k chunk][split][lane]: A operand of Lambda^T = V U^T
        v2 = o; o += 2 * NT * 2 * 3 * 64 * 16;       // [buf][n tile][instruction][split][lane]: B operand of D V_next
        mt = o; o += 2 * 4 * 32 * 2 * 4;             // [buf][wave][32 genes] {logit(pi_d), mask word}
        tb = o; o += 4 * 32 * TS * 4;                // [wave][32 cells][32 genes] transpose buffer
        cs = o; o += 2 * 4 * 32 * 4;                 // [parity][wave][32 genes] column partial sums
        total = o;
    }
};

// The operand images of a gene tile are the same for every row block: they are built ONCE per sweep, in the layout
// the kernel copies into LDS, by this pre-kernel (one work-group per tile of 32 genes):
//   first image  [k chunk][split][lane = 32 (G & 1) + g]: V[g][8 G .. 8 G + 7], thread (g = tid & 31, G = tid >> 5);
//   second image [n tile][instruction q][split][lane = 32 hh + cc]: V_next[gene(q, hh, e)][32 nt + cc], e = 0..7, the
//                genes in the order the accumulator registers of the first product hold them (acc_row).
template <int NT, int KC>
__global__ __launch_bounds__(256) void k_split_images(u4v *__restrict__ img1, u4v *__restrict__ img2,
                                                      const double *__restrict__ V, const double *__restrict__ Vn,
                                                      int64_t m, int K) {
    const int tid = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * 32;
    {
        const int g = tid & 31, G = tid >> 5;
        if (G < 2 * KC) {
            const int64_t j = j0 + g;
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int kk = 8 * G + e;
                x[e] = (j < m && kk < K) ? (float)V[j * K + kk] : 0.f;
            }
            u4v o[3];
            split8(x, o);
            u4v *dst = img1 + (int64_t)blockIdx.x * (KC * 3 * 64) + ((G >> 1) * 3) * 64 + (G & 1) * 32 + g;
#pragma unroll
            for (int sp = 0; sp < 3; ++sp) dst[sp * 64] = o[sp];
        }
    }
    if (Vn) {
        const int nt = tid >> 7, q = (tid >> 6) & 1, hh = (tid >> 5) & 1, cc = tid & 31;
        if (nt < NT) {
            const int kk = nt * 32 + cc;
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int64_t j = j0 + acc_row(8 * q + e, hh);
                x[e] = (j < m && kk < K) ? (float)Vn[j * K + kk] : 0.f;
            }
            u4v o[3];
            split8(x, o);
            u4v *dst = img2 + (int64_t)blockIdx.x * (NT * 2 * 3 * 64) + ((nt * 2 + q) * 3) * 64 + hh * 32 + cc;
#pragma unroll
            for (int sp = 0; sp < 3; ++sp) dst[sp * 64] = o[sp];
        }
    }
}

template <int NT, int KC, bool RATE = false>        // RATE: as k_dropout_sweep
__global__ __launch_bounds__(256, 2) void k_dropout_sweep_b16(float *__restrict__ D_hat, const double *__restrict__ U,
                                                              const u4v *__restrict__ img1, const float *__restrict__ lgit,
                                                              const uint32_t *__restrict__ nzmask,
                                                              double *__restrict__ colsum, const u4v *__restrict__ img2,
                                                              double *__restrict__ DV, int64_t n, int64_t m, int K,
                                                              int64_t j_per_split, const uint8_t *__restrict__ active) {
    extern __shared__ float lds[];
    char *ldsb = reinterpret_cast<char *>(lds);
    const B16Lds L(KC, NT);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int64_t i0w = (int64_t)blockIdx.x * 128 + w * 32;
    const int64_t jb = (int64_t)blockIdx.y * j_per_split;
    const int64_t je = (jb + j_per_split < m) ? jb + j_per_split : m;
    float *T = reinterpret_cast<float *>(ldsb + L.tb) + w * 32 * TS;
    u4v *vt_img = reinterpret_cast<u4v *>(ldsb + L.vt);
    u4v *v2_img = reinterpret_cast<u4v *>(ldsb + L.v2);
    if constexpr (RATE) {
        if (!dn::any_active<128>(active, (int64_t)blockIdx.x * 128, n, lane)) return;     // (work-group uniform)
    }

    // the wave's strip of U_hat as the B operand of the first product: per k chunk, factors 16 kc + 8 h + e of cell c
    u4v ub[KC][3];
    {
        const int64_t i = i0w + c;
        const bool on = RATE ? dn::cell_active(active, i, n) : i < n;
        const double *urow = U + (RATE ? (on ? i : 0) : (i < n ? i : n - 1)) * K;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int kk = 16 * kc + 8 * h + e;
                x[e] = (on && kk < K) ? (float)urow[kk < K ? kk : K - 1] : 0.f;
            }
            split8(x, ub[kc]);
        }
    }

    // Staging of one gene tile: straight 16-byte copies of the two operand images k_split_images has built (loads at
    // the top of the previous tile, consumed right before that tile's stores: see k_dropout_sweep).
    constexpr int N1 = KC * 3 * 64, N2 = NT * 2 * 3 * 64;        // 16-byte pieces per image
    constexpr int R1 = (N1 + 255) / 256, R2 = (N2 + 255) / 256;
    const bool has_next = img2 != nullptr;
    u4v sreg[R1], nreg[R2];
    uint32_t mkreg = 0;
    auto stage_load = [&](int64_t j0) {
        const int64_t tile = j0 >> 5;
        const u4v *s1 = img1 + tile * N1;
#pragma unroll
        for (int r = 0; r < R1; ++r) { const int idx = tid + 256 * r; sreg[r] = s1[idx < N1 ? idx : N1 - 1]; }
        if (has_next) {
            const u4v *s2 = img2 + tile * N2;
#pragma unroll
            for (int r = 0; r < R2; ++r) { const int idx = tid + 256 * r; nreg[r] = s2[idx < N2 ? idx : N2 - 1]; }
        }
    };
    auto stage_store = [&](int buf) {
#pragma unroll
        for (int r = 0; r < R1; ++r) { const int idx = tid + 256 * r; if (N1 % 256 == 0 || idx < N1) vt_img[buf * N1 + idx] = sreg[r]; }
        if (has_next) {
#pragma unroll
            for (int r = 0; r < R2; ++r) { const int idx = tid + 256 * r; if (N2 % 256 == 0 || idx < N2) v2_img[buf * N2 + idx] = nreg[r]; }
        }
    };
    const int mw = (tid >> 5) & 3;
    const int64_t mrow = ((int64_t)blockIdx.x * 128 + mw * 32) >> 5;
    const bool mrow_ok = nzmask && (int64_t)blockIdx.x * 128 + mw * 32 < n;
    float lgreg = 0.f;
    auto meta_load = [&](int64_t j0) {
        if (tid < 128) {
            const int64_t jj = j0 + (tid & 31);
            const int64_t jc = jj < je ? jj : je - 1;
            lgreg = lgit[jc];
            mkreg = mrow_ok ? nzmask[mrow * m + jc] : 0u;
        }
    };
    auto meta_store = [&](int buf) {
        if (tid < 128) {
            float2 pr;
            pr.x = lgreg;
            pr.y = __uint_as_float(mkreg);
            *reinterpret_cast<float2 *>(ldsb + L.mt + (((buf * 4 + mw) * 32 + (tid & 31)) * 2) * 4) = pr;
        }
    };

    f16v dv[NT], dvs[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int v = 0; v < 16; ++v) { dv[nt][v] = 0.f; dvs[nt][v] = 0.f; }
    }
    const bool rowok = i0w + c < n;
    const bool vec_ok = (m & 3) == 0;
    float *csb = reinterpret_cast<float *>(ldsb + L.cs);

    if (jb < je) {
        stage_load(jb);
        meta_load(jb);
        stage_store(0);
        meta_store(0);
    }
    __syncthreads();
    int buf = 0, par = 0, since_flush = 0;
    auto colsum_flush = [&](int64_t jt, int parity) {
        if (colsum && w == 0 && lane < 32 && jt + lane < je) {
            const float *cs = csb + parity * 4 * 32 + lane;
            atomicAdd(&colsum[jt + lane], (double)cs[0] + (double)cs[32] + (double)cs[64] + (double)cs[96]);
        }
    };
    for (int64_t j0 = jb; j0 < je; j0 += 32) {
        const bool more = j0 + 32 < je;
        { const int64_t jn = more ? j0 + 32 : j0; stage_load(jn); meta_load(jn); }   // (the last tile again: unused)
        if constexpr (!RATE) { if (j0 > jb) colsum_flush(j0 - 32, par ^ 1); }
        ORIANA_VMEM_FENCE();
        // ---- Lambda^T = V U^T
        f16v l0;
#pragma unroll
        for (int v = 0; v < 16; ++v) l0[v] = 0.f;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
            const u4v *src = vt_img + buf * N1 + (kc * 3) * 64 + lane;
            u4v a[3];
#pragma unroll
            for (int sp = 0; sp < 3; ++sp) a[sp] = src[sp * 64];
            ORIANA_DN_MF6(l0, a, ub[kc]);
        }
        // ---- sigmoid, overrides
        const int jrem = (je - j0 < 32) ? (int)(je - j0) : 32;
        const float2 *mts = reinterpret_cast<const float2 *>(ldsb + L.mt) + (buf * 4 + w) * 32;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const float2 mt = mts[acc_row(v, h)];
            if ((v & 3) == 0) __builtin_amdgcn_sched_barrier(0);
            const float x = mt.x - l0[v];
            float p = __builtin_amdgcn_rcpf(1.0f + __expf(-x));
            if (mt.x == -INFINITY) p = 1e-10f;                   // pi_d <= 0                         zigap.py:133
            if ((__float_as_uint(mt.y) >> c) & 1u) p = 1.0f;     // X != 0: f32(1 - 1e-10) == 1       zigap.py:135
            l0[v] = p;
        }
        if (!(jrem == 32 && i0w + 32 <= n)) {                    // (uniform) padding never reaches a sum
#pragma unroll
            for (int v = 0; v < 16; ++v) if (!rowok || acc_row(v, h) >= jrem) l0[v] = 0.f;
        }
        if constexpr (!RATE) {
#pragma unroll
            for (int v = 0; v < 16; ++v) T[c * TS + acc_row(v, h)] = l0[v];
        }
        __builtin_amdgcn_wave_barrier();
        stage_store(buf ^ 1);
        meta_store(buf ^ 1);
        ORIANA_VMEM_FENCE();
        // ---- D_hat rows out, column sums of the tile
        if constexpr (!RATE) {
            const int gq = (lane & 7) * 4;
            const bool full = vec_ok && jrem == 32;
            f4v csum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = (lane >> 3) + 8 * q;
                const f4v t = *reinterpret_cast<const f4v *>(T + r * TS + gq);
                csum += t;
                const int64_t i = i0w + r;
                if (D_hat && i < n) {
                    float *dst = D_hat + i * m + j0 + gq;
                    if (full) *reinterpret_cast<f4v *>(dst) = t;
                    else {
                        if (gq + 0 < jrem) dst[0] = t.x;
                        if (gq + 1 < jrem) dst[1] = t.y;
                        if (gq + 2 < jrem) dst[2] = t.z;
                        if (gq + 3 < jrem) dst[3] = t.w;
                    }
                }
            }
            if (colsum) {
                csum.x = sum_mod8(csum.x); csum.y = sum_mod8(csum.y); csum.z = sum_mod8(csum.z); csum.w = sum_mod8(csum.w);
                if (lane < 8) *reinterpret_cast<f4v *>(csb + (par * 4 + w) * 32 + gq) = csum;
            }
        }
        // ---- DV += D V_next: the accumulator registers 8 q .. 8 q + 7 are the eight k slots of instruction q
        if (has_next) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float x[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = l0[8 * q + e];
                u4v a[3];
                split8(x, a);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const u4v *src = v2_img + buf * N2 + ((nt * 2 + q) * 3) * 64 + lane;
                    u4v b[3];
#pragma unroll
                    for (int sp = 0; sp < 3; ++sp) b[sp] = src[sp * 64];
                    ORIANA_DN_MF6(dv[nt], a, b);
                }
            }
            if (++since_flush == 8) {                            // 256 genes: leave the matrix core
                since_flush = 0;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int v = 0; v < 16; ++v) { dvs[nt][v] += dv[nt][v]; dv[nt][v] = 0.f; }
            }
        }
        __syncthreads();
        buf ^= 1;
        par ^= 1;
    }
    if constexpr (!RATE) { if (jb < je) colsum_flush(jb + ((je - jb - 1) / 32) * 32, par ^ 1); }
    if (has_next && DV) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int64_t i = i0w + acc_row(v, h);
                const int k = nt * 32 + c;
                if ((RATE ? dn::cell_active(active, i, n) : i < n) && k < K)
                    atomicAdd(&DV[i * K + k], (double)dvs[nt][v] + (double)dv[nt][v]);
            }
    }
}

// logit(pi_d) in float32, with the overrides of zigap.py:133-134 encoded as -inf (pi_d <= 0: p_d = 1e-10) and +inf
// (pi_d >= 1: p_d = 1 - 1e-10, 1 in float32)
// [r5] lgs (may be NULL): the same as -logit * log2(e) -- the form dn::k_zi_row takes: its sigmoid is
// 1 / (1 + exp2(fma(Lambda, log2 e, lgs))), one fused multiply-add where the subtraction and the scaling were two instructions
// per entry (floating-point vector work beside matrix instructions is the dear kind on this part, DESIGN_HISTORY.md 10 i)
// [r6] flo (with lgs): the floor dn::k_zi_row ADDS to its sigmoid -- 1e-10 where pi_d <= 0 (there lgs = +inf makes the sigmoid
// +0: the column override of zigap.py:133 as one addition), 0 elsewhere.
__global__ void k_logit_f32(float *__restrict__ lg, float *__restrict__ lgs, float *__restrict__ flo,
                            const double *__restrict__ pi_d, int64_t m) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const double pi = pi_d[j];
    const float v = (pi <= 0.0) ? -INFINITY : (pi >= 1.0) ? INFINITY : (float)logit_f64(pi);
    lg[j] = v;
    if (lgs) { lgs[j] = -v * 1.4426950408889634f; flo[j] = (pi <= 0.0) ? 1e-10f : 0.0f; }
}

template <int NT, bool RATE = false>
static int launch_sweep(float *D_hat, const double *U, const double *V, const float *pi_d, const uint32_t *nzmask,
                        double *colsum, const double *Vn, double *DV, int64_t n, int64_t m, int K, hipStream_t st,
                        const uint8_t *active = nullptr) {
    const int KP2 = (K + 1) & ~1;
    const SweepLds L(KP2, NT);
    const size_t lds = (size_t)L.total * sizeof(float);
    const int64_t rb = (n + 127) / 128;
    // gene ranges: whole tiles of 32, as many per row block as fills the chip's work-group slots evenly
    const int64_t splits0 = dn::pick_splits(rb, (m + 255) / 256, dn::SPLITS_F32);
    int64_t jps = (m + splits0 - 1) / splits0;
    jps = (jps + 31) / 32 * 32;
    const int64_t splits = (m + jps - 1) / jps;
    if (splits > 65535 || rb > 0x7fffffffLL) return ORIANA_EINVAL;
    return launch(k_dropout_sweep<NT, RATE>, dim3((unsigned)rb, (unsigned)splits), dim3(256), lds, st, D_hat, U, V, pi_d, nzmask, colsum,
                  Vn, DV, n, m, K, KP2, jps, active);
}

// ------------------------------------------------------------------------------------------------------------------
// out[j, k] += sum_i D[i, j] W[i, k] with the products on the bf16 matrix cores (three-way splits, six cross products).
// W is split ONCE per call into per-chunk operand images (k_split_rows: 16 rows per chunk, [n tile][split][lane =
// 32 hh + cc]: W[16 chunk + 8 hh + e][32 nt + cc], e = 0..7); D is split on the fly -- it is read exactly once.
// A wave owns 32 genes x NT * 32 factors: A[m = gene c][k = cell 8 h + e] comes from eight 4-byte loads per lane and
// chunk (128-byte row pieces per half-wave), four chunks ahead in a register ring; B from the staged images.
template <int NT>
__global__ __launch_bounds__(256) void k_split_rows(u4v *__restrict__ img, const double *__restrict__ W, int64_t n, int K) {
    const int tid = threadIdx.x;
    const int nt = tid >> 6, hh = (tid >> 5) & 1, cc = tid & 31;
    if (nt >= NT) return;
    const int64_t i0 = (int64_t)blockIdx.x * 16 + 8 * hh;
    const int kk = nt * 32 + cc;
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (i0 + e < n && kk < K) ? (float)W[(i0 + e) * K + kk] : 0.f;
    u4v o[3];
    split8(x, o);
    u4v *dst = img + (int64_t)blockIdx.x * (NT * 3 * 64) + (nt * 3) * 64 + hh * 32 + cc;
#pragma unroll
    for (int sp = 0; sp < 3; ++sp) dst[sp * 64] = o[sp];
}

template <int NT>
__global__ __launch_bounds__(256, 2) void k_dt_times_factor_b16(double *__restrict__ out, const float *__restrict__ D,
                                                                const u4v *__restrict__ img, int64_t n, int64_t m, int K,
                                                                int64_t i_per_split) {
    constexpr int CH = 2;                                        // chunks (of 16 rows) per staged group and in the ring
                                                                 // (4: > 256 registers, the slow path's index arithmetic)
    constexpr int NP = NT * 3 * 64;                              // 16-byte pieces per chunk image
    constexpr int RS = (CH * NP + 255) / 256;                    // staged pieces per thread and group
    __shared__ u4v Ws[2][CH * NP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int64_t jw = ((int64_t)blockIdx.x * 4 + w) * 32;
    const int64_t ib = (int64_t)blockIdx.y * i_per_split;       // multiple of 64 (whole groups)
    const int64_t ie = (ib + i_per_split < n) ? ib + i_per_split : n;
    const int64_t j = jw + c;

    f16v acc[NT], accs[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int v = 0; v < 16; ++v) { acc[nt][v] = 0.f; accs[nt][v] = 0.f; }

    u4v wreg[RS];
    auto stage_load = [&](int64_t i0) {                         // (i0 a multiple of 64; images exist for every chunk of n)
        const u4v *src = img + (i0 >> 4) * NP;
        const int64_t avail = (((n + 15) >> 4) - (i0 >> 4)) * NP;           // pieces left in the image array
#pragma unroll
        for (int r = 0; r < RS; ++r) {
            const int idx = tid + 256 * r;
            wreg[r] = src[(idx < CH * NP && idx < avail) ? idx : 0];
        }
    };
    auto stage_store = [&](int buf) {
#pragma unroll
        for (int r = 0; r < RS; ++r) { const int idx = tid + 256 * r; if ((CH * NP) % 256 == 0 || idx < CH * NP) Ws[buf][idx] = wreg[r]; }
    };
    float ring[CH][8];
    auto load_checked = [&](float (&x)[8], int64_t i0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int64_t i = i0 + 8 * h + e;
            x[e] = (i < ie && j < m) ? D[i * m + j] : 0.f;
        }
    };
    const bool wave_fast = jw + 32 <= m;
    if (ib < ie) {
        stage_load(ib);
        stage_store(0);
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) load_checked(ring[ch], ib + 16 * ch);
    }
    __syncthreads();
    int buf = 0, groups = 0;
    // one staged group = CH chunks; FAST: every row the ring will ask for exists and the wave's genes are inside the
    // matrix -- one running pointer, eight plain loads per chunk
    auto group = [&](auto fast_tag, int64_t i0, bool more) {
        constexpr bool FAST = decltype(fast_tag)::value;
        const float *dp = D + (i0 + 16 * CH + 8 * h) * m + j;    // (dereferenced on the fast path only)
        stage_load(more ? i0 + 16 * CH : i0);                    // (unconditional: the last group is staged again, unread)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            u4v a[3];
            split8(ring[ch], a);
            // the slot just consumed takes the chunk one group ahead
            if (FAST) {
                const float *r = dp;
#pragma unroll
                for (int e = 0; e < 8; ++e) { ring[ch][e] = *r; r += m; }
                dp += 16 * m;
            } else {
                load_checked(ring[ch], i0 + 16 * (ch + CH));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const u4v *src = &Ws[buf][ch * NP + (nt * 3) * 64 + lane];
                u4v b[3];
#pragma unroll
                for (int sp = 0; sp < 3; ++sp) b[sp] = src[sp * 64];
                ORIANA_DN_MF6(acc[nt], a, b);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        stage_store(buf ^ 1);
    };
    for (int64_t i0 = ib; i0 < ie; i0 += 16 * CH) {
        const bool more = i0 + 16 * CH < ie;
        if (wave_fast && i0 + 32 * CH <= ie) group(std::true_type{}, i0, more);
        else group(std::false_type{}, i0, more);
        if (++groups == 16 / CH) {                               // 256 rows: leave the matrix core
            groups = 0;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int v = 0; v < 16; ++v) { accs[nt][v] += acc[nt][v]; acc[nt][v] = 0.f; }
        }
        __syncthreads();
        buf ^= 1;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int64_t jj = jw + acc_row(v, h);
            const int k = nt * 32 + c;
            if (jj < m && k < K) atomicAdd(&out[jj * K + k], (double)accs[nt][v] + (double)acc[nt][v]);
        }
}

template <int NT>
static int launch_dt_b16(double *out, const float *D, const double *W, float *scratch, int64_t n, int64_t m, int K,
                         hipStream_t st) {
    if (!scratch || !dn::aligned16(scratch)) return ORIANA_EINVAL;
    u4v *img = reinterpret_cast<u4v *>(scratch);
    const int64_t jb = (m + 127) / 128;
    const int64_t splits0 = dn::pick_splits(jb, (n + 255) / 256, dn::SPLITS_F32);
    int64_t ips = (n + splits0 - 1) / splits0;
    ips = (ips + 63) / 64 * 64;                                  // whole staged groups
    const int64_t splits = (n + ips - 1) / ips;
    if (splits > 65535 || jb > 0x7fffffffLL || (n + 15) / 16 > 0x7fffffffLL) return ORIANA_EINVAL;
    const int rc = launch(k_split_rows<NT>, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, img, W, n, K);
    if (rc) return rc;
    return launch(k_dt_times_factor_b16<NT>, dim3((unsigned)jb, (unsigned)splits), dim3(256), 0, st, out, D, img, n, m, K, ips);
}

// scratch of oriana_dropout_sweep_fused (floats): logit(pi_d) [m rounded up to 64] | first images | second images
static inline int64_t b16_img_floats(int64_t m, int pieces) { return ((m + 31) / 32) * (int64_t)pieces * 4; }

template <int NT, int KC, bool RATE = false>
static int launch_sweep_b16(float *D_hat, const double *U, const double *V, const float *lg, const uint32_t *nzmask,
                            double *colsum, const double *Vn, double *DV, float *img_scratch, int64_t n, int64_t m,
                            int K, hipStream_t st, const uint8_t *active = nullptr) {
    const B16Lds L(KC, NT);
    const size_t lds = (size_t)L.total;
    u4v *img1 = reinterpret_cast<u4v *>(img_scratch);
    u4v *img2 = Vn ? reinterpret_cast<u4v *>(img_scratch + b16_img_floats(m, KC * 3 * 64)) : nullptr;
    const int rc = launch(k_split_images<NT, KC>, dim3((unsigned)((m + 31) / 32)), dim3(256), 0, st, img1, img2, V, Vn, m, K);
    if (rc) return rc;
    const int64_t rb = (n + 127) / 128;
    const int64_t splits0 = dn::pick_splits(rb, (m + 255) / 256, dn::SPLITS_F32);
    int64_t jps = (m + splits0 - 1) / splits0;
    jps = (jps + 31) / 32 * 32;
    const int64_t splits = (m + jps - 1) / jps;
    if (splits > 65535 || rb > 0x7fffffffLL) return ORIANA_EINVAL;
    return launch(k_dropout_sweep_b16<NT, KC, RATE>, dim3((unsigned)rb, (unsigned)splits), dim3(256), lds, st, D_hat, U, img1, lg, nzmask,
                  colsum, img2, DV, n, m, K, jps, active);
}

template <int NT, int GQ>
static int launch_dt(double *out, const float *D, const double *W, int64_t n, int64_t m, int K, hipStream_t st) {
    const int64_t jb = (m + 128 * GQ - 1) / (128 * GQ);
    const int64_t splits0 = dn::pick_splits(jb, (n + 255) / 256, dn::SPLITS_F32);
    int64_t ips = (n + splits0 - 1) / splits0;
    ips = (ips + 63) / 64 * 64;                                  // whole staged chunks
    const int64_t splits = (n + ips - 1) / ips;
    if (splits > 65535 || jb > 0x7fffffffLL) return ORIANA_EINVAL;
    return launch(k_dt_times_factor_f32<NT, GQ>, dim3((unsigned)jb, (unsigned)splits), dim3(256), 0, st, out, D, W, n, m, K, ips);
}

// ------------------------------------------------------------------------------------------------------------------
// oriana_zi_cell_bound: the dropout term of a held-out cell's bound by k_dropout_sweep<NT, false, true>.
// logit(pi~) in float32, pi~ = min(max(pi_d, 1e-10), 1 - 1e-10) -- the two override VALUES of zigap.py:133-134 instead of
// k_logit_f32's +-inf flags: every logit is finite (|.| <= 23.03).  Genes [m_real, m) are the inert padding: -inf = left out.
__global__ void k_logit_clamped_f32(float *__restrict__ lg, const double *__restrict__ pi_d, int64_t m, int64_t m_real) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const double pt = fmin(fmax(pi_d[j], 1e-10), 1.0 - 1e-10);
    lg[j] = (j < m_real) ? (float)(log(pt) - log1p(-pt)) : -INFINITY;
}

// out[i] = the partials of the gene ranges, added in the order of the ranges: every i < n is written
__global__ void k_cell_bound_combine(double *__restrict__ out, const double *__restrict__ partial, int64_t n, int64_t splits) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t sp = 0; sp < splits; ++sp) s += partial[sp * n + i];
    out[i] = s;
}

// Gene ranges of the bound: the entry runs ONCE per call (not once per iteration), so a small batch is cut until the
// work-groups fill the chip's slots once -- in whole tiles, at least two per range (a range stages the U strip of its own);
// from 512 row blocks on, one range.
struct BoundCut { int64_t jps, splits; };
static BoundCut bound_cut(int64_t n, int64_t m) {
    const int64_t rb = (n + 127) / 128, slots = 2 * oriana_device_cus();
    int64_t sp = slots / rb;
    if (sp > (m + 63) / 64) sp = (m + 63) / 64;
    if (sp > 65535) sp = 65535;
    if (sp < 1) sp = 1;
    int64_t jps = (m + sp - 1) / sp;
    jps = (jps + 31) / 32 * 32;
    return BoundCut{jps, (m + jps - 1) / jps};
}
static inline int64_t bound_logit_doubles(int64_t m) { return (m + 63) / 64 * 32; }      // m floats, rounded up to 64

template <int NT>
static int launch_bound(double *partial, const double *U, const double *V, const float *lg, const uint32_t *nzmask, int64_t n,
                        int64_t m, int K, BoundCut cut, hipStream_t st) {
    const int KP2 = (K + 1) & ~1;
    const SweepLds L(KP2, NT);
    const size_t lds = (size_t)L.total * sizeof(float);
    const int64_t rb = (n + 127) / 128;
    if (cut.splits > 65535 || rb > 0x7fffffffLL) return ORIANA_EINVAL;
    return launch(k_dropout_sweep<NT, false, true>, dim3((unsigned)rb, (unsigned)cut.splits), dim3(256), lds, st, nullptr, U, V, lg,
                  nzmask, partial, nullptr, nullptr, n, m, K, KP2, cut.jps, nullptr);
}

// ------------------------------------------------------------------------------------------------------------------
// oriana_zi_gene_rate: the gene-side rate statistic of a folded-in batch (ZIGaP.fold_in_fit),
//   G[j, k] = sum_i d_ij U[i, k],   dsum[j] = sum_i d_ij,   d the dropout posterior of oriana_zi_foldin_rate, never stored.
// The transposed twin of k_dropout_sweep<NT, true>: a work-group holds 4 strips of 32 GENES (the V strips resident in LDS,
// [k][gene]) and walks a range of CELL tiles, each staged in both images ([k][cell] and [cell][k]) by the sweep kernel's
// staging.  Lambda[cell, gene] = U V^T on the matrix core (A = the U tile, B = the wave's V strip), so a lane's 16 accumulator
// registers are 16 cells of ONE gene (c = lane & 31): the logit and its two overrides (k_logit_f32's +-inf flags) live in a
// register, the non-zero bits of the tile's 32 cells are one mask word per lane, and after the sigmoid the registers are the
// A operand of  G[gene, k] += d[gene, cell] U[cell, k].
// G stays in registers across the tiles: out of the matrix core every 256 cells (float32, as the sweep kernel), and every 4096
// cells into the range's own partial in float64 (a plain read-modify-write of memory no other work-group touches), so the
// float32 part of a sum never holds more than 16 pieces whatever the batch.  dsum: a tile's 16 values per lane in float32,
// the tiles in float64; cells i >= n have U = 0 (nothing to G) and d zeroed (nothing to dsum).  In a column with pi_d <= 0,
// float32 cannot hold 1 + 1e-10: its dsum is nnz + 1e-10 (cells - nnz) from the mask's population count, in float64.
// Every range WRITES its partials, k_gene_rate_combine adds them in order: no atomics, nothing pre-zeroed.
struct GeneLds {
    int vs, ut, u2, dm, total;
    int u2s;                      // row stride of the [cell][k] image (as SweepLds::v2s)
    __host__ __device__ GeneLds(int KP2, int NT) {
        u2s = NT * 32 + 8;
        int o = 0;
        vs = o; o += 4 * KP2 * 32;           // [wave][k][32 genes], resident
        ut = o; o += 2 * KP2 * 32;           // [buf][k][32 cells]
        u2 = o; o += 2 * 32 * u2s;           // [buf][32 cells][k]
        dm = o; o += 32;                     // where the staging writes of k >= KP2 land
        total = o;
    }
};

template <int NT>
__global__ __launch_bounds__(256, (NT <= 2) ? 2 : 1) void k_gene_rate(double *__restrict__ Gp, double *__restrict__ dp,
                                                                      const double *__restrict__ U, const double *__restrict__ V,
                                                                      const float *__restrict__ lgit,
                                                                      const uint32_t *__restrict__ nzmask, int64_t n, int64_t m,
                                                                      int K, int KP2, int64_t i_per_split) {
    extern __shared__ float lds[];
    const GeneLds L(KP2, NT);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
    const int64_t j0w = (int64_t)blockIdx.x * 128 + w * 32;
    const int64_t ib = (int64_t)blockIdx.y * i_per_split;        // a multiple of 32: whole mask words
    const int64_t ie = (ib + i_per_split < n) ? ib + i_per_split : n;
    const int KS = KP2 >> 1;
    float *Vs = lds + L.vs + w * KP2 * 32;

    // the wave's strip of V_hat, [k][gene]
    for (int e = lane; e < KP2 * 32; e += 64) {
        const int g = e / KP2, kk = e - g * KP2;
        const int64_t j = j0w + g;
        Vs[kk * 32 + g] = (j < m && kk < K) ? (float)V[j * K + kk] : 0.f;
    }
    // the lane's gene: its logit, and the address of its mask words (clamped: a gene >= m is computed and dropped)
    const int64_t jl = j0w + c;
    const bool jok = jl < m;
    const int64_t jc = jok ? jl : m - 1;
    const float lg = lgit[jc];

    // staging of one cell tile, 8 threads per cell (k_dropout_sweep's, both images from the same registers)
    const int sg = tid >> 3, sk = tid & 7;
    constexpr int NU = NT * 4;
    double sreg[NU];
    bool sok = false;
    auto stage_load = [&](int64_t i0) {
        const int64_t i = i0 + sg;
        sok = i < ie;
        const int64_t ic = sok ? i : ie - 1;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int kk = sk + 8 * u;
            sreg[u] = U[ic * K + (kk < K ? kk : K - 1)];
        }
    };
    auto stage_store = [&](int buf) {
        float *ut = lds + L.ut + buf * KP2 * 32;
        float *u2 = lds + L.u2 + buf * 32 * L.u2s;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int kk = sk + 8 * u;
            const float x = (sok && kk < K) ? (float)sreg[u] : 0.f;
            (kk < KP2 ? ut + kk * 32 : lds + L.dm)[sg] = x;
            u2[sg * L.u2s + kk] = x;
        }
    };

    f16v dv[NT], dvs[NT];                                       // matrix-core accumulators; their sums every 256 cells
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int v = 0; v < 16; ++v) { dv[nt][v] = 0.f; dvs[nt][v] = 0.f; }
    }
    // the range's partial of G: written the first time, added to after that
    bool spilled = false;
    auto spill = [&]() {
        int64_t row0 = (int64_t)blockIdx.y * m + j0w;
        asm volatile("" : "+v"(row0));                           // the 64 addresses are formed here, not kept across the tiles
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int64_t j = j0w + acc_row(v, h);
                const int k = nt * 32 + c;
                if (j < m && k < K) {
                    double *p = Gp + (row0 + acc_row(v, h)) * K + k;
                    const double s = (double)dvs[nt][v] + (double)dv[nt][v];
                    *p = spilled ? *p + s : s;
                }
                dvs[nt][v] = 0.f; dv[nt][v] = 0.f;
            }
        spilled = true;
    };
    double bsum = 0.0;                                           // sum of d over this lane half's cells of the lane's gene
    int64_t nnz = 0;                                             // non-zero counts of the lane's gene in the range
    uint32_t mk = 0;

    if (ib < ie) {
        stage_load(ib);
        mk = nzmask[(ib >> 5) * m + jc];
        stage_store(0);
    }
    __syncthreads();
    int buf = 0, since_flush = 0, flushes = 0;
    for (int64_t i0 = ib; i0 < ie; i0 += 32) {
        const int64_t in = (i0 + 32 < ie) ? i0 + 32 : i0;        // (the last tile again: unused)
        const uint32_t mkc = mk;
        stage_load(in);
        mk = nzmask[(in >> 5) * m + jc];
        ORIANA_VMEM_FENCE();
        // ---- Lambda = U V^T: k_dropout_sweep's turns with the operands exchanged
        const float *ut = lds + L.ut + buf * KP2 * 32;
        f16v l0;
#pragma unroll
        for (int v = 0; v < 16; ++v) l0[v] = 0.f;
        {
            const float *pa = ut + h * 32 + c, *pb = Vs + h * 32 + c;
            float a[4], b[4], an[4], bn[4];
            int s = 0;
            if (KS >= 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) { a[u] = pa[64 * u]; b[u] = pb[64 * u]; }
                for (; s + 8 <= KS; s += 4) {
                    pa += 256; pb += 256;
#pragma unroll
                    for (int u = 0; u < 4; ++u) { an[u] = pa[64 * u]; bn[u] = pb[64 * u]; }
#pragma unroll
                    for (int u = 0; u < 4; ++u) l0 = mfma32(a[u], b[u], l0);
#pragma unroll
                    for (int u = 0; u < 4; ++u) { a[u] = an[u]; b[u] = bn[u]; }
                }
                pa += 256; pb += 256;
                const int rem = KS - s - 4;
#pragma unroll
                for (int u = 0; u < 3; ++u) { const int o = (u < rem) ? 64 * u : 0; an[u] = pa[o]; bn[u] = pb[o]; }
#pragma unroll
                for (int u = 0; u < 4; ++u) l0 = mfma32(a[u], b[u], l0);
#pragma unroll
                for (int u = 0; u < 3; ++u) if (u < rem) l0 = mfma32(an[u], bn[u], l0);
            } else {
                for (; s < KS; ++s) l0 = mfma32(pa[64 * s], pb[64 * s], l0);
            }
        }
        // ---- sigmoid, overrides: register v of lane half h is cell acc_row(v, h) of the tile
        const int irem = (ie - i0 < 32) ? (int)(ie - i0) : 32;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            if ((v & 3) == 0) __builtin_amdgcn_sched_barrier(0);
            const float x = lg - l0[v];
            float p = __builtin_amdgcn_rcpf(1.0f + __expf(-x));
            if (lg == -INFINITY) p = 1e-10f;                     // pi_d <= 0                         zigap.py:133
            if ((mkc >> acc_row(v, h)) & 1u) p = 1.0f;           // X != 0: f32(1 - 1e-10) == 1       zigap.py:135
            l0[v] = p;
        }
        if (irem < 32) {                                         // (uniform) cells past the batch never reach dsum
#pragma unroll
            for (int v = 0; v < 16; ++v) if (acc_row(v, h) >= irem) l0[v] = 0.f;
        }
        {
            float t = l0[0];
#pragma unroll
            for (int v = 1; v < 16; ++v) t += l0[v];
            bsum += (double)t;
            nnz += __popc(mkc);
        }
        stage_store(buf ^ 1);
        ORIANA_VMEM_FENCE();
        // ---- G += d^T U
        {
            const float *u2 = lds + L.u2 + buf * 32 * L.u2s + c;
            float bc[NT], bn[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bc[nt] = u2[acc_row(0, h) * L.u2s + nt * 32];
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int gn = acc_row(v < 15 ? v + 1 : 15, h);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bn[nt] = u2[gn * L.u2s + nt * 32];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) dv[nt] = mfma32(l0[v], bc[nt], dv[nt]);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bc[nt] = bn[nt];
                __builtin_amdgcn_sched_barrier(0);
            }
            if (++since_flush == 8) {                            // 256 cells: leave the matrix core
                since_flush = 0;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int v = 0; v < 16; ++v) { dvs[nt][v] += dv[nt][v]; dv[nt][v] = 0.f; }
                if (++flushes == 16) { flushes = 0; spill(); }   // 4096 cells: leave float32
            }
        }
        __syncthreads();
        buf ^= 1;
    }
    spill();                                                     // (an empty range writes zeros)
    bsum += __shfl_xor(bsum, 32);                                // the other half of the tile's cells
    if (h == 0 && jok) {
        const double cells = (double)(ie > ib ? ie - ib : 0);
        dp[(int64_t)blockIdx.y * m + jl] = (lg == -INFINITY) ? (double)nnz + 1e-10 * (cells - (double)nnz) : bsum;
    }
}

// G[e] and dsum[j] = the partials of the cell ranges, added in the order of the ranges: every element is written
__global__ void k_gene_rate_combine(double *__restrict__ G, double *__restrict__ dsum, const double *__restrict__ Gp,
                                    const double *__restrict__ dp, int64_t mk, int64_t m, int64_t splits) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= mk + m) return;
    const bool g = e < mk;
    const double *src = g ? Gp + e : dp + (e - mk);
    const int64_t stride = g ? mk : m;
    double s = 0.0;
    for (int64_t sp = 0; sp < splits; ++sp) s += src[sp * stride];
    (g ? G + e : dsum + (e - mk))[0] = s;
}

// Cell ranges of the gene rate, cut as bound_cut cuts gene ranges (the entry runs once per call): until the work-groups fill
// the chip's slots once, in whole tiles (whole mask words), at least two per range, at most GENE_RATE_MAX_RANGES.  Ranges times
// blocks of 128 genes never exceed the slots, so the partials hold at most 128 slots (65,536 on MI355X) rows of K doubles
// whatever n and m (67 MB at K = 128), and never more than 32 times G.
constexpr int64_t GENE_RATE_MAX_RANGES = 32;
struct RateCut { int64_t ips, splits; };
static RateCut gene_rate_cut(int64_t n, int64_t m) {
    const int64_t gb = (m + 127) / 128, slots = 2 * oriana_device_cus();
    int64_t sp = slots / gb;
    if (sp > (n + 63) / 64) sp = (n + 63) / 64;
    if (sp > GENE_RATE_MAX_RANGES) sp = GENE_RATE_MAX_RANGES;
    if (sp < 1) sp = 1;
    int64_t ips = (n + sp - 1) / sp;
    ips = (ips + 31) / 32 * 32;
    return RateCut{ips, (n + ips - 1) / ips};
}

template <int NT>
static int launch_gene_rate(double *Gp, double *dp, const double *U, const double *V, const float *lg, const uint32_t *nzmask,
                            int64_t n, int64_t m, int K, RateCut cut, hipStream_t st) {
    const int KP2 = (K + 1) & ~1;
    const GeneLds L(KP2, NT);
    const size_t lds = (size_t)L.total * sizeof(float);
    const int64_t gb = (m + 127) / 128;
    if (cut.splits > 65535 || gb > 0x7fffffffLL) return ORIANA_EINVAL;
    return launch(k_gene_rate<NT>, dim3((unsigned)gb, (unsigned)cut.splits), dim3(256), lds, st, Gp, dp, U, V, lg, nzmask, n, m, K,
                  KP2, cut.ips);
}

}  // namespace oriana

using namespace oriana;

extern "C" int64_t oriana_zi_gene_rate_ranges(int64_t n, int64_t m, int64_t K) {
    if (n <= 0 || m <= 0 || K <= 0 || K > 128) return 0;
    return gene_rate_cut(n, m).splits;
}

extern "C" int64_t oriana_zi_gene_rate_scratch_doubles(int64_t n, int64_t m, int64_t K) {
    if (n <= 0 || m <= 0 || K <= 0 || K > 128) return 0;
    return gene_rate_cut(n, m).splits * (m * K + m) + bound_logit_doubles(m);     // partials of G | of dsum | the logits
}

extern "C" int oriana_zi_gene_rate(double *G, double *dsum, const double *U, const double *V, const double *pi_d,
                                   const uint32_t *nzmask, double *scratch, int64_t n, int64_t m, int64_t K, void *stream) {
    if (n < 0 || m < 0 || K <= 0) return ORIANA_EINVAL;
    if (K > 128) return ORIANA_EKRANGE;
    if (m == 0) return 0;
    if (!G || !dsum) return ORIANA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {                                                    // no cells: the empty sums, written
        if (hipMemsetAsync(G, 0, (size_t)(m * K) * sizeof(double), st) != hipSuccess) return -1000 - (int)hipGetLastError();
        if (hipMemsetAsync(dsum, 0, (size_t)m * sizeof(double), st) != hipSuccess) return -1000 - (int)hipGetLastError();
        return 0;
    }
    if (!U || !V || !pi_d || !nzmask || !scratch) return ORIANA_EINVAL;
    const RateCut cut = gene_rate_cut(n, m);
    double *Gp = scratch, *dp = scratch + cut.splits * m * K;
    float *lg = reinterpret_cast<float *>(dp + cut.splits * m);
    hipLaunchKernelGGL(k_logit_f32, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, lg, nullptr, nullptr, pi_d, m);
    const int rc = with_variant<1, 2, 3, 4>((int)((oriana_kpad(K) + 31) / 32), [&](auto nt) {
        return launch_gene_rate<decltype(nt)::value>(Gp, dp, U, V, lg, nzmask, n, m, (int)K, cut, st);
    });
    if (rc) return rc;
    const int64_t tot = m * K + m;
    hipLaunchKernelGGL(k_gene_rate_combine, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, G, dsum, Gp, dp, m * K, m,
                       cut.splits);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t oriana_zi_cell_bound_scratch_doubles(int64_t n, int64_t m, int64_t K) {
    if (n <= 0 || m <= 0 || K <= 0 || K > 128) return 0;
    return bound_cut(n, m).splits * n + bound_logit_doubles(m);       // the ranges' partials [splits][n] | the clamped logits
}

extern "C" int oriana_zi_cell_bound(double *out, const double *U, const double *V, const double *pi_d, const uint32_t *nzmask,
                                    double *scratch, int64_t n, int64_t m, int64_t m_real, int64_t K, void *stream) {
    if (n < 0 || m < 0 || m_real < 0 || m_real > m || K <= 0) return ORIANA_EINVAL;
    if (K > 128) return ORIANA_EKRANGE;
    if (n == 0) return 0;
    if (!out) return ORIANA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (m == 0) {                                                    // no genes: the empty sum, written
        if (hipMemsetAsync(out, 0, (size_t)n * sizeof(double), st) != hipSuccess) return -1000 - (int)hipGetLastError();
        return 0;
    }
    if (!U || !V || !pi_d || !nzmask || !scratch) return ORIANA_EINVAL;
    const BoundCut cut = bound_cut(n, m);
    double *partial = scratch;
    float *lg = reinterpret_cast<float *>(scratch + cut.splits * n);
    hipLaunchKernelGGL(k_logit_clamped_f32, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, lg, pi_d, m, m_real);
    const int rc = with_variant<1, 2, 3, 4>((int)((oriana_kpad(K) + 31) / 32), [&](auto nt) {
        return launch_bound<decltype(nt)::value>(partial, U, V, lg, nzmask, n, m, (int)K, cut, st);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_cell_bound_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out, partial, n, cut.splits);
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t oriana_dropout_sweep_scratch_floats(int64_t m, int64_t K) {
    if (m < 0 || K < 0) return 0;
    // logit(pi_d) + the two operand images of the b16 family at their largest (4 k chunks, 2 n tiles), or those of the tiles family
    const int64_t a = b16_img_floats(m, 4 * 3 * 64) + b16_img_floats(m, 2 * 2 * 3 * 64);
    const int64_t b = dn::zi_may_use_tiles(oriana_kpad(K)) ? dn::zi_sweep_image_floats(m) : 0;
    return 3 * ((m + 63) / 64 * 64) + (a > b ? a : b);       // logits, scaled logits + floors (dense_zi.hip), images
}

extern "C" int64_t oriana_nzmask_tiles_words(int64_t n, int64_t m) {
    if (n < 0 || m < 0) return 0;
    return dn::zi_tiles_words(n, m);
}

extern "C" int oriana_nzmask_tiles(uint32_t *tiles, const uint32_t *nzmask, int64_t n, int64_t m, void *stream) {
    if (n < 0 || m < 0) return ORIANA_EINVAL;
    if (n == 0 || m == 0) return 0;
    if (!tiles || !nzmask || ((uintptr_t)tiles & 15) != 0) return ORIANA_EINVAL;
    const int rc = dn::zi_tiles(tiles, nzmask, n, m, (hipStream_t)stream);
    if (rc) return rc;
    ORIANA_LAUNCH_CHECK();
    return 0;
}

extern "C" int oriana_dropout_sweep_fused_tiles(float *D_hat, const double *U, const double *V, const double *pi_d64,
                                                const uint32_t *nzmask, const uint32_t *nztiles, double *colsum,
                                                const double *V_next, double *DV_next, float *scratch, int arithmetic,
                                                int64_t n, int64_t m, int64_t K, void *stream) {
    if (n < 0 || m < 0 || K <= 0) return ORIANA_EINVAL;
    if (K > 128) return ORIANA_EKRANGE;
    if (n == 0 || m == 0) return 0;
    if (!D_hat || !U || !V || !pi_d64 || !scratch || ((V_next == nullptr) != (DV_next == nullptr))) return ORIANA_EINVAL;
    if (((uintptr_t)scratch & 15) != 0) return ORIANA_EINVAL;
    if (arithmetic != ORIANA_MATRIX_F32 && arithmetic != ORIANA_MATRIX_BF16X3) return ORIANA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int64_t mpad = (m + 63) / 64 * 64;
    // scratch: logits | scaled logits | floors (tiles) | operand images
    const float *pi_d = scratch, *lgs = scratch + mpad;
    float *img = scratch + 3 * mpad;
    hipLaunchKernelGGL(k_logit_f32, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, scratch, scratch + mpad, scratch + 2 * mpad,
                       pi_d64, m);
    return with_variant<ORIANA_MATRIX_F32, ORIANA_MATRIX_BF16X3>(arithmetic, [&](auto A) {
        return dn::with_cfg<1, dn::ZI_KP_MAX / 16>(dn::kc_tail(oriana_kpad(K)), [&](auto c) {
            return dn::zi_first<dn::ZiOp::update, decltype(c)::KP, decltype(A)::value>(
                [&](dn::ZiFam f) { return dn::zi_update_ok(f, D_hat, lgs, nztiles, V_next, DV_next, m); },
                [&](auto p) {
                    using P = decltype(p);
                    if constexpr (P::fam == dn::ZiFam::tiles)
                        return dn::zi_sweep({P::a, P::b}, D_hat, U, V, lgs, mpad, nztiles, colsum, V_next, DV_next, img, n, m, (int)K, st);
                    else if constexpr (P::fam == dn::ZiFam::b16)
                        return launch_sweep_b16<P::a, P::b>(D_hat, U, V, pi_d, nzmask, colsum, V_next, DV_next, img, n, m, (int)K, st);
                    else
                        return launch_sweep<P::a>(D_hat, U, V, pi_d, nzmask, colsum, V_next, DV_next, n, m, (int)K, st);
                });
        });
    });
}

// The cell-side rate of a ZI FOLD-IN (models/zigap.py fold_in): DV[i, :] += sum_j d_ij V[j, :] with d the float32 dropout
// posterior of the D update above, formed from (U, V, pi_d) tile by tile and never stored -- the same rule (zi_candidate,
// ZiOp::update), the same preconditions (zi_update_ok with no D_hat pointer) and the same kernels with RATE = true.
extern "C" int oriana_zi_foldin_rate(double *DV, const double *U, const double *V, const double *pi_d64, const uint32_t *nzmask,
                                     const uint32_t *nztiles, const uint8_t *active, float *scratch, int arithmetic, int64_t n,
                                     int64_t m, int64_t K, void *stream) {
    if (n < 0 || m < 0 || K <= 0) return ORIANA_EINVAL;
    if (K > 128) return ORIANA_EKRANGE;
    if (n == 0 || m == 0) return 0;
    if (!DV || !U || !V || !pi_d64 || !nzmask || !scratch) return ORIANA_EINVAL;
    if (((uintptr_t)scratch & 15) != 0) return ORIANA_EINVAL;
    if (arithmetic != ORIANA_MATRIX_F32 && arithmetic != ORIANA_MATRIX_BF16X3) return ORIANA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int64_t mpad = (m + 63) / 64 * 64;
    const float *pi_d = scratch, *lgs = scratch + mpad;
    float *img = scratch + 3 * mpad;
    hipLaunchKernelGGL(k_logit_f32, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, scratch, scratch + mpad, scratch + 2 * mpad,
                       pi_d64, m);
    return with_variant<ORIANA_MATRIX_F32, ORIANA_MATRIX_BF16X3>(arithmetic, [&](auto A) {
        return dn::with_cfg<1, dn::ZI_KP_MAX / 16>(dn::kc_tail(oriana_kpad(K)), [&](auto c) {
            return dn::zi_first<dn::ZiOp::update, decltype(c)::KP, decltype(A)::value>(
                [&](dn::ZiFam f) { return dn::zi_update_ok(f, nullptr, lgs, nztiles, V, DV, m); },
                [&](auto p) {
                    using P = decltype(p);
                    if constexpr (P::fam == dn::ZiFam::tiles)
                        return dn::zi_rate({P::a, P::b}, U, V, lgs, mpad, nztiles, DV, active, img, n, m, (int)K, st);
                    else if constexpr (P::fam == dn::ZiFam::b16)
                        return launch_sweep_b16<P::a, P::b, true>(nullptr, U, V, pi_d, nzmask, nullptr, V, DV, img, n, m, (int)K, st, active);
                    else
                        return launch_sweep<P::a, true>(nullptr, U, V, pi_d, nzmask, nullptr, V, DV, n, m, (int)K, st, active);
                });
        });
    });
}

// Which kernel the entries above (op 0: the D update and its rate-only twin) and oriana_dense_t_times_factor_f32 (op 1) launch
// for K under `arithmetic`, asked through the chain they dispatch with -- with_variant, with_cfg, zi_first over zi_candidate --
// so the answer cannot drift from the launch: (family << 16) | (a << 8) | b of the ZiPick that would run.  tiles_ok stands for
// the run-time preconditions of the tiles family (zi_update_ok / zi_dt_ok); the other families have none.  Host only: nothing
// is launched, no device is touched.
template <dn::ZiOp OP>
static int zi_dispatch(int64_t K, int arithmetic, int tiles_ok) {
    return with_variant<ORIANA_MATRIX_F32, ORIANA_MATRIX_BF16X3>(arithmetic, [&](auto A) {
        return dn::with_cfg<1, dn::ZI_KP_MAX / 16>(dn::kc_tail(oriana_kpad(K)), [&](auto c) {
            return dn::zi_first<OP, decltype(c)::KP, decltype(A)::value>(
                [&](dn::ZiFam f) { return f != dn::ZiFam::tiles || tiles_ok != 0; },
                [&](auto p) {
                    using P = decltype(p);
                    return ((int)P::fam << 16) | (P::a << 8) | P::b;
                });
        });
    });
}

extern "C" int oriana_zi_dispatch(int op, int64_t K, int arithmetic, int tiles_ok) {
    if (K <= 0 || (op != 0 && op != 1)) return ORIANA_EINVAL;
    if (K > 128) return ORIANA_EKRANGE;
    if (arithmetic != ORIANA_MATRIX_F32 && arithmetic != ORIANA_MATRIX_BF16X3) return ORIANA_EINVAL;
    return op == 0 ? zi_dispatch<dn::ZiOp::update>(K, arithmetic, tiles_ok) : zi_dispatch<dn::ZiOp::dt>(K, arithmetic, tiles_ok);
}

// the round-2 entry: without the per-lane flags (oriana_nzmask_tiles) the tiles family does not apply (dn::zi_update_ok)
extern "C" int oriana_dropout_sweep_fused(float *D_hat, const double *U, const double *V, const double *pi_d64,
                                          const uint32_t *nzmask, double *colsum, const double *V_next, double *DV_next,
                                          float *scratch, int arithmetic, int64_t n, int64_t m, int64_t K, void *stream) {
    return oriana_dropout_sweep_fused_tiles(D_hat, U, V, pi_d64, nzmask, nullptr, colsum, V_next, DV_next, scratch, arithmetic, n, m,
                                            K, stream);
}

// (One size for every kernel family: the images of the b16 family at NT = 2 plus four chunks, or those of the tiles family at its
//  largest configuration.  The images a call writes end before it -- a guard band behind a scratch of this size does not see an
//  overrun of less than that spare room.)
extern "C" int64_t oriana_dense_t_scratch_floats(int64_t n, int64_t K) {
    if (n < 0 || K < 0) return 0;
    const int64_t a = ((n + 15) / 16 + 4) * (int64_t)(2 * 3 * 64) * 4;       // operand images of W at the b16 family's largest
    const int64_t b = dn::zi_may_use_tiles(oriana_kpad(K)) ? dn::zi_dt_image_floats(n) : 0;
    return a > b ? a : b;
}

extern "C" int oriana_dense_t_times_factor_f32(double *out, const float *D, const double *W, float *scratch, int arithmetic,
                                               int64_t n, int64_t m, int64_t K, void *stream) {
    if (n < 0 || m < 0 || K <= 0) return ORIANA_EINVAL;
    if (K > 128) return ORIANA_EKRANGE;
    if (n == 0 || m == 0) return 0;
    if (!out || !D || !W) return ORIANA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    return with_variant<ORIANA_MATRIX_F32, ORIANA_MATRIX_BF16X3>(arithmetic, [&](auto A) {
        return dn::with_cfg<1, dn::ZI_KP_MAX / 16>(dn::kc_tail(oriana_kpad(K)), [&](auto c) {
            return dn::zi_first<dn::ZiOp::dt, decltype(c)::KP, decltype(A)::value>(
                [&](dn::ZiFam f) { return dn::zi_dt_ok(f, D, scratch, m); },
                [&](auto p) {
                    using P = decltype(p);
                    if constexpr (P::fam == dn::ZiFam::tiles) return dn::zi_dt({P::a, P::b}, out, D, W, scratch, n, m, (int)K, st);
                    else if constexpr (P::fam == dn::ZiFam::b16) return launch_dt_b16<P::a>(out, D, W, scratch, n, m, (int)K, st);
                    else return launch_dt<P::a, P::b>(out, D, W, n, m, (int)K, st);
                });
        });
    });
}
