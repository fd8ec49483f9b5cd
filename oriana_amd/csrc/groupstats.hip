// groupstats.hip -- sums over the stored (non-zero) counts kept per cell and per (cluster, gene): what a marker-gene test of a
// cell clustering needs from X (oriana_amd/models/base.py: cell_totals, cluster_gene_stats, marker_genes; no counterpart in the
// reference).  log1p(0) = 0: the zeros of X contribute nothing to the moments of the log-normalised counts, so everything here
// is one walk over the two layouts the model already holds, shaped like k_count_stats / k_dn_metric with a cluster axis added.
// Counts are read as the layouts hold them (rowrec.x float32, the dense block's uint16); every sum is float64.
#include "common.h"
#include "counts_check.h"
#include "dense_tiles.h"

namespace oriana {

constexpr int GS_CC = 24;              // most clusters per work-group, sliced layout: [GS_CC][256 genes] x 20 bytes = 120 KiB of LDS
constexpr int GS_GROUPS = 4;           // groups of 256 threads per work-group of the sliced kernel, one row block each at a time
constexpr int GS_ITERS = 4;            // row blocks a group walks: GS_GROUPS * GS_ITERS row blocks of a gene tile per flush
constexpr int GS_DCC = 32;             // clusters per work-group, dense block: [GS_DCC][32 genes] x 20 bytes = 20 KiB
constexpr int GS_MAX_GROUPS = 1024;    // oriana_group_stats_max_groups()
constexpr int GS_CTG = 32;             // cell tiles (32 cells) of one gene tile a work-group of the dense kernel walks
constexpr int CT_GTS = 64;             // gene tiles a work-group of the dense totals kernel adds up in registers

// totals[cell] += sum_j x over the stored entries of one tile (caller's row order).  One work-group per tile, as k_count_stats;
// a thread striding by 256 stays with one row per slice (slice lengths are multiples of 64), adds its entries in a register,
// the 4 lanes of the row are combined by a butterfly and one lane adds the (wave, slice) sum into the LDS row table: one global
// float64 atomic per touched (tile, row) leaves the work-group.
__global__ __launch_bounds__(256) void k_cell_totals(oriana_counts cm, double *__restrict__ totals) {
    __shared__ double rs[TILE];
    __shared__ int rn[TILE];
    const int tid = threadIdx.x, rl = (tid & 63) >> 2;
    const int64_t t = blockIdx.x;
    const int64_t rb = t / cm.ncb;
    const int64_t rbase = cm.roff[t];
    rs[tid] = 0.0;
    rn[tid] = 0;
    __syncthreads();
    for (int sl = 0; sl < 16; ++sl) {
        const uint32_t s0 = cm.rslice[t * 17 + sl], s1 = cm.rslice[t * 17 + sl + 1];
        if (s0 == s1) continue;                                  // (uniform over the work-group)
        double a = 0.0;
        int cnt = 0;
        for (uint32_t slot = s0 + tid; slot < s1; slot += 256) {
            const float x = cm.rowrec[rbase + slot].x;
            if (x == 0.f) continue;
            a += (double)x;
            cnt = 1;
        }
        // (a slice's length is a multiple of 64: the lanes of a wave leave the loop together)
        a += __shfl_xor(a, 1, 64); a += __shfl_xor(a, 2, 64);
        cnt |= __shfl_xor(cnt, 1, 64); cnt |= __shfl_xor(cnt, 2, 64);
        if ((tid & 3) == 0 && cnt) {
            atomicAdd(&rs[sl * 16 + rl], a);
            rn[sl * 16 + rl] = 1;
        }
    }
    __syncthreads();
    const int64_t ip = rb * TILE + tid;
    if (rn[tid] && ip < cm.n) {
        const int64_t i = cm.row_perm ? (int64_t)cm.row_perm[ip] : ip;
        atomicAdd(&totals[i], rs[tid]);
    }
}

// The dense block's share: one work-group per (cell tile, range of CT_GTS gene tiles).  A thread reads the four counts
// 4 tid .. 4 tid + 3 of each 32 x 32 block with one 8-byte load; they belong to ONE cell (entry e = ((v / 8) * 64 + l) * 8 + v % 8,
// lane l = (cell c, half h): c = (tid / 2) % 32), so the thread adds them in an integer register over its gene tiles (at most
// 4 * 64 counts below 2^16), the 8 threads of a cell meet in LDS and one global float64 atomic per cell leaves the work-group.
__global__ __launch_bounds__(256) void k_dn_cell_totals(const uint16_t *__restrict__ Xd, const int32_t *__restrict__ row_perm,
                                                        double *__restrict__ totals, int64_t n, int ngt, int nsplit) {
    __shared__ unsigned int rs[32];
    const int tid = threadIdx.x, c = (tid >> 1) & 31;
    const int64_t ct = blockIdx.x / nsplit;
    const int g0 = (int)(blockIdx.x % nsplit) * CT_GTS, g1 = min(ngt, g0 + CT_GTS);
    if (tid < 32) rs[tid] = 0u;
    __syncthreads();
    unsigned int a = 0u;
    for (int gt = g0; gt < g1; ++gt) {
        const uint2 w = *reinterpret_cast<const uint2 *>(Xd + (ct * ngt + gt) * 1024 + 4 * tid);
        a += (w.x & 0xFFFFu) + (w.x >> 16) + (w.y & 0xFFFFu) + (w.y >> 16);
    }
    if (a != 0u) atomicAdd(&rs[c], a);
    __syncthreads();
    const int64_t ip = ct * 32 + tid;
    if (tid < 32 && ip < n && rs[tid] != 0u) {
        const int64_t i = row_perm ? (int64_t)row_perm[ip] : ip;
        atomicAdd(&totals[i], (double)rs[tid]);
    }
}

// One stored count x of a cell with scale s: the value whose moments are kept.
__device__ __forceinline__ double gs_value(double x, const double *scale, double s, int lg) {
    double y = scale ? x * s : x;
    if (lg) y = log1p(y);
    return y;
}

// out (3, C, mtot), caller's gene order: per stored entry of cell i (cluster c = labels[i]) and gene j, with y = gs_value:
// out[0, c, j] += 1, out[1, c, j] += y, out[2, c, j] += y^2.  One work-group of GS_GROUPS x 256 threads per (gene tile, run of
// GS_GROUPS * iters consecutive row blocks, chunk of cc <= GS_CC clusters); the chunk is the fastest index of the grid, so the
// work-groups that re-read a tile for the other chunks run next to each other.  The groups walk different row blocks of the gene
// tile at the same time (group g takes the row blocks g, g + 4, .. of the run, each as k_count_stats walks a tile) and share ONE
// table [cc][256 genes] of {int count, double sum y, double sum y^2} in LDS, fed by LDS atomics as k_count_stats feeds cs / cn:
// 1024 threads keep the CU busy under a table that leaves room for one work-group only once cc passes 13, and a flush serves
// GS_GROUPS * iters row blocks.  Per row block a group stages its 256 labels (relative to the chunk; -1 = not of this chunk) and
// scales in LDS; an entry of another chunk costs its record load and nothing else.  At the end one global float64 atomic per term
// and touched (cluster, gene) goes out through col_perm.  Labels outside [0, C) are never counted: no address depends on their
// value.  Dynamic LDS: cc * 5120 + 12288 bytes.
__global__ __launch_bounds__(256 * GS_GROUPS) void k_group_stats(oriana_counts cm, const int32_t *__restrict__ labels,
                                                                 const double *__restrict__ scale, int lg, int C, int64_t mtot,
                                                                 int64_t joff, int iters, int nchunk, int cc,
                                                                 double *__restrict__ out) {
    extern __shared__ double gs_lds[];
    double *t1 = gs_lds, *t2 = t1 + cc * TILE, *sc = t2 + cc * TILE;                   // [cc][256], [cc][256], [GS_GROUPS][256]
    int *tc = reinterpret_cast<int *>(sc + GS_GROUPS * TILE), *lab = tc + cc * TILE;   // [cc][256], [GS_GROUPS][256]
    const int grp = threadIdx.x >> 8, tid = threadIdx.x & 255, rl = (tid & 63) >> 2;
    const int chunk = (int)(blockIdx.x % (unsigned)nchunk);
    const int64_t rest = blockIdx.x / (unsigned)nchunk;
    const int64_t cb = rest % cm.ncb, rg = rest / cm.ncb;
    const int c0 = chunk * cc, cw = min(cc, C - c0);
    for (int e = threadIdx.x; e < cw * TILE; e += 256 * GS_GROUPS) { t1[e] = 0.0; t2[e] = 0.0; tc[e] = 0; }
    for (int it = 0; it < iters; ++it) {                         // (uniform over the work-group: every thread meets every barrier)
        const int64_t rb = (rg * iters + it) * GS_GROUPS + grp;
        __syncthreads();                                         // (the table is zero; the last row block's labels are done with)
        {
            const int64_t ip = rb * TILE + tid;
            int l = -1;
            double s = 1.0;
            if (rb < cm.nrb && ip < cm.n) {
                const int64_t i = cm.row_perm ? (int64_t)cm.row_perm[ip] : ip;
                l = labels[i] - c0;
                if ((unsigned)l >= (unsigned)cw) l = -1;
                if (scale) s = scale[i];
            }
            lab[grp * TILE + tid] = l;
            sc[grp * TILE + tid] = s;
        }
        __syncthreads();
        if (rb >= cm.nrb) continue;                              // (a group past the last row block; it still meets the barriers)
        const int64_t t = rb * cm.ncb + cb;
        const int64_t rbase = cm.roff[t];
        for (int sl = 0; sl < 16; ++sl) {
            const uint32_t s0 = cm.rslice[t * 17 + sl], s1 = cm.rslice[t * 17 + sl + 1];
            const int r = grp * TILE + sl * 16 + rl;             // (one row per thread and slice: slice lengths are multiples of 64)
            const int l = lab[r];
            if (l < 0) continue;
            const double s = sc[r];
            for (uint32_t slot = s0 + tid; slot < s1; slot += 256) {
                const oriana_rowrec rec = cm.rowrec[rbase + slot];
                if (rec.x == 0.f) continue;
                const double y = gs_value((double)rec.x, scale, s, lg);
                const int e = l * TILE + rec.col;
                atomicAdd(&tc[e], 1);
                atomicAdd(&t1[e], y);
                atomicAdd(&t2[e], y * y);
            }
        }
    }
    __syncthreads();
    const int64_t jp = cb * TILE + tid;
    if (jp >= cm.m) return;
    const int64_t j = cm.col_perm ? (int64_t)cm.col_perm[jp] : jp + joff;
    for (int c = grp; c < cw; c += GS_GROUPS) {
        const int e = c * TILE + tid;
        if (tc[e] == 0) continue;
        double *o = out + (int64_t)(c0 + c) * mtot + j;
        atomicAdd(o, (double)tc[e]);
        atomicAdd(o + (int64_t)C * mtot, t1[e]);
        atomicAdd(o + 2 * (int64_t)C * mtot, t2[e]);
    }
}

// The dense twin: one work-group per (gene tile, group of `ctg` consecutive cell tiles, chunk of GS_DCC clusters), walking the
// 32 x 32 blocks as k_dn_metric does.  A thread holds the four counts 4 tid .. 4 tid + 3 of a block (one 8-byte load): one cell
// c = (tid / 2) % 32, whose label and scale it reads itself, and the genes acc_row(v, h), v = 8 (tid / 128) + 4 (tid % 2) + q,
// h = (tid / 64) % 2.  The lanes of a wave start at different q, so that the LDS atomics of one instruction spread over 8 genes
// of each cluster instead of 2.  The table [GS_DCC][32 genes] is zeroed and flushed once per work-group: 3 * 32 * C' values
// (C' the clusters of the chunk that occur) against ctg * 1024 entries walked.
__global__ __launch_bounds__(256) void k_dn_group_stats(const uint16_t *__restrict__ Xd, const int32_t *__restrict__ row_perm,
                                                        const int32_t *__restrict__ col_perm, const int32_t *__restrict__ labels,
                                                        const double *__restrict__ scale, int lg, int C, int64_t mtot, int64_t n,
                                                        int ngt, int ctg, int nchunk, double *__restrict__ out) {
    __shared__ double t1[GS_DCC * 32], t2[GS_DCC * 32];
    __shared__ int tc[GS_DCC * 32];
    const int tid = threadIdx.x;
    const int chunk = (int)(blockIdx.x % (unsigned)nchunk);
    const int64_t rest = blockIdx.x / (unsigned)nchunk;
    const int gt = (int)(rest % ngt);
    const int64_t cg = rest / ngt;
    const int c0 = chunk * GS_DCC, cw = min(GS_DCC, C - c0);
    for (int e = tid; e < cw * 32; e += 256) { t1[e] = 0.0; t2[e] = 0.0; tc[e] = 0; }
    __syncthreads();
    const int c = (tid >> 1) & 31, h = (tid >> 6) & 1;
    const int gbase = dn::acc_row(8 * (tid >> 7) + 4 * (tid & 1), h);      // gene of q = 0; q adds to it (acc_row: v % 4)
    const int64_t nct = (n + 31) / 32;
    const int64_t ct_end = min(nct, (cg + 1) * (int64_t)ctg);
    for (int64_t ct = cg * ctg; ct < ct_end; ++ct) {
        const int64_t ip = ct * 32 + c;
        if (ip >= n) continue;
        const int64_t i = row_perm ? (int64_t)row_perm[ip] : ip;
        const int l = labels[i] - c0;
        if ((unsigned)l >= (unsigned)cw) continue;
        const double s = scale ? scale[i] : 1.0;
        const uint2 w = *reinterpret_cast<const uint2 *>(Xd + (ct * ngt + gt) * 1024 + 4 * tid);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int q = (qq + (tid >> 1)) & 3;
            const uint32_t xi = ((q & 2 ? w.y : w.x) >> (16 * (q & 1))) & 0xFFFFu;
            if (xi == 0u) continue;
            const double y = gs_value((double)xi, scale, s, lg);
            const int e = l * 32 + gbase + q;
            atomicAdd(&tc[e], 1);
            atomicAdd(&t1[e], y);
            atomicAdd(&t2[e], y * y);
        }
    }
    __syncthreads();
    for (int e = tid; e < cw * 32; e += 256) {
        if (tc[e] == 0) continue;
        const int64_t jp = (int64_t)gt * 32 + (e & 31);
        const int64_t j = col_perm ? (int64_t)col_perm[jp] : jp;
        double *o = out + (int64_t)(c0 + (e >> 5)) * mtot + j;
        atomicAdd(o, (double)tc[e]);
        atomicAdd(o + (int64_t)C * mtot, t1[e]);
        atomicAdd(o + 2 * (int64_t)C * mtot, t2[e]);
    }
}

// ---- gene-set scores: out (n, S) = Y W, Y the transformed counts, W (m_all, S) float64 (oriana_gene_scores) ---------
// The transpose of k_group_stats: the sums run over the genes of a cell, so a cell's sums have one owner and nothing here is an
// atomic.  The order of every sum is a function of the layouts and S alone.

// The sliced layout: one work-group of 256 threads per (row block, chunk of CH sets; the chunk is the fastest index of the grid),
// walking the ncb column tiles of the row block in order.  Per tile the 256 rows of W of the tile's genes are staged in LDS
// through col_perm for the chunk (zeros past m and past S).  Wave w owns the slices w, w + 4, w + 8, w + 12 of every tile and
// walks each of them 64 slots at a time (slot = iteration * 64 + row_in_slice * 4 + u: the lane's row is the same in every
// iteration), so a lane stays with FOUR rows of the row block for the whole walk and keeps their 4 x CH accumulators in
// registers across all tiles (acc_s = fma(W[j, s], y, acc_s)): a row has one wave, its four lanes meet by the butterfly ONCE, at
// the end, and there is no table, no partial sum and no barrier between the waves beyond the two per tile around the staging of W.
// The sums then pass through LDS (the buffer of W) so that thread r WRITES the row r, out[i, s0 .. s0 + cw), through row_perm.
// walk = 0 (a layout without a stored count): zeros are written.  Static LDS: 256 * CH * 8 bytes.
template <int CH>
__global__ __launch_bounds__(256) void k_gene_scores(oriana_counts cm, const double *__restrict__ scale, int lg,
                                                     const double *__restrict__ W, int64_t S, int64_t joff, int nchunk, int walk,
                                                     double *__restrict__ out) {
    __shared__ __align__(16) double wl[TILE * CH];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), rl = (tid & 63) >> 2, u = tid & 3;
    const int chunk = (int)(blockIdx.x % (unsigned)nchunk);
    const int64_t rb = blockIdx.x / (unsigned)nchunk;
    const int64_t s0c = (int64_t)chunk * CH;
    const int cw = (int)min((int64_t)CH, S - s0c);
    double sc[4], acc[4][CH];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t ip = rb * TILE + (4 * q + wave) * 16 + rl;
        sc[q] = 1.0;
        if (scale && ip < cm.n) sc[q] = scale[cm.row_perm ? (int64_t)cm.row_perm[ip] : ip];
#pragma unroll
        for (int s = 0; s < CH; ++s) acc[q][s] = 0.0;
    }
    const int64_t ncb = walk ? cm.ncb : 0;
    for (int64_t cb = 0; cb < ncb; ++cb) {
        __syncthreads();                                         // (the last tile's rows of W are done with)
        {
            const int64_t jp = cb * TILE + tid;
            const double *w = nullptr;
            if (jp < cm.m) w = W + (cm.col_perm ? (int64_t)cm.col_perm[jp] : jp + joff) * S + s0c;
#pragma unroll
            for (int s = 0; s < CH; ++s) wl[tid * CH + s] = (w && s < cw) ? w[s] : 0.0;
        }
        __syncthreads();
        const int64_t t = rb * cm.ncb + cb;
        const int64_t rbase = cm.roff[t];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int sl = 4 * q + wave;
            const uint32_t s0 = cm.rslice[t * 17 + sl], s1 = cm.rslice[t * 17 + sl + 1];
            // (a slice's length is a multiple of 64: the lanes of the wave leave the loop together)
            for (uint32_t slot = s0 + (tid & 63); slot < s1; slot += 64) {
                const oriana_rowrec rec = cm.rowrec[rbase + slot];
                if (rec.x == 0.f) continue;
                const double y = gs_value((double)rec.x, scale, sc[q], lg);
                const double *w = wl + (int)rec.col * CH;
#pragma unroll
                for (int s = 0; s < CH; ++s) acc[q][s] = fma(w[s], y, acc[q][s]);
            }
        }
    }
    __syncthreads();                                             // (W is done with: its buffer takes the sums)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int s = 0; s < CH; ++s) {
            double a = acc[q][s];
            a += __shfl_xor(a, 1, 64);
            a += __shfl_xor(a, 2, 64);
            if (u == 0) wl[((4 * q + wave) * 16 + rl) * CH + s] = a;
        }
    }
    __syncthreads();
    const int64_t ip = rb * TILE + tid;
    if (ip >= cm.n) return;
    const int64_t i = cm.row_perm ? (int64_t)cm.row_perm[ip] : ip;
    for (int s = 0; s < cw; ++s) out[i * S + s0c + s] = wl[tid * CH + s];
}

// The dense block: one work-group per (cell tile of 32 cells, chunk of CH sets), walking ALL gene tiles in order.  A thread holds
// the four counts 4 tid .. 4 tid + 3 of a block as k_dn_cell_totals does -- one cell c = (tid / 2) % 32, the genes gbase + q of
// k_dn_group_stats -- and keeps the chunk's accumulators in registers over the whole walk; the tile's 32 rows of W are staged in
// LDS through col_perm, in two buffers (one barrier per tile).  At the end the 8 threads of a cell (k = tid % 2 + 2 (tid / 64))
// meet in LDS and thread (c, s) adds their sums in the order k = 0 .. 7, then ADDS the result to out[i, s0 + s]: this kernel runs
// second in stream order, after k_gene_scores has written every element, and is the only writer of the element in its launch.
template <int CH>
__global__ __launch_bounds__(256) void k_dn_gene_scores(const uint16_t *__restrict__ Xd, const int32_t *__restrict__ row_perm,
                                                        const int32_t *__restrict__ col_perm, const double *__restrict__ scale,
                                                        int lg, const double *__restrict__ W, int64_t S, int64_t n, int ngt,
                                                        int nchunk, double *__restrict__ out) {
    __shared__ __align__(16) double wl[2][32 * CH];
    __shared__ double part[8 * 32 * CH];
    const int tid = threadIdx.x;
    const int chunk = (int)(blockIdx.x % (unsigned)nchunk);
    const int64_t ct = blockIdx.x / (unsigned)nchunk;
    const int64_t s0c = (int64_t)chunk * CH;
    const int cw = (int)min((int64_t)CH, S - s0c);
    const int c = (tid >> 1) & 31, h = (tid >> 6) & 1, k = (tid & 1) + 2 * (tid >> 6);
    const int gbase = dn::acc_row(8 * (tid >> 7) + 4 * (tid & 1), h);      // gene of q = 0; q adds to it (acc_row: v % 4)
    const int64_t ipc = ct * 32 + c;
    double sv = 1.0;
    if (scale && ipc < n) sv = scale[row_perm ? (int64_t)row_perm[ipc] : ipc];
    double acc[CH];
#pragma unroll
    for (int s = 0; s < CH; ++s) acc[s] = 0.0;
    for (int gt = 0; gt < ngt; ++gt) {
        double *wb = wl[gt & 1];
        for (int e = tid; e < 32 * CH; e += 256) {               // (the buffer was last read two tiles ago: a barrier lies between)
            const int64_t jp = (int64_t)gt * 32 + e / CH;
            const int s = e % CH;
            const int64_t j = col_perm ? (int64_t)col_perm[jp] : jp;
            wb[e] = s < cw ? W[j * S + s0c + s] : 0.0;
        }
        __syncthreads();
        if (ipc >= n) continue;                                  // (a cell past the end; its thread still meets the barriers)
        const uint2 w = *reinterpret_cast<const uint2 *>(Xd + (ct * ngt + gt) * 1024 + 4 * tid);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t xi = ((q & 2 ? w.y : w.x) >> (16 * (q & 1))) & 0xFFFFu;
            if (xi == 0u) continue;
            const double y = gs_value((double)xi, scale, sv, lg);
            const double *wr = wb + (gbase + q) * CH;
#pragma unroll
            for (int s = 0; s < CH; ++s) acc[s] = fma(wr[s], y, acc[s]);
        }
    }
#pragma unroll
    for (int s = 0; s < CH; ++s) part[(k * 32 + c) * CH + s] = acc[s];
    __syncthreads();
    for (int e = tid; e < 32 * CH; e += 256) {
        const int64_t ip = ct * 32 + e / CH;
        const int s = e % CH;
        if (ip >= n || s >= cw) continue;
        double a = part[e];
#pragma unroll
        for (int kk = 1; kk < 8; ++kk) a += part[kk * 32 * CH + e];
        const int64_t i = row_perm ? (int64_t)row_perm[ip] : ip;
        out[i * S + s0c + s] += a;
    }
}

constexpr int GSC_CH = 8;              // oriana_gene_scores_set_chunk(): sets one work-group carries (4 x CH accumulators per lane: 182 VGPRs at 16)
constexpr int GSC_MAX_SETS = 1024;     // oriana_gene_scores_max_sets()

}  // namespace oriana

using namespace oriana;

extern "C" int64_t oriana_gene_scores_max_sets(void) { return GSC_MAX_SETS; }
extern "C" int64_t oriana_gene_scores_set_chunk(void) { return GSC_CH; }

extern "C" int oriana_gene_scores(const oriana_counts *cm, const oriana_dense *dn, const int32_t *row_perm,
                                  const int32_t *col_perm, const double *scale, int log1p_flag, const double *W, int64_t S,
                                  double *out, void *stream) {
    if (!cm || !W || !out || S < 1) return ORIANA_EINVAL;
    if (const int rc = gs_check_layouts(cm, dn)) return rc;
    if (S > GSC_MAX_SETS) return ORIANA_EKRANGE;
    const int64_t gd = dn ? dn->gd : 0, nchunk = (S + GSC_CH - 1) / GSC_CH;
    const int64_t nrb = (cm->n + TILE - 1) / TILE;
    const int64_t ngt = gd / 32, nct = dn && dn->n > 0 ? (dn->n + 31) / 32 : 0;
    const int64_t nwg = nrb * nchunk, ndwg = ngt > 0 ? nct * nchunk : 0;
    if (nwg > 0x7fffffffLL || ndwg > 0x7fffffffLL || ngt > 0x7fffffffLL) return ORIANA_EINVAL;
    const int walk = cm->nrb == nrb && cm->ncb > 0 && cm->rslots > 0;
    if (nwg > 0) {
        hipLaunchKernelGGL(k_gene_scores<GSC_CH>, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, *cm, scale,
                           log1p_flag ? 1 : 0, W, S, gd, (int)nchunk, walk, out);
        ORIANA_LAUNCH_CHECK();
    }
    if (ndwg > 0) {
        hipLaunchKernelGGL(k_dn_gene_scores<GSC_CH>, dim3((unsigned)ndwg), dim3(256), 0, (hipStream_t)stream, dn->x, row_perm,
                           col_perm, scale, log1p_flag ? 1 : 0, W, S, dn->n, (int)ngt, (int)nchunk, out);
        ORIANA_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int64_t oriana_group_stats_max_groups(void) { return GS_MAX_GROUPS; }

extern "C" int oriana_cell_totals(const oriana_counts *cm, const oriana_dense *dn, const int32_t *row_perm,
                                  const int32_t *col_perm, double *totals, void *stream) {
    (void)col_perm;                                              // (a cell's total does not depend on the gene order)
    if (!totals) return ORIANA_EINVAL;
    if (const int rc = gs_check_layouts(cm, dn)) return rc;
    const int64_t nt = cm->nrb * cm->ncb;
    if (nt > 0x7fffffffLL) return ORIANA_EINVAL;
    const int64_t ngt = dn ? dn->gd / 32 : 0, nct = dn ? (dn->n + 31) / 32 : 0, nsplit = (ngt + CT_GTS - 1) / CT_GTS;
    if (ngt > 0x7fffffffLL || nct * nsplit > 0x7fffffffLL) return ORIANA_EINVAL;
    if (nt > 0 && cm->rslots > 0) {
        hipLaunchKernelGGL(k_cell_totals, dim3((unsigned)nt), dim3(256), 0, (hipStream_t)stream, *cm, totals);
        ORIANA_LAUNCH_CHECK();
    }
    if (ngt > 0 && nct > 0) {
        hipLaunchKernelGGL(k_dn_cell_totals, dim3((unsigned)(nct * nsplit)), dim3(256), 0, (hipStream_t)stream, dn->x, row_perm,
                           totals, dn->n, (int)ngt, (int)nsplit);
        ORIANA_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int oriana_group_stats(const oriana_counts *cm, const oriana_dense *dn, const int32_t *row_perm,
                                  const int32_t *col_perm, const int32_t *labels, const double *scale, int log1p_flag,
                                  int64_t C, double *out, void *stream) {
    if (!labels || !out || C < 1) return ORIANA_EINVAL;
    if (const int rc = gs_check_layouts(cm, dn)) return rc;
    if (C > GS_MAX_GROUPS) return ORIANA_EKRANGE;
    const int64_t gd = dn ? dn->gd : 0, mtot = cm->m + gd;
    // the sliced layout: the clusters in nchunk even chunks of cc <= GS_CC; a work-group takes GS_GROUPS * iters row blocks of a
    // gene tile, iters = GS_ITERS once that leaves a gene tile at least 8 work-groups (fewer row blocks: 2, then 1)
    const int64_t nchunk = (C + GS_CC - 1) / GS_CC, cc = (C + nchunk - 1) / nchunk;
    const int64_t iters = cm->nrb >= 8 * GS_GROUPS * GS_ITERS ? GS_ITERS : (cm->nrb >= 4 * GS_GROUPS ? 2 : 1);
    const int64_t nrg = (cm->nrb + GS_GROUPS * iters - 1) / (GS_GROUPS * iters);
    const int64_t nwg = nrg * cm->ncb * nchunk;
    const size_t lds = (size_t)cc * TILE * 20 + (size_t)GS_GROUPS * TILE * 12;
    // the dense block: cell tiles per work-group -- GS_CTG, a quarter while there are fewer than two such groups
    const int64_t ngt = gd / 32, nct = dn ? (dn->n + 31) / 32 : 0;
    const int64_t ctg = nct >= 2 * GS_CTG ? GS_CTG : GS_CTG / 4;
    const int64_t ncg = (nct + ctg - 1) / ctg, ndchunk = (C + GS_DCC - 1) / GS_DCC;
    const int64_t ndwg = ncg * ngt * ndchunk;
    if (nwg > 0x7fffffffLL || ndwg > 0x7fffffffLL || ngt > 0x7fffffffLL) return ORIANA_EINVAL;
    if (nwg > 0 && cm->rslots > 0) {
        const int rc = launch(k_group_stats, dim3((unsigned)nwg), dim3(256 * GS_GROUPS), lds, (hipStream_t)stream, *cm, labels,
                              scale, log1p_flag ? 1 : 0, (int)C, mtot, gd, (int)iters, (int)nchunk, (int)cc, out);
        if (rc) return rc;
    }
    if (ndwg > 0) {
        hipLaunchKernelGGL(k_dn_group_stats, dim3((unsigned)ndwg), dim3(256), 0, (hipStream_t)stream, dn->x, row_perm, col_perm,
                           labels, scale, log1p_flag ? 1 : 0, (int)C, mtot, dn->n, (int)ngt, (int)ctg, (int)ndchunk, out);
        ORIANA_LAUNCH_CHECK();
    }
    return 0;
}
