// ranksum.hip -- per (cluster, gene) the sum of the tie-aware positions of the cluster's stored counts among the sorted stored
// counts of the gene: what a Wilcoxon rank-sum test of a cell clustering needs from X (oriana_amd/models/base.py:
// cluster_rank_sums, marker_genes(method='wilcoxon'); no counterpart in the reference).  The zeros of X tie at the
// bottom of every gene's ranking, so only the stored entries are sorted; the host adds the zeros' share in integers.
//
// One call serves one PANEL of genes [g0, g1) of the packed order, wholly in the dense block or wholly in the sliced part:
//   count    per gene the stored non-zeros (k_rs_sliced / k_rs_dense <FILL = false>), one global atomic per (work-group, gene)
//   scan     k_rs_scan: segment offsets, the panel's total and longest segment; total > capacity sets overflow and every later
//            kernel returns at its top -- nothing is written outside the scratch
//   gather   <FILL = true>: the same walk; a work-group counts its entries per gene in LDS, reserves one range per gene of the
//            segment with ONE global atomic on the gene's cursor, and places its records {key = bits of the float64 product,
//            label} inside the range by LDS atomics.  The order inside a segment varies from run to run; nothing below depends on it.
//   sort     k_rs_sort_lds: a segment of at most sort_cap records is sorted by one work-group in LDS (bitonic); a longer one is cut
//            into runs of R = 2^floor(log2 sort_cap) records, each sorted in LDS, and k_rs_merge doubles the run length per launch
//            over two buffers: a record's place is its index in its own run plus the count of smaller (left run: smaller;
//            right run: smaller or equal) keys in the sibling run, found by binary search -- a permutation whatever the ties.
//   rank     k_rs_rank: one work-group per gene.  A record's tie run [p, q] comes from its two neighbours where the keys around it
//            differ and from two binary searches where they do not; p + q is added into an int64 table [C] in LDS, t^3 - t once
//            per run, and the gene's column is written with plain stores.
// Every term is an integer: no result depends on the order of an atomic.
#include "common.h"
#include "counts_check.h"
#include "dense_tiles.h"

namespace oriana {

constexpr int RS_MAX_GROUPS = 1024;            // oriana_rank_sums_max_groups(): the LDS table of k_rs_rank
constexpr int RS_LDS_CAP = 4096;               // oriana_rank_sums_lds_cap(): 4096 x (8 + 4) bytes = 48 KiB, three work-groups per CU
constexpr int RS_CTG = 32;                     // cell tiles (32 cells) of one gene tile a work-group of the dense walk takes
constexpr int64_t RS_MAX_CELLS = 1LL << 21;    // n below this: sum (t^3 - t) <= n^3 < 2^63
typedef unsigned long long u64;

// where the pieces of the scratch are (passed by value)
struct rs_plan {
    u64 *cnt, *off, *cur;                      // [G] stored entries per gene; [G + 2] offsets, then total, longest; [G] cursors
    u64 *keyA, *keyB;                          // [cap] each
    int32_t *labA, *labB;                      // [cap] each
    int64_t G, cap;                            // genes of the panel, records the buffers hold
    int sort_cap, run;                         // longest segment sorted in LDS; run length R of the longer ones
};
__device__ __forceinline__ bool rs_overflow(const rs_plan &pl) { return pl.off[pl.G] > (u64)pl.cap; }
// merge launch `pass` doubles runs of R << pass records; it has work while that is below the longest segment
__device__ __forceinline__ bool rs_pass_active(const rs_plan &pl, int pass) { return ((u64)pl.run << pass) < pl.off[pl.G + 1]; }

__device__ __forceinline__ u64 rs_key(float x, const double *scale, double s) {
    const double v = scale ? __dmul_rn((double)x, s) : (double)x;        // ONE float64 product; its bits are the key
    return __builtin_bit_cast(u64, v);
}

// The sliced part: one work-group per tile (row block, column block of the panel), walked as k_cell_totals walks it.
template <bool FILL>
__global__ __launch_bounds__(256) void k_rs_sliced(oriana_counts cm, const int32_t *__restrict__ labels,
                                                   const double *__restrict__ scale, int64_t cb0, int ncbp, rs_plan pl) {
    __shared__ unsigned int lc[TILE];
    __shared__ u64 base[TILE];
    if (FILL && rs_overflow(pl)) return;                         // (uniform over the grid)
    const int tid = threadIdx.x, rl = (tid & 63) >> 2;
    const int64_t rb = blockIdx.x / (unsigned)ncbp, cbl = blockIdx.x % (unsigned)ncbp;
    const int64_t t = rb * cm.ncb + cb0 + cbl;
    const int64_t rbase = cm.roff[t];
    lc[tid] = 0u;
    __syncthreads();
    for (int sl = 0; sl < 16; ++sl) {
        const uint32_t s0 = cm.rslice[t * 17 + sl], s1 = cm.rslice[t * 17 + sl + 1];
        for (uint32_t slot = s0 + tid; slot < s1; slot += 256) {
            const oriana_rowrec rec = cm.rowrec[rbase + slot];
            if (rec.x != 0.f) atomicAdd(&lc[rec.col], 1u);
        }
    }
    __syncthreads();
    const int64_t g = cbl * TILE + tid;                          // gene of the panel
    const unsigned int mine = g < pl.G ? lc[tid] : 0u;
    if (!FILL) {
        if (mine) atomicAdd(&pl.cnt[g], (u64)mine);
        return;
    }
    base[tid] = mine ? atomicAdd(&pl.cur[g], (u64)mine) : (u64)pl.cap;     // (no entry reads the base of a gene without one)
    __syncthreads();
    lc[tid] = 0u;
    __syncthreads();
    for (int sl = 0; sl < 16; ++sl) {
        const uint32_t s0 = cm.rslice[t * 17 + sl], s1 = cm.rslice[t * 17 + sl + 1];
        const int64_t ip = rb * TILE + sl * 16 + rl;             // (one row per thread and slice: slice lengths are multiples of 64)
        if (s0 == s1 || ip >= cm.n) continue;
        const int64_t i = cm.row_perm ? (int64_t)cm.row_perm[ip] : ip;
        const int32_t l = labels[i];
        const double s = scale ? scale[i] : 1.0;
        for (uint32_t slot = s0 + tid; slot < s1; slot += 256) {
            const oriana_rowrec rec = cm.rowrec[rbase + slot];
            if (rec.x == 0.f) continue;
            const u64 pos = base[rec.col] + atomicAdd(&lc[rec.col], 1u);
            if (pos < (u64)pl.cap) {                             // (always: the ranges were counted from the same walk)
                pl.keyA[pos] = rs_key(rec.x, scale, s);
                pl.labA[pos] = l;
            }
        }
    }
}

// The dense block: one work-group per (gene tile of the panel, group of ctg cell tiles), walked as k_dn_group_stats walks it: a
// thread holds the counts 4 tid .. 4 tid + 3 of a 32 x 32 block, one cell c = (tid / 2) % 32 and the genes gbase + q.
template <bool FILL>
__global__ __launch_bounds__(256) void k_rs_dense(const uint16_t *__restrict__ Xd, const int32_t *__restrict__ row_perm,
                                                  const int32_t *__restrict__ labels, const double *__restrict__ scale, int64_t n,
                                                  int ngt, int gt0, int ngtp, int ctg, rs_plan pl) {
    __shared__ unsigned int lc[32];
    __shared__ u64 base[32];
    if (FILL && rs_overflow(pl)) return;
    const int tid = threadIdx.x;
    const int gtl = (int)(blockIdx.x % (unsigned)ngtp), gt = gt0 + gtl;
    const int64_t cg = blockIdx.x / (unsigned)ngtp;
    const int c = (tid >> 1) & 31, h = (tid >> 6) & 1;
    const int gbase = dn::acc_row(8 * (tid >> 7) + 4 * (tid & 1), h);
    const int64_t nct = (n + 31) / 32;
    const int64_t ct_end = min(nct, (cg + 1) * (int64_t)ctg);
    if (tid < 32) lc[tid] = 0u;
    __syncthreads();
    for (int64_t ct = cg * ctg; ct < ct_end; ++ct) {
        if (ct * 32 + c >= n) continue;
        const uint2 w = *reinterpret_cast<const uint2 *>(Xd + (ct * ngt + gt) * 1024 + 4 * tid);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t xi = ((q & 2 ? w.y : w.x) >> (16 * (q & 1))) & 0xFFFFu;
            if (xi != 0u) atomicAdd(&lc[gbase + q], 1u);
        }
    }
    __syncthreads();
    const int64_t g = (int64_t)gtl * 32 + tid;
    unsigned int mine = 0u;
    if (tid < 32 && g < pl.G) mine = lc[tid];
    if (!FILL) {
        if (mine) atomicAdd(&pl.cnt[g], (u64)mine);
        return;
    }
    if (tid < 32) base[tid] = mine ? atomicAdd(&pl.cur[g], (u64)mine) : (u64)pl.cap;
    __syncthreads();
    if (tid < 32) lc[tid] = 0u;
    __syncthreads();
    for (int64_t ct = cg * ctg; ct < ct_end; ++ct) {
        const int64_t ip = ct * 32 + c;
        if (ip >= n) continue;
        const uint2 w = *reinterpret_cast<const uint2 *>(Xd + (ct * ngt + gt) * 1024 + 4 * tid);
        if ((w.x | w.y) == 0u) continue;
        const int64_t i = row_perm ? (int64_t)row_perm[ip] : ip;
        const int32_t l = labels[i];
        const double s = scale ? scale[i] : 1.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t xi = ((q & 2 ? w.y : w.x) >> (16 * (q & 1))) & 0xFFFFu;
            if (xi == 0u) continue;
            const u64 pos = base[gbase + q] + atomicAdd(&lc[gbase + q], 1u);
            if (pos < (u64)pl.cap) {
                pl.keyA[pos] = rs_key((float)xi, scale, s);      // (a uint16 is exact in float32)
                pl.labA[pos] = l;
            }
        }
    }
}

// off[g] = cur[g] = sum of cnt[0 .. g), off[G] = the total, off[G + 1] = the longest segment; overflow[0] = 1 where the total
// exceeds the capacity.  One work-group: a thread sums a contiguous share, the 1024 shares are scanned in LDS.
__global__ __launch_bounds__(1024) void k_rs_scan(rs_plan pl, int32_t *__restrict__ overflow) {
    __shared__ u64 part[1024], mx[1024];
    const int tid = threadIdx.x;
    const int64_t per = (pl.G + 1023) / 1024, a = min(pl.G, tid * per), b = min(pl.G, a + per);
    u64 sum = 0, big = 0;
    for (int64_t g = a; g < b; ++g) { sum += pl.cnt[g]; big = max(big, pl.cnt[g]); }
    part[tid] = sum;
    mx[tid] = big;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const u64 v = tid >= d ? part[tid - d] : 0, w = tid >= d ? mx[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        mx[tid] = max(mx[tid], w);
        __syncthreads();
    }
    u64 run = part[tid] - sum;
    for (int64_t g = a; g < b; ++g) { pl.off[g] = run; pl.cur[g] = run; run += pl.cnt[g]; }
    if (tid == 1023) {
        pl.off[pl.G] = part[1023];
        pl.off[pl.G + 1] = mx[1023];
        if (part[1023] > (u64)pl.cap) overflow[0] = 1;
    }
}

// blockIdx.x = gene of the panel; blockIdx.y, strided by gridDim.y, = run of a segment longer than sort_cap.  Sorts records
// [s0, s0 + c) of the segment in LDS: padded to a power of two with keys above every real one (v is positive and finite).
__global__ __launch_bounds__(256) void k_rs_sort_lds(rs_plan pl) {
    __shared__ u64 sk[RS_LDS_CAP];
    __shared__ int32_t sl[RS_LDS_CAP];
    if (rs_overflow(pl)) return;
    const int tid = threadIdx.x;
    const u64 o = pl.off[blockIdx.x];
    const int64_t len = (int64_t)(pl.off[blockIdx.x + 1] - o);
    const bool whole = len <= pl.sort_cap;
    if (!whole && pl.run < 2) return;
    const int64_t step = whole ? len : pl.run;
    for (int64_t r = blockIdx.y; r * step < len; r += gridDim.y) {      // (uniform over the work-group)
        if (whole && r > 0) break;
        const int64_t s0 = r * step;
        const int c = (int)min(step, len - s0);                          // <= RS_LDS_CAP: sort_cap and R are
        if (c < 2) continue;
        int P = 2;
        while (P < c) P <<= 1;
        __syncthreads();                                                 // (the last run's stores have read the tables)
        for (int e = tid; e < P; e += 256) {
            sk[e] = e < c ? pl.keyA[o + s0 + e] : ~0ull;
            sl[e] = e < c ? pl.labA[o + s0 + e] : -1;
        }
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int e = tid; e < P; e += 256) {
                    const int f = e ^ j;
                    if (f > e) {
                        const u64 ke = sk[e], kf = sk[f];
                        if ((ke > kf) == ((e & k) == 0)) {
                            sk[e] = kf; sk[f] = ke;
                            const int32_t le = sl[e]; sl[e] = sl[f]; sl[f] = le;
                        }
                    }
                }
                __syncthreads();
            }
        }
        for (int e = tid; e < c; e += 256) {
            pl.keyA[o + s0 + e] = sk[e];
            pl.labA[o + s0 + e] = sl[e];
        }
    }
}

// One thread per record of the panel.  Launch `pass` merges the sorted runs of L = R << pass records of every segment longer than
// sort_cap pairwise, from buffer A (even passes) to B or back.  A run without a sibling is copied.
__global__ __launch_bounds__(256) void k_rs_merge(rs_plan pl, int pass) {
    if (rs_overflow(pl) || !rs_pass_active(pl, pass)) return;
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r >= pl.off[pl.G]) return;
    int64_t lo = 0, hi = pl.G - 1;                               // the segment of r: the first g with off[g + 1] > r
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (pl.off[mid + 1] > r) hi = mid; else lo = mid + 1;
    }
    const u64 o = pl.off[lo];
    const int64_t len = (int64_t)(pl.off[lo + 1] - o);
    if (len <= pl.sort_cap) return;                              // (sorted in LDS; it stays in A)
    const u64 *ks = (pass & 1 ? pl.keyB : pl.keyA) + o;
    const int32_t *ls = (pass & 1 ? pl.labB : pl.labA) + o;
    u64 *kd = (pass & 1 ? pl.keyA : pl.keyB) + o;
    int32_t *ld = (pass & 1 ? pl.labA : pl.labB) + o;
    const int64_t L = (int64_t)pl.run << pass, i = (int64_t)(r - o);
    const int64_t pb = i / (2 * L) * (2 * L), mid = min(len, pb + L), end = min(len, pb + 2 * L);
    const u64 k = ks[i];
    int64_t a, b, at;
    if (i < mid) {                                               // left run: the keys of the right run below k
        a = mid; b = end;
        while (a < b) { const int64_t c = (a + b) >> 1; if (ks[c] < k) a = c + 1; else b = c; }
        at = i + (a - mid);
    } else {                                                     // right run: the keys of the left run up to k
        a = pb; b = mid;
        while (a < b) { const int64_t c = (a + b) >> 1; if (ks[c] <= k) a = c + 1; else b = c; }
        at = (i - mid) + a;
    }
    kd[at] = k;                                                  // (pb <= at < end <= len: inside the segment)
    ld[at] = ls[i];
}

// One work-group per gene of the panel: pos2[c, j] = sum over the cluster's records of (p + q), [p, q] the 1-based positions of
// the record's tie run; cnt[c, j] = its records; ties[j] = sum over the runs of t^3 - t.  Plain stores: the gene's column is
// this work-group's alone.  A label outside [0, C) is ranked and added nowhere.
__global__ __launch_bounds__(256) void k_rs_rank(rs_plan pl, int npass, int C, int64_t mtot, const int32_t *__restrict__ col_perm,
                                                 int64_t jp0, int64_t *__restrict__ pos2, int64_t *__restrict__ cnt,
                                                 int64_t *__restrict__ ties) {
    __shared__ u64 tab[RS_MAX_GROUPS];
    __shared__ unsigned int tc[RS_MAX_GROUPS];
    __shared__ u64 T;
    if (rs_overflow(pl)) return;
    const int tid = threadIdx.x;
    const u64 o = pl.off[blockIdx.x];
    const int64_t len = (int64_t)(pl.off[blockIdx.x + 1] - o);
    for (int c = tid; c < C; c += 256) { tab[c] = 0; tc[c] = 0u; }
    if (tid == 0) T = 0;
    __syncthreads();
    int nact = 0;
    if (len > pl.sort_cap)
        for (int p = 0; p < npass; ++p) nact += rs_pass_active(pl, p) ? 1 : 0;
    const u64 *ks = (nact & 1 ? pl.keyB : pl.keyA) + o;
    const int32_t *ls = (nact & 1 ? pl.labB : pl.labA) + o;
    u64 tt = 0;
    for (int64_t i = tid; i < len; i += 256) {
        const u64 k = ks[i];
        int64_t p = i, q = i;
        if (i > 0 && ks[i - 1] == k) {                           // the first record of the run: the first key >= k in [0, i - 1)
            int64_t a = 0, b = i - 1;
            while (a < b) { const int64_t c = (a + b) >> 1; if (ks[c] < k) a = c + 1; else b = c; }
            p = a;
        }
        if (i + 1 < len && ks[i + 1] == k) {                     // the last one: the last key <= k in (i + 1, len)
            int64_t a = i + 2, b = len;
            while (a < b) { const int64_t c = (a + b) >> 1; if (ks[c] <= k) a = c + 1; else b = c; }
            q = a - 1;
        }
        const int32_t l = ls[i];
        if ((unsigned)l < (unsigned)C) {
            atomicAdd(&tab[l], (u64)(p + q + 2));
            atomicAdd(&tc[l], 1u);
        }
        if (i == p) {
            const u64 t = (u64)(q - p + 1);
            tt += t * t * t - t;
        }
    }
    if (tt) atomicAdd(&T, tt);
    __syncthreads();
    const int64_t jp = jp0 + blockIdx.x;
    const int64_t j = col_perm ? (int64_t)col_perm[jp] : jp;
    for (int c = tid; c < C; c += 256) {
        pos2[(int64_t)c * mtot + j] = (int64_t)tab[c];
        cnt[(int64_t)c * mtot + j] = (int64_t)tc[c];
    }
    if (tid == 0) ties[j] = (int64_t)T;
}

}  // namespace oriana

using namespace oriana;

static int64_t rs_header_bytes(int64_t genes) { return ((3 * genes + 2) * 8 + 15) / 16 * 16; }

extern "C" int64_t oriana_rank_sums_max_groups(void) { return RS_MAX_GROUPS; }
extern "C" int64_t oriana_rank_sums_lds_cap(void) { return RS_LDS_CAP; }

extern "C" int64_t oriana_rank_sums_scratch_bytes_for(int64_t records, int64_t genes) {
    if (records < 0 || genes < 0 || records > (1LL << 56) || genes > (1LL << 56)) return ORIANA_EINVAL;
    return rs_header_bytes(genes) + records * 24;
}

extern "C" int oriana_rank_sums(const oriana_counts *cm, const oriana_dense *dn, const int32_t *row_perm, const int32_t *col_perm,
                                const int32_t *labels, const double *scale, int64_t C, int64_t g0, int64_t g1, void *scratch,
                                int64_t capacity_records, int64_t lds_cap, int64_t *pos2, int64_t *cnt, int64_t *ties,
                                int32_t *overflow, void *stream) {
    if (!labels || !pos2 || !cnt || !ties || !overflow || !scratch || C < 1) return ORIANA_EINVAL;
    if (const int rc = gs_check_layouts(cm, dn)) return rc;
    if ((reinterpret_cast<uintptr_t>(scratch) & 15) || capacity_records < 0 || capacity_records > (1LL << 38) || lds_cap < 0 ||
        lds_cap > RS_LDS_CAP)
        return ORIANA_EINVAL;
    const int64_t gd = dn ? dn->gd : 0, mtot = cm->m + gd, n = cm->n;
    if (g0 < 0 || g1 < g0 || g1 > mtot) return ORIANA_EINVAL;
    const bool dense = g0 < gd;
    if (g1 > g0) {
        if (dense && (g1 > gd || (g0 & 31) || (g1 & 31))) return ORIANA_EINVAL;
        if (!dense && ((g0 - gd) % TILE != 0 || ((g1 - gd) % TILE != 0 && g1 != mtot))) return ORIANA_EINVAL;
    }
    if (C > RS_MAX_GROUPS || n >= RS_MAX_CELLS) return ORIANA_EKRANGE;
    const int64_t G = g1 - g0;
    if (G == 0 || n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    rs_plan pl;
    char *base = static_cast<char *>(scratch);
    pl.cnt = reinterpret_cast<u64 *>(base);
    pl.off = pl.cnt + G;
    pl.cur = pl.off + G + 2;
    pl.keyA = reinterpret_cast<u64 *>(base + rs_header_bytes(G));
    pl.keyB = pl.keyA + capacity_records;
    pl.labA = reinterpret_cast<int32_t *>(pl.keyB + capacity_records);
    pl.labB = pl.labA + capacity_records;
    pl.G = G;
    pl.cap = capacity_records;
    pl.sort_cap = (int)(lds_cap ? lds_cap : RS_LDS_CAP);
    pl.run = 1;
    while (2 * pl.run <= pl.sort_cap) pl.run *= 2;
    int npass = 0;                                               // (no segment is longer than n)
    while (((int64_t)pl.run << npass) < n) ++npass;
    const int64_t nruns = (n + pl.run - 1) / pl.run;

    // the walks: sliced tiles (row block, column block of the panel), or dense (gene tile of the panel, group of cell tiles)
    const int64_t cb0 = dense ? 0 : (g0 - gd) / TILE, ncbp = dense ? 0 : (G + TILE - 1) / TILE;
    const int64_t nct = (n + 31) / 32, ctg = nct >= 2 * RS_CTG ? RS_CTG : RS_CTG / 4, ncg = (nct + ctg - 1) / ctg;
    const int64_t ngt = gd / 32, gt0 = g0 / 32, ngtp = G / 32;
    const int64_t nwalk = dense ? ncg * ngtp : (cm->rslots > 0 ? cm->nrb * ncbp : 0);
    const int64_t nmerge = (capacity_records + 255) / 256;
    if (!dense && cb0 + ncbp > cm->ncb) return ORIANA_EINVAL;   // (a layout whose ncb is not ceil(m / 256))
    if (nwalk > 0x7fffffffLL || G > 0x7fffffffLL || nmerge > 0x7fffffffLL || ngt > 0x7fffffffLL || ncbp > 0x7fffffffLL)
        return ORIANA_EINVAL;

    ORIANA_HIP_CHECK(hipMemsetAsync(pl.cnt, 0, (size_t)G * 8, st));
    if (nwalk > 0) {
        if (dense)
            hipLaunchKernelGGL(k_rs_dense<false>, dim3((unsigned)nwalk), dim3(256), 0, st, dn->x, row_perm, labels, scale, n,
                               (int)ngt, (int)gt0, (int)ngtp, (int)ctg, pl);
        else
            hipLaunchKernelGGL(k_rs_sliced<false>, dim3((unsigned)nwalk), dim3(256), 0, st, *cm, labels, scale, cb0, (int)ncbp, pl);
        ORIANA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, st, pl, overflow);
    ORIANA_LAUNCH_CHECK();
    if (nwalk > 0 && capacity_records > 0) {
        if (dense)
            hipLaunchKernelGGL(k_rs_dense<true>, dim3((unsigned)nwalk), dim3(256), 0, st, dn->x, row_perm, labels, scale, n,
                               (int)ngt, (int)gt0, (int)ngtp, (int)ctg, pl);
        else
            hipLaunchKernelGGL(k_rs_sliced<true>, dim3((unsigned)nwalk), dim3(256), 0, st, *cm, labels, scale, cb0, (int)ncbp, pl);
        ORIANA_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_rs_sort_lds, dim3((unsigned)G, (unsigned)min((int64_t)65535, nruns)), dim3(256), 0, st, pl);
        ORIANA_LAUNCH_CHECK();
        for (int pass = 0; pass < npass; ++pass) {
            hipLaunchKernelGGL(k_rs_merge, dim3((unsigned)nmerge), dim3(256), 0, st, pl, pass);
            ORIANA_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(k_rs_rank, dim3((unsigned)G), dim3(256), 0, st, pl, npass, (int)C, mtot, col_perm, g0, pos2, cnt, ties);
    ORIANA_LAUNCH_CHECK();
    return 0;
}
