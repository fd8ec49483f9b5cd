// community.hip -- graph communities of the cells on the neighbour graph of oriana_knn (oriana_amd/cluster.py: snn_graph, louvain;
// models/base.py: cell_communities; no counterpart in the reference).
//
//   oriana_snn_weights    w_ij = |Nc(i) & Nc(j)| for every stored entry (i, j) of the symmetric pattern, Nc(i) = the valid entries
//                         of row i of `indices` and i itself.  One wave per row i: Nc(i) is staged once in LDS, lane = stored
//                         entry, the lane walks the k entries of row j and j itself and counts the members of Nc(i).
//   oriana_louvain_sweep  ONE synchronous local-moving sweep: every node decides from the OLD comm / tot / size, so the outcome
//                         is a function of the graph and the state alone.  One work-group per row: the weights towards each
//                         neighbouring community are added into an open-addressing table keyed by community id (claimed by
//                         compare-and-swap, added by integer atomics), the slots are walked, the gain of each candidate is formed
//                         in ONE float64 sequence (lv_gain) and the best is taken under a total order (gain descending, id
//                         ascending).  Rows of at most row_cap entries: a work-group of one wave, table in LDS.  Longer rows: a
//                         work-group of four waves, the same code over a table in the caller's scratch.
// Every k_ic is an integer sum and the order is total: no result depends on the order of an atomic, on `blocks`, on the table
// size or on which path a row takes.  No float atomics anywhere.
#include "launch.h"
#include <limits.h>

namespace oriana {
namespace {

typedef unsigned long long u64;

constexpr int SN_SLOTS = 128;                  // LDS slots of Nc(i): k + 1 <= oriana_knn_max_neighbors(1) + 1 = 80
constexpr int LV_ROW_CAP = 128;                // oriana_louvain_row_cap(): the longest row whose table lives in LDS
constexpr int LV_LDS_SLOTS = 2 * LV_ROW_CAP;   // 256 x (4 + 8) bytes = 3 KiB per one-wave work-group
constexpr int64_t LV_MAX_2M = 3037000499LL;    // floor(sqrt(2^63 - 1)): (2m)^2 < 2^63
constexpr int LV_LONG_NT = 256;

// ---- the shared-neighbour weights ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_snn_weights(const int32_t *__restrict__ idx, int64_t n, int k, const int64_t *__restrict__ rp, const int32_t *__restrict__ col,
              int64_t *__restrict__ wout) {
    __shared__ int32_t nb[SN_SLOTS];
    const int lane = (int)threadIdx.x;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        __syncthreads();                                           // (the last row's lanes have read nb)
        for (int t = lane; t <= k; t += 64) {                      // Nc(i): an entry that is not valid is kept as -1, it matches nothing
            int32_t v = (int32_t)i;
            if (t < k) {
                v = idx[i * k + t];
                if (v < 0 || v >= n || v == i) v = -1;
            }
            nb[t] = v;
        }
        __syncthreads();
        const int64_t e0 = rp[i], e1 = rp[i + 1];
        for (int64_t e = e0 + lane; e < e1; e += 64) {
            const int64_t j = col[e];
            int64_t cnt = 0;
            if (j >= 0 && j < n) {                                 // (a column outside the graph addresses nothing)
                for (int t = 0; t <= k; ++t) {
                    int32_t u = (int32_t)j;
                    if (t < k) {
                        u = idx[j * k + t];
                        if (u < 0 || u >= n || u == j) continue;
                    }
                    for (int s = 0; s <= k; ++s) cnt += nb[s] == u ? 1 : 0;
                }
            }
            wout[e] = cnt;
        }
    }
}

// ---- the local-moving sweep ----------------------------------------------------------------------------------------------------
// THE GAIN of candidate c for node i (include/oriana_hip.h states it): both integer products are exact in int64, each is converted
// once, the product with the resolution and the difference are rounded once each; written with the intrinsics so that no
// contraction setting decides the bits.
__device__ __forceinline__ double lv_gain(int64_t two_m, int64_t kic, double gamma, int64_t degi, int64_t totp) {
    return __dsub_rn((double)(two_m * kic), __dmul_rn(gamma, (double)(degi * totp)));
}
// the total order of the candidates: gain descending, id ascending
__device__ __forceinline__ bool lv_better(double g, int32_t c, double bg, int32_t bc) { return g > bg || (g == bg && c < bc); }

struct lv_slot { int32_t key; int32_t pad; u64 w; };             // a slot of the table in the scratch: 16 bytes

struct LvLdsTab {                                                  // the table of a short row
    static constexpr bool in_scratch = false;
    int32_t *k;
    u64 *w;
    __device__ __forceinline__ int32_t *key(int s) const { return k + s; }
    __device__ __forceinline__ u64 *wt(int s) const { return w + s; }
    __device__ __forceinline__ int32_t read_key(int s) const { return k[s]; }
    __device__ __forceinline__ u64 read_wt(int s) const { return w[s]; }
};
struct LvGlobalTab {                                               // the table of a long row: read past the L1, where the atomics landed
    static constexpr bool in_scratch = true;
    lv_slot *t;
    __device__ __forceinline__ int32_t *key(int s) const { return &t[s].key; }
    __device__ __forceinline__ u64 *wt(int s) const { return &t[s].w; }
    __device__ __forceinline__ int32_t read_key(int s) const { return __hip_atomic_load(&t[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ u64 read_wt(int s) const { return __hip_atomic_load(&t[s].w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// the slot of community c (c >= 0) in a table of T = 1 << lg slots that holds fewer than T keys: claimed if it is new
template <class Tab>
__device__ __forceinline__ int lv_claim(const Tab &tab, int T, int lg, int32_t c) {
    int s = (int)(((uint32_t)c * 0x9E3779B1u) >> (32 - lg));
    for (;;) {
        const int32_t prev = atomicCAS(tab.key(s), -1, c);
        if (prev == -1 || prev == c) return s;
        s = (s + 1) & (T - 1);
    }
}

// slots of the table of a row of len entries: 2 pow2(len), at least 64 (the candidates are at most len + 1 <= T / 2 + 1)
__host__ __device__ __forceinline__ int lv_log_slots(int64_t len) {
    int lg = 6;
    while (((int64_t)1 << lg) < 2 * len) ++lg;                     // 2 pow2ceil(len) is the least power of two >= 2 len
    return lg;
}

struct lv_args {
    int64_t n;
    const int64_t *rp;
    const int32_t *col;
    const int64_t *w, *deg;
    int64_t two_m;
    double gamma;
    const int32_t *comm;
    const int64_t *tot;
    const int32_t *size;
    int32_t *comm_new;
};

// One row by the NT threads of a work-group; returns (in thread 0) whether the node moves.
template <int NT, class Tab>
__device__ __forceinline__ int lv_row(const lv_args &A, const Tab &tab, int lg, int64_t i, double *s_g, int32_t *s_c, double *s_ga) {
    const int tid = (int)threadIdx.x;
    const int T = 1 << lg;
    const int64_t e0 = A.rp[i], e1 = A.rp[i + 1];
    const int32_t a = A.comm[i];
    if (a < 0 || a >= A.n) {                                       // (uniform) a state outside the contract: the node stays
        if (tid == 0) A.comm_new[i] = a;
        return 0;
    }
    __syncthreads();                                               // (the last row's table and sums have been read)
    for (int s = tid; s < T; s += NT) { *tab.key(s) = -1; *tab.wt(s) = 0; }
    if (Tab::in_scratch) __threadfence();                          // the cleared slots are in L2 before another wave's atomics
    __syncthreads();
    if (tid == 0) lv_claim(tab, T, lg, a);                         // a is a candidate whatever k_ia is
    for (int64_t e = e0 + tid; e < e1; e += NT) {
        const int64_t j = A.col[e];
        if (j == i || j < 0 || j >= A.n) continue;                 // the self entry never counts
        const int32_t c = A.comm[j];
        if (c < 0 || c >= A.n) continue;
        const int s = lv_claim(tab, T, lg, c);
        atomicAdd(tab.wt(s), (u64)A.w[e]);
    }
    __syncthreads();
    const int64_t degi = A.deg[i];
    double bg = -INFINITY;
    int32_t bc = INT_MAX;
    for (int s = tid; s < T; s += NT) {
        const int32_t c = tab.read_key(s);
        if (c < 0) continue;
        const int64_t kic = (int64_t)tab.read_wt(s);
        const int64_t totp = A.tot[c] - (c == a ? degi : 0);
        const double g = lv_gain(A.two_m, kic, A.gamma, degi, totp);
        if (c == a) *s_ga = g;
        if (lv_better(g, c, bg, bc)) { bg = g; bc = c; }
    }
    for (int o = 32; o > 0; o >>= 1) {                             // the order is total: any shape gives the same winner
        const double og = __shfl_xor(bg, o, 64);
        const int32_t oc = __shfl_xor(bc, o, 64);
        if (lv_better(og, oc, bg, bc)) { bg = og; bc = oc; }
    }
    if ((tid & 63) == 0) { s_g[tid >> 6] = bg; s_c[tid >> 6] = bc; }
    __syncthreads();
    int move = 0;
    if (tid == 0) {
        for (int v = 1; v < NT / 64; ++v)
            if (lv_better(s_g[v], s_c[v], bg, bc)) { bg = s_g[v]; bc = s_c[v]; }
        move = bc != a && bg > *s_ga;
        if (move && A.size[a] == 1 && A.size[bc] == 1 && !(bc < a)) move = 0;       // the swap guard
        A.comm_new[i] = move ? bc : a;
    }
    return move;
}

// hdr[0] = 1 where the long rows' tables do not fit the scratch (then overflow[0] = 1 and no later kernel writes anything)
__global__ void k_lv_begin(int64_t *hdr, const int64_t *__restrict__ long_off, int64_t n_long, int64_t cap_slots, int64_t *moved,
                           int32_t *overflow) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t total = n_long > 0 ? long_off[n_long] : 0;
    const bool over = total < 0 || total > cap_slots;
    hdr[0] = over ? 1 : 0;
    if (over) overflow[0] = 1;
    else moved[0] = 0;
}

__global__ void __launch_bounds__(64) k_lv_sweep_short(lv_args A, int row_cap, const int64_t *__restrict__ hdr, int64_t *moved) {
    __shared__ int32_t tk[LV_LDS_SLOTS];
    __shared__ u64 tw[LV_LDS_SLOTS];
    __shared__ double s_g[1], s_ga;
    __shared__ int32_t s_c[1];
    if (hdr[0]) return;
    const LvLdsTab tab{tk, tw};
    int nmoved = 0;
    for (int64_t i = blockIdx.x; i < A.n; i += gridDim.x) {
        const int64_t len = A.rp[i + 1] - A.rp[i];
        if (len < 0 || len > row_cap) continue;                    // (uniform) a long row is the other kernel's
        nmoved += lv_row<64>(A, tab, lv_log_slots(len), i, s_g, s_c, &s_ga);
    }
    if (threadIdx.x == 0 && nmoved) atomicAdd((u64 *)moved, (u64)nmoved);        // one atomic per wave
}

__global__ void __launch_bounds__(LV_LONG_NT)
k_lv_sweep_long(lv_args A, int row_cap, const int32_t *__restrict__ long_rows, const int64_t *__restrict__ long_off, int64_t n_long,
                lv_slot *slots, int64_t cap_slots, const int64_t *__restrict__ hdr, int64_t *moved) {
    __shared__ double s_g[LV_LONG_NT / 64], s_ga;
    __shared__ int32_t s_c[LV_LONG_NT / 64];
    if (hdr[0]) return;
    int nmoved = 0;
    for (int64_t q = blockIdx.x; q < n_long; q += gridDim.x) {
        const int64_t i = long_rows[q], off = long_off[q];
        if (i < 0 || i >= A.n) continue;
        const int64_t len = A.rp[i + 1] - A.rp[i];
        if (len <= row_cap || len > (1LL << 29)) continue;         // (a short row is the other kernel's)
        const int lg = lv_log_slots(len);
        if (off < 0 || off + ((int64_t)1 << lg) > cap_slots) continue;           // never outside the scratch
        nmoved += lv_row<LV_LONG_NT>(A, LvGlobalTab{slots + off}, lg, i, s_g, s_c, &s_ga);
    }
    if (threadIdx.x == 0 && nmoved) atomicAdd((u64 *)moved, (u64)nmoved);
}

}  // namespace
}  // namespace oriana

using namespace oriana;

extern "C" int oriana_snn_weights(const int32_t *indices, int64_t n, int64_t k, const int64_t *row_ptr, const int32_t *cols,
                                  int64_t *weights, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || k < 1 || n > 0x7fffffffLL) return ORIANA_EINVAL;
    if (k > oriana_knn_max_neighbors(1)) return ORIANA_EINVAL;
    if (n == 0) return 0;
    if (!indices || !row_ptr) return ORIANA_EINVAL;                // (cols and weights may be NULL for a pattern without entries)
    const int64_t nb = n < (1LL << 20) ? n : (1LL << 20);
    return launch(k_snn_weights, dim3((unsigned)nb), dim3(64), 0, stream, indices, n, (int)k, row_ptr, cols, weights);
}

extern "C" int64_t oriana_louvain_row_cap(void) { return LV_ROW_CAP; }

extern "C" int64_t oriana_louvain_sweep_scratch_bytes_for(int64_t long_slots) {
    if (long_slots < 0 || long_slots > (1LL << 56)) return ORIANA_EINVAL;
    return 16 + 16 * long_slots;
}

extern "C" int oriana_louvain_sweep(int64_t n, const int64_t *row_ptr, const int32_t *cols, const int64_t *weights,
                                    const int64_t *deg, int64_t two_m, double resolution, const int32_t *comm, const int64_t *tot,
                                    const int32_t *size, int64_t row_cap, const int32_t *long_rows, const int64_t *long_off,
                                    int64_t n_long, void *scratch, int64_t scratch_bytes, int32_t *comm_new, int64_t *moved,
                                    int32_t *overflow, int64_t blocks, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || n > 0x7fffffffLL || two_m < 0 || two_m > LV_MAX_2M || !(resolution > 0.0) || !(resolution < INFINITY))
        return ORIANA_EINVAL;
    if (row_cap < 0 || row_cap > LV_ROW_CAP || blocks < 0 || n_long < 0 || n_long > n || scratch_bytes < 16) return ORIANA_EINVAL;
    if (!scratch || ((uintptr_t)scratch & 15) || !moved || !overflow) return ORIANA_EINVAL;
    if (n > 0 && (!row_ptr || !deg || !comm || !tot || !size || !comm_new)) return ORIANA_EINVAL;
    if (n_long > 0 && (!long_rows || !long_off)) return ORIANA_EINVAL;
    const int cap = (int)(row_cap ? row_cap : LV_ROW_CAP);
    int64_t *hdr = static_cast<int64_t *>(scratch);
    lv_slot *slots = reinterpret_cast<lv_slot *>(static_cast<char *>(scratch) + 16);
    const int64_t cap_slots = (scratch_bytes - 16) / 16;
    int rc = launch(k_lv_begin, dim3(1), dim3(1), 0, stream, hdr, long_off, n_long, cap_slots, moved, overflow);
    if (rc || n == 0) return rc;
    const lv_args A{n, row_ptr, cols, weights, deg, two_m, resolution, comm, tot, size, comm_new};
    const int64_t cus = oriana_device_cus();
    int64_t nb = blocks > 0 ? blocks : 32 * cus;
    if (nb > n) nb = n;
    rc = launch(k_lv_sweep_short, dim3((unsigned)nb), dim3(64), 0, stream, A, cap, hdr, moved);
    if (rc || n_long == 0) return rc;
    int64_t nl = blocks > 0 ? blocks : 8 * cus;
    if (nl > n_long) nl = n_long;
    return launch(k_lv_sweep_long, dim3((unsigned)nl), dim3(LV_LONG_NT), 0, stream, A, cap, long_rows, long_off, n_long, slots,
                  cap_slots, hdr, moved);
}
