// pack.hip -- repack the dense count matrix X into the tiled, sliced non-zero layout
// (struct oriana_counts, include/oriana_hip.h).
//
// Replaces `self.X[:].astype(np.float32)` (oriana/models/gap.py:94), which the reference redoes on
// every sweep: X is constant across sweeps (gap.py:29-32), so it is converted ONCE into the layout
// the responsibility kernels stream ("Data layout in HBM").  The counting and the filling kernel, and the scan
// between them; the sequence that strings them together is pack_nest.h (C hosts) / CountTiles._build (engine.py).
#include "common.h"

namespace oriana {

// an entry exists iff its float32 value (what the record stores, gap.py:94) is non-zero: a float64 count that
// rounds to 0.0f must not reserve a slot that would read as padding
template <typename T> __device__ __forceinline__ bool is_nz(T v) { return (float)v != 0.0f; }

// per-tile row / column counts -> slice offsets.  cnt[256] in LDS; thread sl < 16 owns a slice.
__device__ __forceinline__ void slice_offsets(const uint32_t *cnt, uint32_t *slice /*[17] LDS*/, int tid) {
    __shared__ uint32_t len[16];
    if (tid < 16) {
        uint32_t mx = 0;
        for (int r = 0; r < 16; ++r) mx = max(mx, cnt[tid * 16 + r]);
        len[tid] = ((mx + 3) >> 2) * 64;            // iterations of 4 records x 16 lanes-groups
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t o = 0;
        for (int s = 0; s < 16; ++s) { slice[s] = o; o += len[s]; }
        slice[16] = o;
    }
    __syncthreads();
}

// grid = (ncb, row blocks in chunk); block = 256 threads (4 waves); wave w scans rows w, w+4, ...
template <typename T>
__global__ __launch_bounds__(256) void k_pack_count(const T *__restrict__ X, int64_t rows, int64_t m, int64_t ldx,
                                                    int64_t rb0, int64_t ncb, int32_t *__restrict__ tile_nnz,
                                                    int32_t *__restrict__ tile_rslots, int32_t *__restrict__ tile_cslots,
                                                    uint32_t *__restrict__ rslice, uint32_t *__restrict__ cslice) {
    __shared__ uint32_t rcnt[TILE];
    __shared__ uint32_t ccnt[TILE];
    __shared__ uint32_t rs[17], cs[17];
    __shared__ uint32_t tot[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t cb = blockIdx.x, rbl = blockIdx.y;
    const int64_t t = (rb0 + rbl) * ncb + cb;
    ccnt[tid] = 0;
    __syncthreads();
    uint32_t mycol[4] = {0, 0, 0, 0};
    uint32_t wtot = 0;
    for (int r = w; r < TILE; r += 4) {
        const int64_t row = rbl * TILE + r;
        uint32_t rc = 0;
        #pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t col = cb * TILE + u * 64 + lane;
            bool nz = false;
            if (row < rows && col < m) nz = is_nz(X[row * ldx + col]);
            const unsigned long long mask = __ballot(nz);
            rc += __popcll(mask);
            mycol[u] += nz ? 1u : 0u;
        }
        if (lane == 0) rcnt[r] = rc;
        wtot += rc;
    }
    #pragma unroll
    for (int u = 0; u < 4; ++u) atomicAdd(&ccnt[u * 64 + lane], mycol[u]);
    if (lane == 0) tot[w] = wtot;
    __syncthreads();
    slice_offsets(rcnt, rs, tid);
    slice_offsets(ccnt, cs, tid);
    if (tid < 17) {
        rslice[t * 17 + tid] = rs[tid];
        cslice[t * 17 + tid] = cs[tid];
    }
    if (tid == 0) {
        tile_nnz[t] = (int32_t)(tot[0] + tot[1] + tot[2] + tot[3]);
        tile_rslots[t] = (int32_t)rs[16];
        tile_cslots[t] = (int32_t)cs[16] + 64;      // + the write-only dummy slots
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_pack_fill(const T *__restrict__ X, int64_t rows, int64_t m, int64_t ldx,
                                                   int64_t rb0, int64_t ncb, const int64_t *__restrict__ roff,
                                                   const int64_t *__restrict__ coff, const uint32_t *__restrict__ rslice,
                                                   const uint32_t *__restrict__ cslice, oriana_rowrec *__restrict__ rowrec,
                                                   uint8_t *__restrict__ ridx, const float *__restrict__ side,
                                                   int64_t ldside, float *__restrict__ side_nz) {
    __shared__ unsigned long long bits[TILE][4];
    __shared__ uint32_t rs[17], cs[17];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t cb = blockIdx.x, rbl = blockIdx.y;
    const int64_t t = (rb0 + rbl) * ncb + cb;
    const int64_t rbase = roff[t], cbase = coff[t];
    if (tid < 17) { rs[tid] = rslice[t * 17 + tid]; cs[tid] = cslice[t * 17 + tid]; }

    // A: non-zero bitmask of the tile
    for (int r = w; r < TILE; r += 4) {
        const int64_t row = rbl * TILE + r;
        #pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t col = cb * TILE + u * 64 + lane;
            bool nz = false;
            if (row < rows && col < m) nz = is_nz(X[row * ldx + col]);
            const unsigned long long mask = __ballot(nz);
            if (lane == 0) bits[r][u] = mask;
        }
    }
    __syncthreads();

    // B: thread c walks down its column: records go to the row-side slot of (row, rank in row) and
    // the row index to the column-side slot of (column, rank in column); both ranks follow the
    // sorted order, so the layout (and every summation order derived from it) is deterministic
    const int c = tid;
    const int cw = c >> 6, cbit = c & 63;
    const int64_t col = cb * TILE + c;
    const uint32_t cstart = cs[c >> 4] + (uint32_t)(c & 15) * 4u;
    uint32_t kc = 0;
    for (int r = 0; r < TILE; ++r) {
        const unsigned long long word = bits[r][cw];
        if ((word >> cbit) & 1ull) {
            uint32_t rank = __popcll(word & ((1ull << cbit) - 1ull));
            for (int u = 0; u < cw; ++u) rank += __popcll(bits[r][u]);
            const int64_t row = rbl * TILE + r;
            const uint32_t rslot = rs[r >> 4] + (rank >> 2) * 64u + (uint32_t)(r & 15) * 4u + (rank & 3u);
            const uint32_t cslot = cstart + (kc >> 2) * 64u + (kc & 3u);
            ++kc;
            oriana_rowrec rec;
            rec.x = (float)X[row * ldx + col];
            rec.cdst = (uint16_t)cslot;
            rec.col = (uint8_t)c;
            rec.pad = 0;
            rowrec[rbase + rslot] = rec;
            ridx[cbase + cslot] = (uint8_t)r;
            if (side_nz) side_nz[rbase + rslot] = side[row * ldside + col];
        }
    }
}

template <typename T>
static int launch_count(const void *X, int64_t rows, int64_t m, int64_t ldx, int64_t rb0, int64_t ncb,
                        int32_t *tile_nnz, int32_t *tile_rslots, int32_t *tile_cslots, uint32_t *rslice,
                        uint32_t *cslice, hipStream_t s) {
    const int64_t nrbl = (rows + TILE - 1) / TILE;
    if (nrbl == 0 || ncb == 0) return 0;
    for (int64_t y0 = 0; y0 < nrbl; y0 += 65535) {          // gridDim.y limit
        const int64_t ny = (nrbl - y0 < 65535) ? nrbl - y0 : 65535;
        dim3 grid((unsigned)ncb, (unsigned)ny);
        hipLaunchKernelGGL(k_pack_count<T>, grid, dim3(256), 0, s, (const T *)X + y0 * TILE * ldx,
                           rows - y0 * TILE, m, ldx, rb0 + y0, ncb, tile_nnz, tile_rslots, tile_cslots, rslice, cslice);
    }
    ORIANA_LAUNCH_CHECK();
    return 0;
}

template <typename T>
static int launch_fill(const void *X, int64_t rows, int64_t m, int64_t ldx, int64_t rb0, int64_t ncb,
                       const int64_t *roff, const int64_t *coff, const uint32_t *rslice, const uint32_t *cslice,
                       oriana_rowrec *rowrec, uint8_t *ridx, const float *side, int64_t ldside, float *side_nz,
                       hipStream_t s) {
    const int64_t nrbl = (rows + TILE - 1) / TILE;
    if (nrbl == 0 || ncb == 0) return 0;
    for (int64_t y0 = 0; y0 < nrbl; y0 += 65535) {
        const int64_t ny = (nrbl - y0 < 65535) ? nrbl - y0 : 65535;
        dim3 grid((unsigned)ncb, (unsigned)ny);
        hipLaunchKernelGGL(k_pack_fill<T>, grid, dim3(256), 0, s, (const T *)X + y0 * TILE * ldx,
                           rows - y0 * TILE, m, ldx, rb0 + y0, ncb, roff, coff, rslice, cslice, rowrec, ridx,
                           side ? side + y0 * TILE * ldside : nullptr, ldside, side_nz);
    }
    ORIANA_LAUNCH_CHECK();
    return 0;
}

// exclusive scan of int32 counts into int64 offsets (off[nt] = the total), one work-group: nt is at most a few 1e5
__global__ __launch_bounds__(1024) void k_scan_tiles(int64_t *__restrict__ off, const int32_t *__restrict__ cnt, int64_t nt) {
    __shared__ int64_t wsum[16];
    __shared__ int64_t carry_s;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < nt; base += 1024) {
        const int64_t i = base + tid;
        const int64_t v = (i < nt) ? (int64_t)cnt[i] : 0;
        int64_t inc = v;
        #pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int64_t pre = carry_s;
        for (int j = 0; j < w; ++j) pre += wsum[j];
        if (i < nt) off[i] = pre + inc - v;
        __syncthreads();
        if (tid == 1023) carry_s = pre + inc;
        __syncthreads();
    }
    if (tid == 0) off[nt] = carry_s;
}

}  // namespace oriana

using namespace oriana;

extern "C" int oriana_pack_count(const void *X, int xdtype, int64_t rows, int64_t m, int64_t ldx, int64_t rb0,
                                 int64_t ncb, int32_t *tile_nnz, int32_t *tile_rslots, int32_t *tile_cslots,
                                 uint32_t *rslice, uint32_t *cslice, void *stream) {
    if (rows < 0 || m < 0 || ldx < m || rb0 < 0 || ncb != (m + TILE - 1) / TILE) return ORIANA_EINVAL;
    if (rows == 0 || m == 0) return 0;
    if (!X || !tile_nnz || !tile_rslots || !tile_cslots || !rslice || !cslice) return ORIANA_EINVAL;
    hipStream_t s = (hipStream_t)stream;
#define ORIANA_PC(T) return launch_count<T>(X, rows, m, ldx, rb0, ncb, tile_nnz, tile_rslots, tile_cslots, rslice, cslice, s)
    switch (xdtype) {
        case 0: ORIANA_PC(float);
        case 1: ORIANA_PC(int64_t);
        case 2: ORIANA_PC(int32_t);
        case 3: ORIANA_PC(double);
        default: return ORIANA_EINVAL;
    }
#undef ORIANA_PC
}

extern "C" int oriana_pack_fill(const void *X, int xdtype, int64_t rows, int64_t m, int64_t ldx, int64_t rb0,
                                int64_t ncb, const int64_t *roff, const int64_t *coff, const uint32_t *rslice,
                                const uint32_t *cslice, oriana_rowrec *rowrec, uint8_t *ridx, const float *side,
                                int64_t ldside, float *side_nz, void *stream) {
    if (rows < 0 || m < 0 || ldx < m || rb0 < 0 || ncb != (m + TILE - 1) / TILE) return ORIANA_EINVAL;
    if (rows == 0 || m == 0) return 0;
    if (!X || !roff || !coff || !rslice || !cslice || !rowrec || !ridx) return ORIANA_EINVAL;
    if ((side != nullptr) != (side_nz != nullptr)) return ORIANA_EINVAL;
    hipStream_t s = (hipStream_t)stream;
#define ORIANA_PF(T) return launch_fill<T>(X, rows, m, ldx, rb0, ncb, roff, coff, rslice, cslice, rowrec, ridx, side, ldside, side_nz, s)
    switch (xdtype) {
        case 0: ORIANA_PF(float);
        case 1: ORIANA_PF(int64_t);
        case 2: ORIANA_PF(int32_t);
        case 3: ORIANA_PF(double);
        default: return ORIANA_EINVAL;
    }
#undef ORIANA_PF
}

extern "C" int oriana_pack_offsets(int64_t *roff, int64_t *coff, const int32_t *tile_rslots, const int32_t *tile_cslots, int64_t nt,
                                   int64_t *totals, void *stream) {
    if (nt < 0 || !roff || !coff || !totals || (nt > 0 && (!tile_rslots || !tile_cslots))) return ORIANA_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, s, roff, tile_rslots, nt);
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, s, coff, tile_cslots, nt);
    ORIANA_LAUNCH_CHECK();
    // the one host synchronisation of every packing sequence: the slot totals size the record arrays
    ORIANA_HIP_CHECK(hipMemcpyAsync(&totals[0], roff + nt, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    ORIANA_HIP_CHECK(hipMemcpyAsync(&totals[1], coff + nt, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    ORIANA_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}
