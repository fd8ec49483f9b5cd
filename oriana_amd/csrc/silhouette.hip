// silhouette.hip -- per-cluster sums of Euclidean distances of query rows to candidate rows that lie grouped by cluster
// (oriana_cluster_distance_sums): the scan of knn.hip with the per-query list replaced by one float64 sum per query and
// cluster.  DESIGN.md section 5k.
//
// k_sil_scan    A work-group of eight waves owns one 64-query tile, staged once in LDS feature-major ([k][65], zero padding
//               features) exactly as k_knn_scan stages it, and one work item: a contiguous range of candidate rows inside ONE
//               cluster (a table entry; a large cluster is cut into several items, items of a cluster are contiguous in the
//               table).  Lane = query.  The waves take the item's 8-candidate steps in turn (wave w: steps w, w + 8, ..).  The
//               candidates are wave-uniform and come through scalar loads from the 16-byte-aligned pad4(d) image (Y itself
//               where it qualifies, else written by k_sil_pad).  f = sum_j (q_j - c_j)^2 is k_knn_scan's chain; the distance
//               sqrtf(f) (correctly rounded: no fast-math flag) is converted to float64 and added to the lane's one float64
//               running sum.  At the end the eight sums of a query are added through LDS in wave order 0..7 and written as
//               one float64 per (tile, item, lane).
// k_sil_reduce  lane = query: the items of a cluster are added in item order and written (or, with accumulate, added) to
//               sums[c * lds + q]; a cluster without rows gets 0.
// No atomics; every sum has one writer and a fixed order inside a launch.  The staging, the pad kernel and the chain are kept as a
// copy of knn.hip's text (DESIGN.md 5k says why they are not shared through a header).
#include "launch.h"

#include <vector>

namespace oriana {
namespace {

constexpr int SL_ROWS = 64;               // queries of a tile (one per lane)
constexpr int SL_LD = 65;                 // floats between two features of the LDS tile
constexpr int SL_W = 8;                   // waves of a work-group
constexpr int SL_CH = 8;                  // candidates per step
constexpr int64_t SL_MAX_D = 256;
constexpr int64_t SL_MAX_C = 32768;       // clusters of a call (with SL_MAX_SPLIT: items <= 65535, the y extent of a grid)
constexpr int64_t SL_MAX_SPLIT = 32767;   // ranges the candidates are cut into beyond one per cluster

inline int64_t sl_pad4(int64_t d) { return (d + 3) / 4 * 4; }
inline int64_t sl_pad16(int64_t b) { return (b + 15) / 16 * 16; }
inline int64_t sl_lds_bytes(int64_t dp) { return 8 * SL_W * SL_ROWS + 4 * dp * SL_LD; }
// Y itself serves as the candidate image where every row starts 16-byte aligned and holds whole groups of four features
inline bool sl_direct(const float *Y, int64_t ldy, int64_t d) { return d % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)Y & 15) == 0; }

struct SlPlan {
    int64_t dp, ntiles, target, items_ub;
    int64_t off_tab, off_part, total;         // bytes into the scratch (a padded candidate image sits at 0)
};

// sizes in range; items_ub bounds the items of every valid offsets array: one per non-empty cluster and one more per range of
// ceil(steps / target) steps, and sum_c ceil(steps_c / sp) <= clusters + steps / sp <= clusters + target
SlPlan sl_plan(int64_t nq, int64_t n, int64_t d, int64_t C, int64_t blocks, bool direct) {
    SlPlan p;
    p.dp = sl_pad4(d);
    p.ntiles = (nq + SL_ROWS - 1) / SL_ROWS;
    int64_t t = blocks > 0 ? blocks : (2 * oriana_device_cus() + p.ntiles - 1) / (p.ntiles > 0 ? p.ntiles : 1);   // two per CU
    if (t > SL_MAX_SPLIT) t = SL_MAX_SPLIT;
    if (t < 1) t = 1;
    p.target = t;
    p.items_ub = n > 0 ? t + (C < n ? C : n) : 0;
    p.off_tab = direct ? 0 : sl_pad16(n * p.dp * 4);
    p.off_part = p.off_tab + sl_pad16((2 * p.items_ub + C + 1) * 4);
    p.total = p.off_part + p.ntiles * p.items_ub * SL_ROWS * 8;
    return p;
}

// the candidates (n, d) as (n, dp) float32, zero where padded
__global__ void __launch_bounds__(256) k_sil_pad(float *__restrict__ img, const float *__restrict__ Y, int64_t ldy, int d, int dp,
                                                 int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int j = (int)(e % dp);
    const int64_t r = e / dp;
    img[e] = j < d ? Y[r * ldy + j] : 0.0f;
}

// tab: (first row, end row) of every item, int32 pairs; part: [tile][item][64] float64
__global__ void __launch_bounds__(64 * SL_W)
k_sil_scan(const float *__restrict__ Q, int64_t nq, int d, int64_t ldq, const float4 *__restrict__ img, int64_t ldi4, int dp,
           const int32_t *__restrict__ tab, double *__restrict__ part) {
    extern __shared__ double ldsd[];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    double *red = ldsd;                                                   // [wave][64]
    float *tile = reinterpret_cast<float *>(ldsd + SL_W * SL_ROWS);

    for (int e = (int)threadIdx.x; e < dp * SL_LD; e += 64 * SL_W) tile[e] = 0.0f;   // the padding features, column 64
    __syncthreads();
    // ---- stage the tile: wave w takes rows w, w + W, ..; lanes over the features; 64 / W loads in flight
    const int64_t row0 = (int64_t)blockIdx.x * SL_ROWS;
    const int nrow = nq - row0 < SL_ROWS ? (int)(nq - row0) : SL_ROWS;
    for (int kk = lane; kk < d; kk += 64) {
        float v[SL_ROWS / SL_W];
        #pragma unroll
        for (int u = 0; u < SL_ROWS / SL_W; ++u) {
            const int i = w + u * SL_W;
            v[u] = i < nrow ? Q[(row0 + i) * ldq + kk] : 0.0f;
        }
        #pragma unroll
        for (int u = 0; u < SL_ROWS / SL_W; ++u) tile[kk * SL_LD + w + u * SL_W] = v[u];
    }
    __syncthreads();

    const int r0 = __builtin_amdgcn_readfirstlane(tab[2 * blockIdx.y]);     // (rows are ints: n <= 2^31 - 9)
    const int r1 = __builtin_amdgcn_readfirstlane(tab[2 * blockIdx.y + 1]);
    const int nst = (r1 - r0 + SL_CH - 1) / SL_CH;
    const int dq = dp >> 2;
    const float *tl = tile + lane;
    double sum = 0.0;

    for (int st = w; st < nst; st += SL_W) {
        const int c0 = r0 + st * SL_CH;
        const float4 *row[SL_CH];
        #pragma unroll
        for (int j = 0; j < SL_CH; ++j) {
            const int64_t c = c0 + j < r1 ? c0 + j : r1 - 1;                     // (a step's tail re-reads the item's last row)
            row[j] = img + c * ldi4;
        }
        float acc[SL_CH];
        #pragma unroll
        for (int j = 0; j < SL_CH; ++j) acc[j] = 0.0f;
        for (int q = 0; q < dq; ++q) {
            const float y0 = tl[(4 * q + 0) * SL_LD], y1 = tl[(4 * q + 1) * SL_LD];
            const float y2 = tl[(4 * q + 2) * SL_LD], y3 = tl[(4 * q + 3) * SL_LD];
            #pragma unroll
            for (int j = 0; j < SL_CH; ++j) {
                const float4 cv = row[j][q];
                const float e0 = y0 - cv.x, e1 = y1 - cv.y, e2 = y2 - cv.z, e3 = y3 - cv.w;
                acc[j] = fmaf(e0, e0, acc[j]);
                acc[j] = fmaf(e1, e1, acc[j]);
                acc[j] = fmaf(e2, e2, acc[j]);
                acc[j] = fmaf(e3, e3, acc[j]);
            }
        }
        #pragma unroll
        for (int j = 0; j < SL_CH; ++j)
            if (c0 + j < r1) sum += (double)sqrtf(acc[j]);                       // (wave-uniform: candidates ascending)
    }

    // ---- the eight sums of a query in wave order, one float64 per (tile, item, lane)
    red[w * SL_ROWS + lane] = sum;
    __syncthreads();
    if (w == 0) {
        double s = red[lane];
        #pragma unroll
        for (int v = 1; v < SL_W; ++v) s += red[v * SL_ROWS + lane];
        part[((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * SL_ROWS + lane] = s;
    }
}

// sums[c * lds + q] (+)= the items [ioff[c], ioff[c + 1]) of cluster c = blockIdx.y, in item order
__global__ void __launch_bounds__(64)
k_sil_reduce(double *__restrict__ sums, int64_t lds, int64_t nq, const double *__restrict__ part, const int32_t *__restrict__ ioff,
             int nitems, int accumulate) {
    const int lane = (int)threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * SL_ROWS + lane;
    if (q >= nq) return;
    const int i0 = ioff[blockIdx.y], i1 = ioff[blockIdx.y + 1];
    const double *p = part + (int64_t)blockIdx.x * nitems * SL_ROWS + lane;
    double s = 0.0;
    for (int i = i0; i < i1; ++i) s += p[(int64_t)i * SL_ROWS];
    double *out = sums + (int64_t)blockIdx.y * lds + q;
    *out = accumulate ? *out + s : s;
}

int sl_check_sizes(int64_t nq, int64_t n, int64_t d, int64_t C, int64_t blocks) {
    if (nq < 0 || n < 0 || d < 1 || C < 0 || blocks < 0) return ORIANA_EINVAL;
    if (d > SL_MAX_D || C > SL_MAX_C) return ORIANA_EKRANGE;
    if (nq > 0x7fffffffLL || n > 0x7fffffffLL - SL_CH) return ORIANA_EINVAL;      // (the last step's c0 + 7 is an int)
    return 0;
}

}  // namespace
}  // namespace oriana

using namespace oriana;

extern "C" int64_t oriana_cluster_distance_sums_max_clusters(void) { return SL_MAX_C; }

extern "C" int64_t oriana_cluster_distance_sums_scratch_bytes_for(int64_t nq, int64_t n, int64_t d, int64_t C, int64_t blocks,
                                                                  const float *Y, int64_t ldy) {
    const int rc = sl_check_sizes(nq, n, d, C, blocks);
    if (rc == ORIANA_EINVAL || (d >= 1 && ldy < d)) return ORIANA_EINVAL;
    if (rc) return rc;
    return sl_plan(nq, n, d, C, blocks, sl_direct(Y, ldy, d)).total;
}

extern "C" int oriana_cluster_distance_sums(const float *Q, int64_t nq, int64_t ldq, const float *Y, int64_t n, int64_t ldy, int64_t d,
                                            const int64_t *offsets, int64_t C, double *sums, int64_t lds, int accumulate,
                                            void *scratch, int64_t blocks, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = sl_check_sizes(nq, n, d, C, blocks);
    if (rc == ORIANA_EINVAL) return rc;
    if (d >= 1 && (ldq < d || ldy < d)) return ORIANA_EINVAL;
    if (lds < nq) return ORIANA_EINVAL;
    if (rc) return rc;
    if (!offsets || !scratch || (nq > 0 && C > 0 && !sums) || (nq > 0 && !Q) || (n > 0 && !Y)) return ORIANA_EINVAL;
    if ((uintptr_t)scratch & 15) return ORIANA_EINVAL;
    if (offsets[0] != 0 || offsets[C] != n) return ORIANA_EINVAL;
    for (int64_t c = 0; c < C; ++c)
        if (offsets[c + 1] < offsets[c]) return ORIANA_EINVAL;
    if (nq == 0 || C == 0) return 0;

    const bool direct = sl_direct(Y, ldy, d);
    const SlPlan p = sl_plan(nq, n, d, C, blocks, direct);
    // ---- the item table: a cluster of s steps is cut into ceil(s / sp) items of (nearly) equal whole steps
    int64_t steps = 0;
    for (int64_t c = 0; c < C; ++c) steps += (offsets[c + 1] - offsets[c] + SL_CH - 1) / SL_CH;
    const int64_t sp = steps > 0 ? (steps + p.target - 1) / p.target : 1;
    std::vector<int32_t> items, ioff((size_t)C + 1);
    items.reserve((size_t)(2 * p.items_ub));
    for (int64_t c = 0; c < C; ++c) {
        ioff[(size_t)c] = (int32_t)(items.size() / 2);
        const int64_t a = offsets[c], b = offsets[c + 1], s = (b - a + SL_CH - 1) / SL_CH;
        if (s == 0) continue;
        const int64_t pieces = (s + sp - 1) / sp, per = (s + pieces - 1) / pieces;
        for (int64_t s0 = 0; s0 < s; s0 += per) {
            const int64_t e = a + (s0 + per) * SL_CH;
            items.push_back((int32_t)(a + s0 * SL_CH));
            items.push_back((int32_t)(e < b ? e : b));
        }
    }
    const int64_t nitems = (int64_t)(items.size() / 2);
    ioff[(size_t)C] = (int32_t)nitems;
    if (nitems > p.items_ub) return ORIANA_EINVAL;                                // (cannot happen: see sl_plan)

    char *base = static_cast<char *>(scratch);
    int32_t *tab = reinterpret_cast<int32_t *>(base + p.off_tab);
    int32_t *dioff = tab + 2 * nitems;
    double *part = reinterpret_cast<double *>(base + p.off_part);
    if (nitems > 0) {
        items.insert(items.end(), ioff.begin(), ioff.end());
    } else {
        items = ioff;
    }
    ORIANA_HIP_CHECK(hipMemcpyAsync(tab, items.data(), items.size() * 4, hipMemcpyHostToDevice, stream));
    ORIANA_HIP_CHECK(hipStreamSynchronize(stream));          // (the table and the caller's offsets may go when this returns)
    if (nitems > 0) {
        const float *img = Y;
        int64_t ldi = ldy;
        if (!direct) {
            const int64_t npad = n * p.dp;
            rc = launch(k_sil_pad, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<float *>(base), Y,
                        ldy, (int)d, (int)p.dp, npad);
            if (rc) return rc;
            img = reinterpret_cast<const float *>(base);
            ldi = p.dp;
        }
        rc = launch(k_sil_scan, dim3((unsigned)p.ntiles, (unsigned)nitems), dim3(64 * SL_W), (size_t)sl_lds_bytes(p.dp), stream, Q,
                    nq, (int)d, ldq, reinterpret_cast<const float4 *>(img), ldi / 4, (int)p.dp, tab, part);
        if (rc) return rc;
    }
    return launch(k_sil_reduce, dim3((unsigned)p.ntiles, (unsigned)C), dim3(64), 0, stream, sums, lds, nq, part, dioff, (int)nitems,
                  accumulate ? 1 : 0);
}
