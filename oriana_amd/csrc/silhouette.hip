// silhouette.hip -- per-cluster sums of Euclidean distances of query rows to candidate rows that lie grouped by cluster
// (oriana_cluster_distance_sums): the scan of knn.hip with the per-query list replaced by one float64 sum per query and
// cluster.  DESIGN.md section 5k.
//
// k_sil_scan    A work-group of eight waves owns one 64-query tile, staged once in LDS (rowscan.h: stage_tile), and one work
//               item: a contiguous range of candidate rows inside ONE cluster (a table entry; a large cluster is cut into
//               several items, items of a cluster are contiguous in the table).  Lane = query.  The waves take the item's
//               8-candidate steps in turn (wave w: steps w, w + 8, ..).  The candidates are wave-uniform and come through scalar
//               loads from the image of rowscan.h (row_image; the pad kernel is knn.hip's).  f is rowscan.h's chain8; the
//               distance sqrtf(f) (correctly rounded: no fast-math flag) is converted to float64 and added to the lane's one
//               float64 running sum.  At the end the eight sums of a query are added through LDS in wave order 0..7 and written
//               as one float64 per (tile, item, lane).
// k_sil_reduce  lane = query: the items of a cluster are added in item order (rowscan.h: add_ranges) and written (or, with
//               accumulate, added) to sums[c * lds + q]; a cluster without rows gets 0.
// No atomics; every sum has one writer and a fixed order inside a launch.
#include "rowscan.h"

#include <vector>

namespace oriana {
namespace {

constexpr int SL_W = 8;                   // waves of a work-group
constexpr int64_t SL_MAX_C = 32768;       // clusters of a call (with SL_MAX_SPLIT: items <= 65535, the y extent of a grid)
constexpr int64_t SL_MAX_SPLIT = 32767;   // ranges the candidates are cut into beyond one per cluster

inline int64_t sl_lds_bytes(int64_t dp) { return 8 * SL_W * RS_ROWS + 4 * dp * RS_LD; }

struct SlPlan {
    int64_t dp, ntiles, target, items_ub;
    int64_t off_tab, off_part, total;         // bytes into the scratch (a padded candidate image sits at 0)
};

// sizes in range; items_ub bounds the items of every valid offsets array: one per non-empty cluster and one more per range of
// ceil(steps / target) steps, and sum_c ceil(steps_c / sp) <= clusters + steps / sp <= clusters + target
SlPlan sl_plan(int64_t nq, int64_t n, int64_t d, int64_t C, int64_t blocks, bool direct) {
    SlPlan p;
    p.dp = pad4(d);
    p.ntiles = (nq + RS_ROWS - 1) / RS_ROWS;
    int64_t t = two_per_cu(blocks, p.ntiles);
    if (t > SL_MAX_SPLIT) t = SL_MAX_SPLIT;
    if (t < 1) t = 1;
    p.target = t;
    p.items_ub = n > 0 ? t + (C < n ? C : n) : 0;
    p.off_tab = direct ? 0 : pad16(n * p.dp * 4);
    p.off_part = p.off_tab + pad16((2 * p.items_ub + C + 1) * 4);
    p.total = p.off_part + p.ntiles * p.items_ub * RS_ROWS * 8;
    return p;
}

// tab: (first row, end row) of every item, int32 pairs; part: [tile][item][64] float64
__global__ void __launch_bounds__(64 * SL_W)
k_sil_scan(const float *__restrict__ Q, int64_t nq, int d, int64_t ldq, const float4 *__restrict__ img, int64_t ldi4, int dp,
           const int32_t *__restrict__ tab, double *__restrict__ part) {
    extern __shared__ double ldsd[];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    double *red = ldsd;                                                   // [wave][64]
    float *tile = reinterpret_cast<float *>(ldsd + SL_W * RS_ROWS);

    zero_tile<SL_W>(tile, dp);
    __syncthreads();
    stage_tile<SL_W>(tile, Q, nq, d, ldq, (int64_t)blockIdx.x * RS_ROWS, w, lane);
    __syncthreads();

    const int r0 = __builtin_amdgcn_readfirstlane(tab[2 * blockIdx.y]);     // (rows are ints: n <= 2^31 - 9)
    const int r1 = __builtin_amdgcn_readfirstlane(tab[2 * blockIdx.y + 1]);
    const int nst = (r1 - r0 + RS_CH - 1) / RS_CH;
    const int dq = dp >> 2;
    const float *tl = tile + lane;
    double sum = 0.0;

    for (int st = w; st < nst; st += SL_W) {
        const int c0 = r0 + st * RS_CH;
        const float4 *row[RS_CH];
        float acc[RS_CH];
        pick_rows8(row, img, ldi4, c0, r1);
        chain8(acc, tl, dq, row);
        #pragma unroll
        for (int j = 0; j < RS_CH; ++j)
            if (c0 + j < r1) sum += (double)sqrtf(acc[j]);                       // (wave-uniform: candidates ascending)
    }

    // ---- the eight sums of a query in wave order, one float64 per (tile, item, lane)
    red[w * RS_ROWS + lane] = sum;
    __syncthreads();
    if (w == 0) {
        double s = red[lane];
        #pragma unroll
        for (int v = 1; v < SL_W; ++v) s += red[v * RS_ROWS + lane];
        part[((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * RS_ROWS + lane] = s;
    }
}

// sums[c * lds + q] (+)= the items [ioff[c], ioff[c + 1]) of cluster c = blockIdx.y, in item order
__global__ void __launch_bounds__(64)
k_sil_reduce(double *__restrict__ sums, int64_t lds, int64_t nq, const double *__restrict__ part, const int32_t *__restrict__ ioff,
             int nitems, int accumulate) {
    const int lane = (int)threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * RS_ROWS + lane;
    if (q >= nq) return;
    double s[1];
    add_ranges(s, part, nitems, ioff[blockIdx.y], ioff[blockIdx.y + 1], lane);
    double *out = sums + (int64_t)blockIdx.y * lds + q;
    *out = accumulate ? *out + s[0] : s[0];
}

int sl_check_sizes(int64_t nq, int64_t n, int64_t d, int64_t C, int64_t blocks) {
    if (nq < 0 || n < 0 || d < 1 || C < 0 || blocks < 0) return ORIANA_EINVAL;
    if (d > RS_MAX_D || C > SL_MAX_C) return ORIANA_EKRANGE;
    if (!rows_fit_int(nq, n)) return ORIANA_EINVAL;
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
    return sl_plan(nq, n, d, C, blocks, direct_image(Y, ldy, d)).total;
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

    const bool direct = direct_image(Y, ldy, d);
    const SlPlan p = sl_plan(nq, n, d, C, blocks, direct);
    // ---- the item table: a cluster of s steps is cut into ceil(s / sp) items of (nearly) equal whole steps
    int64_t steps = 0;
    for (int64_t c = 0; c < C; ++c) steps += (offsets[c + 1] - offsets[c] + RS_CH - 1) / RS_CH;
    const int64_t sp = steps > 0 ? (steps + p.target - 1) / p.target : 1;
    std::vector<int32_t> items, ioff((size_t)C + 1);
    items.reserve((size_t)(2 * p.items_ub));
    for (int64_t c = 0; c < C; ++c) {
        ioff[(size_t)c] = (int32_t)(items.size() / 2);
        const int64_t a = offsets[c], b = offsets[c + 1], s = (b - a + RS_CH - 1) / RS_CH;
        if (s == 0) continue;
        const int64_t pieces = (s + sp - 1) / sp, per = (s + pieces - 1) / pieces;
        for (int64_t s0 = 0; s0 < s; s0 += per) {
            const int64_t e = a + (s0 + per) * RS_CH;
            items.push_back((int32_t)(a + s0 * RS_CH));
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
        RowImage img;
        rc = row_image(Y, n, ldy, d, base, stream, &img);
        if (rc) return rc;
        rc = launch(k_sil_scan, dim3((unsigned)p.ntiles, (unsigned)nitems), dim3(64 * SL_W), (size_t)sl_lds_bytes(p.dp), stream, Q,
                    nq, (int)d, ldq, img.rows, img.ld4, (int)p.dp, tab, part);
        if (rc) return rc;
    }
    return launch(k_sil_reduce, dim3((unsigned)p.ntiles, (unsigned)C), dim3(64), 0, stream, sums, lds, nq, part, dioff, (int)nitems,
                  accumulate ? 1 : 0);
}
