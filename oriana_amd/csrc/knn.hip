// knn.hip -- exact brute-force k nearest neighbours of query rows among candidate rows (oriana_knn): the assign loop of kmeans.hip
// with the centres replaced by every candidate row and the arg-min by a sorted list per query.  DESIGN.md section 5j.
//
// k_knn_scan   A work-group owns one 64-query tile, staged once in LDS (rowscan.h: stage_tile), and one of S contiguous ranges of
//              the candidates; lane = query.  Its W waves (eight where their lists fit the LDS beside the tile, else four) take
//              the range's 8-candidate steps in turn (wave w: steps w, w + W, ..).  The candidates are wave-uniform: they come
//              through scalar loads from the image of rowscan.h (row_image), 8 candidates x 4 features per step, and f is
//              rowscan.h's chain8.  Every lane keeps its k best (f, index) of the wave's candidates sorted in LDS ([slot][64]: a
//              lane only ever touches its own column) and the k-th best f in a register; a candidate enters the list only when
//              it beats that threshold.  The wave's lists go to the scratch as one partial list per query.
// k_knn_merge  lane = query: a pointer merge of the W S partial lists (and, in merge mode, a copy of the incoming rows) under
//              the total order (f, index); the heads and pointers sit in LDS ([list][64]).
// k_rows_pad   the padded candidate image behind row_image(), for this file and silhouette.hip: the library's one pad kernel.
// No atomics; every list has one writer.  f of a pair is one fixed chain, and the result of a query is the k smallest of a set
// under a total order, so nothing depends on S, on which wave met a candidate, or on how candidates or queries were chunked.
#include "rowscan.h"

namespace oriana {
namespace {

constexpr int KN_W = 4;                   // waves of a work-group: the fewest (oriana_knn_max_neighbors counts their lists) ..
constexpr int KN_W_WIDE = 8;              // .. and where the lists of eight fit the LDS too
constexpr int64_t KN_MAX_LISTS = 64;      // partial lists of a query at most (waves x ranges the candidates are cut into)
constexpr int64_t KN_LDS = 160 * 1024;    // LDS of a CU

inline int64_t kn_lds_bytes(int64_t dp, int64_t k, int64_t W) { return 4 * (dp * RS_LD + 2 * W * k * RS_ROWS); }
inline int64_t kn_waves(int64_t dp, int64_t k) {
    static const bool narrow = [] { const char *e = getenv("ORIANA_KNN_WAVES"); return e && atol(e) == KN_W; }();   // tuning runs
    return !narrow && kn_lds_bytes(dp, k, KN_W_WIDE) <= KN_LDS ? KN_W_WIDE : KN_W;
}

struct KnPlan {
    int64_t dp, W, ntiles, nsteps, S, sps, P;
    int64_t off_pf, off_pi, off_inf, off_ini, total;        // bytes into the scratch (a padded candidate image sits at 0)
};

// sizes in range (nq, n >= 0; d, k >= 1; k within oriana_knn_max_neighbors(d)); direct: no padded image is needed
KnPlan kn_plan(int64_t nq, int64_t n, int64_t d, int64_t k, int64_t blocks, bool direct) {
    KnPlan p;
    p.dp = pad4(d);
    p.W = kn_waves(p.dp, k);
    p.ntiles = (nq + RS_ROWS - 1) / RS_ROWS;
    p.nsteps = (n + RS_CH - 1) / RS_CH;
    int64_t S = two_per_cu(blocks, p.ntiles);
    const int64_t smax = (p.nsteps + p.W - 1) / p.W;        // at least one step per wave
    if (S > smax) S = smax;
    if (S > KN_MAX_LISTS / p.W) S = KN_MAX_LISTS / p.W;
    if (S < 1) S = 1;
    p.S = S;
    p.sps = (p.nsteps + S - 1) / S;
    p.P = n > 0 ? p.W * S : 0;
    const int64_t part = p.ntiles * p.W * S * k * RS_ROWS * 4;
    p.off_pf = direct ? 0 : pad16(n * p.dp * 4);
    p.off_pi = p.off_pf + part;
    p.off_inf = p.off_pi + part;
    p.off_ini = p.off_inf + pad16(nq * k * 4);
    p.total = p.off_ini + pad16(nq * k * 4);
    return p;
}

// the candidates (n, d) as (n, dp) float32, zero where padded
__global__ void __launch_bounds__(256) k_rows_pad(float *__restrict__ img, const float *__restrict__ Y, int64_t ldy, int d, int dp,
                                                  int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int j = (int)(e % dp);
    const int64_t r = e / dp;
    img[e] = j < d ? Y[r * ldy + j] : 0.0f;
}

// (f, c) into the lane's sorted column; ties keep the entries already there in front (their indices are smaller)
__device__ __forceinline__ void kn_insert(float *lf, int *li, int k, float f, int c, float &thr) {
    int s = k - 1;
    while (s > 0) {
        const float g = lf[(s - 1) * RS_ROWS];
        if (!(g > f)) break;
        lf[s * RS_ROWS] = g;
        li[s * RS_ROWS] = li[(s - 1) * RS_ROWS];
        --s;
    }
    lf[s * RS_ROWS] = f;
    li[s * RS_ROWS] = c;
    thr = lf[(k - 1) * RS_ROWS];
}

template <int W>
__global__ void __launch_bounds__(64 * W)
k_knn_scan(const float *__restrict__ Q, int64_t nq, int d, int64_t ldq, const float4 *__restrict__ img, int64_t n, int64_t ldi4, int dp,
           int k, int64_t self_off, int exclude, int y0, float *__restrict__ pf, int32_t *__restrict__ pi, int sps, int nsteps) {
    extern __shared__ float lds[];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    float *tile = lds;
    float *lf = lds + dp * RS_LD + w * k * RS_ROWS + lane;
    int *li = reinterpret_cast<int *>(lds + dp * RS_LD + W * k * RS_ROWS) + w * k * RS_ROWS + lane;

    zero_tile<W>(tile, dp);
    for (int s = 0; s < k; ++s) {
        lf[s * RS_ROWS] = INFINITY;
        li[s * RS_ROWS] = -1;
    }
    __syncthreads();
    const int64_t row0 = (int64_t)blockIdx.x * RS_ROWS;
    stage_tile<W>(tile, Q, nq, d, ldq, row0, w, lane);
    __syncthreads();

    // the candidate this lane skips (its own row), as an index of this call's candidates
    const int64_t sc = self_off + row0 + lane;
    const int self = (exclude && sc >= 0 && sc < n) ? (int)sc : -1;
    const int s_begin = (int)blockIdx.y * sps;                            // (steps are ints: nsteps <= 2^28)
    const int s_end = s_begin + sps < nsteps ? s_begin + sps : nsteps;
    const int dq = dp >> 2;
    const float *tl = tile + lane;
    float thr = INFINITY;

    for (int st = s_begin + w; st < s_end; st += W) {
        const int c0 = st * RS_CH;
        const float4 *row[RS_CH];
        float acc[RS_CH];
        pick_rows8(row, img, ldi4, c0, n);
        chain8(acc, tl, dq, row);
        #pragma unroll
        for (int j = 0; j < RS_CH; ++j)
            if (c0 + j < n && acc[j] < thr && c0 + j != self) kn_insert(lf, li, k, acc[j], y0 + c0 + j, thr);
    }

    // ---- the wave's lists as partial list blockIdx.y * W + w of the tile: [slot][64]
    const int64_t P = (int64_t)gridDim.y * W;
    const int64_t base = (((int64_t)blockIdx.x * P + (int64_t)blockIdx.y * W + w) * k) * RS_ROWS + lane;
    for (int s = 0; s < k; ++s) {
        pf[base + (int64_t)s * RS_ROWS] = lf[s * RS_ROWS];
        pi[base + (int64_t)s * RS_ROWS] = li[s * RS_ROWS];
    }
}

// the k best of P partial lists ([tile][list][slot][64]) and, with `inc`, of the (nq, k) rows (inf, ini), per query, under (f, index)
__global__ void __launch_bounds__(64)
k_knn_merge(int32_t *__restrict__ idx, float *__restrict__ d2, int64_t nq, int k, const float *__restrict__ pf,
            const int32_t *__restrict__ pi, int P, const float *__restrict__ inf, const int32_t *__restrict__ ini, int inc) {
    extern __shared__ float lds[];
    const int lane = (int)threadIdx.x;
    const int L = P + inc;
    float *hf = lds + lane;                                              // head of each list: value, index (-1: exhausted), slot
    int *hi = reinterpret_cast<int *>(lds + L * RS_ROWS) + lane;
    int *hp = reinterpret_cast<int *>(lds + 2 * L * RS_ROWS) + lane;
    const int64_t q = (int64_t)blockIdx.x * RS_ROWS + lane;
    if (q >= nq) return;
    const int64_t pbase = (int64_t)blockIdx.x * P * k * RS_ROWS + lane;
    for (int p = 0; p < L; ++p) {
        const bool part = p < P;
        hf[p * RS_ROWS] = part ? pf[pbase + (int64_t)p * k * RS_ROWS] : inf[q * k];
        hi[p * RS_ROWS] = part ? pi[pbase + (int64_t)p * k * RS_ROWS] : ini[q * k];
        hp[p * RS_ROWS] = 0;
    }
    for (int s = 0; s < k; ++s) {
        float bf = INFINITY;
        int bi = -1, bp = -1;
        for (int p = 0; p < L; ++p) {
            const float f = hf[p * RS_ROWS];
            const int i = hi[p * RS_ROWS];
            if (i >= 0 && (bp < 0 || f < bf || (f == bf && i < bi))) { bf = f; bi = i; bp = p; }
        }
        idx[q * k + s] = bi;
        d2[q * k + s] = bf;
        if (bp < 0) continue;                                            // (every list exhausted: the padding values)
        const int h = hp[bp * RS_ROWS] + 1;
        hp[bp * RS_ROWS] = h;
        if (h < k) {
            hf[bp * RS_ROWS] = bp < P ? pf[pbase + ((int64_t)bp * k + h) * RS_ROWS] : inf[q * k + h];
            hi[bp * RS_ROWS] = bp < P ? pi[pbase + ((int64_t)bp * k + h) * RS_ROWS] : ini[q * k + h];
        } else {
            hi[bp * RS_ROWS] = -1;
        }
    }
}

int kn_check_sizes(int64_t nq, int64_t n, int64_t d, int64_t k, int64_t blocks) {
    if (nq < 0 || n < 0 || d < 1 || k < 1 || blocks < 0) return ORIANA_EINVAL;
    if (k > oriana_knn_max_neighbors(d)) return ORIANA_EKRANGE;
    if (!rows_fit_int(nq, n)) return ORIANA_EINVAL;
    return 0;
}

}  // namespace

int row_image(const float *Y, int64_t n, int64_t ldy, int64_t d, void *scratch, hipStream_t st, RowImage *out) {
    if (direct_image(Y, ldy, d)) {
        *out = {reinterpret_cast<const float4 *>(Y), ldy / 4};
        return 0;
    }
    const int64_t dp = pad4(d), npad = n * dp;
    *out = {static_cast<const float4 *>(scratch), dp / 4};
    return launch(k_rows_pad, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, st, static_cast<float *>(scratch), Y, ldy, (int)d,
                  (int)dp, npad);
}

}  // namespace oriana

using namespace oriana;

extern "C" int64_t oriana_knn_max_neighbors(int64_t d) {
    if (d < 1 || d > RS_MAX_D) return 0;
    return (KN_LDS - 4 * pad4(d) * RS_LD) / (4 * 2 * KN_W * RS_ROWS);
}

extern "C" int64_t oriana_knn_tile_rows(void) { return RS_ROWS; }

extern "C" int64_t oriana_knn_waves(int64_t d, int64_t k) {
    if (d < 1 || k < 1 || k > oriana_knn_max_neighbors(d)) return 0;
    return kn_waves(pad4(d), k);
}

extern "C" int64_t oriana_knn_splits(int64_t nq, int64_t n, int64_t d, int64_t k, int64_t blocks) {
    const int rc = kn_check_sizes(nq, n, d, k, blocks);
    if (rc) return rc;
    return kn_plan(nq, n, d, k, blocks, false).S;
}

extern "C" int64_t oriana_knn_scratch_bytes(int64_t nq, int64_t n, int64_t d, int64_t k, int64_t blocks) {
    const int rc = kn_check_sizes(nq, n, d, k, blocks);
    if (rc) return rc;
    return kn_plan(nq, n, d, k, blocks, false).total;
}

extern "C" int64_t oriana_knn_scratch_bytes_for(int64_t nq, int64_t n, int64_t d, int64_t k, int64_t blocks, const float *Y,
                                                int64_t ldy) {
    const int rc = kn_check_sizes(nq, n, d, k, blocks);
    if (rc == ORIANA_EINVAL || (d >= 1 && ldy < d)) return ORIANA_EINVAL;
    if (rc) return rc;
    return kn_plan(nq, n, d, k, blocks, direct_image(Y, ldy, d)).total;
}

extern "C" int oriana_knn(const float *Q, int64_t nq, int64_t ldq, int64_t q0, const float *Y, int64_t n, int64_t ldy, int64_t y0,
                          int64_t d, int64_t k, int exclude_self, int merge, int32_t *idx, float *d2, void *scratch, int64_t blocks,
                          void *stream) {
    int rc = kn_check_sizes(nq, n, d, k, blocks);
    if (rc == ORIANA_EINVAL) return rc;
    if (d >= 1 && (ldq < d || ldy < d)) return ORIANA_EINVAL;
    if (q0 < 0 || y0 < 0 || q0 > (int64_t)1 << 62) return ORIANA_EINVAL;
    if (rc) return rc;
    if (!idx || !d2 || !scratch || (nq > 0 && !Q) || (n > 0 && !Y)) return ORIANA_EINVAL;
    if (((uintptr_t)scratch & 15) || y0 + n > 0x7fffffffLL) return ORIANA_EINVAL;      // (the indices are int32)
    if (nq == 0 || (n == 0 && merge)) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool direct = direct_image(Y, ldy, d);
    const KnPlan p = kn_plan(nq, n, d, k, blocks, direct);
    char *base = static_cast<char *>(scratch);
    float *pf = reinterpret_cast<float *>(base + p.off_pf);
    int32_t *pi = reinterpret_cast<int32_t *>(base + p.off_pi);
    float *inf = reinterpret_cast<float *>(base + p.off_inf);
    int32_t *ini = reinterpret_cast<int32_t *>(base + p.off_ini);
    if (n > 0) {
        RowImage img;
        rc = row_image(Y, n, ldy, d, base, st, &img);
        if (rc) return rc;
        rc = with_variant<KN_W, KN_W_WIDE>((int)p.W, [&](auto W) {
            return launch(k_knn_scan<W()>, dim3((unsigned)p.ntiles, (unsigned)p.S), dim3(64 * W()), (size_t)kn_lds_bytes(p.dp, k, W()),
                          st, Q, nq, (int)d, ldq, img.rows, n, img.ld4, (int)p.dp, (int)k, q0 - y0,
                          exclude_self ? 1 : 0, (int)y0, pf, pi, (int)p.sps, (int)p.nsteps);
        });
        if (rc) return rc;
    }
    if (merge) {      // the incoming rows are read from a copy: the merge writes idx and d2 in place
        ORIANA_HIP_CHECK(hipMemcpyAsync(inf, d2, (size_t)(nq * k) * 4, hipMemcpyDeviceToDevice, st));
        ORIANA_HIP_CHECK(hipMemcpyAsync(ini, idx, (size_t)(nq * k) * 4, hipMemcpyDeviceToDevice, st));
    }
    const int L = (int)p.P + (merge ? 1 : 0);
    return launch(k_knn_merge, dim3((unsigned)p.ntiles), dim3(64), (size_t)(3 * L * RS_ROWS * 4), st, idx, d2, nq, (int)k, pf, pi,
                  (int)p.P, inf, ini, merge ? 1 : 0);
}
