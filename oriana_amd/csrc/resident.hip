// resident.hip -- [r5] the planning of the resident layout as C host code, and a RESIDENT HANDLE of the C ABI.
//
// What a sweep's kernels depend on beyond the packed records -- the gene order and the dense-gene set of a hybrid layout,
// the column work list, the row split, the splits of the dense-gene kernels -- was Python (oriana_amd/engine.py) through
// round 4: a host in another language could only call the stateless entries (csrc/stateless.hip), which repack X on every
// call.  Here the same decisions are plain C functions over host arrays (oriana_plan_*: no device needed, tested on the
// CPU against a NumPy restatement), engine.py calls them, and oriana_counts_create_* / oriana_zq_*_resident keep a count
// matrix packed across calls for a non-Python host: the reference calls its loop nest once per step() with the same X
// (oriana/models/gap.py:89-94).
#include "pack_nest.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include <new>

#pragma clang fp contract(off)          // the cost model below is checked bit for bit against a NumPy restatement

namespace oriana {

// ---------------------------------------------------------------------------------------------------------------
// kernels of the one-time build
// ---------------------------------------------------------------------------------------------------------------
// per-gene non-zero counts and the number of entries a uint16 block cannot hold (negative, >= 65535, non-integer)
__global__ __launch_bounds__(256) void k_col_stats(const float *__restrict__ X, int64_t rows, int64_t m, int64_t ldx,
                                                   unsigned long long *__restrict__ nnz, unsigned long long *__restrict__ bad) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const int64_t r0 = (int64_t)blockIdx.y * 256, r1 = (r0 + 256 < rows) ? r0 + 256 : rows;
    unsigned long long cn = 0, cb = 0;
    for (int64_t r = r0; r < r1; ++r) {
        const float v = X[r * ldx + j];
        cn += (v != 0.0f) ? 1u : 0u;
        cb += (v < 0.0f || v >= 65535.0f || v != floorf(v)) ? 1u : 0u;
    }
    if (cn) atomicAdd(&nnz[j], cn);
    if (cb) atomicAdd(&bad[j], cb);
}

// out[r, c] = X[r, perm[c]]  (the packer reads the already column-permuted chunk)
__global__ __launch_bounds__(256) void k_gather_cols(float *__restrict__ out, const float *__restrict__ X,
                                                     const int32_t *__restrict__ perm, int64_t rows, int64_t m, int64_t ldx) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= m) return;
    const int64_t src = perm ? (int64_t)perm[c] : c;
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) out[r * m + c] = X[r * ldx + src];     // (gridDim.y <= 65535)
}

// rows [r0, r0 + rows) of a CSR matrix into a zeroed dense chunk: one work-group per row
__global__ __launch_bounds__(256) void k_csr_scatter(float *__restrict__ out, const int64_t *__restrict__ indptr,
                                                     const int32_t *__restrict__ indices, const float *__restrict__ data,
                                                     int64_t e0, int64_t m) {
    const int64_t r = blockIdx.x;
    const int64_t a = indptr[r] - e0, b = indptr[r + 1] - e0;
    for (int64_t e = a + threadIdx.x; e < b; e += 256) atomicAdd(&out[r * m + indices[e]], data[e]);      // (duplicates add up)
}

// longest column-side slice of every tile, in iterations of 64 slots (the cost unit of the column work list)
__global__ __launch_bounds__(256) void k_tile_longest(int32_t *__restrict__ out, const uint32_t *__restrict__ cslice, int64_t nt) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    uint32_t mx = 0;
    for (int s = 0; s < 16; ++s) {
        const uint32_t len = (cslice[t * 17 + s + 1] - cslice[t * 17 + s]) >> 6;
        mx = len > mx ? len : mx;
    }
    out[t] = (int32_t)mx;
}

// w_nz[slot] = D[cell, gene] at every stored entry (row-side slots; the per-entry weights of zigap.py:93-95): what
// oriana_pack_fill gathers while packing, for a matrix D that changes from call to call
__global__ __launch_bounds__(256) void k_gather_nz(oriana_counts cm, const float *__restrict__ D, int64_t ld,
                                                   float *__restrict__ w_nz) {
    const int64_t t = blockIdx.x;
    const int64_t rb = t / cm.ncb, cb = t - rb * cm.ncb;
    const int64_t rbase = cm.roff[t];
    for (int sl = 0; sl < 16; ++sl) {
        const uint32_t s0 = cm.rslice[t * 17 + sl], s1 = cm.rslice[t * 17 + sl + 1];
        for (uint32_t slot = s0 + threadIdx.x; slot < s1; slot += 256) {
            const oriana_rowrec rec = cm.rowrec[rbase + slot];
            float w = 0.0f;
            if (rec.x != 0.f) {
                const int64_t ip = rb * TILE + sl * 16 + (int)(((slot - s0) & 63u) >> 2);
                const int64_t jp = cb * TILE + rec.col;
                const int64_t i = cm.row_perm ? (int64_t)cm.row_perm[ip] : ip;
                const int64_t j = cm.col_perm ? (int64_t)cm.col_perm[jp] : jp;
                w = D[i * ld + j];
            }
            w_nz[rbase + slot] = w;
        }
    }
}

}  // namespace oriana

using namespace oriana;

// ---------------------------------------------------------------------------------------------------------------
// planning (host arrays in, host arrays out; no device)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int64_t oriana_device_cus(void) {
    static const long forced = [] { const char *e = getenv("ORIANA_CUS"); return e ? atol(e) : 0L; }();     // tests, tuning runs
    if (forced > 0) return forced;
    static int cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return 256; }
    if (cached[dev] > 0) return cached[dev];
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) { (void)hipGetLastError(); return 256; }
    cached[dev] = v;
    return v;
}

extern "C" int oriana_plan_gene_order(const int64_t *col_nnz, const int64_t *bad, int64_t m, int64_t n_total,
                                      double dense_density, double min_share, int32_t *order, int64_t *gd_out) {
    if (m < 0 || (m > 0 && (!col_nnz || !order)) || !gd_out || m > 0x7fffffffLL) return ORIANA_EINVAL;
    *gd_out = 0;
    std::vector<int32_t> ord((size_t)m);
    for (int64_t j = 0; j < m; ++j) ord[(size_t)j] = (int32_t)j;
    // decreasing non-zero count, ties in the caller's gene order
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return col_nnz[a] > col_nnz[b]; });
    int64_t gd = 0;
    std::vector<int32_t> cand;
    if (dense_density > 0.0) {
        const double thr = dense_density * (double)(n_total > 1 ? n_total : 1);
        for (int64_t p = 0; p < m; ++p) {
            const int32_t j = ord[(size_t)p];
            if ((double)col_nnz[j] >= thr && (!bad || bad[j] == 0) && col_nnz[j] > 0) cand.push_back(j);
        }
        gd = ((int64_t)cand.size() / 32) * 32;
        if (gd > 0 && min_share > 0.0) {
            double tot = 0.0, got = 0.0;
            for (int64_t j = 0; j < m; ++j) tot += (double)col_nnz[j];
            for (int64_t p = 0; p < gd; ++p) got += (double)col_nnz[cand[(size_t)p]];
            if (!(tot > 0.0) || got < min_share * tot) gd = 0;
        }
    }
    if (gd == 0) {
        for (int64_t p = 0; p < m; ++p) order[p] = ord[(size_t)p];
        return 0;
    }
    std::vector<char> taken((size_t)m, 0);
    for (int64_t p = 0; p < gd; ++p) { order[p] = cand[(size_t)p]; taken[(size_t)cand[(size_t)p]] = 1; }
    int64_t q = gd;
    for (int64_t p = 0; p < m; ++p)
        if (!taken[(size_t)ord[(size_t)p]]) order[q++] = ord[(size_t)p];
    *gd_out = gd;
    return 0;
}

extern "C" int64_t oriana_plan_col_work_capacity(int64_t nrb, int64_t ncb, int64_t width) {
    if (nrb <= 0 || ncb <= 0 || width <= 0) return 0;
    return nrb * ((ncb + width - 1) / width);           // (a column block is cut into at most nrb row ranges)
}

namespace {
struct ColItem { int32_t cb, a, e; };

// one cut of every column block at equal-cost points into about n_items items in all (NumPy's linspace / searchsorted /
// unique, restated)
void col_work_build(const std::vector<std::vector<double>> &cums, int64_t nrb, double total, int64_t n_items, std::vector<ColItem> &out) {
    out.clear();
    double target = total / (double)n_items;
    if (!(target > 1e-9)) target = 1e-9;
    std::vector<int64_t> edges;
    for (size_t cb = 0; cb < cums.size(); ++cb) {
        const std::vector<double> &cum = cums[cb];
        const double last = cum[(size_t)nrb];
        double want = nearbyint(last / target);              // Python's round(): half to even
        if (want < 1.0) want = 1.0;
        if (want > (double)nrb) want = (double)nrb;
        const int64_t nb = (int64_t)want;
        edges.clear();
        edges.push_back(0);
        const double step = last / (double)nb;
        for (int64_t i = 1; i < nb; ++i) {
            const double pt = (double)i * step;
            const int64_t idx = (int64_t)(std::lower_bound(cum.begin(), cum.end(), pt) - cum.begin());
            edges.push_back(idx);
        }
        edges.push_back(nrb);
        std::sort(edges.begin(), edges.end());
        edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
        for (size_t k = 0; k + 1 < edges.size(); ++k)
            if (edges[k + 1] > edges[k]) out.push_back(ColItem{(int32_t)cb, (int32_t)edges[k], (int32_t)edges[k + 1]});
    }
}
}  // namespace

// Work list of the column pass: (column block, first row block, end row block) items of about equal COST, ordered by row band.
// A column block is `width` adjacent column tiles.  Cost of a block's row block = its longest column slice (the work-group
// advances at the pace of its slowest wave; tile_iters [nrb * ncb], iterations of 64 slots) * 1.45 + 3.2 for staging the 256
// factor rows (measured on MI355X, in microseconds).  One 1024-thread group per CU: the pass advances in rounds of `cus` items
// and a partly filled last round costs a whole one, so the list is re-cut until the item count lands just below a multiple
// of `cus` (rounds = 0: the first cut).  target_items = 0: 25-50 tiles per item, between 9 and 36 items per CU.
extern "C" int oriana_plan_col_work(const int32_t *tile_iters, int64_t nrb, int64_t ncb, int64_t width, int64_t cus,
                                    int64_t target_items, int rounds, int sum_price, int32_t *items, int64_t cap,
                                    int64_t *n_items) {
    if (!n_items || nrb < 0 || ncb < 0 || width <= 0 || cus <= 0 || target_items < 0) return ORIANA_EINVAL;
    *n_items = 0;
    if (nrb == 0 || ncb == 0) return 0;
    if (!tile_iters || !items || nrb > 0x7fffffffLL || ncb > 0x7fffffffLL) return ORIANA_EINVAL;
    const int64_t nblk = (ncb + width - 1) / width;
    std::vector<std::vector<double>> cums((size_t)nblk, std::vector<double>((size_t)nrb + 1, 0.0));
    double total = 0.0;
    for (int64_t cb = 0; cb < nblk; ++cb) {
        std::vector<double> &cum = cums[(size_t)cb];
        for (int64_t rb = 0; rb < nrb; ++rb) {
            double nit = 0.0;
            for (int64_t w = 0; w < width; ++w) {
                const int64_t c = cb * width + w;
                const double v = c < ncb ? (double)tile_iters[rb * ncb + c] : 0.0;
                nit = sum_price ? nit + v : (v > nit ? v : nit);
            }
            const double scaled = nit * 1.45;
            const double cost = scaled + 3.2;
            cum[(size_t)rb + 1] = cum[(size_t)rb] + cost;
        }
        total += cum[(size_t)nrb];
    }
    const bool explicit_target = target_items > 0;
    const int64_t nt = nrb * ncb;
    if (!explicit_target) {
        target_items = nt / (50 * width);
        if (target_items < 9 * cus) target_items = 9 * cus;
        if (target_items > 36 * cus) target_items = 36 * cus;
    }
    std::vector<ColItem> cur, trial;
    col_work_build(cums, nrb, total, target_items, cur);
    if (!explicit_target && rounds && (int64_t)cur.size() > cus) {
        const int64_t want = ((int64_t)cur.size() / cus) * cus;
        const int64_t slack = std::max<int64_t>(1, 24 * cus / 256), back = std::max<int64_t>(1, 8 * cus / 256);
        int64_t t = target_items;
        trial = cur;
        for (int it = 0; it < 9; ++it) {
            if (want - slack <= (int64_t)trial.size() && (int64_t)trial.size() <= want) { cur = trial; break; }
            if (it == 8) break;
            const double nxt = nearbyint((double)t * (double)(want - back) / (double)std::max<int64_t>((int64_t)trial.size(), 1));
            t = std::max<int64_t>(cus, (int64_t)nxt);
            col_work_build(cums, nrb, total, t, trial);
        }
    }
    // by row band: the items that run at the same time stage the same factor rows
    std::stable_sort(cur.begin(), cur.end(), [](const ColItem &x, const ColItem &y) {
        const int64_t kx = (int64_t)x.a + x.e, ky = (int64_t)y.a + y.e;
        return kx != ky ? kx < ky : x.cb < y.cb;
    });
    if ((int64_t)cur.size() > cap) return ORIANA_EINVAL;
    for (size_t k = 0; k < cur.size(); ++k) { items[3 * k] = cur[k].cb; items[3 * k + 1] = cur[k].a; items[3 * k + 2] = cur[k].e; }
    *n_items = (int64_t)cur.size();
    return 0;
}

// The planners' inputs from a layout's device tables (include/oriana_hip.h).  gene_tile_cost: the mean iterations of a 16-row slice
// (16 slices of 64 slots) + 2.0 for staging the tile's 256 factor rows, in iterations (flat between 0.5 and 4, DESIGN_HISTORY.md 10 l).
extern "C" int oriana_plan_inputs(const int32_t *tile_rslots, const uint32_t *cslice, int64_t nrb, int64_t ncb,
                                  double *gene_tile_cost, int32_t *tile_iters, void *stream) {
    if (nrb < 0 || ncb < 0 || (gene_tile_cost && !tile_rslots) || (tile_iters && !cslice)) return ORIANA_EINVAL;
    const int64_t nt = nrb * ncb;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> rslots((size_t)(gene_tile_cost ? nt : 0));
    struct Scratch { int32_t *p = nullptr; ~Scratch() { if (p) (void)hipFree(p); } } longest;
    if (!rslots.empty())
        ORIANA_HIP_CHECK(hipMemcpyAsync(rslots.data(), tile_rslots, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, s));
    if (tile_iters && nt > 0) {
        if (hipMalloc((void **)&longest.p, sizeof(int32_t) * nt) != hipSuccess) { (void)hipGetLastError(); return -1000 - (int)hipErrorOutOfMemory; }
        hipLaunchKernelGGL(k_tile_longest, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, longest.p, cslice, nt);
        ORIANA_LAUNCH_CHECK();
        ORIANA_HIP_CHECK(hipMemcpyAsync(tile_iters, longest.p, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, s));
    }
    ORIANA_HIP_CHECK(hipStreamSynchronize(s));
    for (int64_t c = 0; gene_tile_cost && nt > 0 && c < ncb; ++c) {
        double sum = 0.0;
        for (int64_t rb = 0; rb < nrb; ++rb) sum += (double)rslots[(size_t)(rb * ncb + c)];
        gene_tile_cost[c] = sum / (double)nrb / (16.0 * 64.0) + 2.0;
    }
    return 0;
}

// splits of the dense-gene kernels of a hybrid layout: gene ranges of the row kernel (two work-groups per CU at most) and
// cell ranges of the gene-side kernel (four per CU, a multiple of 8 cell tiles)
extern "C" int oriana_plan_dense_splits(int64_t n, int64_t gd, int64_t cus, int64_t *gene_splits, int64_t *cell_splits) {
    if (n < 0 || gd < 0 || gd % 32 != 0 || cus <= 0 || !gene_splits || !cell_splits) return ORIANA_EINVAL;
    const int64_t ngt = gd / 32, nblk = std::max<int64_t>((n + TILE - 1) / TILE, 1);
    *gene_splits = std::max<int64_t>(1, std::min<int64_t>(ngt, (2 * cus + nblk - 1) / nblk));
    const int64_t groups = std::max<int64_t>((ngt + 7) / 8, 1);
    const int64_t per = ((4 * cus + groups - 1) / groups + 7) / 8 * 8;
    *cell_splits = std::max<int64_t>(1, std::min<int64_t>((n + 31) / 32, per));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// the resident handle
// ---------------------------------------------------------------------------------------------------------------
struct oriana_resident {
    int64_t n = 0, m = 0, K = 0, Kp = 0, gd = 0, ms = 0, nrb = 0, ncb = 0, nt = 0, nnz = 0, rslots = 0, cslots = 0;
    int64_t cus = 256, bytes = 0;
    std::vector<void *> allocs;
    // layout
    int32_t *col_perm = nullptr;
    int32_t *tile_nnz = nullptr, *tile_rslots = nullptr, *tile_cslots = nullptr, *tile_flag = nullptr;
    int64_t *roff = nullptr, *coff = nullptr;
    uint32_t *rslice = nullptr, *cslice = nullptr;
    oriana_rowrec *rowrec = nullptr;
    uint8_t *ridx = nullptr;
    uint16_t *dense_x = nullptr;
    oriana_counts cm;
    oriana_dense dn;
    // plans
    oriana_row_split split;
    int32_t *col_work = nullptr;
    int64_t n_col_work = 0, dn_gene_splits = 1, dn_cell_splits = 1;
    // workspace of a call
    float *FU = nullptr, *FV = nullptr, *R = nullptr, *C = nullptr, *s_cs = nullptr, *prep = nullptr;
    float *dn_S = nullptr, *dn_imgV = nullptr, *dn_imgU = nullptr;
    int32_t *dn_flag = nullptr;
    // the ZI / sparse nests (allocated on first use)
    float *w_nz = nullptr, *sw_cs = nullptr, *s_rs = nullptr, *F2 = nullptr, *G2 = nullptr, *C2 = nullptr, *dq = nullptr;
    float *GQ = nullptr;
    // [r6] work list of the dual column pass (one column tile per item) and the caller's declaration about D_hat
    int32_t *col_work1 = nullptr;
    int64_t n_col_work1 = 0;
    int unit_dropout = 0;
};

namespace {

template <typename T>
int dev_alloc(oriana_resident *h, T **p, size_t count, bool zero, hipStream_t s) {
    const size_t bytes = sizeof(T) * (count > 0 ? count : 1);
    void *q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); return -1000 - (int)hipErrorOutOfMemory; }
    h->allocs.push_back(q);
    h->bytes += (int64_t)bytes;
    if (zero && hipMemsetAsync(q, 0, bytes, s) != hipSuccess) return -1000 - (int)hipGetLastError();
    *p = static_cast<T *>(q);
    return 0;
}

void resident_free(oriana_resident *h) {
    if (!h) return;
    for (void *q : h->allocs) (void)hipFree(q);
    delete h;
}

// A source of dense float32 row chunks in the caller's gene order: a dense device matrix (no copy) or CSR host arrays
// (expanded into a device buffer, chunk by chunk)
struct ChunkSource {
    const float *X = nullptr; int64_t ldx = 0;                                   // dense
    const int64_t *indptr = nullptr; const int32_t *indices = nullptr; const float *data = nullptr;   // CSR (host)
    float *buf = nullptr; int64_t *d_indptr = nullptr; int32_t *d_indices = nullptr; float *d_data = nullptr;
    int64_t max_e = 0;
    int64_t m = 0;
    int get(int64_t r0, int64_t rows, const float **out, int64_t *ld, hipStream_t s) {
        if (X) { *out = X + r0 * ldx; *ld = ldx; return 0; }
        const int64_t e0 = indptr[r0], e1 = indptr[r0 + rows];
        if (e1 < e0 || e1 - e0 > max_e) return ORIANA_EINVAL;
        ORIANA_HIP_CHECK(hipMemsetAsync(buf, 0, sizeof(float) * rows * m, s));
        ORIANA_HIP_CHECK(hipMemcpyAsync(d_indptr, indptr + r0, sizeof(int64_t) * (rows + 1), hipMemcpyHostToDevice, s));
        if (e1 > e0) {
            ORIANA_HIP_CHECK(hipMemcpyAsync(d_indices, indices + e0, sizeof(int32_t) * (e1 - e0), hipMemcpyHostToDevice, s));
            ORIANA_HIP_CHECK(hipMemcpyAsync(d_data, data + e0, sizeof(float) * (e1 - e0), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_csr_scatter, dim3((unsigned)rows), dim3(256), 0, s, buf, d_indptr, d_indices, d_data, e0, m);
            ORIANA_LAUNCH_CHECK();
        }
        ORIANA_HIP_CHECK(hipStreamSynchronize(s));          // (the host arrays of the next chunk may be staged by the caller's allocator)
        *out = buf; *ld = m;
        return 0;
    }
};

int resident_build(oriana_resident *h, ChunkSource &src, double dense_density, hipStream_t s) {
    const int64_t n = h->n, m = h->m, K = h->K;
    h->cus = oriana_device_cus();
    // row chunks of about 512 MB, whole row blocks
    int64_t chunk = ((int64_t)(512u << 20) / (m * 4)) / TILE * TILE;
    if (chunk < TILE) chunk = TILE;
    if (chunk > (n + TILE - 1) / TILE * TILE) chunk = (n + TILE - 1) / TILE * TILE;
    if (chunk / TILE > 65535) chunk = (int64_t)65535 * TILE;
    std::vector<void *> scratch;                             // freed at the end of the build
    auto tmp_alloc = [&](void **p, size_t bytes) -> int {
        if (hipMalloc(p, bytes ? bytes : 1) != hipSuccess) { (void)hipGetLastError(); return -1000 - (int)hipErrorOutOfMemory; }
        scratch.push_back(*p);
        return 0;
    };
    struct Cleanup { std::vector<void *> &v; ~Cleanup() { for (void *q : v) (void)hipFree(q); } } cleanup{scratch};
    if (!src.X) {
        int64_t max_e = 0;
        for (int64_t r0 = 0; r0 < n; r0 += chunk) {
            const int64_t r1 = std::min(n, r0 + chunk);
            max_e = std::max(max_e, src.indptr[r1] - src.indptr[r0]);
        }
        src.max_e = max_e;
        ORIANA_TRY(tmp_alloc((void **)&src.buf, sizeof(float) * chunk * m));
        ORIANA_TRY(tmp_alloc((void **)&src.d_indptr, sizeof(int64_t) * (chunk + 1)));
        ORIANA_TRY(tmp_alloc((void **)&src.d_indices, sizeof(int32_t) * std::max<int64_t>(max_e, 1)));
        ORIANA_TRY(tmp_alloc((void **)&src.d_data, sizeof(float) * std::max<int64_t>(max_e, 1)));
    }
    // ---- 1. per-gene statistics -> gene order, dense set
    unsigned long long *d_nnz = nullptr, *d_bad = nullptr;
    ORIANA_TRY(tmp_alloc((void **)&d_nnz, sizeof(unsigned long long) * m));
    ORIANA_TRY(tmp_alloc((void **)&d_bad, sizeof(unsigned long long) * m));
    ORIANA_HIP_CHECK(hipMemsetAsync(d_nnz, 0, sizeof(unsigned long long) * m, s));
    ORIANA_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(unsigned long long) * m, s));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t rows = std::min(n, r0 + chunk) - r0;
        const float *Xc; int64_t ld;
        ORIANA_TRY(src.get(r0, rows, &Xc, &ld, s));
        hipLaunchKernelGGL(k_col_stats, dim3((unsigned)((m + 255) / 256), (unsigned)((rows + 255) / 256)), dim3(256), 0, s, Xc, rows, m, ld, d_nnz, d_bad);
        ORIANA_LAUNCH_CHECK();
    }
    std::vector<int64_t> col_nnz((size_t)m), bad((size_t)m);
    ORIANA_HIP_CHECK(hipMemcpyAsync(col_nnz.data(), d_nnz, sizeof(int64_t) * m, hipMemcpyDeviceToHost, s));
    ORIANA_HIP_CHECK(hipMemcpyAsync(bad.data(), d_bad, sizeof(int64_t) * m, hipMemcpyDeviceToHost, s));
    ORIANA_HIP_CHECK(hipStreamSynchronize(s));
    std::vector<int32_t> order((size_t)m);
    int64_t gd = 0;
    const double dd = (dense_density > 0.0 && oriana_dense_supported(K)) ? dense_density : 0.0;
    ORIANA_TRY(oriana_plan_gene_order(col_nnz.data(), bad.data(), m, n, dd, 0.0, order.data(), &gd));
    h->gd = gd; h->ms = m - gd;
    h->nrb = (n + TILE - 1) / TILE; h->ncb = (h->ms + TILE - 1) / TILE; h->nt = h->nrb * h->ncb;
    ORIANA_TRY(dev_alloc(h, &h->col_perm, (size_t)m, false, s));
    ORIANA_HIP_CHECK(hipMemcpyAsync(h->col_perm, order.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice, s));
    // ---- 2. tile tables
    const size_t nt1 = (size_t)std::max<int64_t>(h->nt, 1);
    ORIANA_TRY(dev_alloc(h, &h->tile_nnz, nt1, true, s));
    ORIANA_TRY(dev_alloc(h, &h->tile_rslots, nt1, true, s));
    ORIANA_TRY(dev_alloc(h, &h->tile_cslots, nt1, true, s));
    ORIANA_TRY(dev_alloc(h, &h->tile_flag, nt1, true, s));
    ORIANA_TRY(dev_alloc(h, &h->rslice, nt1 * 17, true, s));
    ORIANA_TRY(dev_alloc(h, &h->cslice, nt1 * 17, true, s));
    ORIANA_TRY(dev_alloc(h, &h->roff, nt1 + 1, true, s));
    ORIANA_TRY(dev_alloc(h, &h->coff, nt1 + 1, true, s));
    // ---- 3. records and, beside them, the dense block: the packing sequence of pack_nest.h over chunks in the packed gene order
    const int64_t nct = h->nrb * 8, ngt = gd / 32;
    if (gd > 0) ORIANA_TRY(dev_alloc(h, &h->dense_x, (size_t)(nct * ngt * 1024), true, s));
    float *perm_buf = nullptr;
    ORIANA_TRY(tmp_alloc((void **)&perm_buf, sizeof(float) * chunk * m));
    auto permuted = [&](int64_t r0, int64_t rows, bool fill, const float **out, int64_t *ld_out) -> int {
        const float *Xc; int64_t ld;
        ORIANA_TRY(src.get(r0, rows, &Xc, &ld, s));
        hipLaunchKernelGGL(k_gather_cols, dim3((unsigned)((m + 255) / 256), (unsigned)std::min<int64_t>(rows, 65535)), dim3(256), 0, s, perm_buf, Xc,
                           h->col_perm, rows, m, ld);
        ORIANA_LAUNCH_CHECK();
        if (fill && gd > 0) ORIANA_TRY(oriana_dense_pack(perm_buf, 0, rows, gd, m, r0 / 32, h->dense_x, s));
        *out = perm_buf + gd; *ld_out = m;
        return 0;
    };
    auto place = [&](int64_t rslots, int64_t cslots, oriana_rowrec **rowrec, uint8_t **ridx, float **) -> int {
        h->rslots = rslots; h->cslots = cslots;
        ORIANA_TRY(dev_alloc(h, &h->rowrec, (size_t)std::max<int64_t>(rslots, 1), true, s));
        ORIANA_TRY(dev_alloc(h, &h->ridx, (size_t)std::max<int64_t>(cslots, 1), true, s));
        *rowrec = h->rowrec; *ridx = h->ridx;
        return 0;
    };
    const PackTables t{h->tile_nnz, h->tile_rslots, h->tile_cslots, h->roff, h->coff, h->rslice, h->cslice};
    oriana_counts &cm = h->cm;
    int64_t nnz_dense = 0;                                   // (the per-gene counts of step 1 are counts of the same float32 values)
    for (int64_t p = 0; p < m; ++p) h->nnz += col_nnz[(size_t)p];
    for (int64_t p = 0; p < gd; ++p) nnz_dense += col_nnz[(size_t)order[(size_t)p]];
    ORIANA_TRY(pack_sliced(&cm, n, h->ms, chunk, t, h->col_perm + gd, nullptr, 0, h->nnz - nnz_dense, permuted, place, s));
    h->dn.n = n; h->dn.gd = gd; h->dn.nct = nct; h->dn.x = h->dense_x;
    // ---- 4. plans: row split (equal-cost gene ranges), column work list, dense-gene splits
    h->split.nfull = (int32_t)h->nrb; h->split.parts = 1; h->split.edge[0] = 0; h->split.edge[1] = (int32_t)h->ncb;
    if (h->nt > 0) {
        std::vector<double> tile_cost((size_t)h->ncb, 0.0);
        std::vector<int32_t> longest((size_t)h->nt);
        ORIANA_TRY(oriana_plan_inputs(h->tile_rslots, h->cslice, h->nrb, h->ncb, tile_cost.data(), longest.data(), s));
        ORIANA_TRY(oriana_row_pass_plan_cus(&cm, K, tile_cost.data(), h->cus, &h->split));
        const int64_t width = std::max<int64_t>(oriana_col_block_tiles(K), 1);
        auto col_work = [&](int64_t w, int32_t **list, int64_t *count) -> int {
            const int64_t cap = oriana_plan_col_work_capacity(h->nrb, h->ncb, w);
            std::vector<int32_t> items((size_t)cap * 3);
            ORIANA_TRY(oriana_plan_col_work(longest.data(), h->nrb, h->ncb, w, h->cus, 0, 1, 0, items.data(), cap, count));
            ORIANA_TRY(dev_alloc(h, list, (size_t)std::max<int64_t>(*count * 3, 1), false, s));
            ORIANA_HIP_CHECK(hipMemcpyAsync(*list, items.data(), sizeof(int32_t) * *count * 3, hipMemcpyHostToDevice, s));
            ORIANA_HIP_CHECK(hipStreamSynchronize(s));
            return 0;
        };
        if (h->cslots > 0) {
            ORIANA_TRY(col_work(width, &h->col_work, &h->n_col_work));
            // the dual column pass of the sparse nests (two factor images per tile: one column tile per item)
            if (width == 1) { h->col_work1 = h->col_work; h->n_col_work1 = h->n_col_work; }
            else ORIANA_TRY(col_work(1, &h->col_work1, &h->n_col_work1));
        }
    }
    if (gd > 0) ORIANA_TRY(oriana_plan_dense_splits(n, gd, h->cus, &h->dn_gene_splits, &h->dn_cell_splits));
    // ---- 5. workspace of a call
    const int64_t Kp = h->Kp;
    ORIANA_TRY(dev_alloc(h, &h->FU, (size_t)(std::max<int64_t>(n, 1) * Kp), true, s));
    ORIANA_TRY(dev_alloc(h, &h->FV, (size_t)(std::max<int64_t>(m, 1) * Kp), true, s));
    // (slabs 1.. of a last-round split hold the rows of the split row blocks only)
    ORIANA_TRY(dev_alloc(h, &h->R, (size_t)(zq_r_rows(n, &h->split) * Kp), true, s));
    ORIANA_TRY(dev_alloc(h, &h->C, (size_t)(std::max<int64_t>(m, 1) * Kp), true, s));
    ORIANA_TRY(dev_alloc(h, &h->s_cs, (size_t)std::max<int64_t>(h->cslots, 1), true, s));      // (padding slots must stay 0)
    ORIANA_TRY(dev_alloc(h, &h->prep, (size_t)(oriana_prep_scratch_bytes() / 4), true, s));
    if (gd > 0) {
        ORIANA_TRY(dev_alloc(h, &h->dn_S, (size_t)(nct * ngt * 1024), true, s));
        ORIANA_TRY(dev_alloc(h, &h->dn_flag, (size_t)std::max<int64_t>(nct * ngt, 1), true, s));
        ORIANA_TRY(dev_alloc(h, &h->dn_imgV, (size_t)(ngt * oriana_dense_image_pieces(K, 0) * 4), false, s));
        ORIANA_TRY(dev_alloc(h, &h->dn_imgU, (size_t)(std::max<int64_t>((n + 31) / 32, 1) * oriana_dense_image_pieces(K, 1) * 4), false, s));
    }
    ORIANA_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

int resident_create(oriana_resident **out, ChunkSource &src, int64_t n, int64_t m, int64_t K, double dense_density, void *stream) {
    if (!out) return ORIANA_EINVAL;
    *out = nullptr;
    if (n <= 0 || m <= 0 || K <= 0 || m > 0x7fffffffLL) return ORIANA_EINVAL;
    const int64_t Kp = oriana_kpad(K);
    if (Kp == 0) return ORIANA_EKRANGE;
    oriana_resident *h = new (std::nothrow) oriana_resident();
    if (!h) return ORIANA_EINVAL;
    h->n = n; h->m = m; h->K = K; h->Kp = Kp;
    src.m = m;
    const int rc = resident_build(h, src, dense_density, (hipStream_t)stream);
    if (rc) { resident_free(h); return rc; }
    *out = h;
    return 0;
}

}  // namespace

extern "C" int oriana_counts_create_dense_f32(oriana_resident **out, const float *X, int64_t n, int64_t m, int64_t ldx, int64_t K,
                                              double dense_density, void *stream) {
    if (!X || ldx < m) return ORIANA_EINVAL;
    ChunkSource src;
    src.X = X; src.ldx = ldx;
    return resident_create(out, src, n, m, K, dense_density, stream);
}

extern "C" int oriana_counts_create_csr(oriana_resident **out, const int64_t *indptr, const int32_t *indices, const float *data,
                                        int64_t n, int64_t m, int64_t K, double dense_density, void *stream) {
    if (!indptr || (n > 0 && indptr[n] > indptr[0] && (!indices || !data))) return ORIANA_EINVAL;
    for (int64_t r = 0; r < n; ++r)
        if (indptr[r + 1] < indptr[r]) return ORIANA_EINVAL;          // (a non-monotone indptr would send the scatter kernel out of bounds)
    for (int64_t e = indptr[0]; n > 0 && e < indptr[n]; ++e)
        if (indices[e] < 0 || indices[e] >= m) return ORIANA_EINVAL;
    ChunkSource src;
    src.indptr = indptr; src.indices = indices; src.data = data;
    return resident_create(out, src, n, m, K, dense_density, stream);
}

extern "C" int oriana_counts_destroy(oriana_resident *h) {
    if (!h) return 0;
    (void)hipDeviceSynchronize();
    resident_free(h);
    return 0;
}

extern "C" int oriana_counts_info(const oriana_resident *h, int64_t *info, int64_t len) {
    // {n, m, K, Kp, non-zeros, dense genes, row-side slots, column-side slots, resident bytes, column work items, row-split
    //  parts, first split row block, CUs planned for}
    if (!h || !info || len < 13) return ORIANA_EINVAL;
    const int64_t v[13] = {h->n, h->m, h->K, h->Kp, h->nnz, h->gd, h->rslots, h->cslots, h->bytes, h->n_col_work, h->split.parts,
                           h->split.nfull, h->cus};
    memcpy(info, v, sizeof(v));
    return 0;
}

// A view of the handle's buffers for zq_run (zq_nest.h): the two-image kernels and the dynamic den threshold, as engine.zq runs
// the nests for the model classes; the variant extras are whatever the handle holds at this point.
static ZqView resident_view(const oriana_resident *h) {
    ZqView v;
    v.cm = &h->cm; v.dn = &h->dn; v.n = h->n; v.m = h->m; v.K = h->K; v.Kp = h->Kp; v.gd = h->gd;
    v.FU = h->FU; v.FV = h->FV; v.R = h->R; v.C = h->C; v.s_cs = h->s_cs; v.prep = h->prep; v.tile_flag = h->tile_flag;
    v.F2 = h->F2; v.G2 = h->G2; v.C2 = h->C2; v.GQ = h->GQ; v.s_rs = h->s_rs;
    v.dn_S = h->dn_S; v.dn_flag = h->dn_flag; v.dn_imgV = h->dn_imgV; v.dn_imgU = h->dn_imgU;
    v.dn_gene_splits = h->dn_gene_splits; v.dn_cell_splits = h->dn_cell_splits;
    v.split = &h->split; v.col_perm = h->col_perm;
    v.col_work = h->col_work; v.n_col_work = h->n_col_work; v.col_work1 = h->col_work1; v.n_col_work1 = h->n_col_work1;
    v.dynamic_den = true; v.clear_outputs = true; v.two_image = true;
    return v;
}

// The pCMF nest on the resident layout (sliced or hybrid): what engine.zq_gap runs for the model classes.
extern "C" int oriana_zq_gap_resident(oriana_resident *h, float *Z_i, float *Z_j, const float *log_U_hat, const float *log_V_hat,
                                      void *stream) {
    if (!h || !Z_i || !Z_j || !log_U_hat || !log_V_hat) return ORIANA_EINVAL;
    return zq_run(resident_view(h), Z_i, Z_j, nullptr, log_U_hat, log_V_hat, nullptr, nullptr, nullptr, stream);
}

// [r6] The ZI / sparse nests WITHOUT per-entry weights -- D_hat == 1 at every stored entry, which is what every D_hat the
// reference's own models hand to these nests looks like (zigap.py:135 sets p_d = 1 - 1e-10 at the non-zero counts, bernoulli.py:45
// casts it to float32 = 1) and what the caller declares with oriana_counts_declare_unit_dropout -- as engine.zq runs them for the
// model classes: sliced or hybrid layout; Kp <= 64: the sparse nests' S_hat-weighted row sums out of the fused two-image row
// pass and both per-gene sums out of one dual column pass; above: den-only row pass + second row product + two column passes.
// D_hat itself is read for the D_hat[i, k] weights of zigap.py:94 only (dq).  Zlog may be NULL (the reference's caller never
// reads its third output, zigap.py:105-112): the log sums are then skipped.
static int zq_unit_resident(oriana_resident *h, float *Zi, float *Zj, float *Zlog, const float *log_U_hat, const float *log_V_hat,
                            const float *S_tilde, const float *S_hat, const float *D_hat, int quirk, void *stream) {
    const int64_t n = h->n, m = h->m, K = h->K, Kp = h->Kp;
    hipStream_t s = (hipStream_t)stream;
    const bool sparse = S_hat != nullptr;
    // (every buffer of a group is tested on its own: a failed allocation must not leave a later call with a NULL sibling)
    if (sparse && !h->F2) ORIANA_TRY(dev_alloc(h, &h->F2, (size_t)(m * Kp), true, s));
    if (Zlog && !h->G2) ORIANA_TRY(dev_alloc(h, &h->G2, (size_t)(n * Kp), true, s));
    if (Zlog && !h->C2) ORIANA_TRY(dev_alloc(h, &h->C2, (size_t)(m * Kp), true, s));
    if (quirk && !h->dq) ORIANA_TRY(dev_alloc(h, &h->dq, (size_t)(n * K), true, s));
    if (quirk && !h->GQ) ORIANA_TRY(dev_alloc(h, &h->GQ, (size_t)(n * Kp), true, s));
    // (the row-side copy of s for the second row product: the fused form, Kp <= 64, never needs it)
    if (sparse && Kp > 64 && (h->ms > 0 || h->gd == 0) && !h->s_rs)
        ORIANA_TRY(dev_alloc(h, &h->s_rs, (size_t)std::max<int64_t>(h->rslots, 1), true, s));
    ZqView v = resident_view(h);
    v.dq = quirk ? h->dq : nullptr;
    return zq_run(v, Zi, Zj, Zlog, log_U_hat, log_V_hat, S_tilde, S_hat, quirk ? D_hat : nullptr, stream);
}

// The ZI / sparse nests with a GENERAL D_hat (any weight at the stored entries) on a resident SLICED layout: the kernel sequence
// of the stateless entries (stateless.hip: zq_dense) without the packing; D_hat is gathered at the stored entries on every call.
// The dense-gene kernels of a hybrid layout carry no per-entry weights: a hybrid handle serves these nests under the unit
// declaration (above) only.
static int zq_variant_resident(oriana_resident *h, float *Zi, float *Zj, float *Zlog, const float *log_U_hat, const float *log_V_hat,
                               const float *S_tilde, const float *S_hat, const float *D_hat, int quirk, void *stream) {
    if (!h || !Zi || !Zj || !log_U_hat || !log_V_hat) return ORIANA_EINVAL;
    if ((S_tilde == nullptr) != (S_hat == nullptr)) return ORIANA_EINVAL;
    const int64_t n = h->n, m = h->m, K = h->K, Kp = h->Kp;
    if (quirk && (!D_hat || K > m)) return ORIANA_EQUIRK;
    if (!D_hat || h->unit_dropout)
        return zq_unit_resident(h, Zi, Zj, Zlog, log_U_hat, log_V_hat, S_tilde, S_hat, D_hat, quirk, stream);
    if (h->gd > 0) return ORIANA_EUNIT;
    hipStream_t s = (hipStream_t)stream;
    const bool sparse = S_hat != nullptr;
    const size_t rs1 = (size_t)std::max<int64_t>(h->rslots, 1), cs1 = (size_t)std::max<int64_t>(h->cslots, 1);
    if (!h->w_nz) ORIANA_TRY(dev_alloc(h, &h->w_nz, rs1, true, s));
    if (!h->sw_cs) ORIANA_TRY(dev_alloc(h, &h->sw_cs, cs1, true, s));
    if (sparse && !h->s_rs) ORIANA_TRY(dev_alloc(h, &h->s_rs, rs1, true, s));
    if (sparse && !h->F2) ORIANA_TRY(dev_alloc(h, &h->F2, (size_t)(m * Kp), true, s));
    if ((Zlog || quirk) && !h->G2) ORIANA_TRY(dev_alloc(h, &h->G2, (size_t)(n * Kp), true, s));
    if (Zlog && !h->C2) ORIANA_TRY(dev_alloc(h, &h->C2, (size_t)(m * Kp), true, s));
    if (quirk && !h->dq) ORIANA_TRY(dev_alloc(h, &h->dq, (size_t)(n * K), true, s));
    if (h->nt > 0) {
        hipLaunchKernelGGL(k_gather_nz, dim3((unsigned)h->nt), dim3(256), 0, s, h->cm, D_hat, m, h->w_nz);
        ORIANA_LAUNCH_CHECK();
    }
    // (the weighted kernels have no two-image form: the sequence of the stateless entries, FU * dq and the centred factor
    //  one after the other in G2)
    ZqView v = resident_view(h);
    v.w_nz = h->w_nz; v.sw_cs = h->sw_cs; v.dq = quirk ? h->dq : nullptr; v.GQ = h->G2;
    v.two_image = false; v.col_work1 = nullptr; v.n_col_work1 = 0;
    return zq_run(v, Zi, Zj, Zlog, log_U_hat, log_V_hat, S_tilde, S_hat, quirk ? D_hat : nullptr, stream);
}

extern "C" int oriana_counts_declare_unit_dropout(oriana_resident *h, int on) {
    if (!h) return ORIANA_EINVAL;
    h->unit_dropout = on ? 1 : 0;
    return 0;
}

extern "C" int oriana_zq_zigap_resident(oriana_resident *h, float *DZ_hat_i, float *DZ_hat_j, float *DZ_exp_logsum_hat,
                                        const float *log_U_hat, const float *log_V_hat, const float *D_hat, int reference_quirks,
                                        void *stream) {
    if (!D_hat) return ORIANA_EINVAL;
    return zq_variant_resident(h, DZ_hat_i, DZ_hat_j, DZ_exp_logsum_hat, log_U_hat, log_V_hat, nullptr, nullptr, D_hat,
                               reference_quirks ? 1 : 0, stream);
}

extern "C" int oriana_zq_sparse_gap_resident(oriana_resident *h, float *SZ_hat_i, float *Z_hat_j, float *Z_exp_logsum_hat,
                                             const float *log_U_hat, const float *log_V_hat, const float *S_tilde, const float *S_hat,
                                             void *stream) {
    if (!S_tilde || !S_hat || !Z_exp_logsum_hat) return ORIANA_EINVAL;
    return zq_variant_resident(h, SZ_hat_i, Z_hat_j, Z_exp_logsum_hat, log_U_hat, log_V_hat, S_tilde, S_hat, nullptr, 0, stream);
}

extern "C" int oriana_zq_sparse_zigap_resident(oriana_resident *h, float *DSZ_hat, float *DZ_hat, float *DZ_exp_logsum_hat,
                                               const float *log_U_hat, const float *log_V_hat, const float *S_tilde, const float *S_hat,
                                               const float *D_hat, void *stream) {
    if (!S_tilde || !S_hat || !D_hat || !DZ_exp_logsum_hat) return ORIANA_EINVAL;
    return zq_variant_resident(h, DSZ_hat, DZ_hat, DZ_exp_logsum_hat, log_U_hat, log_V_hat, S_tilde, S_hat, D_hat, 0, stream);
}
