// dense_tiles.h -- pieces shared by the matrix-core kernels over dense 32 x 32 tiles (dense_pass.hip: the dense genes of
// pCMF's responsibility pass, Kp <= 100; dense_zi.hip: the D update and D_hat^T U_hat of the ZI models for the widths
// zi_candidate below gives them): bf16 x 3 splits, the six-product macro, accumulator geometry, operand image layout, LDS-DMA
// copies; and, host side, the (KC, TAIL) dispatcher, the rule that says which kernel family serves which ZI product, and
// pick_splits with its two rules (SplitRule): into how many ranges dense_f32.hip and dense_zi.hip cut an axis.
#pragma once
#include "launch.h"
#include <utility>

namespace oriana {
namespace dn {

typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef uint32_t u4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f16v mfma_b16(u4v a, u4v b, f16v c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), c, 0, 0, 0);
}

// two floats -> their (hi, mid, lo) bf16 parts, each pair packed in one dword (x0 in the low half)
__device__ __forceinline__ void split2(float x0, float x1, uint32_t &hi, uint32_t &mid, uint32_t &lo) {
    const uint32_t b0 = __float_as_uint(x0), b1 = __float_as_uint(x1);
    const float r0 = x0 - __uint_as_float(b0 & 0xFFFF0000u), r1 = x1 - __uint_as_float(b1 & 0xFFFF0000u);
    const uint32_t c0 = __float_as_uint(r0), c1 = __float_as_uint(r1);
    const float s0 = r0 - __uint_as_float(c0 & 0xFFFF0000u), s1 = r1 - __uint_as_float(c1 & 0xFFFF0000u);
    hi = __builtin_amdgcn_perm(b1, b0, 0x07060302u);
    mid = __builtin_amdgcn_perm(c1, c0, 0x07060302u);
    lo = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
}

__device__ __forceinline__ void split8(const float (&x)[8], u4v (&o)[3]) {
#pragma unroll
    for (int w2 = 0; w2 < 4; ++w2) {
        uint32_t a, b, c2;
        split2(x[2 * w2], x[2 * w2 + 1], a, b, c2);
        o[0][w2] = a; o[1][w2] = b; o[2][w2] = c2;
    }
}

// the six cross products, small terms first
#define ORIANA_DN_MF6(ACC, A, B)                                                                       \
    do {                                                                                               \
        ACC = mfma_b16(A[2], B[0], ACC); ACC = mfma_b16(A[0], B[2], ACC); ACC = mfma_b16(A[1], B[1], ACC); \
        ACC = mfma_b16(A[1], B[0], ACC); ACC = mfma_b16(A[0], B[1], ACC); ACC = mfma_b16(A[0], B[0], ACC); \
    } while (0)

// row of the accumulator register v in lane half h (v_mfma_f32_32x32x*: D reg v = [8 (v / 4) + 4 h + v % 4][lane & 31])
__device__ __forceinline__ int acc_row(int v, int h) { return 8 * (v >> 2) + 4 * h + (v & 3); }

constexpr int TS = 36;            // row stride of the transpose buffer (floats): 16-byte aligned rows
constexpr int NW = 8;             // waves per work-group

// The rate-only form of the D update (oriana_zi_foldin_rate, template flag RATE of the three kernel families): some cell of
// [i0, i0 + CELLS) is active -- the same answer in every lane of every wave of the work-group, which returns at its top on
// `false`.  active == NULL: every cell counts as active.
template <int CELLS>
__device__ __forceinline__ bool any_active(const uint8_t *__restrict__ active, int64_t i0, int64_t n, int lane) {
    if (!active) return true;
    bool a = false;
#pragma unroll
    for (int o = 0; o < CELLS; o += 64) {
        const int64_t i = i0 + o + lane;
        a = a || (i < n && active[i] != 0);
    }
    return __ballot(a) != 0ull;
}
__device__ __forceinline__ bool cell_active(const uint8_t *__restrict__ active, int64_t i, int64_t n) {
    return i < n && (!active || active[i] != 0);
}

// Operand images, in 16-byte pieces [..][split][lane]: a wave-wide copy of 64 consecutive pieces is one LDS-DMA
// instruction (global_load_lds_dwordx4 writes lane x 16 bytes from a wave-uniform base).
//   first image  (A operand of den^T = FV FU^T)   [k chunk][split][lane = 32 G' + g]: F[g][16 kc + 8 G' .. + 7]
//   second image (B operand of the accumulation)  [n tile][instruction q][split][lane = 32 hh + cc]:
//                F[acc_row(8 q + e, hh)][32 nt + cc], e = 0..7 -- the rows in the order the accumulator registers of
//                the first product hold them
//   tail         32 rows x float4 (factors 16 KC .. 16 KC + 3), plain float32; then the same values as
//                [lane half][tail factor][16 rows in accumulator order]: the B operand of the 4 x 4 x 1 float32 instructions
//                that accumulate the tail factors (lane l = 4 b + j of block b supplies B[b][j])
template <int KC, int TAIL>
struct Cfg {
    static constexpr int NT = (KC + 1) / 2;
    static constexpr int P1 = KC * 3 * 64;
    static constexpr int P2 = NT * 2 * 3 * 64;
    static constexpr int PT = TAIL ? 64 : 0;
    static constexpr int PV_RAW = P1 + P2 + PT;                          // gene side: both images + tail
    static constexpr int PU_RAW = P2 + PT;                               // cell side: second image + tail
    static constexpr int PV = (PV_RAW + NW * 64 - 1) / (NW * 64) * (NW * 64);   // every wave copies the same number of pieces
    // [r6] the gene-side copy of dn::k_zi_row: always two 64-piece slots of padding behind the images (the tile's non-zero flags
    // and logits ride there; KC = 4 without tail had none)
    static constexpr int PVZ = (PV_RAW + 2 * 64 + NW * 64 - 1) / (NW * 64) * (NW * 64);
    static constexpr int PU = (PU_RAW + NW * 64 - 1) / (NW * 64) * (NW * 64);
    static constexpr int KM = 16 * KC;                                    // factors on the matrix core
    static constexpr int kc = KC, tl = TAIL, KP = 16 * KC + 4 * TAIL;
};

// LDS-DMA copy of one image (P pieces, a multiple of 8 x 64) by the 8 waves of a work-group
template <int P>
__device__ __forceinline__ void image_dma(const u4v *__restrict__ src, u4v *dst_lds, int wave, int lane) {
#pragma unroll
    for (int p = 0; p < P / (NW * 64); ++p) {
        const int piece = (p * NW + wave) * 64;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + piece + lane),
                                         (__attribute__((address_space(3))) void *)(dst_lds + piece), 16, 0, 0);
    }
}


// ------------------------------------------------------------------------------------------
// host side: padded width -> (KC, TAIL) -> template arguments
// ------------------------------------------------------------------------------------------
// Kp = 16 KC + 4 TAIL (oriana_kpad: 16 t, or 16 t + 4 up to 100); {0, 0} for a width that has no such form
struct KcTl { int kc, tl; };
constexpr KcTl kc_tail(int64_t Kp) {
    return (Kp > 0 && (Kp % 16 == 0 || Kp % 16 == 4)) ? KcTl{(int)(Kp / 16), Kp % 16 == 4 ? 1 : 0} : KcTl{0, 0};
}

// run-time (kc, tl) -> f(Cfg<KC, TAIL>{}) for KC_MIN <= KC <= KC_MAX, ORIANA_EKRANGE outside (with_variant's form)
template <int KC_MIN, typename F, int... I>
static int with_cfg_seq(KcTl c, F &&f, std::integer_sequence<int, I...>) {
    int rc = ORIANA_EKRANGE;
    (void)((c.kc == KC_MIN + I / 2 && c.tl == I % 2 && ((rc = f(Cfg<KC_MIN + I / 2, I % 2>{})), true)) || ...);
    return rc;
}
template <int KC_MIN, int KC_MAX, typename F>
static int with_cfg(KcTl c, F &&f) {
    return with_cfg_seq<KC_MIN>(c, f, std::make_integer_sequence<int, 2 * (KC_MAX - KC_MIN + 1)>{});
}

// the dense genes (dense_pass.hip): every Kp <= 100  (Kp = 112: three image buffers exceed LDS)
constexpr int DN_KC_MIN = 1, DN_KC_MAX = 6;

// ------------------------------------------------------------------------------------------
// Which kernel family serves which dense product of a ZI sweep.  zi_candidate is the whole rule: the two C entries
// (dense_f32.hip) run the first candidate whose run-time preconditions hold, the launchers name a kernel template only under
// `if constexpr` on its answers (what is compiled is what can be launched), the scratch-size entries ask it too, and DESIGN.md
// section 0 shows it as a table.
// ------------------------------------------------------------------------------------------
enum class ZiOp { update, dt };     // the D update with the next sweep's D_hat V_hat;  out += D_hat^T W
enum class ZiFam {
    none,       // no kernel: ORIANA_EKRANGE
    tiles,      // dense_zi.hip: k_zi_row / k_zi_col<KC = a, TAIL = b>, bf16 x 3 over 32 x 32 tiles with LDS-DMA
    b16,        // dense_f32.hip: k_dropout_sweep_b16<NT = a, KC = b> / k_dt_times_factor_b16<NT = a>
    f32         // dense_f32.hip: k_dropout_sweep<NT = a> / k_dt_times_factor_f32<NT = a, GQ = b>, the float32 matrix instruction
};
struct ZiCand { ZiFam fam; int a, b; };
constexpr int ZI_MAX_CAND = 3;
constexpr int ZI_KP_MAX = 128;      // the widest product of either entry; ZI_KC_* = the (KC, TAIL) range dense_zi.hip compiles from
constexpr int ZI_KC_MIN = 3, ZI_KC_MAX = 6;

// candidate i (in the order they are tried) for the padded width kp under `arithmetic`; none from the end of the list on
constexpr ZiCand zi_candidate(ZiOp op, int kp, int arithmetic, int i) {
    ZiCand list[ZI_MAX_CAND + 1] = {};
    int n = 0;
    const KcTl t = kc_tail(kp);
    if (t.kc == 0 || kp > ZI_KP_MAX || i < 0 || i >= ZI_MAX_CAND) return ZiCand{ZiFam::none, 0, 0};
    if (arithmetic == ORIANA_MATRIX_BF16X3) {
        // tiles from K = 33 (Kp = 36) to Kp = 100.  Measured at 100k x 20k against the b16 kernels (tools/perf_zi_per_k.py, round 6's
        // build): D update 3.37 against 4.11 ms at K = 48, 3.65 against 4.00 ms at K = 50, 3.72 against 4.11 ms at K = 64; D^T U 1.82
        // against 2.00 ms at K = 48 but 2.06 against 1.98 ms at K = 50 WITH the tail factors' 4 x 4 x 1 instructions: below 65 the
        // transposed product takes the next whole chunk instead.
        if (kp >= 36 && kp <= 100) {
            if (op == ZiOp::update) {
                // Kp = 48 .. 100 (k_zi_row has no KC = 2: Kp = 36 goes on to b16).  [r6] Kp = 64 (K = 53 .. 64) too: with room for the
                // flag / logit pieces behind the images (Cfg::PVZ) and the copies issued at the top of the tile, k_zi_row<4, 0> takes
                // 3.68 ms where the b16 kernel takes 4.11 (K = 49 .. 52 stays on <3, 1> with the tail riding in the last factor tile:
                // 3.65 against 3.72 ms zero-padded to four chunks)
                if (t.kc >= ZI_KC_MIN) list[n++] = ZiCand{ZiFam::tiles, t.kc, t.tl};
            } else if (t.tl && t.kc <= 3) {
                // [r6] D_hat^T W below K = 65: Kp = 36 and 52 (K = 50: configs[2]) take the NEXT whole chunk of 16 with zero-padded
                // factors instead of the tail of four -- k_zi_col<4, 0> 1.50 ms against 1.67 ms for k_dt_times_factor_b16 inside the
                // configs[2] sweep (the D update itself is faster WITH the tail: 3.49 against 3.94 ms; profiles/r06_zi_k52_ab.txt)
                list[n++] = ZiCand{ZiFam::tiles, t.kc + 1, 0};
            } else {
                list[n++] = ZiCand{ZiFam::tiles, t.kc, t.tl};
            }
        }
        if (kp <= 64) {             // three-way splits on v_mfma_f32_32x32x16_bf16: KC chunks of 16 factors, NT tiles of 32
            const int kc = (kp + 15) / 16;
            list[n++] = op == ZiOp::update ? ZiCand{ZiFam::b16, (kc + 1) / 2, kc} : ZiCand{ZiFam::b16, kp <= 32 ? 1 : 2, 0};
        }
    }
    {                               // ORIANA_MATRIX_F32, and what bf16 x 3 leaves: NT tiles of 32 factors; GQ gene quads per wave
        const int nt = (kp + 31) / 32;
        list[n++] = op == ZiOp::update ? ZiCand{ZiFam::f32, nt, 0} : ZiCand{ZiFam::f32, nt, nt == 1 ? 4 : nt == 2 ? 2 : 1};
    }
    return list[i];
}
// some product of this width may run on the tiles family: the scratch entries leave room for its images
constexpr bool zi_may_use_tiles(int64_t kp) {
    if (kp <= 0 || kp > ZI_KP_MAX) return false;
    return zi_candidate(ZiOp::update, (int)kp, ORIANA_MATRIX_BF16X3, 0).fam == ZiFam::tiles ||
           zi_candidate(ZiOp::dt, (int)kp, ORIANA_MATRIX_BF16X3, 0).fam == ZiFam::tiles;
}
// the rule can answer tiles<KC, TAIL> for this product at some width: the instantiations dense_zi.hip holds
constexpr bool zi_tiles_reachable(ZiOp op, int kc, int tl) {
    for (int kp = 16; kp <= ZI_KP_MAX; kp += 4) {
        const ZiCand c = zi_candidate(op, kp, ORIANA_MATRIX_BF16X3, 0);
        if (c.fam == ZiFam::tiles && c.a == kc && c.b == tl) return true;
    }
    return false;
}

// Run-time preconditions of a family; a candidate that fails them is passed over.  tiles moves 16-byte pieces of D_hat rows,
// logits, flags and images (gene count a multiple of 4, aligned pointers); the D update is the fused form only (per-lane flags
// of oriana_nzmask_tiles, V_next and DV_next given) and keeps its tile offsets in 32 bits.  b16 and f32 take everything the
// entries admit.
static inline bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}
static inline bool zi_update_ok(ZiFam f, const float *D_hat, const float *lgit, const uint32_t *nztiles, const double *Vn,
                                const double *DV, int64_t m) {
    return f != ZiFam::tiles || (Vn && DV && nztiles && m % 4 == 0 && m <= 16000000 && aligned16(D_hat, lgit, nztiles));
}
static inline bool zi_dt_ok(ZiFam f, const float *D, const float *scratch, int64_t m) {
    return f != ZiFam::tiles || (scratch && m % 4 == 0 && aligned16(D, scratch));
}

// run(ZiPick) for the first candidate of <OP, KP, ARITH> whose preconditions hold (ok(family)); ORIANA_EKRANGE if there is none
template <ZiFam F, int A, int B> struct ZiPick { static constexpr ZiFam fam = F; static constexpr int a = A, b = B; };
template <ZiOp OP, int KP, int ARITH, int I = 0, typename Ok, typename Run>
static int zi_first(Ok &&ok, Run &&run) {
    constexpr ZiCand c = zi_candidate(OP, KP, ARITH, I);
    if constexpr (c.fam == ZiFam::none) return ORIANA_EKRANGE;
    else return ok(c.fam) ? run(ZiPick<c.fam, c.a, c.b>{}) : zi_first<OP, KP, ARITH, I + 1>(ok, run);
}

// ------------------------------------------------------------------------------------------
// Number of ranges to cut the reduction (or gene) axis into, given `blocks` work-groups along the other axis.  The grid runs in
// rounds of per_cu x CUs resident work-groups, and a last round that is nearly empty costs as much as a full one: among the counts
// up to max_ranges whose grid stays within max_rounds rounds' worth, the one that leaves the last round fullest; a larger count
// wins only by more than `margin` (fewer ranges on ties: each one ends in a set of float64 atomics).
// ------------------------------------------------------------------------------------------
struct SplitRule {
    int per_cu;            // resident work-groups per CU
    int64_t max_ranges;    // range limit
    int max_rounds;        // cap on rounds
    double margin;         // tie margin
    int small_rounds;      // small-grid penalty: below this many rounds' worth the fill counts 0.5 .. 1 of itself; 0 = none
};
// dense_f32.hip: rounds of 512 resident work-groups (2 per CU) on MI355X -- 1580 groups take 4 rounds at 77 %.  Among 4 to 12
// rounds' worth (below 4 there are too few groups to hide the tails)
constexpr SplitRule SPLITS_F32 = {2, 4096, 12, 0.02, 4};
// dense_zi.hip: work-groups of 512 threads, one per CU (256 on MI355X)
constexpr SplitRule SPLITS_TILES = {1, 64, 16, 0.03, 0};

static int64_t pick_splits(int64_t blocks, int64_t max_splits, const SplitRule &rule) {
    const int64_t slots = rule.per_cu * oriana_device_cus();
    int64_t best = 1;
    double best_eff = 0.0;
    for (int64_t sp = 1; sp <= max_splits && sp <= rule.max_ranges; ++sp) {
        const int64_t groups = blocks * sp;
        if (groups > rule.max_rounds * slots && sp > 1) break;
        const int64_t rounds = (groups + slots - 1) / slots;
        double eff = (double)groups / (double)(rounds * slots);
        if (groups < rule.small_rounds * slots) eff *= 0.5 + 0.5 / rule.small_rounds * (double)groups / (double)slots;
        if (eff > best_eff + rule.margin) { best_eff = eff; best = sp; }
    }
    return best;
}

// dense_zi.hip, called from the entries of dense_f32.hip
int64_t zi_sweep_image_floats(int64_t m);
int64_t zi_dt_image_floats(int64_t n);
int64_t zi_tiles_words(int64_t n, int64_t m);
int zi_tiles(uint32_t *out, const uint32_t *nzmask, int64_t n, int64_t m, hipStream_t st);
int zi_sweep(KcTl cfg, float *D_hat, const double *U, const double *V, const float *lgit, int64_t mpad, const uint32_t *nztiles,
             double *colsum, const double *Vn, double *DV, float *img_scratch, int64_t n, int64_t m, int K, hipStream_t st);
int zi_dt(KcTl cfg, double *out, const float *D, const double *W, float *scratch, int64_t n, int64_t m, int K, hipStream_t st);
// zi_sweep without the D_hat store and the column sums (k_zi_row<KC, TAIL, RATE = true>): DV += d V over the active cells only
int zi_rate(KcTl cfg, const double *U, const double *V, const float *lgit, int64_t mpad, const uint32_t *nztiles, double *DV,
            const uint8_t *active, float *img_scratch, int64_t n, int64_t m, int K, hipStream_t st);

}  // namespace dn
}  // namespace oriana
