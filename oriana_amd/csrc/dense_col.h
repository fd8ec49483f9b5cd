// dense_col.h -- what the two gene-side kernels over dense 32 x 32 tiles share: dn::k_dn_col (dense_pass.hip: C += S^T FU from
// the packed tiles of s) and dn::k_zi_col (dense_zi.hip: out += D_hat^T W from the row-major D_hat).  Both walk a range of cell
// tiles with the same pipeline: every global read is an LDS-DMA copy (the cell images shared by the 8 waves: ring of three; the
// wave's own 32 x 32 tile: ring of two), issued TWO tiles ahead; the vector-memory counter retires in issue order, so "at most
// the copies of this iteration outstanding" means the previous iteration's have landed.  The partial sums stay on the matrix core
// for COL_FLUSH tiles (256 cells: inside the regime where the bf16 x 3 chain carries the float32 chain's error) and then join the
// running float32 sums; the four tail factors go through v_mfma_f32_4x4x1_16B_f32 (exact float32 FMAs).
// Here: the LDS size, the flush period, the waits, the tail factors' block and the sum of the lane halves.  The ring set-up, the
// loop, the operand split, the six-product block and the flush stay in the two kernels: shared, they changed the compiled
// kernels ("Sharing between the dense tile kernels").
#pragma once
#include "dense_tiles.h"

namespace oriana {
namespace dn {

constexpr int COL_FLUSH = 8;             // tiles between two flushes of the matrix-core sums

// LDS: [3][PU] image ring, then [2][8 waves][256 pieces] tile ring
template <int KC, int TAIL> constexpr int col_lds_bytes() { return 3 * Cfg<KC, TAIL>::PU * 16 + 2 * NW * 256 * 16; }

// LDS-DMA instructions per wave and tile: the image's share + the four of the wave's own tile
template <int KC, int TAIL> constexpr int col_copies() { return Cfg<KC, TAIL>::PU / (NW * 64) + 4; }

// the previous iteration's copies have landed, this iteration's NCOPY may be in flight
template <int NCOPY>
__device__ __forceinline__ void col_wait_prev() {
    static_assert(NCOPY >= 5 && NCOPY <= 7, "the waits below count the copies of one iteration");
    if (NCOPY == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else if (NCOPY == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
}

// t += the other lane half's t (the 4 x 4 x 1 blocks of the tail factors: each lane half has summed its own half of the tiles)
__device__ __forceinline__ void add_lane_halves(f4v &t) {
    t.x += __shfl_xor(t.x, 32, 64); t.y += __shfl_xor(t.y, 32, 64);
    t.z += __shfl_xor(t.z, 32, 64); t.w += __shfl_xor(t.w, 32, 64);
}

// The tail factors of one tile: 16 blocks of 4 genes x 4 factors, one cell per instruction: A[b][i] = the value of gene
// 4 (b % 8) + i (this lane's sc), B[b][j] = factor KM + j of the cell (t2p: the lane's pieces of the image's tail)
__device__ __forceinline__ void col_tail(const f4v *t2p, const f4v (&sc)[4], f4v &cta) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f4v t2 = t2p[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) cta = __builtin_amdgcn_mfma_f32_4x4x1f32(sc[q][e], t2[e], cta, 0, 0, 0);
    }
}

}  // namespace dn
}  // namespace oriana
