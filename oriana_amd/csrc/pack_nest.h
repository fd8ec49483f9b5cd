// pack_nest.h -- the packing sequence of the sliced layout, written ONCE for the C entries that pack: the stateless drop-ins
// (stateless.hip: one chunk, the caller's gene order, a workspace) and the resident handle (resident.hip: row chunks in the packed
// gene order, hipMalloc, the dense block of a hybrid layout beside it).  CountTiles._build (oriana_amd/engine.py) is the ONE Python
// copy; all three share the scan (oriana_pack_offsets) and the planners' inputs (oriana_plan_inputs).
#pragma once
#include "zq_nest.h"

namespace oriana {

// the per-tile tables of a layout (device): [nt] counts, [nt + 1] offsets, [nt][17] slice tables
struct PackTables {
    int32_t *tile_nnz, *tile_rslots, *tile_cslots;
    int64_t *roff, *coff;
    uint32_t *rslice, *cslice;
};

// count -> offsets -> totals (the one host synchronisation) -> zero-filled record arrays -> fill -> struct oriana_counts, for the (n, ms) float32
// matrix that `chunk` hands out in row chunks of chunk_rows (a multiple of 256, or n).
//   chunk(r0, rows, fill, &X, &ld): rows [r0, r0 + rows); once per chunk on the counting pass (fill = false; not at all when ms == 0)
//       and once on the fill pass (fill = true: the dense block of a hybrid layout, packed from the same chunk, rides on this call).
//   place(rslots, cslots, &rowrec, &ridx, &side_nz): the caller's allocation of the record arrays, which it zero-fills (padding slots:
//       x == 0, row index 0; the resident handle fills one while it allocates the next); side_nz only with `side`, a dense (n, ms)
//       matrix gathered at the stored entries (row-side slots).
//   nnz: the non-zeros, where the caller knows them; else any value > 0 (0 keeps oriana_fixup from looking at the flags).
template <typename Chunk, typename Place>
static int pack_sliced(oriana_counts *cm, int64_t n, int64_t ms, int64_t chunk_rows, const PackTables &t, const int32_t *col_perm,
                       const float *side, int64_t ldside, int64_t nnz, Chunk &&chunk, Place &&place, hipStream_t s) {
    const int64_t ncb = (ms + TILE - 1) / TILE, nt = (n + TILE - 1) / TILE * ncb;
    const float *X = nullptr; int64_t ld = 0;
    if (ms > 0) {
        for (int64_t r0 = 0; r0 < n; r0 += chunk_rows) {
            const int64_t rows = (n - r0 < chunk_rows) ? n - r0 : chunk_rows;
            ORIANA_TRY(chunk(r0, rows, false, &X, &ld));
            ORIANA_TRY(oriana_pack_count(X, 0, rows, ms, ld, r0 / TILE, ncb, t.tile_nnz, t.tile_rslots, t.tile_cslots, t.rslice, t.cslice, s));
        }
    }
    int64_t tot[2] = {0, 0};
    ORIANA_TRY(oriana_pack_offsets(t.roff, t.coff, t.tile_rslots, t.tile_cslots, nt, tot, s));
    oriana_rowrec *rowrec = nullptr; uint8_t *ridx = nullptr; float *side_nz = nullptr;
    ORIANA_TRY(place(tot[0], tot[1], &rowrec, &ridx, &side_nz));
    for (int64_t r0 = 0; r0 < n; r0 += chunk_rows) {
        const int64_t rows = (n - r0 < chunk_rows) ? n - r0 : chunk_rows;
        ORIANA_TRY(chunk(r0, rows, true, &X, &ld));
        if (ms > 0)
            ORIANA_TRY(oriana_pack_fill(X, 0, rows, ms, ld, r0 / TILE, ncb, t.roff, t.coff, t.rslice, t.cslice, rowrec, ridx,
                                        side_nz ? side + r0 * ldside : nullptr, ldside, side_nz, s));
    }
    cm->n = n; cm->m = ms; cm->nrb = (n + TILE - 1) / TILE; cm->ncb = ncb; cm->nnz = nnz; cm->rslots = tot[0]; cm->cslots = tot[1];
    cm->roff = t.roff; cm->coff = t.coff; cm->rslice = t.rslice; cm->cslice = t.cslice; cm->rowrec = rowrec; cm->ridx = ridx;
    cm->col_perm = col_perm; cm->row_perm = nullptr;
    return 0;
}

}  // namespace oriana
