// counts_check.h -- the layout checks shared by the entries that walk both layouts of a model's matrix (groupstats.hip,
// ranksum.hip): made before any HIP call.
#pragma once
#include "common.h"

namespace oriana {

static inline int gs_check_layouts(const oriana_counts *cm, const oriana_dense *dn) {
    if (!cm || cm->n < 0 || cm->m < 0 || cm->nrb < 0 || cm->ncb < 0 || cm->rslots < 0) return ORIANA_EINVAL;
    if (cm->nrb * cm->ncb > 0 && cm->rslots > 0 && (!cm->roff || !cm->rslice || !cm->rowrec)) return ORIANA_EINVAL;
    if (dn) {
        if (dn->n < 0 || dn->gd < 0 || dn->nct < 0 || (dn->gd & 31)) return ORIANA_EINVAL;
        if (dn->gd > 0 && dn->n > 0 && (!dn->x || dn->n != cm->n || dn->nct * 32 < dn->n)) return ORIANA_EINVAL;
    }
    return 0;
}

}  // namespace oriana
