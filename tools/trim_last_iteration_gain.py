# -*- coding: utf-8 -*-
"""Steps the two sliced kernels issue at configs[3] (the genes left after the hybrid layout's dense cut, as
tools/tile_slot_efficiency.py builds them) today and with the all-padding steps of a slice's final iteration not issued
(csrc/passes_k100.h): the predicted gain of that change, counted where the time goes.

A slice whose longest row (column) has L entries runs ceil(L / 4) iterations of 4 steps today and L steps trimmed.
  row pass:    a wave carries two slices and runs the longer one's steps; the eight waves of a group meet at the tile
               barrier, so a tile costs the group the maximum over its waves
  column pass: a wave owns one column slice of both tiles of a pair; the sixteen waves meet once per row block
python tools/trim_last_iteration_gain.py [rows]   (CPU; rows = cells of the sample, a multiple of 256)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oriana_amd.singlecell.generation import SyntheticCounts   # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
m, K, W = 30000, 100, 256
gen = SyntheticCounts(1000000, m, K, seed=1234 + 1000 * 4, device='cpu', zero_inflation_level=0.10, row0=0, n=n)
nz = gen.chunk(0, n).numpy() != 0
cnt = nz.sum(0)
order = np.argsort(-cnt, kind='stable')
gd = int((cnt >= 0.2 * n).sum()) // 32 * 32
nzs = nz[:, order[gd:]]
ms = nzs.shape[1]
nt = (ms + W - 1) // W
nb = n // 256
pad = np.zeros((nb * 256, nt * W), bool)
pad[:, :ms] = nzs[:nb * 256]
t4 = pad.reshape(nb, 256, nt, W)


def issued(L):
    return (L + 3) // 4 * 4


def report(name, today, trimmed):
    print('  %-44s %12d -> %12d steps  (-%.2f %%)' % (name, today, trimmed, 100.0 * (today - trimmed) / max(today, 1)))
    return (today - trimmed) / max(today, 1)


print('%d cells x %d sliced genes (%d dense), %d row blocks x %d gene tiles' % (nb * 256, ms, gd, nb, nt))

# ---- row pass: [block][slice][tile] longest row of the slice
rl = t4.sum(3).reshape(nb, 16, 16, nt).max(2)
L0 = rl.reshape(nb, 8, 2, nt)
wave_today, wave_trim = issued(L0).max(2), L0.max(2)          # trimmed: the live slices' remainder = the longer slice's length
print('row pass (k_row_pass_k100)')
report('per slice', int(issued(rl).sum()), int(rl.sum()))
report('per wave (max of its two slices)', int(wave_today.sum()), int(wave_trim.sum()))
g_row = report('per group (max of 8 waves per tile)', int(wave_today.max(1).sum()), int(wave_trim.max(1).sum()))
print('  steps per slice and tile: %.1f today (%.2f iterations); empty steps of a final iteration: %.2f of 4' %
      (issued(rl).mean(), issued(rl).mean() / 4, (issued(rl) - rl)[rl > 0].mean()))

# ---- column pass: [block][tile][slice] longest column of the slice inside the row block
cl = t4.sum(1).reshape(nb, nt, 16, 16).max(3)
ntp = (nt + 1) // 2 * 2
cl2 = np.zeros((nb, ntp, 16), cl.dtype)
cl2[:, :nt] = cl
pair_today = issued(cl2).reshape(nb, ntp // 2, 2, 16).sum(2)   # a wave: its slice of both tiles of the pair
pair_trim = cl2.reshape(nb, ntp // 2, 2, 16).sum(2)
print('column pass (k_col_pass2)')
report('per wave (its slice of both tiles)', int(pair_today.sum()), int(pair_trim.sum()))
g_col = report('per group (max of 16 waves per row block)', int(pair_today.max(2).sum()), int(pair_trim.max(2).sum()))
print('  empty steps of a final iteration: %.2f of 4' % ((issued(cl) - cl)[cl > 0].mean()))

if len(sys.argv) > 3:                                          # measured kernel times (ms) of the parent: row pass, column pass
    tr, tc = float(sys.argv[2]), float(sys.argv[3])
    print('predicted, if a kernel\'s time follows the steps of its groups: row pass %.2f ms -> -%.2f ms, column pass %.2f ms -> '
          '-%.2f ms, together -%.2f ms per sweep' % (tr, tr * g_row, tc, tc * g_col, tr * g_row + tc * g_col))
