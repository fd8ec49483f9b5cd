# -*- coding: utf-8 -*-
"""Shared helpers for the parity tests (tolerances follow SURVEY.md section 7, hard part 4)."""
import glob
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

PARAM_KEYS = ['alpha1', 'alpha2', 'beta1', 'beta2', 'a1', 'a2', 'b1', 'b2', 'pi_d', 'p_d', 'pi_s', 'p_s']
EXPECT_KEYS = ['U_hat', 'V_hat', 'log_U_hat', 'log_V_hat', 'S_hat']

RTOL = 1e-5   # BASELINE.json north_star: "within 1e-5 relative on the variational parameters"
# Achieved errors of the HIP path against the reference's golden states, all models / shapes / starts
# (profiles/r02_parity_errors.json, tools/parity_report.py): Gamma parameters and expectations <= 1.6e-6 in this
# metric and <= 3.3e-6 STRICTLY element-wise relative, i.e. RTOL has a 3x margin even without the column term.
# The dropout posterior is a probability: its error is judged absolutely -- measured 1.2e-7 on p_d and 7e-10 on
# pi_d against the reference (round 1 allowed 1e-4); the bounds below leave room for the larger Lambda of the
# multi-tile / sharded cases (|d p_d| <= 0.25 |d Lambda|, Lambda carries the 1e-6 relative error of U_hat, V_hat).
KEY_ATOL = {'p_d': 2e-6, 'pi_d': 1e-7}
# The sparsity posterior p_s = sigmoid(logit(pi_s) - t), t a float32 difference of two sums of magnitude 1e4..1e6,
# is judged against the EXACT value of the same sweep wherever a test can compute it (exact_twin below: HIP within
# 7.1e-6, the reference's own arithmetic within 2.0e-6).  Where it cannot (the NMF-start goldens, whose float32 loop
# underflows where float64 does not), the bound against the reference's state is 2 x the worst error achieved over all
# goldens and sweeps (profiles/r03_parity_errors.json: p_s, S_hat 5.8e-6 in the column metric; pi_s 5.4e-7, i.e. inside
# RTOL without an entry here).  Round 3 allowed 1e-4.
KEY_RTOL = {'p_s': 1.2e-5, 'S_hat': 1.2e-5}

def golden_files(pattern='*_*.npz'):
    skip_metrics = not pattern.startswith('metrics_')
    return sorted(f for f in glob.glob(os.path.join(GOLDEN, pattern))
                  if not f.endswith('tables.npz') and not os.path.basename(f).startswith('generator_')
                  and not f.endswith('_xcheck.npz')
                  and not (skip_metrics and os.path.basename(f).startswith('metrics_')))


def xcheck_files():
    """The patched-SparseGaP fixtures cross-checked by the reference's unpatched SparseZIGaP class with D_hat == 1
    (tests/golden/make_golden.py xcheck; SURVEY 8a policy ii)."""
    return sorted(glob.glob(os.path.join(GOLDEN, 'sparsegap_*_xcheck.npz')))


def load_golden(path):
    g = np.load(path)
    return {k: g[k] for k in g.files}


def state_of(g, tag):
    pre = tag + '/'
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}


def err_colrel(got, ref):
    """max |got-ref| / (|ref| + colmax|ref|): the per-column relative error of SURVEY 7.4."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    if ref.ndim == 2:
        cm = np.max(np.abs(ref), axis=0, keepdims=True)
    else:
        cm = np.max(np.abs(ref))
    den = np.abs(ref) + cm + 1e-300
    bad = ~np.isfinite(got) | ~np.isfinite(ref)
    if bad.any():
        same = (got == ref) | (np.isnan(got) & np.isnan(ref))
        if not same[bad].all():
            return np.inf
    d = np.where(bad, 0.0, np.abs(got - ref) / den)
    return float(np.max(d))


def exact_twin(oracle_model):
    """A copy of an oracle model (BEFORE its step) whose loop nest runs in float64 (cavi_oracle.zq_exact): the yardstick
    the reference's float32 evaluation and the HIP path are both measured against for the sparsity posterior.

    p_s = sigmoid(logit(pi_s) - t), t = -Zlog + c * Vprime (sparse_gap.py:135-137), is a difference of two sums of
    magnitude 1e3..1e6 that leaves t = O(10): every float32 evaluation of the loop nest -- the reference's own included --
    moves it.  Measured on the goldens (profiles/r03_parity_errors.json): the reference is up to 2.0e-6 away from the
    exact p_s, the HIP path up to 7.1e-6 (1.4e-4 in round 2, before the log sums were centred)."""
    import copy
    E = copy.deepcopy(oracle_model)
    E.exact = True
    return E


PS_FLOOR = {'p_s': 1.4e-5, 'S_hat': 1.4e-5, 'pi_s': 2e-6}   # absolute, against the EXACT value: 2 x the measured worst (7.1e-6 / 1.0e-6)
PS_FACTOR = 8.0                                            # ... or this many times the reference's own distance from exact (<= 2.0e-6)


# The log sums Z_log (and Z_i, Z_j beside them) under scale drift (tests/test_sparse_side_gpu.py, tests/logsum_reference.py:
# n = 300, m = 260, lu = 1.5 N + shift_u, lv = 1.5 N + shift_v at (0, 0), (35, -30), (-40, 38) and (35, -30) with one cell at
# lu - 80; seven kernel forms) are judged against the float64 loop nest (cavi_oracle.zq_exact) in err_colrel: the HIP output may
# be no further from exact than ZLOG_FLOOR, or ZLOG_FACTOR times the distance of the reference's own float32 nest on the same
# inputs, which the test measures at run time.  Measured, all 28 cases (profiles/zlog_drift_errors.json):
#   * HIP / reference distance: Z_log <= 1.32 x, Z_j <= 1.20 x, Z_i <= 1.67 x (HIP 1.1e-7 .. 3.0e-7 on the fast path);
#   * two plain float32 sums without the per-factor centre (logsum_reference.logsum_f32(center=False)) at (-40, 38):
#     3.0e-6 .. 8.1e-6 = 15.2 x (K = 200) .. 24.1 x (K = 100) the reference's distance; the centred evaluation of the same sums
#     <= 1.7 x.  At (35, -30) the un-centred form is only 3.7 .. 6.2 x: that shift alone does not tell the two apart, (-40, 38) does.
#     On the GPU itself, oriana_scale_factor_centered and oriana_finalize_zlog called with acc = NULL at K = 20: 3.3e-6 against
#     1.3e-7 with the centre (test_log_centre_is_applied_consistently).
# ZLOG_FACTOR sits above twice the worst HIP ratio (3.35) and below half the smallest un-centred ratio (7.6).
ZLOG_FACTOR = 4.0
# ... or this, absolute: four float32 roundings (2^-24 each), for a reference that happens to land within a rounding of exact
ZLOG_FLOOR = 2.4e-7
# The yardstick itself must be sharp: the reference's float32 nest within 1e-6 of exact (measured <= 3.9e-7 on the fast path).
# The cell at lu - 80 has lu + lv ~ -75, which the reference rounds to float32 BEFORE the exponential: half an ulp of 75 is
# 2^-18 = 3.8e-6 relative on that cell's r_ijk, and the cell dominates the Z_log entries it touches (measured <= 2.3e-6; the
# slow path of the HIP side reproduces that arithmetic and lands at the same distance).
ZLOG_REF_MAX = 1e-6
ZLOG_REF_MAX_SLOW = 4e-6
# The dense-gene passes (tests/test_dense_pass_gpu.py, tests/dense_pass_reference.py: n = 300, 160 dense genes, one K per padded
# width 16 .. 100, the plain, sparse and zi-quirk nests, one work-group walking all five gene tiles / all ten cell tiles, split
# 2 x 3, one tile per work-group, the slow path, nine gene tiles, the split last round) are held to the SAME bound, nothing
# added.  Measured, all 80 cases (profiles/dense_pass_errors.json): HIP / reference distance Z_i <= 1.32 x, Z_log <= 1.81 x,
# Z_j <= 2.34 x -- the worst where one wave keeps its sums on the matrix core for eight cell tiles (0.6 x with one tile per
# work-group, whose atomics arrive in any order); at most 0.58 of the bound.  On the CPU (tests/test_dense_pass_host.py) the complete six-product evaluation sits at
# <= 0.14 of the bound and one that loses mid x mid, both lo terms or one lo term at 3.5 .. 11.9 times the bound at every width.
# (2 x 2.34 is above ZLOG_FACTOR: these cases have a margin of 1.7, not the factor two the drift cases were given.)
# The sliced row and column passes (tests/test_sliced_pass_gpu.py, tests/sliced_pass_reference.py: counts constructed for the slice
# edges -- every remainder of a slice's longest row, 0 .. 6 and 64 iterations per slice in one tile, empty slices and waves, ragged
# blocks and tiles --, one K per configuration of the dispatcher (18), the plain, weighted, sparse and sparse + weighted nests, one
# work-group per row block, the whole-grid split, the split last round, the planner's split; planned / many-items / one-item work
# lists, the partials, the band grid on 11 row blocks) are held to the SAME bound, nothing added.  Measured, all 330 cases
# (profiles/sliced_pass_errors.json), HIP / reference distance, worst per kernel family:
#   Z_i (row kernel):     narrow 1.67 x, k_row_pass<G,...> 1.55 x, k64 1.47 x, k100 1.10 x; with k_row_spmm behind it 1.46 x / 1.12 x;
#   Z_j (column kernel):  narrow 0.86 x, k_col_pass2 1.64 x, k_col_pass2<DUAL> 1.67 x, k64 1.62 x, k_col_pass 1.45 x;
#   Z_log:                k_col_pass2 1.43 x, k_col_pass2<DUAL> 1.99 x, k64 1.09 x (the partials only), k_col_pass 1.83 x -- up to
#                         Kp = 64 every form with log sums, the weighted one included, takes the DUAL kernel (the test sees
#                         engine.col_pass_dual run), so the narrow kernel never sums them and k64 only in the deterministic mode;
#   the band grid <= 0.84 x, through oriana_zq_gap_f32 <= 1.20 x.  HIP 5.3e-8 .. 4.7e-7 from exact, the reference 7.4e-8 .. 5.4e-7.
# That is at most 0.50 of the bound (Z_log; Z_i and Z_j 0.42): twice the worst ratio, 3.99, is just inside ZLOG_FACTOR.  On the CPU
# (tests/test_sliced_pass_host.py, K = 20) the complete float32 evaluation in slot order sits at <= 0.29 of the bound; with the
# record in the last occupied slot of ONE slice skipped it is at >= 2136 x the bound (Z_i) and >= 2325 x (Z_j), with ONE padding
# slot read as an entry of image row 0 with x = 1 at >= 1083 x and >= 1405 x -- the least over the 115 slices that have slots, on
# the row side and, transposed, on the column side.


def zlog_bound(d_ref):
    """The largest err_colrel from exact a HIP loop-nest output may have where the reference's float32 nest has d_ref."""
    return max(ZLOG_FLOOR, ZLOG_FACTOR * d_ref)


def assert_state_close(got, ref, rtol=RTOL, keys=None, what='', exact=None):
    """|got - ref| <= rtol*|ref| + rtol*colmax|ref| on every key, plus identical clamp
    patterns (entries sitting exactly on the 1e-15 floor / the 1-1e-10 ceiling).  `exact`: the state of the exact twin
    of the same sweep -- the sparsity posterior is then judged against IT: the HIP value may be no further from exact
    than PS_FLOOR, or PS_FACTOR times the distance of `ref` (the reference's float32 arithmetic) from exact."""
    keys = keys or [k for k in PARAM_KEYS + EXPECT_KEYS if k in ref]
    for k in keys:
        if k not in ref or k not in got:
            continue
        if exact is not None and k in PS_FLOOR:
            d_hip = float(np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(exact[k], dtype=np.float64)).max())
            d_ref = float(np.abs(np.asarray(ref[k], dtype=np.float64) - np.asarray(exact[k], dtype=np.float64)).max())
            assert d_hip <= max(PS_FLOOR[k], PS_FACTOR * d_ref), \
                '%s %s: HIP is %.3e from exact, the reference arithmetic %.3e' % (what, k, d_hip, d_ref)
            continue
        if k in KEY_ATOL:
            e = float(np.max(np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(ref[k], dtype=np.float64)))) if np.size(ref[k]) else 0.0
            assert e <= KEY_ATOL[k], '%s %s: abs err %.3e > %.1e' % (what, k, e, KEY_ATOL[k])
        else:
            e = err_colrel(got[k], ref[k])
            tol = max(rtol, KEY_RTOL.get(k, 0.0))
            assert e <= tol, '%s %s: err %.3e > %.1e' % (what, k, e, tol)
        if k in ('a1', 'a2', 'b1', 'b2', 'alpha1', 'alpha2', 'beta1', 'beta2'):
            assert np.array_equal(np.asarray(got[k]) == 1e-15, np.asarray(ref[k]) == 1e-15), \
                '%s %s: 1e-15 clamp pattern differs' % (what, k)
        if k == 'p_d':
            assert np.array_equal(np.asarray(got[k]) == 1. - 1e-10, np.asarray(ref[k]) == 1. - 1e-10), \
                '%s p_d: (1 - 1e-10) mask differs' % what


def dropout_sweep(D, U, V, pi, mask, cs, Vn, DV, scratch, arithmetic, n, m, K):
    """oriana_dropout_sweep_fused_tiles with the per-lane flags built from `mask` (oriana_nzmask_f32 layout; None: no mask,
    which is the round-2 entry oriana_dropout_sweep_fused)."""
    import torch
    from oriana_amd import _lib
    from oriana_amd._lib import call, ptr, stream_ptr
    tiles = None
    if mask is not None:
        tiles = torch.zeros(max(int(_lib.load().oriana_nzmask_tiles_words(n, m)), 4), dtype=torch.int32, device=mask.device)
        call('oriana_nzmask_tiles', ptr(tiles), ptr(mask), n, m, stream_ptr())
    call('oriana_dropout_sweep_fused_tiles', ptr(D), ptr(U), ptr(V), ptr(pi), ptr(mask), ptr(tiles), ptr(cs), ptr(Vn), ptr(DV),
         ptr(scratch), arithmetic, n, m, K, stream_ptr())
    return tiles


# ---- scratch and outputs under a contract (tests/test_scratch_contract_host.py, tests/test_scratch_contract_gpu.py) ---------------
GUARD_BYTES = 4096
# variant -> (interior byte, guard byte).  'nan': every byte 0xFF is NaN as float32 and as float64 and -1 as an integer, and a float
# read past the end meets NaN too.  'stale' starts as 'zero'; the test then makes a valid call of the same sizes on other seeded
# inputs and hands the buffer over as that call left it (stale_scratch below).
SCRATCH_VARIANTS = {'zero': (0x00, 0xA5), 'nan': (0xFF, 0xFF), 'stale': (0x00, 0xA5)}


def guarded(nbytes, interior=0x00, guard=0xA5, dtype=None, device='cuda'):
    """(view, check): a view of EXACTLY nbytes bytes as `dtype` (default uint8), its first byte on a multiple of 256, every byte
    `interior`, inside an allocation whose other bytes -- at least GUARD_BYTES on each side -- are `guard`; check() asserts that
    every byte outside the view still is."""
    import torch
    dtype = torch.uint8 if dtype is None else dtype
    nbytes = int(nbytes)
    size = torch.empty((), dtype=dtype).element_size()
    assert nbytes >= 0 and nbytes % size == 0, (nbytes, dtype)
    raw = torch.full((nbytes + 2 * GUARD_BYTES + 256,), guard, dtype=torch.uint8, device=device)
    lo = GUARD_BYTES + (-(raw.data_ptr() + GUARD_BYTES)) % 256
    hi = lo + nbytes
    raw[lo:hi] = interior
    view = raw[lo:hi].view(dtype)
    assert view.data_ptr() % 256 == 0 and view.numel() * size == nbytes and lo >= GUARD_BYTES and raw.numel() - hi >= GUARD_BYTES

    def check(what=''):
        for name, band, at in (('before', raw[:lo], -lo), ('behind', raw[hi:], nbytes)):
            bad = torch.nonzero(band != guard)
            assert bad.numel() == 0, '%s: %d guard bytes %s the %d-byte buffer were written, the first at byte %d' % (
                what, bad.numel(), name, nbytes, at + int(bad[0]))
    return view, check


def guarded_variant(nbytes, variant, dtype=None, device='cuda'):
    interior, guard = SCRATCH_VARIANTS[variant]
    return guarded(nbytes, interior, guard, dtype, device)


def guarded_out(shape, dtype, fill, device='cuda'):
    """An output tensor of `shape` inside guard bands: `fill` = 'nan' where the entry writes every element (all bytes 0xFF: NaN as
    a float, -1 as an integer), 'zero' where it adds to what is there."""
    import torch
    numel = 1
    for s in shape:
        numel *= int(s)
    view, check = guarded(numel * torch.empty((), dtype=dtype).element_size(), {'nan': 0xFF, 'zero': 0x00}[fill], 0xA5, dtype, device)
    return view.view(*shape), check
