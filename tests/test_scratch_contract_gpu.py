# -*- coding: utf-8 -*-
"""include/oriana_hip.h: "all scratch memory is supplied by the caller", its contents undefined on entry and exit.  Every entry
below runs on a scratch of EXACTLY the size its size function states (helpers.guarded: 256-byte aligned, 4096 guard bytes on each
side) under three fills --

    zero    every byte 0x00 (what the library's own torch.zeros gives),
    nan     every byte 0xFF: NaN as float32 and float64, -1 as an integer, and a float read past the end meets NaN too,
    stale   what a previous valid call of the same sizes on other seeded inputs left behind

-- and re-runs the assertions of the entry's own test (the same float64 reference, the same bounds, the functions those tests
call) on what it wrote.  On top: no guard byte changes, every output is finite where the reference is, and where the header
promises one writer and a fixed order the outputs of the three fills are the same bit for bit.  The outputs lie in guarded
buffers of their own, NaN-filled where the header says that every element is written.

oriana_tsne_repulse, oriana_louvain_sweep, oriana_rank_sums, oriana_zi_cell_bound and oriana_zi_gene_rate have such tests beside
their own (tests/test_tsne_gpu.py, test_community_gpu.py, test_wilcoxon_gpu.py, test_zi_score_gpu.py, test_zi_fold_in_fit_gpu.py)."""
import numpy as np
import pytest
import torch

import kmeans_reference as kr
import knn_reference as nr
import silhouette_reference as sr
from helpers import SCRATCH_VARIANTS, guarded_out, guarded_variant

pytestmark = pytest.mark.gpu

VARIANTS = ('zero', 'nan', 'stale')
assert set(VARIANTS) == set(SCRATCH_VARIANTS)
DEV = 'cuda'
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64


@pytest.fixture(scope='module')
def lib():
    from oriana_amd import _lib
    return _lib.load()


def _scratch(nbytes, variant, dtype, warm):
    """(view, check) of helpers.guarded_variant; 'stale': warm(view) -- a valid call of the same sizes on other inputs -- has run
    on it, inside its bounds."""
    view, check = guarded_variant(nbytes, variant, dtype, DEV)
    if variant == 'stale':
        warm(view)
        torch.cuda.synchronize()
        check('the call that leaves the stale contents')
    return view, check


def _all_checks(checks, what):
    torch.cuda.synchronize()
    for c in checks:
        c(what)


def _same_bits(runs, what):
    """The outputs (tuples of NumPy arrays) of the three fills, bit for bit."""
    first = runs[VARIANTS[0]]
    for v in VARIANTS[1:]:
        assert len(runs[v]) == len(first)
        for a, b in zip(first, runs[v]):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), '%s: %s against %s' % (what, v, VARIANTS[0])


# ---- the dense entries of a ZI sweep (csrc/dense_f32.hip, csrc/dense_zi.hip) ---------------------------------------------------
# One shape per kernel family and (KC, TAIL) branch; every n leaves a partial 16-row chunk (37 and 300: an odd chunk count), every
# m a partial 32-gene tile.
ZI_SHAPES = [(37, 53, 3), (70, 90, 128),                                            # the float32 instruction
             (300, 517, 20), (129, 2050, 33),                                       # bf16 x 3, m no multiple of 4
             (77, 64, 33), (300, 132, 57), (260, 300, 97), (257, 132, 100), (31, 4, 100)]       # the tiles family
ZI_IDS = ['%dx%dx%d' % s for s in ZI_SHAPES]
ARITH = pytest.mark.parametrize('arithmetic', [0, 1], ids=['f32', 'bf16x3'])


@pytest.mark.parametrize('with_next', [True, False], ids=['next', 'no-next'])
@ARITH
@pytest.mark.parametrize('n,m,K', ZI_SHAPES, ids=ZI_IDS)
def test_dropout_sweep(lib, n, m, K, arithmetic, with_next):
    """oriana_dropout_sweep_fused_tiles with the per-lane flags, as helpers.dropout_sweep calls it (oriana_dropout_sweep_fused
    forwards to it with nztiles = NULL and picks among the same kernels), under the assertions of
    tests/test_kernels_gpu.py::test_dropout_sweep_fused_matches_float64.  D_hat is NaN-filled (every element is written), the
    column sums and DV_next are zeroed as the header asks.  The sums are float64 atomics: no bits are promised."""
    from test_kernels_gpu import check_dropout_sweep
    nbytes = 4 * int(lib.oriana_dropout_sweep_scratch_floats(m, K))
    for variant in VARIANTS:
        scr, c0 = _scratch(nbytes, variant, F32, lambda s: check_dropout_sweep(n, m, K, with_next, arithmetic, s, seed=1))
        D, c1 = guarded_out((n, m), F32, 'nan')
        cs, c2 = guarded_out((m,), F64, 'zero')
        DV, c3 = guarded_out((n, K), F64, 'zero')
        d, s, dv = check_dropout_sweep(n, m, K, with_next, arithmetic, scr, bufs=(D, cs, DV))
        _all_checks((c0, c1, c2, c3), variant)
        assert np.isfinite(d).all() and np.isfinite(s).all() and (dv is None or np.isfinite(dv).all()), variant
        if not with_next:
            assert not DV.any(), variant                              # not the entry's to touch


@ARITH
@pytest.mark.parametrize('n,m,K', ZI_SHAPES, ids=ZI_IDS)
def test_dense_t_times_factor(lib, n, m, K, arithmetic):
    """oriana_dense_t_times_factor_f32 under the assertions of tests/test_kernels_gpu.py::test_dense_t_times_factor_f32 (float64
    atomics: no bits are promised)."""
    from test_kernels_gpu import check_dense_t
    nbytes = 4 * int(lib.oriana_dense_t_scratch_floats(n, K))
    for variant in VARIANTS:
        scr, c0 = _scratch(nbytes, variant, F32, lambda s: check_dense_t(n, m, K, arithmetic, s, seed=1))
        out, c1 = guarded_out((m, K), F64, 'zero')
        got = check_dense_t(n, m, K, arithmetic, scr, out=out)
        _all_checks((c0, c1), variant)
        assert np.isfinite(got).all() and np.isfinite(out.cpu().numpy()).all(), variant


def test_unaligned_d_hat_fallback(lib):
    """(300, 260, 100) with a D_hat 4 bytes off a 16-byte boundary: the float32 instruction's kernels run on the scratch the tiles
    family has just used (tests/test_kernels_gpu.py::test_dense_zi_kernels_decline_unaligned_buffers)."""
    from test_kernels_gpu import UNALIGNED_SHAPE, check_unaligned_fallback
    n, m, K = UNALIGNED_SHAPE
    b1, b2 = 4 * int(lib.oriana_dropout_sweep_scratch_floats(m, K)), 4 * int(lib.oriana_dense_t_scratch_floats(n, K))
    for variant in VARIANTS:
        lgs, c0 = guarded_variant(b1, variant, F32, DEV)
        dts, c1 = guarded_variant(b2, variant, F32, DEV)
        if variant == 'stale':
            check_unaligned_fallback(lgs, dts, seed=1)
        outs = check_unaligned_fallback(lgs, dts)
        _all_checks((c0, c1), variant)
        assert all(np.isfinite(o).all() for o in outs), variant


def _rate_inputs(n, m, K):
    """As the rate_case of tests/test_zi_foldin_gpu.py without a fitted model: Gamma(1) factors scaled to Lambda of order 1, one
    pi_d at 0 and one at 1, 20 % non-zeros; the reference is d.astype(float32) @ V in float64."""
    import zi_foldin_reference as zr
    rng = np.random.default_rng(n + 3 * m + 11 * K)
    V = rng.gamma(1.0, 1.0, size=(m, K))
    pi_d = rng.uniform(0.05, 0.95, size=m)
    pi_d[min(7, m - 1)], pi_d[min(9, m - 2)] = 0.0, 1.0
    X = ((rng.poisson(3.0, size=(n, m)) + 1) * (rng.random((n, m)) < 0.2)).astype(np.float64)
    U = rng.gamma(1.0, 1.0, size=(n, K))
    U /= (U @ V.T).mean()
    d = zr.dropout_f32(X, V, pi_d, U)
    assert ((d > 0.01) & (d < 0.99)).mean() > 0.2, 'the case does not exercise the sigmoid'
    return X, U, V, pi_d, d.astype(np.float64) @ V


@ARITH
@pytest.mark.parametrize('n,m,K', ZI_SHAPES, ids=ZI_IDS)
def test_zi_foldin_rate(lib, n, m, K, arithmetic):
    """oriana_zi_foldin_rate under the assertions of tests/test_zi_foldin_gpu.py (test_rate_against_float64 and
    test_rate_skips_inactive_cells), `active` marking one whole row block (256, 128, 32 or 16 cells: the largest below n) and one
    cell more inactive.  DV is zeroed as the header asks, the inactive run's holds the sentinel of that test."""
    from test_zi_foldin_gpu import check_rate, check_rate_skips_inactive
    X, U, V, pi_d, ref = _rate_inputs(n, m, K)
    act = np.ones(n, dtype=np.uint8)
    act[:max(b for b in (256, 128, 32, 16) if b < n)] = 0
    act[n - 2] = 0
    nbytes = 4 * int(lib.oriana_dropout_sweep_scratch_floats((m + 3) // 4 * 4, K))
    for variant in VARIANTS:
        scr, c0 = _scratch(nbytes, variant, F32, lambda s: check_rate(X[::-1].copy(), U[::-1].copy(), V, pi_d, ref[::-1], arithmetic, s))
        DV, c1 = guarded_out((n, K), F64, 'zero')
        got = check_rate(X, U, V, pi_d, ref, arithmetic, scratch=scr, DV=DV)
        DV2, c2 = guarded_out((n, K), F64, 'zero')
        on = check_rate_skips_inactive(X, U, V, pi_d, act, arithmetic, scratch=scr, DV=DV2)
        _all_checks((c0, c1, c2), variant)
        assert np.isfinite(got).all() and np.isfinite(on).all(), variant


# ---- the geometry entries (csrc/kmeans.hip, csrc/knn.hip, csrc/silhouette.hip) -------------------------------------------------
def _dev(Y, extra=0):
    """Y on the device, optionally as the leading columns of a wider matrix (row stride d + extra) whose other columns are NaN."""
    n, d = Y.shape
    if not extra:
        return torch.from_numpy(Y).cuda()
    wide = torch.full((n, d + extra), float('nan'), dtype=torch.float32, device=DEV)
    wide[:, :d] = torch.from_numpy(Y).cuda()
    return wide[:, :d]


def _case(cases, name):
    return next(c for c in cases if c[0] == name)


# (case of kr.STEP_CASES, blocks or None for the case's own): d = 1 pads the centre image (the smallest case), d = 20 does not and
# leaves one row in the second tile, 63 rows leave the only tile partial, five tiles in three blocks
KMEANS_PICKS = [('one_row', None), ('tile_plus', None), ('tile_minus', None), ('d65_stride', None), ('five_tiles_two_blocks', 3)]


def _kmeans_raw(lib, Yd, cen, scratch, blocks, label_restart):
    """oriana_kmeans_step into guarded outputs: ({name: array}, checks)."""
    from oriana_amd._lib import call, ptr, stream_ptr
    n, d = int(Yd.shape[0]), int(Yd.shape[1])
    R, C = cen.shape[:2]
    ldy = int(Yd.stride(0)) if n > 1 else d
    bufs = {'sums': guarded_out((R, C, d), F64, 'nan'), 'counts': guarded_out((R, C), I64, 'nan'),
            'inertia': guarded_out((R,), F64, 'nan'), 'labels': guarded_out((n,), I32, 'nan'), 'mind': guarded_out((R, n), F32, 'nan')}
    o = {k: v[0] for k, v in bufs.items()}
    call('oriana_kmeans_step', ptr(Yd), n, d, ldy, ptr(torch.from_numpy(cen).cuda()), C, R, ptr(o['sums']), ptr(o['counts']),
         ptr(o['inertia']), ptr(o['labels']), int(label_restart), ptr(o['mind']), ptr(scratch), int(blocks), stream_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}, [v[1] for v in bufs.values()]


@pytest.mark.parametrize('name,blocks', KMEANS_PICKS, ids=['%s-%s' % p for p in KMEANS_PICKS])
def test_kmeans_step(lib, name, blocks):
    """oriana_kmeans_step under tests/test_kmeans_gpu.py::_check_restart for every restart; deterministic, no atomics: the outputs
    of the three fills are the same bit for bit."""
    from oriana_amd import cluster
    from test_kmeans_gpu import _check_restart
    case = _case(kr.STEP_CASES, name)
    _, n, d, C, R, extra, own = kr.resolve_case(case, lib)
    blocks = own if blocks is None else blocks
    Y, cen = kr.case_inputs(case, lib)
    Yd = _dev(Y, extra)
    other = _dev(Y[::-1].copy(), extra)
    nbytes = int(lib.oriana_kmeans_scratch_bytes(n, d, C, R, blocks))
    assert nbytes >= 0
    T = cluster.partial_rows()
    runs = {}
    for variant in VARIANTS:
        scr, c0 = _scratch(nbytes, variant, torch.uint8, lambda s: _kmeans_raw(lib, other, cen[:, ::-1].copy(), s, blocks, 0))
        out, checks = _kmeans_raw(lib, Yd, cen, scr, blocks, R - 1)
        _all_checks([c0] + checks, variant)
        assert all(np.isfinite(out[k]).all() for k in ('sums', 'inertia', 'mind')), variant
        for r in range(R):
            if r == R - 1:
                _check_restart(Y, cen[r], out, out['labels'], r, T, '%s %s' % (name, variant))
            else:                               # (the labels of the other restarts: by a call of their own on the same scratch)
                o2, ch2 = _kmeans_raw(lib, Yd, cen, scr, blocks, r)
                _all_checks([c0] + ch2, variant)
                for k in ('sums', 'counts', 'inertia', 'mind'):
                    assert np.array_equal(o2[k], out[k]), k
                _check_restart(Y, cen[r], o2, o2['labels'], r, T, '%s %s' % (name, variant))
        runs[variant] = tuple(out[k] for k in ('sums', 'counts', 'inertia', 'labels', 'mind'))
    _same_bits(runs, name)


# padded image at n = 1 (the smallest) and at d = 65 with stride 68 and a partial query tile, Y itself as the image with one
# query in the second tile, five tiles (stride 104: Y itself) over three candidate ranges
KNN_PICKS = [('one_row', 0), ('cand71', 0), ('tile_plus', 0), ('five_tiles_stride', 3), ('queries', 0)]


def _knn_raw(lib, Qd, Yd, k, exclude, scratch, blocks):
    from oriana_amd._lib import call, ptr, stream_ptr
    nq, n, d = int(Qd.shape[0]), int(Yd.shape[0]), int(Yd.shape[1])
    ldq, ldy = (int(Qd.stride(0)) if nq > 1 else d), (int(Yd.stride(0)) if n > 1 else d)
    idx, c1 = guarded_out((nq, k), I32, 'nan')
    d2, c2 = guarded_out((nq, k), F32, 'nan')
    call('oriana_knn', ptr(Qd), nq, ldq, 0, ptr(Yd), n, ldy, 0, d, k, 1 if exclude else 0, 0, ptr(idx), ptr(d2), ptr(scratch),
         int(blocks), stream_ptr())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy(), [c1, c2]


@pytest.mark.parametrize('name,blocks', KNN_PICKS, ids=['%s-%d' % p for p in KNN_PICKS])
def test_knn(lib, name, blocks):
    """oriana_knn under tests/knn_reference.py::check (tests/test_knn_gpu.py::test_single_call); one writer per list and a fixed
    order: the outputs of the three fills are the same bit for bit."""
    case = _case(nr.CASES, name)
    _, n, d, k, extra, nq = nr.resolve_case(case, lib)
    Y, Q = nr.case_inputs(case)
    Yd = _dev(Y, extra)
    Qd = Yd if Q is None else _dev(Q, extra)
    other = _dev(Y[::-1].copy(), extra)
    assert other.stride(0) == Yd.stride(0)
    nbytes = int(lib.oriana_knn_scratch_bytes_for(Qd.shape[0], n, d, k, blocks, Yd.data_ptr(), int(Yd.stride(0)) if n > 1 else d))
    assert 0 <= nbytes <= int(lib.oriana_knn_scratch_bytes(Qd.shape[0], n, d, k, blocks))
    runs = {}
    for variant in VARIANTS:
        scr, c0 = _scratch(max(nbytes, 16), variant, torch.uint8,
                           lambda s: _knn_raw(lib, other[:Qd.shape[0]] if Q is not None else other, other, k, Q is None, s, blocks))
        idx, d2, checks = _knn_raw(lib, Qd, Yd, k, Q is None, scr, blocks)
        _all_checks([c0] + checks, variant)
        assert not np.isnan(d2).any(), variant
        share = nr.check(Y, idx, d2, k, Q=Q, exclude=Q is None, what='%s %s' % (name, variant))
        assert share <= nr.NEAR_TIE_CAP
        runs[variant] = (idx, d2)
    _same_bits(runs, name)


# padded image at d = 5 with one row in the second query tile (the smallest), Y itself as the image (with a cluster without rows),
# stride 25 with a partial tile, seven clusters over three candidate ranges
SUMS_PICKS = [('one_row_tile', 0), ('edges', 0), ('stride25', 0), ('image_is_y', 3)]


def _sums_raw(lib, Yg, off, C, scratch, blocks):
    from oriana_amd._lib import call, ptr, stream_ptr
    n, d = int(Yg.shape[0]), int(Yg.shape[1])
    ld = int(Yg.stride(0)) if n > 1 else d
    S, c1 = guarded_out((C, n), F64, 'nan')
    call('oriana_cluster_distance_sums', ptr(Yg), n, ld, ptr(Yg), n, ld, d, off.ctypes.data, C, ptr(S), n, 0, ptr(scratch),
         int(blocks), stream_ptr())
    torch.cuda.synchronize()
    return S.cpu().numpy(), [c1]


@pytest.mark.parametrize('name,blocks', SUMS_PICKS, ids=['%s-%d' % p for p in SUMS_PICKS])
def test_cluster_distance_sums(lib, name, blocks):
    """oriana_cluster_distance_sums under tests/silhouette_reference.py::check_sums (tests/test_silhouette_gpu.py::
    test_single_call), the rows grouped by cluster serving as queries and candidates.  One writer per sum and an order fixed by the
    plan: the outputs of the three fills are the same bit for bit."""
    case = _case(sr.CASES, name)
    _, n, d, C, extra, _ = case
    Y, labels = sr.case_inputs(case)
    order = np.argsort(labels, kind='stable')
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=C))]).astype(np.int64))
    Yg = np.ascontiguousarray(Y[order])
    S_ref = sr.silhouette(Yg, labels[order], C)[0]
    Yd = _dev(Yg, extra)
    other = _dev(Yg[::-1] * np.float32(0.5), extra)
    nbytes = int(lib.oriana_cluster_distance_sums_scratch_bytes_for(n, n, d, C, blocks, Yd.data_ptr(), int(Yd.stride(0))))
    assert nbytes >= 0
    runs = {}
    for variant in VARIANTS:
        scr, c0 = _scratch(max(nbytes, 16), variant, torch.uint8, lambda s: _sums_raw(lib, other, off, C, s, blocks))
        S, checks = _sums_raw(lib, Yd, off, C, scr, blocks)
        _all_checks([c0] + checks, variant)
        sr.check_sums(S, S_ref, n, d, '%s %s' % (name, variant))
        runs[variant] = (S,)
    _same_bits(runs, name)


# ---- oriana_col_pass_det on the scratch engine.col_pass caches by byte count (csrc/passes.hip) ------------------------------------
@pytest.fixture(scope='module')
def eng():
    from oriana_amd import engine
    return engine


@pytest.mark.parametrize('K,m', [(100, 700), (20, 530), (200, 300)])
def test_col_pass_det(eng, K, m):
    """The deterministic column pass under tests/test_kernels_gpu.py::test_deterministic_column_pass, the tensor cached in
    engine._det_scratch replaced by a guarded view of the same byte count.  Per-item slabs and an ordered reduction: the results
    of the three fills are the same bit for bit."""
    from test_kernels_gpu import check_deterministic_column_pass
    runs = {}
    try:
        for variant in VARIANTS:
            checks = []

            def scratch(nbytes, install, warm):
                view, check = guarded_variant(nbytes, variant, F32, DEV)
                install(view)
                if variant == 'stale':
                    warm()
                    check('the call that leaves the stale contents')
                checks.append(check)
            Zi, Zj = check_deterministic_column_pass(eng, K, m, scratch=scratch)
            assert len(checks) == 1
            _all_checks(checks, variant)
            assert np.isfinite(Zi).all() and np.isfinite(Zj).all(), variant
            runs[variant] = (Zi, Zj)
    finally:
        eng._det_scratch.clear()
    _same_bits(runs, 'K=%d m=%d' % (K, m))


# ---- the stateless nests on a workspace of the documented minimum (csrc/stateless.hip) ---------------------------------------
NESTS = ['gap', 'zigap-quirk', 'zigap', 'sparse_gap', 'sparse_zigap']
_nest_cases = {}


def _nest_case(K):
    """n = 300, m = 260: the inputs of tests/test_kernels_gpu.py::test_variant_dropins_general_D (a general D_hat, slow-path entries)
    and the oracle's outputs of the five calls -- computed once per K, only read."""
    from oracle import cavi_oracle as co
    from test_kernels_gpu import _rand_counts
    if K not in _nest_cases:
        rng = np.random.default_rng(11 + K)
        n, m = 300, 260
        X = _rand_counts(rng, n, m, 0.2).astype(np.float32)
        lu = rng.normal(size=(n, K)).astype(np.float32)
        lv = rng.normal(size=(m, K)).astype(np.float32)
        lu[3] = -1e15
        lv[7] -= 70.0
        D = rng.random((n, m)).astype(np.float32)
        ps = rng.random((m, K))
        St, Sh = (ps > 0.4).astype(np.float32), ps.astype(np.float32)
        refs = {}
        for nest in NESTS:
            r = [np.empty((n, K), np.float32), np.empty((m, K), np.float32), np.empty((m, K), np.float32)]
            if nest == 'gap':
                co.zq_gap(r[0], r[1], lu, lv, X)
                r = r[:2]
            elif nest.startswith('zigap'):
                co.zq_zigap(r[0], r[1], r[2], lu, lv, D, X, quirk=nest == 'zigap-quirk')
            elif nest == 'sparse_gap':
                co.zq_sparse_gap(r[0], r[1], r[2], lu, lv, St, Sh, X)
            else:
                co.zq_sparse_zigap(r[0], r[1], r[2], lu, lv, St, Sh, D, X)
            refs[nest] = r
        _nest_cases[K] = (dict(X=X, lu=lu, lv=lv, D=D, St=St, Sh=Sh), refs)
    return _nest_cases[K]


def _nest_call(nest, t, outs, ws, n, m, K):
    from oriana_amd._lib import call, ptr, stream_ptr
    base, nbytes, st = ws.data_ptr(), ws.numel(), stream_ptr()
    o = [ptr(x) for x in outs]
    if nest == 'gap':
        call('oriana_zq_gap_f32', o[0], o[1], ptr(t['lu']), ptr(t['lv']), ptr(t['X']), n, m, K, base, nbytes, st)
    elif nest.startswith('zigap'):
        call('oriana_zq_zigap_f32', o[0], o[1], o[2], ptr(t['lu']), ptr(t['lv']), ptr(t['D']), ptr(t['X']), n, m, K,
             1 if nest == 'zigap-quirk' else 0, base, nbytes, st)
    elif nest == 'sparse_gap':
        call('oriana_zq_sparse_gap_f32', o[0], o[1], o[2], ptr(t['lu']), ptr(t['lv']), ptr(t['St']), ptr(t['Sh']), ptr(t['X']),
             n, m, K, base, nbytes, st)
    else:
        call('oriana_zq_sparse_zigap_f32', o[0], o[1], o[2], ptr(t['lu']), ptr(t['lv']), ptr(t['St']), ptr(t['Sh']), ptr(t['D']),
             ptr(t['X']), n, m, K, base, nbytes, st)
    torch.cuda.synchronize()


@pytest.mark.parametrize('nest', NESTS)
@pytest.mark.parametrize('K', [20, 64, 100])
def test_stateless_nests(lib, K, nest):
    """The four oriana_zq_*_f32 entries (oriana_zq_zigap_f32 with both values of reference_quirks) on a workspace of exactly
    oriana_zq_workspace_bytes(n, m, K, nnz) bytes, nnz the true count of non-zeros -- engine._stateless_ws adds 64 records and 256
    bytes --, under the comparison of tests/test_kernels_gpu.py with oracle.cavi_oracle (assert_close_to_oracle).  The outputs are
    NaN-filled: the callee zero-fills them.

    The `nan` fill puts -1 into every integer array of WsLayout.  It runs because each of them is cleared or wholly written before
    its first read with n, m > 0 (csrc/stateless.hip, pack_nest.h, pack.hip): k_pack_count writes tile_nnz / tile_rslots /
    tile_cslots [t] and all 17 entries of rslice / cslice [t] for every tile t; k_scan_tiles writes roff / coff [0 .. nt]; `totals`
    is never used (the totals travel through a host array); rowrec, ridx, s_cs and -- where the nest reads them -- w_nz, sw_cs
    and s_rs are cleared by hipMemsetAsync in `place` before the fill pass; tile_flag is on the clear list of the factor
    preparation.  The `stale` fill comes from a matrix with the same non-zero pattern and other values, on other factors."""
    from test_kernels_gpu import assert_close_to_oracle
    host, refs = _nest_case(K)
    n, m = host['X'].shape
    t = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    other = dict(t, X=t['X'] * 3.0, lu=t['lu'].flip(0).contiguous(), lv=t['lv'].flip(0).contiguous())
    nnz = int(np.count_nonzero(host['X']))
    nbytes = int(lib.oriana_zq_workspace_bytes(n, m, K, nnz))
    assert nbytes > 0 and nbytes % 256 == 0
    shapes = [(n, K), (m, K), (m, K)][:len(refs[nest])]
    for variant in VARIANTS:
        ws, c0 = _scratch(nbytes, variant, torch.uint8,
                          lambda w: _nest_call(nest, other, [torch.empty(s, device=DEV) for s in shapes], w, n, m, K))
        bufs = [guarded_out(s, F32, 'nan') for s in shapes]
        outs = [b[0] for b in bufs]
        _nest_call(nest, t, outs, ws, n, m, K)
        _all_checks([c0] + [b[1] for b in bufs], variant)
        for got, ref in zip(outs, refs[nest]):
            assert np.array_equal(np.isfinite(got.cpu().numpy()), np.isfinite(ref)), variant
        assert_close_to_oracle(outs, refs[nest])


# ---- what a ZWorkspace promises between calls (oriana_amd/engine.py) ------------------------------------------------------------
def _padding_slots(ct):
    """(row-side, column-side) boolean masks of the padding slots of the sliced layout: the row-side slots without a record, the
    column-side slots that no record's cdst names and that are not among the 64 write-only slots at the end of a tile's range."""
    h = ct.host_arrays()
    rec = h['rec'][:ct.rslots]
    cpad = np.ones(ct.cslots, dtype=bool)
    for t in range(ct.nrb * ct.ncb):
        r = rec[h['roff'][t]:h['roff'][t + 1]]
        c0 = int(h['coff'][t])
        cpad[c0 + r['cdst'][r['x'] != 0].astype(np.int64)] = False
        end = c0 + int(h['cslice'][t, 16])
        assert end + 64 == h['coff'][t + 1]
        cpad[end:end + 64] = False
    return rec['x'] == 0, cpad


def _check_invariants(ws, pads, step, present):
    """"padding slots must stay 0" (s_cs, sw_cs, s_rs) and the columns K .. Kp of FU, FV and C.  `present`: the slot buffers the
    workspace must hold at this step -- every one of them is read back, none is skipped."""
    rpad, cpad = pads
    torch.cuda.synchronize()
    have = {name for name in ('s_cs', 'sw_cs', 's_rs') if getattr(ws, name) is not None}
    assert have == set(present), '%s: the workspace holds %s, the step expects %s' % (step, sorted(have), sorted(present))
    for name, pad in (('s_cs', cpad), ('sw_cs', cpad), ('s_rs', rpad)):
        if name in have:
            got = getattr(ws, name).cpu().numpy()
            assert got.size == pad.size and pad.any()
            assert not got[pad].any(), '%s: padding slots of %s are not 0' % (step, name)
    for name in ('FU', 'FV', 'C'):
        assert not getattr(ws, name)[:, ws.K:].any(), '%s: columns K .. Kp of %s' % (step, name)


def _flags(ws):
    """tile_flag and, on a hybrid layout, dn_flag of a workspace, on the host."""
    torch.cuda.synchronize()
    return [getattr(ws, name).cpu().numpy().copy() for name in ('tile_flag', 'dn_flag') if getattr(ws, name, None) is not None]


@pytest.mark.parametrize('K', [20, 33, 64, 100])
@pytest.mark.parametrize('layout', ['sliced', 'hybrid'])
def test_workspace_history(eng, layout, K, monkeypatch):
    """One ZWorkspace, in the deterministic mode, through
      1. the plain nest;
      2. the dq nest;
      3. the sparse nest with a dead gene, in the form the engine picks (fused row pass up to Kp = 64) and then with
         engine._FUSE_SPARSE_ROWS = False, the form that writes s_rs at every K;
      4. sliced layout only (a hybrid layout carries no per-entry weights: engine.zq refuses w_nz there, and its sw_cs never
         exists): the sparse nest with per-entry weights w_nz, the only one that writes sw_cs, on the plain factors and on the
         slow-path factors of step 5;
      5. the plain nest with a cell and a gene on the slow path (the shifts of
         tests/test_dense_gpu.py::test_dense_slow_path_rows_and_tiny_denominators);
      6. the first call again.
    After every step the slot buffers that must exist by then are asserted to exist (s_cs always; s_rs from the unfused sparse
    step on, and from the first sparse step on where Kp > 64; sw_cs from step 4 on, sliced only), the padding slots of each are
    read back and are 0, and the columns K .. Kp of FU, FV and C are 0 (K = 33 has Kp = 36: at 20, 64 and 100 there are no such
    columns).  tile_flag and dn_flag after the last call equal their values after the first: no flag of step 5 is left behind.

    Sliced layout: two fresh workspaces agree bit for bit, and the last result equals the first bit for bit.  Hybrid layout
    (dense_density = 0.3): NOT bit-reproducible on two fresh workspaces at any of the four K (measured; the dense-gene kernels add
    their partial sums with float atomics, csrc/dense_pass.hip), so its last result is judged with helpers.zlog_bound against the
    float64 nest cavi_oracle.zq_exact, as every loop-nest output is; the sliced one is held to that bound as well."""
    from helpers import err_colrel, zlog_bound
    from oracle import cavi_oracle as co
    rng = np.random.default_rng(100 * K + len(layout))
    n, m = 300, 260
    dens = np.full(m, 0.1)
    dens[::3] = 0.6
    X = ((rng.poisson(3.0, size=(n, m)) + 1) * (rng.random((n, m)) < dens)).astype(np.float32)
    lu = rng.normal(size=(n, K)).astype(np.float32)
    lv = rng.normal(size=(m, K)).astype(np.float32)
    lu2, lv2 = lu.copy(), lv.copy()
    lu2[5] += 35.0; lu2[17] -= 80.0; lv2[3] += 30.0; lv2[40] = -120.0
    dq = rng.random((n, K)).astype(np.float32)
    ps = rng.random((m, K))
    St, Sh = (ps > 0.3).astype(np.float32), ps.astype(np.float32)
    St[7] = 0
    D = rng.random((n, m)).astype(np.float32)
    c = lambda v: torch.from_numpy(v).cuda()
    sliced = layout == 'sliced'
    ct = eng.CountTiles.from_dense(c(X), DEV, side=c(D)) if sliced else eng.CountTiles.from_dense(c(X), DEV, dense_density=0.3)
    assert ct.dense is None if sliced else (ct.gd >= 32 and ct.ms > 0)
    pads = _padding_slots(ct)
    assert pads[0].any() and pads[1].any()
    ws = eng.ZWorkspace(ct, K)
    new = lambda: [torch.empty(n, K, device=DEV), torch.empty(m, K, device=DEV), torch.empty(m, K, device=DEV)]
    tlu, tlv, tlu2, tlv2 = c(lu), c(lv), c(lu2), c(lv2)

    def plain(w, a, b):
        o = new()
        eng.zq_gap(w, o[0], o[1], a, b)
        torch.cuda.synchronize()
        return o[0].cpu().numpy(), o[1].cpu().numpy()
    try:
        eng.set_deterministic(True)
        present = {'s_cs'}
        first = plain(ws, tlu, tlv)
        _check_invariants(ws, pads, 'plain', present)
        flags_first = _flags(ws)
        assert len(flags_first) == (1 if sliced else 2) and not any(f.any() for f in flags_first)
        o = new()
        eng.zq(ws, o[0], o[1], o[2], tlu, tlv, dq=c(dq))
        _check_invariants(ws, pads, 'dq', present)
        o = new()
        eng.zq(ws, o[0], o[1], o[2], tlu, tlv, S_tilde=c(St), S_hat=c(Sh))
        if ws.Kp > 64:
            present = present | {'s_rs'}
        _check_invariants(ws, pads, 'sparse', present)
        assert not o[1].cpu().numpy()[7].any()
        monkeypatch.setattr(eng, '_FUSE_SPARSE_ROWS', False)
        o = new()
        eng.zq(ws, o[0], o[1], o[2], tlu, tlv, S_tilde=c(St), S_hat=c(Sh))
        monkeypatch.undo()
        present = present | {'s_rs'}
        _check_invariants(ws, pads, 'sparse, second row product', present)
        assert not o[1].cpu().numpy()[7].any()
        if sliced:
            present = present | {'sw_cs'}
            for what, a, b in (('weighted sparse', tlu, tlv), ('weighted sparse, slow path', tlu2, tlv2)):
                o = new()
                eng.zq(ws, o[0], o[1], o[2], a, b, S_tilde=c(St), S_hat=c(Sh), w_nz=ct.side_nz)
                _check_invariants(ws, pads, what, present)
            assert int(ws.tile_flag.sum().item()) > 0, 'the weighted nest took no slow path'
        slow = plain(ws, tlu2, tlv2)
        assert int(ws.tile_flag.sum().item()) > 0, 'no tile took the slow path'
        assert sliced or int(ws.dn_flag.sum().item()) > 0, 'no dense tile took the slow path'
        _check_invariants(ws, pads, 'slow path', present)
        last = plain(ws, tlu, tlv)
        _check_invariants(ws, pads, 'plain again', present)
        for a, b in zip(flags_first, _flags(ws)):
            assert np.array_equal(a, b), 'a flag of the slow-path step is left behind'
        fresh = plain(eng.ZWorkspace(ct, K), tlu, tlv)
    finally:
        eng.set_deterministic(False)
    assert all(np.isfinite(a).all() for a in first + slow + last)
    reproducible = all(np.array_equal(a, b) for a, b in zip(first, fresh))
    print('%s K=%d: two fresh workspaces agree bit for bit: %s' % (layout, K, reproducible))
    if layout == 'sliced':
        assert reproducible
        assert np.array_equal(last[0], first[0]) and np.array_equal(last[1], first[1])
    r = [np.empty((n, K), np.float32), np.empty((m, K), np.float32)]
    co.zq_gap(r[0], r[1], lu, lv, X)
    exact = co.zq_exact(lu, lv, X)
    for name, got, ref, ex in zip(('Z_i', 'Z_j'), last, r, exact):
        d_hip, d_ref = err_colrel(got, ex), err_colrel(ref, ex)
        print('%s K=%d %s: HIP %.3e from exact, the reference arithmetic %.3e' % (layout, K, name, d_hip, d_ref))
        assert d_hip <= zlog_bound(d_ref), name
