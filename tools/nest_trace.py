# -*- coding: utf-8 -*-
"""The launch sequence of every C entry that runs a whole loop nest, for comparing two builds of the library.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/nest_trace.py run LABELS.txt
    python tools/nest_trace.py list DIR LABELS.txt > A.txt          # ordered (kernel, grid, block) per entry
    python tools/nest_trace.py diff A.txt B.txt                     # exit status 1 if any entry differs

`run` calls the four resident entries (unit-declared and general D_hat, with and without the index quirk of zigap.py:94 and
the third output, where the entry allows) on a sliced and a hybrid handle and the four stateless entries, at K = 20, 64, 100;
every call is preceded by a marker launch (oriana_trigamma_f64 over 256 * index elements) that `list` splits the trace at.
ORIANA_CUS=2 in the environment makes the plans of the small matrix split the last round (row split + dense tail).

    ... -- python tools/nest_trace.py passes LABELS.txt ;  python tools/nest_trace.py list DIR LABELS.txt lds

`passes` is the same for the kernel-level entries csrc/passes.hip dispatches by K: on one small sliced matrix, for one K per
padded width the library compiles (and K = 1), oriana_row_pass_general in its six variants x {no split, even whole-grid split,
last-round split with explicit edges}, oriana_row_spmm with and without weights, oriana_col_pass with and without a work list,
oriana_col_pass_dual and oriana_col_pass_det.  Return codes other than 0 are part of the record (the label ends in rc=...:
ORIANA_EKRANGE is how an entry says "not this form's K"); `list ... lds` adds the LDS bytes of every launch.  `passes-perf` runs the unsplit forms five times each on a 250,000 x 10,000 matrix,
for `rocprofv3 --kernel-trace --stats` (the mean duration of each kernel in two builds).

    ... -- python tools/nest_trace.py models LABELS.txt ;  python tools/nest_trace.py list DIR LABELS.txt

`models` is `run` for the Python sequencer (oriana_amd/engine.py): behind the same markers engine.zq_gap (whole, phase='rows' then
'cols', finalize_rows / finalize_cols = False, zj_packed with a recording on_segment -- the segments end up in the label) and
engine.zq (plain, dq, sparse, and sparse + w_nz on the sliced layout; with and without Z_log; whole and in two phases) on the
sliced and the hybrid layout of the same matrix at K = 20, 64, 100, then two step()s of each of the four model classes per layout.
ORIANA_CUS=2, ORIANA_DETERMINISTIC=1 and ORIANA_FORCE_SHARDED=1 (a one-rank gloo group: the packed-Z_j path of models/gap.py) in the
environment select the other forms of the sequence.  `list ... nocopy` drops the runtime's buffer copies (__amd_rocclr_copyBuffer):
under ORIANA_FORCE_SHARDED=1 the exchange issues them from its own threads, beside the sweep's stream, and their place in the
time-ordered listing changes from run to run.

    ... -- python tools/nest_trace.py dense LABELS.txt ;  python tools/nest_trace.py list DIR LABELS.txt lds

`dense` is `passes` for the dense matrix-core entries (csrc/dense_f32.hip, dense_zi.hip, dense_pass.hip, dense_mfma.hip), on one small
matrix.  oriana_dropout_sweep_fused_tiles and oriana_dense_t_times_factor_f32 for K = 1, one K per padded width up to 128 and K = 129,
with both `arithmetic` values, each in its full form and with one precondition of the first kernel family taken away at a time (no
per-lane flags, no V_next / DV_next, a gene count with m % 4 == 2, D_hat or the scratch 4 bytes off a 16-byte boundary, no scratch);
the forwarding entry oriana_dropout_sweep_fused; the values of the size entries (oriana_dropout_sweep_scratch_floats,
oriana_dense_t_scratch_floats, oriana_nzmask_tiles_words, oriana_dense_supported, oriana_dense_image_pieces) in the label;
oriana_dense_images2 (both sides), oriana_dense_row_pass_tail (unsplit, gene_splits > 1, tail_parts > 1) and oriana_dense_col_pass
(1 and several cell_splits) on the dense block of a hybrid layout for one K per padded width up to 100 and K = 112 (rc=-2);
oriana_dense_times_factor in both orientations for one K per NT case up to 256; oriana_dropout_update_fused and
oriana_dropout_metric at three K; oriana_dense_metric on the same dense block.  Every call is valid for its entry: a refusal is a return code of host-side validation.  ORIANA_CUS=2
in the environment moves the split pickers (both read oriana_device_cus()).
"""
import csv
import ctypes
import difflib
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(labels_path):
    import numpy as np
    import torch
    from oriana_amd import _lib
    from oriana_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    st = stream_ptr()
    labels = []
    mark_in = torch.ones(256 * 400, dtype=torch.float64, device='cuda')
    mark_out = torch.empty_like(mark_in)

    def entry(label, fn, *args):
        torch.cuda.synchronize()
        labels.append(label)
        assert lib.oriana_trigamma_f64(ptr(mark_out), ptr(mark_in), 256 * len(labels), st) == 0
        rc = fn(*args)
        assert rc == 0, (label, rc)
        torch.cuda.synchronize()

    n, m = 1700, 1100
    for K in (20, 64, 100):
        rng = np.random.default_rng(K)
        dens = rng.beta(1.0, 3.0, size=m)
        X = (rng.poisson(3.0, size=(n, m)) * (rng.random((n, m)) < dens[None, :])).astype(np.float32)
        D = rng.random((n, m)).astype(np.float32)
        D[X != 0] = 1.0
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        Xd, Dd, Dg = d(X), d(D), d(rng.random((n, m)))
        lu, lv = d(rng.normal(size=(n, K))), d(rng.normal(size=(m, K)))
        St, Sh = d(rng.random((m, K)) < 0.7), d(rng.random((m, K)))
        Zi, Zj, Zl = (torch.empty(r, K, device='cuda') for r in (n, m, m))
        for layout, dd in (('sliced', 0.0), ('hybrid', 0.2)):
            h = ctypes.c_void_p(None)
            assert lib.oriana_counts_create_dense_f32(ctypes.addressof(h), ptr(Xd), n, m, m, K, dd, st) == 0
            tag = 'K%d %s ' % (K, layout)
            entry(tag + 'gap_resident', lib.oriana_zq_gap_resident, h, ptr(Zi), ptr(Zj), ptr(lu), ptr(lv), st)
            for unit in (1, 0):
                if not unit and dd > 0:
                    continue                                      # (a hybrid handle serves the twins under the declaration only)
                assert lib.oriana_counts_declare_unit_dropout(h, unit) == 0
                w = tag + ('unit ' if unit else 'general ')
                Dx = Dd if unit else Dg
                for quirk in (0, 1):
                    for zl in (Zl, None):
                        entry(w + 'zigap_resident quirk=%d zlog=%d' % (quirk, zl is not None), lib.oriana_zq_zigap_resident, h, ptr(Zi),
                              ptr(Zj), ptr(zl), ptr(lu), ptr(lv), ptr(Dx), quirk, st)
                entry(w + 'sparse_gap_resident', lib.oriana_zq_sparse_gap_resident, h, ptr(Zi), ptr(Zj), ptr(Zl), ptr(lu), ptr(lv),
                      ptr(St), ptr(Sh), st)
                entry(w + 'sparse_zigap_resident', lib.oriana_zq_sparse_zigap_resident, h, ptr(Zi), ptr(Zj), ptr(Zl), ptr(lu), ptr(lv),
                      ptr(St), ptr(Sh), ptr(Dx), st)
            assert lib.oriana_counts_destroy(h) == 0
        nbytes = lib.oriana_zq_workspace_bytes(n, m, K, int(np.count_nonzero(X)))
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device='cuda')
        wp = (ws.data_ptr() + 255) // 256 * 256
        tag = 'K%d stateless ' % K
        entry(tag + 'gap_f32', lib.oriana_zq_gap_f32, ptr(Zi), ptr(Zj), ptr(lu), ptr(lv), ptr(Xd), n, m, K, wp, nbytes, st)
        for quirk in (0, 1):
            entry(tag + 'zigap_f32 quirk=%d' % quirk, lib.oriana_zq_zigap_f32, ptr(Zi), ptr(Zj), ptr(Zl), ptr(lu), ptr(lv), ptr(Dg),
                  ptr(Xd), n, m, K, quirk, wp, nbytes, st)
        entry(tag + 'sparse_gap_f32', lib.oriana_zq_sparse_gap_f32, ptr(Zi), ptr(Zj), ptr(Zl), ptr(lu), ptr(lv), ptr(St), ptr(Sh),
              ptr(Xd), n, m, K, wp, nbytes, st)
        entry(tag + 'sparse_zigap_f32', lib.oriana_zq_sparse_zigap_f32, ptr(Zi), ptr(Zj), ptr(Zl), ptr(lu), ptr(lv), ptr(St), ptr(Sh),
              ptr(Dg), ptr(Xd), n, m, K, wp, nbytes, st)
    entry('end', lambda: 0)
    with open(labels_path, 'w') as f:
        f.write('\n'.join(labels) + '\n')


def passes(labels_path, perf=False):
    import numpy as np
    import torch
    from oriana_amd import _lib, engine
    from oriana_amd._lib import OrianaRowSplit, ptr, stream_ptr
    lib = _lib.load()
    st = stream_ptr()
    labels = []
    mark_in = torch.ones(256 * 600, dtype=torch.float64, device='cuda')
    mark_out = torch.empty_like(mark_in)

    def probe(label, fn, *args):
        torch.cuda.synchronize()
        labels.append(label)
        assert lib.oriana_trigamma_f64(ptr(mark_out), ptr(mark_in), 256 * len(labels), st) == 0
        labels[-1] += ' rc=%d' % fn(*args)
        for _ in range(4 if perf else 0):         # (five launches per kernel for `rocprofv3 --stats`)
            fn(*args)
        torch.cuda.synchronize()

    if perf:      # kernel durations of two builds: a matrix on which a pass runs for milliseconds, the unsplit forms only
        n, m = 250000, 10000
        torch.manual_seed(8)
        X = torch.poisson(torch.full((n, m), 3.0, device='cuda')) * (torch.rand(n, m, device='cuda') < 0.08)
    else:
        n, m = 1700, 1100
        rng = np.random.default_rng(8)
        dens = rng.beta(1.0, 3.0, size=m)
        X = (rng.poisson(3.0, size=(n, m)) * (rng.random((n, m)) < dens[None, :])).astype(np.float32)
    ct = engine.CountTiles.from_dense(X, device='cuda')
    cs, nrb, ncb = ct.sparse_struct, ct.nrb, ct.ncb
    even = OrianaRowSplit(0, 2, (ctypes.c_int32 * 9)(-1))
    last = OrianaRowSplit(nrb - 2, 2, (ctypes.c_int32 * 9)(0, 3, ncb))
    splits = (('none', None), ('even', ctypes.byref(even)), ('last-round', ctypes.byref(last)))[:1 if perf else 3]
    f32 = lambda *shape: torch.rand(*shape, device='cuda') + 0.5
    Ks = sorted({int(lib.oriana_kpad(K)) for K in range(1, 257)} | {1})
    for K in Ks:
        Kp = int(lib.oriana_kpad(K))
        FU, FV, FV2 = f32(nrb * 256, Kp), f32(ncb * 256, Kp), f32(ncb * 256, Kp)
        R = torch.zeros(8 * nrb * 256, Kp, device='cuda')
        C1, C2 = torch.zeros(ncb * 256, Kp, device='cuda'), torch.zeros(ncb * 256, Kp, device='cuda')
        s_cs, sw_cs = f32(max(ct.cslots, 1)), f32(max(ct.cslots, 1))
        s_rs, w_nz = f32(max(ct.rslots, 1)), f32(max(ct.rslots, ct.cslots, 1))
        flag = torch.zeros(nrb * ncb, dtype=torch.int32, device='cuda')
        variants = (('plain', None, None, None, None), ('s_rs', None, None, None, s_rs), ('w_nz', None, w_nz, sw_cs, None),
                    ('w_nz+s_rs', None, w_nz, sw_cs, s_rs), ('FV2', FV2, None, None, None), ('FV2+w_nz', FV2, w_nz, sw_cs, None))
        for vname, f2, w, sw, srow in variants:
            for sname, sp in splits:
                probe('K%d row_pass %s split=%s' % (K, vname, sname), lib.oriana_row_pass_general, cs, ptr(FU), ptr(FV), ptr(f2),
                      ptr(w), ptr(R), ptr(s_cs), ptr(sw), ptr(srow), ptr(flag), K, sp, None, st)
        for w in (None, w_nz):
            probe('K%d row_spmm w_nz=%d' % (K, w is not None), lib.oriana_row_spmm, cs, ptr(s_rs), ptr(w), ptr(FV), ptr(R), K, st)
        work, work1 = ct.col_work_for(K), ct.col_work_width(1)
        if perf:
            probe('K%d col_pass work' % K, lib.oriana_col_pass, cs, ptr(s_cs), ptr(FU), ptr(C1), K, ptr(work), work.shape[0], st)
            continue
        probe('K%d col_pass bands' % K, lib.oriana_col_pass, cs, ptr(s_cs), ptr(FU), ptr(C1), K, None, 0, st)
        probe('K%d col_pass work' % K, lib.oriana_col_pass, cs, ptr(s_cs), ptr(FU), ptr(C1), K, ptr(work), work.shape[0], st)
        probe('K%d col_pass_dual' % K, lib.oriana_col_pass_dual, cs, ptr(s_cs), ptr(FU), ptr(FU), ptr(C1), ptr(C2), K, ptr(work1),
              work1.shape[0], st)
        scratch = torch.empty(int(lib.oriana_col_pass_det_scratch_bytes(K, work.shape[0])) // 4 + 1, device='cuda')
        probe('K%d col_pass_det' % K, lib.oriana_col_pass_det, cs, ptr(s_cs), ptr(FU), ptr(C1), K, ptr(work), work.shape[0], ptr(scratch), st)
    probe('end', lambda: 0)
    with open(labels_path, 'w') as f:
        f.write('\n'.join(labels) + '\n')


def models(labels_path):
    import tempfile
    import numpy as np
    import torch
    import oriana_amd.models as M
    from oriana_amd import _lib, engine
    from oriana_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    st = stream_ptr()
    labels = []
    mark_in = torch.ones(256 * 400, dtype=torch.float64, device='cuda')
    mark_out = torch.empty_like(mark_in)
    pg = None
    if os.environ.get('ORIANA_FORCE_SHARDED') == '1':
        import torch.distributed as dist
        dist.init_process_group('gloo', init_method='file://' + os.path.join(tempfile.mkdtemp(prefix='nest_trace_pg_'), 'rendezvous'), rank=0, world_size=1)
        pg = dist.group.WORLD

    def entry(label, *calls):
        torch.cuda.synchronize()
        labels.append(label)
        assert lib.oriana_trigamma_f64(ptr(mark_out), ptr(mark_in), 256 * len(labels), st) == 0
        for fn in calls:
            fn()
        torch.cuda.synchronize()

    n, m = 1700, 1100
    for K in (20, 64, 100):
        rng = np.random.default_rng(K)
        dens = rng.beta(1.0, 3.0, size=m)
        X = (rng.poisson(3.0, size=(n, m)) * (rng.random((n, m)) < dens[None, :])).astype(np.float32)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        Dg = d(rng.random((n, m)))
        lu, lv = d(rng.normal(size=(n, K))), d(rng.normal(size=(m, K)))
        St, Sh, dq = d(rng.random((m, K)) < 0.7), d(rng.random((m, K))), d(rng.random((n, K)))
        a1, b1 = rng.gamma(1.0, size=(n, K)), rng.gamma(1.0, size=(m, K))
        Zi, Zj, Zl = (torch.empty(r, K, device='cuda') for r in (n, m, m))
        for layout, dd in (('sliced', None), ('hybrid', 0.2)):
            if dd and not engine.dense_supported(K):
                continue
            ct = engine.CountTiles.from_dense(X, 'cuda', side=None if dd else Dg, dense_density=dd)
            assert (ct.gd > 0) == bool(dd) and ct.ms > 0
            ws = engine.ZWorkspace(ct, K)
            tag = 'K%d %s ' % (K, layout)
            gap = lambda **kw: engine.zq_gap(ws, Zi, Zj, lu, lv, **kw)
            entry(tag + 'zq_gap', gap)
            entry(tag + 'zq_gap rows+cols', lambda: gap(phase='rows'), lambda: gap(phase='cols'))
            entry(tag + 'zq_gap finalize_rows=finalize_cols=False', lambda: gap(finalize_rows=False, finalize_cols=False))
            segments = []
            entry(tag + 'zq_gap zj_packed', lambda: gap(zj_packed=True, on_segment=lambda lo, hi: segments.append((lo, hi))))
            labels[-1] += ' segments=%s' % (segments,)
            nests = [('plain', {}), ('dq', dict(dq=dq)), ('sparse', dict(S_tilde=St, S_hat=Sh))]
            if not dd:                                   # (a hybrid layout carries no per-entry weights)
                nests.append(('sparse+w_nz', dict(S_tilde=St, S_hat=Sh, w_nz=ct.side_nz)))
            for name, kw in nests:
                for zl in (Zl, None):
                    nest = lambda kw=kw, zl=zl, **ph: engine.zq(ws, Zi, Zj, zl, lu, lv, **kw, **ph)
                    entry(tag + 'zq %s zlog=%d' % (name, zl is not None), nest)
                    entry(tag + 'zq %s zlog=%d rows+cols' % (name, zl is not None), lambda: nest(phase='rows'),
                          lambda: nest(phase='cols'))
            for name in ('GaP', 'ZIGaP', 'SparseGaP', 'SparseZIGaP'):
                model = getattr(M, name)(X, k=K, init=(a1, b1), dense_density=dd or 0, process_group=pg)
                assert (model.counts.gd > 0) == bool(dd)
                entry(tag + name + '.step x2', model.step, model.step)
    entry('end')
    if pg is not None:
        torch.distributed.destroy_process_group()
    with open(labels_path, 'w') as f:
        f.write('\n'.join(labels) + '\n')


def dense(labels_path):
    import numpy as np
    import torch
    from oriana_amd import _lib, engine
    from oriana_amd._lib import ptr, stream_ptr
    lib = _lib.load()
    st = stream_ptr()
    labels = []
    mark_in = torch.ones(256 * 1200, dtype=torch.float64, device='cuda')
    mark_out = torch.empty_like(mark_in)

    def probe(label, fn, *args):
        torch.cuda.synchronize()
        labels.append(label)
        assert lib.oriana_trigamma_f64(ptr(mark_out), ptr(mark_in), 256 * len(labels), st) == 0
        labels[-1] += ' rc=%d' % fn(*args)
        torch.cuda.synchronize()

    n = 1700
    rng = np.random.default_rng(10)
    f64 = lambda *shape: torch.rand(*shape, dtype=torch.float64, device='cuda') + 0.25
    f32 = lambda *shape: torch.rand(*shape, device='cuda') + 0.5
    off4 = lambda t: t.data_ptr() + 4              # (every buffer handed over this way has room for it)
    widths = sorted({int(lib.oriana_kpad(K)) for K in range(1, 129)})
    assert widths == [16, 20, 32, 36, 48, 52, 64, 68, 80, 84, 96, 100, 112, 128]
    Ks = sorted([1, 50, 129] + widths)

    # ---- the two dense products of a ZI sweep
    for m in (1098, 1100):                            # m % 4 == 2: no 16-byte row pieces; then m % 4 == 0
        X = (rng.poisson(3.0, size=(n, m)) * (rng.random((n, m)) < 0.3)).astype(np.float32)
        Dbuf = torch.zeros(n * m + 4, device='cuda')
        Dbuf[:n * m] = torch.from_numpy(X).cuda().reshape(-1)
        mask = torch.zeros(((n + 31) // 32) * m, dtype=torch.int32, device='cuda')
        assert lib.oriana_nzmask_f32(ptr(mask), ptr(Dbuf), n, m, st) == 0
        words = int(lib.oriana_nzmask_tiles_words(n, m))
        tiles = torch.zeros(max(words, 4), dtype=torch.int32, device='cuda')
        assert lib.oriana_nzmask_tiles(ptr(tiles), ptr(mask), n, m, st) == 0
        pi, colsum = torch.rand(m, dtype=torch.float64, device='cuda') * 0.8 + 0.1, torch.zeros(m, dtype=torch.float64, device='cuda')
        probe('m%d nzmask_tiles_words=%d nzmask_tiles' % (m, words), lib.oriana_nzmask_tiles, ptr(tiles), ptr(mask), n, m, st)
        for K in Ks:
            U, V, Vn, DV, out = f64(n, K), f64(m, K), f64(m, K), torch.zeros(n, K, dtype=torch.float64, device='cuda'), torch.zeros(m, K, dtype=torch.float64, device='cuda')
            ssz, tsz = int(lib.oriana_dropout_sweep_scratch_floats(m, K)), int(lib.oriana_dense_t_scratch_floats(n, K))
            ss, ts = torch.zeros(ssz + 8, device='cuda'), torch.zeros(tsz + 8, device='cuda')
            assert ss.data_ptr() % 16 == 0 and ts.data_ptr() % 16 == 0 and Dbuf.data_ptr() % 16 == 0
            tag = 'm%d K%d ' % (m, K)
            probe(tag + 'sweep_scratch_floats=%d dense_t_scratch_floats=%d' % (ssz, tsz), lambda: 0)
            for arith in (0, 1):
                forms = [('full', {})]
                if m % 4 == 0:
                    forms += [('no-nztiles', dict(tiles=None)), ('no-V_next', dict(Vn=None, DV=None)), ('D_hat+4', dict(D=off4(Dbuf))),
                              ('scratch+4', dict(scratch=off4(ss))), ('scratch=NULL', dict(scratch=None))]
                for name, kw in forms:
                    a = dict(D=ptr(Dbuf), tiles=ptr(tiles), Vn=ptr(Vn), DV=ptr(DV), scratch=ptr(ss))
                    a.update(kw)
                    probe(tag + 'arith=%d sweep_fused_tiles %s' % (arith, name), lib.oriana_dropout_sweep_fused_tiles, a['D'], ptr(U), ptr(V),
                          ptr(pi), ptr(mask), a['tiles'], ptr(colsum), a['Vn'], a['DV'], a['scratch'], arith, n, m, K, st)
                probe(tag + 'arith=%d sweep_fused' % arith, lib.oriana_dropout_sweep_fused, ptr(Dbuf), ptr(U), ptr(V), ptr(pi), ptr(mask),
                      ptr(colsum), ptr(Vn), ptr(DV), ptr(ss), arith, n, m, K, st)
                forms = [('full', {})]
                if m % 4 == 0:
                    forms += [('D_hat+4', dict(D=off4(Dbuf))), ('scratch+4', dict(scratch=off4(ts))), ('scratch=NULL', dict(scratch=None))]
                for name, kw in forms:
                    a = dict(D=ptr(Dbuf), scratch=ptr(ts))
                    a.update(kw)
                    probe(tag + 'arith=%d dense_t_times_factor_f32 %s' % (arith, name), lib.oriana_dense_t_times_factor_f32, ptr(out), a['D'],
                          ptr(U), a['scratch'], arith, n, m, K, st)

    # ---- the float64 products and the exact D update / metric (dense_mfma.hip)
    D = Dbuf[:n * m]
    pi, colsum = torch.rand(m, dtype=torch.float64, device='cuda') * 0.8 + 0.1, torch.zeros(m, dtype=torch.float64, device='cuda')
    for K in (1, 16, 32, 48, 64, 80, 96, 112, 128, 129, 200, 256):
        U, V = f64(n, K), f64(m, K)
        for trans, W, rows in ((0, V, n), (1, U, m)):
            out = torch.zeros(rows, K, dtype=torch.float64, device='cuda')
            probe('K%d dense_times_factor trans=%d' % (K, trans), lib.oriana_dense_times_factor, ptr(out), ptr(D), ptr(W), n, m, K, trans, st)
    for K in (20, 100, 128):                          # (128: more than 64 KB of LDS)
        U, V = f64(n, K), f64(m, K)
        pd, out2 = torch.zeros(n, m, dtype=torch.float64, device='cuda'), torch.zeros(2, dtype=torch.float64, device='cuda')
        probe('K%d dropout_update_fused' % K, lib.oriana_dropout_update_fused, ptr(pd), ptr(D), ptr(U), ptr(V), ptr(pi), ptr(mask),
              ptr(colsum), n, m, K, st)
        probe('K%d dropout_metric' % K, lib.oriana_dropout_metric, ptr(out2), ptr(D), ptr(U), ptr(V), ptr(pi), ptr(mask), n, m, K, st)

    # ---- the dense genes of a hybrid layout (dense_pass.hip)
    dens = rng.beta(1.0, 3.0, size=m)
    X = (rng.poisson(3.0, size=(n, m)) * (rng.random((n, m)) < dens[None, :])).astype(np.float32)
    ct = engine.CountTiles.from_dense(X, 'cuda', dense_density=0.2)
    d = ct.dense
    assert d is not None and d.ngt >= 4
    nrows = d.nct * 32
    for K in [w for w in widths if w <= 100] + [112]:
        Kp = int(lib.oriana_kpad(K))
        pv, pu = int(lib.oriana_dense_image_pieces(K, 0)), int(lib.oriana_dense_image_pieces(K, 1))
        tag = 'K%d dense ' % K
        probe(tag + 'supported=%d image_pieces=%d,%d' % (lib.oriana_dense_supported(K), pv, pu), lambda: 0)
        FU, FV = f32(nrows, Kp), f32(d.gd, Kp)
        imgV, imgU = torch.zeros(max(d.ngt * pv * 4, 4), device='cuda'), torch.zeros(max((nrows // 32) * pu * 4, 4), device='cuda')
        S, flag = torch.zeros(d.nct * d.ngt * 1024, device='cuda'), torch.zeros(d.nct * d.ngt, dtype=torch.int32, device='cuda')
        R, C = torch.zeros(4 * nrows, Kp, device='cuda'), torch.zeros(d.gd, Kp, device='cuda')
        probe(tag + 'images2 side=0', lib.oriana_dense_images2, ptr(imgV), ptr(FV), None, d.gd, K, 0, st)
        probe(tag + 'images2 side=1', lib.oriana_dense_images2, ptr(imgU), ptr(FU), None, n, K, 1, st)
        for name, gsp, nfull, parts in (('unsplit', 1, 0, 1), ('gene_splits=3', 3, 0, 1), ('tail_parts=2', 1, 1, 2)):
            probe(tag + 'row_pass_tail ' + name, lib.oriana_dense_row_pass_tail, d.c_struct, ptr(FU), ptr(imgV), ptr(R), ptr(S), ptr(flag),
                  K, gsp, nfull, parts, None, st)
        for csp in (1, 5):
            probe(tag + 'col_pass cell_splits=%d' % csp, lib.oriana_dense_col_pass, d.c_struct, ptr(imgU), ptr(S), ptr(C), K, csp, st)
        sums = torch.zeros(2 * m + 6, dtype=torch.float64, device='cuda')      # colsum | colnnz | out2 | out4
        probe(tag + 'metric', lib.oriana_dense_metric, d.c_struct, ptr(f64(n, K)), ptr(f64(m, K)), None, None, ptr(sums), ptr(sums) + 8 * m,
              ptr(sums) + 16 * m, ptr(sums) + 16 * m + 16, K, st)
    probe('end', lambda: 0)
    with open(labels_path, 'w') as f:
        f.write('\n'.join(labels) + '\n')


def listing(trace_dir, labels_path, lds=False, nocopy=False):
    """One line per entry: its launches in order as `kernel grid/block` (dimensions of 1 dropped, hipMemsetAsync = memset)."""
    labels = open(labels_path).read().split('\n')
    rows = []
    for path in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        rows += list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    dims = lambda v: 'x'.join(str(x) for x in v if x != 1) or '1'
    out = []
    for r in rows:
        name = r['Kernel_Name'].split('(')[0].replace('void ', '').replace('oriana::', '').replace(', ', ',')
        name = name.replace('__amd_rocclr_fillBufferAligned', 'memset')
        block = [int(r['Workgroup_Size_' + a]) for a in 'XYZ']
        grid = [int(r['Grid_Size_' + a]) // max(bl, 1) for a, bl in zip('XYZ', block)]
        if name.startswith('at::native'):         # (torch's own fills between two entries)
            continue
        if nocopy and name.startswith('__amd_rocclr_copyBuffer'):
            continue
        if 'k_map_f64<1>' in name:
            if labels[grid[0] - 1].startswith('end'):
                break
            out.append([labels[grid[0] - 1]])
        elif out:
            out[-1].append('%s %s/%s' % (name, dims(grid), dims(block)) + (' lds=%s' % r.get('Group_Segment_Size', r.get('LDS_Block_Size')) if lds else ''))
    for e in out:
        print('%s: %s' % (e[0], ' | '.join(e[1:])))


def diff(a_path, b_path):
    load = lambda p: {l.split(': ', 1)[0]: l.split(': ', 1)[1].split(' | ') for l in open(p).read().split('\n') if ': ' in l}
    A, B = load(a_path), load(b_path)
    same, kinds = [], {}
    for k in A:
        if A[k] == B.get(k):
            same.append(k)
            continue
        d = '\n'.join('    ' + l for l in difflib.unified_diff(A[k], B.get(k, []), lineterm='', n=0) if l[:1] in '+-' and l[:3] not in ('---', '+++'))
        kinds.setdefault(d, []).append(k)
    print('same (%d): %s' % (len(same), '; '.join(same)))
    for d, ks in kinds.items():               # entries with the same removed (-) and added (+) launches, once
        print('DIFFERENT (%d): %s\n%s' % (len(ks), '; '.join(ks), d))
    print('%d entries, %d differ' % (len(A), len(A) - len(same)))
    return 1 if len(same) != len(A) or set(A) != set(B) else 0


if __name__ == '__main__':
    if sys.argv[1] == 'run':
        run(sys.argv[2])
    elif sys.argv[1] in ('passes', 'passes-perf'):
        passes(sys.argv[2], perf=sys.argv[1] == 'passes-perf')
    elif sys.argv[1] == 'models':
        models(sys.argv[2])
    elif sys.argv[1] == 'dense':
        dense(sys.argv[2])
    elif sys.argv[1] == 'list':
        listing(sys.argv[2], sys.argv[3], lds='lds' in sys.argv[4:], nocopy='nocopy' in sys.argv[4:])
    else:
        sys.exit(diff(sys.argv[2], sys.argv[3]))
