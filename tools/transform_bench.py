# -*- coding: utf-8 -*-
"""Times a fold-in (GaP.transform's loop, engine.fold_in) against the same loop composed from the entries that existed before
oriana_foldin_update: row phase + oriana_gamma_update_finalize_prep on throw-away (n', K) buffers.

Default: 65,536 x 30,000 new cells, K = 100, 90 % zeros (the benchmark's generator), 20 forced iterations (tol = 0) against
the gene side of a model fitted on `--fit-rows` cells of the same generator for `--fit-sweeps` sweeps.  Device events
around whole loops (after a warm-up loop of each form, the two forms alternating, `--reps` times), then one loop of each
form with per-launch events for the share spent outside the row pass.  Prints one JSON line; `--out` also writes it to a file.
`--zi`: the zero-inflated fold-in instead (main_zi below).  `--score`: one engine.cell_bounds call beside one fold-in iteration
(main_score below).  `--zi --score`: one engine.zi_cell_bounds call beside one ZI fold-in iteration (main_zi_score below).

    python tools/transform_bench.py --out profiles/transform_bench.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main_zi(args):
    """--zi: one iteration of ZIGaP.fold_in's loop (engine.fold_in_zi), and its rate launch -- oriana_zi_foldin_rate, which never
    stores the dropout posterior -- against the storing entry (oriana_dropout_sweep_fused_tiles on a scratch D_hat of the query, whose
    kernels this build compiles instruction for instruction as before the rate entry existed) on the same operands: the two
    launches alternate, device events around runs of `--iters` launches, `--reps` times, after a warm-up of both.

        python tools/transform_bench.py --zi --cells 16384 --genes 20000 --k 50 --out profiles/zi_foldin_bench_k50.json
    """
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('transform_bench needs a GPU: there is nothing to time without one')
    from oriana_amd import _lib, engine
    from oriana_amd._lib import call, ptr, stream_ptr
    from oriana_amd.models import ZIGaP
    from oriana_amd.singlecell import SyntheticCounts
    dev = torch.device('cuda', 0)
    nq, m, K, seed = args.cells, args.genes, args.k, 1234 + 1000 * 4
    gen = SyntheticCounts(args.fit_rows, m, K, seed=seed, device=dev, zero_inflation_level=args.zeros)
    counts = engine.CountTiles.from_chunks(args.fit_rows, m, gen.chunk, args.chunk_rows, dev, dense_density=None)
    a1, b1 = gen.initial_shapes()
    model = ZIGaP(counts, k=K, use_factors=False, init=(a1, b1), device=dev)
    del a1, b1
    model.fit(args.fit_sweeps)
    torch.cuda.synchronize()
    genq = SyntheticCounts(nq, m, K, seed=seed, device=dev, zero_inflation_level=args.zeros)
    ct = engine.CountTiles.from_chunks(nq, m, genq.chunk, args.chunk_rows, dev, dense_density=None)
    alpha1, alpha2, lv, V = model.alpha1.tensor, model.alpha2.tensor, model._log_V_hat, model._V_hat.contiguous()
    pi_d, arith = model.pi_d.tensor.contiguous(), model._matrix_arith
    ws = engine.ZWorkspace(ct, K)
    s1 = (alpha1[None, :] + engine.row_sums_over_k(ws, K).to(torch.float64)).contiguous()
    s2 = torch.clamp(alpha2 + V.sum(0), min=1e-15)[None, :].expand(nq, K).contiguous()

    def loop(timer=None):
        ws.timer = timer
        p1, p2 = s1.clone(), s2.clone()
        engine.fold_in_zi(ct, K, lv, V, pi_d, alpha1, alpha2, p1, p2, args.iters, 0.0, ws=ws, arithmetic=arith)
        ws.timer = None
        return p1, p2

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    p1, p2 = loop()                                                  # warm-up
    t_loop = [timed(loop) for _ in range(args.reps)]
    timer = engine.KernelTimer(prealloc=8 * args.iters)
    loop(timer)
    torch.cuda.synchronize()
    launches = {k: {'count': c, 'mean_ms': round(ms, 4)} for k, (c, ms) in timer.summary().items()}

    # ---- the rate launch alone, both forms on the operands of the loop's last iteration ---------------------------------------
    mp = (m + 3) // 4 * 4
    f64 = dict(dtype=torch.float64, device=dev)
    Vp, pip = torch.zeros(mp, K, **f64), torch.zeros(mp, **f64)
    Vp[:m].copy_(V)
    pip[:m].copy_(pi_d)
    U = (p1 / p2).contiguous()
    st = stream_ptr()
    lib = _lib.load()
    mask = torch.zeros(((nq + 31) // 32) * mp, dtype=torch.int32, device=dev)
    call('oriana_nzmask_counts', ptr(mask), ct.sparse_struct, mp, st)
    tiles = torch.zeros(max(int(lib.oriana_nzmask_tiles_words(nq, mp)), 4), dtype=torch.int32, device=dev)
    call('oriana_nzmask_tiles', ptr(tiles), ptr(mask), nq, mp, st)
    scratch = torch.zeros(int(lib.oriana_dropout_sweep_scratch_floats(mp, K)), dtype=torch.float32, device=dev)
    D = torch.empty(nq, mp, dtype=torch.float32, device=dev)
    cs = torch.zeros(mp, **f64)
    DV_a, DV_b = torch.zeros(nq, K, **f64), torch.zeros(nq, K, **f64)

    def no_store():
        for _ in range(args.iters):
            call('oriana_zi_foldin_rate', ptr(DV_a), ptr(U), ptr(Vp), ptr(pip), ptr(mask), ptr(tiles), None, ptr(scratch), arith,
                 nq, mp, K, st)

    def storing():
        for _ in range(args.iters):
            call('oriana_dropout_sweep_fused_tiles', ptr(D), ptr(U), ptr(Vp), ptr(pip), ptr(mask), ptr(tiles), ptr(cs), ptr(Vp),
                 ptr(DV_b), ptr(scratch), arith, nq, mp, K, st)
    no_store(); storing()                                            # warm-up; DV_a, DV_b hold `iters` sums each
    torch.cuda.synchronize()
    rel = float(((DV_a - DV_b).abs() / (DV_b.abs() + DV_b.abs().max(0, keepdim=True).values)).max())
    t_a, t_b = [], []
    for _ in range(args.reps):
        t_a.append(timed(no_store) / args.iters)
        t_b.append(timed(storing) / args.iters)
    out = {
        'device': torch.cuda.get_device_name(0), 'cells': nq, 'genes': m, 'k': K, 'nnz': int(ct.nnz), 'iters': args.iters,
        'fit_rows': args.fit_rows, 'fit_sweeps': args.fit_sweeps, 'reps': args.reps, 'arithmetic': arith,
        'loop_ms_per_iter': round(float(np.median(t_loop)) / args.iters, 4), 'loop_ms': [round(t, 3) for t in t_loop],
        'loop_launches': launches,
        'rate_no_store_ms': round(float(np.median(t_a)), 4), 'rate_storing_ms': round(float(np.median(t_b)), 4),
        'rate_no_store_all_ms': [round(t, 4) for t in t_a], 'rate_storing_all_ms': [round(t, 4) for t in t_b],
        'D_hat_bytes_not_allocated_by_fold_in': nq * mp * 4,
        'rate_no_store_vs_storing_colrel': rel,
        'note': 'rate_*: `iters` back-to-back launches between two device events, the two forms alternating; the storing form '
                'writes a scratch D_hat of the query and its column sums besides the same DV',
    }
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


def main_zi_score(args):
    """--zi --score: what scoring adds to a ZI fold-in -- E[log U] of the final pair + one engine.zi_cell_bounds call (the data
    path of --score, the query's non-zero mask, oriana_zi_cell_bound, oriana_gamma_kl_rows) beside one iteration of
    engine.fold_in_zi and its rate launch, on the operands of --zi.  Device events around the whole call / loop, `--reps` times
    after a warm-up of both, then one call and one loop with per-launch events.

        python tools/transform_bench.py --zi --score --cells 16384 --genes 20000 --k 50 --fit-rows 16384 --fit-sweeps 3 --iters 10
    """
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('transform_bench needs a GPU: there is nothing to time without one')
    from oriana_amd import engine
    from oriana_amd._lib import call, ptr, stream_ptr
    from oriana_amd.models import ZIGaP
    from oriana_amd.singlecell import SyntheticCounts
    dev = torch.device('cuda', 0)
    nq, m, K, seed = args.cells, args.genes, args.k, 1234 + 1000 * 4
    gen = SyntheticCounts(args.fit_rows, m, K, seed=seed, device=dev, zero_inflation_level=args.zeros)
    counts = engine.CountTiles.from_chunks(args.fit_rows, m, gen.chunk, args.chunk_rows, dev, dense_density=None)
    a1, b1 = gen.initial_shapes()
    model = ZIGaP(counts, k=K, use_factors=False, init=(a1, b1), device=dev)
    del a1, b1
    model.fit(args.fit_sweeps)
    torch.cuda.synchronize()
    genq = SyntheticCounts(nq, m, K, seed=seed, device=dev, zero_inflation_level=args.zeros)
    ct = engine.CountTiles.from_chunks(nq, m, genq.chunk, args.chunk_rows, dev, dense_density=None)
    alpha1, alpha2, lv, V = model.alpha1.tensor, model.alpha2.tensor, model._log_V_hat, model._V_hat.contiguous()
    pi_d, arith = model.pi_d.tensor.contiguous(), model._matrix_arith
    ws = engine.ZWorkspace(ct, K)
    s1 = (alpha1[None, :] + engine.row_sums_over_k(ws, K).to(torch.float64)).contiguous()
    s2 = torch.clamp(alpha2 + V.sum(0), min=1e-15)[None, :].expand(nq, K).contiguous()
    p1, p2 = s1.clone(), s2.clone()

    def loop(timer=None):
        ws.timer = timer
        p1.copy_(s1)
        p2.copy_(s2)
        engine.fold_in_zi(ct, K, lv, V, pi_d, alpha1, alpha2, p1, p2, args.iters, 0.0, ws=ws, arithmetic=arith)
        ws.timer = None

    lu = torch.empty(nq, K, dtype=torch.float32, device=dev)

    def score(timer=None):
        ws.timer = timer
        call('oriana_gamma_update', ptr(p1), ptr(p2), ptr(torch.empty_like(p2)), ptr(lu), None, None, None, None, None, None, None,
             None, None, nq, K, stream_ptr())
        t = engine.zi_cell_bounds(ct, K, p1, p2, lu, lv, V, pi_d, alpha1, alpha2, ws=ws)
        ws.timer = None
        return t

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    loop()
    t0 = score()                                                     # warm-up of both
    t_l, t_s = [], []
    for _ in range(args.reps):
        t_l.append(timed(loop))
        t_s.append(timed(score))
    same = bool(torch.equal(score(), t0))                            # (within one process the loop ends at one pair or reorders atomics)
    timer = engine.KernelTimer(prealloc=16)
    t = score(timer)
    torch.cuda.synchronize()
    launches = {k: {'count': c, 'mean_ms': round(ms, 4)} for k, (c, ms) in timer.summary().items()}
    timer = engine.KernelTimer(prealloc=8 * args.iters)
    loop(timer)
    torch.cuda.synchronize()
    loop_launches = {k: {'count': c, 'mean_ms': round(ms, 4)} for k, (c, ms) in timer.summary().items()}
    per_iter, sc = float(np.median(t_l)) / args.iters, float(np.median(t_s))
    out = {
        'device': torch.cuda.get_device_name(0), 'cells': nq, 'genes': m, 'k': K, 'nnz': int(ct.nnz), 'iters': args.iters,
        'fit_rows': args.fit_rows, 'fit_sweeps': args.fit_sweeps, 'reps': args.reps, 'arithmetic': arith,
        'fold_in_ms_per_iter': round(per_iter, 4), 'fold_in_loop_ms': [round(x, 3) for x in t_l],
        'score_ms': round(sc, 4), 'score_all_ms': [round(x, 3) for x in t_s],
        'score_over_one_iteration': round(sc / per_iter, 3), 'score_launches': launches, 'loop_launches': loop_launches,
        'reruns_bit_identical': same, 'mean_score': float((t[:, 0] - t[:, 1] + t[:, 2] - t[:, 3]).mean()),
        'note': 'score_ms: device events around E[log U] of the final pair + engine.zi_cell_bounds (the mask from the packed counts '
                'and the allocations of the call\'s own buffers included); zi_cell_bound in score_launches: the logit, sweep and '
                'combine launches of the entry together; zi_foldin_rate in loop_launches: the rate launch of an iteration',
    }
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


def main_score(args):
    """--score: what scoring adds to a fold-in -- one engine.cell_bounds call (two factor preparations, the row pass that leaves
    s in the row-side slots, oriana_cell_bound_nnz, oriana_gamma_kl_rows, the float64 product) beside one iteration of
    engine.fold_in on the same new cells and the same fitted gene side as the default mode.  Device events around the whole
    call / loop, `--reps` times after a warm-up of both, then one call with per-launch events.

        python tools/transform_bench.py --score --fit-rows 131072 --fit-sweeps 5 --out profiles/score_bench.json
    """
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('transform_bench needs a GPU: there is nothing to time without one')
    from oriana_amd import engine
    from oriana_amd._lib import call, ptr, stream_ptr
    from oriana_amd.models import GaP
    from oriana_amd.singlecell import SyntheticCounts
    dev = torch.device('cuda', 0)
    nq, m, K, seed = args.cells, args.genes, args.k, 1234 + 1000 * 4
    gen = SyntheticCounts(args.fit_rows, m, K, seed=seed, device=dev, zero_inflation_level=args.zeros)
    counts = engine.CountTiles.from_chunks(args.fit_rows, m, gen.chunk, args.chunk_rows, dev,
                                           dense_density=engine.auto_dense_density(args.fit_rows, m, K))
    a1, b1 = gen.initial_shapes()
    model = GaP(counts, k=K, use_factors=False, init=(a1, b1), device=dev)
    del a1, b1
    model.fit(args.fit_sweeps)
    torch.cuda.synchronize()
    genq = SyntheticCounts(nq, m, K, seed=seed, device=dev, zero_inflation_level=args.zeros)
    ct = engine.CountTiles.from_chunks(nq, m, genq.chunk, args.chunk_rows, dev, dense_density=None)
    alpha1, alpha2, lv = model.alpha1.tensor, model.alpha2.tensor, model._log_V_hat
    sum_v = (model._accV[0] if model._v_sums_in_acc else model._sumV[0]).clone()
    a2_row = torch.clamp(alpha2 + sum_v, min=1e-15)
    ws = engine.ZWorkspace(ct, K)
    start = (alpha1[None, :] + engine.row_sums_over_k(ws, K).to(torch.float64)).contiguous()
    a1q = start.clone()

    def loop():
        a1q.copy_(start)
        engine.fold_in(ct, K, lv, alpha1, a2_row, a1q, args.iters, 0.0, ws=ws)

    lu = torch.empty(nq, K, dtype=torch.float32, device=dev)
    a2 = a2_row.expand(nq, K).contiguous()

    def score(timer=None):
        ws.timer = timer
        call('oriana_gamma_update', ptr(a1q), ptr(a2), ptr(torch.empty_like(a2)), ptr(lu), None, None, None, None, None, None, None,
             None, None, nq, K, stream_ptr())
        t = engine.cell_bounds(ct, K, a1q, a2_row, lu, lv, sum_v, alpha1, alpha2, ws=ws)
        ws.timer = None
        return t

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    loop()
    t0 = score()                                                     # warm-up of both
    t_l, t_s = [], []
    for _ in range(args.reps):
        t_l.append(timed(loop))
        t_s.append(timed(score))
    same = bool(torch.equal(score(), t0))                            # (the loop ends at the same a1 every time)
    timer = engine.KernelTimer(prealloc=16)
    t = score(timer)
    torch.cuda.synchronize()
    launches = {k: {'count': c, 'mean_ms': round(ms, 4)} for k, (c, ms) in timer.summary().items()}
    per_iter, sc = float(np.median(t_l)) / args.iters, float(np.median(t_s))
    out = {
        'device': torch.cuda.get_device_name(0), 'cells': nq, 'genes': m, 'k': K, 'nnz': int(ct.nnz), 'iters': args.iters,
        'fit_rows': args.fit_rows, 'fit_sweeps': args.fit_sweeps, 'reps': args.reps,
        'fold_in_ms_per_iter': round(per_iter, 4), 'fold_in_loop_ms': [round(x, 3) for x in t_l],
        'score_ms': round(sc, 4), 'score_all_ms': [round(x, 3) for x in t_s],
        'score_over_one_iteration': round(sc / per_iter, 3), 'score_launches': launches,
        'reruns_bit_identical': same, 'mean_score': float((t[:, 0] - t[:, 1] - t[:, 2] - t[:, 3]).mean()),
        'note': 'score_ms: device events around E[log U] of the final shapes + engine.cell_bounds (allocations of the call\'s '
                'own buffers included); score_launches: per-launch events of one further call (the factor preparations, the '
                'E[log U] launch and the float64 product are not among them)',
    }
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--zi', action='store_true', help='time ZIGaP.fold_in\'s iteration and its rate launch (see main_zi)')
    ap.add_argument('--score', action='store_true', help='time one engine.cell_bounds call beside a fold-in iteration (see main_score)')
    ap.add_argument('--cells', type=int, default=65536)
    ap.add_argument('--genes', type=int, default=30000)
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--zeros', type=float, default=0.10, help='zero_inflation_level of the generator (0.10: ~90 %% zeros)')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--fit-rows', type=int, default=1000000)
    ap.add_argument('--fit-sweeps', type=int, default=10)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--chunk-rows', type=int, default=8192)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.zi and args.score:
        return main_zi_score(args)
    if args.zi:
        return main_zi(args)
    if args.score:
        return main_score(args)

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('transform_bench needs a GPU: there is nothing to time without one')
    from oriana_amd import engine
    from oriana_amd._lib import call, ptr, stream_ptr
    from oriana_amd.models import GaP
    from oriana_amd.singlecell import SyntheticCounts
    dev = torch.device('cuda', 0)
    nq, m, K, seed = args.cells, args.genes, args.k, 1234 + 1000 * 4

    # ---- the fitted gene side -------------------------------------------------------------------------------------------------
    gen = SyntheticCounts(args.fit_rows, m, K, seed=seed, device=dev, zero_inflation_level=args.zeros)
    counts = engine.CountTiles.from_chunks(args.fit_rows, m, gen.chunk, args.chunk_rows, dev,
                                           dense_density=engine.auto_dense_density(args.fit_rows, m, K))
    a1, b1 = gen.initial_shapes()
    model = GaP(counts, k=K, use_factors=False, init=(a1, b1), device=dev)
    del a1, b1
    model.fit(args.fit_sweeps)
    torch.cuda.synchronize()

    # ---- the new cells (same seed: the same V; their own loadings) ------------------------------------------------------------
    genq = SyntheticCounts(nq, m, K, seed=seed, device=dev, zero_inflation_level=args.zeros)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ct = engine.CountTiles.from_chunks(nq, m, genq.chunk, args.chunk_rows, dev, dense_density=None)
    torch.cuda.synchronize()
    pack_ms = (time.perf_counter() - t0) * 1e3

    alpha1, alpha2, lv = model.alpha1.tensor, model.alpha2.tensor, model._log_V_hat
    sum_v = (model._accV[0] if model._v_sums_in_acc else model._sumV[0]).clone()
    a2_row = torch.clamp(alpha2 + sum_v, min=1e-15)
    ws_f = engine.ZWorkspace(ct, K)
    start = (alpha1[None, :] + engine.row_sums_over_k(ws_f, K).to(torch.float64)).contiguous()

    def fused(timer=None):
        ws_f.timer = timer
        a1q = start.clone()
        engine.fold_in(ct, K, lv, alpha1, a2_row, a1q, args.iters, 0.0, ws=ws_f)
        ws_f.timer = None
        return a1q

    # the composed loop: what a caller could assemble before -- the sweep's cell side on buffers of its own
    ws_c = engine.ZWorkspace(ct, K)
    f64 = dict(dtype=torch.float64, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    c_a2, c_E = torch.ones(nq, K, **f64), torch.empty(nq, K, **f64)
    c_lu, c_Zi, c_Zj = torch.empty(nq, K, **f32), torch.empty(nq, K, **f32), torch.empty(m, K, **f32)
    c_sums = torch.zeros(2, K, **f64)

    def composed(timer=None):
        ws_c.timer = timer
        a1q = start.clone()
        st = stream_ptr()
        ws_c.fu_pending = False
        c_sums.zero_()
        call('oriana_gamma_update_prep', ptr(a1q), ptr(c_a2), ptr(c_E), ptr(c_lu), ptr(c_sums[0]), ptr(c_sums[1]), None, None, None,
             None, None, None, None, nq, K, None, None, None, st)              # E[log U] of the start (a2 = 1, as a new model)
        for _ in range(args.iters):
            engine.zq_gap(ws_c, c_Zi, c_Zj, c_lu, lv, phase='rows', finalize_rows=False, clear=(c_sums,))
            prep = ws_c.prep_outputs(True) or (None, None, None)
            with engine._span(ws_c, 'composed_update'):
                call('oriana_gamma_update_finalize_prep', ptr(a1q), ptr(c_a2), ptr(c_E), ptr(c_lu), ptr(c_sums[0]), ptr(c_sums[1]),
                     ptr(alpha1), ptr(alpha2), ptr(c_Zi), ptr(ws_c.FU), ptr(ws_c.R), ws_c.row_gene_splits, ws_c.row_slab_row0,
                     ptr(ct.row_perm), ptr(sum_v), nq, K, ptr(prep[0]), ptr(prep[1]), ptr(prep[2]), st)
            if prep[0] is not None:
                ws_c.fu_pending, ws_c.fu_source = True, c_lu.data_ptr()
        ws_c.timer = None
        return a1q

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    ra, rb = fused(), composed()                                     # warm-up of every shape the timed loops use
    torch.cuda.synchronize()
    # (from the second iteration on the two loops evaluate the same map: the composed one starts from a2 = 1)
    rel = float(((ra - rb).abs() / (rb.abs() + rb.abs().max(0, keepdim=True).values)).max())
    t_f, t_c = [], []
    for _ in range(args.reps):
        t_f.append(timed(fused))
        t_c.append(timed(composed))

    def breakdown(fn):
        timer = engine.KernelTimer(prealloc=8 * args.iters)
        fn(timer)
        torch.cuda.synchronize()
        return {k: {'count': c, 'mean_ms': round(ms, 4)} for k, (c, ms) in timer.summary().items()}
    bf, bc = breakdown(fused), breakdown(composed)

    def per_iter(ts):
        return float(np.median(ts)) / args.iters

    def outside(total_ms, bd):
        rp = bd.get('row_pass', {'count': 0, 'mean_ms': 0.0})
        return total_ms - rp['mean_ms'] * rp['count'] / args.iters

    pf, pc = per_iter(t_f), per_iter(t_c)
    of, oc = outside(pf, bf), outside(pc, bc)
    out = {
        'device': torch.cuda.get_device_name(0), 'cells': nq, 'genes': m, 'k': K, 'nnz': int(ct.nnz), 'iters': args.iters,
        'fit_rows': args.fit_rows, 'fit_sweeps': args.fit_sweeps, 'reps': args.reps,
        'pack_ms': round(pack_ms, 2),
        'fused_ms_per_iter': round(pf, 4), 'composed_ms_per_iter': round(pc, 4),
        'fused_loop_ms': [round(t, 3) for t in t_f], 'composed_loop_ms': [round(t, 3) for t in t_c],
        'fused_outside_row_pass_ms': round(of, 4), 'composed_outside_row_pass_ms': round(oc, 4),
        'fused_outside_share': round(of / pf, 4), 'composed_outside_share': round(oc / pc, 4),
        'outside_fused_over_composed': round(of / oc, 4),
        'fused_launches': bf, 'composed_launches': bc,
        'a1_fused_vs_composed_colrel': rel,
        'note': 'loop times: device events around the whole loop (start launch, host reads of the active counter every 5 '
                'iterations and the clone of the start included); launches: per-launch events of one further loop',
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
