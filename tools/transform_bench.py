# -*- coding: utf-8 -*-
"""Times a fold-in (GaP.transform's loop, heldout.fold_in) against the same loop composed from the entries that existed before
oriana_foldin_update: row phase + oriana_gamma_update_finalize_prep on throw-away (n', K) buffers.

Default: 65,536 x 30,000 new cells, K = 100, 90 % zeros (the benchmark's generator), 20 forced iterations (tol = 0) against
the gene side of a model fitted on `--fit-rows` cells of the same generator for `--fit-sweeps` sweeps.  Device events
around whole loops (after a warm-up loop of each form, the two forms alternating, `--reps` times), then one loop of each
form with per-launch events for the share spent outside the row pass.  Prints one JSON line; `--out` also writes it to a file.
`--zi`: the zero-inflated fold-in instead (main_zi below).  `--score`: one heldout.cell_bounds call beside one fold-in iteration
(main_score below).  `--zi --score`: one heldout.zi_cell_bounds call beside one ZI fold-in iteration (main_score too).
`--sparse [--zi]`: one iteration of SparseGaP / SparseZIGaP.project()'s loop per K of `--sparse-ks`, and the second row product
with and without the active bytes (main_sparse below).

    python tools/transform_bench.py --out profiles/transform_bench.json
"""
import argparse
import json
import os
import sys
import time

from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def setup(args, zi, sparse=False):
    """What every mode times against: a model (ZIGaP if `zi`, else GaP; `sparse`: SparseZIGaP / SparseGaP) fitted on `--fit-rows`
    cells for `--fit-sweeps` sweeps, the new cells packed on the sliced layout (same seed: the same V; their own loadings), a
    workspace over them and the default start of a fold-in.  Returns a namespace of them and of the model's gene side as the
    fold-in reads it."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('transform_bench needs a GPU: there is nothing to time without one')
    from oriana_amd import engine, heldout
    from oriana_amd.models import GaP, SparseGaP, SparseZIGaP, ZIGaP
    from oriana_amd.singlecell import SyntheticCounts
    dev = torch.device('cuda', 0)
    nq, m, K, seed = args.cells, args.genes, args.k, 1234 + 1000 * 4
    gen = SyntheticCounts(args.fit_rows, m, K, seed=seed, device=dev, zero_inflation_level=args.zeros)
    counts = engine.CountTiles.from_chunks(args.fit_rows, m, gen.chunk, args.chunk_rows, dev,
                                           dense_density=None if zi or sparse else engine.auto_dense_density(args.fit_rows, m, K))
    a1, b1 = gen.initial_shapes()
    cls = (SparseZIGaP if zi else SparseGaP) if sparse else (ZIGaP if zi else GaP)
    model = cls(counts, k=K, use_factors=False, init=(a1, b1), device=dev)
    del a1, b1
    model.fit(args.fit_sweeps)
    genq = SyntheticCounts(nq, m, K, seed=seed, device=dev, zero_inflation_level=args.zeros)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ct = engine.CountTiles.from_chunks(nq, m, genq.chunk, args.chunk_rows, dev, dense_density=None)
    torch.cuda.synchronize()
    b = SimpleNamespace(dev=dev, nq=nq, m=m, K=K, model=model, ct=ct, pack_ms=(time.perf_counter() - t0) * 1e3,
                        alpha1=model.alpha1.tensor, alpha2=model.alpha2.tensor, lv=model._log_V_hat, ws=engine.ZWorkspace(ct, K))
    if sparse:
        return b
    b.start = (b.alpha1[None, :] + heldout.row_sums_over_k(b.ws, K).to(torch.float64)).contiguous()
    if zi:
        b.V, b.pi_d, b.arith = model._V_hat.contiguous(), model.pi_d.tensor.contiguous(), model._matrix_arith
        b.start2 = torch.clamp(b.alpha2 + b.V.sum(0), min=1e-15)[None, :].expand(nq, K).contiguous()
    else:
        b.sum_v = (model._accV[0] if model._v_sums_in_acc else model._sumV[0]).clone()
        b.a2_row = torch.clamp(b.alpha2 + b.sum_v, min=1e-15)
    return b


def timed(fn):
    """Milliseconds between two device events around fn()."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def launches(fn, prealloc):
    """Per-launch events of one further fn(timer): {name: {count, mean_ms}}."""
    import torch
    from oriana_amd import engine
    timer = engine.KernelTimer(prealloc=prealloc)
    fn(timer)
    torch.cuda.synchronize()
    return {k: {'count': c, 'mean_ms': round(ms, 4)} for k, (c, ms) in timer.summary().items()}


def emit(out, args):
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


def main_zi(args):
    """--zi: one iteration of ZIGaP.fold_in's loop (heldout.fold_in_zi), and its rate launch -- oriana_zi_foldin_rate, which never
    stores the dropout posterior -- against the storing entry (oriana_dropout_sweep_fused_tiles on a scratch D_hat of the query, whose
    kernels this build compiles instruction for instruction as before the rate entry existed) on the same operands: the two
    launches alternate, device events around runs of `--iters` launches, `--reps` times, after a warm-up of both.

        python tools/transform_bench.py --zi --cells 16384 --genes 20000 --k 50 --out profiles/zi_foldin_bench_k50.json
    """
    import numpy as np
    import torch
    from oriana_amd import _lib, heldout
    from oriana_amd._lib import call, ptr, stream_ptr
    b = setup(args, zi=True)
    nq, m, K, ct, ws, dev, arith = b.nq, b.m, b.K, b.ct, b.ws, b.dev, b.arith

    def loop(timer=None):
        ws.timer = timer
        p1, p2 = b.start.clone(), b.start2.clone()
        heldout.fold_in_zi(ct, K, b.lv, b.V, b.pi_d, b.alpha1, b.alpha2, p1, p2, args.iters, 0.0, ws=ws, arithmetic=arith)
        ws.timer = None
        return p1, p2

    p1, p2 = loop()                                                  # warm-up
    t_loop = [timed(loop) for _ in range(args.reps)]
    loop_launches = launches(loop, 8 * args.iters)

    # ---- the rate launch alone, both forms on the operands of the loop's last iteration ---------------------------------------
    f64 = dict(dtype=torch.float64, device=dev)
    mp, Vp, pip, mask = heldout._padded_genes(ct, K, b.V, b.pi_d)
    U = (p1 / p2).contiguous()
    st = stream_ptr()
    lib = _lib.load()
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
    emit({
        'device': torch.cuda.get_device_name(0), 'cells': nq, 'genes': m, 'k': K, 'nnz': int(ct.nnz), 'iters': args.iters,
        'fit_rows': args.fit_rows, 'fit_sweeps': args.fit_sweeps, 'reps': args.reps, 'arithmetic': arith,
        'loop_ms_per_iter': round(float(np.median(t_loop)) / args.iters, 4), 'loop_ms': [round(t, 3) for t in t_loop],
        'loop_launches': loop_launches,
        'rate_no_store_ms': round(float(np.median(t_a)), 4), 'rate_storing_ms': round(float(np.median(t_b)), 4),
        'rate_no_store_all_ms': [round(t, 4) for t in t_a], 'rate_storing_all_ms': [round(t, 4) for t in t_b],
        'D_hat_bytes_not_allocated_by_fold_in': nq * mp * 4,
        'rate_no_store_vs_storing_colrel': rel,
        'note': 'rate_*: `iters` back-to-back launches between two device events, the two forms alternating; the storing form '
                'writes a scratch D_hat of the query and its column sums besides the same DV',
    }, args)


def main_score(args, zi):
    """--score: what scoring adds to a fold-in -- E[log U] of the final shapes + one heldout.cell_bounds call (two factor
    preparations, the row pass that leaves s in the row-side slots, oriana_cell_bound_nnz, oriana_gamma_kl_rows, the float64
    product) beside one iteration of heldout.fold_in on the same new cells and the same fitted gene side as the default mode.
    --zi --score: the same for ZI-pCMF -- heldout.zi_cell_bounds (the data path, the query's non-zero mask, oriana_zi_cell_bound,
    oriana_gamma_kl_rows) beside one iteration of heldout.fold_in_zi and its rate launch, on the operands of --zi.  Device events
    around the whole call / loop, `--reps` times after a warm-up of both, then one call (--zi: and one loop) with per-launch events.

        python tools/transform_bench.py --score --fit-rows 131072 --fit-sweeps 5 --out profiles/score_bench.json
        python tools/transform_bench.py --zi --score --cells 16384 --genes 20000 --k 50 --fit-rows 16384 --fit-sweeps 3 --iters 10
    """
    import numpy as np
    import torch
    from oriana_amd import heldout
    from oriana_amd.nodes import gamma_expectations
    b = setup(args, zi)
    nq, m, K, ct, ws = b.nq, b.m, b.K, b.ct, b.ws
    p1 = b.start.clone()
    p2 = b.start2.clone() if zi else b.a2_row.expand(nq, K).contiguous()

    def loop(timer=None):
        ws.timer = timer
        p1.copy_(b.start)
        if zi:
            p2.copy_(b.start2)
            heldout.fold_in_zi(ct, K, b.lv, b.V, b.pi_d, b.alpha1, b.alpha2, p1, p2, args.iters, 0.0, ws=ws, arithmetic=b.arith)
        else:
            heldout.fold_in(ct, K, b.lv, b.alpha1, b.a2_row, p1, args.iters, 0.0, ws=ws)
        ws.timer = None

    def score(timer=None):
        ws.timer = timer
        lu = gamma_expectations(p1, p2)[1]
        if zi:
            t = heldout.zi_cell_bounds(ct, K, p1, p2, lu, b.lv, b.V, b.pi_d, b.alpha1, b.alpha2, ws=ws)
        else:
            t = heldout.cell_bounds(ct, K, p1, b.a2_row, lu, b.lv, b.sum_v, b.alpha1, b.alpha2, ws=ws)
        ws.timer = None
        return t

    loop()
    t0 = score()                                                     # warm-up of both
    t_l, t_s = [], []
    for _ in range(args.reps):
        t_l.append(timed(loop))
        t_s.append(timed(score))
    same = bool(torch.equal(score(), t0))                            # (the loop ends at the same shapes every time)
    t = score()
    per_iter, sc = float(np.median(t_l)) / args.iters, float(np.median(t_s))
    out = {
        'device': torch.cuda.get_device_name(0), 'cells': nq, 'genes': m, 'k': K, 'nnz': int(ct.nnz), 'iters': args.iters,
        'fit_rows': args.fit_rows, 'fit_sweeps': args.fit_sweeps, 'reps': args.reps}
    if zi:
        out['arithmetic'] = b.arith
    out.update({
        'fold_in_ms_per_iter': round(per_iter, 4), 'fold_in_loop_ms': [round(x, 3) for x in t_l],
        'score_ms': round(sc, 4), 'score_all_ms': [round(x, 3) for x in t_s],
        'score_over_one_iteration': round(sc / per_iter, 3), 'score_launches': launches(score, 16)})
    if zi:
        out['loop_launches'] = launches(loop, 8 * args.iters)
    out['reruns_bit_identical'] = same
    if zi:
        out['mean_score'] = float((t[:, 0] - t[:, 1] + t[:, 2] - t[:, 3]).mean())
        out['note'] = ('score_ms: device events around E[log U] of the final pair + heldout.zi_cell_bounds (the mask from the packed '
                       'counts and the allocations of the call\'s own buffers included); zi_cell_bound in score_launches: the logit, '
                       'sweep and combine launches of the entry together; zi_foldin_rate in loop_launches: the rate launch of an '
                       'iteration')
    else:
        out['mean_score'] = float((t[:, 0] - t[:, 1] - t[:, 2] - t[:, 3]).mean())
        out['note'] = ('score_ms: device events around E[log U] of the final shapes + heldout.cell_bounds (allocations of the '
                       'call\'s own buffers included); score_launches: per-launch events of one further call (the factor '
                       'preparations, the E[log U] launch and the float64 product are not among them)')
    emit(out, args)


def main_sparse(args, zi):
    """--sparse [--zi]: a REPORT, no threshold.  Per K of `--sparse-ks` (50: the two-image row pass; 100: the s_rs pass and the
    second row product): a sparse model fitted as `setup` fits it, then -- a few sweeps from the generator's start leave p_s ~ 1 --
    a p_s of this tool's own loaded over it (U(0, 1) entries, every third gene at 0.1 in every factor: fully masked); one
    iteration of project()'s loop (heldout.fold_in / fold_in_zi with the masks, tol = 0, `--iters` iterations, device events
    around the loop, `--reps` times after a warm-up) and its per-launch events; where the row phase has a second row product,
    its share of the iteration and the launch alone in three forms on the loop's own operands -- oriana_row_spmm,
    oriana_row_spmm_active with every cell active, and with every other 256-row block frozen -- alternating, 10 back-to-back
    launches between two device events, 5 repetitions.  `active_all_not_slower`: the all-active form's median is not above
    oriana_row_spmm's by more than the spread (max - min) of the repetitions.

        python tools/transform_bench.py --sparse --cells 16384 --genes 20000 --fit-rows 16384 --fit-sweeps 3 \
            --out profiles/sparse_project_bench.json
    """
    import numpy as np
    import torch
    from oriana_amd import heldout
    from oriana_amd._lib import call, ptr, stream_ptr
    runs = []
    for K in [int(k) for k in args.sparse_ks.split(',')]:
        args.k = K
        b = setup(args, zi, sparse=True)
        nq, m, ct, ws, dev, model = b.nq, b.m, b.ct, b.ws, b.dev, b.model
        P = torch.rand(m, K, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(K))
        P[::3] = 0.1
        model.load_state({'p_s': P.cpu().numpy()})
        model.update_expectations()
        S_tilde = (P > model.tau).to(torch.float32)
        S_hat = P.to(torch.float32)
        Veff = (model._V_hat * S_hat).contiguous()
        a2_row = torch.clamp(b.alpha2 + Veff.sum(0), min=1e-15)
        start = (b.alpha1[None, :] + heldout.masked_row_sums(ws, K, S_tilde, S_hat).to(torch.float64)).contiguous()
        start2 = a2_row[None, :].expand(nq, K).contiguous()

        def loop(timer=None):
            ws.timer = timer
            p1 = start.clone()
            if zi:
                heldout.fold_in_zi(ct, K, b.lv, Veff, model.pi_d.tensor.contiguous(), b.alpha1, b.alpha2, p1, start2.clone(),
                                   args.iters, 0.0, ws=ws, arithmetic=model._matrix_arith, S_tilde=S_tilde, S_hat=S_hat)
            else:
                heldout.fold_in(ct, K, b.lv, b.alpha1, a2_row, p1, args.iters, 0.0, ws=ws, S_tilde=S_tilde, S_hat=S_hat)
            ws.timer = None

        loop()                                                           # warm-up
        t_loop = [timed(loop) for _ in range(args.reps)]
        ll = launches(loop, 8 * args.iters)
        per_iter = float(np.median(t_loop)) / args.iters
        run = {'k': K, 'cells': nq, 'genes': m, 'nnz': int(ct.nnz), 'fully_masked_genes': float((S_tilde.sum(1) == 0).double().mean()),
               'row_phase': 'two-launch' if 'row_spmm' in ll else 'two-image', 'rows_nslab': ws.rows_nslab,
               'loop_ms_per_iter': round(per_iter, 4), 'loop_ms': [round(t, 3) for t in t_loop], 'loop_launches': ll}
        if 'row_spmm' in ll:
            sp = ll['row_spmm']
            run['second_product_share'] = round(sp['mean_ms'] * sp['count'] / args.iters / per_iter, 4)
            st, cs = stream_ptr(), ct.sparse_struct
            F2 = ws.extra('FVS', m)
            all_on = torch.ones(nq, dtype=torch.uint8, device=dev)
            half = torch.ones(nq, dtype=torch.uint8, device=dev)
            blocks = torch.arange(nq, device=dev) // 256
            packed_off = (blocks % 2 == 1)
            # (the bytes are in the caller's row order: the packed rows of every other block, through the row permutation)
            half[(ct.row_perm.long() if ct.row_perm is not None else torch.arange(nq, device=dev))[packed_off]] = 0

            def plain():
                for _ in range(10):
                    call('oriana_row_spmm', cs, ptr(ws.s_rs), None, ptr(F2), ptr(ws.R), K, st)

            def active(a):
                def run_():
                    for _ in range(10):
                        call('oriana_row_spmm_active', cs, ptr(ws.s_rs), None, ptr(F2), ptr(ws.R), ptr(a), K, st)
                return run_
            forms = {'row_spmm': plain, 'active_all': active(all_on), 'active_half_blocks_frozen': active(half)}
            for f in forms.values():
                f()                                                      # warm-up
            ts = {name: [] for name in forms}
            for _ in range(5):
                for name, f in forms.items():
                    ts[name].append(timed(f) / 10)
            med = {name: float(np.median(v)) for name, v in ts.items()}
            spread = max(max(ts[n]) - min(ts[n]) for n in ('row_spmm', 'active_all'))
            run['second_product'] = {
                'ms': {n: round(v, 4) for n, v in med.items()}, 'all_ms': {n: [round(t, 4) for t in v] for n, v in ts.items()},
                'spread_ms': round(spread, 4), 'active_all_not_slower': bool(med['active_all'] - med['row_spmm'] <= spread),
                'frozen_share_of_cells': float((half == 0).double().mean())}
        runs.append(run)
    emit({'device': torch.cuda.get_device_name(0), 'model': 'SparseZIGaP' if zi else 'SparseGaP', 'iters': args.iters,
          'fit_rows': args.fit_rows, 'fit_sweeps': args.fit_sweeps, 'reps': args.reps, 'runs': runs,
          'note': 'loop times: device events around the whole loop (start launch, host reads of the active counter every 5 iterations '
                  'and the clone of the start included), tol = 0: no cell freezes inside the loop; second_product: 10 back-to-back '
                  'launches between two device events per figure, the three forms alternating, 5 repetitions; p_s is the tool\'s '
                  'own (every third gene fully masked), loaded over the fitted model'}, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sparse', action='store_true', help='time project()\'s iteration and the second row product (see main_sparse)')
    ap.add_argument('--sparse-ks', default='50,100', help='the K of --sparse, comma-separated')
    ap.add_argument('--zi', action='store_true', help='time ZIGaP.fold_in\'s iteration and its rate launch (see main_zi)')
    ap.add_argument('--score', action='store_true', help='time one heldout.cell_bounds call beside a fold-in iteration (see main_score)')
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
    if args.sparse:
        return main_sparse(args, args.zi)
    if args.score:
        return main_score(args, args.zi)
    if args.zi:
        return main_zi(args)

    import numpy as np
    import torch
    from oriana_amd import engine, heldout
    from oriana_amd._lib import call, ptr, stream_ptr
    b = setup(args, zi=False)
    nq, m, K, ct, dev, ws_f = b.nq, b.m, b.K, b.ct, b.dev, b.ws
    alpha1, alpha2, lv, sum_v, a2_row, start = b.alpha1, b.alpha2, b.lv, b.sum_v, b.a2_row, b.start

    def fused(timer=None):
        ws_f.timer = timer
        a1q = start.clone()
        heldout.fold_in(ct, K, lv, alpha1, a2_row, a1q, args.iters, 0.0, ws=ws_f)
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

    ra, rb = fused(), composed()                                     # warm-up of every shape the timed loops use
    torch.cuda.synchronize()
    # (from the second iteration on the two loops evaluate the same map: the composed one starts from a2 = 1)
    rel = float(((ra - rb).abs() / (rb.abs() + rb.abs().max(0, keepdim=True).values)).max())
    t_f, t_c = [], []
    for _ in range(args.reps):
        t_f.append(timed(fused))
        t_c.append(timed(composed))

    bf, bc = launches(fused, 8 * args.iters), launches(composed, 8 * args.iters)

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
        'pack_ms': round(b.pack_ms, 2),
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
    emit(out, args)


if __name__ == '__main__':
    main()
