# -*- coding: utf-8 -*-
"""Times one GaP.partial_fit() call and sets it beside a CAVI sweep over the same batch held resident.

Default: a batch of 8,192 x 30,000 cells, K = 100, 90 % zeros (the benchmark's generator); the gene side is that of
GaP(batch) after `--fit-sweeps` sweeps.  Device events around whole partial_fit() calls with `--iters` forced fold-in
iterations (tol = 0) after a warm-up call, `--reps` times, then one call composed from the same pieces (GaP._fold_in_start,
heldout.fold_in, heldout.gene_statistics, heldout.svi_gene_update) on a workspace with a KernelTimer: one span around each
piece and the per-launch spans of the passes inside.  The sweep: `--reps` step() calls of the resident model between two
events.  Prints one JSON line; `--out` also writes it to a file.

    python tools/partial_fit_bench.py --out profiles/partial_fit_bench.json

`--zi`: the same for ZIGaP.fold_in_fit() -- whole calls, then one call composed from its pieces (ZIGaP._fold_in_start,
heldout.fold_in_zi, heldout.gene_statistics, heldout.zi_gene_rate, heldout.svi_gene_update) under a KernelTimer, and
oriana_zi_gene_rate on its own beside the same statistic composed from the entries that existed before it
(oriana_dropout_sweep_fused_tiles with ORIANA_MATRIX_F32 storing a scratch D_hat, then oriana_dense_t_times_factor_f32) on the
same operands.

    python tools/partial_fit_bench.py --zi --out profiles/zi_fold_in_fit_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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


def main_zi(args):
    import numpy as np
    import torch
    from oriana_amd import _lib, engine, heldout
    from oriana_amd._lib import call, ptr, stream_ptr
    from oriana_amd.models import ZIGaP
    from oriana_amd.singlecell import SyntheticCounts
    dev = torch.device('cuda', 0)
    n, m, K = args.cells, args.genes, args.k
    gen = SyntheticCounts(n, m, K, seed=5234, device=dev, zero_inflation_level=args.zeros)
    batch = engine.CountTiles.from_chunks(n, m, gen.chunk, args.chunk_rows, dev, dense_density=None)
    a1, b1 = gen.initial_shapes()
    model = ZIGaP(batch, k=K, use_factors=False, init=(a1, b1), device=dev)
    del a1, b1
    model.fit(args.fit_sweeps)
    keep = {k: getattr(model, k).tensor.clone() for k in ('b1', 'b2', 'pi_d')}
    keep.update(V=model._V_hat.clone(), lv=model._log_V_hat.clone(), sums=model._sumV.clone())

    def rewind():
        for k in ('b1', 'b2', 'pi_d'):
            getattr(model, k).tensor.copy_(keep[k])
        model._V_hat.copy_(keep['V']); model._log_V_hat.copy_(keep['lv']); model._sumV.copy_(keep['sums'])
        model._touch()

    def whole():
        model.fold_in_fit(batch, args.n_total, rho=0.5, n_iter=args.iters, tol=0)
    whole()                                                           # warm-up
    rewind()
    t_call = []
    for _ in range(args.reps):
        t_call.append(timed(whole))
        rewind()

    timer = engine.KernelTimer(prealloc=24 * args.iters + 64)
    kept = {}

    def composed():
        ws = engine.ZWorkspace(batch, K)
        ws.timer = timer
        V, pi = model._V_hat.contiguous(), model.pi_d.tensor.contiguous()
        a2_row = torch.clamp(torch.nan_to_num(model.alpha2.tensor + V.sum(dim=0)), min=1e-15)
        with timer.span('piece/start'):
            a1q = model._fold_in_start(batch, ws, None)
            a2q = a2_row[None, :].expand(n, K).contiguous()
        with timer.span('piece/fold_in'):
            heldout.fold_in_zi(batch, K, model._log_V_hat, V, pi, model.alpha1.tensor, model.alpha2.tensor, a1q, a2q, args.iters, 0.0,
                               ws=ws, arithmetic=model._matrix_arith)
        with timer.span('piece/statistics'):
            stats, _ = heldout.gene_statistics(batch, K, a1q, a2q, model._log_V_hat, ws=ws, finalize=False)
            U = a1q / a2q
            G, dsum = heldout.zi_gene_rate(batch, K, U, V, pi, ws=ws)
        kept.update(U=U, V=V.clone(), pi=pi.clone())
        with timer.span('piece/gene_update'):
            heldout.svi_gene_update(model.b1.tensor, model.b2.tensor, model._V_hat, model._log_V_hat, model._sumV, model.beta1.tensor,
                                    model.beta2.tensor, stats, G, float(args.n_total) / n, 0.5, ws=ws)
            model.pi_d.tensor.mul_(0.5).add_(dsum / float(n), alpha=0.5)
    composed()
    torch.cuda.synchronize()
    spans = {k: {'count': c, 'mean_ms': round(ms, 4)} for k, (c, ms) in timer.summary().items()}
    rewind()

    # the entry on its own against the same statistic from the entries that existed before it, on the same operands
    lib = _lib.load()
    U, V, pi = kept['U'], kept['V'], kept['pi']
    mp, Vp, pip, nzmask = heldout._padded_genes(batch, K, V, pi)
    scratch = torch.empty(int(lib.oriana_zi_gene_rate_scratch_doubles(n, mp, K)), dtype=torch.float64, device=dev)
    G, dsum = torch.empty(mp, K, dtype=torch.float64, device=dev), torch.empty(mp, dtype=torch.float64, device=dev)

    def fused():
        call('oriana_zi_gene_rate', ptr(G), ptr(dsum), ptr(U), ptr(Vp), ptr(pip), ptr(nzmask), ptr(scratch), n, mp, K, stream_ptr())
    nztiles = torch.zeros(max(int(lib.oriana_nzmask_tiles_words(n, mp)), 4), dtype=torch.int32, device=dev)
    call('oriana_nzmask_tiles', ptr(nztiles), ptr(nzmask), n, mp, stream_ptr())
    lg = torch.zeros(int(lib.oriana_dropout_sweep_scratch_floats(mp, K)), dtype=torch.float32, device=dev)
    dt = torch.zeros(int(lib.oriana_dense_t_scratch_floats(n, K)), dtype=torch.float32, device=dev)
    D = torch.empty(n, mp, dtype=torch.float32, device=dev)
    cs, G2 = torch.zeros(mp, dtype=torch.float64, device=dev), torch.zeros(mp, K, dtype=torch.float64, device=dev)

    def composition():
        cs.zero_(); G2.zero_()
        call('oriana_dropout_sweep_fused_tiles', ptr(D), ptr(U), ptr(Vp), ptr(pip), ptr(nzmask), ptr(nztiles), ptr(cs), None, None,
             ptr(lg), 0, n, mp, K, stream_ptr())
        call('oriana_dense_t_times_factor_f32', ptr(G2), ptr(D), ptr(U), ptr(dt), 0, n, mp, K, stream_ptr())
    fused(); composition()                                            # warm-up
    t_fused = [timed(fused) for _ in range(args.reps)]
    t_comp = [timed(composition) for _ in range(args.reps)]
    agree = float(((G[:m] - G2[:m]).abs() / (G2[:m].abs() + G2[:m].abs().amax(dim=0, keepdim=True) + 1e-300)).max())
    med = lambda t: round(float(np.median(t)), 3)
    out = {
        'device': torch.cuda.get_device_name(0), 'model': 'ZIGaP', 'cells': n, 'genes': m, 'k': K, 'nnz': int(batch.nnz),
        'zero_inflation_level': args.zeros, 'zero_share': round(1.0 - float(batch.nnz) / (float(n) * m), 4),
        'fold_in_iters': args.iters, 'fit_sweeps': args.fit_sweeps, 'reps': args.reps, 'n_total': args.n_total,
        'fold_in_fit_ms': med(t_call), 'fold_in_fit_all_ms': [round(t, 3) for t in t_call],
        'fold_in_ms_per_iter': round(spans['piece/fold_in']['mean_ms'] / max(args.iters, 1), 4),
        'statistics_ms': spans['piece/statistics']['mean_ms'], 'gene_update_ms': spans['piece/gene_update']['mean_ms'],
        'start_ms': spans['piece/start']['mean_ms'], 'spans': spans,
        'zi_gene_rate_ms': med(t_fused), 'zi_gene_rate_all_ms': [round(t, 3) for t in t_fused],
        'composition_ms': med(t_comp), 'composition_all_ms': [round(t, 3) for t in t_comp],
        'zi_gene_rate_ranges': int(lib.oriana_zi_gene_rate_ranges(n, mp, K)),
        'zi_gene_rate_scratch_mb': round(scratch.numel() * 8 / 1e6, 2), 'composition_D_hat_mb': round(D.numel() * 4 / 1e6, 2),
        'fused_against_composition_colrel': agree,
        'note': 'fold_in_fit_ms: whole calls (packing excluded: the batch is a prebuilt CountTiles), tol = 0 so that every call runs '
                '`fold_in_iters` iterations; piece/*: one call composed from the same pieces under a KernelTimer; composition: '
                'oriana_dropout_sweep_fused_tiles (ORIANA_MATRIX_F32) storing a scratch D_hat + oriana_dense_t_times_factor_f32',
    }
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=8192)
    ap.add_argument('--genes', type=int, default=30000)
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--zeros', type=float, default=0.10, help='zero_inflation_level of the generator (0.10: ~90 %% zeros)')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--fit-sweeps', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n-total', type=int, default=1000000)
    ap.add_argument('--chunk-rows', type=int, default=8192)
    ap.add_argument('--out', default=None)
    ap.add_argument('--zi', action='store_true', help='time ZIGaP.fold_in_fit() and oriana_zi_gene_rate instead')
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('partial_fit_bench needs a GPU: there is nothing to time without one')
    if args.zi:
        return main_zi(args)
    from oriana_amd import engine, heldout
    from oriana_amd.models import GaP
    from oriana_amd.singlecell import SyntheticCounts
    dev = torch.device('cuda', 0)
    n, m, K = args.cells, args.genes, args.k
    gen = SyntheticCounts(n, m, K, seed=5234, device=dev, zero_inflation_level=args.zeros)
    resident = engine.CountTiles.from_chunks(n, m, gen.chunk, args.chunk_rows, dev, dense_density=engine.auto_dense_density(n, m, K))
    a1, b1 = gen.initial_shapes()
    model = GaP(resident, k=K, use_factors=False, init=(a1, b1), device=dev)
    del a1, b1
    model.fit(args.fit_sweeps)
    batch = engine.CountTiles.from_chunks(n, m, gen.chunk, args.chunk_rows, dev, dense_density=None)      # as a stream would pack it
    state = {k: getattr(model, k).tensor.clone() for k in ('b1', 'b2')}

    def rewind():
        model.load_state({k: v.cpu().numpy() for k, v in state.items()})
        model.update_expectations()

    def call():
        model.partial_fit(batch, args.n_total, rho=0.5, n_iter=args.iters, tol=0)
    call()                                                            # warm-up
    t_call = [timed(call) for _ in range(args.reps)]
    rewind()

    timer = engine.KernelTimer(prealloc=16 * args.iters + 64)

    def composed():
        ws = engine.ZWorkspace(batch, K)
        ws.timer = timer
        sum_v = model._accV[0] if model._v_sums_in_acc else model._sumV[0]
        a2_row = torch.clamp(torch.nan_to_num(model.alpha2.tensor + sum_v), min=1e-15)
        with timer.span('piece/start'):
            a1q = model._fold_in_start(batch, ws, None)
        with timer.span('piece/fold_in'):
            heldout.fold_in(batch, K, model._log_V_hat, model.alpha1.tensor, a2_row, a1q, args.iters, 0.0, ws=ws)
        with timer.span('piece/statistics'):
            stats, sum_u = heldout.gene_statistics(batch, K, a1q, a2_row, model._log_V_hat, ws=ws, finalize=False)
        with timer.span('piece/gene_update'):
            heldout.svi_gene_update(model.b1.tensor, model.b2.tensor, model._V_hat, model._log_V_hat, model._sumV, model.beta1.tensor,
                                    model.beta2.tensor, stats, sum_u, float(args.n_total) / n, 0.5, ws=ws)
        model._v_sums_in_acc = False
        model._touch()
    composed()
    torch.cuda.synchronize()
    spans = {k: {'count': c, 'mean_ms': round(ms, 4)} for k, (c, ms) in timer.summary().items()}
    rewind()

    model.step()                                                      # warm-up
    t_sweep = [timed(model.step) for _ in range(args.reps)]
    out = {
        'device': torch.cuda.get_device_name(0), 'cells': n, 'genes': m, 'k': K, 'nnz': int(batch.nnz), 'zero_inflation_level': args.zeros,
        'zero_share': round(1.0 - float(batch.nnz) / (float(n) * m), 4),
        'fold_in_iters': args.iters, 'fit_sweeps': args.fit_sweeps, 'reps': args.reps, 'n_total': args.n_total,
        'partial_fit_ms': round(float(np.median(t_call)), 3), 'partial_fit_all_ms': [round(t, 3) for t in t_call],
        'fold_in_ms_per_iter': round(spans['piece/fold_in']['mean_ms'] / max(args.iters, 1), 4),
        'statistics_ms': spans['piece/statistics']['mean_ms'], 'gene_update_ms': spans['piece/gene_update']['mean_ms'],
        'start_ms': spans['piece/start']['mean_ms'], 'spans': spans,
        'resident_sweep_ms': round(float(np.median(t_sweep)), 3), 'resident_sweep_all_ms': [round(t, 3) for t in t_sweep],
        'resident_dense_genes': int(resident.gd),
        'note': 'partial_fit_ms: whole calls (packing excluded: the batch is a prebuilt CountTiles), tol = 0 so that every call '
                'runs `fold_in_iters` iterations; piece/*: one call composed from the same pieces under a KernelTimer',
    }
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
