# -*- coding: utf-8 -*-
"""Times one GaP.partial_fit() call and sets it beside a CAVI sweep over the same batch held resident.

Default: a batch of 8,192 x 30,000 cells, K = 100, 90 % zeros (the benchmark's generator); the gene side is that of
GaP(batch) after `--fit-sweeps` sweeps.  Device events around whole partial_fit() calls with `--iters` forced fold-in
iterations (tol = 0) after a warm-up call, `--reps` times, then one call composed from the same pieces (GaP._fold_in_start,
heldout.fold_in, heldout.gene_statistics, heldout.svi_gene_update) on a workspace with a KernelTimer: one span around each
piece and the per-launch spans of the passes inside.  The sweep: `--reps` step() calls of the resident model between two
events.  Prints one JSON line; `--out` also writes it to a file.

    python tools/partial_fit_bench.py --out profiles/partial_fit_bench.json
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
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('partial_fit_bench needs a GPU: there is nothing to time without one')
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
