# -*- coding: utf-8 -*-
"""Cost report of FactorModel.gene_deviance() / cell_deviance(): a REPORT, no threshold.

Per layout (sliced; hybrid: the dense genes on the matrix cores, engine.auto_dense_density) one model of `--model` on the
benchmark generator's counts (`--cells` x `--genes`, K = `--k`, ~90 % zeros), fitted for `--fit-sweeps` sweeps; then, in the same
run and on the same state, explained_deviance() (the full metric: row pass + oriana_metric_nnz, with a dropout node
oriana_dropout_metric), gene_deviance() and cell_deviance().  Wall-clock time around each call between two device
synchronisations (the calls end in a host read), medians of `--reps` (default 5) after one warm-up call of each, the three forms
alternating.  `--yardstick` times explained_deviance() alone: the form to run on a checkout of an earlier commit, whose figure
the report is read against.  Prints one JSON line; `--out` also writes it to a file.

    python tools/axis_deviance_bench.py --cells 262144 --out profiles/axis_deviance_bench.json
    python tools/axis_deviance_bench.py --model ZIGaP --cells 16384 --genes 20000 --k 50 --out profiles/axis_deviance_bench_zigap.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='GaP', choices=['GaP', 'ZIGaP', 'SparseGaP', 'SparseZIGaP'])
    ap.add_argument('--cells', type=int, default=262144)
    ap.add_argument('--genes', type=int, default=30000)
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--zeros', type=float, default=0.10, help='zero_inflation_level of the generator (0.10: ~90 %% zeros)')
    ap.add_argument('--fit-sweeps', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--chunk-rows', type=int, default=8192)
    ap.add_argument('--layouts', default='sliced,hybrid')
    ap.add_argument('--yardstick', action='store_true', help='time explained_deviance() alone')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('axis_deviance_bench needs a GPU: there is nothing to time without one')
    from oriana_amd import engine, models
    from oriana_amd.singlecell import SyntheticCounts
    dev = torch.device('cuda', 0)
    n, m, K, seed = args.cells, args.genes, args.k, 1234 + 1000 * 4

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    runs = []
    for layout in args.layouts.split(','):
        dd = engine.auto_dense_density(n, m, K) if layout == 'hybrid' and engine.dense_supported(K) else None
        if layout == 'hybrid' and not dd:
            runs.append({'layout': layout, 'skipped': 'no dense block at this shape / K'})
            continue
        gen = SyntheticCounts(n, m, K, seed=seed, device=dev, zero_inflation_level=args.zeros)
        counts = engine.CountTiles.from_chunks(n, m, gen.chunk, args.chunk_rows, dev, dense_density=dd)
        a1, b1 = gen.initial_shapes()
        G = getattr(models, args.model)(counts, k=K, use_factors=False, init=(a1, b1), device=dev)
        del a1, b1, gen
        G.fit(args.fit_sweeps)
        print('%s: fitted, nnz %d, %d dense genes' % (layout, counts.nnz, counts.gd), file=sys.stderr, flush=True)
        forms = {'explained_deviance': G.explained_deviance}
        if not args.yardstick:
            forms.update(gene_deviance=G.gene_deviance, cell_deviance=G.cell_deviance)
        last = {name: f() for name, f in forms.items()}                          # warm-up (scratch, count constants)
        ts = {name: [] for name in forms}
        for _ in range(args.reps):
            for name, f in forms.items():
                t, last[name] = timed(f)
                ts[name].append(t)
        med = {name: float(np.median(v)) for name, v in ts.items()}
        run = {'layout': layout, 'dense_genes': int(counts.gd), 'nnz': int(counts.nnz),
               'ms': {name: round(v, 3) for name, v in med.items()},
               'all_ms': {name: [round(t, 3) for t in v] for name, v in ts.items()},
               'explained_deviance': float(last['explained_deviance'])}
        if not args.yardstick:
            g, c = last['gene_deviance'], last['cell_deviance']
            run.update(gene_over_explained_deviance=round(med['gene_deviance'] / med['explained_deviance'], 3),
                       cell_over_explained_deviance=round(med['cell_deviance'] / med['explained_deviance'], 3),
                       # the axes against the scalar metric: (sum factors - sum mean) / (sum counts - sum mean)
                       explained_deviance_from_genes=float((g['factors'].sum() - g['mean'].sum()) / (g['counts'].sum() - g['mean'].sum())),
                       explained_deviance_from_cells=float((c['factors'].sum() - c['mean'].sum()) / (c['counts'].sum() - c['mean'].sum())),
                       genes_not_finite=int((~np.isfinite(g['explained_deviance'])).sum()),
                       cells_not_finite=int((~np.isfinite(c['explained_deviance'])).sum()))
        runs.append(run)
        del G, counts, forms, last
        torch.cuda.empty_cache()
    out = {'device': torch.cuda.get_device_name(0), 'model': args.model, 'cells': n, 'genes': m, 'k': K, 'fit_sweeps': args.fit_sweeps,
           'reps': args.reps, 'yardstick': bool(args.yardstick), 'runs': runs,
           'note': 'wall-clock ms around each call between two device synchronisations, medians of `reps` after a warm-up of each, '
                   'the forms alternating'}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
