# -*- coding: utf-8 -*-
"""Cost report of FactorModel.deviance_path(): a REPORT, no threshold.

Per layout (sliced; hybrid: the dense genes on the matrix cores, engine.auto_dense_density) one model of `--model` on the
benchmark generator's counts (`--cells` x `--genes`, K = `--k`, ~90 % zeros), fitted for `--fit-sweeps` sweeps; then, in the same
run and on the same state, explained_deviance() (one pass: row pass + oriana_metric_nnz), deviance_path() with ks=None (all K
prefixes) and deviance_path() with 8 prefix lengths spread over 1..K.  Wall-clock time around each call between two device
synchronisations (the calls end in a host read), medians of `--reps` (default 5) after one warm-up call of each, the three forms
alternating.  Prints one JSON line; `--out` also writes it to a file.

    python tools/deviance_path_bench.py --out profiles/deviance_path_bench.json
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
    ap.add_argument('--cells', type=int, default=1000000)
    ap.add_argument('--genes', type=int, default=30000)
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--zeros', type=float, default=0.10, help='zero_inflation_level of the generator (0.10: ~90 %% zeros)')
    ap.add_argument('--fit-sweeps', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--chunk-rows', type=int, default=8192)
    ap.add_argument('--layouts', default='sliced,hybrid')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('deviance_path_bench needs a GPU: there is nothing to time without one')
    from oriana_amd import engine, models
    from oriana_amd.singlecell import SyntheticCounts
    dev = torch.device('cuda', 0)
    n, m, K, seed = args.cells, args.genes, args.k, 1234 + 1000 * 4
    ks8 = sorted(set(int(k) for k in np.unique(np.linspace(1, K, 8).round())))

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
        forms = {'explained_deviance': G.explained_deviance, 'deviance_path_all': G.deviance_path,
                 'deviance_path_8': lambda: G.deviance_path(ks=ks8)}
        last = {name: f() for name, f in forms.items()}                          # warm-up (scratch, count constants)
        ts = {name: [] for name in forms}
        for _ in range(args.reps):
            for name, f in forms.items():
                t, last[name] = timed(f)
                ts[name].append(t)
        med = {name: float(np.median(v)) for name, v in ts.items()}
        p = last['deviance_path_all']
        runs.append({
            'layout': layout, 'dense_genes': int(counts.gd), 'nnz': int(counts.nnz), 'ks8': ks8,
            'ms': {name: round(v, 3) for name, v in med.items()}, 'all_ms': {name: [round(t, 3) for t in v] for name, v in ts.items()},
            'path_all_over_explained_deviance': round(med['deviance_path_all'] / med['explained_deviance'], 3),
            'path_8_over_explained_deviance': round(med['deviance_path_8'] / med['explained_deviance'], 3),
            'explained_deviance': float(last['explained_deviance']), 'path_at_K': float(p['explained_deviance'][-1]),
            'path_at_ks8': [float(v) for v in last['deviance_path_8']['explained_deviance']]})
        del G, counts, forms, last
        torch.cuda.empty_cache()
    out = {'device': torch.cuda.get_device_name(0), 'model': args.model, 'cells': n, 'genes': m, 'k': K, 'fit_sweeps': args.fit_sweeps,
           'reps': args.reps, 'runs': runs,
           'note': 'wall-clock ms around each call between two device synchronisations, medians of `reps` after a warm-up of each, '
                   'the three forms alternating'}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
