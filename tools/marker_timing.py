# -*- coding: utf-8 -*-
"""Cost report of FactorModel.cluster_gene_stats() (the device half of marker_genes()): a REPORT, no threshold.

Per layout (sliced; hybrid: the dense genes in the uint16 block, engine.auto_dense_density) one GaP model on the benchmark
generator's counts (`--cells` x `--genes`, ~90 % zeros; K plays no part, the model is not fitted).  Timed, in the same run and on
the same model: cluster_gene_stats() with the defaults (normalised, log1p) for every C of `--clusters` on seeded random labels
resident on the device, cell_totals() uncached, and an uncached _count_constants() walk -- oriana_count_stats +
oriana_dense_metric, the C = 1 floor of the same traversal (one pass over the same records, per-gene sums without a cluster
axis).  Wall-clock time around each call between two device synchronisations (every call ends in a host read), medians of `--reps`
(default 5) after `--warmups` (default 2) calls of each, the forms alternating, one untimed launch before each window.
`--yardstick` times the _count_constants() walk alone: the form to run on a checkout of an earlier commit.  Prints one JSON
line; `--out` also writes it to a file.

    python tools/marker_timing.py --out profiles/marker_timing.json
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
    ap.add_argument('--cells', type=int, default=262144)
    ap.add_argument('--genes', type=int, default=30000)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--zeros', type=float, default=0.10, help='zero_inflation_level of the generator (0.10: ~90 %% zeros)')
    ap.add_argument('--clusters', default='8,64')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmups', type=int, default=2)
    ap.add_argument('--chunk-rows', type=int, default=8192)
    ap.add_argument('--layouts', default='sliced,hybrid')
    ap.add_argument('--yardstick', action='store_true', help='time the _count_constants() walk alone')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('marker_timing needs a GPU: there is nothing to time without one')
    from oriana_amd import engine, models
    from oriana_amd.singlecell import SyntheticCounts
    dev = torch.device('cuda', 0)
    n, m, K, seed = args.cells, args.genes, args.k, 1234 + 1000 * 4
    Cs = [int(c) for c in args.clusters.split(',') if c]

    tick = torch.zeros(1, device=dev)

    def timed(fn):
        # (an untimed launch first: the form before this one has just dropped its (3, C, m) host result, and the first launch
        #  after such a release was seen to wait some 20 ms -- whichever form came next, here the cheapest one)
        torch.cuda.synchronize()
        tick.add_(1.0)
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
        G = models.GaP(counts, k=K, use_factors=False, init=(a1, b1), device=dev)
        del a1, b1, gen
        print('%s: packed, nnz %d, %d dense genes' % (layout, counts.nnz, counts.gd), file=sys.stderr, flush=True)

        def count_constants():
            G._xconst = None
            return float(G._count_constants()[2][1])               # (the host read ends the walk)

        forms = {'count_constants': count_constants}
        if not args.yardstick:
            def cell_totals():
                G._xtotals = None
                return G.cell_totals()
            forms['cell_totals'] = cell_totals
            g = torch.Generator(device='cpu').manual_seed(seed)
            for C in Cs:
                lab = torch.randint(0, C, (n,), generator=g).to(dev)
                forms['cluster_gene_stats_C%d' % C] = (lambda lab=lab, C=C: G.cluster_gene_stats(lab, n_clusters=C))
        last = {}
        for _ in range(args.warmups):
            for name, f in forms.items():
                last[name] = f()
        ts = {name: [] for name in forms}
        for _ in range(args.reps):
            for name, f in forms.items():
                t, last[name] = timed(f)
                ts[name].append(t)
        med = {name: float(np.median(v)) for name, v in ts.items()}
        run = {'layout': layout, 'dense_genes': int(counts.gd), 'nnz': int(counts.nnz),
               'ms': {name: round(v, 3) for name, v in med.items()},
               'all_ms': {name: [round(t, 3) for t in v] for name, v in ts.items()},
               'sum_x2': last['count_constants']}
        if not args.yardstick:
            tot = last['cell_totals']
            run['total_counts'] = float(tot.sum())
            for C in Cs:
                st = last['cluster_gene_stats_C%d' % C]
                name = 'cluster_gene_stats_C%d' % C
                run[name + '_over_count_constants'] = round(med[name] / med['count_constants'], 3)
                # every non-zero count is counted once, whatever C: the walk visited what the layout holds
                run[name + '_n_expressing'] = float(st['n_expressing'].sum())
        runs.append(run)
        del G, counts, forms, last
        torch.cuda.empty_cache()
    out = {'device': torch.cuda.get_device_name(0), 'cells': n, 'genes': m, 'k': K, 'clusters': Cs, 'reps': args.reps,
           'warmups': args.warmups, 'yardstick': bool(args.yardstick), 'runs': runs,
           'note': 'wall-clock ms around each call between two device synchronisations (each call ends in a host read and, for '
                   'cluster_gene_stats, the copy of the (3, C, m) result to the host), medians of `reps` after `warmups` calls of '
                   'each, the forms alternating, one untimed launch before each window'}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
