# -*- coding: utf-8 -*-
"""Cost report of FactorModel.cluster_rank_sums() (the device half of marker_genes(method='wilcoxon')): a REPORT, no threshold.

Per layout (sliced; hybrid: the dense genes in the uint16 block, engine.auto_dense_density) one GaP model on the benchmark
generator's counts (`--cells` x `--genes`, ~90 % zeros; K plays no part, the model is not fitted).  Timed, in the same process and
on the same model, for every C of `--clusters` on seeded random labels resident on the device: cluster_rank_sums() with the
defaults, and cluster_gene_stats() at the same C -- the t-test's device cost, its code unchanged.  Second yardstick: torch.sort of
one int64 tensor with as many keys as the largest panel holds, the library's unsegmented sort without a payload; scaled by the
number of records over all panels it says what one such sort per panel would cost.  Wall-clock time around each call between two
device synchronisations, medians of `--reps` (default 5) after `--warmups` (default 2) calls of each, the forms alternating.
`--once` runs cluster_rank_sums() a single time per C after one warm-up and times nothing: the form to put behind
`rocprofv3 --kernel-trace --stats --` for the split by kernel.  Prints one JSON line; `--out` also writes it to a file.

    python tools/wilcoxon_timing.py --out profiles/wilcoxon_timing.json
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
    ap.add_argument('--scratch-bytes', type=int, default=1 << 30)
    ap.add_argument('--once', action='store_true', help='one untimed cluster_rank_sums() per C after a warm-up (for a kernel trace)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('wilcoxon_timing needs a GPU: there is nothing to time without one')
    from oriana_amd import engine, markers, models
    from oriana_amd.singlecell import SyntheticCounts
    dev = torch.device('cuda', 0)
    n, m, K, seed = args.cells, args.genes, args.k, 1234 + 1000 * 4
    Cs = [int(c) for c in args.clusters.split(',') if c]

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
        G = models.GaP(counts, k=K, use_factors=False, init=(a1, b1), device=dev)
        del a1, b1, gen
        print('%s: packed, nnz %d, %d dense genes' % (layout, counts.nnz, counts.gd), file=sys.stderr, flush=True)
        perm = counts.col_perm.cpu().numpy() if counts.col_perm is not None else np.arange(m)
        nnz_packed = np.rint(G._count_constants()[1].cpu().numpy()).astype(np.int64)[perm]
        panels = markers.plan_rank_panels(nnz_packed, counts.gd, args.scratch_bytes // 24)
        largest = max(p[2] for p in panels)

        g = torch.Generator(device='cpu').manual_seed(seed)
        forms = {}
        for C in Cs:
            lab = torch.randint(0, C, (n,), generator=g).to(dev)
            forms['cluster_rank_sums_C%d' % C] = (lambda lab=lab, C=C: G.cluster_rank_sums(lab, n_clusters=C,
                                                                                           scratch_bytes=args.scratch_bytes))
            if not args.once:
                forms['cluster_gene_stats_C%d' % C] = (lambda lab=lab, C=C: G.cluster_gene_stats(lab, n_clusters=C))
        if not args.once:
            keys = torch.randint(0, 2 ** 62, (largest,), generator=g, dtype=torch.int64).to(dev)
            forms['torch_sort_largest_panel'] = lambda: int(torch.sort(keys).values[0])
        last = {}
        for w in range(1 if args.once else args.warmups):
            for name, f in forms.items():
                t, last[name] = timed(f)
                print('%s: warm-up %d %s %.1f ms' % (layout, w, name, t), file=sys.stderr, flush=True)
        ts = {name: [] for name in forms}
        for _ in range(1 if args.once else args.reps):
            for name, f in forms.items():
                t, last[name] = timed(f)
                ts[name].append(t)
        run = {'layout': layout, 'dense_genes': int(counts.gd), 'nnz': int(counts.nnz), 'panels': len(panels),
               'largest_panel_records': int(largest), 'longest_gene': int(nnz_packed.max())}
        if not args.once:
            med = {name: float(np.median(v)) for name, v in ts.items()}
            run['ms'] = {name: round(v, 3) for name, v in med.items()}
            run['all_ms'] = {name: [round(t, 3) for t in v] for name, v in ts.items()}
            run['torch_sort_scaled_to_all_panels_ms'] = round(med['torch_sort_largest_panel'] * counts.nnz / largest, 3)
            for C in Cs:
                name = 'cluster_rank_sums_C%d' % C
                run[name + '_over_cluster_gene_stats'] = round(med[name] / med['cluster_gene_stats_C%d' % C], 3)
                run[name + '_over_torch_sort_scaled'] = round(med[name] / run['torch_sort_scaled_to_all_panels_ms'], 3)
                # every stored count is ranked once, whatever C, and the ranks of a gene's n cells add up to n (n + 1) / 2
                run[name + '_n_expressing'] = float(last[name]['n_expressing'].sum())
                run[name + '_genes_whose_ranks_add_up'] = int((last[name]['rank_sum'].sum(0) == n * (n + 1) / 2.0).sum())
        runs.append(run)
        del G, counts, forms, last
        torch.cuda.empty_cache()
    out = {'device': torch.cuda.get_device_name(0), 'cells': n, 'genes': m, 'k': K, 'clusters': Cs, 'reps': args.reps,
           'warmups': args.warmups, 'scratch_bytes': args.scratch_bytes, 'once': bool(args.once), 'runs': runs,
           'note': 'wall-clock ms around each call between two device synchronisations (cluster_rank_sums and cluster_gene_stats end '
                   'in the copy of their (C, m) results to the host and include their host assembly), medians of `reps` after '
                   '`warmups` calls of each, the forms alternating; torch_sort: one int64 tensor of largest_panel_records random keys, '
                   'no payload; scaled: times nnz / largest_panel_records'}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
