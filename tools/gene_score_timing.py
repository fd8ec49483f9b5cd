# -*- coding: utf-8 -*-
"""Cost report of oriana_gene_scores (the device half of FactorModel.gene_scores() / score_genes()): a REPORT, no threshold.

Per layout (sliced; hybrid: the dense genes in the uint16 block, engine.auto_dense_density) one GaP model on the matrix of
tools/marker_timing.py (the benchmark generator's `--cells` x `--genes` counts, ~90 % zeros; the model is not fitted).  Timed in
ONE process with device events around each form, `--warmups` (2) untimed calls, then median and range of `--reps` (5), the forms
alternating:

  gene_scores_S<S>   the entry on device-resident W (N(0, 1), seeded), scales and output, defaults (normalised, log1p), for
                     S = 1, one chunk (oriana_gene_scores_set_chunk()) and 64; `method_S<S>` is FactorModel.gene_scores(W,
                     as_tensor=True) around it (the scale formed, the weights checked, the output allocated);
  cell_totals        (a) oriana_cell_totals on the same layouts: the unweighted walk over the same records, the floor of one chunk;
  sparse_mm_S<S>     (b) the route without this entry: torch.sparse.mm of a float64 CSR matrix of y (int32 indices) with W on the
                     device, timed WITHOUT building that matrix; `csr_build_s` is the time to build it from the generator's
                     chunks once the totals are known (host clock, seconds), reported apart.  A failure of that route is
                     recorded as such and nothing is measured for it.

The largest |gene_scores - sparse.mm| relative to sum_j |W| y is recorded as a sanity check of both, not as a test.  Prints one
JSON line; `--out` also writes it to a file.

    python tools/gene_score_timing.py --out profiles/gene_score_timing.json
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
    ap.add_argument('--sets', default=None, help='comma-separated S (default: 1, the chunk, 64)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmups', type=int, default=2)
    ap.add_argument('--chunk-rows', type=int, default=8192)
    ap.add_argument('--layouts', default='sliced,hybrid')
    ap.add_argument('--no-sparse-mm', action='store_true', help='skip baseline (b)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('gene_score_timing needs a GPU: there is nothing to time without one')
    from oriana_amd import engine, models, _lib
    from oriana_amd._lib import call, ptr, stream_ptr
    from oriana_amd.singlecell import SyntheticCounts
    dev = torch.device('cuda', 0)
    n, m, K, seed = args.cells, args.genes, args.k, 1234 + 1000 * 4
    ch = int(_lib.load().oriana_gene_scores_set_chunk())
    Ss = [int(s) for s in args.sets.split(',') if s] if args.sets else [1, ch, 64]
    g = torch.Generator(device='cpu').manual_seed(seed)
    Ws = {S: torch.randn(m, S, generator=g, dtype=torch.float64).to(dev) for S in Ss}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def measure(forms):
        last = {}
        for _ in range(args.warmups):
            for name, f in forms.items():
                last[name] = f()
        torch.cuda.synchronize()
        ts = {name: [] for name in forms}
        for _ in range(args.reps):
            for name, f in forms.items():
                t, last[name] = timed(f)
                ts[name].append(t)
        return {name: {'median_ms': round(float(np.median(v)), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3)}
                for name, v in ts.items()}, last

    runs, sparse = [], None
    for layout in args.layouts.split(','):
        dd = engine.auto_dense_density(n, m, K) if layout == 'hybrid' and engine.dense_supported(K) else None
        if layout == 'hybrid' and not dd:
            runs.append({'layout': layout, 'skipped': 'no dense block at this shape / K'})
            continue
        gen = SyntheticCounts(n, m, K, seed=seed, device=dev, zero_inflation_level=args.zeros)
        counts = engine.CountTiles.from_chunks(n, m, gen.chunk, args.chunk_rows, dev, dense_density=dd)
        a1, b1 = gen.initial_shapes()
        G = models.GaP(counts, k=K, use_factors=False, init=(a1, b1), device=dev)
        del a1, b1
        print('%s: packed, nnz %d, %d dense genes' % (layout, counts.nnz, counts.gd), file=sys.stderr, flush=True)
        ct = G.counts
        dstruct = ct.dense.c_struct if ct.dense is not None else None
        tot = G._cell_totals_device()
        scale = torch.where(tot > 0, 1e4 / tot, torch.zeros_like(tot)).contiguous()
        totbuf = torch.zeros(n, dtype=torch.float64, device=dev)
        outs = {S: torch.empty(n, S, dtype=torch.float64, device=dev) for S in Ss}

        def entry(S):
            call('oriana_gene_scores', ct.sparse_struct, dstruct, ptr(ct.row_perm), ptr(ct.col_perm), ptr(scale), 1, ptr(Ws[S]), S,
                 ptr(outs[S]), stream_ptr())
            return outs[S]

        def totals():
            call('oriana_cell_totals', ct.sparse_struct, dstruct, ptr(ct.row_perm), ptr(ct.col_perm), ptr(totbuf), stream_ptr())
            return totbuf

        forms = {'cell_totals': totals}
        for S in Ss:
            forms['gene_scores_S%d' % S] = (lambda S=S: entry(S))
            forms['method_S%d' % S] = (lambda S=S: G.gene_scores(Ws[S], as_tensor=True))
        ms, last = measure(forms)
        run = {'layout': layout, 'dense_genes': int(counts.gd), 'nnz': int(counts.nnz), 'ms': ms}
        for S in Ss:
            run['gene_scores_S%d_over_cell_totals' % S] = round(ms['gene_scores_S%d' % S]['median_ms'] / ms['cell_totals']['median_ms'], 3)
            assert torch.equal(last['gene_scores_S%d' % S], last['method_S%d' % S]), 'the entry and the method disagree'

        if sparse is None and not args.no_sparse_mm:
            sparse = {}
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                crow, cols, vals = [torch.zeros(1, dtype=torch.int64, device=dev)], [], []
                for r0 in range(0, n, args.chunk_rows):
                    r1 = min(n, r0 + args.chunk_rows)
                    Xc = gen.chunk(r0, r1)
                    nz = Xc != 0
                    crow.append(nz.sum(dim=1))
                    rc = nz.nonzero()
                    cols.append(rc[:, 1].to(torch.int32))
                    vals.append(torch.log1p(Xc[nz].double() * scale[r0:r1][rc[:, 0]]))
                    del Xc, nz, rc
                crow = torch.cumsum(torch.cat(crow), 0).to(torch.int32)
                Y = torch.sparse_csr_tensor(crow, torch.cat(cols), torch.cat(vals), size=(n, m))
                del cols, vals
                torch.cuda.synchronize()
                sparse['csr_build_s'] = round(time.perf_counter() - t0, 2)
                sparse['csr_bytes'] = int(Y.values().numel() * 12 + (n + 1) * 4)
                sms, slast = measure({'sparse_mm_S%d' % S: (lambda S=S: torch.sparse.mm(Y, Ws[S])) for S in Ss})
                sparse['ms'] = sms
                mag = {S: torch.sparse.mm(Y, Ws[S].abs()) for S in Ss}
                sparse['max_rel_diff'] = {str(S): float(((slast['sparse_mm_S%d' % S] - last['gene_scores_S%d' % S]).abs()
                                                         / mag[S].clamp_min(1e-300)).max()) for S in Ss}
                del Y, slast, mag
            except Exception as e:                                  # (the route is a comparison, not a dependency)
                sparse['failed'] = '%s: %s' % (type(e).__name__, str(e)[:300])
            torch.cuda.empty_cache()
        if sparse and 'ms' in sparse:
            for S in Ss:
                run['sparse_mm_S%d_over_gene_scores' % S] = round(sparse['ms']['sparse_mm_S%d' % S]['median_ms']
                                                                  / ms['gene_scores_S%d' % S]['median_ms'], 3)
        runs.append(run)
        del G, counts, ct, forms, last, gen, outs
        torch.cuda.empty_cache()
    out = {'device': torch.cuda.get_device_name(0), 'cells': n, 'genes': m, 'k': K, 'sets': Ss, 'set_chunk': ch, 'reps': args.reps,
           'warmups': args.warmups, 'runs': runs, 'sparse_mm': sparse if sparse is not None else 'not measured',
           'note': 'device-event ms around each form in one process: `warmups` untimed calls of each, then median / min / max of '
                   '`reps`, the forms alternating; sparse_mm is timed without building its matrix (csr_build_s: host clock)'}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
