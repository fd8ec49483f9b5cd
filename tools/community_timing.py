# -*- coding: utf-8 -*-
"""Milliseconds of the community functions of cluster.py (csrc/community.hip) against the same sweep written in torch, in one
process on the same tensors: a REPORT, no threshold.

Workload: the seeded Gaussian blobs of tools/tsne_timing.py (`--n` x `--d` float32, `--blobs` centres N(0, 3^2), noise N(0, 1)); the
neighbour lists are cluster.knn(Y, `--k`), the graph is cluster.snn_graph(indices, 'snn').

    snn_weights     one oriana_snn_weights call on the pattern
    snn_graph       one cluster.snn_graph call: the repeat check, the pattern by torch, the weights
    sweep_first     one cluster.louvain_sweep call at level 0 from singletons
    sweep_later     the same from the state after five sweeps (each applied whatever it does to the modularity)
    louvain         one cluster.louvain run (its per-level sweep counts are reported)
    torch_first / torch_later   THE SAME SWEEP BY TORCH: keys (i, comm[j]) of all stored entries, torch.unique (a sort), a segment
                    sum by index_add_, the gains in float64 in the kernel's order, the per-row argmax by two scatter_reduce_.  It
                    is what a user would write without the kernel; its result must equal the kernel's, label for label.

Each is timed with device events around one call, after `--warmup` untimed calls, `--reps` times; the median is reported with the
minimum and maximum.  Beside them: the bytes one sweep must move (16 per stored entry: column, weight and the gathered community;
24 per row: pointer, degree, community, result) over `--hbm-rate` as a floor.  `--quality FILE` embeds a JSON object produced by
`--quality-only` (which needs no GPU: the modularity of tests/community_reference.py on the test cases over the worst of five
seeded runs of networkx's Louvain).  Prints one JSON line; `--out` also writes it to a file.

    python tools/community_timing.py --quality-only --out quality.json
    python tools/community_timing.py --quality quality.json --out profiles/community_timing.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def quality():
    """ours / worst-of-five networkx per (case, weights, resolution), on the host."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import networkx as nx
    import community_cases as cc
    import community_reference as cr
    out = {}
    for name in cc.ALL_CASES:
        for weights in cc.WEIGHTS:
            crow, col, w = cc.graph(name, weights)
            G = nx.Graph()
            G.add_nodes_from(range(crow.size - 1))
            for i, j, v in zip(cr.graph_rows(crow).tolist(), col.tolist(), w.tolist()):
                if i <= j:
                    G.add_edge(i, j, weight=v if i < j else v // 2)
            for gamma in cc.GAMMAS:
                if gamma != 1.0 and name not in ('blobs130', 'blobs600'):
                    continue
                theirs = min(nx.community.modularity(G, nx.community.louvain_communities(G, weight='weight', resolution=gamma, seed=s),
                                                     weight='weight', resolution=gamma) for s in range(5))
                ours = cc.run(name, weights, gamma)['modularity']
                out['%s/%s/%g' % (name, weights, gamma)] = {'ours': ours, 'networkx_worst_of_5': theirs,
                                                           'ratio': ours / theirs if theirs else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=262144)
    ap.add_argument('--d', type=int, default=100)
    ap.add_argument('--blobs', type=int, default=20)
    ap.add_argument('--k', type=int, default=15)
    ap.add_argument('--resolution', type=float, default=1.0)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--hbm-rate', type=float, default=6.29e12)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--quality', default=None)
    ap.add_argument('--quality-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    def emit(out):
        line = json.dumps(out)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write(line + '\n')

    if args.quality_only:
        return emit(quality())

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('community_timing needs a GPU: there is nothing to time without one')
    from oriana_amd import cluster
    from oriana_amd._lib import call, ptr, stream_ptr
    dev = torch.device('cuda', 0)
    n, d, gamma = args.n, args.d, args.resolution
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    mu = 3.0 * torch.randn(args.blobs, d, generator=gen, device=dev)
    which = torch.randint(0, args.blobs, (n,), generator=gen, device=dev)
    Y = mu[which]
    Y += torch.randn(n, d, generator=gen, device=dev)
    idx = cluster.knn(Y, args.k)['indices']
    del Y
    g = cluster.snn_graph(idx, 'snn')
    crow, col, w = g['crow'], g['col'], g['weight']
    nnz = int(col.numel())
    rows = cluster._graph_rows(crow, n)
    col64 = col.to(torch.int64)
    deg = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, rows, w)
    two_m = int(deg.sum())
    plan = cluster.louvain_plan(g)
    lens = crow[1:] - crow[:-1]

    def state_of(comm):
        tot, size, _, _ = cluster._partition_sums(rows, col, w, deg, comm, n)
        return comm, tot, size

    first = state_of(torch.arange(n, device=dev, dtype=torch.int32))
    later = first
    for _ in range(5):
        later = state_of(cluster.louvain_sweep(g, deg, two_m, *later, gamma, plan=plan)['comm'])

    def hip_sweep(state):
        return cluster.louvain_sweep(g, deg, two_m, *state, gamma, plan=plan)

    me = torch.arange(n, device=dev, dtype=torch.int64)
    zeros = torch.zeros(n, dtype=torch.int64, device=dev)

    def torch_sweep(state):
        comm, tot, size = state
        c64 = comm.to(torch.int64)
        keep = col64 != rows
        r = torch.cat([rows[keep], me])
        c = torch.cat([c64[col64[keep]], c64])
        ww = torch.cat([w[keep], zeros])
        uk, inv = torch.unique(r * n + c, return_inverse=True)
        k = torch.zeros(int(uk.numel()), dtype=torch.int64, device=dev).index_add_(0, inv, ww)
        ur = torch.div(uk, n, rounding_mode='floor')
        uc = uk - ur * n
        a, di = c64[ur], deg[ur]
        own = uc == a
        totp = tot[uc] - torch.where(own, di, torch.zeros_like(di))
        gain = (two_m * k).to(torch.float64) - gamma * (di * totp).to(torch.float64)
        gmax = torch.full((n,), -float('inf'), dtype=torch.float64, device=dev).scatter_reduce_(0, ur, gain, 'amax')
        bc = torch.full((n,), n, dtype=torch.int64, device=dev).scatter_reduce_(0, ur, torch.where(gain == gmax[ur], uc, n), 'amin')
        ga = torch.empty(n, dtype=torch.float64, device=dev)
        ga[ur[own]] = gain[own]
        move = (bc != c64) & (gmax > ga)
        move &= ~((size[c64] == 1) & (size[bc] == 1) & ~(bc < c64))
        return {'comm': torch.where(move, bc, c64).to(torch.int32), 'moved': move.sum().reshape(1)}

    def snn_weights_side():
        out = torch.empty(nnz, dtype=torch.int64, device=dev)
        call('oriana_snn_weights', ptr(idx), n, args.k, ptr(crow), ptr(col), ptr(out), stream_ptr())
        return out

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    equal = {}
    for name, state in (('first', first), ('later', later)):
        h, t = hip_sweep(state), torch_sweep(state)
        equal[name] = bool(torch.equal(h['comm'], t['comm'])) and int(h['moved'][0]) == int(t['moved'][0])
        equal[name + '_moved'] = int(h['moved'][0])
    run = cluster.louvain(g, resolution=gamma)

    sides = (('snn_weights', snn_weights_side), ('snn_graph', lambda: cluster.snn_graph(idx, 'snn')),
             ('sweep_first', lambda: hip_sweep(first)), ('sweep_later', lambda: hip_sweep(later)),
             ('torch_first', lambda: torch_sweep(first)), ('torch_later', lambda: torch_sweep(later)),
             ('louvain', lambda: cluster.louvain(g, resolution=gamma)))
    times = {}
    for name, fn in sides:
        for _ in range(args.warmup):
            timed(fn)
        times[name] = [timed(fn) for _ in range(args.reps)]
        sys.stderr.write('%s: %s ms\n' % (name, ', '.join('%.3f' % t for t in times[name])))
        sys.stderr.flush()
    med = {name: float(np.median(t)) for name, t in times.items()}
    sweep_bytes = 16 * nnz + 24 * n
    floor_ms = sweep_bytes / args.hbm_rate * 1e3
    out = {'tool': 'community_timing', 'device': torch.cuda.get_device_name(0), 'n': n, 'd': d, 'blobs': args.blobs, 'k': args.k,
           'resolution': gamma, 'stored_entries': nnz, 'two_m': two_m, 'longest_row': int(lens.max()),
           'rows_beyond_row_cap': int(plan['long_rows'].numel()), 'row_cap': plan['row_cap'], 'warmup_calls': args.warmup,
           'reps': args.reps, 'timer': 'device events around one call', 'ms': med,
           'ms_min_max': {name: [min(t), max(t)] for name, t in times.items()},
           'sweep_equals_torch': equal,
           'torch_first_min_over_sweep_first_median': min(times['torch_first']) / med['sweep_first'],
           'torch_later_min_over_sweep_later_median': min(times['torch_later']) / med['sweep_later'],
           'sweep_bytes': sweep_bytes, 'hbm_rate': args.hbm_rate, 'sweep_floor_ms': floor_ms,
           'sweep_first_over_floor': med['sweep_first'] / floor_ms, 'sweep_later_over_floor': med['sweep_later'] / floor_ms,
           'louvain': {'n_communities': run['n_communities'], 'modularity': run['modularity'],
                       'levels': [{'nodes': lev['nodes'], 'sweeps': lev['sweeps'], 'hit_max_sweeps': lev['hit_max_sweeps']}
                                  for lev in run['levels']]}}
    if args.quality:
        with open(args.quality) as f:
            out['quality_against_networkx_on_the_test_cases'] = json.load(f)
    emit(out)


if __name__ == '__main__':
    main()
