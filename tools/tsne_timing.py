# -*- coding: utf-8 -*-
"""Milliseconds of the exact t-SNE gradient of cluster.tsne (csrc/tsne.hip) against a torch formulation, in one process on the
same tensors: a REPORT, no threshold.

Workload: seeded Gaussian blobs (`--n` x `--d` float32, `--blobs` centres N(0, 3^2), noise N(0, 1)) as tools/knn_timing.py draws
them; the graph is cluster.knn(Y, k) with tsne()'s default k at `--perplexity`, P is tsne_affinities() + tsne_joint(); the layout
that is timed is the one after the first 50-iteration run from the PCA start (all of it under early exaggeration).

    repulse    one cluster.tsne_repulse call, all rows against all rows
    gradient   one cluster.tsne_gradient call: attract, repulse, the float64 assembly in torch
    run        cluster.tsne(Y, graph=.., n_iter=50, exaggeration_iter=50): affinities, joint P, PCA start, 50 iterations, final KL
    torch      the float64 reference's arithmetic by broadcasting: per chunk of `--chunk` query rows the (chunk, n, 2) differences
               against all rows, w = 1 / (1 + |.|^2), rep = sum w^2 diff, zrow = sum w, on the first `--torch-rows` rows and
               scaled by n / rows; the attractive term by gathers over the non-zeros of P for all rows.  Not the code under test.

Each is timed with device events around one call, after `--warmup` untimed calls, `--reps` times; the median is reported with the
minimum and maximum.  Beside them: the lane-operations of the repulsive pass, 10 per pair (2 subtractions, 4 fused multiply-adds,
the reciprocal, one product, the conversion of w and its float64 addition), over the median time of the repulse call, next to the
rate of one vector instruction per lane and clock (`--lane-ops-peak`, 256 CUs x 128 lanes x 2.4 GHz), and the agreement of the
kernel with the torch side on its rows.  Prints one JSON line; `--out` also writes it to a file.

    python tools/tsne_timing.py --out profiles/tsne_timing.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=262144)
    ap.add_argument('--d', type=int, default=100)
    ap.add_argument('--blobs', type=int, default=20)
    ap.add_argument('--perplexity', type=float, default=20.0)
    ap.add_argument('--chunk', type=int, default=128)
    ap.add_argument('--torch-rows', type=int, default=4096)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--lane-ops-peak', type=float, default=256 * 128 * 2.4e9)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tsne_timing needs a GPU: there is nothing to time without one')
    from oriana_amd import cluster
    dev = torch.device('cuda', 0)
    n, d = args.n, args.d
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    mu = 3.0 * torch.randn(args.blobs, d, generator=g, device=dev)
    which = torch.randint(0, args.blobs, (n,), generator=g, device=dev)
    Y = mu[which]
    Y += torch.randn(n, d, generator=g, device=dev)
    del which
    k = cluster.tsne_default_neighbors(args.perplexity, d, n)
    graph = cluster.knn(Y, k)
    graph = (graph['indices'], graph['sq_distances'])
    p, _ = cluster.tsne_affinities(graph[1], args.perplexity)
    P = cluster.tsne_joint(graph[0], p)
    del p
    nt = min(args.torch_rows, n) if args.torch_rows > 0 else n

    def run_side():
        return cluster.tsne(Y, perplexity=args.perplexity, graph=graph, n_iter=50, exaggeration_iter=50)

    first = run_side()
    y32 = first['embedding'].to(torch.float32)
    y64 = y32.to(torch.float64)

    def repulse_side():
        return cluster.tsne_repulse(y32, y32)

    def gradient_side():
        return cluster.tsne_gradient(P, y32)

    def torch_repulse():
        rep = torch.empty(nt, 2, dtype=torch.float64, device=dev)
        z = torch.empty(nt, dtype=torch.float64, device=dev)
        for a in range(0, nt, args.chunk):
            b = min(a + args.chunk, nt)
            diff = y64[a:b, None, :] - y64[None, :, :]
            w = 1.0 / (1.0 + (diff * diff).sum(-1))
            z[a:b] = w.sum(1)
            rep[a:b] = ((w * w)[:, :, None] * diff).sum(1)
        return rep, z

    rows = torch.repeat_interleave(torch.arange(n, device=dev), P['crow'][1:] - P['crow'][:-1])
    cols = P['col'].to(torch.int64)

    def torch_attract():
        diff = y64[rows] - y64[cols]
        pw = P['val'].to(torch.float64) / (1.0 + (diff * diff).sum(-1))
        return torch.zeros(n, 2, dtype=torch.float64, device=dev).index_add_(0, rows, pw[:, None] * diff)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    # one call of each: do they agree?
    rep, z = repulse_side()
    trep, tz = torch_repulse()
    agree_z = float(((z[:nt] - tz).abs() / tz).max())
    agree_rep = float((rep[:nt] - trep).abs().max() / trep.abs().max())
    attr, _ = cluster.tsne_attract(P, y32)
    agree_attr = float((attr - torch_attract()).abs().max() / attr.abs().max())
    del rep, z, trep, tz, attr

    sides = (('repulse', repulse_side), ('gradient', gradient_side), ('run', run_side), ('torch_repulse', torch_repulse),
             ('torch_attract', torch_attract))
    times = {}
    for name, fn in sides:
        for _ in range(args.warmup):
            timed(fn)
        times[name] = [timed(fn) for _ in range(args.reps)]
        sys.stderr.write('%s: %s ms\n' % (name, ', '.join('%.2f' % t for t in times[name])))
        sys.stderr.flush()
    med = {name: float(np.median(t)) for name, t in times.items()}
    rate = 10.0 * n * n / (med['repulse'] * 1e-3)
    torch_gradient = med['torch_repulse'] * n / nt + med['torch_attract']
    out = {'tool': 'tsne_timing', 'device': torch.cuda.get_device_name(0), 'n': n, 'd': d, 'blobs': args.blobs,
           'perplexity': args.perplexity, 'n_neighbors': k, 'nnz_of_P': int(P['col'].numel()), 'kl_after_50_iterations': first['kl'],
           'warmup_calls': args.warmup, 'reps': args.reps, 'lane_ops_peak': args.lane_ops_peak, 'lane_ops_per_pair': 10,
           'timer': 'device events around one call', 'torch_query_rows': nt, 'torch_query_chunk': args.chunk,
           'repulse_ranges': int(cluster._repulse_scratch_bytes(n, n, 0) // (1536 * ((n + 63) // 64))),
           'ms': med, 'ms_min_max': {name: [min(t), max(t)] for name, t in times.items()},
           'run_ms_per_iteration': med['run'] / 50.0,
           'torch_repulse_ms_scaled_to_all_rows': med['torch_repulse'] * n / nt, 'torch_gradient_ms_scaled': torch_gradient,
           'torch_gradient_scaled_over_gradient': torch_gradient / med['gradient'],
           'repulse_lane_ops_per_s': rate, 'repulse_share_of_lane_ops_peak': rate / args.lane_ops_peak,
           'zrow_max_rel_difference_to_torch': agree_z, 'rep_max_difference_over_max_abs': agree_rep,
           'attr_max_difference_over_max_abs': agree_attr}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
