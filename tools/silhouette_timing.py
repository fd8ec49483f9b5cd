# -*- coding: utf-8 -*-
"""Milliseconds of one exact silhouette by cluster.silhouette (oriana_cluster_distance_sums) against the k-nearest-neighbour scan
that does the same distance arithmetic and against a torch formulation, in one process on the same tensor: a REPORT, no
threshold.

Workload: seeded Gaussian blobs (`--n` x `--d` float32, `--blobs` centres N(0, 3^2), noise N(0, 1)); two labellings: the blob of
each row (`--blobs` clusters) and the blobs merged into `--groups` groups (blob id modulo `--groups`).

    silhouette  one cluster.silhouette call per labelling (grouping of the rows by cluster, the scan, the assembly)
    knn         one cluster.knn(k = `--k`) call on the same tensor: the same n^2 d distance arithmetic, per-query lists instead of
                per-cluster sums; silhouette / knn is recorded per labelling
    torch       the practical alternative, on the first `--torch-rows` rows as queries against all rows, per chunk of `--chunk`
                query rows: torch.cdist(.., compute_mode='donot_use_mm_for_euclid_dist') -- an (n_chunk, n) float32 distance
                matrix -- then its float64 product with the (n, C) one-hot labels.  (That cdist launch fails beyond 2^24
                distances per call, tools/knn_timing.py; the tool lowers `--chunk` accordingly.)  Its time is reported as
                measured and scaled by n / rows; its sums go through silhouette_from_sums and the largest difference to
                cluster.silhouette's values over those rows is recorded.

All are timed with device events around one call, after `--warmup` untimed calls of each, `--reps` times, alternating; the median is
reported with the minimum and maximum.  Beside them the float32 lane-operations of the distances (n n d 2) over the median time,
next to the rate of one vector instruction per lane and clock (`--lane-ops-peak`).
Prints one JSON line; `--out` also writes it to a file.

    python tools/silhouette_timing.py --out profiles/silhouette_timing.json
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
    ap.add_argument('--k', type=int, default=15)
    ap.add_argument('--blobs', type=int, default=20)
    ap.add_argument('--groups', type=int, default=8)
    ap.add_argument('--chunk', type=int, default=32)
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
        raise SystemExit('silhouette_timing needs a GPU: there is nothing to time without one')
    from oriana_amd import cluster
    dev = torch.device('cuda', 0)
    n, d = args.n, args.d
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    mu = 3.0 * torch.randn(args.blobs, d, generator=g, device=dev)
    which = torch.randint(0, args.blobs, (n,), generator=g, device=dev)
    Y = mu[which]
    Y += torch.randn(n, d, generator=g, device=dev)
    chunk = max(1, min(args.chunk, (2 ** 24 - 1) // n))
    nt = min(args.torch_rows, n) if args.torch_rows > 0 else n

    def torch_sums(labels, C):
        onehot = torch.zeros(n, C, dtype=torch.float64, device=dev)
        onehot[torch.arange(n, device=dev), labels] = 1.0
        S = torch.empty(nt, C, dtype=torch.float64, device=dev)
        for a in range(0, nt, chunk):
            b = min(a + chunk, nt)
            D = torch.cdist(Y[a:b], Y, compute_mode='donot_use_mm_for_euclid_dist')
            S[a:b] = D.to(torch.float64) @ onehot
        return S

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    knn_side = lambda: cluster.knn(Y, args.k)
    runs = []
    for what, labels, C in (('blobs', which, args.blobs), ('groups', which % args.groups, args.groups)):
        sil_side = lambda: cluster.silhouette(Y, labels, n_clusters=C)
        torch_side = lambda: torch_sums(labels, C)
        # one call of each: do they agree?
        res = sil_side()
        S = torch_side()
        tv, _, _ = cluster.silhouette_from_sums(S.t().contiguous(), res['counts'], labels[:nt])
        diff = float((tv - res['values'][:nt]).abs().max())
        mean = res['mean']
        del res, S, tv
        for fn in (sil_side, knn_side, torch_side):
            for _ in range(args.warmup):
                timed(fn)
        t_sil, t_knn, t_torch = [], [], []
        for _ in range(args.reps):
            t_sil.append(timed(sil_side))
            t_knn.append(timed(knn_side))
            t_torch.append(timed(torch_side))
            sys.stderr.write('%s, repetition %d: silhouette %.1f ms, knn %.1f ms, torch %.1f ms\n'
                             % (what, len(t_sil), t_sil[-1], t_knn[-1], t_torch[-1]))
            sys.stderr.flush()
        ms, mk, mt = float(np.median(t_sil)), float(np.median(t_knn)), float(np.median(t_torch))
        rate = 2.0 * n * n * d / (ms * 1e-3)
        plan = cluster.silhouette_plan(n, n, d, C)
        runs.append({'labels': what, 'clusters': C, 'mean_silhouette': mean,
                     'silhouette_ms': ms, 'silhouette_ms_min_max': [min(t_sil), max(t_sil)],
                     'knn_k': args.k, 'knn_ms': mk, 'knn_ms_min_max': [min(t_knn), max(t_knn)], 'silhouette_over_knn': ms / mk,
                     'torch_query_rows': nt, 'torch_ms': mt, 'torch_ms_min_max': [min(t_torch), max(t_torch)],
                     'torch_ms_scaled_to_all_rows': mt * n / nt, 'torch_scaled_over_silhouette': mt * n / nt / ms,
                     'silhouette_distance_lane_ops_per_s': rate, 'silhouette_share_of_lane_ops_peak': rate / args.lane_ops_peak,
                     'values_max_difference_to_torch': diff, 'query_block': plan[0], 'candidate_chunk': plan[1],
                     'scratch_bytes': plan[2]})
    out = {'tool': 'silhouette_timing', 'device': torch.cuda.get_device_name(0), 'n': n, 'd': d, 'blobs': args.blobs,
           'torch_query_chunk': chunk, 'warmup_calls': args.warmup, 'reps': args.reps, 'lane_ops_peak': args.lane_ops_peak,
           'timer': 'device events around one call', 'runs': runs}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
