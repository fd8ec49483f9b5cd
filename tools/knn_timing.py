# -*- coding: utf-8 -*-
"""Milliseconds of one exact k-nearest-neighbour graph by cluster.knn (oriana_knn) against a torch formulation, in one process on
the same tensors: a REPORT, no threshold.

Workload: seeded Gaussian blobs (`--n` x `--d` float32, `--blobs` centres N(0, 3^2), noise N(0, 1)); for every k of `--k` the k
nearest other rows of every row:

    knn     one cluster.knn call (the default: one oriana_knn call, no distance matrix)
    torch   per chunk of `--chunk` query rows torch.cdist(.., compute_mode='donot_use_mm_for_euclid_dist') against all rows -- an
            (n_chunk, n) float32 distance matrix in device memory -- then topk(k + 1, largest=False, sorted=True) and the row's own
            index dropped.  That cdist launch fails ("invalid configuration argument") at 2,048 x 262,144 distances per call:
            it appears to take one work-group of 256 threads per distance, and a launch holds fewer than 2^32 threads, so a
            chunk holds fewer than 2^24 / n rows (63 at n = 262,144; the tool lowers `--chunk` to that).
            `--torch-rows` (default: all) limits this side to the first rows as queries, still against all rows: its time is
            reported as measured and scaled by n / rows, and the agreement is taken over those rows.

Both are timed with device events around one call, after `--warmup` untimed calls of each, `--reps` times, the two sides
alternating; the median is reported with the minimum and maximum (the defaults, two warm-up calls and five repetitions, are those
of tools/kmeans_timing.py; one call of the torch side takes 50 s at the default size, so a run takes a quarter of an hour).
Beside them: the float32 lane-operations of the distances
(n n d 2: one subtraction and one fused multiply-add per pair and feature) over the median time, next to the rate of one vector
instruction per lane and clock (`--lane-ops-peak`, 256 CUs x 128 lanes x 2.4 GHz), and the agreement of the two sides: the share
of cluster.knn's neighbours that the torch side lists for the same row, and the largest relative difference between the squared
distances of the first neighbours.
`--waves 4` sets ORIANA_KNN_WAVES=4 before the library is loaded: work-groups of four waves at every k (a tuning run; the
results do not change), recorded as 'waves_per_work_group'.
Prints one JSON line; `--out` also writes it to a file.

    python tools/knn_timing.py --out profiles/knn_timing.json
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
    ap.add_argument('--k', default='15,30')
    ap.add_argument('--blobs', type=int, default=20)
    ap.add_argument('--chunk', type=int, default=32)
    ap.add_argument('--torch-rows', type=int, default=0)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--lane-ops-peak', type=float, default=256 * 128 * 2.4e9)
    ap.add_argument('--waves', type=int, default=0, choices=(0, 4))
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('knn_timing needs a GPU: there is nothing to time without one')
    if args.waves:
        os.environ['ORIANA_KNN_WAVES'] = str(args.waves)
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
    rows = torch.arange(n, device=dev)
    chunk = max(1, min(args.chunk, (2 ** 24 - 1) // n))
    nt = min(args.torch_rows, n) if args.torch_rows > 0 else n

    def knn_side(k):
        o = cluster.knn(Y, k)
        return o['indices'], o['sq_distances']

    def torch_side(k):
        idx = torch.empty(nt, k, dtype=torch.int64, device=dev)
        dist = torch.empty(nt, k, dtype=torch.float32, device=dev)
        for a in range(0, nt, chunk):
            b = min(a + chunk, nt)
            D = torch.cdist(Y[a:b], Y, compute_mode='donot_use_mm_for_euclid_dist')
            v, i = torch.topk(D, k + 1, dim=1, largest=False, sorted=True)
            # the row's own index out of its k + 1 (where it is not among them -- duplicates -- the last one goes)
            own = i == rows[a:b, None]
            own[:, k] |= ~own.any(dim=1)
            keep = ~own
            idx[a:b] = i[keep].view(-1, k)
            dist[a:b] = v[keep].view(-1, k)
        return idx, dist

    def timed(fn, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(k)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    runs = []
    for k in [int(x) for x in args.k.split(',')]:
        # one call of each: do they agree?
        ki, kd = knn_side(k)
        ti, td = torch_side(k)
        hit = 0
        for a in range(0, nt, 65536):
            b = min(a + 65536, nt)
            hit += int((ki[a:b, :, None].to(torch.int64) == ti[a:b, None, :]).any(dim=2).sum())
        first = float(((kd[:nt, 0].sqrt() - td[:, 0]).abs() / td[:, 0].clamp(min=1e-30)).max())
        del ki, kd, ti, td
        for fn in (knn_side, torch_side):
            for _ in range(args.warmup):
                timed(fn, k)
        t_knn, t_torch = [], []
        for _ in range(args.reps):
            t_knn.append(timed(knn_side, k))
            t_torch.append(timed(torch_side, k))
            sys.stderr.write('k = %d, repetition %d: knn %.1f ms, torch %.1f ms\n' % (k, len(t_knn), t_knn[-1], t_torch[-1]))
            sys.stderr.flush()
        mk, mt = float(np.median(t_knn)), float(np.median(t_torch))
        sys.stderr.write('k = %d: knn %.1f ms, torch %.1f ms for %d of %d query rows\n' % (k, mk, mt, nt, n))
        sys.stderr.flush()
        rate = 2.0 * n * n * d / (mk * 1e-3)
        runs.append({'k': k, 'knn_ms': mk, 'knn_ms_min_max': [min(t_knn), max(t_knn)],
                     'torch_query_rows': nt, 'torch_ms': mt, 'torch_ms_min_max': [min(t_torch), max(t_torch)],
                     'torch_ms_scaled_to_all_rows': mt * n / nt, 'torch_scaled_over_knn': mt * n / nt / mk,
                     'knn_distance_lane_ops_per_s': rate, 'knn_share_of_lane_ops_peak': rate / args.lane_ops_peak,
                     'torch_distance_matrix_bytes_per_chunk': chunk * n * 4,
                     'knn_neighbours_listed_by_torch': hit / float(nt * k),
                     'first_neighbour_distance_max_rel_difference': first,
                     'candidate_splits': int(cluster._lib.load().oriana_knn_splits(n, n, d, k, 0)),
                     'waves_per_work_group': int(cluster._lib.load().oriana_knn_waves(d, k))})
    out = {'tool': 'knn_timing', 'device': torch.cuda.get_device_name(0), 'n': n, 'd': d, 'blobs': args.blobs,
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
