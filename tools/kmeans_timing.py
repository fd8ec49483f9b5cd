# -*- coding: utf-8 -*-
"""Milliseconds per Lloyd iteration of oriana_kmeans_step against a torch formulation, in one process on the same tensors: a
REPORT, no threshold.

Workload: seeded Gaussian blobs (`--n` x `--d` float32, `--blobs` centres N(0, 3^2), noise N(0, 1)), `--c` clusters, R restarts
for every R of `--restarts`, explicit initial centres (R x C seeded rows of the data), so both sides do identical work:

    step    one oriana_kmeans_step over all R restarts plus the centre update (sums / counts in float64, an empty cluster keeps
            its centre, the cast to float32) -- one iteration of cluster.kmeans' loop
    torch   per restart torch.cdist, argmin, index_add_ of the rows into (C, d) float32 sums, bincount, the same centre update

Both are timed with device events around `--iters` consecutive iterations, after `--warmup` untimed iterations of each, `--reps`
times, the two sides alternating; the median per iteration is reported with the minimum and maximum.  Beside them: the bytes of Y
one iteration of the step reads (n * d * 4 per group of restarts that shares a row tile) and the share of the HBM peak
(`--hbm-tbs`, 8 TB/s) those bytes over the median time come to, the float32 lane-operations of the distances (n R C d 2) over the
time, and the agreement of the two sides' labels and sums after one iteration from the same centres.
Prints one JSON line; `--out` also writes it to a file.

    python tools/kmeans_timing.py --out profiles/kmeans_timing.json
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
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--d', type=int, default=100)
    ap.add_argument('--c', type=int, default=20)
    ap.add_argument('--blobs', type=int, default=20)
    ap.add_argument('--restarts', default='1,10,100')
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--hbm-tbs', type=float, default=8.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('kmeans_timing needs a GPU: there is nothing to time without one')
    from oriana_amd import cluster
    dev = torch.device('cuda', 0)
    n, d, C = args.n, args.d, args.c
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    mu = 3.0 * torch.randn(args.blobs, d, generator=g, device=dev)
    which = torch.randint(0, args.blobs, (n,), generator=g, device=dev)
    Y = mu[which]
    Y += torch.randn(n, d, generator=g, device=dev)
    del which

    def update(sums, counts, cur):
        new = torch.where(counts[..., None] > 0, sums.to(torch.float64) / counts.clamp(min=1)[..., None].to(torch.float64), cur)
        return new, new.to(torch.float32)

    def step_iter(c64, c32):
        o = cluster.lloyd_step(Y, c32)
        return update(o['sums'], o['counts'], c64)

    def torch_iter(c64, c32):
        R = c32.shape[0]
        sums = torch.zeros(R, C, d, dtype=torch.float32, device=dev)
        counts = torch.empty(R, C, dtype=torch.int64, device=dev)
        for r in range(R):
            lab = torch.cdist(Y, c32[r]).argmin(dim=1)
            sums[r].index_add_(0, lab, Y)
            counts[r] = torch.bincount(lab, minlength=C)
        return update(sums, counts, c64)

    def timed(fn, c64, c32, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            c64, c32 = fn(c64, c32)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    runs = []
    for R in [int(x) for x in args.restarts.split(',')]:
        gi = torch.Generator()
        gi.manual_seed(args.seed + R)
        rows = torch.stack([torch.randperm(n, generator=gi)[:C] for _ in range(R)]).to(dev)
        c32 = Y[rows].contiguous()
        c64 = c32.to(torch.float64)
        # one iteration of each from the same centres: do they agree?
        o = cluster.lloyd_step(Y, c32, label_restart=R - 1)
        lab_t = torch.cdist(Y, c32[R - 1]).argmin(dim=1)
        label_agreement = float((o['labels'].to(torch.int64) == lab_t).double().mean())
        sums_t = torch.zeros(C, d, dtype=torch.float64, device=dev).index_add_(0, o['labels'].to(torch.int64), Y.to(torch.float64))
        sums_err = float(((o['sums'][R - 1] - sums_t).abs().max() / sums_t.abs().max()))
        for fn in (step_iter, torch_iter):
            timed(fn, c64, c32, args.warmup)
        t_step, t_torch = [], []
        for _ in range(args.reps):
            t_step.append(timed(step_iter, c64, c32, args.iters))
            t_torch.append(timed(torch_iter, c64, c32, args.iters))
        G = cluster.restart_group(d, C)
        y_bytes = -(-R // G) * n * d * 4
        ms, mt = float(np.median(t_step)), float(np.median(t_torch))
        runs.append({'R': R, 'restarts_per_row_tile_read': G,
                     'step_ms_per_iter': ms, 'step_ms_min_max': [min(t_step), max(t_step)],
                     'torch_ms_per_iter': mt, 'torch_ms_min_max': [min(t_torch), max(t_torch)],
                     'torch_over_step': mt / ms,
                     'step_y_bytes_per_iter': y_bytes, 'step_hbm_share': y_bytes / (ms * 1e-3) / (args.hbm_tbs * 1e12),
                     'torch_y_bytes_per_iter_at_least': 2 * R * n * d * 4,
                     'step_distance_lane_ops_per_s': 2.0 * n * R * C * d / (ms * 1e-3),
                     'label_agreement_with_torch': label_agreement, 'sums_max_error_over_max_sum': sums_err})
        del rows, c32, c64, o, lab_t, sums_t
    out = {'tool': 'kmeans_timing', 'device': torch.cuda.get_device_name(0), 'n': n, 'd': d, 'C': C, 'blobs': args.blobs,
           'iters_per_window': args.iters, 'warmup_iters': args.warmup, 'reps': args.reps, 'hbm_peak_tbs': args.hbm_tbs,
           'timer': 'device events around the window', 'runs': runs}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
