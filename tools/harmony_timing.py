# -*- coding: utf-8 -*-
"""Milliseconds of the three Harmony entries, of one round and of one full run of cluster.harmony against the same arithmetic in
torch, in one process on the same tensors: a REPORT, no threshold.

Workload: seeded Gaussian blobs (`--n` x `--d` float32, `--types` centres N(0, 3^2), one offset N(0, 1.5^2) per batch, noise
N(0, 1)), `--b` batches, `--k` clusters, explicit start centres (seeded rows; the k-means start serves fewer clusters than the
kernels at this width).  Timed, each against its torch twin:

    assign    one oriana_harmony_assign over all rows         torch: matmul, min, exp, the gathered penalty, row sums, per-batch sums
    moments   one oriana_harmony_moments                      torch: per batch index_select, matmul and column sums
    correct   one oriana_harmony_correct                      torch: per batch matmul against W[:, b], then the row norms
    round     the centres from the moments, then `--blocks` block visits with the O / E / P updates between them
    run       cluster.harmony with its defaults (eps_cluster, eps_harmony, 10 x 20 rounds at the most); the torch twin runs the
              same number of rounds per iteration as the run reported

Every window has `--warmup` untimed calls, then `--reps` timed ones between device events; the median is reported with the
minimum and maximum.  Beside them the float32 lane operations of the call (2 n K d for assign, moments and correct) over the
median time as a share of the float32 vector peak (`--f32-tflops`), and the bytes the call must move at least (its inputs and
outputs once) as a share of the HBM peak (`--hbm-tbs`).  Prints one JSON line; `--out` also writes it to a file.

    python tools/harmony_timing.py --out profiles/harmony_timing.json
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
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--b', type=int, default=8)
    ap.add_argument('--types', type=int, default=10)
    ap.add_argument('--blocks', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--hbm-tbs', type=float, default=8.0)
    ap.add_argument('--f32-tflops', type=float, default=157.3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--skip-run', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('harmony_timing needs a GPU: there is nothing to time without one')
    from oriana_amd import cluster
    dev = torch.device('cuda', 0)
    n, d, K, B, nb = args.n, args.d, args.k, args.b, args.blocks
    f64 = torch.float64
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    mu = 3.0 * torch.randn(args.types, d, generator=g, device=dev)
    off = 1.5 * torch.randn(B, d, generator=g, device=dev)
    which = torch.randint(0, args.types, (n,), generator=g, device=dev)
    batch64 = torch.randint(0, B, (n,), generator=g, device=dev)
    Z = (mu[which] + off[batch64] + torch.randn(n, d, generator=g, device=dev)).contiguous()
    batch = batch64.to(torch.int32)
    Zcos = (Z / Z.norm(dim=1, keepdim=True)).contiguous()
    gi = torch.Generator()
    gi.manual_seed(args.seed)
    c0 = Zcos[torch.randperm(n, generator=gi)[:K].to(dev)].contiguous()
    P = torch.exp(torch.randn(K, B, generator=g, device=dev) * 0.3).contiguous()
    inv_sigma = 10.0
    Pr = torch.bincount(batch64, minlength=B).to(f64) / n
    theta = torch.full((B,), 2.0, dtype=f64, device=dev)
    idx = [torch.nonzero(batch64 == b).squeeze(1) for b in range(B)]
    cuts = cluster.harmony_block_cuts(n, nb)
    blk_idx = [[torch.nonzero(batch64[cuts[j]:cuts[j + 1]] == b).squeeze(1) for b in range(B)] for j in range(nb)]

    # ---- the torch twins
    def batch_sums(R, rows_of):
        # per batch a float64 column sum of its rows (index_add_ of the (n, K) rows into a (B, K) table is 26 million atomic
        # additions on 800 addresses: 170 ms at this shape, which no one would write)
        return torch.stack([R.index_select(0, i).sum(0, dtype=f64) for i in rows_of], dim=1)

    def t_assign(zc, bt, rows_of, cen, Pm, R_out):
        dist = 2.0 - 2.0 * (zc @ cen.t())
        e = torch.exp(-(dist - dist.min(dim=1, keepdim=True).values) * inv_sigma) * Pm.t()[bt]
        R = e / e.sum(dim=1, keepdim=True)
        R_out.copy_(R)
        return batch_sums(R, rows_of), (R * dist).sum(dtype=f64), torch.xlogy(R, R).sum(dtype=f64)

    def t_moments(X, R):
        S = torch.stack([R.index_select(0, i).t() @ X.index_select(0, i) for i in idx], dim=1).to(f64)
        return S, batch_sums(R, idx)

    def t_correct(X, R, W):
        Zc = torch.empty_like(X)
        for b, i in enumerate(idx):
            Zc[i] = X.index_select(0, i) - R.index_select(0, i) @ W[:, b, :]
        nr = Zc.norm(dim=1, keepdim=True)
        return Zc, torch.where(nr > 0, Zc / nr, torch.zeros_like(Zc))

    def objective(sums, O, E, sigma=0.1):
        return sums[:, 0].sum() + sigma * sums[:, 1].sum() + sigma * (theta[None, :] * O * torch.log((O + 1.0) / (E + 1.0))).sum()

    def centres(S, cen64):
        C = S.sum(1)
        cn = torch.sqrt((C * C).sum(1, keepdim=True))
        return torch.where(cn > 0, C / torch.where(cn > 0, cn, torch.ones_like(cn)), cen64)

    st = {}

    def reset():
        st['R'] = torch.zeros(n, K, dtype=torch.float32, device=dev)
        st['O_blk'] = torch.zeros(nb, K, B, dtype=f64, device=dev)
        st['sums'] = torch.zeros(nb, 2, dtype=f64, device=dev)
        st['cen64'] = c0.to(f64)
        ones = torch.ones(K, B, dtype=torch.float32, device=dev)
        for j in range(nb):
            cluster.harmony_assign(Zcos, batch, c0, ones, inv_sigma, st['R'], rows=(cuts[j], cuts[j + 1]), O_blk=st['O_blk'][j], sums=st['sums'][j])
        st['O'] = st['O_blk'].sum(0)
        st['E'] = st['O'].sum(1)[:, None] * Pr[None, :]

    def a_round(hip):
        R, O_blk, sums, O, E = st['R'], st['O_blk'], st['sums'], st['O'], st['E']
        S = cluster.harmony_moments(Zcos, R, batch, B)[0] if hip else t_moments(Zcos, R)[0]
        st['cen64'] = centres(S, st['cen64'])
        cen = st['cen64'].to(torch.float32)
        for j in range(nb):
            a, b = cuts[j], cuts[j + 1]
            O = O - O_blk[j]
            E = E - O_blk[j].sum(1)[:, None] * Pr[None, :]
            Pm = torch.pow((E + 1.0) / (O + 1.0), theta[None, :]).to(torch.float32)
            if hip:
                cluster.harmony_assign(Zcos, batch, cen, Pm, inv_sigma, R, rows=(a, b), O_blk=O_blk[j], sums=sums[j])
            else:
                Oj, sd, se = t_assign(Zcos[a:b], batch64[a:b], blk_idx[j], cen, Pm, R[a:b])
                O_blk[j].copy_(Oj)
                sums[j, 0], sums[j, 1] = sd, se
            O = O + O_blk[j]
            E = E + O_blk[j].sum(1)[:, None] * Pr[None, :]
        st['O'], st['E'] = O, E
        return objective(sums, O, E)

    def t_run(rounds):
        reset()
        lam = torch.ones(B, dtype=f64, device=dev)
        for nr in rounds:
            for _ in range(nr):
                a_round(False)
            S, Om = t_moments(Z, st['R'])
            W = cluster.harmony_ridge_weights(S, Om, lam).to(torch.float32)
            t_correct(Z, st['R'], W)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return {'ms': float(np.median(ts)), 'ms_min_max': [min(ts), max(ts)]}

    def entry(name, hip, twin, flops, nbytes):
        h, t = timed(hip), timed(twin)
        r = {'what': name, 'hip': h, 'torch': t, 'torch_over_hip': t['ms'] / h['ms']}
        if flops:
            r['hip_f32_vector_share'] = flops / (h['ms'] * 1e-3) / (args.f32_tflops * 1e12)
            r['hip_hbm_share_of_least_bytes'] = nbytes / (h['ms'] * 1e-3) / (args.hbm_tbs * 1e12)
        return r

    reset()
    R = st['R']
    Rt = torch.empty_like(R)
    W = (0.1 * torch.randn(K, B, d, generator=g, device=dev)).contiguous()
    flops = 2.0 * n * K * d
    results = [
        entry('assign', lambda: cluster.harmony_assign(Zcos, batch, c0, P, inv_sigma, R), lambda: t_assign(Zcos, batch64, idx, c0, P, Rt),
              flops, 4.0 * n * (d + K + 1)),
        entry('moments', lambda: cluster.harmony_moments(Z, R, batch, B), lambda: t_moments(Z, R), flops, 4.0 * n * (d + K + 1)),
        entry('correct', lambda: cluster.harmony_correct(Z, R, batch, W), lambda: t_correct(Z, R, W), flops, 4.0 * n * (3 * d + K + 1)),
    ]
    # how far the twins are from the entries on the same inputs
    cluster.harmony_assign(Zcos, batch, c0, P, inv_sigma, R)
    t_assign(Zcos, batch64, idx, c0, P, Rt)
    agree = {'assign_R_max_abs_diff': float((R - Rt).abs().max())}
    Sh, Oh = cluster.harmony_moments(Z, R, batch, B)
    Stw, Otw = t_moments(Z, R)
    agree['moments_S_max_diff_over_max'] = float((Sh - Stw).abs().max() / Stw.abs().max())
    Zh, _ = cluster.harmony_correct(Z, R, batch, W)
    Ztw, _ = t_correct(Z, R, W)
    agree['correct_max_abs_diff'] = float((Zh - Ztw).abs().max())
    reset()
    results.append(entry('round of %d blocks' % nb, lambda: a_round(True), lambda: a_round(False), 2.0 * flops, 0.0))
    if not args.skip_run:
        out = cluster.harmony(Z, batch64, n_clusters=K, centers=c0)
        rounds = out['rounds']
        r = entry('full default run', lambda: cluster.harmony(Z, batch64, n_clusters=K, centers=c0), lambda: t_run(rounds), 0.0, 0.0)
        r.update(rounds=rounds, n_iter=out['n_iter'], converged=out['converged'])
        results.append(r)
    res = {'tool': 'harmony_timing', 'device': torch.cuda.get_device_name(0), 'n': n, 'd': d, 'K': K, 'B': B, 'blocks_per_round': nb,
           'warmup': args.warmup, 'reps': args.reps, 'hbm_peak_tbs': args.hbm_tbs, 'f32_vector_peak_tflops': args.f32_tflops,
           'timer': 'device events around each call', 'agreement': agree, 'results': results}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
