# -*- coding: utf-8 -*-
"""Milliseconds of the diffusion-map functions of cluster.py (csrc/diffusion.hip) against the same steps written in float64
torch, in one process on the same tensors: a REPORT, no threshold.

Workload: seeded Gaussian blobs drawn as tools/community_timing.py draws them (`--n` x `--d` float32, `--blobs` centres
N(0, `--centre-scale`^2), noise N(0, 1)) -- but OVERLAPPING (0.25, not 3): blobs that far apart give one component each, and a
diffusion map is defined on a connected graph (the component count is reported; with more than one the map is left out); the
neighbour lists are cluster.knn(Y, `--k`), the graph is cluster.diffusion_graph(indices, sq_distances).

    diffusion_graph      one cluster.diffusion_graph call: the pattern and the elementwise steps by torch, the two row sums
    spmv                 one oriana_csr_spmv_f64 call, y = T x
    orth_j100 / j500     one oriana_basis_orthogonalize_f64 call (two passes) against j orthonormal columns
    diffusion_map        one cluster.diffusion_map run (its step count is reported), host checks included
    torch_spmv           torch.sparse CSR mv of the same matrix
    torch_orth_j100 / j500   THE SAME TWO PASSES BY TORCH: c = Q w, w -= Q^T c, h += c, twice, then w . w (rocBLAS gemv: the
                         order of its sums is its own)

Each is timed with device events around one call, after `--warmup` untimed calls, `--reps` times; the median is reported with the
minimum and maximum.  Beside them: the bytes a call must move (spmv: 20 per stored entry -- column, value and the gathered x --
and 16 per row; orthogonalize: 32 n j for the four walks over Q and 48 n for w) over `--hbm-rate` as a floor.  Prints one JSON
line; `--out` also writes it to a file.

    python tools/diffusion_timing.py --out profiles/diffusion_timing.json
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
    ap.add_argument('--centre-scale', type=float, default=0.25)
    ap.add_argument('--k', type=int, default=15)
    ap.add_argument('--n-comps', type=int, default=15)
    ap.add_argument('--tol', type=float, default=1e-8)
    ap.add_argument('--max-steps', type=int, default=None)
    ap.add_argument('--js', type=int, nargs='+', default=[100, 500])
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--hbm-rate', type=float, default=6.29e12)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('diffusion_timing needs a GPU: there is nothing to time without one')
    from oriana_amd import cluster
    dev = torch.device('cuda', 0)
    n, d = args.n, args.d
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    mu = args.centre_scale * torch.randn(args.blobs, d, generator=gen, device=dev)
    which = torch.randint(0, args.blobs, (n,), generator=gen, device=dev)
    Y = mu[which]
    Y += torch.randn(n, d, generator=gen, device=dev)
    nb = cluster.knn(Y, args.k)
    idx, d2 = nb['indices'], nb['sq_distances']
    del Y
    g = cluster.diffusion_graph(idx, d2)
    crow, col, T = g['crow'], g['col'], g['weight']
    nnz = int(col.numel())
    lens = crow[1:] - crow[:-1]
    comps = cluster.graph_components(g)['n_components']
    x = torch.randn(n, dtype=torch.float64, generator=gen, device=dev)
    y = torch.empty(n, dtype=torch.float64, device=dev)
    A = torch.sparse_csr_tensor(crow, col.to(torch.int64), T, size=(n, n))
    ld = n + (n & 1)
    jmax = max(args.js)
    # an orthonormal basis: the Q factor of a seeded matrix (unit random columns where the QR is not available)
    Q = torch.zeros(jmax + 1, ld, dtype=torch.float64, device=dev)
    R = torch.randn(n, jmax, dtype=torch.float64, generator=gen, device=dev)
    try:
        Q[:jmax, :n] = torch.linalg.qr(R).Q.t()
        basis = 'Q factor of a seeded matrix'
    except RuntimeError:
        Q[:jmax, :n] = (R / R.norm(dim=0)).t()
        basis = 'seeded columns of unit norm (not orthogonal)'
    del R
    b2 = torch.zeros(1, dtype=torch.float64, device=dev)
    scratch = torch.empty(cluster._scratch_bytes('oriana_basis_orthogonalize_scratch_bytes_for', n, jmax), dtype=torch.uint8, device=dev)
    w0 = torch.randn(n, dtype=torch.float64, generator=gen, device=dev)
    w = torch.empty(n, dtype=torch.float64, device=dev)
    h = torch.zeros(jmax, dtype=torch.float64, device=dev)

    def hip_orth(j):
        w.copy_(w0)
        h.zero_()
        cluster.basis_orthogonalize(Q, n, j, w, h, b2, passes=2, scratch=scratch)
        return w, h[:j], b2

    def torch_orth(j):
        Qj = Q[:j, :n]
        wt = w0.clone()
        ht = torch.zeros(j, dtype=torch.float64, device=dev)
        for _ in range(2):
            c = Qj @ wt
            wt -= Qj.t() @ c
            ht += c
        return wt, ht, (wt @ wt).reshape(1)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    agree = {}
    ys = cluster.csr_spmv(crow, col, T, x).clone()
    agree['spmv_max_abs_diff'] = float((ys - A @ x).abs().max())
    for j in args.js:
        hw, hh, hb = (t.clone() for t in hip_orth(j))
        tw, th, tb = torch_orth(j)
        agree['orth_j%d' % j] = {'w_max_abs_diff': float((hw - tw).abs().max()), 'h_max_abs_diff': float((hh - th).abs().max()),
                                 'beta2_rel_diff': float(((hb - tb) / tb).abs().max()),
                                 'hip_max_abs_QTw': float((Q[:j, :n] @ hw).abs().max()), 'torch_max_abs_QTw': float((Q[:j, :n] @ tw).abs().max())}
    map_kw = dict(n_comps=args.n_comps, tol=args.tol, max_steps=args.max_steps)
    run = cluster.diffusion_map(g, **map_kw) if comps == 1 else None
    if run is not None:
        sys.stderr.write('diffusion_map: %d steps, converged %s\n' % (run['steps'], run['converged']))

    sides = [('diffusion_graph', lambda: cluster.diffusion_graph(idx, d2)), ('spmv', lambda: cluster.csr_spmv(crow, col, T, x, out=y)),
             ('torch_spmv', lambda: A @ x)]
    for j in args.js:
        sides += [('orth_j%d' % j, lambda j=j: hip_orth(j)), ('torch_orth_j%d' % j, lambda j=j: torch_orth(j))]
    # (what the orthogonalisation sides share and the kernel does not need: the copy of w0 and the zeroing of h)
    sides.append(('orth_setup', lambda: (w.copy_(w0), h.zero_())))
    if run is not None:
        sides.append(('diffusion_map', lambda: cluster.diffusion_map(g, **map_kw)))
    times = {}
    for name, fn in sides:
        for _ in range(args.warmup):
            timed(fn)
        times[name] = [timed(fn) for _ in range(args.reps)]
        sys.stderr.write('%s: %s ms\n' % (name, ', '.join('%.3f' % t for t in times[name])))
        sys.stderr.flush()
    med = {name: float(np.median(t)) for name, t in times.items()}
    spmv_bytes = 20 * nnz + 16 * n
    floors = {'spmv': spmv_bytes / args.hbm_rate * 1e3}
    over = {'spmv': med['spmv'] / floors['spmv']}
    for j in args.js:
        floors['orth_j%d' % j] = (32 * n * j + 48 * n) / args.hbm_rate * 1e3
        over['orth_j%d' % j] = (med['orth_j%d' % j] - med['orth_setup']) / floors['orth_j%d' % j]
    out = {'tool': 'diffusion_timing', 'device': torch.cuda.get_device_name(0), 'n': n, 'd': d, 'blobs': args.blobs, 'centre_scale': args.centre_scale, 'k': args.k,
           'stored_entries': nnz, 'longest_row': int(lens.max()), 'components': comps, 'basis_tile_rows': cluster.basis_tile_rows(), 'basis': basis,
           'warmup_calls': args.warmup, 'reps': args.reps, 'timer': 'device events around one call', 'ms': med,
           'ms_min_max': {name: [min(t), max(t)] for name, t in times.items()},
           'agreement_with_torch': agree, 'hbm_rate': args.hbm_rate, 'spmv_bytes': spmv_bytes,
           'orth_bytes': {'j%d' % j: 32 * n * j + 48 * n for j in args.js}, 'floor_ms': floors,
           'median_over_floor (orth: less orth_setup)': over,
           'torch_min_over_hip_median': dict([('spmv', min(times['torch_spmv']) / med['spmv'])] +
                                             [('orth_j%d' % j, min(times['torch_orth_j%d' % j]) / med['orth_j%d' % j]) for j in args.js])}
    if run is not None:
        out['diffusion_map'] = {'n_comps': args.n_comps, 'tol': args.tol, 'steps': run['steps'], 'converged': run['converged'],
                                'eigenvalues': [float(v) for v in run['eigenvalues']], 'max_residual_estimate': float(run['residuals'].max()),
                                'ms_per_step': med['diffusion_map'] / run['steps']}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
