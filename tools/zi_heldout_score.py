# -*- coding: utf-8 -*-
"""Mean held-out score per cell of ZI-pCMF fits (ZIGaP.fold_in_score) and of pCMF fits (GaP.score) on the same held-out cells of
planted rank-3 zero-inflated counts, for k = 1, 2, 3, 5, 8: a report, nothing is asserted.

293 training and 150 held-out cells over 131 genes: Gamma(1) factors of rank 3, Poisson counts, each gene kept with a probability of
its own drawn from U(0.5, 0.95); fits of `--sweeps` sweeps from Gamma(1) starts.  Prints one JSON line.

    python tools/zi_heldout_score.py --out profiles/zi_heldout_score.json
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
    ap.add_argument('--sweeps', type=int, default=40)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('zi_heldout_score needs a GPU')
    from oriana_amd.models import GaP, ZIGaP
    n, nq, m, rank = 293, 150, 131, 3
    rng = np.random.default_rng(args.seed)
    Vt = rng.gamma(1.0, 1.0, (m, rank))
    pi_true = rng.uniform(0.5, 0.95, m)

    def draw(rows):
        U = rng.gamma(1.0, 1.0, (rows, rank))
        return (rng.poisson(U @ Vt.T) * (rng.random((rows, m)) < pi_true)).astype(np.float64)
    X, Xq = draw(n), draw(nq)
    rows = []
    for k in (1, 2, 3, 5, 8):
        r = np.random.default_rng(10 + k)
        init = (r.gamma(1.0, 1.0, (n, k)), r.gamma(1.0, 1.0, (m, k)))
        Z = ZIGaP(X, k=k, init=init).fit(args.sweeps)
        zi = Z.fold_in_score(Xq)
        G = GaP(X, k=k, init=init).fit(args.sweeps)
        pc = G.score(Xq)
        rows.append({'k': k, 'zi_mean_score': zi, 'zi_unconverged': Z.fold_in_unconverged_, 'pcmf_mean_score': pc,
                     'pcmf_unconverged': G.transform_unconverged_})
    out = {'device': torch.cuda.get_device_name(0), 'train_cells': n, 'held_out_cells': nq, 'genes': m, 'planted_rank': rank,
           'sweeps': args.sweeps, 'seed': args.seed, 'zeros_share': float((X == 0).mean()), 'fits': rows}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
