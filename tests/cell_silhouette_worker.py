# -*- coding: utf-8 -*-
"""One rank of the row-sharded cell_silhouette() run of tests/test_silhouette_gpu.py (a fresh process per rank; gloo between
the ranks, which share cuda:0).  Usage: cell_silhouette_worker.py RANK WORLD PORT OUT_PREFIX"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np                       # noqa: E402
import torch                             # noqa: E402
import torch.distributed as dist         # noqa: E402

from test_cluster_cells_gpu import build_model, N_CELLS     # noqa: E402


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from oriana_amd import dist as odist
        r0, r1 = odist.shard_rows(N_CELLS, rank, world)
        model = build_model('GaP', r0, r1, pg=dist.group.WORLD)
        labels = model.cluster_cells(3, n_init=2, seed=0)['labels']
        res = model.cell_silhouette(labels)
        chunked = model.cell_silhouette(labels, candidate_chunk=50, query_block=64, blocks=2)
        keys = ('values', 'a', 'b', 'mean', 'cluster_means', 'counts')
        np.savez(out + '.rank%d.npz' % rank, labels=labels, features=res['features'], row0=r0,
                 **{k: np.asarray(res[k]) for k in keys}, **{'chunked_' + k: np.asarray(chunked[k]) for k in keys})
        dist.barrier()
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(0)          # (as tests/test_sharded_gpu.py: no static destructors with a HIP context and gloo threads alive)


if __name__ == '__main__':
    main()
