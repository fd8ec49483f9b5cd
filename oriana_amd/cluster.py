# -*- coding: utf-8 -*-
"""k-means on the device: all restarts of a run advance together through oriana_kmeans_step (csrc/kmeans.hip), which reads a row
tile once for a group of restarts and emits only per-cluster sums.  The reference's pipeline ends in
``KMeans(n_clusters, n_init=100).fit(np.log(U))`` (experiments/clustering.py); this is that step without the host copy.
DESIGN.md section 5i.

knn() is the exact k-nearest-neighbour graph of the same rows through oriana_knn (csrc/knn.hip): brute force, no distance
matrix, results independent of every partition of the work.  DESIGN.md section 5j.

silhouette() is the exact silhouette of a labelling of the same rows through oriana_cluster_distance_sums (csrc/silhouette.hip):
all Euclidean distances of all pairs, added per cluster in float64, no distance matrix; adjusted_rand() is the exact adjusted
Rand index of two labellings.  DESIGN.md section 5k.

tsne() is the exact t-SNE layout of the same rows (csrc/tsne.hip): the neighbour graph of knn(), perplexity-calibrated affinities,
and a gradient whose repulsive term is all n^2 pairs by brute force -- no tree, no sampling, deterministic.  DESIGN.md section 5m.

louvain() is a deterministic Louvain clustering of the graph snn_graph() forms from the neighbour lists of knn()
(csrc/community.hip): integer weights, every node of a sweep decides from the old state, so a labelling is a function of the
graph alone and a NumPy restatement matches it label for label.  DESIGN.md section 5o.

diffusion_map() is the diffusion map of the same neighbour graph (csrc/diffusion.hip): the Gaussian affinities of
diffusion_graph(), and Lanczos with full reorthogonalisation whose sums over rows run in a fixed order, so the eigenpairs are a
function of the graph and the start vector alone; diffusion_pseudotime() orders the cells from a root.  DESIGN.md section 5p.

harmony() is Harmony batch correction of the same rows (csrc/harmony.hip): soft k-means under a batch-diversity penalty, then a
per-cluster ridge correction in closed form; one permutation per run and a fixed block order make a run a function of its
arguments, and a NumPy restatement follows it step for step.  DESIGN.md section 5r."""
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from . import dist as odist

__all__ = ['kmeans', 'lloyd_step', 'max_centers', 'restart_group', 'partial_rows', 'tile_rows', 'draws', 'distinct_rows',
           'knn', 'knn_plan', 'knn_step', 'max_neighbors',
           'silhouette', 'silhouette_plan', 'silhouette_from_sums', 'distance_sums', 'max_clusters', 'adjusted_rand',
           'tsne', 'tsne_plan', 'tsne_default_neighbors', 'tsne_affinities', 'tsne_joint', 'tsne_attract', 'tsne_repulse',
           'tsne_gradient', 'tsne_pca_init',
           'snn_graph', 'louvain', 'louvain_sweep', 'louvain_plan', 'louvain_row_cap', 'modularity',
           'diffusion_graph', 'diffusion_map', 'diffusion_pseudotime', 'graph_components', 'csr_spmv', 'basis_tile_rows',
           'basis_orthogonalize', 'basis_append', 'basis_combine',
           'harmony', 'harmony_assign', 'harmony_moments', 'harmony_correct', 'harmony_max_clusters', 'harmony_max_batches',
           'harmony_partial_rows', 'harmony_default_clusters', 'harmony_block_cuts', 'harmony_ridge_weights']

SCRATCH_BUDGET = 1 << 30          # bytes a launch may take for scratch, minimum distances and their cumulative sums


# ---- what kmeans(), knn(), silhouette() and tsne() share on the host -----------------------------------------------------------
def _scratch_bytes(entry, *args):
    """Bytes of scratch of one call, from the library's `entry` (a *_scratch_bytes* function of the call's sizes)."""
    nbytes = int(getattr(_lib.load(), entry)(*args))
    if nbytes < 0:
        raise _lib.OrianaHipError('%s failed with code %d' % (entry, nbytes))
    return nbytes


def _scratch_for(scratch, nbytes, device):
    """The caller's scratch, refused where it holds fewer than nbytes (the entries take no size: they would write past it), or
    a new one."""
    if scratch is None:
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    if scratch.numel() * scratch.element_size() < nbytes:
        raise ValueError('the scratch holds %d bytes, this call needs %d' % (scratch.numel() * scratch.element_size(), nbytes))
    return scratch


def _check_cuts(blocks, candidate_chunk, query_block):
    if int(blocks) < 0 or any(v is not None and int(v) < 1 for v in (candidate_chunk, query_block)):
        raise ValueError('blocks >= 0, candidate_chunk >= 1 and query_block >= 1 are required')


def _block_sizes(total, block):
    """The sizes that occur when `total` rows are cut into blocks of `block`: the full block and the shorter last one."""
    return {min(block, total)} | ({total % block} if total > block else set())


def _plan(nq, n, candidate_chunk, query_block, budget, scratch, need=None, chunk_need=None):
    """The planning of knn_plan(), silhouette_plan() and tsne_plan(): (query_block, candidate_chunk, scratch(query_block,
    candidate_chunk)).  What the caller left open starts at everything in one call; then the candidates are halved while
    chunk_need(chunk, tile) exceeds half the budget (never without a chunk_need), then the queries, in whole tiles of the
    kernels, while need(query_block, chunk) (default: the scratch) exceeds the budget."""
    budget = SCRATCH_BUDGET if budget is None else int(budget)
    tile = int(_lib.load().oriana_knn_tile_rows())
    need = scratch if need is None else need
    chunk = int(candidate_chunk) if candidate_chunk is not None else max(n, 1)
    qb = int(query_block) if query_block is not None else max(nq, 1)
    if candidate_chunk is None and chunk_need is not None:
        while chunk > 1 and chunk_need(chunk, tile) > budget // 2:
            chunk = (chunk + 1) // 2
    if query_block is None:
        while qb > tile and need(qb, chunk) > budget:
            qb = max(tile, -(-qb // (2 * tile)) * tile)
    return qb, chunk, scratch(qb, chunk)


def _finite_flag(*tensors):
    """(1,) float64 on the tensors' device: 1 where every entry of every tensor is finite, else 0."""
    ok = torch.isfinite(tensors[0]).all()
    for t in tensors[1:]:
        ok = ok & torch.isfinite(t).all()
    return ok.to(torch.float64).reshape(1)


def _all_finite(pg, *tensors):
    """Whether the tensors are finite on every rank (one all-reduced flag under sharding)."""
    finite = _finite_flag(*tensors)
    if odist.sharded(pg):
        finite = 1.0 - finite
        odist.all_reduce_sum(finite, pg)
        finite = 1.0 - finite.clamp(max=1.0)
    return bool(finite.item())


def max_centers(d):
    """The largest number of clusters served at feature width d (0: d is not served)."""
    return int(_lib.load().oriana_kmeans_max_centers(int(d)))


def restart_group(d, C):
    """Restarts that share one read of a row tile at (d, C)."""
    return int(_lib.load().oriana_kmeans_group(int(d), int(C)))


def partial_rows():
    return int(_lib.load().oriana_kmeans_partial_rows())


def tile_rows():
    return int(_lib.load().oriana_kmeans_tile_rows())


def lloyd_step(Y, centers, label_restart=None, want_mind=False, blocks=0):
    """One oriana_kmeans_step: Y (n, d) float32 device tensor (row stride >= d, unit column stride), centers (R, C, d) float32.
    Returns a dict of device tensors: 'sums' (R, C, d) float64, 'counts' (R, C) int64, 'inertia' (R,) float64, and on request
    'labels' (n,) int32 of restart `label_restart` and 'mind' (R, n) float32."""
    n, d = int(Y.shape[0]), int(Y.shape[1])
    R, C = int(centers.shape[0]), int(centers.shape[1])
    dev = Y.device
    if Y.dtype != torch.float32 or centers.dtype != torch.float32 or not centers.is_contiguous() or int(centers.shape[2]) != d:
        raise ValueError('lloyd_step needs float32 Y (n, d) and contiguous float32 centers (R, C, d)')
    if Y.stride(1) != 1 and n > 1:
        raise ValueError('the columns of Y must be contiguous')
    ldy = int(Y.stride(0)) if n > 1 else d
    nbytes = _scratch_bytes('oriana_kmeans_scratch_bytes', n, d, C, R, int(blocks))
    out = {'sums': torch.empty(R, C, d, dtype=torch.float64, device=dev),
           'counts': torch.empty(R, C, dtype=torch.int64, device=dev),
           'inertia': torch.empty(R, dtype=torch.float64, device=dev)}
    labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if label_restart is not None else None
    mind = torch.empty(R, max(n, 1), dtype=torch.float32, device=dev) if want_mind else None
    scratch = _scratch_for(None, nbytes, dev)
    call('oriana_kmeans_step', ptr(Y) if n else None, n, d, ldy, ptr(centers), C, R, ptr(out['sums']), ptr(out['counts']),
         ptr(out['inertia']), ptr(labels), int(label_restart or 0), ptr(mind), ptr(scratch), int(blocks), stream_ptr())
    if labels is not None:
        out['labels'] = labels[:n]
    if mind is not None:
        out['mind'] = mind[:, :n]
    return out


def draws(seed, n_init, C):
    """The uniform draws of a run: an (n_init, C) float64 CPU tensor from torch.Generator().manual_seed(seed)."""
    g = torch.Generator()
    g.manual_seed(int(seed))
    return torch.rand(int(n_init), int(C), dtype=torch.float64, generator=g)


def distinct_rows(u, n):
    """C distinct indices in [0, n) from C uniform draws (Floyd's sampling: every C-subset is equally likely)."""
    C = len(u)
    chosen, out = set(), []
    for j in range(C):
        top = n - C + j
        t = min(int(u[j] * (top + 1)), top)
        if t in chosen:
            t = top
        chosen.add(t)
        out.append(t)
    return out


def _reduced_step(Y, c32, pg, **kw):
    """lloyd_step with sums, counts and inertia summed over the row shards in one packed all-reduce."""
    o = lloyd_step(Y, c32, **kw)
    if odist.sharded(pg):
        R, C, d = c32.shape
        packed = torch.cat([o['sums'].reshape(-1), o['counts'].to(torch.float64).reshape(-1), o['inertia']])
        odist.all_reduce_sum(packed, pg)
        o['sums'] = packed[:R * C * d].view(R, C, d)
        o['counts'] = packed[R * C * d:R * C * d + R * C].view(R, C).to(torch.int64)     # (exact: counts stay below 2^53)
        o['inertia'] = packed[R * C * d + R * C:]
    return o


class _Rows:
    """Where this rank's rows sit among all rows, and the gather of rows by global index through an all-reduce."""

    def __init__(self, Y, pg):
        self.Y, self.pg = Y, pg
        self.n = int(Y.shape[0])
        self.world, self.rank = odist.world_size(pg), odist.rank(pg)
        if odist.sharded(pg):
            t = torch.zeros(self.world, dtype=torch.int64, device=Y.device)
            t[self.rank] = self.n
            odist.all_reduce_sum(t, pg)
            sizes = t.cpu().numpy()
            self.row0 = int(sizes[:self.rank].sum())
            self.N = int(sizes.sum())
            self.sizes = [int(v) for v in sizes]
        else:
            self.row0, self.N = 0, self.n
            self.sizes = [self.n]

    def gather(self, g):
        """The rows with global indices g (int64 device tensor, any shape) as float32 (.., d): a zero buffer to which the
        owning rank adds its row, summed over the ranks."""
        li = g - self.row0
        mine = (li >= 0) & (li < self.n)
        buf = torch.zeros(tuple(g.shape) + (int(self.Y.shape[1]),), dtype=torch.float32, device=self.Y.device)
        if self.n:
            buf[mine] = self.Y[li[mine]]
        return odist.all_reduce_sum(buf, self.pg)

    def shards(self, labels=None):
        """All rows as candidates, shard after shard in rank order: yields (first global row, rows) or, with this rank's
        `labels` (int64), (first global row, rows, labels).  Under sharding shard s is made available on every rank: zero
        buffers to which its owner adds its rows (and labels), summed over the ranks (exact); else Y as it lies."""
        mine = (self.Y,) if labels is None else (self.Y, labels)
        row0 = 0
        for s, ns in enumerate(self.sizes):
            shard = mine
            if odist.sharded(self.pg):
                shard = tuple(torch.zeros((ns,) + tuple(t.shape[1:]), dtype=t.dtype, device=self.Y.device) for t in mine)
                for buf, t in zip(shard, mine):
                    if s == self.rank and ns:
                        buf.copy_(t)
                    odist.all_reduce_sum(buf, self.pg)
            yield (row0,) + shard
            row0 += ns


def _kmeanspp(rows, u, C, pg):
    """Plain single-trial k-means++ for the restarts of `u` (R, C) float64 device draws: (R, C, d) float32 centres, rows of Y."""
    Y, dev = rows.Y, rows.Y.device
    R, n, N, W, rank = int(u.shape[0]), rows.n, rows.N, rows.world, rows.rank
    first = torch.clamp((u * N).floor().to(torch.int64), max=N - 1)          # the pick where there are no weights
    cen = torch.zeros(R, C, int(Y.shape[1]), dtype=torch.float32, device=dev)
    cen[:, 0] = rows.gather(first[:, 0])
    for j in range(1, C):
        mind = lloyd_step(Y, cen[:, :j].contiguous(), want_mind=True)['mind']
        cum = torch.cumsum(mind.to(torch.float64), dim=1)                      # (R, n)
        tot = torch.zeros(R, W, dtype=torch.float64, device=dev)
        if n:
            tot[:, rank] = cum[:, -1]
        odist.all_reduce_sum(tot, pg)
        rank_cum = torch.cumsum(tot, dim=1)
        total = rank_cum[:, -1]
        target = u[:, j] * total
        # the owner is decided from the all-reduced totals alone: every rank sees the same one
        owner = torch.searchsorted(rank_cum, target[:, None], right=True).squeeze(1)
        has = (tot > 0).to(torch.int64) * torch.arange(1, W + 1, device=dev)
        owner = torch.where(owner < W, owner, has.max(dim=1).values - 1)    # (u * total rounded up to total: the last weight)
        g = first[:, j].clone()                                                # (total == 0: as the first centre)
        if n:
            offset = rank_cum[:, rank] - tot[:, rank]
            idx = torch.searchsorted(cum, (target - offset)[:, None], right=True).squeeze(1)
            pos = (mind > 0).to(torch.int64) * torch.arange(1, n + 1, device=dev)
            idx = torch.where(idx < n, idx, pos.max(dim=1).values - 1)
            sel = (owner == rank) & (total > 0)
            g = torch.where(sel, idx + rows.row0, torch.where(total > 0, torch.full_like(g, -1), g))
        else:
            g = torch.where(total > 0, torch.full_like(g, -1), g)
        cen[:, j] = rows.gather(g)
    return cen


def _variance(Y, rows, pg):
    """mean_k Var(Y[:, k]) over all rows, float64 (scikit-learn's tolerance scale)."""
    d = int(Y.shape[1])
    s = Y.sum(0, dtype=torch.float64)
    odist.all_reduce_sum(s, pg)
    mean = s / rows.N
    q = torch.zeros(d, dtype=torch.float64, device=Y.device)
    for a in range(0, rows.n, 1 << 18):
        q += ((Y[a:a + (1 << 18)].to(torch.float64) - mean) ** 2).sum(0)
    odist.all_reduce_sum(q, pg)
    return float((q / rows.N).mean())


def _lloyd(Y, c0, max_iter, thr, check_every, pg):
    """Lloyd's iteration for the restarts of c0 (R, C, d) float64, all advancing together; converged restarts are compacted out
    of the batch whenever the host reads the flags.  Returns centres (R, C, d) float64, n_iter (R,) int64, converged (R,) bool."""
    R = int(c0.shape[0])
    dev = Y.device
    centers = c0.clone()
    n_iter = torch.zeros(R, dtype=torch.int64, device=dev)
    conv = torch.zeros(R, dtype=torch.bool, device=dev)
    act = torch.arange(R, device=dev)
    cur, done, its = c0.clone(), conv.clone(), n_iter.clone()
    it = 0
    while it < max_iter and act.numel():
        o = _reduced_step(Y, cur.to(torch.float32), pg)
        cnt = o['counts']
        new = torch.where(cnt[:, :, None] > 0, o['sums'] / cnt.clamp(min=1)[:, :, None].to(torch.float64), cur)
        shift = ((new - cur) ** 2).sum(dim=(1, 2))
        run = ~done
        cur = torch.where(run[:, None, None], new, cur)
        its = its + run.to(torch.int64)
        done = done | (run & (shift <= thr))
        it += 1
        if it % check_every == 0 or it == max_iter:
            centers[act], n_iter[act], conv[act] = cur, its, done
            keep = ~done
            if not bool(keep.all()):                      # (the one host read)
                act, cur, its, done = act[keep], cur[keep], its[keep], done[keep]
    return centers, n_iter, conv


def _default_restarts_per_pass(n, d, C, n_init, plus):
    lib = _lib.load()
    R = n_init
    while R > 1:
        need = int(lib.oriana_kmeans_scratch_bytes(n, d, C, R, 0)) + R * C * d * 28
        if plus:
            need += R * n * 12 + R * n * 16               # minimum distances, their float64 cumulative sums, the ranks
        if need <= SCRATCH_BUDGET:
            break
        R = (R + 1) // 2
    return R


def kmeans(Y, n_clusters, n_init=10, max_iter=300, tol=1e-4, init='k-means++', seed=0, check_every=5, pg=None,
           restarts_per_pass=None):
    """k-means of the rows of Y, an (n, d) float32 C-contiguous device tensor (with `pg`: this rank's rows), by Lloyd's iteration
    from `n_init` starts that all advance together on the device.

    init : 'k-means++' (the plain single-trial algorithm, not scikit-learn's greedy variant), 'random' (n_clusters distinct rows
        per restart) or explicit centres (n_init, n_clusters, d) / (n_clusters, d) (one restart).  All random draws are
        ``draws(seed, n_init, n_clusters)``: the first k-means++ centre is row floor(u * n), each later one the first row whose
        float64 cumulative minimum squared distance exceeds u * total.
    tol : restart r has converged when sum |new - old|^2 <= tol * mean_k Var(Y[:, k]) (scikit-learn's rule), evaluated on the
        device; the host reads the flags every `check_every` iterations and drops the converged restarts from the batch.
    restarts_per_pass : restarts per launch (default: from a scratch budget); beyond it the restarts run in chunks.

    New centres are sums / counts in float64, cast to float32 for the next step.  A cluster that loses all its rows KEEPS ITS
    PREVIOUS CENTRE -- the one deliberate difference from scikit-learn, which relocates it.  After the loop one more step with the
    final centres gives consistent labels and inertia; the restart with the smallest inertia wins (the lowest index on a tie).

    Returns a dict: 'labels' (n,) int32 NumPy (the caller's row order; this rank's rows), 'centers' (C, d) float64, 'inertia',
    'n_iter', 'best' of the chosen restart, and per restart 'inertias', 'converged', 'n_iters', 'all_centers' (n_init, C, d),
    'init_centers' (n_init, C, d) float64.  Under row sharding every rank returns the same centres and inertias.
    ValueError before any launch for arguments out of range, a Y that is not float32 / contiguous / finite, an init of the wrong
    shape, or n_clusters beyond max_centers(d)."""
    if not isinstance(Y, torch.Tensor) or Y.dim() != 2:
        raise ValueError('Y must be a 2-D torch tensor')
    if Y.dtype != torch.float32:
        raise ValueError('Y must be float32, got %s' % Y.dtype)
    if not Y.is_contiguous():
        raise ValueError('Y must be C-contiguous')
    C, n_init, max_iter, tol, check_every = int(n_clusters), int(n_init), int(max_iter), float(tol), int(check_every)
    n, d = int(Y.shape[0]), int(Y.shape[1])
    if C < 1:
        raise ValueError('n_clusters must be at least 1')
    if n_init < 1 or max_iter < 0 or not tol >= 0 or check_every < 1:
        raise ValueError('n_init >= 1, max_iter >= 0, tol >= 0 and check_every >= 1 are required')
    if restarts_per_pass is not None and int(restarts_per_pass) < 1:
        raise ValueError('restarts_per_pass must be at least 1')
    if d < 1:
        raise ValueError('Y needs at least one column')
    explicit = None
    if not isinstance(init, str):
        explicit = torch.as_tensor(np.asarray(init.detach().cpu() if isinstance(init, torch.Tensor) else init, dtype=np.float64))
        if explicit.dim() == 2:
            explicit = explicit[None]
            n_init = 1
        if tuple(explicit.shape) != (n_init, C, d):
            raise ValueError('init must be (n_init, n_clusters, d) = %s or (n_clusters, d), got %s'
                             % ((n_init, C, d), tuple(explicit.shape)))
    elif init not in ('k-means++', 'random'):
        raise ValueError("init must be 'k-means++', 'random' or an array of centres")
    cmax = max_centers(d)
    if C > cmax:
        raise ValueError('n_clusters = %d is beyond the %d served at %d features' % (C, cmax, d))
    if not odist.sharded(pg) and C > n:
        raise ValueError('n_clusters = %d exceeds the %d rows' % (C, n))
    if not Y.is_cuda:
        raise ValueError('Y must be a device tensor')
    rows = _Rows(Y, pg)
    if C > rows.N:
        raise ValueError('n_clusters = %d exceeds the %d rows' % (C, rows.N))
    if not _all_finite(pg, Y):
        raise ValueError('Y has non-finite entries')

    dev = Y.device
    rpp = int(restarts_per_pass) if restarts_per_pass is not None else _default_restarts_per_pass(n, d, C, n_init, explicit is None and init == 'k-means++')
    thr = tol * _variance(Y, rows, pg)
    u = draws(seed, n_init, C)
    init_c = torch.empty(n_init, C, d, dtype=torch.float64, device=dev)
    all_c = torch.empty_like(init_c)
    n_iters = torch.empty(n_init, dtype=torch.int64, device=dev)
    conv = torch.empty(n_init, dtype=torch.bool, device=dev)
    inertias = torch.empty(n_init, dtype=torch.float64, device=dev)
    for a in range(0, n_init, rpp):
        b = min(a + rpp, n_init)
        if explicit is not None:
            c0 = explicit[a:b].to(dev)
        elif init == 'random':
            g = torch.as_tensor([distinct_rows(u[r].tolist(), rows.N) for r in range(a, b)], dtype=torch.int64, device=dev)
            c0 = rows.gather(g).to(torch.float64)
        else:
            c0 = _kmeanspp(rows, u[a:b].to(dev), C, pg).to(torch.float64)
        init_c[a:b] = c0
        all_c[a:b], n_iters[a:b], conv[a:b] = _lloyd(Y, c0, max_iter, thr, check_every, pg)
        inertias[a:b] = _reduced_step(Y, all_c[a:b].to(torch.float32), pg)['inertia']
    inertias_h = inertias.cpu().numpy()
    best = int(np.argmin(inertias_h))                   # (the first minimum: the lowest index wins a tie)
    labels = lloyd_step(Y, all_c[best:best + 1].to(torch.float32), label_restart=0)['labels']
    n_iters_h = n_iters.cpu().numpy()
    return {'labels': labels.cpu().numpy(), 'centers': all_c[best].cpu().numpy(), 'inertia': float(inertias_h[best]),
            'n_iter': int(n_iters_h[best]), 'inertias': inertias_h, 'converged': conv.cpu().numpy(), 'best': best,
            'n_iters': n_iters_h, 'all_centers': all_c.cpu().numpy(), 'init_centers': init_c.cpu().numpy()}


# ---- exact k nearest neighbours (csrc/knn.hip) ----------------------------------------------------------------
def max_neighbors(d):
    """The largest n_neighbors served at feature width d (0: d is not served)."""
    return int(_lib.load().oriana_knn_max_neighbors(int(d)))


def _rows_ld(T):
    """(rows, row stride) of a 2-D float32 tensor with unit column stride, as the kernels take it."""
    n, d = int(T.shape[0]), int(T.shape[1])
    return n, (int(T.stride(0)) if n > 1 else d)


def _knn_scratch_bytes(nq, n, d, k, blocks, y_ptr, ldy):
    """Bytes of scratch of one oriana_knn call whose candidates start at y_ptr with row stride ldy."""
    return _scratch_bytes('oriana_knn_scratch_bytes_for', nq, n, d, k, int(blocks), y_ptr, ldy)


def knn_plan(nq, n, d, k, blocks=0, y_ptr=16, ldy=None, candidate_chunk=None, query_block=None, budget=None):
    """How knn() cuts nq queries against n candidates (of its largest shard) into oriana_knn calls: (query_block,
    candidate_chunk, scratch bytes that serve every call issued).  Needs no device.  The scratch of a call is NOT monotone in its
    queries (fewer query tiles are cut into more candidate ranges, each with partial lists of its own), so the bytes are the
    largest need over the block sizes that occur: the full block and the shorter last one.  What is not given is chosen so that the scratch stays
    within `budget` (default SCRATCH_BUDGET): first the candidates are halved until a padded image of a chunk (needed only where
    Y does not serve as the image: y_ptr, ldy) takes at most half the budget, then the queries -- whose partial lists and copy
    of the incoming rows are the part of the scratch that no candidate chunk shrinks -- are halved, in whole tiles, until the
    call fits.  Either split leaves the result unchanged bit for bit."""
    nq, n, d, k = int(nq), int(n), int(d), int(k)
    ldy = d if ldy is None else int(ldy)

    def scratch(qb, c):
        return max(_knn_scratch_bytes(b, min(c, n), d, k, blocks, y_ptr, ldy) for b in _block_sizes(nq, qb))

    return _plan(nq, n, candidate_chunk, query_block, budget, scratch, chunk_need=lambda c, tile: scratch(tile, c))


def knn_step(Q, Y, idx, d2, q0=0, y0=0, exclude_self=False, merge=False, blocks=0, scratch=None):
    """One oriana_knn call: the rows of Q (nq, d) against the candidates Y (n, d), both float32 device tensors (row stride >= d,
    unit column stride) whose first rows have the global indices q0 and y0; idx (nq, k) int32 and d2 (nq, k) float32, contiguous,
    are written, or with `merge` merged with what they hold."""
    nq, ldq = _rows_ld(Q)
    n, ldy = _rows_ld(Y)
    d, k = int(Q.shape[1]), int(idx.shape[1])
    scratch = _scratch_for(scratch, _knn_scratch_bytes(nq, n, d, k, blocks, ptr(Y) if n else None, ldy), idx.device)
    call('oriana_knn', ptr(Q) if nq else None, nq, ldq, int(q0), ptr(Y) if n else None, n, ldy, int(y0), d, k,
         1 if exclude_self else 0, 1 if merge else 0, ptr(idx), ptr(d2), ptr(scratch), int(blocks), stream_ptr())


def _check_rows(T, what):
    if not isinstance(T, torch.Tensor) or T.dim() != 2:
        raise ValueError('%s must be a 2-D torch tensor' % what)
    if T.dtype != torch.float32:
        raise ValueError('%s must be float32, got %s' % (what, T.dtype))
    if T.shape[0] > 1 and T.shape[1] > 0 and (T.stride(1) != 1 or T.stride(0) < T.shape[1]):
        raise ValueError('the columns of %s must be contiguous and its rows must not overlap' % what)
    if T.shape[0] == 1 and T.shape[1] > 1 and T.stride(1) != 1:
        raise ValueError('the columns of %s must be contiguous' % what)


def knn(Y, n_neighbors, queries=None, exclude_self=None, pg=None, candidate_chunk=None, blocks=0, query_block=None):
    """The exact n_neighbors nearest rows of Y, an (n, d) float32 device tensor (unit column stride, row stride >= d; with `pg`:
    this rank's rows), for every row of `queries` ((n_q, d) float32, same device), or of Y itself.

    The squared distance of a pair is sum_j (q_j - y_j)^2 in float32 as one sequential fma chain (oriana_knn); a row of the
    result holds the candidates smallest under (distance, index), in that order, padded with index -1 / distance +inf where
    fewer exist.  exclude_self (default: True exactly when queries is None) leaves a row out of its own list -- only itself:
    other identical rows come back at distance 0.  candidate_chunk splits the candidates over merging calls and query_block
    the queries over calls (default: one call unless its scratch exceeds SCRATCH_BUDGET, see knn_plan()); `blocks` is
    oriana_knn's.  None of them changes a bit of the result.

    Under row sharding the candidates are every rank's rows in rank order under their global indices: shard after shard is made
    available on all ranks by an all-reduce onto a zero buffer and merged in.  The concatenated output of the ranks equals a
    one-process run on the concatenated rows bit for bit; explicit queries are each rank's own.

    Returns {'indices': (n_q, k) int32, 'sq_distances': (n_q, k) float32}, device tensors.  ValueError before any launch for a
    wrong dtype, rank or device, non-finite entries, n_neighbors < 1 or beyond max_neighbors(d)."""
    _check_rows(Y, 'Y')
    if queries is not None:
        _check_rows(queries, 'queries')
        if int(queries.shape[1]) != int(Y.shape[1]):
            raise ValueError('queries have %d columns, Y has %d' % (queries.shape[1], Y.shape[1]))
    if exclude_self is None:
        exclude_self = queries is None
    if exclude_self and queries is not None:
        raise ValueError('exclude_self needs queries=None: explicit queries are not rows of Y')
    k, blocks = int(n_neighbors), int(blocks)
    n, d = int(Y.shape[0]), int(Y.shape[1])
    if k < 1:
        raise ValueError('n_neighbors must be at least 1')
    _check_cuts(blocks, candidate_chunk, query_block)
    kmax = max_neighbors(d) if d >= 1 else 0
    if kmax == 0:
        raise ValueError('%d features are not served' % d)
    if k > kmax:
        raise ValueError('n_neighbors = %d is beyond the %d served at %d features' % (k, kmax, d))
    if not Y.is_cuda or (queries is not None and queries.device != Y.device):
        raise ValueError('Y and queries must be tensors of one device')
    if not _all_finite(pg, *((Y,) if queries is None else (Y, queries))):
        raise ValueError('Y or queries have non-finite entries')
    rows = _Rows(Y, pg)
    if rows.N > 2 ** 31 - 1:
        raise ValueError('%d rows are beyond the int32 indices' % rows.N)

    dev = Y.device
    Q, q0 = (Y, rows.row0) if queries is None else (queries, 0)
    nq = int(Q.shape[0])
    # the shards (_Rows.shards) arrive in contiguous buffers of their own; without sharding the candidates are Y as it lies
    y_ptr, ldy = (16, d) if odist.sharded(pg) else (ptr(Y) if n else None, _rows_ld(Y)[1])
    qb, chunk, nbytes = knn_plan(nq, max(rows.sizes), d, k, blocks, y_ptr, ldy, candidate_chunk, query_block)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
    d2 = torch.empty(nq, k, dtype=torch.float32, device=dev)
    merge = False
    for y0, cand in rows.shards():
        for a in range(0, int(cand.shape[0]), chunk):
            for b in range(0, nq, qb):
                knn_step(Q[b:b + qb], cand[a:a + chunk], idx[b:b + qb], d2[b:b + qb], q0=q0 + b, y0=y0 + a,
                         exclude_self=exclude_self, merge=merge, blocks=blocks, scratch=scratch)
            merge = True
    if not merge:                                     # (no candidates at all: the padding values)
        knn_step(Q, Y[:0], idx, d2, q0=q0, blocks=blocks)
    return {'indices': idx, 'sq_distances': d2}


# ---- the silhouette of a labelling (csrc/silhouette.hip) ------------------------------------------------------
def max_clusters():
    """The largest number of clusters one oriana_cluster_distance_sums call serves."""
    return int(_lib.load().oriana_cluster_distance_sums_max_clusters())


def _sums_scratch_bytes(nq, n, d, C, blocks, y_ptr, ldy):
    """Bytes of scratch of one oriana_cluster_distance_sums call whose candidates start at y_ptr with row stride ldy."""
    return _scratch_bytes('oriana_cluster_distance_sums_scratch_bytes_for', nq, n, d, C, int(blocks), y_ptr, ldy)


def distance_sums(Q, Y, offsets, sums=None, accumulate=False, blocks=0, scratch=None):
    """One oriana_cluster_distance_sums call: for the rows of Q (nq, d) the float64 sums of the Euclidean distances to the
    candidates Y (n, d) of every cluster, both float32 device tensors (row stride >= d, unit column stride).  The candidates lie
    grouped by cluster: cluster c owns the rows [offsets[c], offsets[c + 1]) (C + 1 ascending host integers from 0 to n).
    sums : a (C, nq) float64 view with unit column stride (its row stride may exceed nq: what lies beyond nq is not touched);
    default a new tensor.  With `accumulate` the call's sums are added to what `sums` holds.  Returns `sums`."""
    nq, ldq = _rows_ld(Q)
    n, ldy = _rows_ld(Y)
    d = int(Q.shape[1])
    if int(Y.shape[1]) != d:
        raise ValueError('Q has %d columns, Y has %d' % (d, Y.shape[1]))
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    if off.ndim != 1 or off.size < 1:
        raise ValueError('offsets must be a 1-D array of C + 1 entries')
    C = int(off.size) - 1
    if sums is None:
        if accumulate:
            raise ValueError('accumulate needs the sums to add to')
        sums = torch.empty(C, nq, dtype=torch.float64, device=Q.device)
    if sums.dtype != torch.float64 or sums.dim() != 2 or tuple(sums.shape) != (C, nq) or (nq > 1 and sums.stride(1) != 1):
        raise ValueError('sums must be a (C, nq) = %s float64 tensor with unit column stride' % ((C, nq),))
    lds = int(sums.stride(0)) if C > 1 else nq
    if lds < nq:
        raise ValueError('the rows of sums overlap')
    scratch = _scratch_for(scratch, _sums_scratch_bytes(nq, n, d, C, blocks, ptr(Y) if n else None, ldy), Q.device)
    call('oriana_cluster_distance_sums', ptr(Q) if nq else None, nq, ldq, ptr(Y) if n else None, n, ldy, d, off.ctypes.data, C,
         ptr(sums), lds, 1 if accumulate else 0, ptr(scratch), int(blocks), stream_ptr())
    return sums


def silhouette_from_sums(S, counts, labels):
    """The silhouette of m rows from their distance sums: S (C, m) float64 (S[c, i] = sum of the distances of row i to the rows
    of cluster c, the row itself included at 0), counts (C,) the sizes of the clusters (all rows, not only these m) and labels
    (m,) the rows' own clusters.  a = S[A, i] / (n_A - 1), b = min over the non-empty c != A of S[c, i] / n_c,
    s = (b - a) / max(a, b); s = 0 (and a = 0) where n_A = 1, s = 0 where max(a, b) = 0 -- scikit-learn's silhouette_samples.
    Float64 torch on the device of S (the CPU included); one pass over the clusters, no second (C, m) array.
    Returns (values, a, b), (m,) float64."""
    if not isinstance(S, torch.Tensor) or S.dim() != 2 or S.dtype != torch.float64:
        raise ValueError('S must be a (C, m) float64 tensor')
    dev = S.device
    C, m = int(S.shape[0]), int(S.shape[1])
    cnt_h = np.asarray(counts.detach().cpu() if isinstance(counts, torch.Tensor) else counts).astype(np.int64).reshape(-1)
    if cnt_h.size != C or (cnt_h < 0).any():
        raise ValueError('counts must hold %d non-negative entries' % C)
    if int((cnt_h > 0).sum()) < 2:
        raise ValueError('the silhouette needs at least two non-empty clusters')
    lab = torch.as_tensor(np.asarray(labels) if not isinstance(labels, torch.Tensor) else labels).to(dev, torch.int64).reshape(-1)
    if int(lab.numel()) != m:
        raise ValueError('%d labels for %d rows' % (lab.numel(), m))
    cnt = torch.as_tensor(cnt_h).to(dev)
    own = cnt[lab] if m else cnt[:0]
    a = S.gather(0, lab[None, :])[0] / (own - 1).clamp(min=1).to(torch.float64)
    a = torch.where(own > 1, a, torch.zeros_like(a))
    b = torch.full((m,), float('inf'), dtype=torch.float64, device=dev)
    for c in np.nonzero(cnt_h)[0]:
        b = torch.where(lab == int(c), b, torch.minimum(b, S[int(c)] / float(cnt_h[c])))
    top = torch.maximum(a, b)
    ok = (own > 1) & (top > 0)
    values = torch.where(ok, (b - a) / torch.where(ok, top, torch.ones_like(top)), torch.zeros_like(top))
    return values, a, b


def silhouette_plan(nq, n, d, C, blocks=0, candidate_chunk=None, query_block=None, budget=None, resident=False):
    """How silhouette() cuts nq queries against n candidates (of its largest shard) in C clusters into distance_sums() calls:
    (query_block, candidate_chunk, scratch bytes that serve every call issued).  Needs no device.  What is not given is chosen so
    that the sums of a query block (C x block x 8 bytes; with `resident`, the row-sharded run, of all nq queries), the copy of a
    candidate chunk grouped by cluster (its rows, labels and sort permutation) and the kernel scratch (a padded image where d is
    no multiple of four, and 512 bytes per query tile and work item) stay within `budget` (default SCRATCH_BUDGET): first the
    candidates are halved until their part takes at most half the budget, then the queries, in whole tiles, until all fits.  As
    for knn_plan() the scratch of a call is not monotone in its queries, so the bytes are the largest need over the block sizes
    that occur.  Either split changes the float64 summation order and nothing else."""
    nq, n, d, C = int(nq), int(n), int(d), int(C)

    def scratch(qb, c):                               # (the grouped copy is contiguous and aligned)
        return max(_sums_scratch_bytes(b, min(c, n), d, C, blocks, 16, d) for b in _block_sizes(nq, qb))

    def candidates(c):
        return min(c, n) * (4 * d + 24)

    def need(qb, c):
        return scratch(qb, c) + candidates(c) + 8 * C * (nq if resident else min(qb, nq))

    return _plan(nq, n, candidate_chunk, query_block, budget, scratch, need,
                 chunk_need=lambda c, tile: candidates(c) + (scratch(tile, c) - scratch(tile, 1)))


def _label_tensor(labels, n, what):
    """`labels` (an integer array or tensor of n entries) as a 1-D int64 tensor on the device it lives on."""
    if isinstance(labels, torch.Tensor):
        t = labels.detach()
        if t.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError('%s must be integers, got %s' % (what, t.dtype))
    else:
        arr = np.asarray(labels)
        if arr.dtype.kind not in 'iu':
            raise ValueError('%s must be integers, got %s' % (what, arr.dtype))
        t = torch.as_tensor(arr.astype(np.int64))
    if t.dim() != 1:
        raise ValueError('%s must be one-dimensional' % what)
    if n is not None and int(t.numel()) != n:
        raise ValueError('%d %s for %d rows' % (t.numel(), what, n))
    t = t.to(torch.int64)
    if t.numel() and int(t.min()) < 0:
        raise ValueError('%s must not be negative' % what)
    return t


def _global_max(v, device, pg):
    """max of one integer per rank (a zero buffer with the rank's own slot filled, summed over the ranks)."""
    if not odist.sharded(pg):
        return int(v)
    t = torch.zeros(odist.world_size(pg), dtype=torch.int64, device=device)
    t[odist.rank(pg)] = int(v)
    odist.all_reduce_sum(t, pg)
    return int(t.max())


def silhouette(Y, labels, n_clusters=None, pg=None, candidate_chunk=None, query_block=None, blocks=0):
    """The exact silhouette (Euclidean metric, scikit-learn's silhouette_samples) of the labelling `labels` of the rows of Y, an
    (n, d) float32 device tensor (unit column stride, row stride >= d; with `pg`: this rank's rows and their labels).

    labels : an integer array or tensor of n entries in [0, n_clusters) (default n_clusters: the largest label + 1); ids without
    rows are allowed and ignored.  All n^2 distances are formed, in float32 as oriana_knn forms them and then the correctly rounded
    square root, and added per cluster in float64 (oriana_cluster_distance_sums); no distance matrix exists.  A candidate chunk
    (first a range of rows) is grouped by cluster with a stable argsort and index_select -- candidate_chunk bounds that copy --
    and the queries are taken in blocks of query_block rows whose (C, block) sums are assembled and dropped; what is not given,
    silhouette_plan() chooses.  `blocks` is oriana_cluster_distance_sums'.  None of the three changes more than the order of the
    float64 additions.

    Under row sharding the candidates are every rank's rows: shard after shard of rows AND labels is made available on all ranks
    by an all-reduce onto a zero buffer and accumulated into the rank's own (C, n) sums, WHICH STAY RESIDENT until the last
    shard is in (8 C bytes per local row); the counts are all-reduced.

    Returns a dict: 'values', 'a', 'b' (n,) float64 device tensors in the caller's row order (this rank's rows), 'mean' (float,
    over all ranks), 'cluster_means' (C,) float64 NumPy (NaN for an id without rows) and 'counts' (C,) int64 NumPy (global).
    ValueError before any launch for a wrong dtype, rank or device, non-finite Y, negative labels, a label count other than n,
    fewer than 2 or more than N - 1 non-empty clusters, or more clusters than max_clusters()."""
    _check_rows(Y, 'Y')
    n, d = int(Y.shape[0]), int(Y.shape[1])
    blocks = int(blocks)
    if d < 1 or d > 256:
        raise ValueError('%d features are not served' % d)
    _check_cuts(blocks, candidate_chunk, query_block)
    lab = _label_tensor(labels, n, 'labels')
    sharded = odist.sharded(pg)
    if sharded and not Y.is_cuda:
        raise ValueError('Y must be a device tensor')
    lab = lab.to(Y.device)
    top = _global_max(int(lab.max()) + 1 if n else 0, Y.device, pg)
    C = top if n_clusters is None else int(n_clusters)
    if C < top:
        raise ValueError('labels must lie in [0, n_clusters = %d)' % C)
    if C > max_clusters():
        raise ValueError('%d clusters are beyond the %d served' % (C, max_clusters()))
    counts = torch.bincount(lab, minlength=C).to(torch.float64)              # (exact: counts stay below 2^53)
    packed = torch.cat([counts, 1.0 - _finite_flag(Y)])         # (the flag travels with the counts: one all-reduce)
    odist.all_reduce_sum(packed, pg)
    packed = packed.cpu().numpy()
    counts_h = packed[:C].astype(np.int64)
    N, filled = int(counts_h.sum()), int((counts_h > 0).sum())
    if packed[C] > 0:
        raise ValueError('Y has non-finite entries')
    if not 2 <= filled <= N - 1:
        raise ValueError('the silhouette needs between 2 and N - 1 = %d non-empty clusters, got %d' % (N - 1, filled))
    if not Y.is_cuda:
        raise ValueError('Y must be a device tensor')

    dev = Y.device
    rows = _Rows(Y, pg)
    qb, chunk, nbytes = silhouette_plan(n, max(rows.sizes), d, C, blocks, candidate_chunk, query_block, resident=sharded)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    out = {k: torch.empty(n, dtype=torch.float64, device=dev) for k in ('values', 'a', 'b')}

    def grouped(cand, clab, a0, a1):
        """Rows [a0, a1) grouped by cluster, and the clusters' offsets."""
        part = clab[a0:a1]
        rows_c = cand[a0:a1].index_select(0, torch.argsort(part, stable=True))
        off = np.zeros(C + 1, dtype=np.int64)
        off[1:] = np.cumsum(torch.bincount(part, minlength=C).cpu().numpy())
        return rows_c, off

    def assemble(S, b0, b1):
        out['values'][b0:b1], out['a'][b0:b1], out['b'][b0:b1] = silhouette_from_sums(S, counts_h, lab[b0:b1])

    if sharded:
        S = torch.zeros(C, n, dtype=torch.float64, device=dev)
        for _, cand, clab in rows.shards(lab):
            ns = int(cand.shape[0])
            for a0 in range(0, ns, chunk):
                g, off = grouped(cand, clab, a0, min(a0 + chunk, ns))
                for b0 in range(0, n, qb):
                    distance_sums(Y[b0:b0 + qb], g, off, sums=S[:, b0:b0 + qb], accumulate=True, blocks=blocks, scratch=scratch)
        for b0 in range(0, n, qb):
            assemble(S[:, b0:b0 + qb], b0, min(b0 + qb, n))
    else:
        whole = grouped(Y, lab, 0, n) if chunk >= n else None         # (one chunk: grouped once for all query blocks)
        for b0 in range(0, n, qb):
            b1 = min(b0 + qb, n)
            S = torch.empty(C, b1 - b0, dtype=torch.float64, device=dev)
            for a0 in range(0, n, chunk):
                g, off = whole if whole is not None else grouped(Y, lab, a0, min(a0 + chunk, n))
                distance_sums(Y[b0:b1], g, off, sums=S, accumulate=a0 > 0, blocks=blocks, scratch=scratch)
            assemble(S, b0, b1)

    sums = torch.zeros(C + 1, dtype=torch.float64, device=dev)
    sums[:C].index_add_(0, lab, out['values'])
    sums[C] = out['values'].sum()
    odist.all_reduce_sum(sums, pg)
    sums = sums.cpu().numpy()
    with np.errstate(invalid='ignore', divide='ignore'):
        means = np.where(counts_h > 0, sums[:C] / counts_h, np.nan)
    out.update(mean=float(sums[C] / N), cluster_means=means, counts=counts_h)
    return out


def adjusted_rand(labels_a, labels_b, pg=None):
    """The adjusted Rand index of two labellings of the same rows (integer arrays or tensors of non-negative ids; with `pg`: this
    rank's rows), exact: the contingency table comes from torch.bincount on the labels' device (all-reduced under sharding), the
    pair counts of scikit-learn's formula 2 (tp tn - fn fp) / ((tp + fn)(fn + tn) + (tp + fp)(fp + tn)) are Python integers up
    to the one final division (their products pass 2^63 from about 10^5 rows on).  1.0 where both labellings agree on every pair,
    two single-cluster labellings included."""
    a = _label_tensor(labels_a, None, 'labels_a')
    b = _label_tensor(labels_b, int(a.numel()), 'labels_b')
    dev = b.device if b.is_cuda else a.device
    a, b = a.to(dev), b.to(dev)
    m = int(a.numel())
    Ca = _global_max(int(a.max()) + 1 if m else 0, dev, pg)
    Cb = _global_max(int(b.max()) + 1 if m else 0, dev, pg)
    if Ca * Cb > 1 << 26:
        raise ValueError('a contingency table of %d x %d entries is not served' % (Ca, Cb))
    table = torch.bincount(a * Cb + b, minlength=Ca * Cb)
    odist.all_reduce_sum(table, pg)
    M = table.cpu().numpy().reshape(Ca, Cb)
    n = int(M.sum())
    squares = sum(int(v) ** 2 for v in M[M > 0])
    rows2 = sum(int(v) ** 2 for v in M.sum(1))
    cols2 = sum(int(v) ** 2 for v in M.sum(0))
    tp, fp, fn = squares - n, cols2 - squares, rows2 - squares
    tn = n * n - fp - fn - squares
    if fn == 0 and fp == 0:
        return 1.0
    return 2 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


# ---- the exact t-SNE layout (csrc/tsne.hip) --------------------------------------------------------------------
def tsne_default_neighbors(perplexity, d, n, kmax=None):
    """n_neighbors where tsne() is given none: min(ceil(3 perplexity), max_neighbors(d), n - 1).  `kmax` replaces the
    max_neighbors(d) of the library (then no library is needed)."""
    kmax = max_neighbors(d) if kmax is None else int(kmax)
    return min(int(math.ceil(3.0 * float(perplexity))), kmax, int(n) - 1)


def _check_layout(T, what):
    if not isinstance(T, torch.Tensor) or T.dim() != 2 or int(T.shape[1]) != 2:
        raise ValueError('%s must be an (n, 2) torch tensor' % what)
    if T.dtype != torch.float32:
        raise ValueError('%s must be float32, got %s' % (what, T.dtype))
    if not T.is_contiguous():
        raise ValueError('%s must be C-contiguous' % what)


def tsne_affinities(sq_distances, perplexity):
    """One oriana_tsne_affinities call: `sq_distances` (n, k) float32 contiguous device tensor as knn() returns it (rows ascending,
    padded with +inf).  Returns (p, beta): p (n, k) float32 with p[i, j] = p_{j|i} over the finite entries of row i at the beta[i]
    (float64) whose entropy is log(perplexity); exactly 0 at the padded slots.  ValueError for a perplexity below 1 and (one host
    read) for a row with fewer than ceil(perplexity) + 1 finite entries."""
    D = sq_distances
    if not isinstance(D, torch.Tensor) or D.dim() != 2 or D.dtype != torch.float32 or not D.is_contiguous() or int(D.shape[1]) < 1:
        raise ValueError('sq_distances must be a contiguous (n, k >= 1) float32 tensor')
    perplexity = float(perplexity)
    if not (1.0 <= perplexity < float('inf')):
        raise ValueError('perplexity must be a finite number >= 1')
    n, k = int(D.shape[0]), int(D.shape[1])
    need = int(math.ceil(perplexity)) + 1
    if n and int((D < float('inf')).sum(1).min()) < need:
        raise ValueError('a row has fewer than ceil(perplexity) + 1 = %d finite distances' % need)
    p = torch.empty(n, k, dtype=torch.float32, device=D.device)
    beta = torch.empty(n, dtype=torch.float64, device=D.device)
    call('oriana_tsne_affinities', ptr(D) if n else None, n, k, perplexity, ptr(p) if n else None, ptr(beta) if n else None,
         stream_ptr())
    return p, beta


def tsne_joint(indices, p):
    """The joint P = (p_{j|i} + p_{i|j}) / (2 n) of the conditional probabilities p (n, k) over the neighbours `indices` (n, k)
    int32, as CSR on the device: both directions as one COO matrix, coalesced by torch.  Padded slots (index -1) and exact zeros
    are dropped; the two directions are added in float64 (two terms: no order), the values are stored as float32, the columns
    ascend inside a row.  Returns {'crow': (n + 1) int64, 'col': (nnz) int32, 'val': (nnz) float32, 'n': n,
    'sum': the float64 sum of the stored values (a device scalar)}."""
    if not isinstance(indices, torch.Tensor) or not isinstance(p, torch.Tensor) or indices.dim() != 2 or indices.shape != p.shape:
        raise ValueError('indices and p must be (n, k) tensors of one shape')
    if indices.dtype not in (torch.int32, torch.int64) or p.dtype != torch.float32:
        raise ValueError('indices must be int32 or int64 and p float32')
    n, k = int(indices.shape[0]), int(indices.shape[1])
    dev = p.device
    idx = indices.to(torch.int64)
    keep = (idx >= 0) & (idx < n) & (p > 0)
    r = torch.arange(n, device=dev, dtype=torch.int64)[:, None].expand(n, k)[keep]
    c = idx[keep]
    v = p[keep].to(torch.float64)
    coo = torch.sparse_coo_tensor(torch.stack([torch.cat([r, c]), torch.cat([c, r])]), torch.cat([v, v]), (n, n)).coalesce()
    ij = coo.indices()
    val = (coo.values() / (2.0 * n)).to(torch.float32) if n else coo.values().to(torch.float32)
    crow = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        crow[1:] = torch.cumsum(torch.bincount(ij[0], minlength=n), 0)
    return {'crow': crow, 'col': ij[1].to(torch.int32).contiguous(), 'val': val.contiguous(), 'n': n,
            'sum': val.sum(dtype=torch.float64)}


def _check_joint(P, n):
    if not isinstance(P, dict) or int(P['n']) != n:
        raise ValueError('P must be what tsne_joint() returned for these %d rows' % n)
    crow, col, val = P['crow'], P['col'], P['val']
    if crow.dtype != torch.int64 or col.dtype != torch.int32 or val.dtype != torch.float32 or int(crow.numel()) != n + 1 \
            or col.numel() != val.numel() or not (crow.is_contiguous() and col.is_contiguous() and val.is_contiguous()):
        raise ValueError('P must hold int64 row pointers (n + 1), int32 columns and float32 values, contiguous')


def tsne_attract(P, Y):
    """One oriana_tsne_attract call: P as tsne_joint() returns it, Y (n, 2) float32 contiguous.  Returns (attr, klrow), float64:
    attr[i] = sum_j P_ij (y_i - y_j) / (1 + |y_i - y_j|^2), klrow[i] = sum_j P_ij (log P_ij + log(1 + |y_i - y_j|^2))."""
    _check_layout(Y, 'Y')
    n = int(Y.shape[0])
    _check_joint(P, n)
    attr = torch.empty(n, 2, dtype=torch.float64, device=Y.device)
    klrow = torch.empty(n, dtype=torch.float64, device=Y.device)
    nnz = int(P['col'].numel())
    call('oriana_tsne_attract', ptr(P['crow']), ptr(P['col']) if nnz else None, ptr(P['val']) if nnz else None,
         ptr(Y) if n else None, n, ptr(attr) if n else None, ptr(klrow) if n else None, stream_ptr())
    return attr, klrow


def _repulse_scratch_bytes(nq, n, blocks):
    return _scratch_bytes('oriana_tsne_repulse_scratch_bytes_for', int(nq), int(n), int(blocks))


def tsne_repulse(Q, Y, rep=None, zrow=None, accumulate=False, blocks=0, scratch=None):
    """One oriana_tsne_repulse call: for the queries Q (nq, 2) against ALL candidates Y (n, 2), float32 contiguous device tensors,
    rep[i] = sum_j w_ij^2 (q_i - y_j) ((nq, 2) float64) and zrow[i] = sum_j w_ij ((nq,) float64), w = 1 / (1 + |q_i - y_j|^2).
    rep / zrow : contiguous float64 tensors to write (default: new ones) or, with `accumulate`, to add to.  Returns (rep, zrow)."""
    _check_layout(Q, 'Q')
    _check_layout(Y, 'Y')
    nq, n = int(Q.shape[0]), int(Y.shape[0])
    if (rep is None or zrow is None) and accumulate:
        raise ValueError('accumulate needs the sums to add to')
    if rep is None:
        rep = torch.empty(nq, 2, dtype=torch.float64, device=Q.device)
    if zrow is None:
        zrow = torch.empty(nq, dtype=torch.float64, device=Q.device)
    if rep.dtype != torch.float64 or tuple(rep.shape) != (nq, 2) or not rep.is_contiguous():
        raise ValueError('rep must be a contiguous (nq, 2) = %s float64 tensor' % ((nq, 2),))
    if zrow.dtype != torch.float64 or tuple(zrow.shape) != (nq,) or not zrow.is_contiguous():
        raise ValueError('zrow must be a contiguous (nq,) = %s float64 tensor' % ((nq,),))
    scratch = _scratch_for(scratch, _repulse_scratch_bytes(nq, n, blocks), Q.device)
    call('oriana_tsne_repulse', ptr(Q) if nq else None, nq, ptr(Y) if n else None, n, ptr(rep) if nq else None,
         ptr(zrow) if nq else None, 1 if accumulate else 0, ptr(scratch), int(blocks), stream_ptr())
    return rep, zrow


def tsne_plan(n, blocks=0, query_block=None, candidate_chunk=None, budget=None):
    """How tsne_gradient() cuts the n x n repulsive pass into tsne_repulse() calls: (query_block, candidate_chunk, scratch bytes
    that serve every call issued).  What is not given: all candidates in one call (a chunk costs nothing but launches), and the
    queries halved in whole tiles until the scratch (1,536 bytes per query tile and candidate range) stays within `budget`
    (default SCRATCH_BUDGET)."""
    n = int(n)
    _check_cuts(blocks, candidate_chunk, query_block)

    def scratch(q, c):
        return max(_repulse_scratch_bytes(a, b, blocks) for a in _block_sizes(n, q) for b in _block_sizes(n, c))

    return _plan(n, n, candidate_chunk, query_block, budget, scratch)


def tsne_gradient(P, Y32, exaggeration=1.0, query_block=None, candidate_chunk=None, blocks=0):
    """The gradient of the t-SNE objective at the layout Y32 ((n, 2) float32 contiguous) for the joint P of tsne_joint():
    grad = 4 (exaggeration attr - rep / Z), (n, 2) float64, with Z = sum zrow - n (the n self pairs, each exactly 1), and
    kl = sum klrow + log Z sum P, the Kullback-Leibler divergence where exaggeration = 1, as a device scalar.  Everything is
    enqueued on the current stream; nothing is read on the host.  Returns (grad, kl)."""
    _check_layout(Y32, 'Y32')
    n = int(Y32.shape[0])
    _check_joint(P, n)
    qb, chunk, nbytes = tsne_plan(n, blocks, query_block, candidate_chunk)
    dev = Y32.device
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    attr, klrow = tsne_attract(P, Y32)
    rep = torch.empty(n, 2, dtype=torch.float64, device=dev)
    zrow = torch.empty(n, dtype=torch.float64, device=dev)
    for b in range(0, n, qb):
        for a in range(0, n, chunk):
            tsne_repulse(Y32[b:b + qb], Y32[a:a + chunk], rep[b:b + qb], zrow[b:b + qb], accumulate=a > 0, blocks=blocks,
                         scratch=scratch)
    Z = zrow.sum() - float(n)
    grad = 4.0 * (float(exaggeration) * attr - rep / Z)
    kl = klrow.sum() + torch.log(Z) * P['sum']
    return grad, kl


def tsne_pca_init(Y):
    """The start of init='pca': the rows of Y (n, d) float32 projected on the top two principal axes of the d x d covariance
    (torch.linalg.eigh in float64), every axis signed so that its largest-magnitude loading is positive, rescaled so that the
    first coordinate has standard deviation 1e-4 (scikit-learn's rule).  (n, 2) float64 on Y's device."""
    n, d = int(Y.shape[0]), int(Y.shape[1])
    mean = Y.sum(0, dtype=torch.float64) / n
    cov = torch.zeros(d, d, dtype=torch.float64, device=Y.device)
    for a in range(0, n, 1 << 18):
        X = Y[a:a + (1 << 18)].to(torch.float64) - mean
        cov += X.T @ X
    _, vec = torch.linalg.eigh(cov / max(n - 1, 1))
    axes = vec[:, -2:].flip(1) if d >= 2 else torch.cat([vec, torch.zeros_like(vec)], 1)      # (eigenvalues ascend)
    top = axes.gather(0, axes.abs().argmax(0, keepdim=True))[0]
    axes = axes * torch.where(top < 0, -torch.ones_like(top), torch.ones_like(top))
    out = torch.empty(n, 2, dtype=torch.float64, device=Y.device)
    for a in range(0, n, 1 << 18):
        out[a:a + (1 << 18)] = (Y[a:a + (1 << 18)].to(torch.float64) - mean) @ axes
    sd = out[:, 0].std(unbiased=False)
    return out / sd * 1e-4


def _tsne_descend(P, y, n_steps, exaggeration, momentum, lr, kw, trace=None, check_every=0, it0=0):
    """scikit-learn's _gradient_descent on the float64 master copy y (in place): gains + 0.2 where the update and the gradient
    disagree in sign, x 0.8 elsewhere, floor 0.01; update = momentum update - lr gains grad.  Update and gains start afresh."""
    update = torch.zeros_like(y)
    gains = torch.ones_like(y)
    for it in range(n_steps):
        grad, kl = tsne_gradient(P, y.to(torch.float32), exaggeration, **kw)
        inc = update * grad < 0.0
        gains = torch.where(inc, gains + 0.2, gains * 0.8).clamp_(min=0.01)
        update = momentum * update - lr * (gains * grad)
        y += update
        if trace is not None and (it0 + it + 1) % check_every == 0:
            trace.append((it0 + it, float(kl)))                                # (the KL at the layout BEFORE this step)
    return y


def tsne(Y, perplexity=20.0, n_neighbors=None, n_iter=750, early_exaggeration=12.0, exaggeration_iter=250, learning_rate='auto',
         init='pca', seed=0, graph=None, check_every=50, pg=None, **plan_kw):
    """The exact t-SNE layout in two dimensions of the rows of Y, an (n, d) float32 device tensor (unit column stride).

    The neighbour graph is knn(Y, n_neighbors) (or `graph` = (indices, sq_distances) as knn() / cell_neighbors() returned them,
    tensors or arrays); n_neighbors defaults to tsne_default_neighbors(); perplexity <= n_neighbors / 2 is required.  The
    affinities are tsne_affinities() and tsne_joint(); the gradient is tsne_gradient() -- the repulsive term over all n^2 pairs,
    nothing approximated, nothing random after the start.  The optimiser is scikit-learn's: `exaggeration_iter` iterations with
    P x early_exaggeration at momentum 0.5, then the rest of `n_iter` at momentum 0.8, gains + 0.2 / x 0.8 with floor 0.01
    (update and gains start afresh at the switch, as scikit-learn's two calls do), learning_rate 'auto' =
    max(n / early_exaggeration / 4, 50); elementwise torch on a float64 master copy of the layout whose float32 cast the kernels
    read.  init : 'pca' (tsne_pca_init), 'random' (N(0, 1e-4^2) from a host generator seeded with `seed`) or an (n, 2) array.
    plan_kw : query_block, candidate_chunk, blocks of tsne_gradient(), and candidate_chunk / blocks also serve knn().

    The host reads the KL divergence every `check_every` iterations after the exaggeration ends, and nothing else.
    Returns a dict: 'embedding' (n, 2) float64 device tensor, 'kl' (float, at the final layout's float32 cast, exaggeration 1),
    'kl_trace' (a list of (iteration, kl)), 'n_iter', 'beta' (n,) float64 device tensor, 'n_neighbors'.
    ValueError before any launch for a wrong dtype, rank or device, non-finite entries or arguments out of range;
    NotImplementedError for a process group of more than one rank: row-sharded layouts are not implemented."""
    if odist.world_size(pg) > 1:
        raise NotImplementedError('tsne() is not implemented for a process group of more than one rank: gather the rows first')
    _check_rows(Y, 'Y')
    n, d = int(Y.shape[0]), int(Y.shape[1])
    perplexity, n_iter, exaggeration_iter = float(perplexity), int(n_iter), int(exaggeration_iter)
    early_exaggeration, check_every = float(early_exaggeration), int(check_every)
    unknown = set(plan_kw) - {'query_block', 'candidate_chunk', 'blocks'}
    if unknown:
        raise ValueError('unknown arguments: %s' % ', '.join(sorted(unknown)))
    if n < 4 or d < 1:
        raise ValueError('tsne() needs at least 4 rows and one column')
    if not (1.0 <= perplexity < float('inf')):
        raise ValueError('perplexity must be a finite number >= 1')
    if n_iter < 0 or not 0 <= exaggeration_iter <= n_iter or check_every < 1 or not early_exaggeration >= 1.0:
        raise ValueError('0 <= exaggeration_iter <= n_iter, check_every >= 1 and early_exaggeration >= 1 are required')
    if learning_rate != 'auto' and not float(learning_rate) > 0.0:
        raise ValueError("learning_rate must be 'auto' or positive")
    explicit = None
    if not isinstance(init, str):
        explicit = np.asarray(init.detach().cpu() if isinstance(init, torch.Tensor) else init, dtype=np.float64)
        if explicit.shape != (n, 2) or not np.isfinite(explicit).all():
            raise ValueError('init must be a finite (n, 2) = %s array' % ((n, 2),))
    elif init not in ('pca', 'random'):
        raise ValueError("init must be 'pca', 'random' or an (n, 2) array")
    if graph is not None:
        gi, gd = graph
        k = int(gi.shape[1]) if getattr(gi, 'ndim', 0) == 2 else 0
        if tuple(gi.shape) != (n, k) or tuple(gd.shape) != (n, k) or k < 1:
            raise ValueError('graph must be (indices, sq_distances), both (n, k)')
        if n_neighbors is not None and int(n_neighbors) != k:
            raise ValueError('n_neighbors = %d, the graph holds %d' % (int(n_neighbors), k))
    else:
        kmax = max_neighbors(d)
        if kmax == 0:
            raise ValueError('%d features are not served' % d)
        k = tsne_default_neighbors(perplexity, d, n, kmax) if n_neighbors is None else int(n_neighbors)
        if k < 1 or k > kmax or k > n - 1:
            raise ValueError('n_neighbors = %d must lie within 1..min(%d, n - 1 = %d)' % (k, kmax, n - 1))
    if not perplexity <= k / 2.0:
        raise ValueError('perplexity = %g needs n_neighbors >= %d, got %d' % (perplexity, int(math.ceil(2 * perplexity)), k))
    if not Y.is_cuda:
        raise ValueError('Y must be a device tensor')
    if not bool(torch.isfinite(Y).all()):
        raise ValueError('Y has non-finite entries')

    dev = Y.device
    if graph is None:
        g = knn(Y, k, **{a: plan_kw[a] for a in ('candidate_chunk', 'blocks') if a in plan_kw})
        gi, gd = g['indices'], g['sq_distances']
    else:
        gi = torch.as_tensor(np.asarray(gi) if not isinstance(gi, torch.Tensor) else gi).to(dev, torch.int32).contiguous()
        gd = torch.as_tensor(np.asarray(gd) if not isinstance(gd, torch.Tensor) else gd).to(dev, torch.float32).contiguous()
    p, beta = tsne_affinities(gd, perplexity)
    P = tsne_joint(gi, p)
    if explicit is not None:
        y = torch.as_tensor(explicit).to(dev)
    elif init == 'pca':
        y = tsne_pca_init(Y)
    else:
        gen = torch.Generator()
        gen.manual_seed(int(seed))
        y = (torch.randn(n, 2, dtype=torch.float64, generator=gen) * 1e-4).to(dev)
    y = y.clone()
    lr = max(n / early_exaggeration / 4.0, 50.0) if learning_rate == 'auto' else float(learning_rate)
    trace = []
    _tsne_descend(P, y, exaggeration_iter, early_exaggeration, 0.5, lr, plan_kw)
    _tsne_descend(P, y, n_iter - exaggeration_iter, 1.0, 0.8, lr, plan_kw, trace, check_every, exaggeration_iter)
    _, kl = tsne_gradient(P, y.to(torch.float32), 1.0, **plan_kw)
    return {'embedding': y, 'kl': float(kl), 'kl_trace': trace, 'n_iter': n_iter, 'beta': beta, 'n_neighbors': k}


# ---- communities on the neighbour graph (csrc/community.hip) -----------------------------------------------------
LOUVAIN_MAX_2M = 3037000499       # floor(sqrt(2^63 - 1)): (2m)^2 < 2^63, so every product of a sweep is exact in int64


def louvain_row_cap():
    """The longest row whose table oriana_louvain_sweep keeps in LDS, and the largest `row_cap`."""
    return int(_lib.load().oriana_louvain_row_cap())


def _csr_pointers(rows, n):
    crow = torch.zeros(n + 1, dtype=torch.int64, device=rows.device)
    if n:
        crow[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    return crow


def _check_indices(indices, weights=None):
    """The refusals snn_graph() (with its `weights`) and diffusion_graph() share, in snn_graph()'s order."""
    if not isinstance(indices, torch.Tensor) or indices.dim() != 2 or indices.dtype != torch.int32:
        raise ValueError('indices must be an (n, k) int32 torch tensor')
    if weights is not None and weights not in ('snn', 'count'):
        raise ValueError("weights must be 'snn' or 'count'")
    if int(indices.shape[1]) < 1:
        raise ValueError('indices must hold at least one column')


def _neighbour_pattern(indices):
    """The symmetric pattern of the neighbour lists `indices` ((n, k) int32, checked by _check_indices), for snn_graph() and
    diffusion_graph(): N(i) = the entries of row i inside [0, n) other than i; {i, j} is stored iff j is in N(i) or i is in N(j).
    Returns {'valid': (n, k) bool, 'r', 'c': the (row, neighbour) of every valid entry in row-major order, int64, 'key': the stored
    pairs as row * n + column, ascending, 'count': per stored pair [j in N(i)] + [i in N(j)], 'rows' int64, 'col' int32, 'crow'}.
    ValueError (one device sort, one host read) for a row that holds a valid entry twice."""
    n, k = int(indices.shape[0]), int(indices.shape[1])
    dev = indices.device
    idx = indices.to(torch.int64)
    me = torch.arange(n, device=dev, dtype=torch.int64)[:, None]
    valid = (idx >= 0) & (idx < n) & (idx != me)
    srt = torch.sort(torch.where(valid, idx, torch.full_like(idx, -1)), dim=1).values
    if n and k > 1 and bool(((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any()):
        raise ValueError('a row of indices holds a neighbour twice')
    r = me.expand(n, k)[valid]
    c = idx[valid]
    key, cnt = torch.unique(torch.cat([r * n + c, c * n + r]), return_counts=True)        # (sorted: rows, then columns, ascend)
    rows = torch.div(key, max(n, 1), rounding_mode='floor')
    col = (key - rows * n).to(torch.int32).contiguous()
    return {'valid': valid, 'r': r, 'c': c, 'key': key, 'count': cnt, 'rows': rows, 'col': col, 'crow': _csr_pointers(rows, n)}


def snn_graph(indices, weights='snn'):
    """The symmetric weighted graph of the neighbour lists `indices`, an (n, k) int32 tensor as knn() / cell_neighbors() return it.
    N(i) = the entries of row i inside [0, n) other than i (anything else, the -1 padding included, is skipped); {i, j} is an edge
    iff j is in N(i) or i is in N(j).  weights : 'snn' -- w_ij = |Nc(i) & Nc(j)| with Nc(i) = N(i) and i itself, the
    shared-neighbour count (oriana_snn_weights; needs a device tensor and k <= max_neighbors(1)); 'count' -- w_ij = [j in N(i)] +
    [i in N(j)], formed by torch on the tensor's device.  Returns {'crow': (n + 1) int64, 'col': (nnz) int32 ascending inside a
    row, 'weight': (nnz) int64, 'n': n}, no self entries.  ValueError for a wrong dtype or rank and (one device sort, one host
    read) for a row that holds a valid entry twice."""
    _check_indices(indices, weights if weights is not None else '')
    n, k = int(indices.shape[0]), int(indices.shape[1])
    if weights == 'snn':
        if k > max_neighbors(1):
            raise ValueError('%d neighbours per row exceed the %d served' % (k, max_neighbors(1)))
        if not indices.is_cuda:
            raise ValueError("weights='snn' needs a device tensor")
    dev = indices.device
    pat = _neighbour_pattern(indices)
    crow, col, cnt = pat['crow'], pat['col'], pat['count']
    if weights == 'count':
        w = cnt.to(torch.int64).contiguous()
    else:
        w = torch.empty(int(col.numel()), dtype=torch.int64, device=dev)
        ind = indices.contiguous()
        nnz = int(col.numel())
        call('oriana_snn_weights', ptr(ind) if n else None, n, k, ptr(crow), ptr(col) if nnz else None, ptr(w) if nnz else None,
             stream_ptr())
    return {'crow': crow, 'col': col, 'weight': w, 'n': n}


def _graph_rows(crow, n):
    return torch.repeat_interleave(torch.arange(n, device=crow.device, dtype=torch.int64), crow[1:] - crow[:-1])


def _check_graph(graph, weight_dtype=torch.int64):
    """The validated graph: (crow, col, weight, n, rows, deg, two_m).  One torch check (one host read) for the pointers, the
    order inside the rows, the symmetry of pattern and weights and the sign of the weights.  weight_dtype : torch.int64 for the
    graphs of snn_graph(), torch.float64 for those of diffusion_graph(): their weights must be finite as well, and deg and two_m
    are None (a float sum by index_add_ has no fixed bits: the row sums of such a graph are oriana_csr_spmv_f64's)."""
    if not isinstance(graph, dict) or not all(a in graph for a in ('crow', 'col', 'weight', 'n')):
        raise ValueError("graph must be a dict with 'crow', 'col', 'weight' and 'n', as snn_graph() returns it")
    crow, col, w, n = graph['crow'], graph['col'], graph['weight'], int(graph['n'])
    if not all(isinstance(t, torch.Tensor) and t.dim() == 1 for t in (crow, col, w)):
        raise ValueError('crow, col and weight must be 1-D torch tensors')
    if crow.dtype != torch.int64 or col.dtype != torch.int32 or w.dtype != weight_dtype:
        raise ValueError('crow must be int64, col int32 and weight %s' % str(weight_dtype).replace('torch.', ''))
    if n < 0 or int(crow.numel()) != n + 1 or col.numel() != w.numel():
        raise ValueError('crow must hold n + 1 pointers, col and weight one entry per stored pair')
    if not (crow.device == col.device == w.device):
        raise ValueError('crow, col and weight must live on one device')
    if not (crow.is_contiguous() and col.is_contiguous() and w.is_contiguous()):
        raise ValueError('crow, col and weight must be contiguous')
    nnz = int(col.numel())
    lens = crow[1:] - crow[:-1]
    head = torch.stack([crow[0] != 0, crow[-1] != nnz, (lens < 0).any()]).cpu()
    if bool(head.any()):
        raise ValueError('crow must ascend from 0 to the number of stored entries')
    rows = _graph_rows(crow, n)
    c64 = col.to(torch.int64)
    key = rows * n + c64
    back = c64 * n + rows
    order = torch.argsort(back)
    flags = [((c64 < 0) | (c64 >= n)).any(), (key[1:] <= key[:-1]).any(), (back[order] != key).any(), (w[order] != w).any(),
             (w < 0).any()]
    exact = weight_dtype == torch.int64
    if not exact:
        flags[4] = flags[4] | ~torch.isfinite(w).all()
    deg = torch.zeros(n, dtype=torch.int64, device=w.device).index_add_(0, rows, w) if nnz and exact else \
        torch.zeros(n, dtype=torch.int64, device=w.device)
    bad = torch.stack(flags).cpu() if nnz else torch.zeros(5, dtype=torch.bool)
    if bool(bad[0]):
        raise ValueError('a column lies outside [0, n)')
    if bool(bad[1]):
        raise ValueError('the columns of a row must ascend strictly (an unsorted graph)')
    if not exact and bool(bad[4]):                                 # (ahead of the symmetry: NaN differs from itself)
        raise ValueError('the weights must be finite and not negative')
    if bool(bad[2]) or bool(bad[3]):
        raise ValueError('the graph must be symmetric in pattern and weights (an asymmetric graph)')
    if bool(bad[4]):
        raise ValueError('the weights must not be negative')
    if not exact:
        return crow, col, w, n, rows, None, None
    two_m = int(w.to(torch.float64).sum()) if nnz else 0           # (a first look that cannot wrap)
    if two_m > LOUVAIN_MAX_2M:
        raise ValueError('the weights sum to 2m = %d: (2m)^2 must stay below 2^63 (2m <= %d)' % (two_m, LOUVAIN_MAX_2M))
    two_m = int(deg.sum())
    return crow, col, w, n, rows, deg, two_m


def _check_resolution(resolution):
    resolution = float(resolution)
    if not (0.0 < resolution < float('inf')):
        raise ValueError('resolution must be finite and positive')
    return resolution


def _modularity_value(I, S, two_m, resolution):
    """Q = I / 2m - resolution S / (2m)^2 in float64 from the exact integers (0.0 for a graph without weight)."""
    if two_m == 0:
        return 0.0
    return I / two_m - resolution * float(S) / float(two_m * two_m)


def _partition_sums(rows, col, w, deg, comm, n):
    """Of a labelling comm (n) with ids in [0, n): tot (n) int64, size (n) int32, I and S as int64 device scalars."""
    c = comm.to(torch.int64)
    tot = torch.zeros(n, dtype=torch.int64, device=deg.device).index_add_(0, c, deg)
    size = torch.bincount(c, minlength=n).to(torch.int32)
    inside = torch.where(c[rows] == c[col.to(torch.int64)], w, torch.zeros_like(w)).sum()
    return tot, size, inside, (tot * tot).sum()


def modularity(graph, labels, resolution=1.0):
    """Newman's modularity with resolution, Q = I / 2m - resolution S / (2m)^2, of the labelling `labels` (integer ids >= 0, one
    per node) on a graph as snn_graph() returns it: I = the weight of the stored entries inside a community (self entries
    included), S = the sum of the squared community degrees, both exact integers formed by torch on the graph's device; the float64
    value is formed on the host from the two."""
    crow, col, w, n, rows, deg, two_m = _check_graph(graph)
    resolution = _check_resolution(resolution)
    lab = _label_tensor(labels, n, 'labels').to(crow.device)
    _, inv = torch.unique(lab, return_inverse=True)
    _, _, inside, squares = _partition_sums(rows, col, w, deg, inv, n)
    return _modularity_value(int(inside), int(squares), two_m, resolution)


def louvain_plan(graph, row_cap=None):
    """Which rows of the graph oriana_louvain_sweep serves through tables in the scratch, and where: {'row_cap', 'long_rows'
    (int32, the rows with more than row_cap entries), 'long_off' (int64, the first slot of each row's table and their total),
    'slots', 'scratch_bytes'}.  A row of len entries takes max(64, the least power of two >= 2 len) slots.  One host read."""
    crow = graph['crow']
    cap = louvain_row_cap() if row_cap is None else int(row_cap)
    if not 1 <= cap <= louvain_row_cap():
        raise ValueError('row_cap must lie within 1..%d' % louvain_row_cap())
    lens = crow[1:] - crow[:-1]
    long_rows = torch.nonzero(lens > cap).reshape(-1)
    L = lens[long_rows]
    T = torch.full_like(L, 64)
    for _ in range(32):
        T = torch.where(T < 2 * L, T * 2, T)
    off = torch.zeros(int(L.numel()) + 1, dtype=torch.int64, device=crow.device)
    off[1:] = torch.cumsum(T, 0)
    slots = int(off[-1])
    return {'row_cap': cap, 'long_rows': long_rows.to(torch.int32).contiguous(), 'long_off': off, 'slots': slots,
            'scratch_bytes': _scratch_bytes('oriana_louvain_sweep_scratch_bytes_for', slots)}


def louvain_sweep(graph, deg, two_m, comm, tot, size, resolution=1.0, plan=None, row_cap=None, blocks=0, scratch=None):
    """One oriana_louvain_sweep call, nothing checked beyond dtypes and sizes and nothing read on the host: graph as snn_graph()
    returns it (at aggregated levels with self entries), deg (n) int64 the row sums of the weights, two_m their sum (an int), the
    state comm (n) int32, tot (n) int64, size (n) int32.  Every node decides from this state (include/oriana_hip.h states the
    rule).  plan : louvain_plan(graph, row_cap), formed here if absent.  scratch : a uint8 device tensor; one that is too small for
    the plan sets 'overflow' and leaves everything else as it was.  Returns {'comm': (n) int32 the proposed labelling, 'moved':
    (1,) int64 the nodes that change, 'overflow': (1,) int32}, device tensors."""
    crow, col, w, n = graph['crow'], graph['col'], graph['weight'], int(graph['n'])
    for t, dt, m, what in ((crow, torch.int64, n + 1, 'crow'), (col, torch.int32, None, 'col'), (w, torch.int64, int(col.numel()), 'weight'),
                           (deg, torch.int64, n, 'deg'), (comm, torch.int32, n, 'comm'), (tot, torch.int64, n, 'tot'),
                           (size, torch.int32, n, 'size')):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1 or (m is not None and int(t.numel()) != m) \
                or not t.is_contiguous() or not t.is_cuda:
            raise ValueError('%s must be a contiguous 1-D %s device tensor%s' % (what, dt, '' if m is None else ' of %d entries' % m))
    if plan is None:
        plan = louvain_plan(graph, row_cap)
    dev = crow.device
    if scratch is None:
        scratch = torch.empty(plan['scratch_bytes'], dtype=torch.uint8, device=dev)
    # ('comm' starts as the labelling it was given: a sweep that overflows writes nothing, and louvain() sums over the proposed
    #  labelling before the host reads the flag -- with undefined entries those sums indexed out of bounds)
    out = {'comm': comm.clone(), 'moved': torch.zeros(1, dtype=torch.int64, device=dev),
           'overflow': torch.zeros(1, dtype=torch.int32, device=dev)}
    nnz, nlong = int(col.numel()), int(plan['long_rows'].numel())
    call('oriana_louvain_sweep', n, ptr(crow), ptr(col) if nnz else None, ptr(w) if nnz else None, ptr(deg) if n else None,
         int(two_m), float(resolution), ptr(comm) if n else None, ptr(tot) if n else None, ptr(size) if n else None,
         int(plan['row_cap']), ptr(plan['long_rows']) if nlong else None, ptr(plan['long_off']) if nlong else None, nlong,
         ptr(scratch), int(scratch.numel() * scratch.element_size()), ptr(out['comm']) if n else None, ptr(out['moved']),
         ptr(out['overflow']), int(blocks), stream_ptr())
    return out


def louvain(graph, resolution=1.0, max_sweeps=64, max_levels=32, row_cap=None, blocks=0, scratch=None, pg=None):
    """Deterministic Louvain communities of a graph as snn_graph() returns it (symmetric CSR, integer weights >= 0).

    A level starts from singletons.  A sweep (oriana_louvain_sweep) lets every node choose, from the state before the sweep, the
    neighbouring community of the largest gain, ties to the smallest id, with the swap guard for two singletons.  If no node moves
    the level ends; otherwise the sweep is accepted iff float64(2m (I_new - I)) > resolution float64(S_new - S), the exact integers
    of modularity(), that is iff the modularity rises; a rejected sweep is discarded and ends the level, and so do `max_sweeps`
    accepted sweeps (reported, not an error).  Between levels the communities are renumbered by ascending id and become the nodes
    of the coalesced graph, the weight inside a community its self entry.  The run ends when a level accepts no sweep or merges
    nothing, or after `max_levels`.  The final labels are renumbered by descending size, ties by the smallest member: 0 is the
    largest community.  Everything but the sweep is integer torch on the device; per sweep the host reads one small tensor (the
    moved count, I, S and the overflow flag), per level the plan's slot count and the level's own integers.

    row_cap, blocks : of louvain_sweep(); they change no bit.  scratch : a uint8 device tensor for the long rows' tables.
    Returns {'labels': (n,) int32 device tensor, 'n_communities', 'modularity' (float), 'levels': a list of {'nodes', 'sweeps'
    (accepted), 'moved' (per accepted sweep), 'modularity' (at the level's end), 'hit_max_sweeps'}}.
    ValueError before any launch for wrong dtypes, ranks or devices, a graph that is asymmetric or unsorted, negative weights, a
    resolution that is not finite and positive, or (2m)^2 >= 2^63; NotImplementedError for a process group of more than one
    rank."""
    if odist.world_size(pg) > 1:
        raise NotImplementedError('louvain() is not implemented for a process group of more than one rank: gather the graph first')
    resolution = _check_resolution(resolution)
    max_sweeps, max_levels, blocks = int(max_sweeps), int(max_levels), int(blocks)
    if max_sweeps < 1 or max_levels < 1 or blocks < 0:
        raise ValueError('max_sweeps >= 1, max_levels >= 1 and blocks >= 0 are required')
    crow, col, w, n, rows, deg, two_m = _check_graph(graph)
    if row_cap is not None and not 1 <= int(row_cap) <= louvain_row_cap():
        raise ValueError('row_cap must lie within 1..%d' % louvain_row_cap())
    if not crow.is_cuda:
        raise ValueError('the graph must live on the device')
    dev = crow.device
    n0 = n
    labels = torch.arange(n0, device=dev, dtype=torch.int64)
    levels = []
    for _ in range(max_levels):
        g = {'crow': crow, 'col': col, 'weight': w, 'n': n}
        comm = torch.arange(n, device=dev, dtype=torch.int32)
        tot, size, inside, squares = _partition_sums(rows, col, w, deg, comm, n)
        I, S = int(inside), int(squares)
        plan = louvain_plan(g, row_cap)
        moved, hit = [], False
        for _ in range(max_sweeps):
            out = louvain_sweep(g, deg, two_m, comm, tot, size, resolution, plan=plan, blocks=blocks, scratch=scratch)
            tot_n, size_n, inside_n, squares_n = _partition_sums(rows, col, w, deg, out['comm'], n)
            mv, I_n, S_n, over = (int(v) for v in torch.stack([out['moved'][0], inside_n, squares_n,
                                                               out['overflow'][0].to(torch.int64)]).cpu())
            if over:
                raise _lib.OrianaHipError('the scratch is too small for the tables of the long rows (%d bytes needed)'
                                          % plan['scratch_bytes'])
            if mv == 0 or not float(two_m * (I_n - I)) > resolution * float(S_n - S):
                break
            comm, tot, size, I, S = out['comm'], tot_n, size_n, I_n, S_n
            moved.append(mv)
        else:
            hit = True
        levels.append({'nodes': n, 'sweeps': len(moved), 'moved': moved, 'modularity': _modularity_value(I, S, two_m, resolution),
                       'hit_max_sweeps': hit})
        if not moved:
            break
        uniq, inv = torch.unique(comm.to(torch.int64), return_inverse=True)
        C = int(uniq.numel())
        labels = inv[labels]
        if C == n:
            break
        key, kinv = torch.unique(inv[rows] * C + inv[col.to(torch.int64)], return_inverse=True)
        w = torch.zeros(int(key.numel()), dtype=torch.int64, device=dev).index_add_(0, kinv, w)
        rows = torch.div(key, C, rounding_mode='floor')
        col = (key - rows * C).to(torch.int32).contiguous()
        n = C
        crow = _csr_pointers(rows, n)
        deg = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, rows, w)
    _, labels = torch.unique(labels, return_inverse=True)
    C = int(labels.max()) + 1 if n0 else 0
    sizes = torch.bincount(labels, minlength=C)
    first = torch.full((C,), n0, dtype=torch.int64, device=dev).scatter_reduce_(0, labels, torch.arange(n0, device=dev), 'amin')
    order = torch.argsort((n0 - sizes) * (n0 + 1) + first)
    rank = torch.empty(C, dtype=torch.int64, device=dev)
    rank[order] = torch.arange(C, device=dev)
    return {'labels': rank[labels].to(torch.int32), 'n_communities': C, 'modularity': levels[-1]['modularity'], 'levels': levels}


# ---- diffusion maps on the neighbour graph (csrc/diffusion.hip) --------------------------------------------------
def basis_tile_rows():
    """The rows of one partial sum of oriana_basis_orthogonalize_f64: a constant of the library."""
    return int(_lib.load().oriana_basis_tile_rows())


def _f64_device(t, least, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != 1 or not t.is_contiguous() or not t.is_cuda \
            or int(t.numel()) < least:
        raise ValueError('%s must be a contiguous 1-D float64 device tensor of at least %d entries' % (what, least))


def _check_basis(Q, n, j, what='Q'):
    """A basis is a (columns, ld) float64 device tensor, contiguous: column c is row c of the tensor, ld >= n and even."""
    if not isinstance(Q, torch.Tensor) or Q.dtype != torch.float64 or Q.dim() != 2 or not Q.is_contiguous() or not Q.is_cuda:
        raise ValueError('%s must be a contiguous (columns, ld) float64 device tensor' % what)
    if n < 0 or int(Q.shape[1]) < n or int(Q.shape[1]) % 2 or not 0 <= j <= int(Q.shape[0]):
        raise ValueError('%s must hold %d columns of ld >= %d entries, ld even' % (what, j, n))


def csr_spmv(crow, col, val, x, out=None, blocks=0):
    """y = A x by oriana_csr_spmv_f64 for the CSR matrix (crow (n + 1) int64, col int32, val float64) and x of at least n entries,
    device tensors; nothing of the matrix is checked.  A row's sum depends on the row alone: `blocks` changes no bit.  Returns y
    ((n,) float64; `out` if given)."""
    n = int(crow.numel()) - 1
    if crow.dtype != torch.int64 or col.dtype != torch.int32 or val.dtype != torch.float64 or col.numel() != val.numel() or n < 0 \
            or not (crow.is_cuda and crow.is_contiguous() and col.is_contiguous() and val.is_contiguous()) or int(blocks) < 0:
        raise ValueError('crow must be int64, col int32 and val float64, contiguous device tensors, and blocks >= 0')
    _f64_device(x, n, 'x')
    y = torch.empty(n, dtype=torch.float64, device=crow.device) if out is None else out
    _f64_device(y, n, 'out')
    nnz = int(col.numel())
    call('oriana_csr_spmv_f64', n, ptr(crow), ptr(col) if nnz else None, ptr(val) if nnz else None, ptr(x) if n else None,
         ptr(y) if n else None, int(blocks), stream_ptr())
    return y


def basis_orthogonalize(Q, n, j, w, h, beta2, passes=2, blocks=0, scratch=None):
    """One oriana_basis_orthogonalize_f64 call: `passes` (1 or 2) rounds of c = Q[:j] w, w -= Q[:j]^T c, h[:j] += c in place, then
    beta2[0] = ||w||^2, everything on the device.  Q : a basis as _check_basis() states it (column c is Q[c]); w at least n
    entries, h at least j (ADDED to: zero it for a new w), beta2 at least one.  scratch : a uint8 device tensor of at least
    oriana_basis_orthogonalize_scratch_bytes_for(n, j) bytes, contents undefined.  `blocks` changes no bit."""
    n, j = int(n), int(j)
    _check_basis(Q, n, j)
    if j < 1 or int(passes) not in (1, 2) or int(blocks) < 0:
        raise ValueError('j >= 1, passes 1 or 2 and blocks >= 0 are required')
    _f64_device(w, n, 'w')
    _f64_device(h, j, 'h')
    _f64_device(beta2, 1, 'beta2')
    need = _scratch_bytes('oriana_basis_orthogonalize_scratch_bytes_for', n, j)
    scratch = _scratch_for(scratch, need, Q.device)
    call('oriana_basis_orthogonalize_f64', n, ptr(Q), int(Q.shape[1]), j, ptr(w), ptr(h), ptr(beta2), int(passes), ptr(scratch),
         int(scratch.numel() * scratch.element_size()), int(blocks), stream_ptr())


def basis_append(Q, n, j, w, beta2):
    """Q[j] = w / sqrt(beta2[0]) by oriana_basis_append_f64; beta2 is read on the device."""
    n, j = int(n), int(j)
    _check_basis(Q, n, j + 1)
    _f64_device(w, n, 'w')
    _f64_device(beta2, 1, 'beta2')
    call('oriana_basis_append_f64', n, ptr(Q), int(Q.shape[1]), j, ptr(w), ptr(beta2), stream_ptr())


def basis_combine(Q, n, j, S, out=None, blocks=0):
    """out[c] = sum_k S[k, c] Q[k] over k = 0 .. j - 1 ascending (one fma chain per element) by oriana_basis_combine_f64: S a
    (j, m) float64 device tensor, out a basis of m columns (a new one of ld = Q's if absent).  Returns out."""
    n, j = int(n), int(j)
    _check_basis(Q, n, j)
    if not isinstance(S, torch.Tensor) or S.dtype != torch.float64 or S.dim() != 2 or int(S.shape[0]) != j or not S.is_contiguous() \
            or not S.is_cuda or j < 1 or int(blocks) < 0:
        raise ValueError('S must be a contiguous (j, m) float64 device tensor with j >= 1, and blocks >= 0')
    m = int(S.shape[1])
    if out is None:
        out = torch.empty(m, int(Q.shape[1]), dtype=torch.float64, device=Q.device)
    _check_basis(out, n, m, 'out')
    call('oriana_basis_combine_f64', n, ptr(Q), int(Q.shape[1]), j, ptr(S) if m else None, m, ptr(out) if m else None,
         int(out.shape[1]), int(blocks), stream_ptr())
    return out


def diffusion_graph(indices, sq_distances, blocks=0):
    """The symmetric diffusion transition matrix of the neighbour lists (indices, sq_distances), (n, k) int32 / float32 device
    tensors as knn() / cell_neighbors() return them (padded with -1 / inf), after Haghverdi et al. 2016 (scanpy's
    ``method='gauss'``), everything in float64.

    Pattern : that of snn_graph(): {i, j} is stored iff j is in N(i) or i is in N(j), no self entries, columns ascending.
    d2{i, j} : the value row min(i, j) stores for the other node if it lists it, else the value of row max(i, j): the same bits
        in both directions for any input.
    sigma_i^2 : np.median of the valid squared distances of row i (an even count: the mean of the two middle values); a zero
        median is replaced by the row's smallest positive valid value.
    W_ij = sqrt(2 sigma_i sigma_j / (sigma_i^2 + sigma_j^2)) exp(-d2_ij / (sigma_i^2 + sigma_j^2)); q = W 1, K_ij = W_ij /
    (q_i q_j); z = K 1, T_ij = K_ij / sqrt(z_i z_j).  The elementwise steps are float64 torch; the two row sums are
    oriana_csr_spmv_f64 applied to ones (no atomics: fixed bits; `blocks` changes none).

    Returns {'crow': (n + 1) int64, 'col': (nnz) int32, 'weight': (nnz) float64 the entries of T, bit-symmetric, 'n', 'z': (n)
    float64}.  ValueError for wrong dtypes, shapes or devices, a row that holds a neighbour twice, a valid entry whose distance is
    negative or not finite, and (stating their number) for rows without any positive valid distance."""
    _check_indices(indices)
    if not isinstance(sq_distances, torch.Tensor) or sq_distances.dtype != torch.float32 or sq_distances.shape != indices.shape \
            or sq_distances.device != indices.device:
        raise ValueError('sq_distances must be a float32 torch tensor of the shape and on the device of indices')
    if not indices.is_cuda:
        raise ValueError('diffusion_graph() needs device tensors')
    if int(blocks) < 0:
        raise ValueError('blocks >= 0 is required')
    n, k = int(indices.shape[0]), int(indices.shape[1])
    dev = indices.device
    pat = _neighbour_pattern(indices)
    valid, r, c, key, rows, col, crow = (pat[a] for a in ('valid', 'r', 'c', 'key', 'rows', 'col', 'crow'))
    d = sq_distances.to(torch.float64)
    inf = torch.full_like(d, float('inf'))
    shown = torch.where(valid, d, inf)
    cnt = valid.sum(1)
    srt = torch.sort(shown, dim=1).values
    lo = torch.gather(srt, 1, (torch.clamp(cnt - 1, min=0) // 2)[:, None])[:, 0]
    hi = torch.gather(srt, 1, torch.clamp(cnt // 2, max=k - 1)[:, None])[:, 0]
    med = (lo + hi) / 2
    pos = torch.where(valid & (d > 0), d, inf).min(1).values if n else med
    sig2 = torch.where((cnt > 0) & (med > 0), med, pos)
    dv = d[valid]
    flags = torch.stack([(~torch.isfinite(dv) | (dv < 0)).sum(), (~torch.isfinite(sig2)).sum()]).cpu()
    if int(flags[0]):
        raise ValueError('%d valid entries hold a squared distance that is negative or not finite' % int(flags[0]))
    if int(flags[1]):
        raise ValueError('%d rows hold no positive valid squared distance: their local scale is undefined' % int(flags[1]))
    nnz = int(col.numel())
    own = torch.zeros(nnz, dtype=torch.float64, device=dev)        # the value row i stores for j, per stored (i, j)
    other = torch.zeros(nnz, dtype=torch.float64, device=dev)      # the value row j stores for i
    has_own = torch.zeros(nnz, dtype=torch.bool, device=dev)
    has_other = torch.zeros(nnz, dtype=torch.bool, device=dev)
    fpos, bpos = torch.searchsorted(key, r * n + c), torch.searchsorted(key, c * n + r)
    own[fpos] = dv
    has_own[fpos] = True
    other[bpos] = dv
    has_other[bpos] = True
    c64 = col.to(torch.int64)
    low = rows < c64                                               # row min(i, j) is this entry's own row
    d2 = torch.where(torch.where(low, has_own, has_other), torch.where(low, own, other), torch.where(low, other, own))
    sig = torch.sqrt(sig2)
    den = sig2[rows] + sig2[c64]
    W = (torch.sqrt(2 * sig[rows] * sig[c64] / den) * torch.exp(-d2 / den)).contiguous()
    ones = torch.ones(n, dtype=torch.float64, device=dev)
    q = csr_spmv(crow, col, W, ones, blocks=blocks)
    K = (W / (q[rows] * q[c64])).contiguous()
    z = csr_spmv(crow, col, K, ones, blocks=blocks)
    T = (K / torch.sqrt(z[rows] * z[c64])).contiguous()
    return {'crow': crow, 'col': col, 'weight': T, 'n': n, 'z': z}


def graph_components(graph):
    """The connected components of a symmetric graph as snn_graph() or diffusion_graph() returns it, an entry of weight zero
    counting as absent: minimum-label propagation with pointer jumping in integer torch on the graph's device (one host read per
    round).  Returns {'labels': (n,) int64, the components numbered by their smallest member, 'n_components'}."""
    w = graph.get('weight') if isinstance(graph, dict) else None
    floats = isinstance(w, torch.Tensor) and w.dtype == torch.float64
    crow, col, w, n, rows, _, _ = _check_graph(graph, torch.float64 if floats else torch.int64)
    keep = w != 0
    a, b = rows[keep], col.to(torch.int64)[keep]
    lab = torch.arange(n, device=crow.device, dtype=torch.int64)
    while n:
        new = lab.clone().scatter_reduce_(0, a, lab[b], 'amin')                     # the least label among a node and its neighbours
        new = torch.minimum(new, lab.clone().scatter_reduce_(0, lab, new, 'amin')[lab])     # ... handed to the node's representative
        new = new[new]
        if bool((new == lab).all()):
            break
        lab = new
    uniq, inv = torch.unique(lab, return_inverse=True)                              # (ascending: by the smallest member)
    return {'labels': inv, 'n_components': int(uniq.numel())}


def _ritz(alpha, beta, m):
    """Of the Lanczos matrix (diagonal alpha, off-diagonal beta[:-1]): the m largest Ritz values, descending, their vectors
    (steps, m) and the residual estimates |beta[-1] s_last|."""
    steps = alpha.size
    Tm = np.diag(alpha)
    if steps > 1:
        Tm += np.diag(beta[:-1], 1) + np.diag(beta[:-1], -1)
    theta, S = np.linalg.eigh(Tm)
    top = np.argsort(-theta, kind='stable')[:m]
    return theta[top], np.ascontiguousarray(S[:, top]), np.abs(beta[-1] * S[-1, top])


def diffusion_map(graph, n_comps=15, tol=1e-8, max_steps=None, check_every=10, seed=0, start=None, blocks=0, pg=None):
    """The n_comps leading eigenpairs of the symmetric transition matrix T of diffusion_graph(): Lanczos with full
    reorthogonalisation, no restarts, float64 on the device (csrc/diffusion.hip).

    q_0 is `start` ((n,) float64) normalised, or without one ``torch.randn(n, float64)`` of a CPU generator seeded with `seed`.
    Step j: w = T q_j (oriana_csr_spmv_f64), w is orthogonalised against q_0 .. q_j by classical Gram-Schmidt applied twice
    (oriana_basis_orthogonalize_f64; alpha_j is the coefficient on q_j, beta_j = ||w||), q_{j+1} = w / beta_j is appended; nothing
    is read on the host.  Every `check_every` steps, and at the last, the host reads alpha and beta, takes numpy.linalg.eigh of the
    tridiagonal matrix and stops when |beta_j s_{last,l}| <= tol for the n_comps largest Ritz pairs.  The Ritz vectors are Q S
    (oriana_basis_combine_f64).  Every sum over rows has a fixed order: the result is a function of the graph and the start alone,
    the same bits for every `blocks` and on repetition.

    max_steps : default min(n, 1000), never more than n; the basis takes 8 ld (max_steps + 1) bytes (ld = n rounded up to even).
        The step count GROWS with n -- seeded blobs on the CPU: n = 2,000: 160 steps to tol 1e-6 / 180 to 1e-9; 20,000: 320 /
        360; 60,000: 430 / 480; a path of 20,000 nodes needs 150.  Not converged at max_steps is reported, not an error.
    A single vector cannot see the multiplicity of the eigenvalue 1 on a disconnected graph: graph_components() runs first (an
    entry of weight zero counts as absent) and more than one component is a ValueError that states their number.

    Returns {'eigenvalues': (m,) float64 NumPy, descending, 'components': (n, m) float64 device tensor, each column of unit norm
    (to the orthonormality of the basis) with its entry of largest magnitude positive (the smallest index on ties), 'residuals':
    (m,) the estimates of the last check, 'steps', 'converged'}.
    ValueError for a graph _check_graph() refuses or that lives on the host, n_comps outside [1, min(n, max_steps)], a start of
    the wrong shape or one that is zero or not finite; NotImplementedError for a process group of more than one rank."""
    if odist.world_size(pg) > 1:
        raise NotImplementedError('diffusion_map() is not implemented for a process group of more than one rank: gather the graph first')
    crow, col, w, n, rows, _, _ = _check_graph(graph, torch.float64)
    if not crow.is_cuda:
        raise ValueError('the graph must live on the device')
    if n < 1:
        raise ValueError('the graph has no nodes')
    dev = crow.device
    max_steps = min(n, 1000) if max_steps is None else int(max_steps)
    n_comps, check_every, blocks, tol = int(n_comps), int(check_every), int(blocks), float(tol)
    if max_steps < 1 or check_every < 1 or blocks < 0 or not tol >= 0.0:
        raise ValueError('max_steps >= 1, check_every >= 1, blocks >= 0 and tol >= 0 are required')
    max_steps = min(max_steps, n)
    if not 1 <= n_comps <= max_steps:
        raise ValueError('n_comps must lie within [1, min(n, max_steps)] = [1, %d]' % max_steps)
    if start is None:
        gen = torch.Generator()
        gen.manual_seed(int(seed))
        v = torch.randn(n, dtype=torch.float64, generator=gen).to(dev)
    else:
        v = torch.as_tensor(start)
        if v.dim() != 1 or int(v.numel()) != n:
            raise ValueError('start must hold %d entries' % n)
        v = v.to(dev, torch.float64).contiguous().clone()
        if not bool(torch.isfinite(v).all()) or not bool((v != 0).any()):
            raise ValueError('start must be finite and not zero')
    comps = graph_components(graph)['n_components']
    if comps > 1:
        raise ValueError('the graph has %d connected components: a diffusion map is defined on a connected graph' % comps)
    ld = n + (n & 1)
    Q = torch.empty(max_steps + 1, ld, dtype=torch.float64, device=dev)
    scratch = torch.empty(_scratch_bytes('oriana_basis_orthogonalize_scratch_bytes_for', n, max_steps), dtype=torch.uint8, device=dev)
    alpha = torch.zeros(max_steps, dtype=torch.float64, device=dev)
    beta2 = torch.zeros(max_steps + 1, dtype=torch.float64, device=dev)
    # q_0: against a zero column the orthogonalisation changes nothing and leaves ||start||^2 in the kernels' own order
    Q[0].zero_()
    basis_orthogonalize(Q, n, 1, v, torch.zeros(1, dtype=torch.float64, device=dev), beta2[max_steps:], passes=1, blocks=blocks,
                        scratch=scratch)
    basis_append(Q, n, 0, v, beta2[max_steps:])
    wv = torch.empty(ld, dtype=torch.float64, device=dev)
    theta = S = res = None
    steps, converged = 0, False
    for s in range(max_steps):
        s0 = s - s % check_every
        if s == s0:
            H = torch.zeros(min(check_every, max_steps - s0), max_steps, dtype=torch.float64, device=dev)    # the h of each step
        csr_spmv(crow, col, w, Q[s], out=wv, blocks=blocks)
        basis_orthogonalize(Q, n, s + 1, wv, H[s - s0], beta2[s:], passes=2, blocks=blocks, scratch=scratch)
        basis_append(Q, n, s + 1, wv, beta2[s:])
        if s + 1 - s0 < int(H.shape[0]):
            continue
        at = torch.arange(int(H.shape[0]), device=dev)
        alpha[s0:s + 1] = H[at, s0 + at]
        a, b2 = alpha[:s + 1].cpu().numpy(), beta2[:s + 1].cpu().numpy()
        steps = s + 1
        broke = np.flatnonzero(~(b2 > 0))                          # (beta = 0, or not a number: the Krylov space ended there)
        if broke.size:
            steps = int(broke[0]) + 1
            b2 = np.where(b2 > 0, b2, 0.0)
        if steps < n_comps:
            if broke.size:
                raise ValueError('the Krylov space of the start vector has %d dimensions, fewer than n_comps' % steps)
            continue
        theta, S, res = _ritz(a[:steps], np.sqrt(b2[:steps]), n_comps)
        converged = bool((res <= tol).all())
        if converged or broke.size:
            break
    out = basis_combine(Q, n, steps, torch.as_tensor(S).to(dev), blocks=blocks)
    psi = out[:, :n].t().contiguous()
    mag = psi.abs()
    first = torch.where(mag == mag.max(0).values, torch.arange(n, device=dev)[:, None], n).min(0).values
    sign = torch.where(psi.gather(0, first[None, :]) < 0, -1.0, 1.0).to(torch.float64)
    return {'eigenvalues': theta, 'components': psi * sign, 'residuals': res, 'steps': steps, 'converged': converged}


def diffusion_pseudotime(eigenvalues, components, root):
    """Diffusion pseudotime from the cell `root` (Haghverdi et al. 2016): dpt(i) = sqrt(sum over l >= 1 with lambda_l < 1 of
    (lambda_l / (1 - lambda_l))^2 (psi_l(i) - psi_l(root))^2), the terms added for l ascending in float64, each formed as
    ((lambda_l / (1 - lambda_l))^2) * (d * d) with every product rounded: torch on the device of `components`, one small step per
    term, no reduction whose order is open.  eigenvalues (m,), components (n, m) as diffusion_map() returns them.  Returns
    {'dpt': (n,) float64, 'pseudotime': dpt / max dpt (dpt itself where that is 0)}."""
    lam = np.asarray(eigenvalues, dtype=np.float64)
    if not isinstance(components, torch.Tensor) or components.dtype != torch.float64 or components.dim() != 2 or lam.ndim != 1 \
            or int(components.shape[1]) != lam.size:
        raise ValueError('eigenvalues must be (m,) and components an (n, m) float64 torch tensor')
    n = int(components.shape[0])
    if isinstance(root, bool) or not isinstance(root, (int, np.integer)) or not 0 <= int(root) < n:
        raise ValueError('root must be a cell index within [0, %d)' % n)
    acc = torch.zeros(n, dtype=torch.float64, device=components.device)
    for l in range(1, lam.size):
        if not lam[l] < 1.0:
            continue
        wl = lam[l] / (1.0 - lam[l])
        d = components[:, l] - components[int(root), l]
        acc = acc + (d * d) * float(wl * wl)
    dpt = torch.sqrt(acc)
    top = dpt.max() if n else None
    return {'dpt': dpt, 'pseudotime': dpt / top if n and float(top) > 0 else dpt.clone()}


# ---- Harmony batch correction (csrc/harmony.hip) --------------------------------------------------------------
def harmony_max_clusters(d):
    """The largest number of clusters harmony() serves at feature width d (0: d is not served)."""
    return int(_lib.load().oriana_harmony_max_clusters(int(d)))


def harmony_max_batches():
    return int(_lib.load().oriana_harmony_max_batches())


def harmony_partial_rows():
    """Rows of one batch that harmony_moments() adds in float32 before the sum is promoted to float64."""
    return int(_lib.load().oriana_harmony_partial_rows())


def harmony_default_clusters(n):
    """harmonypy's default: min(round(n / 30), 100), at least 1 (halves round up)."""
    return max(1, min(int(math.floor(n / 30.0 + 0.5)), 100))


def harmony_block_cuts(n, n_blocks=20):
    """The row cuts of the blocks of a round: block j is the permuted rows [cuts[j], cuts[j + 1]), min(n_blocks, n) blocks."""
    nb = min(int(n_blocks), int(n))
    return [(j * int(n)) // nb for j in range(nb + 1)]


def _harmony_rows(X, R, batch, what):
    """(n, d, K, row stride) of float32 rows X, their responsibilities R (n, K) and batches (n,) int32, checked."""
    _check_rows(X, what)
    n, ld = _rows_ld(X)
    d = int(X.shape[1])
    if not isinstance(R, torch.Tensor) or R.dim() != 2 or R.dtype != torch.float32 or not R.is_contiguous() or int(R.shape[0]) != n:
        raise ValueError('R must be a contiguous float32 (n, K) tensor with the rows of %s' % what)
    if not isinstance(batch, torch.Tensor) or batch.dtype != torch.int32 or tuple(batch.shape) != (n,) or not batch.is_contiguous():
        raise ValueError('batch must be a contiguous int32 (n,) tensor')
    if d < 1 or int(R.shape[1]) < 1:
        raise ValueError('%s and R need at least one column' % what)
    return n, d, int(R.shape[1]), ld


def _harmony_out(t, shape, dtype, device, what):
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError('%s must be a contiguous %s tensor of shape %s' % (what, dtype, tuple(shape)))
    return t


def harmony_assign(Zcos, batch, centers, P, inv_sigma, R, rows=None, blocks=0, scratch=None, O_blk=None, sums=None):
    """One oriana_harmony_assign: the responsibilities of the rows [rows[0], rows[1]) of Zcos (n, d) float32 (default: all) under
    centers (K, d) float32 and the penalty table P (K, B) float32, written into those rows of R (n, K) float32; batch (n,) int32.
    Returns (O_blk (K, B), sums (2,)) float64 device tensors of the range: the responsibilities per cluster and batch, and
    sum R dist, sum R log R."""
    n, d, K, ld = _harmony_rows(Zcos, R, batch, 'Zcos')
    if (centers.dtype != torch.float32 or P.dtype != torch.float32 or not centers.is_contiguous() or not P.is_contiguous()
            or tuple(centers.shape) != (K, d) or P.dim() != 2 or int(P.shape[0]) != K or int(P.shape[1]) < 1):
        raise ValueError('harmony_assign needs contiguous float32 centers (K, d) and P (K, B)')
    B = int(P.shape[1])
    a, b = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= a <= b <= n:
        raise ValueError('rows must be a range within [0, %d]' % n)
    if not (float(inv_sigma) > 0 and math.isfinite(float(inv_sigma))):
        raise ValueError('inv_sigma must be finite and positive')
    dev = R.device
    m = b - a
    nbytes = _scratch_bytes('oriana_harmony_assign_scratch_bytes', m, d, K, B, int(blocks))
    scratch = _scratch_for(scratch, nbytes, dev)
    O_blk = _harmony_out(O_blk, (K, B), torch.float64, dev, 'O_blk')
    sums = _harmony_out(sums, (2,), torch.float64, dev, 'sums')
    call('oriana_harmony_assign', ptr(Zcos) + 4 * a * ld if m else None, m, d, ld, ptr(batch) + 4 * a if m else None, ptr(centers), K,
         ptr(P), B, float(inv_sigma), ptr(R) + 4 * a * K if m else None, ptr(O_blk), ptr(sums), ptr(scratch), int(blocks), stream_ptr())
    return O_blk, sums


def harmony_moments(X, R, batch, n_batches, blocks=0, scratch=None, S=None, O=None):
    """One oriana_harmony_moments: S[k, b, :] = sum_{batch_i = b} R_ik x_i (K, B, d) and O[k, b] = sum_{batch_i = b} R_ik (K, B),
    float64 device tensors, from X (n, d) float32, R (n, K) float32 and batch (n,) int32."""
    n, d, K, ld = _harmony_rows(X, R, batch, 'X')
    B = int(n_batches)
    if B < 1:
        raise ValueError('n_batches must be at least 1')
    dev = R.device
    nbytes = _scratch_bytes('oriana_harmony_moments_scratch_bytes', n, d, K, B, int(blocks))
    scratch = _scratch_for(scratch, nbytes, dev)
    S = _harmony_out(S, (K, B, d), torch.float64, dev, 'S')
    O = _harmony_out(O, (K, B), torch.float64, dev, 'O')
    call('oriana_harmony_moments', ptr(X) if n else None, n, d, ld, ptr(R) if n else None, K, ptr(batch) if n else None, B, ptr(S),
         ptr(O), ptr(scratch), int(blocks), stream_ptr())
    return S, O


def harmony_correct(Z, R, batch, W, blocks=0, scratch=None, Zcorr=None, Zcos=None):
    """One oriana_harmony_correct: Zcorr = Z - sum_k R_ik W[k, batch_i, :] and its cosine-normalised rows Zcos, (n, d) float32
    device tensors, from Z (n, d) float32, R (n, K) float32, batch (n,) int32 and W (K, B, d) float32."""
    n, d, K, ld = _harmony_rows(Z, R, batch, 'Z')
    if W.dtype != torch.float32 or not W.is_contiguous() or W.dim() != 3 or int(W.shape[0]) != K or int(W.shape[2]) != d or int(W.shape[1]) < 1:
        raise ValueError('harmony_correct needs a contiguous float32 W (K, B, d)')
    B = int(W.shape[1])
    dev = R.device
    nbytes = _scratch_bytes('oriana_harmony_correct_scratch_bytes', n, d, K, B, int(blocks))
    scratch = _scratch_for(scratch, nbytes, dev)
    Zcorr = _harmony_out(Zcorr, (n, d), torch.float32, dev, 'Zcorr')
    Zcos = _harmony_out(Zcos, (n, d), torch.float32, dev, 'Zcos')
    call('oriana_harmony_correct', ptr(Z) if n else None, n, d, ld, ptr(R) if n else None, K, ptr(batch) if n else None, ptr(W), B,
         ptr(Zcorr) if n else None, ptr(Zcos) if n else None, ptr(scratch), int(blocks), stream_ptr())
    return Zcorr, Zcos


def harmony_ridge_weights(S, O, ridge):
    """The closed form of harmonypy's per-cluster ridge system with an unpenalised intercept, elementwise in float64: from
    S (K, B, d), O (K, B) and ridge (B,) > 0 (torch tensors on one device), W (K, B, d) with
    w0 = sum_b l_b S_b / (O_b + l_b) / sum_b l_b O_b / (O_b + l_b) and W_kb = (S_b - O_b w0) / (O_b + l_b); 0 where the
    denominator of w0 is 0.  The intercept w0 is not returned."""
    den = O + ridge[None, :]
    g = ridge[None, :] / den                                        # (K, B)
    num = (g[:, :, None] * S).sum(1)                                # (K, d)
    c = (g * O).sum(1)                                              # (K,)
    ok = c > 0
    w0 = num / torch.where(ok, c, torch.ones_like(c))[:, None]
    W = (S - O[:, :, None] * w0[:, None, :]) / den[:, :, None]
    return torch.where(ok[:, None, None], W, torch.zeros_like(W))


def _harmony_vector(v, B, what, positive):
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(B, float(a))
    if a.shape != (B,) or not np.isfinite(a).all() or (positive and not (a > 0).all()) or (not positive and (a < 0).any()):
        raise ValueError('%s must be a %s scalar or (%d,) vector' % (what, 'positive' if positive else 'non-negative', B))
    return a


def harmony(Y, batch, n_clusters=None, theta=2.0, sigma=0.1, ridge=1.0, n_blocks=20, max_iter=10, max_rounds=20, eps_cluster=1e-5,
            eps_harmony=1e-4, centers=None, seed=0, blocks=0, pg=None):
    """Harmony batch correction (Korsunsky et al. 2019; harmonypy's algorithm) of the rows of Y, an (n, d) float32 C-contiguous
    device tensor, given batch (n,) integers within [0, B) with every batch present.  DESIGN.md section 5r defines every step.

    The two deliberate differences from harmonypy, both for determinism: ONE permutation ``torch.randperm(n, generator=
    manual_seed(seed))`` per run, whose min(n_blocks, n) blocks every round visits in ascending order (harmonypy reshuffles every
    round); and the ridge correction in closed form (harmony_ridge_weights) instead of a matrix inverse per cluster.

    theta, ridge : scalars or (B,) vectors (theta >= 0, ridge > 0); sigma > 0.  n_clusters : default harmony_default_clusters(n).
    centers : optional (K, d) start centres (their rows are normalised), else kmeans(Zcos, K, n_init=10, max_iter=25, seed=seed).
    eps_cluster : a round's stopping rule, from the fifth round of an iteration on: (old - new) / |old| < eps_cluster with old /
    new the sums of the three objectives before the last one / the last three; None: exactly max_rounds rounds.  eps_harmony :
    iterations stop when the last objectives of two successive iterations differ by less than eps_harmony relatively; None: all
    max_iter iterations.  Between the block launches only small float64 device operations on (K, B) run; the host reads the
    round objectives once per round from the fifth round on and once per iteration.

    Returns a dict: 'corrected' (n, d) float32, 'responsibilities' (n, K) float32 and 'centers' (K, d) float32 device tensors in
    the caller's row order; 'objective' (the start first, then one per iteration), 'objective_rounds' (every round of every
    iteration), 'rounds' (per iteration), 'n_iter', 'converged', 'batch_sizes' (B,) int64 NumPy.
    ValueError before any launch for arguments out of range, a batch that occurs nowhere, a non-finite entry or a zero row;
    NotImplementedError for a process group of more than one rank."""
    if odist.world_size(pg) > 1:
        raise NotImplementedError('harmony() does not shard its rows: gather the features on one rank')
    if not isinstance(Y, torch.Tensor) or Y.dim() != 2:
        raise ValueError('Y must be a 2-D torch tensor')
    if Y.dtype != torch.float32:
        raise ValueError('Y must be float32, got %s' % Y.dtype)
    if not Y.is_contiguous():
        raise ValueError('Y must be C-contiguous')
    n, d = int(Y.shape[0]), int(Y.shape[1])
    if n < 1 or d < 1:
        raise ValueError('Y needs at least one row and one column')
    bh = batch.detach().cpu().numpy() if isinstance(batch, torch.Tensor) else np.asarray(batch)
    if bh.ndim != 1 or bh.shape[0] != n or bh.dtype.kind not in 'iu':
        raise ValueError('batch must be (n,) integers')
    bh = bh.astype(np.int64)
    if bh.min() < 0:
        raise ValueError('batch must be non-negative')
    B = int(bh.max()) + 1
    if B > harmony_max_batches():
        raise ValueError('%d batches are beyond the %d served' % (B, harmony_max_batches()))
    sizes = np.bincount(bh, minlength=B).astype(np.int64)
    if (sizes == 0).any():
        raise ValueError('batch %d occurs nowhere: number the batches 0 .. B - 1' % int(np.nonzero(sizes == 0)[0][0]))
    K = harmony_default_clusters(n) if n_clusters is None else int(n_clusters)
    if K < 1 or K > n:
        raise ValueError('n_clusters must lie within [1, n]')
    if d > 256 or K > harmony_max_clusters(d):
        raise ValueError('n_clusters = %d is beyond the %d served at %d features' % (K, harmony_max_clusters(d) if d <= 256 else 0, d))
    th = _harmony_vector(theta, B, 'theta', False)
    lam = _harmony_vector(ridge, B, 'ridge', True)
    sigma = float(sigma)
    if not (sigma > 0 and math.isfinite(sigma)):
        raise ValueError('sigma must be finite and positive')
    n_blocks, max_iter, max_rounds, blocks = int(n_blocks), int(max_iter), int(max_rounds), int(blocks)
    if n_blocks < 1 or max_iter < 1 or max_rounds < 1 or blocks < 0:
        raise ValueError('n_blocks >= 1, max_iter >= 1, max_rounds >= 1 and blocks >= 0 are required')
    for e, what in ((eps_cluster, 'eps_cluster'), (eps_harmony, 'eps_harmony')):
        if e is not None and not float(e) >= 0:
            raise ValueError('%s must be None or non-negative' % what)
    c0 = None
    if centers is not None:
        c0 = np.asarray(centers.detach().cpu() if isinstance(centers, torch.Tensor) else centers, dtype=np.float64)
        if c0.shape != (K, d) or not np.isfinite(c0).all() or not (np.abs(c0).sum(1) > 0).all():
            raise ValueError('centers must be finite non-zero rows of shape (n_clusters, d) = %s' % ((K, d),))
    if c0 is None and K > max_centers(d):
        raise ValueError('the k-means start serves %d clusters at %d features: pass centers= for n_clusters = %d' % (max_centers(d), d, K))
    ok = torch.isfinite(Y).all() & (Y != 0).any(dim=1).all()
    if not bool(ok.item()):
        raise ValueError('Y has non-finite entries or a zero row (cosine normalisation of a zero row is undefined)')
    if not Y.is_cuda:
        raise ValueError('Y must be a device tensor')

    dev = Y.device
    f64 = torch.float64
    g = torch.Generator()
    g.manual_seed(int(seed))
    perm = torch.randperm(n, generator=g).to(dev)
    Z = Y.index_select(0, perm).contiguous()
    bt = torch.as_tensor(bh[perm.cpu().numpy()].astype(np.int32), device=dev)
    cuts = harmony_block_cuts(n, n_blocks)
    nb = len(cuts) - 1
    Pr = torch.as_tensor(sizes / float(n), dtype=f64, device=dev)
    th_d, lam_d = torch.as_tensor(th, dtype=f64, device=dev), torch.as_tensor(lam, dtype=f64, device=dev)
    inv_sigma = 1.0 / sigma
    lib = _lib.load()
    sc_assign = _scratch_for(None, max(int(lib.oriana_harmony_assign_scratch_bytes(m, d, K, B, blocks))
                                       for m in {cuts[j + 1] - cuts[j] for j in range(nb)}), dev)
    sc_moments = _scratch_for(None, _scratch_bytes('oriana_harmony_moments_scratch_bytes', n, d, K, B, blocks), dev)
    sc_correct = _scratch_for(None, _scratch_bytes('oriana_harmony_correct_scratch_bytes', n, d, K, B, blocks), dev)

    R = torch.zeros(n, K, dtype=torch.float32, device=dev)
    # the cosine-normalised rows: the correction with W = 0
    _, Zcos = harmony_correct(Z, R, bt, torch.zeros(K, B, d, dtype=torch.float32, device=dev), blocks=blocks, scratch=sc_correct)
    Zcorr = Z
    if c0 is None:
        c0 = np.asarray(kmeans(Zcos, K, n_init=10, max_iter=25, seed=seed)['centers'], dtype=np.float64)
        if not (np.abs(c0).sum(1) > 0).all():
            raise ValueError('k-means returned a zero centre')
    c0 = c0 / np.sqrt((c0 * c0).sum(1, keepdims=True))
    cen64 = torch.as_tensor(c0, dtype=f64, device=dev)
    cen = cen64.to(torch.float32)

    O_blk = torch.zeros(nb, K, B, dtype=f64, device=dev)
    sums = torch.zeros(nb, 2, dtype=f64, device=dev)
    ones = torch.ones(K, B, dtype=torch.float32, device=dev)

    def assign(j, P):
        harmony_assign(Zcos, bt, cen, P, inv_sigma, R, rows=(cuts[j], cuts[j + 1]), blocks=blocks, scratch=sc_assign,
                       O_blk=O_blk[j], sums=sums[j])

    def objective(O, E):
        return sums[:, 0].sum() + sigma * sums[:, 1].sum() + sigma * (th_d[None, :] * O * torch.log((O + 1.0) / (E + 1.0))).sum()

    for j in range(nb):
        assign(j, ones)
    O = O_blk.sum(0)
    E = O.sum(1)[:, None] * Pr[None, :]
    obj_iter = [float(objective(O, E).item())]
    obj_rounds, rounds = [], []
    converged = False
    n_iter = 0
    for it in range(max_iter):
        robj = []
        nr = 0
        while nr < max_rounds:
            S, _ = harmony_moments(Zcos, R, bt, B, blocks=blocks, scratch=sc_moments)
            C = S.sum(1)
            cn = torch.sqrt((C * C).sum(1, keepdim=True))
            cen64 = torch.where(cn > 0, C / torch.where(cn > 0, cn, torch.ones_like(cn)), cen64)
            cen = cen64.to(torch.float32)
            for j in range(nb):
                O = O - O_blk[j]
                E = E - O_blk[j].sum(1)[:, None] * Pr[None, :]
                P = torch.pow((E + 1.0) / (O + 1.0), th_d[None, :]).to(torch.float32)
                assign(j, P)
                O = O + O_blk[j]
                E = E + O_blk[j].sum(1)[:, None] * Pr[None, :]
            robj.append(objective(O, E))
            nr += 1
            if eps_cluster is not None and nr >= 5:
                h = torch.stack(robj[-4:]).cpu().numpy()              # (the one host read of the round)
                old, new = float(h[0] + h[1] + h[2]), float(h[1] + h[2] + h[3])
                if (old - new) / abs(old) < float(eps_cluster):
                    break
        h = [float(v) for v in torch.stack(robj).cpu().numpy()]
        obj_rounds.extend(h)
        rounds.append(nr)
        obj_iter.append(h[-1])
        S, Om = harmony_moments(Z, R, bt, B, blocks=blocks, scratch=sc_moments)
        W = harmony_ridge_weights(S, Om, lam_d).to(torch.float32)
        Zcorr, Zcos = harmony_correct(Z, R, bt, W, blocks=blocks, scratch=sc_correct)
        n_iter = it + 1
        if eps_harmony is not None and abs(obj_iter[-2] - obj_iter[-1]) / abs(obj_iter[-2]) < float(eps_harmony):
            converged = True
            break
    corrected = torch.empty_like(Zcorr)
    corrected[perm] = Zcorr
    resp = torch.empty_like(R)
    resp[perm] = R
    return {'corrected': corrected, 'responsibilities': resp, 'centers': cen, 'objective': obj_iter, 'objective_rounds': obj_rounds,
            'rounds': rounds, 'n_iter': n_iter, 'converged': converged, 'batch_sizes': sizes}
