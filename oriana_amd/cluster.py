# -*- coding: utf-8 -*-
"""k-means on the device: all restarts of a run advance together through oriana_kmeans_step (csrc/kmeans.hip), which reads a row
tile once for a group of restarts and emits only per-cluster sums.  The reference's pipeline ends in
``KMeans(n_clusters, n_init=100).fit(np.log(U))`` (experiments/clustering.py); this is that step without the host copy.
DESIGN.md section 5i.

knn() is the exact k-nearest-neighbour graph of the same rows through oriana_knn (csrc/knn.hip): brute force, no distance
matrix, results independent of every partition of the work.  DESIGN.md section 5j."""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from . import dist as odist

__all__ = ['kmeans', 'lloyd_step', 'max_centers', 'restart_group', 'partial_rows', 'tile_rows', 'draws', 'distinct_rows',
           'knn', 'knn_plan', 'knn_step', 'max_neighbors']

SCRATCH_BUDGET = 1 << 30          # bytes a launch may take for scratch, minimum distances and their cumulative sums


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
    lib = _lib.load()
    nbytes = int(lib.oriana_kmeans_scratch_bytes(n, d, C, R, int(blocks)))
    if nbytes < 0:
        raise _lib.OrianaHipError('oriana_kmeans_scratch_bytes failed with code %d' % nbytes)
    out = {'sums': torch.empty(R, C, d, dtype=torch.float64, device=dev),
           'counts': torch.empty(R, C, dtype=torch.int64, device=dev),
           'inertia': torch.empty(R, dtype=torch.float64, device=dev)}
    labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if label_restart is not None else None
    mind = torch.empty(R, max(n, 1), dtype=torch.float32, device=dev) if want_mind else None
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
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
    finite = torch.isfinite(Y).all().to(torch.float64).reshape(1)
    if odist.sharded(pg):
        finite = 1.0 - finite
        odist.all_reduce_sum(finite, pg)
        finite = 1.0 - finite.clamp(max=1.0)
    if not bool(finite.item()):
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
    nbytes = int(_lib.load().oriana_knn_scratch_bytes_for(nq, n, d, k, int(blocks), y_ptr, ldy))
    if nbytes < 0:
        raise _lib.OrianaHipError('oriana_knn_scratch_bytes_for failed with code %d' % nbytes)
    return nbytes


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
    budget = SCRATCH_BUDGET if budget is None else int(budget)
    ldy = d if ldy is None else int(ldy)
    tile = int(_lib.load().oriana_knn_tile_rows())

    def need(qb, c):
        sizes = {min(qb, nq)} | ({nq % qb} if nq > qb else set())
        return max(_knn_scratch_bytes(b, min(c, n), d, k, blocks, y_ptr, ldy) for b in sizes)

    chunk = int(candidate_chunk) if candidate_chunk is not None else max(n, 1)
    qb = int(query_block) if query_block is not None else max(nq, 1)
    if candidate_chunk is None:
        while chunk > 1 and need(tile, chunk) > budget // 2:
            chunk = (chunk + 1) // 2
    if query_block is None:
        while qb > tile and need(qb, chunk) > budget:
            qb = max(tile, -(-qb // (2 * tile)) * tile)
    return qb, chunk, need(qb, chunk)


def knn_step(Q, Y, idx, d2, q0=0, y0=0, exclude_self=False, merge=False, blocks=0, scratch=None):
    """One oriana_knn call: the rows of Q (nq, d) against the candidates Y (n, d), both float32 device tensors (row stride >= d,
    unit column stride) whose first rows have the global indices q0 and y0; idx (nq, k) int32 and d2 (nq, k) float32, contiguous,
    are written, or with `merge` merged with what they hold."""
    nq, ldq = _rows_ld(Q)
    n, ldy = _rows_ld(Y)
    d, k = int(Q.shape[1]), int(idx.shape[1])
    nbytes = _knn_scratch_bytes(nq, n, d, k, blocks, ptr(Y) if n else None, ldy)
    if scratch is None:
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=idx.device)
    elif scratch.numel() * scratch.element_size() < nbytes:            # (oriana_knn itself takes no size: it would write past it)
        raise ValueError('the scratch holds %d bytes, this call needs %d' % (scratch.numel() * scratch.element_size(), nbytes))
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
    if blocks < 0 or (candidate_chunk is not None and int(candidate_chunk) < 1) or (query_block is not None and int(query_block) < 1):
        raise ValueError('blocks >= 0, candidate_chunk >= 1 and query_block >= 1 are required')
    kmax = max_neighbors(d) if d >= 1 else 0
    if kmax == 0:
        raise ValueError('%d features are not served' % d)
    if k > kmax:
        raise ValueError('n_neighbors = %d is beyond the %d served at %d features' % (k, kmax, d))
    if not Y.is_cuda or (queries is not None and queries.device != Y.device):
        raise ValueError('Y and queries must be tensors of one device')
    finite = torch.isfinite(Y).all() if queries is None else torch.isfinite(Y).all() & torch.isfinite(queries).all()
    finite = finite.to(torch.float64).reshape(1)
    if odist.sharded(pg):
        finite = 1.0 - finite
        odist.all_reduce_sum(finite, pg)
        finite = 1.0 - finite.clamp(max=1.0)
    if not bool(finite.item()):
        raise ValueError('Y or queries have non-finite entries')
    rows = _Rows(Y, pg)
    if rows.N > 2 ** 31 - 1:
        raise ValueError('%d rows are beyond the int32 indices' % rows.N)

    dev = Y.device
    Q, q0 = (Y, rows.row0) if queries is None else (queries, 0)
    nq = int(Q.shape[0])
    # the shards arrive in contiguous buffers of their own; without sharding the candidates are Y as it lies
    y_ptr, ldy = (16, d) if odist.sharded(pg) else (ptr(Y) if n else None, _rows_ld(Y)[1])
    qb, chunk, nbytes = knn_plan(nq, max(rows.sizes), d, k, blocks, y_ptr, ldy, candidate_chunk, query_block)
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
    d2 = torch.empty(nq, k, dtype=torch.float32, device=dev)
    merge = False
    y0 = 0
    for s, ns in enumerate(rows.sizes):
        if odist.sharded(pg):
            # shard s on every rank: a zero buffer to which its owner adds its rows, summed over the ranks (exact)
            cand = torch.zeros(ns, d, dtype=torch.float32, device=dev)
            if s == rows.rank and ns:
                cand.copy_(Y)
            odist.all_reduce_sum(cand, pg)
        else:
            cand = Y
        for a in range(0, ns, chunk):
            for b in range(0, nq, qb):
                knn_step(Q[b:b + qb], cand[a:a + chunk], idx[b:b + qb], d2[b:b + qb], q0=q0 + b, y0=y0 + a,
                         exclude_self=exclude_self, merge=merge, blocks=blocks, scratch=scratch)
            merge = True
        y0 += ns
    if not merge:                                     # (no candidates at all: the padding values)
        knn_step(Q, Y[:0], idx, d2, q0=q0, blocks=blocks)
    return {'indices': idx, 'sq_distances': d2}
