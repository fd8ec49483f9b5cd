# -*- coding: utf-8 -*-
"""k-means on the device: all restarts of a run advance together through oriana_kmeans_step (csrc/kmeans.hip), which reads a row
tile once for a group of restarts and emits only per-cluster sums.  The reference's pipeline ends in
``KMeans(n_clusters, n_init=100).fit(np.log(U))`` (experiments/clustering.py); this is that step without the host copy.
DESIGN.md section 5i."""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from . import dist as odist

__all__ = ['kmeans', 'lloyd_step', 'max_centers', 'restart_group', 'partial_rows', 'tile_rows', 'draws', 'distinct_rows']

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
        else:
            self.row0, self.N = 0, self.n

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
