# -*- coding: utf-8 -*-
"""Cells the model was not fitted on: folding them into a fitted gene side (fold_in, fold_in_zi) and each cell's share of the
variational bound (cell_bounds, zi_cell_bounds), and -- a streaming fit's global step, GaP.partial_fit -- a folded-in batch's
per-gene statistics and their blend into the gene side (gene_statistics, svi_gene_update; for ZIGaP.fold_in_fit the dropout-weighted
rate statistic beside them, zi_gene_rate), on a ZWorkspace of the call's own.  This module calls into the sweep sequencer of
engine.py (the row phase: zq_rows_open, plain or -- S_tilde, S_hat given: the sparse models' project() -- masked); nothing in a
sweep calls back."""
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .engine import ZWorkspace, _span, factor_prep, zq, zq_rows_open
from .nodes import gamma_expectations

_F32, _F64 = torch.float32, torch.float64


def _operand(name, t, dtype, shape):
    """TypeError unless `t` is a C-contiguous device tensor of this dtype and shape (ValueError: a float32 factor's shape alone)."""
    kind = isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous()
    if not (kind and tuple(t.shape) == tuple(shape)):
        raise (ValueError if kind and dtype == _F32 else TypeError)(
            '%s must be a C-contiguous %s %s device tensor' % (name, tuple(shape), str(dtype).split('.')[-1]))


def row_sums_over_k(ws, K):
    """rowsum(x) / K per cell and factor, (n, K) float32 in the caller's row order: the row pass against all-ones factors
    (uniform responsibilities: s = x / K, R = sum_j s), completed as the sweeps complete Z_i."""
    ct = ws.ct
    ones_u, ones_v = ws.extra('ONE_U', ct.n), ws.extra('ONE_V', ct.m)
    ones_u[:, :K] = 1.0
    ones_v[:, :K] = 1.0
    Z = torch.zeros(max(ct.n, 1), K, dtype=_F32, device=ct.device)
    ws.tile_flag.zero_()
    st = stream_ptr()
    call('oriana_row_pass', ct.sparse_struct, ptr(ones_u), ptr(ones_v), None, ptr(ws.R), ptr(ws.s_cs), None, None,
         ptr(ws.tile_flag), K, st)
    call('oriana_finalize_slabs_from', ptr(Z), ptr(ones_u), ptr(ws.R), 1, 0, ptr(ct.row_perm), ct.n, K, st)
    return Z[:ct.n]


def masked_row_sums(ws, K, S_tilde, S_hat):
    """sum_j x_ij S_hat_jk S_tilde_jk / max(1, sum_k S_tilde_jk) per cell and factor, (n, K) float32 in the caller's row order: the
    sparse row phase of a sweep against E[log U] = E[log V] = 0 (responsibilities uniform over a gene's unmasked factors; a
    fully masked gene gives nothing).  rowsum(x) / K -- row_sums_over_k -- when nothing is masked and S_hat = 1."""
    ct = ws.ct
    f32 = dict(dtype=_F32, device=ct.device)
    Z, Zj = torch.zeros(max(ct.n, 1), K, **f32), torch.zeros(max(ct.m, 1), K, **f32)
    ws.fu_pending = False
    zq(ws, Z[:ct.n], Zj[:ct.m], None, torch.zeros(ct.n, K, **f32), torch.zeros(ct.m, K, **f32), S_tilde=S_tilde, S_hat=S_hat,
       phase='rows')
    return Z[:ct.n]


def _padded_genes(ct, K, V_hat, pi_d):
    """What the zero-inflated kernels read per gene, padded to a multiple of 4 genes with inert ones (no counts, V_hat row 0,
    pi_d 0, as _padG of models/zigap.py), and the query's own non-zero mask from its packed counts: (mp, Vp, pip, nzmask)."""
    n, m, dev = ct.n, ct.m, ct.device
    mp = (m + 3) // 4 * 4
    if mp != m:
        Vp, pip = torch.zeros(mp, K, dtype=_F64, device=dev), torch.zeros(mp, dtype=_F64, device=dev)
        Vp[:m].copy_(V_hat)
        pip[:m].copy_(pi_d)
    else:
        Vp, pip = V_hat, pi_d
    nzmask = torch.zeros(((n + 31) // 32) * mp, dtype=torch.int32, device=dev)
    call('oriana_nzmask_counts', ptr(nzmask), ct.sparse_struct, mp, stream_ptr())
    return mp, Vp, pip, nzmask


def _fold_in_buffers(ws, n_iter):
    """What a fold-in loop keeps beside the shapes: the workspace set up for in-place factor preparation, and (E[log U], Z_i,
    Z_j, the active bytes, one counter of active cells per iteration)."""
    ct, K = ws.ct, ws.K
    n, m, dev = ct.n, ct.m, ct.device
    f32 = dict(dtype=_F32, device=dev)
    # the cell side of every factor preparation comes from oriana_foldin_update (the fused form of factor_prep_pair), in
    # place: no kernel reads FU while it is rewritten, so the double buffer of the sweeps is one buffer here
    ws.prep_blocks = int(_lib.load().oriana_foldin_update_blocks(n))
    ws.FU_alt = ws.FU
    ws.mu_u = torch.zeros(n, **f32)
    ws.upart = torch.zeros(4 * ws.prep_blocks, **f32)
    lu = torch.empty(n, K, **f32)
    Zi, Zj = torch.empty(n, K, **f32), torch.empty(max(m, 1), K, **f32)       # (Z_j: the slow path adds into it; never read)
    active = torch.ones(n, dtype=torch.uint8, device=dev)
    left = torch.zeros(max(n_iter, 1), dtype=torch.int32, device=dev)        # one counter per iteration: no clearing launch
    return lu, Zi, Zj, active, left


def _drive(ct, K, log_V_hat, n_iter, tol, check_every, ws, operands, launches):
    """The fold-in loop of both models.  `operands`: (name, tensor, dtype, shape) beside log_V_hat, checked first.
    `launches(ws, tol)`: the model's own set-up, run once the workspace exists; returns start(lu, active), the launch that forms
    E[log U] and the first FU from the starting shapes, and step(it, rows, ...), the launches of iteration `it`: it calls
    rows(), or rows(S_tilde, S_hat, active) for the masked row phase of the sparse models, where the row phase of the sweep
    belongs (ws.rows_nslab then says how many slabs of R it filled) and ends with the update launch that counts the cells still
    active into n_active."""
    if ct.gd:
        raise ValueError('fold_in walks the sliced layout only: pack the new counts without dense_density')
    n, m, dev = ct.n, ct.m, ct.device
    n_iter, check_every, tol = int(n_iter), int(check_every), float(tol)
    if n_iter < 0 or check_every < 1 or not tol >= 0.0:
        raise ValueError('fold_in needs n_iter >= 0, check_every >= 1 and tol >= 0')
    for name, t, dtype, shape in (('log_V_hat', log_V_hat, _F32, (m, K)),) + tuple(operands):
        _operand(name, t, dtype, shape)
    froze_at = torch.full((n,), n_iter, dtype=torch.int32, device=dev)
    if n == 0:
        return froze_at, 0, 0
    if ws is None:
        ws = ZWorkspace(ct, K)
    start, step = launches(ws, tol)
    lu, Zi, Zj, active, left = _fold_in_buffers(ws, n_iter)
    start(lu, active)
    def rows(S_tilde=None, S_hat=None, active=None):
        ws.fu_pending, ws.fu_source = True, lu.data_ptr()
        zq_rows_open(ws, Zi, Zj, lu, log_V_hat, S_tilde=S_tilde, S_hat=S_hat, active=active)
    n_left, done = n, 0
    for it in range(n_iter):
        step(it, rows, lu, Zi, active, froze_at, ptr(left) + 4 * it)
        done = it + 1
        if done % check_every == 0 or done == n_iter:
            n_left = int(left[it].item())
            if n_left == 0:
                break
    return froze_at, n_left, done


def _masks(m, K, S_tilde, S_hat):
    """The operands of the masked row phase as _drive checks them: none, or both (m, K) float32."""
    if (S_tilde is None) != (S_hat is None):
        raise ValueError('S_tilde and S_hat go together')
    return () if S_hat is None else (('S_tilde', S_tilde, _F32, (m, K)), ('S_hat', S_hat, _F32, (m, K)))


def fold_in(ct_new, K, log_V_hat, alpha1, a2_row, a1, n_iter, tol, check_every=5, ws=None, S_tilde=None, S_hat=None):
    """Fold the cells of `ct_new` (CountTiles, sliced layout) into a fitted pCMF model whose gene side stays as it is: the
    per-cell fixed point of  a1 <- max(1e-15, alpha1 + sum_j x_ij r_ijk),  r_ij. = softmax_k(E[log U]_ik + E[log V]_jk),
    E[log U] = psi(a1) - log a2_row  (gap.py:97-102 with sum_j V_hat frozen).  `a1` (n', K) float64 device tensor: the start,
    updated in place; log_V_hat (m, K) float32, alpha1 / a2_row [K] float64: the model's, only read.
    Each iteration is the row phase of a sweep on a workspace of this call's own (zq_gap(phase='rows', finalize_rows=False):
    validity test + gene-side factor from log_V_hat through the new tiles' gene order, row pass, slow path) and ONE launch of
    oriana_foldin_update, which completes Z_i, updates a1 / E[log U], freezes the cells that moved by at most tol * a1 and
    prepares the next row pass's FU in place.  The host reads the number of active cells every `check_every` iterations
    and stops at zero.
    S_tilde, S_hat (m, K) float32 (SparseGaP.project(): log_V_hat is then E[log V'], a2_row = alpha2 + sum_j S_hat V'_hat): the
    row phase is the sparse models' -- e_ijk = exp(lu + lv) S_tilde_jk, sums weighted with S_hat_jk, sparse_gap.py:81-97 -- the
    two-image row pass for Kp <= 64, else the s_rs pass and oriana_row_spmm_active over the cells still active; only read.
    Returns (froze_at int32 [n'] -- the 0-based iteration a cell froze at, n_iter if never --, the number
    of cells still active, the iterations run)."""
    n = ct_new.n
    def launches(ws, tol):
        st, perm = stream_ptr(), ptr(ct_new.row_perm)
        def start(lu, active):
            call('oriana_foldin_update', ptr(a1), ptr(lu), ptr(active), None, None, None, ptr(a2_row), None, None, None, 1, 0,
                 perm, n, K, tol, 0, ptr(ws.FU), ptr(ws.mu_u), ptr(ws.upart), st)
        def step(it, rows, lu, Zi, active, froze_at, n_active):
            rows() if S_hat is None else rows(S_tilde, S_hat, active)
            with _span(ws, 'foldin_update'):
                call('oriana_foldin_update', ptr(a1), ptr(lu), ptr(active), ptr(froze_at), n_active, ptr(alpha1), ptr(a2_row),
                     ptr(Zi), ptr(ws.FU), ptr(ws.R), ws.rows_nslab, ws.row_slab_row0, perm, n, K, tol, it,
                     ptr(ws.FU), ptr(ws.mu_u), ptr(ws.upart), st)
        return start, step

    return _drive(ct_new, K, log_V_hat, n_iter, tol, check_every, ws,
                  (('a1', a1, _F64, (n, K)),) + _masks(ct_new.m, K, S_tilde, S_hat), launches)


def fold_in_zi(ct_new, K, log_V_hat, V_hat, pi_d, alpha1, alpha2, a1, a2, n_iter, tol, check_every=5, ws=None, arithmetic=1,
               S_tilde=None, S_hat=None):
    """Fold the cells of `ct_new` (CountTiles, sliced layout) into a fitted ZI-pCMF model whose gene side stays as it is: per
    cell the fixed point of the pair (a1, a2) under zigap.py:115-136 with V_hat, E[log V] and pi_d frozen --
      a1' = max(1e-15, alpha1 + sum_j x_ij r_ijk)        (the pCMF row pass: D_hat = f32(1 - 1e-10) = 1 at the non-zeros)
      a2' = max(1e-15, alpha2 + sum_j d_ij V_hat_jk),    d_ij = 1 at x_ij != 0, the column overrides of zigap.py:133-134, else
                                                         f32(sigmoid(logit(pi_d_j) - U_hat_i . V_hat_j)),  U_hat = a1 / a2
    both from the OLD pair (the reference's sweep order: the rate reads the D_hat formed from the U_hat that enters the sweep).
    `a1`, `a2` (n', K) float64 device tensors: the start, updated in place; log_V_hat (m, K) float32, V_hat (m, K) float64,
    pi_d [m], alpha1 / alpha2 [K] float64: the model's, only read.
    Each iteration: the rate buffer is zeroed, the row phase of a sweep runs on a workspace of this call's own (as fold_in),
    ONE oriana_zi_foldin_rate launch forms sum_j d_ij V_hat_jk from the call's own U_hat over the cells still active -- d is never
    stored: no (n', m) matrix exists at any point -- and ONE oriana_foldin_update_zi launch updates the pair, U_hat, E[log U],
    freezes the cells that moved by at most tol in both halves and prepares the next row pass's FU in place.  The per-gene
    operands are padded to a multiple of 4 genes with inert ones (V_hat row 0, pi_d 0), as the models do; both non-zero masks
    come from the packed counts, once per call.
    S_tilde, S_hat (m, K) float32 (SparseZIGaP.project(): log_V_hat is then E[log V'] and V_hat the effective S_hat * V'_hat,
    which both the posterior d and the rate read, sparse_zigap.py:138-140, 163-169): the masked row phase, as fold_in.
    Returns (froze_at, cells still active, iterations run) as fold_in."""
    n, m, dev = ct_new.n, ct_new.m, ct_new.device
    if K > 128 and not ct_new.gd:
        raise ValueError('the zero-inflated fold-in serves K <= 128 (the float32 dense kernels), got K = %d' % K)

    def launches(ws, tol):
        lib = _lib.load()
        mp, Vp, pip, nzmask = _padded_genes(ct_new, K, V_hat, pi_d)
        st, perm = stream_ptr(), ptr(ct_new.row_perm)
        nztiles = torch.zeros(max(int(lib.oriana_nzmask_tiles_words(n, mp)), 4), dtype=torch.int32, device=dev)
        call('oriana_nzmask_tiles', ptr(nztiles), ptr(nzmask), n, mp, st)
        scratch = torch.empty(int(lib.oriana_dropout_sweep_scratch_floats(mp, K)), dtype=_F32, device=dev)   # the call's own, undefined contents
        rate, U_hat = torch.empty(n, K, dtype=_F64, device=dev), torch.empty(n, K, dtype=_F64, device=dev)
        def start(lu, active):
            call('oriana_foldin_update_zi', ptr(a1), ptr(a2), ptr(U_hat), ptr(lu), ptr(active), None, None, None, None, None, None,
                 None, None, 1, 0, perm, n, K, tol, 0, ptr(ws.FU), ptr(ws.mu_u), ptr(ws.upart), st)
        def step(it, rows, lu, Zi, active, froze_at, n_active):
            rate.zero_()
            rows() if S_hat is None else rows(S_tilde, S_hat, active)
            with _span(ws, 'zi_foldin_rate'):
                call('oriana_zi_foldin_rate', ptr(rate), ptr(U_hat), ptr(Vp), ptr(pip), ptr(nzmask), ptr(nztiles), ptr(active),
                     ptr(scratch), int(arithmetic), n, mp, K, st)
            with _span(ws, 'foldin_update'):
                call('oriana_foldin_update_zi', ptr(a1), ptr(a2), ptr(U_hat), ptr(lu), ptr(active), ptr(froze_at), n_active,
                     ptr(alpha1), ptr(alpha2), ptr(rate), ptr(Zi), ptr(ws.FU), ptr(ws.R), ws.rows_nslab, ws.row_slab_row0,
                     perm, n, K, tol, it, ptr(ws.FU), ptr(ws.mu_u), ptr(ws.upart), st)
        return start, step

    operands = (('a1', a1, _F64, (n, K)), ('a2', a2, _F64, (n, K)), ('V_hat', V_hat, _F64, (m, K)), ('pi_d', pi_d, _F64, (m,)))
    operands += _masks(m, K, S_tilde, S_hat)
    return _drive(ct_new, K, log_V_hat, n_iter, tol, check_every, ws, operands, launches)


def gene_statistics(ct, K, a1, a2_row, log_V_hat, ws=None, finalize=True):
    """The per-gene sufficient statistics of a folded-in batch (GaP.partial_fit, the global step of a streaming fit): at the
    batch's final shapes a1 (n', K) float64 and the rate a2_row [K] every cell shares,
      Z_j[j,k] = sum_{i in batch} x_ij softmax_k(lu_i. + lv_j.),  lu = float32(psi(a1) - log a2_row) UNSHIFTED, from the Gamma node's
                 own kernel (nodes.gamma_expectations: what score_samples() evaluates the bound at), lv = log_V_hat (m, K) float32;
      sum_u[k] = sum_{i in batch} a1_ik / a2_row_k   (float64).
    ONE full plain responsibility pass (engine.zq_gap: factor preparation, row pass, slow path, column pass) over the batch's
    own tiles on `ws`, a ZWorkspace over `ct` -- the one the fold-in ran on (its in-place FU arrangement and the pending
    preparation are reset here: this pass prepares both factors from lu and log_V_hat) or None for a fresh one.  The cell
    sums of the pass are not completed: nothing reads them.
    a2_row may also be the (n', K) rate matrix of a ZI pair (ZIGaP.fold_in_fit: every cell its own rate): lu and sum_u then read
    each cell's own row, sum_u[k] = sum_i a1_ik / a2_ik.
    Returns (Z_j (m, K) float32, sum_u); with finalize=False the first is (Z_j, F, C, row_index) instead -- Z_j then holds the
    slow path's additions only and Z_j[row_index[p]] += F[p] * C[p] is left to the caller (oriana_svi_gene_update folds it
    into the blend: one launch and one pass over Z_j less).  Nothing in a sweep calls this."""
    n, m, dev = ct.n, ct.m, ct.device
    if ct.gd:
        raise ValueError('fold_in walks the sliced layout only: pack the new counts without dense_density')
    pair = isinstance(a2_row, torch.Tensor) and a2_row.dim() == 2
    for name, t, dtype, shape in (('log_V_hat', log_V_hat, _F32, (m, K)), ('a1', a1, _F64, (n, K)),
                                  ('a2_row', a2_row, _F64, (n, K) if pair else (K,))):
        _operand(name, t, dtype, shape)
    sum_u = (a1 / a2_row).sum(dim=0)
    Zj = torch.zeros(max(m, 1), K, dtype=_F32, device=dev)
    if n == 0:
        return (Zj[:m] if finalize else (Zj[:m], None, None, None)), sum_u
    if ws is None:
        ws = ZWorkspace(ct, K)
    else:
        ws.fu_pending, ws.prep_blocks = False, 0
        ws.FU_alt = ws.mu_u = ws.upart = None
    lu = gamma_expectations(a1, a2_row if pair else a2_row.expand(n, K).contiguous())[1]
    Zi = torch.empty(n, K, dtype=_F32, device=dev)
    zq(ws, Zi, Zj[:m], None, lu, log_V_hat, finalize_rows=False, finalize_cols=finalize)
    return (Zj[:m] if finalize else (Zj[:m], ws.FV, ws.C, ct.col_perm)), sum_u


def svi_gene_update(b1, b2, V_hat, log_V_hat, sums, beta1, beta2, stats, sum_u, scale, rho, ws=None):
    """The blend of a streaming fit's global step, ONE oriana_svi_gene_update launch, everything in place:
      b1 <- max(1e-15, (1 - rho) b1 + rho (beta1 + scale Z_j)),   b2 <- max(1e-15, (1 - rho) b2 + rho (beta2 + scale sum_u)),
    V_hat = b1 / b2, log_V_hat = float32 E[log V] and their column sums into `sums` (2, K) float64, zeroed here.
    `stats`: Z_j complete, or gene_statistics' unfinished (Z_j, F, C, row_index).  `sum_u`: the K-vector every gene shares, or an
    (m, K) float64 matrix in the caller's gene order (zi_gene_rate: oriana_svi_gene_update_mat, the same kernels).  `ws`: whose
    timer the launch reports to."""
    m, K = b1.shape
    Zj, F, C, perm = stats if isinstance(stats, tuple) else (stats, None, None, None)
    if sum_u.dim() == 2:
        _operand('sum_u', sum_u, _F64, (m, K))
    sums.zero_()
    with _span(ws, 'svi_gene_update'):
        call('oriana_svi_gene_update_mat' if sum_u.dim() == 2 else 'oriana_svi_gene_update', ptr(b1), ptr(b2), ptr(V_hat), ptr(log_V_hat), ptr(sums[0]), ptr(sums[1]), ptr(beta1),
             ptr(beta2), ptr(Zj), ptr(F), ptr(C), 1, ptr(perm), ptr(sum_u), float(scale), float(rho), m, K, stream_ptr())


def zi_gene_rate(ct, K, U_hat, V_hat, pi_d, ws=None):
    """The dropout-weighted rate statistic of a folded-in batch under a ZI model (ZIGaP.fold_in_fit), at the batch's final
    U_hat (n', K) float64 with V_hat (m, K) and pi_d [m] float64 as the fold-in read them:
      G[j,k] = sum_{i in batch} d_ij U_hat_ik   (m, K) float64,     dsum[j] = sum_{i in batch} d_ij   [m] float64,
    d the dropout posterior of fold_in_zi at that pair (1 at the non-zeros, the column overrides, else the float32 sigmoid), never
    stored: ONE oriana_zi_gene_rate launch sequence over the query's own non-zero mask with the per-gene operands padded to a
    multiple of 4 genes (_padded_genes), on scratch of the call's own.  Every element is written in a fixed order (two calls agree
    bit for bit).  K <= 128.  `ws`: whose timer the launches report to.  Returns (G, dsum)."""
    n, m, dev = ct.n, ct.m, ct.device
    if ct.gd:
        raise ValueError('fold_in walks the sliced layout only: pack the new counts without dense_density')
    if K > 128:
        raise ValueError('the zero-inflated gene rate serves K <= 128 (the float32 dense kernels), got K = %d' % K)
    for name, t, dtype, shape in (('U_hat', U_hat, _F64, (n, K)), ('V_hat', V_hat, _F64, (m, K)), ('pi_d', pi_d, _F64, (m,))):
        _operand(name, t, dtype, shape)
    if n == 0 or m == 0:
        return torch.zeros(m, K, dtype=_F64, device=dev), torch.zeros(m, dtype=_F64, device=dev)
    mp, Vp, pip, nzmask = _padded_genes(ct, K, V_hat, pi_d)
    scratch = torch.empty(max(int(_lib.load().oriana_zi_gene_rate_scratch_doubles(n, mp, K)), 1), dtype=_F64, device=dev)
    G, dsum = torch.empty(mp, K, dtype=_F64, device=dev), torch.empty(mp, dtype=_F64, device=dev)
    with _span(ws, 'zi_gene_rate'):
        call('oriana_zi_gene_rate', ptr(G), ptr(dsum), ptr(U_hat), ptr(Vp), ptr(pip), ptr(nzmask), ptr(scratch), n, mp, K, stream_ptr())
    return (G[:m], dsum[:m]) if mp == m else (G[:m].contiguous(), dsum[:m])        # (the inert genes' rows are dropped)


PI_D_FLOOR = 1e-10                # the override values of zigap.py:133-134: pi~ = min(max(pi_d, 1e-10), 1 - 1e-10)


def _cell_data_terms(ws, K, log_U, log_V_hat):
    """{sum_j x_ij log den_ij, sum_j lgamma(x_ij + 1)} per cell of ws.ct as a device (n', 2) float64 tensor: both factors prepared
    with their row maxima into buffers of this call's own, one oriana_row_pass that leaves s in the row-side slots, and
    oriana_cell_bound_nnz (the data term of cell_bounds and of zi_cell_bounds)."""
    ct = ws.ct
    n, m, dev = ct.n, ct.m, ct.device
    f32 = dict(dtype=_F32, device=dev)
    FU, FV = torch.zeros(n, ws.Kp, **f32), torch.zeros(max(m, 1), ws.Kp, **f32)
    mu_u, mu_v = torch.zeros(n, **f32), torch.zeros(max(m, 1), **f32)
    factor_prep(FU, log_U, mu=mu_u, row_index=ct.row_perm)
    factor_prep(FV, log_V_hat, mu=mu_v, row_index=ct.col_perm)
    if ws.s_rs is None:
        ws.s_rs = torch.zeros(max(ct.rslots, 1), **f32)
    ws.tile_flag.zero_()
    st = stream_ptr()
    with _span(ws, 'row_pass'):
        call('oriana_row_pass', ct.sparse_struct, ptr(FU), ptr(FV), None, ptr(ws.R), ptr(ws.s_cs), None, ptr(ws.s_rs),
             ptr(ws.tile_flag), K, st)
    pair = torch.empty(n, 2, dtype=_F64, device=dev)
    with _span(ws, 'cell_bound_nnz'):
        call('oriana_cell_bound_nnz', ct.sparse_struct, ptr(ws.s_rs), ptr(mu_u), ptr(mu_v), ptr(log_U), ptr(log_V_hat), K,
             ptr(pair), st)
    return pair


def _bounds(ct, K, log_U, log_V_hat, a1, a2, a2_is_row, alpha1, alpha2, operands, third, ws):
    """The (n', 4) float64 terms [data, lgamma, third(ws), kl] per cell of `ct`, caller's row order.  `operands`: (name, tensor,
    dtype, shape) beside those checked here; a2: the K-vector rate of every cell (a2_is_row) or the cells' own (n', K)."""
    if ct.gd:
        raise ValueError('fold_in walks the sliced layout only: pack the new counts without dense_density')
    n, m, dev = ct.n, ct.m, ct.device
    for name, t, dtype, shape in (('log_V_hat', log_V_hat, _F32, (m, K)), ('log_U', log_U, _F32, (n, K)), ('a1', a1, _F64, (n, K)),
                                  ('alpha1', alpha1, _F64, (K,)), ('alpha2', alpha2, _F64, (K,))) + tuple(operands):
        _operand(name, t, dtype, shape)
    out = torch.empty(n, 4, dtype=_F64, device=dev)
    if n == 0:
        return out
    if ws is None:
        ws = ZWorkspace(ct, K)
    out[:, :2] = _cell_data_terms(ws, K, log_U, log_V_hat)
    out[:, 2] = third(ws)
    kl = torch.empty(n, dtype=_F64, device=dev)
    with _span(ws, 'gamma_kl_rows'):
        call('oriana_gamma_kl_rows', ptr(kl), ptr(a1), ptr(a2), 1 if a2_is_row else 0, ptr(alpha1), ptr(alpha2), n, K, stream_ptr())
    out[:, 3] = kl
    return out


def cell_bounds(ct, K, a1, a2_row, log_U, log_V_hat, sum_v, alpha1, alpha2, ws=None):
    """Each cell's share of pCMF's collapsed variational bound with the gene side as given: a device (n', 4) float64 tensor
    [data, lgamma, product, kl] per cell of `ct` (CountTiles, sliced layout), caller's row order --
      data_i    = sum_{j: x_ij != 0} x_ij logsumexp_k(log_U_ik + log_V_hat_jk)         lgamma_i = sum_{j: x_ij != 0} lgamma(x_ij + 1)
      product_i = sum_k (a1_ik / a2_row_k) sum_v_k                                    kl_i = sum_k KL(Gamma(a1_ik, a2_row_k) || Gamma(alpha1_k, alpha2_k))
    and the cell's score is data - lgamma - product - kl.  a1 (n', K) float64, log_U (n', K) float32 (the E[log U] the data
    term is evaluated at, unshifted), log_V_hat (m, K) float32, a2_row / sum_v / alpha1 / alpha2 [K] float64: all only read.
    The data term is GaP._elbo_terms' per cell: both factors prepared with their row maxima into buffers of this call's own,
    one oriana_row_pass that leaves s in the row-side slots, and oriana_cell_bound_nnz, which reads that stream once and
    writes every cell's two sums in a fixed order (no atomics: two calls agree bit for bit); the Kullback-Leibler term is
    oriana_gamma_kl_rows.  `ws`: a ZWorkspace over `ct` of the caller's own (its row-pass scratch is overwritten); None
    makes one."""
    return _bounds(ct, K, log_U, log_V_hat, a1, a2_row, True, alpha1, alpha2,
                   (('a2_row', a2_row, _F64, (K,)), ('sum_v', sum_v, _F64, (K,))),
                   lambda ws: ((a1 / a2_row) * sum_v).sum(dim=1), ws)


def zi_cell_bounds(ct, K, a1, a2, log_U, log_V_hat, V_hat, pi_d, alpha1, alpha2, ws=None):
    """Each cell's share of ZI-pCMF's variational bound with the gene side as given and q(Z), q(d) collapsed at their optima: a
    device (n', 4) float64 tensor [data, lgamma, dropout, kl] per cell of `ct` (CountTiles, sliced layout), caller's row order --
      data_i, lgamma_i as cell_bounds;    kl_i = sum_k KL(Gamma(a1_ik, a2_ik) || Gamma(alpha1_k, alpha2_k))
      dropout_i = sum_j log(1 - pi~_j) + sum_{x_ij != 0} z_ij + sum_{x_ij = 0} softplus(z_ij),
      z_ij = logit(pi~_j) - (a1_i / a2_i) . V_hat_j,    pi~ = min(max(pi_d, 1e-10), 1 - 1e-10)
    and the cell's score is data - lgamma + dropout - kl.  a1, a2 (n', K), V_hat (m, K), pi_d [m], alpha1 / alpha2 [K] float64,
    log_U (n', K) float32 (the E[log U] the data term is evaluated at, unshifted), log_V_hat (m, K) float32: all only read.
    The dropout term is ONE oriana_zi_cell_bound launch sequence over the query's own non-zero mask (oriana_nzmask_counts, as
    fold_in_zi builds it) with the per-gene operands padded to a multiple of 4 genes; the cell-independent sum is added here in
    float64.  No (n', m) matrix exists at any point; every term is written in a fixed order (two calls agree bit for bit).
    `ws`: a ZWorkspace over `ct` of the caller's own (its row-pass scratch is overwritten); None makes one."""
    n, m, dev = ct.n, ct.m, ct.device
    if K > 128 and not ct.gd:
        raise ValueError('the zero-inflated bound serves K <= 128 (the float32 dense kernels), got K = %d' % K)

    def dropout(ws):
        mp, Vp, pip, nzmask = _padded_genes(ct, K, V_hat, pi_d)
        U_hat = a1 / a2
        scratch = torch.empty(max(int(_lib.load().oriana_zi_cell_bound_scratch_doubles(n, mp, K)), 1), dtype=_F64, device=dev)
        drop = torch.empty(n, dtype=_F64, device=dev)
        with _span(ws, 'zi_cell_bound'):
            call('oriana_zi_cell_bound', ptr(drop), ptr(U_hat), ptr(Vp), ptr(pip), ptr(nzmask), ptr(scratch), n, mp, m, K, stream_ptr())
        return drop + torch.log1p(-torch.clamp(pi_d, PI_D_FLOOR, 1.0 - PI_D_FLOOR)).sum()

    return _bounds(ct, K, log_U, log_V_hat, a1, a2, False, alpha1, alpha2,
                   (('a2', a2, _F64, (n, K)), ('V_hat', V_hat, _F64, (m, K)), ('pi_d', pi_d, _F64, (m,))), dropout, ws)
