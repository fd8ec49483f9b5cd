# -*- coding: utf-8 -*-
"""pCMF = Gamma-Poisson factor model (reference oriana/models/gap.py:14-135)."""
import os

import torch

from .. import engine, heldout
from .. import dist as odist
from .._lib import call, ptr, stream_ptr
from ..nodes import gamma_expectations
from .base import FactorModel

__all__ = ['GaP']


class GaP(FactorModel):

    @staticmethod
    def compute_Z_q_expectations(Z_hat_i, Z_hat_j, log_U_hat, log_V_hat, X):
        """Drop-in for the reference's loop nest (gap.py:67-80): outputs first, caller allocates,
        callee zero-fills, returns None.  All arguments are 2-D C-contiguous float32 DEVICE tensors
        (TypeError otherwise, like numba's explicit signature); X is dense (n, m) and is repacked on
        every call through the stateless C entry oriana_zq_gap_f32 (the model itself keeps X packed
        across sweeps)."""
        engine.zq_gap_stateless(Z_hat_i, Z_hat_j, log_U_hat, log_V_hat, X)

    def update_variational_parameters(self):
        """gap.py:82-115 (E-step)."""
        # both Z sums use the PRE-update E[log U], E[log V] (one joint pass, gap.py:89-94); the cell side only
        # needs Z_i, so its update runs between the row pass and the column pass and every partial of the
        # sweep's single exchange exists when the column pass ends
        # Launch count matters on a small matrix (configs[1]: a sweep is ~10 launches of a few microseconds of work each):
        # the zero-fills ride on the factor preparation, Z += F * R on the Gamma updates, both M-steps share a launch.
        ws, ct = self._ws, self.counts
        if self._v_sums_in_acc:                # an E-step without the M-step before it: sum_j V_hat is still in scratch
            self._sumV.copy_(self._accV)
            self._v_sums_in_acc = False
        fold_cols = not self.sharded           # (under row sharding Z_j is completed per rank, then exchanged)
        # Row sharding, K == Kp: the per-gene sums are exchanged in the PACKED gene order, where the dense genes [0, gd) and
        # the sliced genes [gd, m) are contiguous segments -- the sliced segment (86 % of the 12 MB at C4) starts its
        # all-reduce as soon as the sliced column pass has finished and travels under the dense gene-side kernel; the
        # gene-side update then reads the reduced sums through the permutation (Z[o] = 1 * Zx[p], exact).
        packed = self.sharded and ws.Kp == self.k
        engine.zq_gap(ws, self._Zi, self._Zj, self._log_U_hat, self._log_V_hat, phase='rows', finalize_rows=False,
                      clear=(self._sumU, self._accV) + ((self._Zj_o,) if packed else ()), zj_packed=packed)
        # U_q: a1 = alpha1 + Z_i ; a2 = alpha2 + sum_j V_hat (OLD V_hat)                gap.py:97-102
        lazy = self._gamma_side_finalize('u', self._Zi, ws.FU, ws.R, ct.row_perm, self._sumV[0], self._sumU,
                                         nslab=ws.row_gene_splits, slab_row0=ws.row_slab_row0,
                                         a2_row=self._a2_row if self._lazy_ok else None)
        if lazy:
            self._u_on_access()
        else:
            self._lazy_ok = False            # (no vector kernel for this K / a launch-bound size: decided once per model)
        self._exchange_start()                  # sum_i U_hat | sum_i log U_hat (float64): reduced under the column pass
        engine.zq_gap(ws, self._Zi, self._Zj, self._log_U_hat, self._log_V_hat, phase='cols', finalize_cols=not fold_cols,
                      zj_packed=packed,
                      on_segment=(lambda lo, hi: self._xch.reduce_rows_async('Zj', lo, hi)) if packed else None)
        self._exchange()                        # Z_j (float32, 12 MB at C4; its segments are already on their way) + wait
        # V_q: b1 = beta1 + Z_j ; b2 = beta2 + sum_i U_hat (NEW U_hat)                   gap.py:105-110
        # (its column sums go to scratch: _sumV still holds sum_j V_hat of the sweep's start, which the M-step replaces)
        if fold_cols:
            self._gamma_side_finalize('v', self._Zj, ws.FV, ws.C, ct.col_perm, self._sumU[0], self._accV)
        elif packed:
            self._gamma_side_finalize('v', self._Zj_o, self._ones_v, self._Zj, ct.col_perm, self._sumU[0], self._accV)
        else:
            self._gamma_side('v', self._Zj, rate_vec=self._sumU[0], sums_arg=self._accV, zero=False)
        self._v_sums_in_acc = True

    # ---- [r6] a2 and U_hat of the cell side are evaluated on access ---------------------------------------------------------
    # Inside a sweep nothing reads them: a2[i, :] = alpha2 + sum_j V_hat is the same K numbers for every cell (gap.py:98) and
    # U_hat = a1 / a2 (gap.py:101) enters the sweep only through its column sums, which the update kernel forms itself.  The
    # kernel therefore writes the K rate values once (_a2_row) and model.a2 / model.U_hat / factors() / state() / save()
    # materialise the (n, K) float64 matrices when somebody asks -- a broadcast and a float64 division, bit for bit what the
    # kernel would have stored.  1.6 of the 4.8 GB of the cell-side update at configs[3] (ORIANA_LAZY_U=0: stored every sweep).
    _u_stale = False
    _U_buf = None
    _a2_row = None
    _lazy_ok = True

    @property
    def _U_hat(self):
        if self._u_stale:
            torch.div(self.a1.tensor, self._a2_row, out=self._U_buf)           # Gamma._mean, gamma.py:37-46
            self._u_stale = False
        return self._U_buf

    @_U_hat.setter
    def _U_hat(self, t):
        self._U_buf, self._u_stale = t, False

    def _u_on_access(self):
        n, K = self.n, self.k
        row = self._a2_row
        self.a2.defer(lambda: row.clone().expand(n, K).contiguous())
        self._u_stale = True

    def load_state(self, st):
        # U_hat is formed from the a1 / a2 it belongs to BEFORE a loaded a1 replaces them: load_state recomputes nothing, so
        # keys that are not loaded keep their values, as in the storing form.  The loaded a2, if any, is then the
        # materialised parameter; _a2_row is only read while U_hat is stale, which the next sweep's kernel decides anew.
        self._U_hat
        FactorModel.load_state(self, st)

    def step(self):
        FactorModel.step(self)
        if self._graph is not None and self._a2_row is not None and self._lazy_ok:
            self._u_on_access()              # (a replayed graph ran the kernel again: what was materialised is stale)

    # ---- the variational bound ---------------------------------------------------------------------------------------------
    # With q(Z) at its multinomial optimum for the current q(U) q(V) (Gamma(shape, rate) throughout):
    #   ELBO = sum_{x != 0} [x log den - lgamma(x + 1)] - sum_k (sum_i U_hat_ik)(sum_j V_hat_jk) - KL_U - KL_V,
    #   log den_ij = logsumexp_k(E[log U]_ik + E[log V]_jk)            (the float32 expectations the next sweep reads)
    # Every update of step() maximises the uncollapsed bound in one coordinate and collapsing q(Z) only raises it, so the
    # value never decreases from sweep to sweep (M-step included) beyond its float32 evaluation error.  Its only
    # Theta(nnz K) term is the first one, and den is what the row pass forms: one row pass over factors prepared into scratch
    # of the call's own (the FU the last update prepared for the next sweep stays as it is), a read of s, and Theta((n + m) K)
    # float64 work.
    _no_elbo = None

    def _elbo_terms(self):
        """The five terms {data, lgamma, product, kl_u, kl_v} as a float64 device vector (all-reduced over the row shards)."""
        ct, K, n, m, dev, ws = self.counts, self.k, self.n, self.m, self.device, self._ws
        st = stream_ptr()
        lu, lv = self._log_U_hat, self._log_V_hat
        FU, FV = ws.extra('EU', n), ws.extra('EV', m)
        mu = getattr(self, '_elbo_mu', None)
        if mu is None:
            mu = self._elbo_mu = torch.zeros(max(n, 1) + max(m, 1), dtype=torch.float32, device=dev)
        mu_u, mu_v = mu[:max(n, 1)], mu[max(n, 1):]
        engine.factor_prep(FU, lu, mu=mu_u, row_index=ct.row_perm)
        engine.factor_prep(FV, lv, mu=mu_v, row_index=ct.col_perm)
        if ws.s_rs is None:
            ws.s_rs = torch.zeros(max(ct.rslots, 1), dtype=torch.float32, device=dev)
        ws.tile_flag.zero_()
        # (hybrid layout: the sliced part covers the packed genes [gd, m), the dense genes are summed in float64)
        call('oriana_row_pass', ct.sparse_struct, ptr(FU), ptr(FV) + 4 * ct.gd * ws.Kp, None, ptr(ws.R), ptr(ws.s_cs), None,
             ptr(ws.s_rs), ptr(ws.tile_flag), K, st)
        # cell-side partials in one packed vector: [sum x log den, sum lgamma(x + 1), KL_U, sum_i U_hat (K)]
        part = torch.zeros(3 + K, dtype=torch.float64, device=dev)
        call('oriana_elbo_nnz', ct.sparse_struct, ptr(ws.s_rs), ptr(mu_u), ptr(mu_v) + 4 * ct.gd, ptr(lu), ptr(lv), K, ptr(part), st)
        if ct.dense is not None:
            call('oriana_dense_elbo', ct.dense.c_struct, ptr(lu), ptr(lv), ptr(ct.row_perm), ptr(ct.col_perm), ptr(part), K, st)
        # the cell-side rate: the K numbers of the lazy form while a2 is deferred (it is not materialised here)
        a2 = self.a2
        row = self._a2_row is not None and not getattr(a2, 'materialised', True)
        call('oriana_gamma_kl', ptr(part[2:]), ptr(self.a1.tensor), ptr(self._a2_row if row else a2.tensor), 1 if row else 0,
             ptr(self.alpha1.tensor), ptr(self.alpha2.tensor), n, K, st)
        if self._u_stale:                       # U_hat = a1 / a2_row is not stored: its column sums from a1
            part[3:] = self.a1.tensor.sum(0) / self._a2_row
        else:
            part[3:] = self._U_buf.sum(0)
        odist.all_reduce_sum(part, self.pg)
        # the gene side is replicated: counted once
        kl_v = torch.zeros(1, dtype=torch.float64, device=dev)
        call('oriana_gamma_kl', ptr(kl_v), ptr(self.b1.tensor), ptr(self.b2.tensor), 0, ptr(self.beta1.tensor),
             ptr(self.beta2.tensor), m, K, st)
        prod = (part[3:] * self._V_hat.sum(0)).sum().reshape(1)
        return torch.cat([part[:2], prod, part[2:3], kl_v])

    def elbo(self):
        """The evidence lower bound of the current variational state, q(Z) at its optimum (a Python float).  Non-decreasing
        from sweep to sweep; leaves the state and the next sweep untouched ("The variational bound")."""
        t = self._elbo_terms()
        return float(t[0] - t[1] - t[2] - t[3] - t[4])

    # ---- folding in new cells ----------------------------------------------------------------------------------------------
    # For a cell the model was not fitted on, with the gene side held fixed, the cell-side update of the sweep (lines 97-102 of
    # the reference's gap.py) is a fixed-point iteration of that cell alone: a2 = alpha2 + sum_j V_hat never moves, a1 <- alpha1 +
    # sum_j x_ij r_ijk with r the softmax of E[log U]_i. + E[log V]_j. .  heldout.fold_in runs it on a workspace of its own:
    # nothing the model or its workspace hold is written ("Folding in new cells").
    transform_unconverged_ = None

    def transform(self, cmatrix, n_iter=200, tol=1e-4, init=None, return_params=False, check_every=5):
        """Fold new cells into the fitted model: E[U] = a1 / a2_row of `cmatrix` (anything the constructor takes; the same
        genes) as a host (n', K) float64 array, V and the priors as they are.  Each cell iterates its own update until it
        moves by at most tol * a1 in every factor (then it is frozen: its result does not depend on the other cells) or
        `n_iter` is reached; ``transform_unconverged_`` counts the cells that never froze.  `init`: (n', K) starting a1
        (default alpha1 + rowsum(x) / K: uniform responsibilities, no RNG).  return_params=True: (E[U], a1, a2_row, the
        0-based iteration each cell froze at -- n_iter for those that did not).  Under row sharding the call is local to the
        rank (V is replicated): no collective."""
        ct, ws, a1, a2_row, sum_v, froze_at = self._fold_in_cells(cmatrix, n_iter, tol, init, check_every)
        E = (a1 / a2_row).cpu().numpy()
        if return_params:
            return E, a1.cpu().numpy(), a2_row.cpu().numpy(), froze_at.cpu().numpy()
        return E

    def _fold_in_cells(self, cmatrix, n_iter, tol, init, check_every):
        """The fold-in of transform() and score_samples(): (the packed cells, the call's workspace -- None for no cells --, the
        final a1 (n', K), a2_row [K], sum_j V_hat [K] as the sweep reads it, froze_at), all on the device; sets
        ``transform_unconverged_``."""
        ct = self._query_counts(cmatrix)
        K = self.k
        sum_v = self._accV[0] if self._v_sums_in_acc else self._sumV[0]          # as the sweep reads sum_j V_hat
        a2_row = torch.clamp(torch.nan_to_num(self.alpha2.tensor + sum_v), min=1e-15)       # gap.py:98, 100
        ws = engine.ZWorkspace(ct, K) if ct.n > 0 else None
        a1 = self._fold_in_start(ct, ws, init)
        froze_at, left, _ = heldout.fold_in(ct, K, self._log_V_hat, self.alpha1.tensor, a2_row, a1, n_iter, tol,
                                            check_every=check_every, ws=ws)
        self.transform_unconverged_ = int(left)
        return ct, ws, a1, a2_row, sum_v, froze_at

    # ---- scoring held-out cells --------------------------------------------------------------------------------------------
    # The bound of elbo() is a sum over the cells minus the gene side's KL: with the gene side frozen, cell i contributes
    #   score_i = sum_{j: x_ij != 0} [x_ij log den_ij - lgamma(x_ij + 1)] - sum_k (a1_ik / a2_row_k) sum_j V_hat_jk - KL_i,
    # log den_ij = logsumexp_k(lu_ik + E[log V]_jk), lu = float32(psi(a1) - log a2_row) UNSHIFTED (what the cell would carry into
    # a sweep), KL_i = sum_k KL(Gamma(a1_ik, a2_row_k) || Gamma(alpha1_k, alpha2_k)).  One fold-in iteration is exact coordinate
    # ascent on score_i (the rate a2_row is already the optimal one), so the value does not decrease along the fold-in beyond
    # its evaluation error and the float32 cast of lu.  Held-out cells' mean score answers "how many factors?": unlike elbo()
    # on the training cells it does not keep rising with k ("Scoring held-out cells").

    def score_samples(self, cmatrix, n_iter=200, tol=1e-4, init=None, check_every=5, return_terms=False):
        """The per-cell variational bound of new cells with the gene side frozen: `cmatrix` is folded in exactly as transform()
        does (same arguments, same result, ``transform_unconverged_`` set) and each cell's share of the bound of elbo() is
        evaluated at its final a1: a host (n',) float64 array, higher = better explained.  return_terms=True: a dict with
        score = data - lgamma - product - kl and those four terms (each (n',)), a1, a2_row, froze_at and log_U_hat, the float32
        E[log U] = psi(a1) - log a2_row the data term was evaluated at.  The model and its workspace are not written; under row
        sharding the call is local to the rank."""
        ct, ws, a1, a2_row, sum_v, froze_at = self._fold_in_cells(cmatrix, n_iter, tol, init, check_every)
        K = self.k
        # E[log U] of the final shapes by the Gamma node's own kernel, against the rate expanded to every cell
        lu = gamma_expectations(a1, a2_row.expand(ct.n, K).contiguous())[1]
        terms = heldout.cell_bounds(ct, K, a1, a2_row, lu, self._log_V_hat, sum_v.contiguous(), self.alpha1.tensor,
                                    self.alpha2.tensor, ws=ws)
        return self._score_result(terms.cpu().numpy(), ('data', 'lgamma', 'product', 'kl'), '+---',
                                  dict(a1=a1.cpu().numpy(), a2_row=a2_row.cpu().numpy(), froze_at=froze_at.cpu().numpy(),
                                       log_U_hat=lu.cpu().numpy()), return_terms)

    def score(self, cmatrix, **kw):
        """The mean of score_samples(cmatrix, **kw) as a Python float (nan for no cells): compare it across fits with
        different k on cells none of them was fitted on."""
        return self._mean_score(self.score_samples(cmatrix, **kw))

    # ---- streaming fits ----------------------------------------------------------------------------------------------------
    # Stochastic variational inference (Hoffman et al. 2013; for Poisson factorisation Gopalan et al.): a batch of cells the
    # model does not hold is folded in against the current gene side (the LOCAL step: exactly the fold-in of transform()), its
    # per-gene sufficient statistics at the converged cell side are scaled to the population, n_total / n_B, and blended into
    # b1, b2 with a step size rho (the GLOBAL step, a natural-gradient step on the bound of elbo()):
    #   b1 <- (1 - rho) b1 + rho (beta1 + scale Z_j),   b2 <- (1 - rho) b2 + rho (beta2 + scale sum_{i in B} E[U_i.])
    # The priors stay where the fit left them and the model's own cells are not touched.  It needs a gene side that already
    # separates the factors -- fit on what is resident, then stream the rest ("Streaming fits: partial_fit()").
    n_batches_ = 0
    partial_fit_rho_ = None
    partial_fit_unconverged_ = None

    def partial_fit(self, cmatrix, n_total, rho=None, tau0=1.0, kappa=0.7, n_iter=200, tol=1e-4, init=None, check_every=5):
        """One stochastic variational update of the gene side from a batch of cells: `cmatrix` (anything transform() takes, a
        prebuilt sliced ``engine.CountTiles`` included: epochs need not repack) is a sample of a population of `n_total` cells.
        The batch is folded in as transform() folds it (`n_iter`, `tol`, `init`, `check_every`; ``partial_fit_unconverged_`` counts
        the cells that never froze), and b1, b2 move towards the batch's estimate by the step size `rho` in [0, 1] -- default
        min(1, (tau0 + n_batches_) ** -kappa), tau0 > 0, kappa in (0.5, 1]; the value used is kept in ``partial_fit_rho_`` and
        ``n_batches_`` counts the non-empty calls.  V_hat, E[log V] and their column sums follow in the same launch, so step(),
        elbo(), transform() and score() read the streamed gene side; the priors and the model's own cell side stay as they
        are (a later step() is ordinary CAVI on the construction cells).  An empty batch changes nothing.  Returns self."""
        if self.sharded:
            raise NotImplementedError('partial_fit() under row sharding is not implemented: the batch statistics of the ranks '
                                      'would need a collective of their own')
        tau0, kappa = float(tau0), float(kappa)
        if not tau0 > 0.0:
            raise ValueError('partial_fit needs tau0 > 0, got %r' % (tau0,))
        if not 0.5 < kappa <= 1.0:
            raise ValueError('partial_fit needs kappa in (0.5, 1], got %r' % (kappa,))
        if rho is not None and not 0.0 <= float(rho) <= 1.0:
            raise ValueError('partial_fit needs rho in [0, 1], got %r' % (rho,))
        ct = self._query_counts(cmatrix)
        if not int(n_total) >= ct.n:
            raise ValueError('partial_fit needs n_total >= the %d cells of the batch, got %r' % (ct.n, n_total))
        if ct.n == 0:
            return self
        rho = min(1.0, (tau0 + self.n_batches_) ** -kappa) if rho is None else float(rho)
        kept = self.transform_unconverged_
        ct, ws, a1, a2_row, _, _ = self._fold_in_cells(ct, n_iter, tol, init, check_every)
        self.partial_fit_unconverged_, self.transform_unconverged_ = self.transform_unconverged_, kept
        stats, sum_u = heldout.gene_statistics(ct, self.k, a1, a2_row, self._log_V_hat, ws=ws, finalize=False)
        # what load_state() would leave: the pair, its expectations and their column sums where the next sweep reads them
        heldout.svi_gene_update(self.b1.tensor, self.b2.tensor, self._V_hat, self._log_V_hat, self._sumV, self.beta1.tensor,
                                self.beta2.tensor, stats, sum_u, float(int(n_total)) / ct.n, rho, ws=ws)
        self._v_sums_in_acc = False
        self._touch()
        self.n_batches_ += 1
        self.partial_fit_rho_ = rho
        return self

    def _init_extra(self):
        if os.environ.get('ORIANA_LAZY_U', '1') != '0':
            from ..parameters import LazyParameter
            n, K, dev = self.n, self.k, self.device
            self._a2_row = torch.ones(K, dtype=torch.float64, device=dev)
            self.a2 = LazyParameter((n, K), dev, lambda: torch.ones(n, K, dtype=torch.float64, device=dev))   # gap.py:43 (ones)
        if self.sharded and self._ws.Kp == self.k:
            # the gene-side update of the packed exchange: Z in the caller's gene order (cleared by the factor preparation's
            # launch every sweep) and the all-ones factor of  Z[o] = 1 * Zx[p]
            self._Zj_o = torch.zeros(self.m, self.k, dtype=torch.float32, device=self.device)
            self._ones_v = torch.ones(self.m, self._ws.Kp, dtype=torch.float32, device=self.device)
