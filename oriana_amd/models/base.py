# -*- coding: utf-8 -*-
"""Factor models: the reference's driver surface (constructor, ``step()``, ``factors()``, public
attribute names -- reference oriana/models/base.py:13-130) over device-resident state and the HIP
kernels of include/oriana_hip.h.  One process per GPU; cells (rows) are sharded across ranks.

What is kept from the reference: attribute names and shapes (``alpha1 .. p_s`` are ``Parameter``
objects holding float64 buffers, parameters.py:8-32), the order of the updates inside a sweep, the
float32 / float64 split of every quantity, the clamps, and -- behind ``reference_quirks=True`` --
the reference's index quirk (zigap.py:94).  What is not: the dense n x m rate matrix is never
materialised (``UV`` is evaluated on demand), X is packed once instead of re-cast every sweep.
"""
import numpy as np
import torch

from .. import engine, heldout
from .._lib import call, ptr, stream_ptr, OrianaHipError
from ..parameters import Parameter
from ..dims import Dimensions
from .. import dist as odist

__all__ = ['FactorModel']


class _Buffer:
    """Minimal stand-in for a reference node (``model.U[:]``, ``.buffer``, ``.asarray()``)."""

    def __init__(self, getter):
        self._getter = getter

    @property
    def buffer(self):
        return self._getter()

    def asarray(self):
        return self._getter().detach().cpu().numpy()

    def __getitem__(self, key):
        return self._getter()[key].detach().cpu().numpy()


def _is_sparse_input(c):
    """SciPy sparse matrices and CountMatrix objects built from one (`._sparse`).  A torch sparse tensor is
    not a supported container: say so instead of failing inside SciPy."""
    import scipy.sparse as sp
    if isinstance(c, torch.Tensor) and (c.is_sparse or c.layout != torch.strided):
        raise TypeError('torch sparse tensors are not supported: pass a SciPy sparse matrix, a dense array / tensor '
                        'or engine.CountTiles')
    return sp.issparse(c) or sp.issparse(getattr(c, '_sparse', None))


class FactorModel:
    """Base class (reference models/base.py:13-56).

    Parameters
    ----------
    cmatrix : object with ``.shape`` and ``.as_array()`` (reference CountMatrix, base.py:22-23,
        gap.py:31), a NumPy array, a torch tensor, or an ``engine.CountTiles`` already resident
        on the device.  With a process group this is the LOCAL row shard.
    k : number of factors.  use_factors : warm-start a1 / b1 from NMF factors (base.py:37-40).
    init : optional ``(a1, b1)`` arrays (post-clamp initial shapes) -- bypasses NMF / host RNG; or
        ``'nmf'`` / ``'random'``: starts computed on the device (models/deviceinit.py), for counts that are
        already resident, sparse or row-sharded (``seed`` keys them by global row).
    device : torch device (default cuda).  process_group : torch.distributed group for row sharding.
    reference_quirks : reproduce zigap.py:94 (``D_hat[i, k]``) -- see SURVEY.md 8(a) policy.
    dense_density : genes expressed in at least this share of the cells are evaluated densely on the bf16 matrix cores in
        float32-equivalent arithmetic (hybrid layout, csrc/dense_pass.hip; DESIGN_HISTORY.md section 10).  Every model takes it:
        inside the ZI models D_hat = 1 at every non-zero count, so their nest is the pCMF nest plus the D_hat[i, k] weight
        on the gene side; the sparse models' den runs against the masked FV image, their accumulation against FV * S_hat,
        their log sums through a second gene-side pass.  ``'auto'`` for the ZI / sparse models: the same threshold, but only
        when the genes above it hold at least 75 % of the non-zeros (i.e. on data that are about half dense or denser).
        ``'auto'``: engine.auto_dense_density -- engine.DENSE_DENSITY_DEFAULT (or the environment's ORIANA_DENSE_DENSITY;
        ``0`` / ``off`` disables) for matrices of at least 2e8 entries and a K the dense kernels are compiled for; ignored
        for a prebuilt ``engine.CountTiles`` (its own layout is used).
    """

    zi = False
    sparse = False
    _graph_capturing = False

    def __init__(self, cmatrix, k=2, use_factors=True, tau=0.5, init=None, device=None, process_group=None,
                 reference_quirks=True, n_total=None, seed=0, dense_density='auto'):
        if not torch.cuda.is_available():
            raise OrianaHipError('oriana_amd needs a ROCm GPU: the CAVI kernels are HIP only (no CPU fallback)')
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.cmatrix = cmatrix
        self.k = int(k)
        self.tau = tau
        self.use_factors = use_factors
        self.reference_quirks = reference_quirks
        self.seed = int(seed)
        self.pg = process_group
        self.world = odist.world_size(process_group)
        self.sharded = odist.sharded(process_group)     # (also the one-rank rehearsal mode, dist._forced)

        X_host = None
        # Under row sharding every rank must pack the genes in the SAME internal order (the replicated
        # gene-side matrices of the on-device NMF start live in packed order): the per-gene counts that
        # define the order are summed over the shards.
        rf = (lambda t: odist.all_reduce_sum(t, process_group)) if self.sharded else None
        dd = self._dense_density(dense_density, cmatrix, n_total, init)
        if isinstance(cmatrix, engine.CountTiles):
            self.counts = cmatrix
        elif _is_sparse_input(cmatrix):
            A = cmatrix._sparse if hasattr(cmatrix, '_sparse') else cmatrix
            X_host = A                     # the host-side initialisation reads it in sparse form
            self.counts = engine.CountTiles.from_scipy(A, self.device, reduce_fn=rf, dense_density=dd, n_total=n_total,
                                                       dense_min_share=getattr(self, '_dense_min_share', 0.0))
        else:
            X = cmatrix.as_array() if hasattr(cmatrix, 'as_array') else cmatrix
            if not isinstance(X, torch.Tensor):
                X = np.asarray(X)
                X_host = X
            self.counts = engine.CountTiles.from_dense(X, self.device, reduce_fn=rf, dense_density=dd, n_total=n_total,
                                                       dense_min_share=getattr(self, '_dense_min_share', 0.0))
        self.n = self.counts.n
        self.m = self.p = self.counts.m
        self.n_total = int(n_total) if n_total is not None else odist.sum_int(self.n, process_group, self.device)
        self.dims = Dimensions({'n': self.n, 'm': self.m, 'p': self.p, 'k': self.k})
        if self.zi and self.reference_quirks and self.k > self.m:
            raise ValueError('reference_quirks=True needs k <= number of genes (zigap.py:94 reads D_hat[i, k])')

        K, n, m, dev = self.k, self.n, self.m, self.device
        f64 = dict(dtype=torch.float64, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        # prior hyper-parameters (build_u_node / build_v_node, gap.py:19-27): every value is
        # overwritten by the first M-step except alpha2 = beta2 = 1, which that M-step reads
        self.alpha1 = Parameter(torch.ones(K, **f64))
        self.alpha2 = Parameter(torch.ones(K, **f64))
        self.beta1 = Parameter(torch.ones(K, **f64))
        self.beta2 = Parameter(torch.ones(K, **f64))
        # variational parameters (define_variational_distribution, gap.py:34-44)
        a1_0, b1_0, nmf = self._initial_shapes(X_host, init)
        self.nmf_factors = nmf
        # (copy=True: a device tensor given as `init` must not become the parameter buffer of the model)
        self.a1 = Parameter(a1_0.to(copy=True, **f64).clamp_(min=1e-15).contiguous())       # gap.py:55
        self.a2 = Parameter(torch.ones(n, K, **f64))
        self.b1 = Parameter(b1_0.to(copy=True, **f64).clamp_(min=1e-15).contiguous())       # gap.py:65
        self.b2 = Parameter(torch.ones(m, K, **f64))
        # expectations (device); exposed as NumPy through the properties below
        self._U_hat = torch.empty(n, K, **f64)
        self._V_hat = torch.empty(m, K, **f64)
        self._log_U_hat = torch.empty(n, K, **f32)
        self._log_V_hat = torch.empty(m, K, **f32)
        self._Zi = torch.empty(max(n, 1), K, **f32)
        # everything a sweep exchanges between row shards lives in ONE packed float32 buffer (dist.SweepExchange):
        # the per-gene sums are views into it, written in place by the kernels
        f32_seg = {'Zj': (max(m, 1), K)}
        if self.sparse:
            f32_seg['Zlog'] = (max(m, 1), K)
        f64_seg = {'DtU': (m, K)} if self.zi else {}
        f64_seg['sumU'] = (2, K)
        self._xch = odist.SweepExchange(dev, process_group, f32_seg, f64_seg)
        self._Zj = self._xch.f32['Zj']
        self._sumU = torch.zeros(2, K, **f64)        # [sum_i U_hat, sum_i log_U_hat]
        self._sumV = torch.zeros(2, K, **f64)
        # the gene side's column sums while a sweep accumulates them (cleared with the other scratch of the sweep by the
        # factor preparation's launch; the M-step copies them to _sumV, which the next cell-side update reads)
        self._accV = torch.zeros(2, K, **f64)
        self._v_sums_in_acc = False
        self._ws = engine.ZWorkspace(self.counts, K, need_sw=False, need_srow=False)     # (s_rs: allocated on first use)
        self._init_extra()
        self.U = _Buffer(lambda: self._U_hat)
        self.V = _Buffer(lambda: self._effective_V())
        self.UV = _Buffer(lambda: self._U_hat @ self._effective_V().t())          # lazy Einsum('nk,mk->nm')
        self.n_sweeps = 0
        self._graph = None
        self.initialize_parameters()

    def _dense_density(self, dense_density, cmatrix, n_total, init=None):
        """The density threshold of the hybrid layout for this model, or None."""
        if isinstance(cmatrix, engine.CountTiles):
            return None
        # 'auto' for the ZI / sparse models: the dense block is neutral for them at the benchmark's 90 % zeros and pays
        # 1.4-2 x at the reference generator's own ~50 % (profiles/r04_zigap_hybrid_ab.json, r04_sparsegap_hybrid_ab.json), so
        # they take it only when the genes above the threshold hold most of the non-zeros (decided at packing, from the
        # per-gene counts: CountTiles.dense_order min_share)
        self._dense_min_share = 0.75 if ((self.zi or self.sparse) and isinstance(dense_density, str)) else 0.0
        if isinstance(init, str) and init == 'nmf':      # the on-device NMF start walks the sliced layout only
            return None
        shape = getattr(cmatrix, 'shape', None)
        rows = int(n_total) if n_total is not None else (int(shape[0]) if shape is not None else 0)
        cols = int(shape[1]) if shape is not None else 0
        if isinstance(dense_density, str):
            if dense_density != 'auto':
                raise ValueError("dense_density must be 'auto', a density in (0, 1] or 0 / None")
            return engine.auto_dense_density(rows, cols, self.k)
        if not dense_density or not engine.dense_supported(self.k):
            return None
        return float(dense_density)

    # ---- initial shapes -------------------------------------------------------------------------
    def _initial_shapes(self, X_host, init):
        """a1, b1 before the clamp.  With ``init`` given: exactly those.  Otherwise the reference's
        host-side sequence is replayed (same np.random calls in the same order, then scikit-learn
        NMF) so that ``np.random.seed(s)`` before the constructor gives the reference's start."""
        if isinstance(init, str):
            # on-device starts (deviceinit.py): no host copy of X, sharding-invariant
            from . import deviceinit
            seed = int(getattr(self, 'seed', 0))
            row0 = deviceinit.global_row_offset(self.n, self.pg, self.device)
            if init == 'nmf':
                W, H = deviceinit.device_nmf(self.counts, self.k, seed=seed, pg=self.pg, row0=row0)
                if self.use_factors:
                    return W, H, (W, H)
                a1, b1 = deviceinit.random_shapes(self.n, self.m, self.k, seed=seed + 1, device=self.device, row0=row0)
                return a1, b1, (W, H)
            if init == 'random':
                a1, b1 = deviceinit.random_shapes(self.n, self.m, self.k, seed=seed, device=self.device, row0=row0)
                return a1, b1, None
            raise ValueError("init must be (a1, b1), 'nmf' or 'random'")
        if init is not None:
            a1, b1 = init
            a1 = a1 if isinstance(a1, torch.Tensor) else torch.as_tensor(np.asarray(a1, dtype=np.float64))
            b1 = b1 if isinstance(b1, torch.Tensor) else torch.as_tensor(np.asarray(b1, dtype=np.float64))
            if tuple(a1.shape) != (self.n, self.k) or tuple(b1.shape) != (self.m, self.k):
                raise ValueError('init shapes must be (n, k) and (m, k)')
            return a1, b1, None
        if X_host is None:
            raise ValueError("init=(a1, b1), 'nmf' or 'random' is required when the count matrix is already on the device")
        if self.world > 1:
            raise ValueError("init=(a1, b1), 'nmf' or 'random' is required under row sharding (the host NMF sees the whole matrix)")
        from .hostinit import reference_initial_shapes
        a1, b1, nmf = reference_initial_shapes(type(self).__name__, X_host, self.k, self.use_factors)
        return torch.from_numpy(a1), torch.from_numpy(b1), nmf

    def _init_extra(self):
        pass

    def _effective_V(self):
        return self._V_hat

    # ---- reference surface ------------------------------------------------------------------------
    def initialize_parameters(self):
        """base.py:43-52: variational initialisation was done in __init__; expectations; M-step."""
        self.update_expectations()
        self.update_prior_hyper_parameters()

    def step(self):
        """One CAVI sweep (base.py:54-56)."""
        if self._graph is not None:
            self._graph.replay()
        else:
            self._sweep()
        self.n_sweeps += 1

    def _sweep(self):
        self.update_variational_parameters()   # E-step
        self.update_prior_hyper_parameters()   # M-step

    def capture_graph(self):
        """Capture one sweep into a hipGraph and replay it from step() on (single process only:
        the launches of a sweep have no host-side decision, so small problems stop being
        launch-bound).  The state tensors are updated in place, exactly as without the graph."""
        if self.sharded:
            raise RuntimeError('graph capture is for single-process models (collectives are not captured)')
        if self.zi:
            # the lazy p_d of the ZI models is host-side state (snapshot + deferred evaluation) that a replayed
            # graph would not refresh: model.p_d / state() would go stale
            raise RuntimeError('graph capture is not available for the zero-inflated models (p_d is evaluated lazily on the host side)')
        if self._graph is not None:
            return self
        # (a captured sweep replays fixed buffers: the FU double buffer of the fused preparation would alternate)
        self._graph_capturing = True
        self._ws.fu_pending = False
        self._sweep()                          # warm-up: allocations, lazy scratch buffers
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._sweep()
        self.n_sweeps += 1                     # the warm-up sweep
        self._graph = g
        return self

    def fit(self, n_iter=50, tol=None, check_every=5):
        """The loop user scripts write around step() (reference main.py:37-51): `n_iter` sweeps.
        With a `tol` the variational bound decides when to stop: elbo() is evaluated after every `check_every` sweeps,
        each (n_sweeps, value) pair is appended to ``self.elbo_trace_``, and the loop ends early once
        |E_t - E_prev| <= tol * |E_t|.  tol=None: exactly the n_iter sweeps, nothing else is launched."""
        n_iter = int(n_iter)
        if tol is None:
            for _ in range(n_iter):
                self.step()
            return self
        if self._no_elbo is not None:
            raise NotImplementedError(self._no_elbo)
        tol, check_every = float(tol), int(check_every)
        if check_every < 1:
            raise ValueError('check_every must be at least 1')
        if not hasattr(self, 'elbo_trace_'):
            self.elbo_trace_ = []
        prev = None
        for it in range(1, n_iter + 1):
            self.step()
            if it % check_every == 0:
                cur = self.elbo()
                self.elbo_trace_.append((self.n_sweeps, cur))
                if prev is not None and abs(cur - prev) <= tol * abs(cur):
                    break
                prev = cur
        return self

    # The variational bound exists for pCMF only (models/gap.py).  The reference's zero-inflated and sparse updates are not
    # coordinate ascent on one stated bound: the per-gene sums are weighted with D_hat[i, k] instead of D_hat[i, j]
    # (zigap.py:94), p_d is pinned to 1 - 1e-10 at every non-zero count (zigap.py:135), and S_tilde = (p_s > tau)
    # (sparse_gap.py:113) thresholds the posterior the other updates read -- no value is non-decreasing under them.
    _no_elbo = ('elbo() is defined for pCMF (GaP) only: the zero-inflated and sparse updates of the reference (the D_hat[i, k] '
                'index of zigap.py:94, p_d pinned to 1 - 1e-10 at the non-zero counts, the tau threshold on p_s) are not '
                'coordinate ascent on one stated bound, so no such value is monotone for them')

    def elbo(self):
        """The evidence lower bound of the current variational state (GaP); NotImplementedError on the other models."""
        raise NotImplementedError(self._no_elbo)

    # Folding new cells into a fitted model exists for pCMF only (models/gap.py).  A new cell of the zero-inflated models needs
    # a dropout posterior of its own (p_d over its zeros, which the cell-side rate then reads through D_hat^T), and the sparse
    # models' responsibilities run against the masked gene images (S_tilde, S_hat): neither is transform()'s iteration.  ZIGaP has
    # fold_in() and the sparse models project() (models/zigap.py), each under a name of its own.
    _no_transform = ('transform() is defined for pCMF (GaP) only: folding a new cell into a zero-inflated model needs the dropout '
                     'posterior of that unseen cell, and the sparse models evaluate the responsibilities against masked gene '
                     'images; neither fold-in is implemented')

    def _query_counts(self, cmatrix, what='transform()'):
        """The new cells as CountTiles on the sliced layout (packed here unless they already are), gene count checked first."""
        if isinstance(cmatrix, engine.CountTiles):
            ct = cmatrix
        else:
            sparse = _is_sparse_input(cmatrix)
            if sparse:
                X = cmatrix._sparse if hasattr(cmatrix, '_sparse') else cmatrix
            else:
                X = cmatrix.as_array() if hasattr(cmatrix, 'as_array') else cmatrix
                if not isinstance(X, torch.Tensor):
                    X = np.asarray(X)
            if len(X.shape) != 2 or int(X.shape[1]) != self.m:
                raise ValueError('%s needs an (n\', %d) count matrix: the model was fitted on %d genes, got shape %s'
                                 % (what, self.m, self.m, tuple(X.shape)))
            pack = engine.CountTiles.from_scipy if sparse else engine.CountTiles.from_dense
            ct = pack(X, self.device, dense_density=None)
        if ct.m != self.m:
            raise ValueError('%s needs counts over the %d genes the model was fitted on, got %d' % (what, self.m, ct.m))
        if ct.gd:
            raise ValueError('%s walks the sliced layout only: pack the new counts without dense_density' % what)
        return ct

    def _fold_in_start(self, ct, ws, init, masks=None):
        """The a1 (n', K) float64 a fold-in of `ct` starts from: `init` (checked, copied to the device), by default
        alpha1 + rowsum(x) / K (uniform responsibilities, no RNG; `ws`: the call's workspace) -- with `masks` = (S_tilde, S_hat)
        of the sparse models uniform over each gene's unmasked factors (heldout.masked_row_sums); clamped as the sweeps clamp."""
        K, dev, nq = self.k, self.device, ct.n
        if init is not None:
            a1 = init if isinstance(init, torch.Tensor) else torch.as_tensor(np.asarray(init, dtype=np.float64))
            if tuple(a1.shape) != (nq, K):
                raise ValueError('init must be an (n\', k) array of starting shapes, got %s' % (tuple(a1.shape),))
            a1 = a1.to(device=dev, dtype=torch.float64, copy=True)
        elif nq > 0:
            Z = heldout.row_sums_over_k(ws, K) if masks is None else heldout.masked_row_sums(ws, K, *masks)
            a1 = self.alpha1.tensor[None, :] + Z.to(torch.float64)
        else:
            a1 = torch.empty(0, K, dtype=torch.float64, device=dev)
        return torch.clamp(torch.nan_to_num(a1), min=1e-15).contiguous()

    @staticmethod
    def _score_result(terms, names, signs, extras, return_terms):
        """A held-out score from its (n', 4) float64 host terms, added left to right with `signs` ('+' / '-' per term): the
        array, or with return_terms a dict of score, a copy of each term under its name and the `extras`."""
        score = terms[:, 0] if signs[0] == '+' else -terms[:, 0]
        for j in (1, 2, 3):
            score = score + terms[:, j] if signs[j] == '+' else score - terms[:, j]
        if not return_terms:
            return score
        return dict(score=score, **{name: terms[:, j].copy() for j, name in enumerate(names)}, **extras)

    @staticmethod
    def _mean_score(s):
        """The mean of a per-cell score (the array, or the dict of return_terms) as a Python float; nan for no cells."""
        if isinstance(s, dict):
            s = s['score']
        return float(s.mean()) if s.size else float('nan')

    def transform(self, cmatrix, n_iter=200, tol=1e-4, init=None, return_params=False):
        """E[U] of cells the model was not fitted on (GaP); NotImplementedError on the other models."""
        raise NotImplementedError(self._no_transform)

    # The per-cell bound of held-out cells exists for pCMF only (models/gap.py): it is a cell's share of the bound of elbo(),
    # reached by the fold-in of transform(), and the other models have no such bound (see _no_elbo above).
    _no_score = ('score_samples() / score() are defined for pCMF (GaP) only: the score is a cell\'s share of the variational bound '
                 'of elbo() after the fold-in of transform(), and the zero-inflated and sparse updates of the reference are not '
                 'coordinate ascent on one stated bound, so there is no such value to evaluate for them')

    def score_samples(self, cmatrix, n_iter=200, tol=1e-4, init=None, check_every=5, return_terms=False):
        """The per-cell variational bound of cells the model was not fitted on (GaP); NotImplementedError on the other models."""
        raise NotImplementedError(self._no_score)

    def score(self, cmatrix, **kw):
        """The mean of score_samples() (GaP); NotImplementedError on the other models."""
        raise NotImplementedError(self._no_score)

    # Streaming updates from cell batches exist for pCMF only (models/gap.py): the global step is a natural-gradient step on the
    # bound of elbo(), and the other models' sweeps ascend no single bound (see _no_elbo above).
    _no_partial_fit = ('partial_fit() is defined for pCMF (GaP) only: its global step is a natural-gradient step on the variational '
                       'bound of elbo(), and the zero-inflated and sparse updates of the reference are not coordinate ascent on '
                       'one stated bound, so there is no such gradient to follow for them')

    def partial_fit(self, cmatrix, n_total, rho=None, tau0=1.0, kappa=0.7, n_iter=200, tol=1e-4, init=None, check_every=5):
        """One stochastic variational update of the gene side from a batch of cells (GaP); NotImplementedError on the other
        models."""
        raise NotImplementedError(self._no_partial_fit)

    def factors(self):
        """base.py:97-98: (U[:], V[:]) as host arrays."""
        return self.U[:], self.V[:]

    # expectations as host NumPy (the reference stores ndarrays in these attributes)
    @property
    def U_hat(self):
        return self._U_hat.cpu().numpy()

    @property
    def V_hat(self):
        return self._V_hat.cpu().numpy()

    @property
    def log_U_hat(self):
        return self._log_U_hat.cpu().numpy()

    @property
    def log_V_hat(self):
        return self._log_V_hat.cpu().numpy()

    # ---- pieces shared by the four models ----------------------------------------------------------
    _ver = 0

    def _touch(self):
        """Counts the writes to the expectations a product kept across sweeps depends on (V_hat, S_hat, D_hat)."""
        self._ver += 1

    def _gamma_side(self, side, Z, zmul=None, rate_vec=None, rate_mat=None, rmul=None, update=True, sums_arg=None, zero=True):
        """One side of update_variational_parameters + Gamma.mean / meanlog (oriana_gamma_update).  `sums_arg`: where the
        column sums go (default: _sumU / _sumV); zero=False: they are zero already."""
        if side == 'v':
            self._touch()
        if side == 'u':
            s1, s2, E, Elog, sums, p1, p2, r = self.a1, self.a2, self._U_hat, self._log_U_hat, self._sumU, self.alpha1, self.alpha2, self.n
        else:
            s1, s2, E, Elog, sums, p1, p2, r = self.b1, self.b2, self._V_hat, self._log_V_hat, self._sumV, self.beta1, self.beta2, self.m
        if sums_arg is not None:
            sums = sums_arg
        if zero:
            sums.zero_()
        prep = self._prep_outputs(side, packed_rows=False)
        call('oriana_gamma_update_prep', ptr(s1.tensor), ptr(s2.tensor), ptr(E), ptr(Elog), ptr(sums[0]), ptr(sums[1]),
             ptr(p1.tensor), ptr(p2.tensor), ptr(Z) if update else None, ptr(zmul), ptr(rate_vec), ptr(rate_mat),
             ptr(rmul), r, self.k, ptr(prep[0]), ptr(prep[1]), ptr(prep[2]), stream_ptr())
        if prep[0] is not None:
            self._ws.fu_pending, self._ws.fu_source = True, Elog.data_ptr()

    def _prep_outputs(self, side, packed_rows):
        """The cell-side update also prepares the next sweep's FU (engine.ZWorkspace.prep_outputs); any update of E[log U]
        invalidates what an earlier one prepared."""
        if side != 'u' or getattr(self, '_ws', None) is None:
            return (None, None, None)
        self._ws.fu_pending = False
        if self._graph_capturing:
            return (None, None, None)
        return self._ws.prep_outputs(packed_rows) or (None, None, None)

    def _gamma_side_finalize(self, side, Z, F, R, row_index, rate_vec, sums, nslab=1, slab_row0=0, a2_row=None):
        """pCMF: Z += F * R (the last step of the responsibility pass, packed rows scattered through `row_index`) and the
        Gamma update of that side in one launch (oriana_gamma_update_finalize).  `sums` (2, K) must be zero on entry.
        `a2_row` (cell side, [r6]): the rate matrix a2 and the mean U_hat are NOT stored -- the K rate values go to a2_row
        (oriana_gamma_update_finalize_lazy); returns True when that form ran, False when the full form did."""
        if side == 'v':
            self._touch()
        prep = self._prep_outputs(side, packed_rows=True)
        if a2_row is not None:
            assert side == 'u'
            from .. import _lib
            rc = _lib.load().oriana_gamma_update_finalize_lazy(
                ptr(self.a1.tensor), ptr(a2_row), ptr(self._log_U_hat), ptr(sums[0]), ptr(sums[1]), ptr(self.alpha1.tensor),
                ptr(self.alpha2.tensor), ptr(Z), ptr(F), ptr(R), int(nslab), int(slab_row0), ptr(row_index), ptr(rate_vec), self.n,
                self.k, ptr(prep[0]), ptr(prep[1]), ptr(prep[2]), stream_ptr())
            if rc == 0:
                if prep[0] is not None:
                    self._ws.fu_pending, self._ws.fu_source = True, self._log_U_hat.data_ptr()
                return True
            if rc != -2:                    # ORIANA_EKRANGE: no vector kernel for this K -- the full form below
                raise OrianaHipError('oriana_gamma_update_finalize_lazy failed with code %d' % rc)
        if side == 'u':
            s1, s2, E, Elog, p1, p2, r = self.a1, self.a2, self._U_hat, self._log_U_hat, self.alpha1, self.alpha2, self.n
        else:
            s1, s2, E, Elog, p1, p2, r = self.b1, self.b2, self._V_hat, self._log_V_hat, self.beta1, self.beta2, self.m
        call('oriana_gamma_update_finalize_prep', ptr(s1.tensor), ptr(s2.tensor), ptr(E), ptr(Elog), ptr(sums[0]), ptr(sums[1]),
             ptr(p1.tensor), ptr(p2.tensor), ptr(Z), ptr(F), ptr(R), int(nslab), int(slab_row0), ptr(row_index), ptr(rate_vec), r,
             self.k, ptr(prep[0]), ptr(prep[1]), ptr(prep[2]), stream_ptr())
        if prep[0] is not None:
            self._ws.fu_pending, self._ws.fu_source = True, Elog.data_ptr()
        return False

    def _mstep_side(self, side):
        if side == 'u':
            call('oriana_mstep_gamma', ptr(self.alpha1.tensor), ptr(self.alpha2.tensor), ptr(self._sumU[0]),
                 ptr(self._sumU[1]), float(self.n_total), self.k, stream_ptr())
        else:
            call('oriana_mstep_gamma', ptr(self.beta1.tensor), ptr(self.beta2.tensor), ptr(self._sumV[0]),
                 ptr(self._sumV[1]), float(self.m), self.k, stream_ptr())

    def update_expectations(self):
        """gap.py:131-135: expectations from the current a1, a2, b1, b2 (no parameter update)."""
        self._gamma_side('u', None, update=False)
        odist.all_reduce_sum(self._sumU, self.pg)
        self._gamma_side('v', None, update=False)
        self._v_sums_in_acc = False

    def update_prior_hyper_parameters(self):
        """gap.py:117-129: both Gamma nodes in one launch."""
        acc = self._v_sums_in_acc
        sv = self._accV if acc else self._sumV
        call('oriana_mstep_gamma_pair', ptr(self.alpha1.tensor), ptr(self.alpha2.tensor), ptr(self._sumU[0]),
             ptr(self._sumU[1]), float(self.n_total), ptr(self.beta1.tensor), ptr(self.beta2.tensor), ptr(sv[0]), ptr(sv[1]),
             float(self.m), ptr(self._sumV) if acc else None, self.k, stream_ptr())
        self._v_sums_in_acc = False

    def update_variational_parameters(self):
        raise NotImplementedError

    def _exchange_start(self, **partials64):
        """First half of the sweep's exchange, called BEFORE the column pass: the float64 partials that already exist
        (the cell-side column sums, D_hat^T U_hat of the ZI models) start their all-reduce asynchronously and the
        column pass runs under it."""
        x = self._xch
        x.put64('sumU', self._sumU)
        for name, t in partials64.items():
            x.put64(name, t)
        x.start64()
        self._xch_names = tuple(partials64)

    def _exchange(self, **partials64):
        """The exchange of a sweep: the float32 buffer (per-gene sums written in place by the column pass) and the
        float64 partials (started by _exchange_start, or handed in here) are summed over the row shards.  Returns the
        reduced float64 partials by name."""
        x = self._xch
        names = getattr(self, '_xch_names', None)
        if names is None:
            x.put64('sumU', self._sumU)
            for name, t in partials64.items():
                x.put64(name, t)
            names = tuple(partials64)
        self._xch_names = None
        x.reduce()
        x.get64('sumU', out=self._sumU)
        return {name: x.get64(name) for name in names}

    # ---- metrics (reference base.py:58-87; loglikelihood_X: sparse_zigap.py:44-51) --------------------
    # The reference defines loglikelihood_X on SparseZIGaP only (the deviances raise AttributeError on
    # the other classes); here the absent nodes read as the constants the formulas reduce to
    # (pi_d = 1, D = 1, S_hat = 1).  With N = {X != 0}, Z = {X == 0}, M = {round(D_hat) == 0} (M never
    # meets N: D_hat = 1 at the non-zeros), Lambda = U_hat (S_hat * V_hat)^T and mu_j = mean_i X_ij:
    #   ll(X | X)      = sum_j nnz_j log pi_j + sum_N (x log x - x)                  (zeros give log 1 = 0)
    #   ll(X | Lambda) = sum_{Z - M} log(pi_j e^-Lambda + 1 - pi_j) + sum_j nnz_j log pi_j
    #                    - sum_N Lambda + sum_N x log Lambda
    #   ll(X | mu)     = sum_j (n - nnz_j) log(pi_j e^-mu_j + 1 - pi_j) + sum_j nnz_j (log pi_j - mu_j)
    #                    + sum_j colsum_j log mu_j
    # The sums over N come from the responsibility kernels (metrics.hip), the sum over Z - M from the
    # f64-MFMA kernel of the D update in metric mode (or, without a D node, from column sums:
    # sum_Z Lambda = sum_k (sum_i U_ik)(sum_j V_jk) - sum_N Lambda).  Float64 semantics: what the
    # reference computes for a float X (for an integer X it truncates every term, sparse_zigap.py:45).
    def _count_constants(self):
        """Per-gene sums / non-zero counts of X and sum_N (x log x - x), sum_N x^2 (all-reduced, cached)."""
        if getattr(self, '_xconst', None) is None:
            dev = self.device
            colsum = torch.zeros(self.m, dtype=torch.float64, device=dev)
            colnnz = torch.zeros(self.m, dtype=torch.float64, device=dev)
            out2 = torch.zeros(2, dtype=torch.float64, device=dev)
            ct = self.counts
            call('oriana_count_stats', ct.sparse_struct, ptr(colsum), ptr(colnnz), ptr(out2), stream_ptr())
            if ct.dense is not None:
                call('oriana_dense_metric', ct.dense.c_struct, None, None, ptr(ct.row_perm), ptr(ct.col_perm), ptr(colsum),
                     ptr(colnnz), ptr(out2), None, self.k, stream_ptr())
            for t in (colsum, colnnz, out2):
                odist.all_reduce_sum(t, self.pg)
            self._xconst = (colsum, colnnz, out2)
        return self._xconst

    def _rate_pass(self):
        """The row pass over float32 casts of U_hat, V_eff: leaves s = x / Lambda in the row-side slots (ws.s_rs), the rate every
        sum over the stored entries reads.  Returns the float64 (U, V) the fall-back entries are recomputed from."""
        ct, K, n, m, dev = self.counts, self.k, self.n, self.m, self.device
        st = stream_ptr()
        U, V = self._U_hat, self._effective_V().contiguous()
        ws = self._ws
        FU, FV = ws.extra('MU', n), ws.extra('MV', m)
        call('oriana_factor_cast_f32', ptr(FU), ptr(U), None, ptr(ct.row_perm), n, K, st)
        call('oriana_factor_cast_f32', ptr(FV), ptr(V), None, ptr(ct.col_perm), m, K, st)
        if ws.s_rs is None:
            ws.s_rs = torch.zeros(max(ct.rslots, 1), dtype=torch.float32, device=dev)
        ws.tile_flag.zero_()
        # with these factors the row pass leaves s = x / Lambda in the row-side slots
        # (hybrid layout: the sliced part covers the packed genes [gd, m); the dense genes are summed in float64)
        call('oriana_row_pass', ct.sparse_struct, ptr(FU), ptr(FV) + 4 * ct.gd * ws.Kp, None, ptr(ws.R), ptr(ws.s_cs), None,
             ptr(ws.s_rs), ptr(ws.tile_flag), K, st)
        return U, V

    def _metric_terms(self):
        ct, K, n, m, dev = self.counts, self.k, self.n, self.m, self.device
        st = stream_ptr()
        ws = self._ws
        U, V = self._rate_pass()
        nz = torch.zeros(4, dtype=torch.float64, device=dev)      # sum Lambda, sum x log Lambda, sum Lambda^2, sum x Lambda
        call('oriana_metric_nnz', ct.sparse_struct, ptr(ws.s_rs), ptr(U), ptr(V), K, ptr(nz), st)
        if ct.dense is not None:
            call('oriana_dense_metric', ct.dense.c_struct, ptr(U), ptr(V), ptr(ct.row_perm), ptr(ct.col_perm), None, None, None,
                 ptr(nz), K, st)
        zz = torch.zeros(2, dtype=torch.float64, device=dev)      # over Z - M: sum log(pi e^-Lambda + 1 - pi), sum Lambda^2
        if self.zi:
            # (the gene axis of the dropout node's matrices is padded with inert genes to a multiple of 4, zigap.py _init_zi:
            # pi_d = 0 there, so log(pi e^-Lambda + 1 - pi) = 0, and Lambda = 0)
            call('oriana_dropout_metric', ptr(zz), ptr(self._Dp), ptr(U), ptr(self._padG(V, 'Vm')), ptr(self._padG(self.pi_d.tensor, 'pim')),
                 ptr(self._nzmask), n, self._mp, K, st)
            odist.all_reduce_sum(zz, self.pg)
            odist.all_reduce_sum(nz, self.pg)
        else:
            su = U.sum(0)
            gram_u = U.t() @ U
            packed = torch.cat([nz, su, gram_u.reshape(-1)])
            odist.all_reduce_sum(packed, self.pg)
            nz, su, gram_u = packed[:4], packed[4:4 + K], packed[4 + K:].reshape(K, K)
            all_lam = (su * V.sum(0)).sum()
            all_lam2 = (gram_u * (V.t() @ V)).sum()
            zz[0] = -(all_lam - nz[0])
            zz[1] = all_lam2 - nz[2]
        return nz, zz

    def _log_pi(self):
        if self.zi:
            return torch.log(self.pi_d.tensor), self.pi_d.tensor
        one = torch.ones(self.m, dtype=torch.float64, device=self.device)
        return torch.zeros_like(one), one

    def _gene_ll_terms(self):
        """Per gene, what the log-likelihoods hold apart from the rate matrix (device float64, global under row sharding):
        lpi = log pi_j, mu = the mean count, t = log(pi e^-mu + 1 - pi) (one zero's term of ll(X | mean)), log_mu (0 for a gene
        without counts), nnz_lpi = nnz_j log pi_j and the gene's share of ll(X | mean)."""
        colsum, colnnz, _ = self._count_constants()
        lpi, pi = self._log_pi()
        has = colnnz > 0
        nnz_lpi = torch.where(has, colnnz * lpi, torch.zeros_like(lpi))
        ntot = float(self.n_total)
        mu = colsum / ntot
        # log(pi e^-mu + 1 - pi) as a log-sum-exp.  Without a dropout node (pi = 1) the literal form is log e^-mu, which
        # underflows to log 0 = -inf once mu passes ~745: -inf for such a gene with a zero among its counts, 0 * -inf = NaN
        # for one without, and explained_deviance NaN either way.  (With pi <= 1 - 1e-10 the 1 - pi keeps it finite.)
        t = torch.logaddexp(lpi - mu, torch.log1p(-pi))
        log_mu = torch.log(torch.where(has, mu, torch.ones_like(mu)))
        zero_term = (ntot - colnnz) * t
        nz_term = torch.where(has, colnnz * (lpi - mu) + colsum * log_mu, torch.zeros_like(mu))
        return dict(lpi=lpi, mu=mu, t=t, log_mu=log_mu, has=has, nnz_lpi=nnz_lpi, mean=zero_term + nz_term)

    def _ll_constants(self):
        """What the log-likelihoods hold apart from the rate matrix: sum_j nnz_j log pi_j, ll(X | X), ll(X | mean) (device
        scalars) and the count constants."""
        xc = self._count_constants()[2]
        g = self._gene_ll_terms()
        nnz_lpi = g['nnz_lpi'].sum()
        ll_x = nnz_lpi + xc[0]
        ll_mean = g['mean'].sum()
        return nnz_lpi, ll_x, ll_mean, xc

    def _loglikelihoods(self):
        nnz_lpi, ll_x, ll_mean, xc = self._ll_constants()
        nz, zz = self._metric_terms()
        ll_uv = zz[0] + nnz_lpi - nz[0] + nz[1]
        return float(ll_x), float(ll_uv), float(ll_mean), nz, zz, xc

    def loglikelihood_X(self, given='factors'):
        """The zero-inflated Poisson log-likelihood of the counts (reference sparse_zigap.py:44-51) for the three Poisson
        means the reference's metrics put into the UV node before calling it: 'factors' -- Lambda = U_hat (S_hat * V_hat)^T,
        zeroed where round(D_hat) == 0 (base.py:64-68: the buffer reconstruction_deviance leaves behind, i.e. what a call
        after it returns); 'counts' -- Lambda = X (base.py:59-63); 'mean' -- Lambda = the per-gene mean (base.py:76-77)."""
        ll_x, ll_uv, ll_mean, _, _, _ = self._loglikelihoods()
        try:
            return {'factors': ll_uv, 'counts': ll_x, 'mean': ll_mean}[given]
        except KeyError:
            raise ValueError("given must be 'factors', 'counts' or 'mean'") from None

    def reconstruction_deviance(self):
        """-2 (ll(X | U_hat V_hat^T) - ll(X | X)), reference base.py:58-69."""
        ll_x, ll_uv, _, _, _, _ = self._loglikelihoods()
        return -2.0 * (ll_uv - ll_x)

    def explained_deviance(self):
        """(ll(X | U_hat V_hat^T) - ll(X | mean)) / (ll(X | X) - ll(X | mean)), reference base.py:71-82
        evaluated on the current expectations (the reference reads the node buffers its own
        reconstruction_deviance call left behind, experiments/clustering.py:26-27)."""
        ll_x, ll_uv, ll_mean, _, _, _ = self._loglikelihoods()
        return (ll_uv - ll_mean) / (ll_x - ll_mean)

    def frobenius_norm(self):
        """|| Lambda - X ||_F with Lambda = U_hat V_hat^T, zeroed where round(D_hat) == 0 (reference
        base.py:84-87 on the UV buffer the deviance calls leave behind)."""
        _, _, _, nz, zz, xc = self._loglikelihoods()
        # sum_N (Lambda - x)^2 + sum_{Z - M} Lambda^2
        return float(torch.sqrt(torch.clamp(nz[2] - 2.0 * nz[3] + xc[1] + zz[1], min=0.0)))

    # ---- the deviance per gene and per cell ---------------------------------------------------------------
    # The three log-likelihoods above are sums over the entries (i, j); kept per gene j (summed over the cells) or per cell i
    # (summed over the genes), in the notation above _count_constants and with t_j = log(pi_j e^-mu_j + 1 - pi_j):
    #   factors: x != 0: log pi_j - Lambda_ij + x log Lambda_ij     x == 0, not in M: log(pi_j e^-Lambda_ij + 1 - pi_j)    in M: 0
    #   counts : x != 0: log pi_j + x log x - x                     x == 0: 0
    #   mean   : x != 0: log pi_j - mu_j + x log mu_j               x == 0: t_j
    # The sums over the non-zeros of a gene / a cell come from oriana_metric_nnz_axes (oriana_dense_metric_axes for the dense
    # genes of a hybrid layout) behind the same row pass as _metric_terms, the zero term of a dropout node from
    # oriana_dropout_metric_axes.  Without a dropout node the zero term is -Lambda and needs no pass: per gene
    # factors_j = -(V_eff su)_j + sum_{N_j} x log Lambda (su the column sums of U_hat), per cell -(U_hat sv)_i + sum_{N_i} ...
    # Per cell the mean's sum over ALL genes is sum_j t_j + sum_{N_i} (c1_j + x c2_j), c1_j = log pi_j - mu_j - t_j,
    # c2_j = log mu_j: the kernels read {log pi_j, c1_j, c2_j} per gene.  A gene without a count has mean 0, and its t_j is
    # log 1 = 0 exactly (the log-sum-exp of _gene_ll_terms may leave an ulp there): counts_j = mean_j = 0.
    def _axis_terms(self, genes, cells):
        """(factors, counts, mean) as host float64 arrays for the gene axis (m,), the cell axis (n_local,) or both: a dict
        with 'genes' / 'cells'.  Only the requested axis is computed.  Under row sharding the gene arrays are summed over the
        ranks in one packed all-reduce; the cell arrays are this rank's rows against the global per-gene mean."""
        ct, K, n, m, dev = self.counts, self.k, self.n, self.m, self.device
        if self.zi and K > 256:
            raise ValueError('gene_deviance() / cell_deviance() with a dropout node need k <= 256')
        st, ws = stream_ptr(), self._ws
        g = self._gene_ll_terms()
        zero = torch.zeros_like(g['t'])
        t = torch.where(g['has'], g['t'], zero)
        nnz_lpi = g['nnz_lpi']
        U, V = self._rate_pass()
        gene_out = torch.zeros(max(m, 1), 3, dtype=torch.float64, device=dev) if genes else None
        cell_out = torch.zeros(max(n, 1), 5, dtype=torch.float64, device=dev) if cells else None
        gconst = torch.stack([g['lpi'], g['lpi'] - g['mu'] - t, g['log_mu']], dim=1).contiguous() if cells else None
        call('oriana_metric_nnz_axes', ct.sparse_struct, ptr(ws.s_rs), ptr(U), ptr(V), K, ptr(gconst), ptr(gene_out),
             ptr(cell_out), st)
        if ct.dense is not None:
            call('oriana_dense_metric_axes', ct.dense.c_struct, ptr(U), ptr(V), ptr(ct.row_perm), ptr(ct.col_perm), K,
                 ptr(gconst), ptr(gene_out), ptr(cell_out), st)
        zg = zc = None
        if self.zi:
            # (the padded gene axis of the dropout node's matrices, as in _metric_terms: pi_d = 0 there, the term is 0)
            zg = torch.zeros(self._mp, dtype=torch.float64, device=dev) if genes else None
            zc = torch.zeros(max(n, 1), dtype=torch.float64, device=dev) if cells else None
            call('oriana_dropout_metric_axes', ptr(zg), ptr(zc), ptr(self._Dp), ptr(U), ptr(self._padG(V, 'Vm')),
                 ptr(self._padG(self.pi_d.tensor, 'pim')), ptr(self._nzmask), n, self._mp, K, st)
        out = {}
        if genes:
            packed = torch.cat([gene_out[:m].reshape(-1), zg[:m] if self.zi else U.sum(0)])
            odist.all_reduce_sum(packed, self.pg)
            go, tail = packed[:3 * m].reshape(m, 3), packed[3 * m:]
            if self.zi:
                factors = tail + nnz_lpi - go[:, 0] + go[:, 1]
            else:                              # sum_i Lambda_ij = (V_eff su)_j: sum_N Lambda cancels against the zero term
                factors = -(V @ tail) + nnz_lpi + go[:, 1]
            counts = nnz_lpi + go[:, 2]
            mean = torch.where(g['has'], g['mean'], zero)
            out['genes'] = tuple(a.cpu().numpy() for a in (factors, counts, mean))
        if cells:
            co = cell_out[:n]
            if self.zi:
                factors = zc[:n] + co[:, 3] - co[:, 0] + co[:, 1]
            else:
                factors = -(U @ V.sum(0)) + co[:, 3] + co[:, 1]
            counts = co[:, 3] + co[:, 2]
            mean = t.sum() + co[:, 4]
            out['cells'] = tuple(a.cpu().numpy() for a in (factors, counts, mean))
        return out

    @staticmethod
    def _axis_result(factors, counts, mean):
        with np.errstate(divide='ignore', invalid='ignore'):
            return {'factors': factors, 'counts': counts, 'mean': mean,
                    'reconstruction_deviance': -2.0 * (factors - counts),
                    'explained_deviance': (factors - mean) / (counts - mean)}

    def gene_deviance(self):
        """The deviance metrics per gene: a dict of (m,) float64 arrays in the caller's gene order.  'factors', 'counts',
        'mean': each gene's share of loglikelihood_X(given=...) (they sum to it, up to the order of the additions);
        'reconstruction_deviance' = -2 (factors - counts) and 'explained_deviance' = (factors - mean) / (counts - mean) per
        gene, the literal float64 values: a gene without a count has counts = mean = 0 and gives a non-finite value (NaN when
        its rate is 0 as well), a rate that is exactly 0 at a non-zero count -inf (+inf) for that gene alone.  Under row
        sharding every rank returns the same arrays.  Nothing of the model's state is written.  With a dropout node: k <= 256."""
        return self._axis_result(*self._axis_terms(True, False)['genes'])

    def cell_deviance(self):
        """gene_deviance() along the other axis: a dict of (n_local,) float64 arrays in the caller's row order, each cell's
        share of the three log-likelihoods (against the global per-gene mean under row sharding) and the two deviances of
        the cell.  A cell without a count has counts = 0 and a finite explained deviance."""
        return self._axis_result(*self._axis_terms(False, True)['cells'])

    # ---- the deviance along a prefix of the factors ------------------------------------------------------
    # The columns of U_hat / V_hat come out in the arbitrary order of the start.  With an order o of the factors and
    # Lambda^(k) = sum_{l < k} U_hat[:, o_l] V_eff[:, o_l]^T (V_eff = _effective_V()), everything else as the full metric has it
    # (pi_d, the mask M, ll(X | X), ll(X | mean)), in the notation above _count_constants:
    #   ll_uv^(k) = zz0^(k) + sum_j nnz_j log pi_j - sum_N Lambda^(k) + sum_N x log Lambda^(k)
    #   ed^(k) = (ll_uv^(k) - ll_mean) / (ll_x - ll_mean),   rd^(k) = -2 (ll_uv^(k) - ll_x)
    # zz0^(k) = sum_{Z - M} log(pi_j e^-Lambda^(k) + 1 - pi_j).  Without a dropout node it is -sum_Z Lambda^(k), so
    # zz0^(k) - sum_N Lambda^(k) = -sum_{l < k} su_l sv_l from the permuted column sums; with one it is a call of
    # oriana_dropout_metric on the first k permuted columns per requested k.  The two sums over N for ALL requested k come from
    # one walk over the stored counts (oriana_metric_nnz_prefix, oriana_dense_metric_prefix for the dense genes of a hybrid
    # layout): the full metric's route through the row pass (s = x / Lambda) yields Lambda only as a whole.
    def factor_order(self):
        """The factors by decreasing mass (sum_i U_hat_ik)(sum_j V_eff_jk), V_eff = S_hat * V_hat on the sparse models: an int64
        permutation of range(K), ties by index.  The cell sums are summed over the row shards: every rank returns the same
        order."""
        from .. import prefix
        su = self._U_hat.sum(0)
        odist.all_reduce_sum(su, self.pg)
        sv = self._effective_V().sum(0)
        return prefix.order_by_mass(su.cpu().numpy(), sv.cpu().numpy())

    def deviance_path(self, order=None, ks=None):
        """explained_deviance() / reconstruction_deviance() of the fitted model restricted to the first k factors of `order`,
        for every k of `ks`, from one pass over the stored counts.

        order : a permutation of range(K) (default: factor_order()).  ks : strictly increasing prefix lengths within 1..K
        (default: 1..K).  Anything else raises ValueError before a launch.  Returns a dict: 'order', 'k' (int64) and
        'explained_deviance', 'reconstruction_deviance' (float64, one value per k): entry t is what the two metrics would return
        if the model had only the factors order[:k_t].  A prefix whose rate is exactly 0 at a non-zero count (masked factors of
        a sparse model) gives -inf (+inf for the reconstruction deviance) for that k alone.  Nothing of the model's state is
        written.

        Cost: the pass over the non-zero counts takes all k at once, one logarithm per count and k.  With a dropout node
        (ZIGaP, SparseZIGaP; K <= 256) the zero term is one dense n x m pass PER requested k: pass a handful of `ks` at scale
        rather than the default."""
        from .. import prefix
        K, n, m, dev = self.k, self.n, self.m, self.device
        order = prefix.check_order(order, K) if order is not None else None
        ks = prefix.check_ks(ks, K)
        if self.zi and K > 256:
            raise ValueError('deviance_path() with a dropout node needs k <= 256')
        if order is None:
            order = self.factor_order()
        ct, ws, st, E = self.counts, self._ws, stream_ptr(), int(ks.size)
        idx = torch.as_tensor(order, device=dev)
        U = self._U_hat.index_select(1, idx).contiguous()
        V = self._effective_V().index_select(1, idx).contiguous()
        ends = torch.as_tensor(ks, dtype=torch.int32, device=dev)
        FU, FV = ws.extra('MU', n), ws.extra('MV', m)
        call('oriana_factor_cast_f32', ptr(FU), ptr(U), None, ptr(ct.row_perm), n, K, st)
        call('oriana_factor_cast_f32', ptr(FV), ptr(V), None, ptr(ct.col_perm), m, K, st)
        nz = torch.zeros(E, 2, dtype=torch.float64, device=dev)     # per k: sum_N Lambda^(k), sum_N x log Lambda^(k)
        # (hybrid layout: the sliced part covers the packed genes [gd, m), as in _metric_terms)
        call('oriana_metric_nnz_prefix', ct.sparse_struct, ptr(FU), ptr(FV) + 4 * ct.gd * ws.Kp, ptr(U), ptr(V), K, ptr(ends), E,
             ptr(nz), st)
        if ct.dense is not None:
            call('oriana_dense_metric_prefix', ct.dense.c_struct, ptr(U), ptr(V), ptr(ct.row_perm), ptr(ct.col_perm), K, ptr(ends),
                 E, ptr(nz), st)
        if self.zi:
            zz = torch.zeros(E, 2, dtype=torch.float64, device=dev)
            Vp = torch.zeros(self._mp, K, dtype=torch.float64, device=dev)      # (the inert genes of the padded gene axis)
            Vp[:m].copy_(V)
            pim = self._padG(self.pi_d.tensor, 'pim')
            for t, k in enumerate(ks.tolist()):
                Uk, Vk = U[:, :k].contiguous(), Vp[:, :k].contiguous()
                call('oriana_dropout_metric', ptr(zz[t]), ptr(self._Dp), ptr(Uk), ptr(Vk), ptr(pim), ptr(self._nzmask), n,
                     self._mp, k, st)
            tail = zz[:, 0]
        else:
            tail = U.sum(0)
        packed = torch.cat([nz.reshape(-1), tail])
        odist.all_reduce_sum(packed, self.pg)
        nnz_lpi, ll_x, ll_mean, _ = self._ll_constants()
        packed = packed.cpu().numpy()
        nz, tail = packed[:2 * E].reshape(E, 2), packed[2 * E:]
        if self.zi:
            ll_uv = tail + float(nnz_lpi) - nz[:, 0] + nz[:, 1]
        else:                                  # zz0^(k) - sum_N Lambda^(k) = -sum_{l < k} su_l sv_l
            all_lam = np.cumsum(tail * V.sum(0).cpu().numpy())
            ll_uv = -all_lam[ks - 1] + float(nnz_lpi) + nz[:, 1]
        return prefix.assemble_path(order, ks, ll_uv, float(ll_x), float(ll_mean))

    # ---- clustering the cells (the last step of the reference's pipeline, experiments/clustering.py) -----------------
    def cluster_cells(self, n_clusters, features='log_mean', factors=None, **kmeans_kw):
        """k-means of the cells on the fitted cell factors, on the device (cluster.kmeans; its keywords pass through).

        features : 'log_mean' -- float32(log(U_hat)), the logarithm taken in float64: the reference's ``np.log(U)``; 'mean_log' --
            the model's own float32 E[log U].  factors : an optional index array of the columns to use, for example
            ``model.factor_order()[:k]``.  Returns the dict of cluster.kmeans plus 'features' (the (n_local, d) float32 matrix that
            was clustered, NumPy) and 'factors' (the column indices, int64).  Under row sharding the model's process group is used:
            every rank returns the same centres and its own rows' labels.  Nothing of the model's state is written."""
        from .. import cluster
        cols = self._cell_feature_columns(features, factors)
        if 'pg' in kmeans_kw:
            raise ValueError('cluster_cells() uses the process group of the model')
        F = self._cell_features(features, cols)
        out = cluster.kmeans(F, n_clusters, pg=self.pg, **kmeans_kw)
        out['features'] = F.cpu().numpy()
        out['factors'] = cols
        return out

    def integrate_cells(self, batch, features='log_mean', factors=None, as_tensor=False, **harmony_kw):
        """Harmony batch correction of the feature matrix cluster_cells() uses, on the device (cluster.harmony; its keywords pass
        through).  batch : (n,) integers within [0, B), the sample of origin of every cell, every batch present.

        Returns the dict of cluster.harmony plus 'features' (the (n, d) float32 matrix that was corrected) and 'factors' (the
        column indices, int64); 'corrected', 'responsibilities', 'centers' and 'features' are NumPy arrays, or with
        ``as_tensor=True`` device tensors, so that ``out['corrected']`` feeds cluster.knn, cluster.kmeans, cluster.tsne,
        cluster.snn_graph + cluster.louvain and cluster.diffusion_* without a host copy.  A model sharded over more than one rank
        raises NotImplementedError.  Nothing of the model's state is written."""
        from .. import cluster
        if odist.world_size(self.pg) > 1:
            raise NotImplementedError('integrate_cells() does not shard the cells: fit on one rank, or gather the features')
        cols = self._cell_feature_columns(features, factors)
        if 'pg' in harmony_kw:
            raise ValueError('integrate_cells() uses the process group of the model')
        F = self._cell_features(features, cols)
        out = cluster.harmony(F, batch, pg=self.pg, **harmony_kw)
        out['features'] = F
        out['factors'] = cols
        if not as_tensor:
            for key in ('corrected', 'responsibilities', 'centers', 'features'):
                out[key] = out[key].cpu().numpy()
        return out

    def _cell_feature_columns(self, features, factors):
        """The validated `features` / `factors` arguments of cluster_cells() and cell_neighbors(): the column indices, int64."""
        if features not in ('log_mean', 'mean_log'):
            raise ValueError("features must be 'log_mean' or 'mean_log'")
        cols = np.arange(self.k, dtype=np.int64) if factors is None else np.asarray(factors)
        if cols.ndim != 1 or cols.size < 1 or cols.dtype.kind not in 'iu' or cols.min() < 0 or cols.max() >= self.k:
            raise ValueError('factors must be a non-empty 1-D array of column indices within [0, %d)' % self.k)
        return cols.astype(np.int64)

    def _cell_features(self, features, cols, U=None):
        """The (n_local, len(cols)) float32 feature matrix of the fitted cells, or with `U` ((n_q, K) float64 device tensor of
        E[U] rows of other cells, 'log_mean' only) of those."""
        if U is not None:
            F = torch.log(U).to(torch.float32)
        elif features == 'log_mean':
            F = torch.log(self.U.buffer).to(torch.float32)          # (the accessor factors() reads: a lazy U_hat is evaluated)
        else:
            F = self._log_U_hat
        return F.index_select(1, torch.as_tensor(cols, device=self.device)).contiguous()

    def cell_neighbors(self, n_neighbors=15, features='log_mean', factors=None, queries=None, **knn_kw):
        """The exact k-nearest-neighbour graph of the cells on the feature matrix cluster_cells() uses, on the device (cluster.knn;
        its keywords candidate_chunk and blocks pass through).

        Without `queries` every fitted cell gets its n_neighbors nearest OTHER cells (a cell is never its own neighbour; an
        identical cell is, at distance 0).  queries : an (n_q, K) array or tensor of E[U] rows of other cells -- what
        transform() / fold_in() / project() return; they go through the same float64 logarithm, float32 cast and column
        selection and are searched against the fitted cells, nothing excluded; defined for features='log_mean' only.
        Returns NumPy arrays: 'indices' (n_q, n_neighbors) int32 global cell indices and 'sq_distances' float32, each row ordered
        by (distance, index) and padded with -1 / inf where fewer cells exist; 'features' (the (n_local, d) float32 matrix that
        was searched) and 'factors' as cluster_cells() returns them.  Under row sharding the model's process group is used: every
        rank returns the rows of its own cells (or of its own queries), the candidates are all ranks' cells.  Nothing of the
        model's state is written."""
        from .. import cluster
        cols = self._cell_feature_columns(features, factors)
        if 'pg' in knn_kw:
            raise ValueError('cell_neighbors() uses the process group of the model')
        if 'exclude_self' in knn_kw:
            raise ValueError('cell_neighbors() excludes a cell from its own list exactly when queries is None')
        if int(n_neighbors) < 1:
            raise ValueError('n_neighbors must be at least 1')
        Qf = None
        if queries is not None:
            if features != 'log_mean':
                raise ValueError("queries are rows of E[U]: they are defined for features='log_mean' only")
            q = queries.detach().cpu().numpy() if isinstance(queries, torch.Tensor) else queries
            q = np.asarray(q, dtype=np.float64)
            if q.ndim != 2 or q.shape[1] != self.k:
                raise ValueError('queries must be (n_q, %d), got %s' % (self.k, q.shape))
            if not (np.isfinite(q).all() and (q > 0).all()):
                raise ValueError('queries must be finite and positive')
            Qf = self._cell_features(features, cols, U=torch.as_tensor(q).to(self.device))
        F = self._cell_features(features, cols)
        out = cluster.knn(F, n_neighbors, queries=Qf, pg=self.pg, **knn_kw)
        return {'indices': out['indices'].cpu().numpy(), 'sq_distances': out['sq_distances'].cpu().numpy(),
                'features': F.cpu().numpy(), 'factors': cols}

    def cell_silhouette(self, labels, features='log_mean', factors=None, **silhouette_kw):
        """The exact silhouette of a labelling of the cells (for example ``cluster_cells(C)['labels']``) on the feature matrix
        cluster_cells() clusters, on the device (cluster.silhouette; its keywords n_clusters, candidate_chunk, query_block and
        blocks pass through): the number that compares clusterings across n_clusters and across `factors`.

        labels : an integer array or tensor, one id >= 0 per local cell.  Returns 'values', 'a', 'b' ((n_local,) float64 NumPy),
        'mean' (float, over all cells), 'cluster_means' ((C,) float64, NaN for an id without cells), 'counts' ((C,) int64, global),
        'features' (the (n_local, d) float32 matrix that was measured) and 'factors' as cluster_cells() returns them.  Under
        row sharding the model's process group is used.  Nothing of the model's state is written."""
        from .. import cluster
        cols = self._cell_feature_columns(features, factors)
        if 'pg' in silhouette_kw:
            raise ValueError('cell_silhouette() uses the process group of the model')
        F = self._cell_features(features, cols)
        out = cluster.silhouette(F, labels, pg=self.pg, **silhouette_kw)
        for k in ('values', 'a', 'b'):
            out[k] = out[k].cpu().numpy()
        out['features'] = F.cpu().numpy()
        out['factors'] = cols
        return out

    def cell_layout(self, features='log_mean', factors=None, **tsne_kw):
        """The exact t-SNE layout of the cells in two dimensions on the feature matrix cluster_cells() uses, on the device
        (cluster.tsne; its keywords perplexity, n_neighbors, n_iter, early_exaggeration, exaggeration_iter, learning_rate, init,
        seed, graph, check_every, query_block, candidate_chunk and blocks pass through): the picture of the fit.  Deterministic:
        the repulsive term is all pairs by brute force, and nothing is random after the start.

        graph : ``(indices, sq_distances)`` as cell_neighbors() returned them on the same features, to spare the search.
        Returns NumPy arrays: 'embedding' (n, 2) float64 and 'beta' (n,) float64; 'kl' (float, at the final layout), 'kl_trace',
        'n_iter', 'n_neighbors'; 'features' (the (n, d) float32 matrix that was laid out) and 'factors' as cluster_cells()
        returns them.  A model sharded over more than one rank raises NotImplementedError: row-sharded layouts are not
        implemented.  Nothing of the model's state is written."""
        from .. import cluster
        cols = self._cell_feature_columns(features, factors)
        if 'pg' in tsne_kw:
            raise ValueError('cell_layout() uses the process group of the model')
        if odist.world_size(self.pg) > 1:
            raise NotImplementedError('cell_layout() is not implemented for a model sharded over more than one rank')
        F = self._cell_features(features, cols)
        out = cluster.tsne(F, pg=self.pg, **tsne_kw)
        out['embedding'] = out['embedding'].cpu().numpy()
        out['beta'] = out['beta'].cpu().numpy()
        out['features'] = F.cpu().numpy()
        out['factors'] = cols
        return out

    def cell_communities(self, n_neighbors=15, resolution=1.0, weights='snn', features='log_mean', factors=None, graph=None,
                         **louvain_kw):
        """Graph communities of the cells: deterministic Louvain (cluster.louvain; its keywords max_sweeps, max_levels, row_cap,
        blocks and scratch pass through) on the shared-neighbour graph (cluster.snn_graph, `weights` 'snn' or 'count') of the
        n_neighbors nearest neighbours on the feature matrix cluster_cells() uses.  No number of clusters is asked for:
        `resolution` sets the grain.

        graph : ``(indices, sq_distances)`` as cell_neighbors() returned them on the same features, to spare the search (then
        n_neighbors is the width of `indices`).  Returns the dict of cluster.louvain: 'labels' ((n,) int32 device tensor, 0 the
        largest community; it feeds cell_silhouette() and marker_genes() as it is), 'n_communities', 'modularity', 'levels'.  A
        model sharded over more than one rank raises NotImplementedError.  Nothing of the model's state is written."""
        from .. import cluster
        cols = self._cell_feature_columns(features, factors)
        if 'pg' in louvain_kw:
            raise ValueError('cell_communities() uses the process group of the model')
        if odist.world_size(self.pg) > 1:
            raise NotImplementedError('cell_communities() is not implemented for a model sharded over more than one rank')
        if weights not in ('snn', 'count'):
            raise ValueError("weights must be 'snn' or 'count'")
        if graph is None:
            if int(n_neighbors) < 1:
                raise ValueError('n_neighbors must be at least 1')
            F = self._cell_features(features, cols)
            gi = cluster.knn(F, int(n_neighbors), pg=self.pg)['indices']
        else:
            gi = graph[0]
            if getattr(gi, 'ndim', 0) != 2 or int(gi.shape[0]) != self.n:
                raise ValueError('graph must be (indices, sq_distances) of the %d fitted cells' % self.n)
            gi = torch.as_tensor(np.asarray(gi) if not isinstance(gi, torch.Tensor) else gi).to(self.device, torch.int32).contiguous()
        return cluster.louvain(cluster.snn_graph(gi, weights), resolution=resolution, pg=self.pg, **louvain_kw)

    def cell_diffusion(self, n_comps=15, n_neighbors=15, features='log_mean', factors=None, graph=None, **diffusion_kw):
        """The diffusion map of the cells (scanpy's ``diffmap``): the n_comps leading eigenpairs of the symmetric transition
        matrix (cluster.diffusion_graph) of the n_neighbors nearest neighbours on the feature matrix cluster_cells() uses, by
        Lanczos on the device (cluster.diffusion_map; its keywords tol, max_steps, check_every, seed, start and blocks pass
        through).  Deterministic: a function of the features and the start vector alone.

        graph : ``(indices, sq_distances)`` as cell_neighbors() returned them on the same features, to spare the search (then
        n_neighbors is the width of `indices`).  Returns the dict of cluster.diffusion_map -- 'eigenvalues' ((m,) float64 NumPy,
        descending; the first is 1), 'components' ((n, m) float64 device tensor), 'residuals', 'steps', 'converged' -- plus
        'features' (the (n, d) float32 matrix, NumPy) and 'factors' as cluster_cells() returns them.  A neighbour graph that is not
        connected is a ValueError that states the number of components.  A model sharded over more than one rank raises
        NotImplementedError.  Nothing of the model's state is written."""
        from .. import cluster
        cols = self._cell_feature_columns(features, factors)
        if 'pg' in diffusion_kw:
            raise ValueError('cell_diffusion() uses the process group of the model')
        if odist.world_size(self.pg) > 1:
            raise NotImplementedError('cell_diffusion() is not implemented for a model sharded over more than one rank')
        F = self._cell_features(features, cols)
        if graph is None:
            if int(n_neighbors) < 1:
                raise ValueError('n_neighbors must be at least 1')
            nb = cluster.knn(F, int(n_neighbors), pg=self.pg)
            gi, gd = nb['indices'], nb['sq_distances']
        else:
            gi, gd = graph
            if getattr(gi, 'ndim', 0) != 2 or int(gi.shape[0]) != self.n or tuple(getattr(gd, 'shape', ())) != tuple(gi.shape):
                raise ValueError('graph must be (indices, sq_distances) of the %d fitted cells' % self.n)
            gi, gd = (torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t).to(self.device, dt).contiguous()
                      for t, dt in ((gi, torch.int32), (gd, torch.float32)))
        out = cluster.diffusion_map(cluster.diffusion_graph(gi, gd), n_comps=n_comps, pg=self.pg, **diffusion_kw)
        out['features'] = F.cpu().numpy()
        out['factors'] = cols
        return out

    def cell_pseudotime(self, root, diffusion=None, **diffusion_kw):
        """Diffusion pseudotime of the cells from the cell `root` (scanpy's ``dpt`` without branch detection;
        cluster.diffusion_pseudotime): how far along the fit's main directions of variation a cell lies from the root.

        root : a cell index within [0, n).  diffusion : a cell_diffusion() result to reuse; without one cell_diffusion() is
        called with the remaining keywords.  Returns 'dpt' and 'pseudotime' (dpt divided by its maximum), (n,) float64 device
        tensors, 'root', and 'diffusion' (the map that was used).  A model sharded over more than one rank raises
        NotImplementedError.  Nothing of the model's state is written."""
        from .. import cluster
        if 'pg' in diffusion_kw:
            raise ValueError('cell_pseudotime() uses the process group of the model')
        if odist.world_size(self.pg) > 1:
            raise NotImplementedError('cell_pseudotime() is not implemented for a model sharded over more than one rank')
        if isinstance(root, bool) or not isinstance(root, (int, np.integer)) or not 0 <= int(root) < self.n:
            raise ValueError('root must be a cell index within [0, %d)' % self.n)
        if diffusion is None:
            diffusion = self.cell_diffusion(**diffusion_kw)
        elif diffusion_kw:
            raise ValueError('with diffusion= no keyword of cell_diffusion() applies: %s' % ', '.join(sorted(diffusion_kw)))
        out = cluster.diffusion_pseudotime(diffusion['eigenvalues'], diffusion['components'], int(root))
        out['root'] = int(root)
        out['diffusion'] = diffusion
        return out

    # ---- which genes distinguish a cluster (scanpy's rank_genes_groups(method='t-test') on the counts the model holds) --------
    # Per cluster and gene the test needs the mean, the variance and the expressing fraction of the log-normalised counts
    # y_ij = log1p(x_ij target_sum / total_i).  y = 0 wherever x = 0, so the moments are sums over the non-zero counts only:
    # one walk over the sliced layout and the dense block (csrc/groupstats.hip) with the labels as a cluster axis, never a dense
    # n x m matrix; the statistic itself is assembled on the host from (C, m) arrays (markers.py).
    def _cell_totals_device(self):
        """sum_j x_ij of this rank's cells: an (n_local,) float64 device tensor in the caller's row order, cached like
        _count_constants() (X is constant)."""
        if getattr(self, '_xtotals', None) is None:
            ct = self.counts
            tot = torch.zeros(max(self.n, 1), dtype=torch.float64, device=self.device)
            call('oriana_cell_totals', ct.sparse_struct, ct.dense.c_struct if ct.dense is not None else None, ptr(ct.row_perm),
                 ptr(ct.col_perm), ptr(tot), stream_ptr())
            self._xtotals = tot[:self.n]
        return self._xtotals

    def cell_totals(self):
        """The total count of every local cell (the library size): an (n_local,) float64 NumPy array in the caller's row order,
        exact for integer counts.  Computed once on the device from the layouts the model holds, then cached."""
        return self._cell_totals_device().cpu().numpy()

    def _cluster_labels(self, labels, n_clusters, target_sum, limit):
        """The checks cluster_gene_stats() and cluster_rank_sums() share, before any launch: (labels as an int64 tensor on the
        device, C)."""
        from .. import cluster
        lab = cluster._label_tensor(labels, self.n, 'labels')
        if not float(target_sum) > 0.0:
            raise ValueError('target_sum must be positive')
        top = int(lab.max()) + 1 if lab.numel() else 0
        if n_clusters is None:
            C = cluster._global_max(top, self.device, self.pg)
        else:
            C = int(n_clusters)
            if top > C:
                raise ValueError('labels must lie within [0, n_clusters = %d), found %d' % (C, top - 1))
        if C < 1 or C > limit:
            raise ValueError('the number of clusters must lie within 1..%d, got %d' % (limit, C))
        return lab.to(self.device), C

    def cluster_gene_stats(self, labels, n_clusters=None, normalize=True, target_sum=1e4, log1p=True):
        """Per cluster and gene the moments of the (log-normalised) counts, on the device.

        labels : an integer array or tensor, one id >= 0 per local cell (for example ``cluster_cells(C)['labels']``).
        n_clusters : C (default: the largest id + 1 over all ranks).  normalize : scale every cell to `target_sum` counts
        (scale_i = target_sum / total_i, 0 for a cell without counts); log1p : take log1p of the scaled count -- the defaults are
        scanpy's ``normalize_total(target_sum=1e4)`` + ``log1p``.  Returns (C, m) float64 NumPy arrays in the caller's gene order:
        'n_expressing' (cells of the cluster with a non-zero count), 'sum' and 'sumsq' of the values over them (= over all cells of
        the cluster: a zero count gives 0), and 'sizes' (C,) int64, the cells per cluster.  Under row sharding everything is summed
        over the ranks in one packed all-reduce and every rank returns the same arrays.  ValueError before any launch for labels
        that are not n_local non-negative integers below n_clusters, target_sum <= 0 or more clusters than
        oriana_group_stats_max_groups().  Nothing of the model's state is written."""
        from .. import _lib
        n, m, dev, ct = self.n, self.m, self.device, self.counts
        lab, C = self._cluster_labels(labels, n_clusters, target_sum, int(_lib.load().oriana_group_stats_max_groups()))
        scale = None
        if normalize:
            tot = self._cell_totals_device()
            scale = torch.where(tot > 0, float(target_sum) / tot, torch.zeros_like(tot)).contiguous()
        lab32 = lab.to(torch.int32).contiguous()
        packed = torch.zeros(3 * C * m + C, dtype=torch.float64, device=dev)
        if n > 0:
            call('oriana_group_stats', ct.sparse_struct, ct.dense.c_struct if ct.dense is not None else None, ptr(ct.row_perm),
                 ptr(ct.col_perm), ptr(lab32), ptr(scale), 1 if log1p else 0, C, ptr(packed), stream_ptr())
        packed[3 * C * m:] = torch.bincount(lab, minlength=C).to(torch.float64)        # (exact: cell counts below 2^53)
        odist.all_reduce_sum(packed, self.pg)
        host = packed.cpu().numpy()
        st = host[:3 * C * m].reshape(3, C, m)
        return {'n_expressing': st[0], 'sum': st[1], 'sumsq': st[2], 'sizes': np.rint(host[3 * C * m:]).astype(np.int64)}

    def cluster_rank_sums(self, labels, n_clusters=None, normalize=True, target_sum=1e4, scratch_bytes=1 << 30, sort_cap=None):
        """Per cluster and gene the sum of the ranks of the cluster's cells, the ranks taken per gene over ALL cells on the
        normalised counts v_ij = x_ij * scale_i in float64 (normalize=False: on x_ij), ties averaged as
        ``scipy.stats.rankdata(method='average')`` has them: what a Wilcoxon rank-sum test takes (csrc/ranksum.hip).

        labels, n_clusters, normalize, target_sum : as cluster_gene_stats().  The scale is formed on the host, target_sum /
        cell_totals() in float64 NumPy (0 for a cell without counts); the device forms one float64 product per stored count and
        sorts its bit pattern, so a tie is a tie of those float64 values.  log1p is monotone and plays no part.  The stored
        counts of a gene are sorted panel by panel (markers.plan_rank_panels): scratch_bytes bounds the records of a panel at
        24 bytes each (a single gene tile above it is still taken, with a scratch of its own size), sort_cap the longest gene
        sorted inside LDS (default and largest: oriana_rank_sums_lds_cap()).  Neither changes a bit of the result.

        Returns NumPy arrays in the caller's gene order: 'rank_sum' (C, m) float64, exact half-integers; 'tie_term' (m,) int64,
        sum over the tie runs of t^3 - t, the run of the zeros included; 'n_expressing' (C, m) float64; 'sizes' (C,) int64.
        ValueError before any launch as cluster_gene_stats() raises it, and for a scratch_bytes or sort_cap out of range; a model
        sharded over more than one rank raises NotImplementedError before any launch or collective (rank sums do not add up
        over shards of cells).  Nothing of the model's state is written."""
        from .. import markers, _lib
        if odist.world_size(self.pg) > 1:
            raise NotImplementedError('cluster_rank_sums() is not implemented for a model sharded over more than one rank')
        n, m, dev, ct = self.n, self.m, self.device, self.counts
        lib = _lib.load()
        lab, C = self._cluster_labels(labels, n_clusters, target_sum, int(lib.oriana_rank_sums_max_groups()))
        cap = int(lib.oriana_rank_sums_lds_cap())
        if sort_cap is not None and not 1 <= int(sort_cap) <= cap:
            raise ValueError('sort_cap must lie within 1..%d, got %d' % (cap, int(sort_cap)))
        sort_cap = 0 if sort_cap is None else int(sort_cap)     # (0: the library's default)
        if int(scratch_bytes) < 0:
            raise ValueError('scratch_bytes must not be negative')
        if n >= 1 << 21:
            raise ValueError('cluster_rank_sums() takes fewer than 2^21 cells, got %d' % n)
        scale = None
        if normalize:
            tot = self.cell_totals()
            with np.errstate(divide='ignore'):
                scale = torch.as_tensor(np.where(tot > 0, float(target_sum) / tot, 0.0), device=dev).contiguous()
        lab32 = lab.to(torch.int32).contiguous()
        perm = ct.col_perm.cpu().numpy() if ct.col_perm is not None else np.arange(m)
        nnz_packed = np.rint(self._count_constants()[1].cpu().numpy()).astype(np.int64)[perm]
        panels = markers.plan_rank_panels(nnz_packed, ct.gd, int(scratch_bytes) // 24)
        records = max([p[2] for p in panels] + [0])
        by = int(lib.oriana_rank_sums_scratch_bytes_for(records, max([p[1] - p[0] for p in panels] + [0])))
        scratch = torch.empty(max(by, 16), dtype=torch.uint8, device=dev)
        out = torch.zeros((2 * C + 1) * m, dtype=torch.int64, device=dev)
        pos2, cnt, ties = out[:C * m], out[C * m:2 * C * m], out[2 * C * m:]
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        for g0, g1, _ in panels:
            call('oriana_rank_sums', ct.sparse_struct, ct.dense.c_struct if ct.dense is not None else None, ptr(ct.row_perm),
                 ptr(ct.col_perm), ptr(lab32), ptr(scale), C, g0, g1, ptr(scratch), records, sort_cap, ptr(pos2), ptr(cnt),
                 ptr(ties), ptr(overflow), stream_ptr())
        sizes = torch.bincount(lab, minlength=C).cpu().numpy().astype(np.int64)
        host = out.cpu().numpy()
        if int(overflow.cpu()[0]) != 0:
            raise _lib.OrianaHipError('oriana_rank_sums: a panel holds more stored counts than the per-gene counts of the model say')
        pos2, cnt, ties = host[:C * m].reshape(C, m), host[C * m:2 * C * m].reshape(C, m), host[2 * C * m:]
        # twice the rank sum in integers (below 2^43): the cluster's zeros tie at (z + 1) / 2, its stored counts stand z positions up
        z = n - cnt.sum(0)
        twice = (sizes[:, None] - cnt) * (z + 1)[None, :] + 2 * cnt * z[None, :] + pos2
        return {'rank_sum': twice.astype(np.float64) / 2.0, 'tie_term': ties + z * z * z - z,
                'n_expressing': cnt.astype(np.float64), 'sizes': sizes}

    def marker_genes(self, labels, n_top=50, method='t-test', tie_correct=False, **stats_kw):
        """The genes that distinguish each cluster of a labelling of the cells, every cluster against the rest, without a host
        copy of X.  method='t-test': Welch's t statistic on the log-normalised counts, scanpy's
        ``rank_genes_groups(method='t-test')``; method='wilcoxon': the rank-sum statistic on the normalised counts, its
        ``method='wilcoxon'`` (tie_correct as there; ranks are taken on the float64 values before log1p: cluster_rank_sums()).

        labels and the keywords n_clusters, normalize, target_sum, log1p: as cluster_gene_stats().  Returns its arrays plus,
        per cluster and gene ((C, m) float64, caller's gene order; NaN rows for an id without cells): 'scores' (exactly 0 for a
        gene without variance on both sides), 'df' (Welch-Satterthwaite, NaN where undefined), 'logfoldchanges', 'pct_in',
        'pct_out' (markers.welch_from_moments), and 'genes', a (C, min(n_top, m)) int64 array: per cluster the gene indices by
        decreasing score, ties by index (markers.rank).  With 'wilcoxon' (which also takes scratch_bytes and sort_cap of
        cluster_rank_sums()) 'scores' is the rank-sum z score (markers.wilcoxon_from_rank_sums; exactly 0 where every cell is
        tied under the correction), 'auc' = U / (n_c n_r), 'rank_sum' and 'tie_term' come along and there is no 'df'.  p-values
        are not computed.  ValueError for fewer than 2 non-empty clusters or another method; 'wilcoxon' on a model sharded over
        more than one rank raises NotImplementedError.  Nothing of the model's state is written."""
        from .. import markers
        if int(n_top) < 0:
            raise ValueError('n_top must not be negative')
        if method not in ('t-test', 'wilcoxon'):
            raise ValueError("method must be 't-test' or 'wilcoxon', got %r" % (method,))
        rank_kw = {}
        if method == 'wilcoxon':
            if odist.world_size(self.pg) > 1:
                raise NotImplementedError("marker_genes(method='wilcoxon') is not implemented for a model sharded over more "
                                          "than one rank")
            rank_kw = {k: stats_kw.pop(k) for k in ('scratch_bytes', 'sort_cap') if k in stats_kw}
        out = self.cluster_gene_stats(labels, **stats_kw)
        w = markers.welch_from_moments(out['n_expressing'], out['sum'], out['sumsq'], out['sizes'],
                                       log1p=bool(stats_kw.get('log1p', True)))
        if method == 'wilcoxon':
            rank_kw.update({k: stats_kw[k] for k in ('normalize', 'target_sum') if k in stats_kw})
            rs = self.cluster_rank_sums(labels, n_clusters=out['sizes'].shape[0], **rank_kw)
            r = markers.wilcoxon_from_rank_sums(rs['rank_sum'], rs['tie_term'], rs['sizes'], tie_correct=bool(tie_correct))
            out.update(rank_sum=rs['rank_sum'], tie_term=rs['tie_term'], auc=r['auc'])
            w = dict(w, scores=r['scores'])
            keys = ('scores', 'logfoldchanges', 'pct_in', 'pct_out')
        else:
            keys = ('scores', 'df', 'logfoldchanges', 'pct_in', 'pct_out')
        for k in keys:
            out[k] = w[k]
        out['genes'] = markers.rank(w['scores'], n_top)
        return out

    # ---- how strongly a cell expresses a gene set (scanpy's score_genes(), Seurat's AddModuleScore()) ------------------------------
    # score_is = sum_j W_js y_ij over the stored counts of cell i: the product of the packed matrix of the log-normalised counts
    # with an (m, S) weight matrix, one walk over both layouts with a fixed summation order (csrc/groupstats.hip);
    # which genes carry which weight is decided on the host (signatures.py).
    def gene_scores(self, weights, normalize=True, target_sum=1e4, log1p=True, as_tensor=False):
        """Linear read-outs of the (log-normalised) counts of every local cell: ``Y @ weights`` without forming Y.

        weights : (m,) or (m, S) array or tensor of finite values in the caller's gene order, taken as float64 (a column per
        read-out: signatures.score_weights(), a signature with real weights, loadings from elsewhere).  normalize, target_sum,
        log1p : as cluster_gene_stats(), with the same scale.  Returns the (n_local, S) float64 result in the caller's row order
        ((n_local, 1) for 1-D weights): a NumPy array, or with as_tensor=True the device tensor.  A cell without a count scores
        exactly 0.  Every sum is taken in an order fixed by the layouts and S: the same call returns the same bits.  A cell's
        score is local, so under row sharding there is no collective.  ValueError before any launch for a wrong shape, entries
        that are not finite, S outside 1..oriana_gene_scores_max_sets() or target_sum <= 0.  Nothing of the model's state is
        written."""
        from .. import _lib
        n, m, dev, ct = self.n, self.m, self.device, self.counts
        W = weights if isinstance(weights, torch.Tensor) else torch.as_tensor(np.asarray(weights))
        if W.is_complex() or W.dtype == torch.bool:
            raise ValueError('weights must be real numbers, got %s' % W.dtype)
        if W.ndim == 1:
            W = W.reshape(-1, 1)
        if W.ndim != 2 or int(W.shape[0]) != m:
            raise ValueError('weights must be (%d,) or (%d, S), got %s' % (m, m, tuple(weights.shape) if hasattr(weights, 'shape')
                                                                            else tuple(W.shape)))
        S, limit = int(W.shape[1]), int(_lib.load().oriana_gene_scores_max_sets())
        if S < 1 or S > limit:
            raise ValueError('the number of weight columns must lie within 1..%d, got %d' % (limit, S))
        if not float(target_sum) > 0.0:
            raise ValueError('target_sum must be positive')
        W = W.to(device=dev, dtype=torch.float64).contiguous()
        if not bool(torch.isfinite(W).all()):
            raise ValueError('weights must be finite')
        scale = None
        if normalize:
            tot = self._cell_totals_device()
            scale = torch.where(tot > 0, float(target_sum) / tot, torch.zeros_like(tot)).contiguous()
        out = torch.empty((n, S), dtype=torch.float64, device=dev)
        if n > 0:
            call('oriana_gene_scores', ct.sparse_struct, ct.dense.c_struct if ct.dense is not None else None, ptr(ct.row_perm),
                 ptr(ct.col_perm), ptr(scale), 1 if log1p else 0, ptr(W), S, ptr(out), stream_ptr())
        return out if as_tensor else out.cpu().numpy()

    def score_genes(self, gene_sets, ctrl_size=50, n_bins=25, seed=0, gene_pool=None, control_genes=None, **kw):
        """The score of every local cell for each of S gene sets: the mean log-normalised expression of the set minus the mean of
        control genes drawn from the same expression bins (signatures.control_genes; scanpy's ``score_genes()``), on the device.

        gene_sets : a sequence of integer index arrays, or a dict name -> array.  ctrl_size, n_bins, seed : the draw of the
        controls (set s uses the generator of (seed, s)); gene_pool : the genes that define the bins and may be drawn (default:
        all).  The gene means come from cluster_gene_stats() with a single cluster -- all-reduced under row sharding, so every
        rank draws the same controls.  control_genes : the 'control_genes' of an earlier result instead of a draw (another
        model, a shard or held-out cells scored against the same controls); no means are computed then and 'gene_means' is None.
        Further keywords: normalize, target_sum, log1p, as_tensor of gene_scores().

        Returns 'scores' (n_local, S) float64, 'control_genes' (a list of sorted int64 arrays), 'gene_means' (m,) float64,
        'names' (the dict's keys, or 0 .. S - 1) and 'weights', the (m, S) matrix that was multiplied.  ValueError before any
        launch for an empty set, indices outside [0, m) or repeated within a set, ctrl_size < 1, n_bins < 2, target_sum <= 0,
        control_genes that do not match the sets or hold an empty list (TypeError for a keyword gene_scores() does not take);
        after the means for a set whose bins hold no other gene.  Nothing of the model's state is written."""
        from .. import signatures, _lib
        unknown = sorted(set(kw) - {'normalize', 'target_sum', 'log1p', 'as_tensor'})
        if unknown:
            raise TypeError('score_genes() takes no keyword %s' % ', '.join(unknown))
        m = self.m
        names, sets = signatures.named_sets(m, gene_sets)
        limit = int(_lib.load().oriana_gene_scores_max_sets())
        if len(sets) > limit:
            raise ValueError('at most %d gene sets per call, got %d' % (limit, len(sets)))
        ctrl_size, n_bins = signatures.check_draw(ctrl_size, n_bins)
        if not float(kw.get('target_sum', 1e4)) > 0.0:
            raise ValueError('target_sum must be positive')
        pool = None if gene_pool is None else signatures.check_set(m, gene_pool, 'gene_pool')
        means = None
        if control_genes is not None:
            controls = list(control_genes)
            if len(controls) != len(sets):
                raise ValueError('%d gene sets but %d control sets' % (len(sets), len(controls)))
            controls = [signatures.check_set(m, c, 'control set %r' % (nm,)) for nm, c in zip(names, controls)]
        else:
            stats_kw = {k: v for k, v in kw.items() if k != 'as_tensor'}
            st = self.cluster_gene_stats(np.zeros(self.n, dtype=np.int64), n_clusters=1, **stats_kw)
            means = st['sum'][0] / max(int(st['sizes'][0]), 1)
            controls = [signatures.control_genes(means, g, ctrl_size=ctrl_size, n_bins=n_bins, seed=seed, set_index=s, pool=pool)
                        for s, g in enumerate(sets)]
        W = signatures.score_weights(m, sets, controls)
        return {'scores': self.gene_scores(W, **kw), 'control_genes': controls, 'gene_means': means, 'names': names, 'weights': W}

    # ---- state I/O (tests, checkpoints) ---------------------------------------------------------------
    _PARAMS =('alpha1', 'alpha2', 'beta1', 'beta2', 'a1', 'a2', 'b1', 'b2', 'pi_d', 'p_d', 'pi_s', 'p_s')

    def state(self):
        """Host copy of every parameter and expectation, keyed like the oracle / golden files."""
        out = {}
        for k in self._PARAMS:
            if hasattr(self, k):
                out[k] = getattr(self, k).asarray()
        out.update(U_hat=self.U_hat, V_hat=self.V_hat, log_U_hat=self.log_U_hat, log_V_hat=self.log_V_hat)
        if hasattr(self, '_S_hat'):
            out['S_hat'] = self.S_hat
        return out

    def load_state(self, st):
        """Overwrite parameters (and recompute nothing): used to start a sweep from a given state."""
        for k in self._PARAMS:
            if k in st and hasattr(self, k):
                getattr(self, k).tensor.copy_(torch.as_tensor(np.asarray(st[k], dtype=np.float64)).to(self.device))
        for k, t in (('U_hat', self._U_hat), ('V_hat', self._V_hat), ('log_U_hat', self._log_U_hat),
                     ('log_V_hat', self._log_V_hat)):
            if k in st:
                t.copy_(torch.as_tensor(np.asarray(st[k])).to(self.device, dtype=t.dtype))
        self._touch()
        self._ws.fu_pending = False             # (E[log U] was overwritten)
        # column sums that the next sweep reads
        self._sumU[0] = self._U_hat.sum(0); self._sumU[1] = self._log_U_hat.double().sum(0)
        odist.all_reduce_sum(self._sumU, self.pg)
        self._sumV[0] = self._V_hat.sum(0); self._sumV[1] = self._log_V_hat.double().sum(0)
        self._load_extra(st)

    def _load_extra(self, st):
        pass

    def save(self, path):
        """Checkpoint: the state of this rank (state(), plus the sweep count and the shapes) as one .npz file.  The
        reference has no save / load; under row sharding every rank saves its own rows."""
        st = self.state()
        st['meta/n_sweeps'] = np.int64(self.n_sweeps)
        st['meta/shape'] = np.asarray([self.n, self.m, self.k], dtype=np.int64)
        st['meta/model'] = np.asarray(type(self).__name__)
        np.savez(path, **st)

    def restore(self, path):
        """Load a checkpoint written by save() into this model (same class, same counts and k): the next step()
        continues the run (the expectations are stored, nothing is recomputed)."""
        with np.load(path, allow_pickle=False) as f:
            shape = tuple(int(v) for v in f['meta/shape'])
            if shape != (self.n, self.m, self.k) or str(f['meta/model']) != type(self).__name__:
                raise ValueError('checkpoint of %s %s does not fit %s %s' % (str(f['meta/model']), shape, type(self).__name__,
                                                                              (self.n, self.m, self.k)))
            self.load_state({k: f[k] for k in f.files if not k.startswith('meta/')})
            self.n_sweeps = int(f['meta/n_sweeps'])
        return self
