# -*- coding: utf-8 -*-
"""Gene-set scores, the host side (NumPy only): which control genes a set is held against and the weight matrix that turns
the transformed counts into scores (models/base.py: score_genes, gene_scores).

The score of a cell for a gene set G is the mean of its log-normalised expression over G minus the mean over control genes of
similar average expression -- scanpy's ``score_genes()``, Seurat's ``AddModuleScore()``.  Both means are linear in the cell's
expression, so the score is ``sum_j w_j y_ij`` with w = 1/|G| on the set, -1/|ctrl| on the controls and 0 elsewhere: one column
of the matrix score_weights() builds, multiplied on the device by oriana_gene_scores.

control_genes() follows scanpy's procedure: the genes of the pool are ranked by their mean, the ranks are cut into bins of equal
width, and for every bin a gene of the set falls into, up to ctrl_size other genes of that bin are drawn.  The draw is this
module's own (a seeded NumPy generator per set), so the lists are reproducible here and not the ones scanpy would draw.
"""
import numpy as np


def check_set(m, genes, what='gene set'):
    """`genes` as a 1-D int64 array of distinct indices within [0, m), not empty; ValueError otherwise."""
    a = np.asarray(genes)
    if a.ndim != 1 or a.size == 0:
        raise ValueError('%s must be a non-empty 1-D sequence of gene indices' % what)
    if a.dtype.kind not in 'iu':
        raise ValueError('%s must hold integer gene indices, got dtype %s' % (what, a.dtype))
    a = a.astype(np.int64)
    if a.min() < 0 or a.max() >= int(m):
        raise ValueError('%s must lie within [0, %d)' % (what, int(m)))
    if np.unique(a).size != a.size:
        raise ValueError('%s holds a gene more than once' % what)
    return a


def check_draw(ctrl_size, n_bins):
    """The two parameters of the draw; ValueError for ctrl_size < 1 or n_bins < 2."""
    if isinstance(ctrl_size, bool) or not isinstance(ctrl_size, (int, np.integer)) or int(ctrl_size) < 1:
        raise ValueError('ctrl_size must be an integer of at least 1, got %r' % (ctrl_size,))
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or int(n_bins) < 2:
        raise ValueError('n_bins must be an integer of at least 2, got %r' % (n_bins,))
    return int(ctrl_size), int(n_bins)


def named_sets(m, gene_sets):
    """(names, [int64 array per set]) of a dict name -> indices or a sequence of index arrays (names 0, 1, ..); every set checked
    by check_set.  ValueError for no set at all."""
    if isinstance(gene_sets, dict):
        names, sets = list(gene_sets.keys()), list(gene_sets.values())
    else:
        sets = list(gene_sets)
        names = list(range(len(sets)))
    if not sets:
        raise ValueError('gene_sets holds no set')
    return names, [check_set(m, g, 'gene set %r' % (nm,)) for nm, g in zip(names, sets)]


def expression_bins(means, pool, genes, n_bins):
    """The bin of every gene of `genes`: rank_j = 1 + #{l in pool: mean_l < mean_j} (ties share the lowest rank),
    n_items = max(1, round(len(pool) / (n_bins - 1))), bin_j = rank_j // n_items."""
    sorted_means = np.sort(means[pool])
    rank = 1 + np.searchsorted(sorted_means, means[genes], side='left')
    n_items = max(1, int(round(len(pool) / (n_bins - 1))))
    return rank // n_items


def control_genes(means, gene_set, ctrl_size=50, n_bins=25, seed=0, set_index=0, pool=None):
    """The control genes of one set: a sorted int64 array.

    means : (m,) the average expression of every gene.  gene_set : distinct indices within [0, m).  pool : the genes that may be
    drawn and that define the ranks (default: all m).  Per distinct bin of the set's genes (expression_bins), in ascending order,
    the pool genes of that bin that are not in the set are taken in ascending index order, permuted by ONE generator
    ``np.random.default_rng([seed, set_index])`` used bin after bin, and the first ctrl_size kept; the result is the sorted union.
    The generator belongs to the set: what another set draws does not change this one's controls.  ValueError for an empty set,
    indices outside [0, m) or repeated, ctrl_size < 1, n_bins < 2, or when no control gene is left."""
    means = np.asarray(means, dtype=np.float64)
    if means.ndim != 1:
        raise ValueError('means must be a 1-D array, one value per gene')
    m = means.shape[0]
    ctrl_size, n_bins = check_draw(ctrl_size, n_bins)
    gene_set = check_set(m, gene_set)
    pool = np.arange(m, dtype=np.int64) if pool is None else np.sort(check_set(m, pool, 'pool'))
    set_bins = np.unique(expression_bins(means, pool, gene_set, n_bins))
    free = pool[~np.isin(pool, gene_set)]
    free_bins = expression_bins(means, pool, free, n_bins)
    rng = np.random.default_rng([int(seed), int(set_index)])
    picked = []
    for b in set_bins:
        cand = free[free_bins == b]
        picked.append(rng.permutation(cand)[:ctrl_size])
    ctrl = np.unique(np.concatenate(picked)) if picked else np.zeros(0, dtype=np.int64)
    if ctrl.size == 0:
        raise ValueError('no control gene is left for the set: its bins hold no other gene of the pool')
    return ctrl.astype(np.int64)


def score_weights(m, gene_sets, controls):
    """The (m, S) float64 matrix whose column s is 1 / |G_s| on the genes of set s, -1 / |ctrl_s| on its controls and exactly 0
    elsewhere (a gene listed on both sides carries the sum of the two).  ValueError as check_set raises it, or when the two
    lists differ in length."""
    m = int(m)
    gene_sets, controls = list(gene_sets), list(controls)
    if len(gene_sets) != len(controls):
        raise ValueError('%d gene sets but %d control sets' % (len(gene_sets), len(controls)))
    if not gene_sets:
        raise ValueError('gene_sets holds no set')
    W = np.zeros((m, len(gene_sets)), dtype=np.float64)
    for s, (g, c) in enumerate(zip(gene_sets, controls)):
        g = check_set(m, g, 'gene set %d' % s)
        c = check_set(m, c, 'control set %d' % s)
        W[g, s] += 1.0 / g.size
        W[c, s] -= 1.0 / c.size
    return W
