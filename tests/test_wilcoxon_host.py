# -*- coding: utf-8 -*-
"""marker_genes(method='wilcoxon') without a GPU: markers.wilcoxon_from_rank_sums against the SciPy reference of
tests/wilcoxon_reference.py within the bound derived there, its edge cases, markers.plan_rank_panels, and the argument checks of
the new C entries before any HIP call."""
import ctypes

import numpy as np
import pytest
import scipy.stats

import wilcoxon_reference as wr
from oriana_amd import markers
from test_deviance_path_gpu import _counts, N_ROWS, M_COLS

ZERO_GENE, FULL_GENE = 5, 250
_cache = {}


def _X():
    if 'X' not in _cache:
        _cache['X'] = _counts(3)
        assert _cache['X'].shape == (N_ROWS, M_COLS) == (805, 301)
    return _cache['X']


def _ranks(normalize):
    """The ranks of all cells per gene, computed once per value kind and shared."""
    key = ('ranks', normalize)
    if key not in _cache:
        _cache[key] = scipy.stats.rankdata(wr.values(_X(), normalize), axis=0, method='average')
    return _cache[key]


def _blocked_labels():
    lab = np.empty(N_ROWS, dtype=np.int64)
    lab[:16], lab[16:255], lab[255], lab[256:600], lab[600:790], lab[790:] = 0, 1, 2, 4, 5, 6
    return lab, 7


LABELLINGS = [('C=%d' % C, lambda C=C: (np.random.default_rng(40 + C).integers(0, C, size=N_ROWS), C)) for C in (2, 3, 17)]
LABELLINGS.append(('blocked', _blocked_labels))


@pytest.mark.parametrize('normalize', [True, False], ids=['normalized', 'raw'])
@pytest.mark.parametrize('what,make', LABELLINGS, ids=[w for w, _ in LABELLINGS])
def test_scores_against_the_reference(what, make, normalize):
    X = _X()
    lab, C = make()
    ref = wr.rank_sums(X, lab, C, normalize=normalize, ranked=_ranks(normalize))
    if what == 'blocked':
        assert ref['sizes'][3] == 0 and ref['sizes'][2] == 1
    for tc in (False, True):
        got = markers.wilcoxon_from_rank_sums(ref['rank_sum'], ref['tie_term'], ref['sizes'], tie_correct=tc)
        rs = wr.scores(ref, tie_correct=tc)
        wr.assert_scores(got['scores'], rs, '%s tie_correct=%s' % (what, tc))
        live = ref['sizes'] > 0
        assert np.isnan(got['auc'][~live]).all() and np.isnan(got['u'][~live]).all()
        assert np.allclose(got['auc'][live], rs['auc'].astype(np.float64)[live], rtol=4 * wr.U, atol=0)
        assert (got['auc'][live] >= 0).all() and (got['auc'][live] <= 1).all()
        # the all-zero gene: every cell tied, rank sums n_c (N + 1) / 2, score 0 (corrected: sigma = 0, exactly 0), auc 1 / 2
        n_c = ref['sizes'][live].astype(np.float64)
        assert np.array_equal(ref['rank_sum'][live, ZERO_GENE], n_c * (N_ROWS + 1) / 2)
        assert (got['scores'][live, ZERO_GENE] == 0).all() and (got['auc'][live, ZERO_GENE] == 0.5).all()
    # the gene every cell with a count expresses: the one cell without counts is a zero run of its own, t^3 - t = 0
    assert ref['n_expressing'][:, FULL_GENE].sum() == N_ROWS - 1
    assert int(ref['tie_term'][ZERO_GENE]) == N_ROWS ** 3 - N_ROWS


def test_scipy_ranksums_and_tiecorrect_agree_with_the_reference():
    X = _X()
    C = 3
    lab = np.random.default_rng(43).integers(0, C, size=N_ROWS)
    ref = wr.rank_sums(X, lab, C, ranked=_ranks(True))
    V = wr.values(X)
    plain, corrected = wr.scores(ref, False)['scores'], wr.scores(ref, True)
    rng = np.random.default_rng(7)
    pairs = [(int(rng.integers(0, C)), int(j)) for j in rng.choice(M_COLS, size=12, replace=False)] + [(0, FULL_GENE), (1, 0)]
    for c, j in pairs:
        if j == ZERO_GENE:
            continue
        st = scipy.stats.ranksums(V[lab == c, j], V[lab != c, j]).statistic
        assert abs(st - float(plain[c, j])) <= 1e-12 * max(1.0, abs(st)), (c, j)
        factor = scipy.stats.tiecorrect(ref['ranks'][:, j])
        n_c, n_r = int(ref['sizes'][c]), N_ROWS - int(ref['sizes'][c])
        sigma = np.sqrt(n_c * n_r * (N_ROWS + 1) / 12.0 * factor)
        assert abs(sigma - float(corrected['sigma'][c, j])) <= 1e-12 * sigma, (c, j)


def test_edge_cases():
    # a gene constant over all cells: one tie run of N, T = N^3 - N; corrected sigma is 0 and the score exactly 0
    sizes = np.array([3, 0, 5], dtype=np.int64)
    N = 8
    R = np.array([[3 * 4.5, 6.0], [0.0, 0.0], [5 * 4.5, 30.0]])
    T = np.array([N ** 3 - N, 0], dtype=np.int64)
    for tc in (False, True):
        got = markers.wilcoxon_from_rank_sums(R, T, sizes, tie_correct=tc)
        assert (got['scores'][[0, 2], 0] == 0).all() and not np.signbit(got['scores'][[0, 2], 0]).any()
        assert np.isnan(got['scores'][1]).all() and np.isnan(got['auc'][1]).all()
        assert got['auc'][0, 1] == 0.0 and got['auc'][2, 1] == 1.0                 # the three smallest / the five largest
        assert got['scores'][0, 1] < 0 < got['scores'][2, 1]
    # nearly every cell tied at a large N: the integer numerator keeps the correction's leading digits
    N = 2 ** 20
    sizes = np.array([N // 2, N // 2], dtype=np.int64)
    T = np.array([(N - 1) ** 3 - (N - 1)], dtype=object)
    R = np.array([[N // 2 * (N + 1) / 2.0 + 1.0], [N // 2 * (N + 1) / 2.0 - 1.0]])
    got = markers.wilcoxon_from_rank_sums(R, T, sizes, tie_correct=True)
    full = N ** 3 - N
    sigma = np.sqrt(np.longdouble(N // 2) ** 2 * (N + 1) / 12 * (np.longdouble(full - int(T[0])) / np.longdouble(full)))
    assert abs(got['scores'][0, 0] - float(1 / sigma)) <= 8 * wr.U / float(sigma)
    with pytest.raises(ValueError):
        markers.wilcoxon_from_rank_sums(R, T, np.array([N, 0]), tie_correct=True)   # one non-empty cluster: no rest
    with pytest.raises(ValueError):
        markers.wilcoxon_from_rank_sums(R, T[:0], sizes)
    with pytest.raises(ValueError):
        markers.wilcoxon_from_rank_sums(R, np.array([0.5]), sizes)


@pytest.mark.parametrize('gd', [0, 64, 96])
def test_plan_rank_panels(gd):
    rng = np.random.default_rng(gd)
    m = 96 + 3 * 256 + 41
    nnz = rng.integers(0, 900, size=m)
    nnz[:gd] += 5000
    tiles = [(t, min(gd, t + 32)) for t in range(0, gd, 32)] + [(t, min(m, t + 256)) for t in range(gd, m, 256)]
    heaviest = max(int(nnz[a:b].sum()) for a, b in tiles)
    for budget in (0, 1, heaviest - 1, heaviest, 3 * heaviest, 10 ** 9):
        panels = markers.plan_rank_panels(nnz, gd, budget)
        assert [p[0] for p in panels] == [0] + [p[1] for p in panels[:-1]] and panels[-1][1] == m     # every gene exactly once
        for g0, g1, rec in panels:
            assert g0 < g1 and rec == int(nnz[g0:g1].sum())
            assert g1 <= gd or g0 >= gd                                                              # never across gd
            if g1 <= gd:
                assert g0 % 32 == 0 and g1 % 32 == 0
            else:
                assert (g0 - gd) % 256 == 0 and ((g1 - gd) % 256 == 0 or g1 == m)
            single = (g0, g1) in tiles
            assert rec <= budget or single, (budget, g0, g1)
        if budget >= 10 ** 9:
            assert len(panels) == (2 if gd else 1)
        if budget == 0:
            assert len(panels) == len(tiles)
    assert markers.plan_rank_panels(np.zeros(0, dtype=np.int64), 0, 5) == []
    for bad in (dict(gd=33), dict(gd=-32), dict(gd=m + 32 - m % 32), dict(budget=-1)):
        with pytest.raises(ValueError):
            markers.plan_rank_panels(nnz, bad.get('gd', 0), bad.get('budget', 10))


# ---- the C entries: every check comes before any HIP call ---------------------------------------------------------------------

@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from oriana_amd import _lib
    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    from oriana_amd import _lib
    for name in ('oriana_rank_sums', 'oriana_rank_sums_max_groups', 'oriana_rank_sums_lds_cap', 'oriana_rank_sums_scratch_bytes_for'):
        assert hasattr(lib, name) and name in _lib.declared_symbols(), name
    assert lib.oriana_rank_sums_max_groups() == 1024 and lib.oriana_rank_sums_lds_cap() >= 1024
    by = lib.oriana_rank_sums_scratch_bytes_for
    assert by(-1, 3) == -1 and by(3, -1) == -1
    assert by(0, 0) == 16 and by(1000, 0) - by(0, 0) == 24000 and by(0, 256) % 16 == 0 and by(0, 256) >= 3 * 256 * 8


def test_rank_sums_argument_errors(lib):
    from oriana_amd._lib import OrianaCounts, OrianaDense
    EINVAL, EKRANGE = -1, -2
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    p = a - a % 16 + 16

    def counts(n=0, m=0):
        c = OrianaCounts()
        c.n, c.m, c.nrb, c.ncb = n, m, (n + 255) // 256, (m + 255) // 256      # rslots = 0: no stored count, no array is read
        return c

    def rs(cm=None, dn=None, labels=p, C=3, g0=0, g1=0, scratch=p, cap=0, lds=0, pos2=p, cnt=p, ties=p, ovf=p):
        cm = counts() if cm is None else cm
        return lib.oriana_rank_sums(ctypes.byref(cm) if cm else None, ctypes.byref(dn) if dn is not None else None, None, None,
                                    labels, None, C, g0, g1, scratch, cap, lds, pos2, cnt, ties, ovf, None)

    assert rs(cm=False) == EINVAL
    for kw in (dict(labels=None), dict(scratch=None), dict(pos2=None), dict(cnt=None), dict(ties=None), dict(ovf=None), dict(C=0),
               dict(C=-2), dict(cap=-1), dict(lds=-1), dict(lds=lib.oriana_rank_sums_lds_cap() + 1), dict(scratch=p + 8),
               dict(g0=-1), dict(g0=1, g1=0), dict(g1=1)):
        assert rs(**kw) == EINVAL, kw
    neg = counts()
    neg.n = -1
    assert rs(cm=neg) == EINVAL
    assert rs(dn=OrianaDense(0, 33, 0, p)) == EINVAL                              # a dense block oriana_group_stats refuses
    assert rs(cm=counts(40, 600), dn=OrianaDense(64, 32, 2, p)) == EINVAL        # its cells are not cm's
    wide = counts(40, 600)                                                       # 600 sliced genes behind 64 dense ones
    dn = OrianaDense(40, 64, 8, p)
    for g0, g1 in ((0, 16), (16, 32), (32, 128), (0, 320), (64, 100), (65, 320), (64 + 256, 64 + 500), (64 + 512, 64 + 601)):
        assert rs(cm=wide, dn=dn, g0=g0, g1=g1) == EINVAL, (g0, g1)               # not tile-aligned, or across the two layouts
    assert rs(cm=wide, dn=dn, g0=0, g1=64, C=1025) == EKRANGE
    assert rs(cm=counts(2 ** 21, 600), g0=0, g1=256) == EKRANGE                   # sum (t^3 - t) must stay below 2^63
    assert rs(cm=wide, dn=dn, g0=64, g1=64) == 0                                  # an empty panel: no launch
    assert rs(cm=counts(0, 600), g0=0, g1=600) == 0                               # no cells: no launch
    assert rs() == 0
    assert not any(buf), 'a refused or empty call wrote through a pointer'
