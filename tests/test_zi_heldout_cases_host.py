# -*- coding: utf-8 -*-
"""tests/zi_heldout_cases.py held to the code it is meant to cover, without a GPU: the rate cases against the dispatch rule itself
(oriana_zi_dispatch answers through the chain the entries launch with), the K of the loop forms against the loop bounds of
k_dropout_sweep / k_gene_rate, the long batches against the flush and spill periods of k_gene_rate, and every case against the
condition that the sigmoid decides its result.  A change of the rule that adds an instantiation fails here until a case reaches
it."""
import numpy as np
import pytest

import zi_foldin_reference as zr
import zi_heldout_cases as zc

EKRANGE, EINVAL = -2, -1


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from oriana_amd import _lib
    return _lib.load()


def _unpack(code):
    assert code >= 0, code
    return code >> 16, (code >> 8) & 255, code & 255


def _tiles_ok(m, with_tiles):
    """The run-time preconditions of the tiles family that a test chooses (dn::zi_update_ok; the buffers are 16-byte aligned)."""
    return int(with_tiles and m % 4 == 0)


# ---- 1. the rate cases and the rule ------------------------------------------------------------------------------------------

def test_rate_cases_reach_every_instantiation_the_rule_can_answer(lib):
    can = {}
    for arithmetic in (zc.F32, zc.BF16X3):
        for tiles_ok in (0, 1):
            for K in range(1, 129):
                can.setdefault(_unpack(lib.oriana_zi_dispatch(zc.UPDATE, K, arithmetic, tiles_ok)), []).append((K, arithmetic, tiles_ok))
    reached = {}
    for K, arithmetic, m, with_tiles in zc.RATE_CASES:
        reached.setdefault(_unpack(lib.oriana_zi_dispatch(zc.UPDATE, K, arithmetic, _tiles_ok(m, with_tiles))), []).append((K, m, with_tiles))
    for inst in sorted(can):
        print('family %d <%d, %d>: %s' % (inst + (reached.get(inst),)))
    missing = sorted(set(can) - set(reached))
    assert not missing, 'no rate case reaches %s (the rule answers them at (K, arithmetic, tiles_ok) = %s)' % (
        missing, [can[i][0] for i in missing])
    assert set(reached) <= set(can)
    # what the rule is known to hold today: a count that moves means the text of the table needs another look
    fams = sorted(f for f, _, _ in can)
    assert (fams.count(zc.TILES), fams.count(zc.B16), fams.count(zc.F32_FAMILY)) == (8, 4, 4)
    assert len(set(zc.RATE_CASES)) == len(zc.RATE_CASES)


def test_b16_and_f32_are_reached_first_and_by_both_fallbacks(lib):
    """Per instantiation of the two families of dense_f32.hip: as the first candidate (the rule's answer with tiles_ok = 1), after
    tiles was passed over for m % 4 != 0, and after it was passed over for want of the per-lane flags -- wherever the rule offers
    that route at all."""
    def route(K, arithmetic, m, with_tiles):
        first = _unpack(lib.oriana_zi_dispatch(zc.UPDATE, K, arithmetic, 1))
        if first[0] != zc.TILES:
            return 'first'
        return 'unaligned' if m % 4 else ('no-flags' if not with_tiles else 'tiles')
    offered, taken = {}, {}
    for K in range(1, 129):
        for arithmetic in (zc.F32, zc.BF16X3):
            first = _unpack(lib.oriana_zi_dispatch(zc.UPDATE, K, arithmetic, 1))
            second = _unpack(lib.oriana_zi_dispatch(zc.UPDATE, K, arithmetic, 0))
            if first[0] != zc.TILES:
                assert second == first
                offered.setdefault(first, set()).add('first')
            else:
                offered.setdefault(second, set()).update(('unaligned', 'no-flags'))
    for K, arithmetic, m, with_tiles in zc.RATE_CASES:
        inst = _unpack(lib.oriana_zi_dispatch(zc.UPDATE, K, arithmetic, _tiles_ok(m, with_tiles)))
        taken.setdefault(inst, set()).add(route(K, arithmetic, m, with_tiles))
    for inst in sorted(offered):
        print('family %d <%d, %d>: offered %s, taken %s' % (inst + (sorted(offered[inst]), sorted(taken.get(inst, ())))))
        assert offered[inst] <= taken.get(inst, set()), inst
    assert offered[(zc.B16, 2, 4)] == {'unaligned', 'no-flags'}          # k_dropout_sweep_b16<2, 4>: by the fallback only


def test_edge_cases_take_one_instantiation_per_family(lib):
    fams = {}
    for K, arithmetic, n, m, with_tiles in zc.RATE_EDGE_CASES:
        inst = _unpack(lib.oriana_zi_dispatch(zc.UPDATE, K, arithmetic, _tiles_ok(m, with_tiles)))
        fams.setdefault(inst[0], set()).add((n, m))
    shapes = set(zc.EDGE_SHAPES)
    assert fams[zc.TILES] == {s for s in shapes if s[1] % 4 == 0}      # (three genes: the fallback)
    assert fams[zc.B16] >= shapes and fams[zc.F32_FAMILY] == shapes
    assert {(1, zc.M_ALIGNED), (33, zc.M_ALIGNED), (zc.N_BODY, 4), (zc.N_BODY, 3), (zc.N_BODY, 256)} == shapes


def test_dispatch_return_codes(lib):
    f = lib.oriana_zi_dispatch
    assert f(0, 129, zc.BF16X3, 1) == EKRANGE and f(1, 129, zc.F32, 0) == EKRANGE
    assert f(0, 0, zc.BF16X3, 1) == EINVAL and f(0, -3, zc.F32, 1) == EINVAL
    assert f(2, 20, zc.BF16X3, 1) == EINVAL and f(-1, 20, zc.BF16X3, 1) == EINVAL
    assert f(0, 20, 2, 1) == EINVAL and f(0, 20, -1, 1) == EINVAL
    # both products, the ends of the range
    assert _unpack(f(0, 1, zc.BF16X3, 1)) == (zc.B16, 1, 1) and _unpack(f(0, 128, zc.BF16X3, 1)) == (zc.F32_FAMILY, 4, 0)
    assert _unpack(f(1, 50, zc.BF16X3, 1)) == (zc.TILES, 4, 0) and _unpack(f(1, 50, zc.BF16X3, 0)) == (zc.B16, 2, 0)
    assert _unpack(f(1, 20, zc.F32, 1)) == (zc.F32_FAMILY, 1, 4)


# ---- 2. the loop forms -------------------------------------------------------------------------------------------------------

def _loop(K):
    """(form, KS, rem) from the bounds of the factor loop:  if (KS >= 4) { prologue; for (s = 0; s + 8 <= KS; s += 4) body;
    rem = KS - s - 4; epilogue } else one step at a time."""
    KS = (K + 1) // 2
    if KS < 4:
        return 'short', KS, None
    s = turns = 0
    while s + 8 <= KS:
        s += 4
        turns += 1
    rem = KS - s - 4
    assert 0 <= rem <= 3 and rem == KS % 4
    return ('body' if turns else 'empty'), KS, rem


def test_k_forms_cover_every_factor_tile_count_and_loop_form(lib):
    nt_of = lambda K: (int(lib.oriana_kpad(K)) + 31) // 32
    for K, note in zc.K_FORMS_TABLE.items():
        assert note == (nt_of(K),) + _loop(K), K
    assert lib.oriana_zi_dispatch(zc.UPDATE, max(zc.K_FORMS) + 1, zc.F32, 1) == EKRANGE
    # every NT at its narrowest and at its widest K
    for nt in (1, 2, 3, 4):
        ks = [K for K in range(1, 129) if nt_of(K) == nt]
        assert min(ks) in zc.K_FORMS, (nt, min(ks))
        widest_kp = [K for K in ks if lib.oriana_kpad(K) == lib.oriana_kpad(max(ks))]
        assert set(widest_kp) & set(zc.K_FORMS), (nt, widest_kp)
        assert _unpack(lib.oriana_zi_dispatch(zc.UPDATE, min(ks), zc.F32, 1)) == (zc.F32_FAMILY, nt, 0)
    # every loop form (the loop does not know NT: KS is a run-time value of one kernel template)
    seen = set()
    for K in zc.K_FORMS:
        form, KS, rem = _loop(K)
        seen.add((form, KS if form == 'short' else rem))
    assert seen >= set(zc.LOOP_FORMS), sorted(set(zc.LOOP_FORMS) - seen)
    assert {K % 2 for K in zc.K_FORMS} == {0, 1}
    # the rate cases of ORIANA_MATRIX_F32 run every K of the table, the other two entries take it whole
    assert {K for K, a, m, t in zc.RATE_CASES if a == zc.F32} >= set(zc.K_FORMS)
    assert {nt_of(K) for K in zc.GENE_RATE_LONG_KS} == {1, 2, 3, 4}


# ---- 3. the batches of the gene rate -------------------------------------------------------------------------------------------

def test_long_batches_pass_the_spill_and_go_on():
    """At GENE_RATE_RANGES ranges (what oriana_zi_gene_rate_ranges answers on an MI355X; the GPU test asserts it) a range of the
    long batch holds more than 4096 cells, the last one fewer; the ranges of the mid batch pass 256 cells and stay below 4096."""
    def ranges(n):
        ips = (-(-n // zc.GENE_RATE_RANGES) + 31) // 32 * 32
        return ips, n - (-(-n // ips) - 1) * ips, -(-n // ips)
    ips, last, count = ranges(zc.LONG_N)
    assert count == zc.GENE_RATE_RANGES and 4096 + 32 < ips < 2 * 4096 and 256 < last < 4096
    assert zc.LONG_N == 132128 and zc.LONG_M == 36 and 32 < zc.LONG_M < 64
    ips, last, count = ranges(zc.MID_N)
    assert count == zc.GENE_RATE_RANGES and ips == last == 288


# ---- 4. every case exercises the sigmoid ---------------------------------------------------------------------------------------

def _shapes():
    s = {(K, zc.N_BODY, zc.M_REAL) for K, _, _, _ in zc.RATE_CASES} | {(K, zc.N_BODY, zc.M_REAL) for K in zc.K_FORMS}
    s |= {(K, n, m) for K, _, n, m, _ in zc.RATE_EDGE_CASES} | {(zc.GENE_EDGE_K, n, m) for n, m in zc.EDGE_SHAPES}
    s |= {(K, zc.LONG_N, zc.LONG_M) for K in zc.GENE_RATE_LONG_KS} | {(zc.MID_K, zc.MID_N, zc.MID_M)}
    return sorted(s)


def test_every_case_exercises_the_sigmoid():
    worst = {}
    for K, n, m in _shapes():
        X, U, V, pi_d = zc.inputs(K, n, m)
        d = zr.dropout_f32(X, V, pi_d, U)
        f = zc.middle_fraction(d)
        assert f > zc.MIDDLE_MIN, 'K = %d at %d x %d: %.3f of the entries in the middle of the sigmoid' % (K, n, m, f)
        z = X[:, zc.PI_ZERO] == 0
        assert (d[z, zc.PI_ZERO] == np.float32(1e-10)).all() and (d[~z, zc.PI_ZERO] == 1).all() and (d[:, zc.PI_ONE] == 1).all()
        assert not X[:, zc.ZERO_GENE].any() and (n == 1 or not X[min(zc.ZERO_CELL, n - 1)].any())
        assert n < 200 or (X[:, zc.PI_ZERO] != 0).any()
        lam = float((U @ V.T).mean()) if n * m * K < 5e7 else 1.0
        assert abs(lam - 1.0) < 1e-9
        key = (n, m)
        worst[key] = (min(worst.get(key, (1.0, 0.0))[0], f), max(worst.get(key, (1.0, 0.0))[1], f))
    for key in sorted(worst):
        print('%d x %d: %.3f .. %.3f of the entries have 0.01 < d < 0.99' % (key + worst[key]))
    lo, hi = worst[(zc.N_BODY, zc.M_REAL)]
    assert 0.6 < lo <= hi < 0.7
    # the same (K, n, m) again: the same arrays
    assert zc.inputs(30)[1] is zc.inputs(30, zc.N_BODY, zc.M_REAL)[1]
    assert np.array_equal(zc.inputs(30)[2], zc._inputs.__wrapped__(30, zc.N_BODY, zc.M_REAL)[2])


# ---- 5. the bounds reject what a wrong index would compute ---------------------------------------------------------------------

@pytest.mark.parametrize('K', [K for K, note in zc.K_FORMS_TABLE.items() if note[3] == 3])
def test_a_dropped_remainder_step_is_outside_every_bound(K):
    """The third step of the epilogue's remainder (rem = 3) is the last pair of factors.  Lambda without it, evaluated in
    float64, misses the bound of each of the three entries by orders of magnitude; so does one wrong d_ij in the rate of a cell,
    and a range's first 4096 cells lost from G (the spill that overwrites where it should add)."""
    import zi_score_reference as zs
    from helpers import RTOL, err_colrel
    X, U, V, pi_d = zc.inputs(K)
    keep = 2 * ((K + 1) // 2 - 1)
    d = zr.dropout_f32(X, V, pi_d, U).astype(np.float64)
    dw = zr.dropout_f32(X, V[:, :keep], pi_d, U[:, :keep]).astype(np.float64)
    e_rate, e_gene = err_colrel(dw @ V, d @ V), err_colrel(dw.T @ U, d.T @ U)
    ref, Lam, lg, g = zs.dropout_sums(X, V, pi_d, U)
    wrong = zs.dropout_sums(X, V[:, :keep], pi_d, U[:, :keep])[0]
    over = np.abs(wrong - ref) / zs.dropout_bound(K, Lam, lg, g)
    print('K=%d without factors %d..: rate %.2e, G %.2e (bound %.0e); cell bound %.1f .. %.1f of its bound' % (
        K, keep, e_rate, e_gene, RTOL, over.min(), over.max()))
    assert e_rate > 100 * RTOL and e_gene > 100 * RTOL
    assert np.median(over) > 10
    # one d_ij of one cell: 1 where the sigmoid said less
    i, j = 40, int(np.argmin(np.where((X[40] == 0) & (pi_d > 0) & (pi_d < 1), d[40], 2.0)))
    d1 = d.copy()
    d1[i, j] = 1.0
    e_one = err_colrel(d1 @ V, d @ V)
    print('  d[%d, %d] = 1 for %.3f: rate %.2e' % (i, j, d[i, j], e_one))
    assert d[i, j] < 0.9 and e_one > 10 * RTOL
    # 4096 of a range's 4160 cells lost
    lost = d[:280].T @ U[:280]
    assert err_colrel(d.T @ U - lost, d.T @ U) > 1000 * RTOL


def test_inactive_patterns_are_what_they_say():
    p = zc.inactive_patterns()
    assert sorted(p) == ['group-of-128', 'group-of-256', 'scattered']
    a = p['group-of-256']
    assert not a[:256].any() and a[256:].all()
    a = p['group-of-128']
    assert a[:128].all() and not a[128:256].any() and a[256:].all()
    a = p['scattered']
    assert 0 < (a == 0).sum() < 16 and all(a[g:g + 128].any() for g in range(0, zc.N_BODY, 128)) and not a[0] and not a[-1]
    assert sorted(zc.inactive_patterns(33)) == ['scattered'] and zc.inactive_patterns(1) == {}
