# -*- coding: utf-8 -*-
"""The assembly of a held-out score from its (n', 4) terms (FactorModel._score_result / _mean_score): no GPU, no HIP library."""
import math

import numpy as np

from oriana_amd.models.base import FactorModel

T = np.array([[-1234.5678901234, 321.000000001, 17.25, 0.1],
              [1.0, 1e16, -1e16, 1e-3],          # (the order of additions shows under the pCMF signs)
              [1.0, 1e16, 1e16, 1e-3]], dtype=np.float64)   # (and under the zero-inflated ones)
EXTRAS = {'a1': np.ones((3, 2)), 'froze_at': np.array([0, 5, 9], dtype=np.int32)}


def _check(names, signs, expected):
    before = T.copy()
    s = FactorModel._score_result(T, names, signs, dict(EXTRAS), False)
    assert isinstance(s, np.ndarray) and s.dtype == np.float64 and s.shape == (3,)
    assert np.array_equal(s, expected)
    d = FactorModel._score_result(T, names, signs, dict(EXTRAS), True)
    assert set(d) == {'score'} | set(names) | set(EXTRAS)
    assert np.array_equal(d['score'], expected)
    for j, name in enumerate(names):
        assert np.array_equal(d[name], T[:, j]) and d[name].dtype == np.float64
        assert not np.shares_memory(d[name], T)
    assert not np.shares_memory(d['score'], T) and not np.shares_memory(s, T)
    for k, v in EXTRAS.items():
        assert d[k] is v
    assert np.array_equal(T, before)


def test_pcmf_signs_left_to_right():
    _check(('data', 'lgamma', 'product', 'kl'), '+---', T[:, 0] - T[:, 1] - T[:, 2] - T[:, 3])


def test_zi_signs_left_to_right():
    _check(('data', 'lgamma', 'dropout', 'kl'), '+-+-', T[:, 0] - T[:, 1] + T[:, 2] - T[:, 3])


def test_the_order_of_additions_is_visible_in_these_terms():
    """(Rows 1 and 2 separate left-to-right from any other association, so the two tests above can tell.)"""
    assert ((T[1, 0] - T[1, 1]) - T[1, 2]) - T[1, 3] == -1e-3 != T[1, 0] - (T[1, 1] + T[1, 2] + T[1, 3])
    assert ((T[2, 0] - T[2, 1]) + T[2, 2]) - T[2, 3] == -1e-3 != T[2, 0] + (T[2, 2] - T[2, 1]) - T[2, 3]


def test_mean_score():
    empty = FactorModel._mean_score(np.empty(0, dtype=np.float64))
    assert isinstance(empty, float) and math.isnan(empty)
    s = T[:, 0] - T[:, 1]
    m = FactorModel._mean_score(s)
    assert type(m) is float and m == float(s.mean())
    assert FactorModel._mean_score({'score': s, 'data': T[:, 0]}) == m
    assert math.isnan(FactorModel._mean_score({'score': s[:0]}))
