# -*- coding: utf-8 -*-
"""The argument errors of the t-SNE entry points (include/oriana_hip.h): all of them are raised before any HIP call, so this runs
without a GPU."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from oriana_amd import _lib
    return _lib.load()


_BUF = (ctypes.c_double * 8)()


@pytest.fixture(scope='module')
def p():
    """A 16-byte aligned host address inside _BUF: never dereferenced by a call that fails its argument checks."""
    a = ctypes.addressof(_BUF)
    return a - a % 16 + 16


def test_symbols_are_exported_and_bound(lib):
    from oriana_amd import _lib
    for name in ('oriana_tsne_affinities', 'oriana_tsne_affinity_steps', 'oriana_tsne_attract', 'oriana_tsne_repulse',
                 'oriana_tsne_repulse_scratch_bytes_for'):
        assert hasattr(lib, name) and name in _lib.declared_symbols(), name
    assert lib.oriana_tsne_affinity_steps() >= 100


def test_affinities_argument_errors(lib, p):
    def aff(D=p, n=4, k=3, perp=2.0, out=p, beta=p):
        return lib.oriana_tsne_affinities(D, n, k, perp, out, beta, None)

    for kw in (dict(n=-1), dict(k=0), dict(k=-3), dict(perp=0.5), dict(perp=float('nan')), dict(perp=float('inf')), dict(perp=-2.0),
               dict(D=None), dict(out=None), dict(beta=None)):
        assert aff(**kw) == -1, kw                                               # ORIANA_EINVAL
    assert aff(k=2 ** 31) == -2                                                  # ORIANA_EKRANGE
    assert aff(n=0, D=None, out=None, beta=None) == 0                            # no rows: a no-op, no HIP call


def test_attract_argument_errors(lib, p):
    def att(rp=p, col=p, val=p, Y=p, n=4, attr=p, kl=p):
        return lib.oriana_tsne_attract(rp, col, val, Y, n, attr, kl, None)

    for kw in (dict(n=-1), dict(n=2 ** 31), dict(rp=None), dict(Y=None), dict(attr=None), dict(kl=None), dict(Y=p + 4)):
        assert att(**kw) == -1, kw
    assert att(n=0, rp=None, Y=None, attr=None, kl=None) == 0


def test_repulse_argument_errors(lib, p):
    def rep(Q=p, nq=10, Y=p, n=10, out=p, z=p, acc=0, scratch=p, blocks=0):
        return lib.oriana_tsne_repulse(Q, nq, Y, n, out, z, acc, scratch, blocks, None)

    for kw in (dict(nq=-1), dict(n=-1), dict(blocks=-1), dict(nq=2 ** 31), dict(n=2 ** 31 - 8), dict(n=2 ** 40), dict(Q=None),
               dict(Y=None), dict(out=None), dict(z=None), dict(scratch=None), dict(scratch=p + 8), dict(Q=p + 4), dict(Y=p + 4)):
        assert rep(**kw) == -1, kw
    assert rep(nq=0, Q=None, out=None, z=None) == 0                              # no queries: a no-op, no HIP call
    assert rep(nq=0, Q=None, out=None, z=None, n=0, Y=None) == 0
    by = lib.oriana_tsne_repulse_scratch_bytes_for
    for args in ((-1, 10, 0), (10, -1, 0), (10, 10, -1), (2 ** 31, 10, 0), (10, 2 ** 31 - 8, 0)):
        assert by(*args) == -1, args
    # 1,536 bytes per query tile and range; ranges hold whole 8-candidate steps and none is empty
    assert by(300, 300, 1) == 5 * 1536 and by(300, 300, 3) == 5 * 3 * 1536 and by(64, 7, 5) == 1536 and by(65, 17, 5) == 2 * 3 * 1536
    assert by(300, 33, 4) == 5 * 3 * 1536                                        # (5 steps in 4 ranges: 2 + 2 + 1)
    assert by(0, 0, 0) == 16 and by(10, 0, 0) == 16
    assert by(2 ** 31 - 1, 2 ** 31 - 9, 1) == 2 ** 25 * 1536
