# -*- coding: utf-8 -*-
"""helpers.guarded on the CPU: the view has exactly the size asked for on a 256-byte boundary, the three fills are what they
claim, and check() notices ONE byte written right before the start, right behind the end, or at the far end of either band."""
import numpy as np
import pytest
import torch

from helpers import GUARD_BYTES, SCRATCH_VARIANTS, guarded, guarded_out, guarded_variant

SIZES = (0, 8, 1000, 4096, 70000)


def _raw(view):
    """The whole allocation behind a guarded view, as bytes, and the view's offset in it."""
    st = view.untyped_storage()
    raw = torch.empty(0, dtype=torch.uint8).set_(st)
    return raw, view.storage_offset() * view.element_size()


@pytest.mark.parametrize('nbytes', SIZES)
@pytest.mark.parametrize('variant', sorted(SCRATCH_VARIANTS))
def test_size_alignment_and_fill(nbytes, variant):
    interior, guard = SCRATCH_VARIANTS[variant]
    view, check = guarded_variant(nbytes, variant, torch.uint8, 'cpu')
    raw, lo = _raw(view)
    assert view.numel() == nbytes and (raw.data_ptr() + lo) % 256 == 0 and (nbytes == 0 or view.data_ptr() == raw.data_ptr() + lo)
    assert lo >= GUARD_BYTES and raw.numel() - lo - nbytes >= GUARD_BYTES
    assert bool((view == interior).all())
    assert bool((raw[:lo] == guard).all()) and bool((raw[lo + nbytes:] == guard).all())
    check()


def test_the_nan_fill_is_nan_in_both_widths_and_minus_one():
    for dtype in (torch.float32, torch.float64):
        view, _ = guarded_variant(4096, 'nan', dtype, 'cpu')
        assert view.numel() * view.element_size() == 4096 and bool(torch.isnan(view).all())
        raw, lo = _raw(view)                                   # a float read past either end meets NaN as well
        assert bool(torch.isnan(raw[lo - 64:lo].view(dtype)).all()) and bool(torch.isnan(raw[lo + 4096:lo + 4160].view(dtype)).all())
    for dtype in (torch.int32, torch.int64):
        view, _ = guarded_variant(4096, 'nan', dtype, 'cpu')
        assert bool((view == -1).all())
    view, _ = guarded_variant(4096, 'zero', torch.float64, 'cpu')
    assert bool((view == 0).all())


def test_the_stale_fill_is_what_the_previous_call_left():
    view, check = guarded_variant(800, 'stale', torch.float64, 'cpu')
    left = torch.from_numpy(np.random.default_rng(3).normal(size=100))
    view.copy_(left)                                           # "a previous valid call": it writes inside the buffer only
    check()
    raw, lo = _raw(view)
    assert bool((raw[lo:lo + 800].view(torch.float64) == left).all()) and bool((raw[:lo] == 0xA5).all())
    assert bool((raw[lo + 800:] == 0xA5).all())


@pytest.mark.parametrize('variant', sorted(SCRATCH_VARIANTS))
@pytest.mark.parametrize('where', ['before', 'behind', 'first', 'last'])
def test_one_byte_outside_is_noticed(variant, where):
    nbytes = 1000
    view, check = guarded_variant(nbytes, variant, torch.uint8, 'cpu')
    raw, lo = _raw(view)
    at = {'before': lo - 1, 'behind': lo + nbytes, 'first': 0, 'last': raw.numel() - 1}[where]
    view[0] = 0x11                                             # writes inside are the callee's business
    view[nbytes - 1] = 0x11
    check()
    raw[at] = 0x5A
    with pytest.raises(AssertionError, match='guard bytes'):
        check()
    raw[at] = SCRATCH_VARIANTS[variant][1]
    check()


def test_nothing_but_whole_elements():
    with pytest.raises(AssertionError):
        guarded(10, dtype=torch.float32, device='cpu')


def test_guarded_out():
    out, check = guarded_out((7, 5), torch.float64, 'nan', 'cpu')
    assert out.shape == (7, 5) and out.is_contiguous() and bool(torch.isnan(out).all())
    idx, _ = guarded_out((3, 4), torch.int32, 'nan', 'cpu')
    assert bool((idx == -1).all())
    acc, check2 = guarded_out((4,), torch.float32, 'zero', 'cpu')
    assert bool((acc == 0).all())
    out.fill_(1.0)
    check()
    raw, lo = _raw(out)
    raw[lo + 7 * 5 * 8] = 0
    with pytest.raises(AssertionError, match='behind'):
        check()
    check2()
