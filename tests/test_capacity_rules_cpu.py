"""The binning-capacity bookkeeping of the rasterizer's host side (rasterizer._first_cap / _note_fitted / _note_overflow): the one running
estimate every route (the two autograd entries, the late count wait, the compiled host's entry) reads and raises.  Pure host arithmetic:
the expected values are the rules written out literally."""
import pytest

from gaussianavatars_amd import rasterizer as R

Q = 1 << 16
KEY = (0, 208, 176, False)   # (device index, H, W, production path?)


def _round(n):
    return max(Q, (int(n) + Q - 1) // Q * Q)


@pytest.fixture(autouse=True)
def _clean_bookkeeping():
    hint, peak = dict(R._capacity_hint), R._forward_peak[0]
    R._capacity_hint.clear()
    R._forward_peak[0] = 0
    try:
        yield
    finally:
        R._capacity_hint.clear()
        R._capacity_hint.update(hint)
        R._forward_peak[0] = peak


@pytest.mark.parametrize("P", [0, 1, 8191, 8193, 100_000])
def test_first_cap_without_a_hint_is_a_rounded_multiple_of_the_splat_count(P):
    assert R._CAP_QUANTUM == Q and R._round_cap(P) == _round(P)
    assert R._first_cap(KEY, P, False) == _round(8 * P)
    assert R._first_cap(KEY[:3] + (True,), P, True) == _round(24 * P)
    assert not R._capacity_hint    # asking does not write


def test_first_cap_returns_a_hint_written_by_hand_raw():
    R._capacity_hint[KEY] = 1024
    assert R._first_cap(KEY, 100_000, False) == 1024


def test_note_fitted_keeps_a_quarter_headroom_and_never_falls_below_it():
    peak = 0
    for cap, I in ((65536, 0), (65536, 52428), (65536, 52429), (1 << 20, 70_000), (1 << 20, 600_000)):
        R._note_fitted(KEY, cap, I)
        assert R._capacity_hint[KEY] == max(_round(int(I * 1.25) + 1), min(cap, _round(2 * I + 1))), (cap, I)
        peak = max(peak, I)
        assert R._forward_peak[0] == peak
    assert int(52428 * 1.25) + 1 == 65536 and int(52429 * 1.25) + 1 == 65537     # the pair straddles one quantum
    R._note_fitted(KEY, 65536, 52428)
    assert R._capacity_hint[KEY] == 65536
    R._note_fitted(KEY, 65536, 52429)
    assert R._capacity_hint[KEY] == 131072
    assert R._forward_peak[0] == 600_000   # a smaller frame does not lower the peak


@pytest.mark.parametrize("I", [65537, 1_000_000])
def test_note_overflow_sets_the_hint_to_the_frame_plus_a_quarter(I):
    R._capacity_hint[KEY] = Q
    assert R._note_overflow(KEY, I) == _round(int(I * 1.25) + 1)
    assert R._capacity_hint[KEY] == _round(int(I * 1.25) + 1)
    assert R._first_cap(KEY, 1, False) == _round(int(I * 1.25) + 1)
    assert R._forward_peak[0] == 0         # a frame that rendered nothing is no peak
