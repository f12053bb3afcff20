"""The clamp in front of the shift (``i8_front_strip_kernel``: csrc/bn_requant.h, ``shifted_bounds``).

The strip form of the requantisation ends in ``clamp(h >> e1, lo, hi)`` with ``h = hi32(x m + C)``.  The front strip kernel clamps first,
against bounds shifted once per channel, so that the shift is the last instruction and can deposit its byte where it is read:

    clamp(h >> e1, lo, hi) == clamp(h, lo << e1, ((hi + 1) << e1) - 1) >> e1

for every int32 ``h``, every ``e1 >= 0`` and every ``lo <= hi`` (the arithmetic shift is monotone and floors: ``h >> e1 >= lo`` iff
``h >= lo << e1`` and ``h >> e1 <= hi`` iff ``h < (hi + 1) << e1``).  ``_strip_requant`` admits shifts ``e = e1 + 1`` in 1 .. 22, so the
shifted bounds stay inside +-2^28.  Plain numpy, no device."""
from __future__ import annotations

import numpy as np

INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1
E1S = range(0, 22)
GRID = (-128, -127, -64, -1, 0, 5, 100, 126, 127)
BOUNDS = [(lo, hi) for lo in GRID for hi in GRID if lo <= hi]


def shifted_bounds(lo: int, hi: int, e1: int) -> tuple[int, int]:
    """The kernel's per-channel bounds (same expressions as ``shifted_bounds`` in csrc/bn_requant.h)."""
    return lo << e1, ((hi + 1) << e1) - 1


def _values(lo: int, hi: int, e1: int, rnd: np.ndarray) -> np.ndarray:
    a, b = shifted_bounds(lo, hi, e1)
    near = [t + d for t in (a, b, a - 1, b + 1) for d in (-2, -1, 0, 1, 2)]
    return np.concatenate([np.asarray(near + [INT32_MIN, INT32_MAX], np.int64), rnd])


def test_grid_covers_what_the_issue_names():
    assert (-128, 127) in BOUNDS
    assert any(lo == hi for lo, hi in BOUNDS)
    assert any(-128 < lo < hi < 127 for lo, hi in BOUNDS)
    assert list(E1S) == list(range(22))


def test_clamp_before_shift_equals_shift_before_clamp():
    rnd = np.random.default_rng(20260).integers(INT32_MIN, INT32_MAX, 100_000, dtype=np.int64, endpoint=True)
    for e1 in E1S:
        for lo, hi in BOUNDS:
            h = _values(lo, hi, e1, rnd)
            assert h.min() >= INT32_MIN and h.max() <= INT32_MAX
            a, b = shifted_bounds(lo, hi, e1)
            want = np.clip(h >> e1, lo, hi)
            got = np.clip(h, a, b) >> e1
            bad = np.nonzero(want != got)[0]
            assert bad.size == 0, f"e1 = {e1}, bounds ({lo}, {hi}): h = {int(h[bad[0]])} gives {int(got[bad[0]])}, the shift-first form {int(want[bad[0]])}"


def test_shifted_bounds_fit_the_registers():
    """Both bounds are int32 with room to spare for every admitted shift, and ordered (``v_med3_i32`` needs lo <= hi)."""
    for e1 in E1S:
        for lo, hi in BOUNDS:
            a, b = shifted_bounds(lo, hi, e1)
            assert -(2**28) <= a <= b < 2**28


def test_low_byte_of_the_result_is_the_int8_value():
    """The deposit writes the LOW BYTE of the shifted dword: for results inside int8 that byte is the value's two's complement."""
    rnd = np.random.default_rng(7).integers(INT32_MIN, INT32_MAX, 10_000, dtype=np.int64, endpoint=True)
    for e1 in (0, 1, 17, 21):
        for lo, hi in ((-128, 127), (-100, 100), (5, 5)):
            a, b = shifted_bounds(lo, hi, e1)
            q = np.clip(rnd, a, b) >> e1
            assert np.array_equal((q & 0xFF).astype(np.uint8).view(np.int8).astype(np.int64), q)
