"""Seeded inputs shared by tools/make_activity_fixture.py (which records what the reference's audio/activity.py returns for them in
tests/golden/reference_activity.json) and the tests that replay them.  Everything is regenerated from ``np.random.default_rng(seed)``."""

from __future__ import annotations

import numpy as np

SR, CD = 8000, 1.0   # chunk = 8000 samples >= 4096, so smart_crop analyses frames of 1024 at hops of 512
CHUNK = int(SR * CD)


def _burst(x, rng, at_s, amp, dur_s=0.25, f=1800.0):
    a, n = int(at_s * SR), int(dur_s * SR)
    n = min(n, x.shape[0] - a)
    t = np.arange(n) / SR
    x[a : a + n] += (amp * np.sin(2 * np.pi * f * t) * np.hanning(n)).astype(np.float32)


def crop_signal(name: str, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if name == "zeros":
        return np.zeros(5 * SR, np.float32)
    if name == "short":
        return (0.1 * rng.standard_normal(5000)).astype(np.float32)
    if name == "one_chunk":
        return (0.1 * rng.standard_normal(CHUNK)).astype(np.float32)
    x = (1e-3 * rng.standard_normal(10 * SR)).astype(np.float32)
    if name == "four_bursts":
        for at, amp in ((1.2, 0.5), (3.9, 0.9), (6.4, 0.3), (8.8, 0.7)):
            _burst(x, rng, at, amp, 0.9)
    elif name == "close_bursts":   # two stretches nearer than half a chunk, one far away
        _burst(x, rng, 3.0, 0.8, 1.0)
        _burst(x, rng, 4.2, 0.6, 1.0)
        _burst(x, rng, 8.0, 0.4, 1.0)
    elif name == "end_burst":
        _burst(x, rng, 9.4, 0.9, 0.6)
        _burst(x, rng, 2.0, 0.2, 2.0)
    elif name == "ties":           # a square wave of constant amplitude: many frames with exactly equal energy
        x = np.where((np.arange(10 * SR) // 256) % 2 == 0, 0.25, -0.25).astype(np.float32)
        x[3 * SR : 4 * SR] *= 2
        x[7 * SR : 8 * SR] *= 2
    elif name == "quantised":
        x = (np.round(rng.standard_normal(10 * SR) * 4) / 4).astype(np.float32) * 0.1
    else:
        raise KeyError(name)
    return x


CROP_CASES = [("zeros", 1), ("short", 2), ("one_chunk", 3), ("four_bursts", 4), ("close_bursts", 5), ("end_burst", 6), ("ties", 7), ("quantised", 8)]


def activity_input(name: str, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if name == "zeros_map":
        return np.zeros((257, 32), np.float32)
    if name == "sparse_map":       # a quiet map with a few loud cells
        x = (0.01 * np.abs(rng.standard_normal((257, 64)))).astype(np.float32)
        x[40:60, 10:30] += 0.5
        return x
    if name == "broadband_map":    # the evenly spaced samples are silent, everything else is noise: ratio > max_active -> 0.0
        x = np.abs(rng.standard_normal((257, 64))).astype(np.float32) + np.float32(0.1)
        x.ravel()[np.linspace(0, x.size - 1, 512, dtype=int)] = 0.0
        return x
    if name == "small_map":        # n = 400 < subsample
        return np.abs(rng.standard_normal((20, 20))).astype(np.float32)
    if name == "odd_small":        # n = 399: odd m
        return rng.standard_normal(399).astype(np.float32)
    if name == "tied_map":
        return (np.round(np.abs(rng.standard_normal((257, 16))) * 3) / 3).astype(np.float32)
    if name == "half_tied":
        x = rng.standard_normal(4096).astype(np.float32)
        x[::2] = 0.5
        return x
    if name == "waveform":
        x = (0.02 * rng.standard_normal(CHUNK)).astype(np.float32)
        _burst(x, rng, 0.3, 0.8, 0.2)
        return x
    if name == "negative_wave":
        return (-np.abs(rng.standard_normal(6000))).astype(np.float32)
    raise KeyError(name)


ACTIVITY_CASES = [("zeros_map", 11), ("sparse_map", 12), ("broadband_map", 13), ("small_map", 14), ("odd_small", 15), ("tied_map", 16), ("half_tied", 17),
                  ("waveform", 18), ("negative_wave", 19)]


def sort_samples(seed: int, kind: str) -> list[np.ndarray]:
    """Lists for sort_by_activity / sort_by_s2n: maps (or waveforms) of differing activity, two of them identical (a tie)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(6):
        if kind == "maps":
            x = (0.01 * np.abs(rng.standard_normal((64, 32)))).astype(np.float32)
            x[: 4 * i, : 3 * i] += 0.5
        else:
            x = (0.01 * rng.standard_normal(4000)).astype(np.float32) + np.float32(0.005 * i)
            x[: 300 * i] += 0.4
        out.append(x)
    out.insert(3, out[1].copy())
    out.append(np.zeros_like(out[0]))
    return out


SORT_CASES = [("maps", 21), ("waves", 22)]
STE_CASES = [(31, 1024), (32, 5000)]   # (seed, samples)


def ste_signal(seed: int, n: int) -> np.ndarray:
    return (np.random.default_rng(seed).standard_normal(n) * 0.3).astype(np.float32)


def locate(chunk: np.ndarray, audio: np.ndarray) -> int:
    """Start of ``chunk`` in ``audio`` (-1: padded short recording, -2: not found)."""
    n = chunk.shape[0]
    if audio.shape[0] < n:
        return -1
    win = np.lib.stride_tricks.sliding_window_view(audio, n)
    hits = np.flatnonzero((win[:, 0] == chunk[0]) & (win[:, -1] == chunk[-1]) & (win[:, n // 2] == chunk[n // 2]))
    for h in hits:
        if np.array_equal(win[h], chunk):
            return int(h)
    return -2
