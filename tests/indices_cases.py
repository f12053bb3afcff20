"""Inputs of the acoustic-index tests (tests/test_indices_host.py, tests/test_gpu_indices.py): everything here runs on the CPU.

Two kinds of spectrogram batches ``[B = 3, 257, W]`` float32, ``W`` in ``WIDTHS``:

* integer-valued (entries 0 .. 15): every sum of ``S``, ``|dS|`` and ``P = S * S`` over a row, and of ``p_f`` over a default band, stays
  below 2^24 and is exact in float32 in any order, so ``ACI_f``, ``CVR_f``, the band counts and NDSI have one float32 value;
* float-valued: plain numpy STFT magnitudes (the framing of ``bn_stft_mag``: centre zero padding of 256, periodic Hann, hop ``T // W``) of
  3 s at 22050 Hz of a tone, two tones, white noise, gated chirps and zeros.

``WIDTHS``: 4 and 6 are the smallest rows with and without whole 16-byte pieces, 256 fills every lane once, 260 needs a second piece per
lane (a piece boundary inside the row) — each also read through a view that starts one float off a 16-byte boundary by the GPU tests.

The tolerance of the float cases is not invented: ``YARDSTICK_*`` is the largest error of ``indices_reference_f32`` (float32 numpy, its
own pairwise sums) against ``indices_reference`` (float64) over exactly these float cases, measured on the CPU
(``measure_yardstick``; ``test_indices_host.py`` checks the constants still cover it), and the kernel is allowed ``SLACK`` = 8 times that:
its order of summation differs (a lane's elements, then a tree) but both errors grow with log n.
"""

from __future__ import annotations

import functools

import numpy as np

from birdnet_stm32.evaluation import indices as IX

SAMPLE_RATE, CHUNK_SECONDS = 22050, 3.0
WIDTHS = (4, 6, 256, 260)
BATCH = 3
PARAMS = IX.IndexParams()

# Largest error of the float32 restatement against float64 over float_cases() (measure_yardstick(), numpy 2.2 on x86-64):
# relative, over the scalars with |value| >= NEAR_ZERO; absolute, over the per-bin values and the scalars below NEAR_ZERO.
# Measured 4.08e-6 (BI of white noise at W = 260: a sum of 139 differences of nearly equal levels) and 7.06e-6 (ACI_f of the gated chirps at
# W = 256); the constants are those rounded up, so a numpy whose pairwise sums split a row elsewhere still lies below them.
NEAR_ZERO = 0.05
YARDSTICK_REL = 4.5e-6
YARDSTICK_ABS = 7.5e-6
SLACK = 8.0
RTOL, ATOL = SLACK * YARDSTICK_REL, SLACK * YARDSTICK_ABS


def stft_mag(x: np.ndarray, W: int) -> np.ndarray:
    """Raw magnitudes ``[257, W]`` float32 of one chunk, float64 arithmetic rounded once."""
    x = np.asarray(x, np.float64)
    hop = x.shape[0] // W
    padded = np.pad(x, (256, 256))
    idx = np.arange(W)[:, None] * hop + np.arange(512)[None, :]
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(512) / 512.0)
    return np.abs(np.fft.rfft(padded[idx] * win, axis=1)).T.astype(np.float32)


def signals() -> dict:
    """The five signal families, 3 s at 22050 Hz, peak 1 (as the ingest leaves chunks)."""
    n = int(SAMPLE_RATE * CHUNK_SECONDS)
    t = np.arange(n) / SAMPLE_RATE
    rng = np.random.default_rng(20261021)
    gate = ((t % 0.5) < 0.2).astype(np.float64)
    sweep = np.sin(2 * np.pi * (2500.0 * t + 0.5 * 4000.0 * (t % 0.5) ** 2 / 0.2 * 0.4)) * gate
    out = {
        "tone3k": np.sin(2 * np.pi * 3000.0 * t),
        "tone1k5": np.sin(2 * np.pi * 1500.0 * t),
        "two_tones": 0.6 * np.sin(2 * np.pi * 1500.0 * t) + 0.4 * np.sin(2 * np.pi * 5200.0 * t),
        "noise": rng.standard_normal(n),
        "chirps": sweep + 0.01 * rng.standard_normal(n),
        "zeros": np.zeros(n),
    }
    return {k: (v / np.abs(v).max() if np.abs(v).max() > 0 else v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def float_cases() -> tuple:
    """``(name, S [3, 257, W] float32)``: two batches per width, every family at every width."""
    sig = signals()
    groups = (("tones_noise", ("tone3k", "two_tones", "noise")), ("chirps_zeros_tone", ("chirps", "zeros", "tone1k5")))
    return tuple((f"{gname}_w{W}", np.stack([stft_mag(sig[k], W) for k in keys])) for W in WIDTHS for gname, keys in groups)


def band_edge_bins() -> list[int]:
    """First and last bin of each default band, from ``f_k``."""
    f = IX.bin_frequencies(SAMPLE_RATE)
    bins = []
    for lo, hi in (PARAMS.anthro, PARAMS.bio):
        inside = np.flatnonzero((f >= lo) & (f < hi))
        bins += [int(inside[0]), int(inside[-1])]
    return bins


@functools.lru_cache(maxsize=None)
def integer_cases() -> tuple:
    """``(name, S [3, 257, W] float32 with integer entries 0 .. 15)``: two batches per width.

    ``zeros``: a dense chunk with all-zero bins, an all-zero chunk, a chunk with energy only in bin 256;
    ``edges``: energy only on the first and last bin of each default band, a dense chunk, a sparse chunk (most cells 0)."""
    rng = np.random.default_rng(7)
    cases = []
    for W in WIDTHS:
        dense = rng.integers(0, 16, (257, W)).astype(np.float32)
        dense[[0, 5, 46, 47, 100, 255]] = 0.0
        top = np.zeros((257, W), np.float32)
        top[256] = rng.integers(1, 16, W)
        cases.append((f"zeros_w{W}", np.stack([dense, np.zeros((257, W), np.float32), top])))
        edges = np.zeros((257, W), np.float32)
        for k in band_edge_bins():
            edges[k] = rng.integers(0, 16, W)
            edges[k, 0] = 15.0
        full = rng.integers(0, 16, (257, W)).astype(np.float32)
        sparse = (rng.integers(0, 16, (257, W)) * (rng.random((257, W)) < 0.1)).astype(np.float32)
        sparse[3, W - 1] = 15.0
        cases.append((f"edges_w{W}", np.stack([edges, full, sparse])))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def reference(kind: str, name: str):
    """``(scalars [3, 8], per-bin [3, 3, 257])`` float64 of a case by ``indices_reference``; computed once, shared, read-only."""
    S = dict(float_cases() if kind == "float" else integer_cases())[name]
    got = [IX.indices_reference(s, SAMPLE_RATE, PARAMS) for s in S]
    out = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_f32(kind: str, name: str):
    """The same by ``indices_reference_f32`` (float32 arrays)."""
    S = dict(float_cases() if kind == "float" else integer_cases())[name]
    got = [IX.indices_reference_f32(s, SAMPLE_RATE, PARAMS) for s in S]
    out = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
    for a in out:
        a.setflags(write=False)
    return out


def measure_yardstick() -> tuple[float, float]:
    """``(relative, absolute)`` largest error of the float32 restatement against float64 over ``float_cases()`` (see the module doc)."""
    rel = ab = 0.0
    for name, _S in float_cases():
        s64, b64 = reference("float", name)
        s32, b32 = reference_f32("float", name)
        err = np.abs(s32.astype(np.float64) - s64)
        big = np.abs(s64) >= NEAR_ZERO
        if big.any():
            rel = max(rel, float((err[big] / np.abs(s64[big])).max()))
        if (~big).any():
            ab = max(ab, float(err[~big].max()))
        ab = max(ab, float(np.abs(b32.astype(np.float64) - b64).max()))
    return rel, ab


def within(got: np.ndarray, ref64: np.ndarray) -> np.ndarray:
    """``|got - ref64| <= ATOL + RTOL * |ref64|`` per element."""
    return np.abs(np.asarray(got, np.float64) - ref64) <= ATOL + RTOL * np.abs(ref64)
