"""Which chunks of a recording carry signal: short-time-energy cropping and activity ranking.

Same module path, function names, signatures, defaults and return types as the reference's ``birdnet_stm32/audio/activity.py``;
its loader (data/generator.py ``_process_file``) picks candidate chunks of a weakly-labelled file with ``smart_crop`` (long files) or
the plain chunk grid (short ones), ranks them with ``sort_by_activity`` and keeps the first few.

This numpy module is also the *specification* of the device path (csrc/bn_activity.hip): the two per-sample reductions are
written out here as explicit float32 operation orders --

* :func:`short_time_energy` -- ``np.mean(frame ** 2)`` over float32 frames, as numpy's pairwise summation evaluates it;
* :func:`activity_stats` -- the median / MAD / threshold / count chain of ``get_activity_ratio`` on float32 input

-- so that the kernels' float32 and integer results are compared with them for equality, not within a tolerance.  Everything that
orders or thresholds candidates (percentile, regions, ratios, ``max_active``, argsort) stays on the host, here, in float64.
"""

from __future__ import annotations

import numpy as np

_F32 = np.float32
_MAD_EPS = _F32(1e-10)
_PW_BLOCK = 128  # numpy's pairwise summation sums runs of at most 128 elements with eight strided accumulators


def _frame_count(n: int, frame_length: int, hop_length: int) -> int:
    return max(1, 1 + (n - frame_length) // hop_length)


def _pairwise_tree(parts: np.ndarray) -> np.ndarray:
    """Fold the last axis (a power of two long) as a balanced binary tree of float32 additions: ((p0+p1)+(p2+p3))+..."""
    while parts.shape[-1] > 1:
        parts = parts[..., 0::2] + parts[..., 1::2]
    return parts[..., 0]


def short_time_energy(audio: np.ndarray, frame_length: int = 1024, hop_length: int = 512) -> np.ndarray:
    """Mean square of every analysis frame, float32, in a fixed operation order.

    For float32 ``audio`` and full frames of a power-of-two length >= 128 the result equals
    ``np.float32(np.mean(audio[s : s + frame_length] ** 2))`` bit for bit.  The order, which the device kernel repeats:

    1. every sample is squared (one float32 multiplication);
    2. the frame is cut into blocks of 128 squares; inside a block eight accumulators ``r[j]`` take the squares
       ``j, j + 8, j + 16, ...`` one after another (sixteen values each, fifteen additions), and the block's sum is
       ``((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7))``;
    3. the block sums are added as a balanced binary tree (for 1024 samples: eight blocks, three levels);
    4. the total is divided by ``frame_length``.

    Frames that are not of this form (a signal shorter than one frame, other lengths) fall back to ``np.mean`` itself.
    There are ``max(1, 1 + (n - frame_length) // hop_length)`` frames.
    """
    audio = np.asarray(audio)
    n = audio.shape[0]
    n_frames = _frame_count(n, frame_length, hop_length)
    blocks = frame_length // _PW_BLOCK
    spelled = (
        audio.dtype == _F32 and n >= frame_length and frame_length >= _PW_BLOCK and frame_length % _PW_BLOCK == 0 and (blocks & (blocks - 1)) == 0
    )
    if not spelled:
        out = np.empty(n_frames, dtype=_F32)
        for f in range(n_frames):
            frame = audio[f * hop_length : f * hop_length + frame_length]
            out[f] = np.mean(frame**2)
        return out
    sq = audio * audio
    frames = np.lib.stride_tricks.sliding_window_view(sq, frame_length)[::hop_length][:n_frames]
    acc = frames.reshape(n_frames, blocks, _PW_BLOCK // 8, 8)
    r = acc[:, :, 0, :].copy()
    for i in range(1, _PW_BLOCK // 8):
        r = r + acc[:, :, i, :]
    block_sums = ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))
    return (_pairwise_tree(block_sums) / _F32(frame_length)).astype(_F32)


def _crop_starts(ste: np.ndarray, n: int, chunk_size: int, hop: int, max_chunks: int, energy_percentile: float) -> list[int]:
    """Start samples of the salient chunks, given the energy profile of a recording of ``n > chunk_size`` samples.

    Split from :func:`smart_crop` so that the device pipeline, which gets ``ste`` from ``bn_short_time_energy``, runs the same
    host decisions: percentile threshold, runs of frames at or above it, one chunk centred on each run's loudest frame
    (clamped into the recording), loudest runs first (stable), a start nearer than half a chunk to one already taken skipped.
    """
    centre = [max(0, n // 2 - chunk_size // 2)]
    if ste.max() < 1e-10:
        return centre
    active = ste >= np.percentile(ste, energy_percentile)
    padded = np.concatenate(([False], active, [False]))
    edges = np.flatnonzero(padded[1:] != padded[:-1])
    if edges.size == 0:
        return centre
    lo = edges[0::2]                              # first frame of every run
    # loudest frame of every run, first occurrence (np.argmax): frames between runs lie below the threshold, so the maximum over
    # [lo_i, lo_i+1) is the run's own; run_of[f] = index of the run frame f belongs to (meaningful where active)
    peak = np.maximum.reduceat(ste, lo)
    run_of = np.cumsum(padded[1:-1] & ~padded[:-2]) - 1
    hits = np.flatnonzero(active & (ste == peak[np.maximum(run_of, 0)]))
    frame = hits[np.concatenate(([True], run_of[hits][1:] != run_of[hits][:-1]))]
    starts = np.maximum(0, np.minimum(frame.astype(np.int64) * hop - chunk_size // 2, n - chunk_size)).tolist()
    taken: list[int] = []
    for i in np.argsort(-peak, kind="stable").tolist():   # loudest first; equal peaks keep their time order
        if all(abs(starts[i] - s) >= chunk_size // 2 for s in taken):
            taken.append(starts[i])
            if len(taken) >= max_chunks:
                break
    return taken if taken else [0]


def smart_crop_starts(audio: np.ndarray, sample_rate: int, chunk_duration: float, max_chunks: int = 5, energy_percentile: float = 75.0) -> list[int]:
    """The start samples :func:`smart_crop` cuts at (``[0]`` for a recording of at most one chunk, which is padded)."""
    chunk_size = int(sample_rate * chunk_duration)
    n = audio.shape[0]
    if n <= chunk_size:
        return [0]
    frame_len = min(1024, chunk_size // 4)
    ste = short_time_energy(audio, frame_length=frame_len, hop_length=frame_len // 2)
    return _crop_starts(ste, n, chunk_size, frame_len // 2, max_chunks, energy_percentile)


def smart_crop(audio: np.ndarray, sample_rate: int, chunk_duration: float, max_chunks: int = 5, energy_percentile: float = 75.0) -> list[np.ndarray]:
    """Up to ``max_chunks`` chunks around the loudest stretches of a long recording, loudest first.

    The energy profile uses frames of ``min(1024, chunk_size // 4)`` samples at half-frame hops.  Frames at or above the
    ``energy_percentile`` of the profile form runs; each run gives one chunk centred on its loudest frame.  A recording of
    at most one chunk is zero-padded to one chunk; a silent one (all energies < 1e-10) gives its centre chunk.

    Args:
        audio: 1-D mono signal (peak-normalised by the loader).
        sample_rate: samples per second.
        chunk_duration: chunk length in seconds.
        max_chunks: most chunks returned.
        energy_percentile: threshold on the energy profile.

    Returns:
        A list of float32 chunks of ``int(sample_rate * chunk_duration)`` samples.
    """
    chunk_size = int(sample_rate * chunk_duration)
    n = audio.shape[0]
    if n <= chunk_size:
        out = np.zeros(chunk_size, dtype=_F32)
        out[:n] = audio
        return [out]
    return [audio[s : s + chunk_size].astype(_F32) for s in smart_crop_starts(audio, sample_rate, chunk_duration, max_chunks, energy_percentile)]


def get_s2n_from_spectrogram(spectrogram: np.ndarray) -> float:
    """Mean over standard deviation of a spectrogram: a crude signal-to-noise figure."""
    return np.mean(spectrogram) / (np.std(spectrogram) + 1e-10)


def get_s2n_from_audio(audio: np.ndarray) -> float:
    """Mean over standard deviation of a waveform: a crude signal-to-noise figure."""
    return np.mean(audio) / (np.std(audio) + 1e-10)


def _ranked(samples: list[np.ndarray], values: np.ndarray, threshold: float) -> list[np.ndarray]:
    """``samples`` by descending ``values`` (``np.argsort(values)[::-1]``: ties fall as that gives them), those below ``threshold`` dropped, one kept at least."""
    order = np.argsort(values)[::-1]
    kept = [samples[i] for i in order if values[i] >= threshold]
    return kept if kept else [samples[order[0]]]


def sort_by_s2n(samples: list[np.ndarray], threshold: float = 0.1) -> list[np.ndarray]:
    """Samples by descending signal-to-noise figure, scaled by the largest; those under ``threshold`` dropped (one is always kept)."""
    ndim = len(samples[0].shape)
    if ndim not in (1, 2):
        raise ValueError("Samples must be 1D or 2D arrays (raw audio or spectrograms).")
    measure = get_s2n_from_spectrogram if ndim == 2 else get_s2n_from_audio
    values = np.array([measure(s) for s in samples])
    values /= values.max() + 1e-10
    return _ranked(samples, values, threshold)


def subsample_indices(n: int, subsample: int = 512) -> np.ndarray:
    """Flat indices the median and MAD are taken over: all ``n`` when ``n <= subsample``, else ``np.linspace(0, n - 1, subsample, dtype=int)``."""
    if n <= subsample:
        return np.arange(n, dtype=np.int64)
    return np.linspace(0, n - 1, subsample, dtype=int)


def _median_f32(sorted_vals: np.ndarray) -> np.float32:
    m = sorted_vals.shape[0]
    lo, hi = sorted_vals[(m - 1) // 2], sorted_vals[m // 2]
    return lo if m % 2 else _F32(_F32(lo + hi) / _F32(2.0))


def activity_stats(x: np.ndarray, k: float = 2.0, subsample: int = 512) -> tuple[np.float32, np.float32, np.float32, int]:
    """``(median, mad, threshold, active_count)`` of ``get_activity_ratio``, every operation in float32, in this order:

    1. ``a = |x|`` flattened; ``v = sort(a[subsample_indices(a.size, subsample)])``, ``m`` values;
    2. ``median`` = the middle value for odd ``m``, else ``fl32(fl32(v[m/2 - 1] + v[m/2]) / 2)``;
    3. ``mad`` = the same median of ``fl32(|v - median|)``, then ``fl32(mad + fl32(1e-10))``;
    4. ``threshold = fl32(median + fl32(fl32(k) * mad))`` -- a multiplication and an addition, never a fused multiply-add;
    5. ``active_count`` = the number of elements of ``a`` strictly greater than ``threshold``.

    On float32 input this is what numpy (2.x promotion rules) evaluates for the reference's expression; ``bn_activity_counts``
    computes the same four numbers per row.  Input is converted to float32; it must be finite.
    """
    a = np.abs(np.asarray(x, dtype=_F32)).ravel()
    v = np.sort(a[subsample_indices(a.size, subsample)])
    med = _median_f32(v)
    with np.errstate(over="ignore"):
        mad = _F32(_median_f32(np.sort(np.abs(v - med))) + _MAD_EPS)
        thresh = _F32(med + _F32(_F32(k) * mad))
    return med, mad, thresh, int(np.count_nonzero(a > thresh))


def get_activity_ratio(x: np.ndarray, k: float = 2.0, max_active: float = 0.8, subsample: int = 512) -> float:
    """Share of elements of ``|x|`` above median + k * MAD (taken over ``subsample`` evenly spaced elements).

    A share above ``max_active`` is broadband noise, not a call, and counts as 0.0.

    Args:
        x: waveform or feature map.
        k: how many MADs above the median an element must lie.
        max_active: largest share still believed.
        subsample: elements the median and MAD are taken over.

    Returns:
        The share, in [0, max_active], as a Python float.
    """
    x = np.asarray(x)
    if x.dtype == _F32:
        active = activity_stats(x, k, subsample)[3]
    else:
        a = np.abs(x).ravel()
        v = a[subsample_indices(a.size, subsample)]
        med = np.median(v)
        mad = np.median(np.abs(v - med)) + 1e-10
        active = int(np.count_nonzero(a > med + k * mad))
    return ratio_from_count(active, x.size, max_active)


def ratio_from_count(active: int, total: int, max_active: float = 0.8) -> float:
    """The float64 ratio and the ``max_active`` rule, from an element count (the device path enters here with its counts)."""
    ratio = float(active) / float(total)
    return 0.0 if ratio > max_active else ratio


def rank_by_activity(ratios, threshold: float) -> list[int]:
    """Indices by descending ratio (``np.argsort(r)[::-1]``), those under ``threshold`` dropped, the first kept when none passes."""
    r = np.asarray(ratios, dtype=np.float64)
    order = np.argsort(r)[::-1]
    kept = [int(i) for i in order if r[i] >= threshold]
    return kept if kept else [int(order[0])]


def sort_by_activity(samples: list[np.ndarray], threshold: float = 0.25) -> list[np.ndarray]:
    """Samples by descending activity ratio; those under ``threshold`` dropped (one is always kept)."""
    return _ranked(samples, np.array([get_activity_ratio(s) for s in samples]), threshold)


def pick_random_samples(samples: list[np.ndarray], num_samples: int = 1, pick_first: bool = False) -> list[np.ndarray] | np.ndarray:
    """Draw ``num_samples`` of ``samples`` without replacement from numpy's global generator.

    With ``pick_first`` the first sample is always taken (alone when ``num_samples == 1``) and the rest are drawn from the
    others.  One sample comes back as an array, several as a list; an empty input gives ``[]``.
    """
    if len(samples) == 0:
        return []
    num_samples = min(num_samples, len(samples))
    if pick_first:
        if num_samples == 1:
            return samples[0]
        extra = np.random.choice(len(samples) - 1, size=num_samples - 1, replace=False) + 1
        return [samples[0]] + [samples[i] for i in extra]
    picked = np.random.choice(len(samples), size=num_samples, replace=False)
    return [samples[i] for i in picked] if num_samples > 1 else samples[picked[0]]
