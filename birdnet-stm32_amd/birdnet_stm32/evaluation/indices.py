"""Acoustic indices of whole recordings: how complex, how even, how biological, how busy is each chunk — no model involved.

The specification of ``csrc/bn_indices.hip`` (C ABI ``bn_acoustic_indices``) and of the ``indices`` command.  Files take the path every other
command takes (``audio/pipeline.py``: read, resample, peak-normalise and chunk on the device), ``bn_stft_mag(normalize = 0)`` leaves each
chunk's raw magnitudes ``S [257, W]`` and their maximum in device memory, and one launch reduces every chunk to the numbers below.

Notation.  ``P = S * S``; ``f_k = k * sample_rate / 512``; ``r_f = sum_t S[f, t]``; ``p_f = sum_t P[f, t]``; ``e_t = sum_f P[f, t]``;
``smax = max S``.  A band ``[lo, hi)`` in Hz is the set of bins with ``lo <= f_k < hi`` (``band_bins``: decided once on the host in float64;
the kernel sees bin ranges).  ``H(v) = -sum q ln q / ln(len v)`` with ``q = v / sum v``, terms with ``q = 0`` giving 0, and 0 when ``sum v = 0``.

Per chunk, in this order (``INDEX_COLUMNS``):

1. ``aci``   Acoustic complexity (Pieretti 2011): ``sum_f ACI_f``, ``ACI_f = sum_{t >= 1} |S[f, t] - S[f, t-1]| / r_f`` (0 where ``r_f = 0``).
2. ``hf``    Spectral entropy ``H(p)`` over the 257 bins.
3. ``ht``    Temporal entropy ``H(e)`` over the ``W`` frames.  The envelope is the frame energy, as Towsey uses it, not a Hilbert envelope
             of the waveform (soundecology, scikit-maad).
4. ``h``     ``hf * ht`` (Sueur 2008).
5. ``ndsi``  Normalised difference soundscape index (Kasten 2012): ``(B - A) / (B + A)``, ``A`` / ``B`` the sums of ``p_f`` over the
             anthrophony band (default 1000-2000 Hz) and the biophony band (default 2000-8000 Hz); 0 when ``A + B = 0``.
6. ``bi``    Bioacoustic index (Boelman 2007): ``sum over the biophony band of (L_f - min L_f) * df_kHz`` with
             ``L_f = 10 log10(max(p_f / W, 1e-12 smax^2))``, the minimum over the same band, ``df_kHz = sample_rate / 512 / 1000``.
7. ``adi``   Acoustic diversity (Villanueva-Rivera 2011): bands ``band_hz`` wide (default 1000) from 0 up to ``min(max_hz = 10000,
             sample_rate / 2)``, whole bands only, at most 16; ``c_b`` the share of a band's cells with ``S > thr``,
             ``thr = fl32(smax * fl32(10^(db / 20)))`` with ``db = -50``, both sides of the comparison float32;
             ``adi = -sum q ln q`` with ``q = c / sum c``, not normalised; 0 when ``sum c = 0``.
8. ``aei``   Acoustic evenness: the Gini coefficient of the ``c_b``, ``2 sum_i i x_(i) / (n sum x) - (n + 1) / n`` over the ascending ``x``
             (``i`` from 1); 0 when ``sum c = 0``.

Per chunk and bin (``SPECTRAL_COLUMNS``, each ``[257]``) — the channels of Towsey's false-colour long-duration spectrograms:

* ``aci``  ``ACI_f``;
* ``ent``  ``1 - H(P[f, :])``, 0 where ``p_f = 0``;
* ``cvr``  ``fl32(count_t(S[f, t] > thr)) / fl32(W)``.

An all-zero chunk gives zeros everywhere.  Every index is unchanged when ``S`` is multiplied by a constant, on purpose: the ingest
peak-normalises each file, so level-dependent indices (background noise in dB and the like) would mean nothing here and are out of scope.
The threshold of the cover counts is relative to the chunk's own maximum for the same reason (soundecology measures it against the file's).

``indices_reference`` is this text in float64 numpy, ``indices_reference_f32`` the same formulas over float32 arrays with numpy's own sums:
the yardstick of the device tolerance (``DESIGN.md`` §5r), nothing else.  ``aggregate`` turns per-chunk rows into rows per window of
``window_s`` seconds: the MEAN of the chunks whose start falls into the window — per-chunk indices averaged, not indices of the whole minute.
"""

from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np

INDEX_COLUMNS = ("aci", "hf", "ht", "h", "ndsi", "bi", "adi", "aei")
SPECTRAL_COLUMNS = ("aci", "ent", "cvr")
N_FFT, N_BINS = 512, 257
N_SCALARS = len(INDEX_COLUMNS)            # BN_INDICES_SCALARS
MAX_BANDS = 16                            # BN_INDICES_MAX_BANDS
MIN_WIDTH, MAX_WIDTH = 2, 1024            # BN_INDICES_MIN_W, BN_INDICES_MAX_W
BI_FLOOR = 1e-12                          # L_f is clamped at this share of smax^2


@dataclass(frozen=True)
class IndexParams:
    """The bands and thresholds of the indices; ``validate(sample_rate)`` refuses what does not fit below ``sample_rate / 2``."""

    anthro: tuple = (1000.0, 2000.0)
    bio: tuple = (2000.0, 8000.0)
    db: float = -50.0
    band_hz: float = 1000.0
    max_hz: float = 10000.0

    def validate(self, sample_rate: int) -> "IndexParams":
        sr = int(sample_rate)
        if sr <= 0:
            raise ValueError(f"sample_rate {sample_rate} must be positive")
        nyq = sr / 2.0
        for name, band in (("anthro", self.anthro), ("bio", self.bio)):
            if len(band) != 2 or not all(math.isfinite(float(v)) for v in band):
                raise ValueError(f"{name} band {band!r}: two frequencies in Hz")
            lo, hi = float(band[0]), float(band[1])
            if not 0.0 <= lo < hi:
                raise ValueError(f"{name} band {lo:g}-{hi:g} Hz: 0 <= low < high")
            if hi > nyq:
                raise ValueError(f"{name} band {lo:g}-{hi:g} Hz does not fit below {nyq:g} Hz, half the sample rate {sr}")
            k0, k1 = band_bins(lo, hi, sr)
            if k1 <= k0:
                raise ValueError(f"{name} band {lo:g}-{hi:g} Hz holds no bin (bins are {sr / N_FFT:g} Hz apart)")
        if not (math.isfinite(float(self.db)) and float(self.db) <= 0.0):
            raise ValueError(f"db threshold {self.db} must be finite and <= 0 (dB below the chunk's maximum)")
        if not (math.isfinite(float(self.band_hz)) and float(self.band_hz) > 0.0):
            raise ValueError(f"band_hz {self.band_hz} must be positive")
        if not (math.isfinite(float(self.max_hz)) and float(self.max_hz) > 0.0):
            raise ValueError(f"max_hz {self.max_hz} must be positive")
        n = int(math.floor(min(float(self.max_hz), nyq) / float(self.band_hz)))
        if n < 1:
            raise ValueError(f"no whole band of {self.band_hz:g} Hz fits below {min(float(self.max_hz), nyq):g} Hz")
        if n > MAX_BANDS:
            raise ValueError(f"{n} bands of {self.band_hz:g} Hz up to {min(float(self.max_hz), nyq):g} Hz: at most {MAX_BANDS}")
        edges = diversity_edges(self, sr)
        if np.any(np.diff(edges) <= 0):
            raise ValueError(f"band_hz {self.band_hz:g}: a band holds no bin (bins are {sr / N_FFT:g} Hz apart)")
        return self


def bin_frequencies(sample_rate: int) -> np.ndarray:
    """``f_k`` of the 257 bins, float64."""
    return np.arange(N_BINS, dtype=np.float64) * float(sample_rate) / float(N_FFT)


def band_bins(lo: float, hi: float, sample_rate: int) -> tuple[int, int]:
    """The bin range ``[k0, k1)`` of the band ``[lo, hi)`` Hz: the bins with ``lo <= f_k < hi``."""
    f = bin_frequencies(sample_rate)
    return int(np.searchsorted(f, float(lo), side="left")), int(np.searchsorted(f, float(hi), side="left"))


def diversity_edges(params: IndexParams, sample_rate: int) -> np.ndarray:
    """Bin edges ``[n_bands + 1]`` of the ADI / AEI bands: band ``b`` is ``[b * band_hz, (b + 1) * band_hz)``."""
    top = min(float(params.max_hz), float(sample_rate) / 2.0)
    n = min(MAX_BANDS, int(math.floor(top / float(params.band_hz))))
    f = bin_frequencies(sample_rate)
    return np.array([np.searchsorted(f, b * float(params.band_hz), side="left") for b in range(n + 1)], np.int64)


def cover_ratio(params: IndexParams) -> np.float32:
    """``fl32(10^(db / 20))``: the cover threshold as a share of the chunk's maximum."""
    return np.float32(10.0 ** (float(params.db) / 20.0))


class DeviceParams(ctypes.Structure):
    """``bn_indices_params`` (include/birdnet_hip.h)."""

    _fields_ = [("anthro_k0", ctypes.c_int32), ("anthro_k1", ctypes.c_int32), ("bio_k0", ctypes.c_int32), ("bio_k1", ctypes.c_int32),
                ("n_bands", ctypes.c_int32), ("band_edge", ctypes.c_int32 * (MAX_BANDS + 1)), ("cover_ratio", ctypes.c_float),
                ("df_khz", ctypes.c_float)]


def device_params(params: IndexParams, sample_rate: int) -> DeviceParams:
    """What the kernel sees of ``params``: bin ranges, the float32 cover ratio and the bin spacing in kHz."""
    params.validate(sample_rate)
    edges = diversity_edges(params, sample_rate)
    dp = DeviceParams()
    dp.anthro_k0, dp.anthro_k1 = band_bins(*params.anthro, sample_rate)
    dp.bio_k0, dp.bio_k1 = band_bins(*params.bio, sample_rate)
    dp.n_bands = len(edges) - 1
    for i in range(MAX_BANDS + 1):
        dp.band_edge[i] = int(edges[min(i, len(edges) - 1)])
    dp.cover_ratio = float(cover_ratio(params))
    dp.df_khz = float(sample_rate) / N_FFT / 1000.0
    return dp


# -- the specification ------------------------------------------------------------------------------------------------------------------
def cover_threshold(S: np.ndarray, params: IndexParams) -> np.float32:
    """``thr = fl32(smax * fl32(10^(db / 20)))``."""
    S = np.asarray(S, np.float32)
    smax = np.float32(S.max()) if S.size else np.float32(0)
    return np.float32(smax * cover_ratio(params))


def cover_counts(S: np.ndarray, sample_rate: int, params: IndexParams) -> tuple[np.ndarray, np.ndarray]:
    """``(cells above thr per bin [257], per ADI band [n_bands])`` as integers: a float32 comparison on both sides."""
    S = np.asarray(S, np.float32)
    per_bin = (S > cover_threshold(S, params)).sum(axis=1).astype(np.int64)
    edges = diversity_edges(params, sample_rate)
    return per_bin, np.array([per_bin[edges[b]:edges[b + 1]].sum() for b in range(len(edges) - 1)], np.int64)


def _entropy(v: np.ndarray, dt) -> float:
    """``H(v)`` in the arithmetic of ``dt``."""
    s = v.sum(dtype=dt)
    if not s > 0 or v.shape[0] < 2:
        return dt(0)
    q = (v / s).astype(dt)
    q = q[q > 0]
    return dt(-(q * np.log(q)).sum(dtype=dt) / np.log(dt(v.shape[0])))


def _indices(S: np.ndarray, sample_rate: int, params: IndexParams, dt):
    S32 = np.asarray(S, np.float32)
    if S32.ndim != 2 or S32.shape[0] != N_BINS or not MIN_WIDTH <= S32.shape[1] <= MAX_WIDTH:
        raise ValueError(f"S must be [{N_BINS}, {MIN_WIDTH}..{MAX_WIDTH}] magnitudes, got {S32.shape}")
    params.validate(sample_rate)
    W = S32.shape[1]
    X = S32.astype(dt)
    P = X * X
    r, p, e = X.sum(axis=1, dtype=dt), P.sum(axis=1, dtype=dt), P.sum(axis=0, dtype=dt)
    smax = dt(S32.max())
    d = np.abs(np.diff(X, axis=1)).sum(axis=1, dtype=dt)
    aci_f = np.where(r > 0, d / np.where(r > 0, r, dt(1)), dt(0)).astype(dt)
    ent_f = np.array([dt(1) - _entropy(P[f], dt) if p[f] > 0 else dt(0) for f in range(N_BINS)], dt)
    per_bin, per_band = cover_counts(S32, sample_rate, params)
    cvr_f = (per_bin.astype(np.float32) / np.float32(W)).astype(dt)

    hf, ht = _entropy(p, dt), _entropy(e, dt)
    a0, a1 = band_bins(*params.anthro, sample_rate)
    b0, b1 = band_bins(*params.bio, sample_rate)
    A, B = p[a0:a1].sum(dtype=dt), p[b0:b1].sum(dtype=dt)
    ndsi = dt((B - A) / (A + B)) if A + B > 0 else dt(0)
    bi = dt(0)
    if smax > 0:
        L = dt(10) * np.log10(np.maximum(p[b0:b1] / dt(W), dt(BI_FLOOR) * smax * smax)).astype(dt)
        bi = dt((L - L.min()).sum(dtype=dt) * dt(float(sample_rate) / N_FFT / 1000.0))
    edges = diversity_edges(params, sample_rate)
    cells = (np.diff(edges) * W).astype(dt)
    c = (per_band.astype(dt) / cells).astype(dt)
    adi = aei = dt(0)
    total = c.sum(dtype=dt)
    if total > 0:
        q = (c / total).astype(dt)
        q = q[q > 0]
        adi = dt(-(q * np.log(q)).sum(dtype=dt))
        x, n = np.sort(c), c.shape[0]
        aei = dt(dt(2) * (np.arange(1, n + 1).astype(dt) * x).sum(dtype=dt) / (dt(n) * total) - dt(n + 1) / dt(n))
    scalars = np.array([aci_f.sum(dtype=dt), hf, ht, dt(hf * ht), ndsi, bi, adi, aei], dt)
    return scalars, np.stack([aci_f, ent_f, cvr_f]).astype(dt)


def indices_reference(S: np.ndarray, sample_rate: int, params: IndexParams | None = None) -> tuple[np.ndarray, np.ndarray]:
    """``(scalars [8], per-bin [3, 257])`` of one chunk's float32 magnitudes ``S [257, W]``, in float64: the specification."""
    return _indices(S, sample_rate, params or IndexParams(), np.float64)


def indices_reference_f32(S: np.ndarray, sample_rate: int, params: IndexParams | None = None) -> tuple[np.ndarray, np.ndarray]:
    """The same formulas over float32 arrays with numpy's own sums: the yardstick of the device tolerance.  Where every sum is exact
    (integer-valued magnitudes below 16) its ``ACI_f``, ``CVR_f`` and NDSI are the values a correct float32 kernel must give bit for bit."""
    return _indices(S, sample_rate, params or IndexParams(), np.float32)


# -- windows -----------------------------------------------------------------------------------------------------------------------------
@dataclass
class IndexTable:
    """Rows per window: ``values [n, C]`` float64 are the means of ``chunks`` per-chunk rows of file ``file_index`` whose start lies in
    ``[start_s, start_s + window_s)``; ``end_s`` is where the last of them ends."""

    file_index: np.ndarray
    start_s: np.ndarray
    end_s: np.ndarray
    chunks: np.ndarray
    values: np.ndarray

    def __len__(self) -> int:
        return int(self.file_index.shape[0])


def aggregate(rows, chunk_file, chunk_start_s, window_s: float = 60.0, chunk_end_s=None) -> IndexTable:
    """The mean of the per-chunk ``rows [N, C]`` over the chunks of each file whose START falls into each window of ``window_s`` seconds
    (a file's last chunk starts at ``n - size``, as ``analyze`` cuts it: its start decides its window).  Windows without a chunk give no
    row; rows are ordered by file, then time.  ``window_s = 0``: one row per chunk.  ``chunk_end_s`` (default: the chunk's start) gives
    ``end_s``, the end of the window's last chunk.  These are per-chunk indices averaged, not indices of the whole window."""
    rows = np.asarray(rows)
    if rows.ndim != 2:
        raise ValueError("rows must be [N, C]")
    file = np.asarray(chunk_file, np.int64)
    start = np.asarray(chunk_start_s, np.float64)
    end = start if chunk_end_s is None else np.asarray(chunk_end_s, np.float64)
    N = rows.shape[0]
    if file.shape != (N,) or start.shape != (N,) or end.shape != (N,):
        raise ValueError(f"{N} rows need {N} chunk files and start times")
    window_s = float(window_s)
    if not (math.isfinite(window_s) and window_s >= 0.0):
        raise ValueError(f"window_s {window_s} must be >= 0")
    if window_s == 0.0 or N == 0:
        return IndexTable(file.copy(), start.copy(), end.copy(), np.ones(N, np.int64), rows.astype(np.float64))
    win = np.floor(start / window_s).astype(np.int64)
    order = np.lexsort((np.arange(N), win, file))
    f, w = file[order], win[order]
    first = np.flatnonzero(np.concatenate([[True], (f[1:] != f[:-1]) | (w[1:] != w[:-1])]))
    counts = np.diff(np.append(first, N))
    sums = np.add.reduceat(rows[order].astype(np.float64), first, axis=0)
    return IndexTable(f[first], w[first].astype(np.float64) * window_s, np.maximum.reduceat(end[order], first), counts.astype(np.int64),
                      sums / counts[:, None])


# -- the device path ---------------------------------------------------------------------------------------------------------------------
def acoustic_indices_device(ctx, spec, minmax, sample_rate: int, params: IndexParams | None = None, spectral: bool = True, out=None,
                            spectral_out=None):
    """``bn_acoustic_indices`` on CUDA tensors: raw magnitudes ``spec [B, 257, W]`` and ``minmax [B, 2]`` as ``stft_device(...,
    normalize=False, return_minmax=True)`` leaves them -> ``(scalars [B, 8], per-bin [B, 3, 257] or None)`` float32.  ``out`` /
    ``spectral_out``: contiguous tensors to fill instead of new ones."""
    import torch

    from birdnet_stm32 import _hip

    dp = device_params(params or IndexParams(), sample_rate)
    if not (spec.is_cuda and spec.dtype == torch.float32 and spec.dim() == 3 and spec.is_contiguous()):
        raise ValueError("spec must be a contiguous float32 CUDA tensor [B, 257, W]")
    B, F, W = spec.shape
    if not (minmax.is_cuda and minmax.dtype == torch.float32 and tuple(minmax.shape) == (B, 2) and minmax.is_contiguous()):
        raise ValueError(f"minmax must be a contiguous float32 CUDA tensor [{B}, 2]")
    if out is None:
        out = torch.empty((B, N_SCALARS), dtype=torch.float32, device=spec.device)
    if spectral and spectral_out is None:
        spectral_out = torch.empty((B, len(SPECTRAL_COLUMNS), N_BINS), dtype=torch.float32, device=spec.device)
    for name, t, shape in (("out", out, (B, N_SCALARS)), ("spectral_out", spectral_out if spectral else None, (B, len(SPECTRAL_COLUMNS), N_BINS))):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 CUDA tensor {list(shape)}")
    with torch.cuda.device(spec.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(spec.device).cuda_stream)
        _hip.check(ctx.lib.bn_acoustic_indices(ctx.handle, spec.data_ptr(), minmax.data_ptr(), B, F, W, ctypes.byref(dp), out.data_ptr(),
                                               spectral_out.data_ptr() if spectral else None, stream))
    return out, (spectral_out if spectral else None)


class IndicesRunner:
    """What ``EvaluatePipeline`` needs of a runner, without a model: a context, a device, a slice size, the width of an output row, and
    ``infer_audio_device`` — here ``stft_device(normalize=False)`` and ``bn_acoustic_indices``, slice by slice of ``max_batch`` chunks.
    A row is the 8 scalars, followed with ``spectral`` by the ``3 * 257`` per-bin values."""

    def __init__(self, sample_rate: int = 22050, spec_width: int = 256, params: IndexParams | None = None, spectral: bool = True,
                 device: int = 0, max_batch: int = 4096, ctx=None):
        import torch

        from birdnet_stm32 import _hip

        if not torch.cuda.is_available():
            raise RuntimeError("the indices are computed on the GPU and no device is available; there is no CPU path")
        if not MIN_WIDTH <= int(spec_width) <= MAX_WIDTH:
            raise ValueError(f"spec_width {spec_width} must be {MIN_WIDTH}..{MAX_WIDTH}")
        if int(max_batch) < 1:
            raise ValueError(f"max_batch {max_batch} must be >= 1")
        self.params = (params or IndexParams()).validate(sample_rate)
        self.sample_rate, self.spec_width, self.spectral = int(sample_rate), int(spec_width), bool(spectral)
        self.device = torch.device("cuda", int(device))
        self.max_batch = int(max_batch)
        self.ctx = ctx if ctx is not None else _shared_context(int(device), self.max_batch)
        self.num_classes = N_SCALARS + (len(SPECTRAL_COLUMNS) * N_BINS if self.spectral else 0)
        self._scalars = self._bins = None

    def infer_audio_device(self, audio, out=None):
        import torch

        from birdnet_stm32.models.runners import stft_device

        n = int(audio.shape[0])
        if out is None:
            out = torch.empty((n, self.num_classes), dtype=torch.float32, device=audio.device)
        if self._scalars is None:
            self._scalars = torch.empty((self.max_batch, N_SCALARS), dtype=torch.float32, device=audio.device)
            self._bins = torch.empty((self.max_batch, len(SPECTRAL_COLUMNS), N_BINS), dtype=torch.float32, device=audio.device) if self.spectral else None
        for b0 in range(0, n, self.max_batch):
            nb = min(self.max_batch, n - b0)
            spec, minmax = stft_device(self.ctx, audio[b0 : b0 + nb], N_FFT, None, self.spec_width, False, return_minmax=True)
            acoustic_indices_device(self.ctx, spec, minmax, self.sample_rate, self.params, self.spectral, self._scalars[:nb],
                                    self._bins[:nb] if self.spectral else None)
            out[b0 : b0 + nb, :N_SCALARS].copy_(self._scalars[:nb])
            if self.spectral:
                out[b0 : b0 + nb, N_SCALARS:].copy_(self._bins[:nb].reshape(nb, -1))
        return out


_CONTEXTS: dict = {}


def _shared_context(device: int, max_batch: int):
    """One context per device for the runners of this module, kept for the life of the process: the pipeline's helper threads may still
    page-lock slabs through it after a call has returned."""
    from birdnet_stm32 import _hip

    if device not in _CONTEXTS:
        _CONTEXTS[device] = _hip.Context(device, max_batch)
    return _CONTEXTS[device]


@dataclass
class FileIndices:
    """Result of :func:`indices_files`, per chunk in file then chunk order: ``scalars [N, 8]`` float32, ``spectral [N, 3, 257]`` float32 or
    None, the owning file, start and end in seconds; per input file ``chunks_per_file`` and ``duration_s`` (0 for a skipped file)."""

    scalars: np.ndarray
    spectral: np.ndarray | None
    chunk_file: np.ndarray
    chunk_start_s: np.ndarray
    chunk_end_s: np.ndarray
    paths: list
    chunks_per_file: np.ndarray
    duration_s: np.ndarray
    skipped: list
    sample_rate: int

    def __len__(self) -> int:
        return int(self.scalars.shape[0])


def indices_files(paths, sample_rate: int = 22050, chunk_duration: float = 3.0, spec_width: int = 256, overlap: float = 0.0, max_duration=0,
                  spectral: bool = True, params: IndexParams | None = None, device: int = 0, max_batch: int = 4096, ctx=None,
                  pipeline_options: dict | None = None, budget_bytes: int = 256 << 20) -> FileIndices:
    """The indices of every chunk of every file of ``paths``, through ``EvaluatePipeline(stream_long=True)`` as ``analyze`` runs it: files are
    read, resampled to ``sample_rate``, peak-normalised and cut into chunks of ``chunk_duration`` seconds on the device, and rows come to
    the host in blocks of files that fit ``budget_bytes``.  ``max_duration = 0`` reads whole files."""
    from birdnet_stm32.audio.pipeline import EvaluatePipeline, plan_files
    from birdnet_stm32.evaluation.detections import chunk_table
    from birdnet_stm32.evaluation.embeddings import _to_host, embedding_blocks

    sr, cd, ov = int(sample_rate), float(chunk_duration), float(overlap)
    if int(sr * cd) // int(spec_width) < 1:
        raise ValueError(f"chunks of {int(sr * cd)} samples are too short for {spec_width} frames")
    runner = IndicesRunner(sr, spec_width, params, spectral, device, max_batch, ctx)
    C = runner.num_classes
    paths = list(paths)
    opts = dict(pipeline_options or {})
    opts.setdefault("stream_long", True)
    pipe = None
    try:
        pipe = EvaluatePipeline(runner, sr, cd, ov, max_duration=max_duration, **opts)
        tab = plan_files(paths, sr, cd, ov, max_duration, pipe.readers)
        counts = tab.n_chunks.astype(np.int64)
        parts = []
        for lo, hi in embedding_blocks(counts, C * 4, budget_bytes):
            if int(counts[lo:hi].sum()) == 0:
                continue
            rows, got, _stats, _lat = pipe.run(paths[lo:hi], table=tab.sub(lo, hi))
            if list(got) != counts[lo:hi].tolist():
                raise RuntimeError("the pipeline cut a different number of chunks than it planned")
            parts.append(_to_host(rows.contiguous()))
    finally:
        if pipe is not None:
            pipe.close()
    rows = np.concatenate(parts) if parts else np.zeros((0, C), np.float32)
    chunks = chunk_table(tab.n_out, sr, cd, ov)
    if rows.shape[0] != chunks.file.shape[0]:
        raise RuntimeError(f"{rows.shape[0]} rows for {chunks.file.shape[0]} chunks")
    bins = rows[:, N_SCALARS:].reshape(-1, len(SPECTRAL_COLUMNS), N_BINS) if spectral else None
    per_file = np.bincount(chunks.file, minlength=len(paths)).astype(np.int64) if paths else np.zeros(0, np.int64)
    return FileIndices(np.ascontiguousarray(rows[:, :N_SCALARS]), bins, chunks.file, chunks.start_s, chunks.end_s, paths, per_file,
                       np.asarray(tab.n_out, np.float64) / sr, [p for p, k in zip(paths, tab.kind) if k < 0], sr)
