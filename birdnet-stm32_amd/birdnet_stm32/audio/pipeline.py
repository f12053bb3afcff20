"""Files -> chunk scores as a three-stage pipeline: reader pool -> pinned slab -> H2D on a copy stream -> ingest + inference.

What the reference does for every test file, one after another on one thread (reference: birdnet_stm32/evaluation/metrics.py:117-141:
``load_audio_file`` -> spectrograms -> ``predict`` in batches of ``batch_size``; audio/io.py:63-130,177-213), runs here as three
stages that overlap:

1. **read** (host threads, ``csrc/host/bn_pcmio.c``): the RIFF headers of all files are walked once (``bn_wav_probe_many``); per
   *group* of files the read windows — the first ``max_duration`` seconds, as they lie in the file — are ``pread`` straight into a
   ring of page-locked slabs (``bn_file_read_many``; no intermediate ``bytes`` objects, no ``np.concatenate``).  Windows that share
   (sample format, channels, native rate) lie back to back, which is the layout ``bn_ingest_resample`` takes.  Every offset table of
   the group (window offsets, resampled offsets, chunk starts / valid lengths / owners) is written into ONE pinned table.
2. **H2D** (copy stream): one ``non_blocking`` copy of the slab and one of the table per group into a ring of two device slabs, so
   the copy of group g+1 runs under the kernels of group g.
3. **compute** (the caller's stream): ``bn_ingest_resample`` per sub-group, one ``bn_ingest_chunks``, ``bn_infer_audio`` in slices
   of the runner's ``max_batch`` into a preallocated score tensor.

Nothing synchronises the host inside the loop except the ring hand-overs (events).  The chunk scores of all files stay on the GPU;
the caller pools them (``bn_pool_scores``) once at the end.

**Long files** (``stream_long=True``, opt-in): a file whose read window does not fit one slab, or is longer than one
``bn_ingest_resample`` launch can index, is cut into *segments* (``plan_segments``): an output range of its window plus the input
frames those outputs touch.  Segments take the same ring as groups (pinned slab -> copy stream -> device slab); each one is one
``bn_ingest_resample_span`` launch into a device buffer that holds the file's resampled samples.  Behind its last segment the file's
chunks are cut and scored in slices of ``group_chunks``.  Device memory: one file's mono samples plus one slice of chunks.

**Selection** (``select=ChunkSelection(...)``, opt-in): instead of every grid chunk, each file contributes its few most active chunks, chosen
as the reference's training loader chooses them (data/generator.py ``_process_file``; ``audio/activity.py``).  Per group, behind the resampler:
files with more grid chunks than ``candidate_chunks`` get their short-time energy from ``bn_short_time_energy`` (one launch per group), the host
turns the energies into smart-crop starts, one ``bn_ingest_chunks`` cuts the candidates, ``bn_stft_mag(normalize=1)`` + ``bn_activity_counts``
give every candidate's active-element count, the host ranks and thresholds per file, a second ``bn_ingest_chunks`` cuts the selected rows and only
those are scored.  Two host round trips per group; reader and copy threads keep running beside them.  Needs ``chunk_overlap = 0``.

There is no CPU fallback: the module needs ``libbirdnet_hip.so`` and a GPU.  Files that are not plain PCM / float32 WAV (FLAC,
8-bit, float64, containers only ``soundfile`` reads) are decoded on the host by ``audio.ingest.read_pcm_window`` inside the read
stage and copied into the slab; their arithmetic still happens on the device.
"""

from __future__ import annotations

import ctypes
import queue
import os
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from math import gcd

import numpy as np

from birdnet_stm32 import _hip
from birdnet_stm32.audio import _pcmio
from birdnet_stm32.audio import io as _io
from birdnet_stm32.audio.ingest import PCM_F32, PCM_S16, PCM_S24, PCM_S32, _BYTES, polyphase_filter, read_pcm_window

_RAW_FORMATS = {(1, 16): PCM_S16, (1, 24): PCM_S24, (1, 32): PCM_S32, (3, 32): PCM_F32}
_ALIGN = 256
MAX_WINDOWS_PER_GROUP = 65535  # bn_ingest_resample's limit per launch
SPAN_MAX_OUT = 1 << 26         # outputs per bn_ingest_resample_span launch of a streamed file (its block-peak scratch stays <= 256 KiB)
MONO_BUDGET_BYTES = 16 << 30   # device bytes of one streamed file's resampled samples (~50 h at 22.05 kHz)
_READ_PIECE = 8 << 20          # a segment is read (or copied) as pieces of this many bytes, in parallel


def filter_geometry(sr0: int, sample_rate: int) -> tuple[int, int, int, int]:
    """``(up, down, taps per phase, leading outputs dropped)`` of ``resample_poly`` from ``sr0`` to ``sample_rate`` (1, 1, 0, 0: same rate)."""
    if sr0 == sample_rate:
        return 1, 1, 0, 0
    g = gcd(int(sr0), int(sample_rate))
    up, down = int(sample_rate) // g, int(sr0) // g
    _taps, per_phase, pre = polyphase_filter(up, down)
    return up, down, int(per_phase), int(pre)


def span_inputs(o0: int, o1: int, n_in: int, up: int, down: int, hpp: int, pre: int) -> tuple[int, int]:
    """Input frames ``[s0, s1)`` that outputs ``[o0, o1)`` of a window of ``n_in`` frames touch, clipped to the window.  Output n reads
    the ``hpp`` frames ending at ``floor((n + pre) * down / up)`` (the same rate: frame n).  Python integers: exact at any length."""
    if hpp == 0:
        lo, hi = o0, o1
    else:
        lo = (o0 + pre) * down // up - (hpp - 1)
        hi = (o1 - 1 + pre) * down // up + 1
    lo, hi = max(lo, 0), min(hi, n_in)
    return (lo, hi) if lo < hi else (lo, lo) if lo < n_in else (n_in, n_in)


def plan_segments(n_in: int, n_out: int, up: int, down: int, hpp: int, pre: int, frame_bytes: int, budget_bytes: int,
                  max_out: int = SPAN_MAX_OUT) -> list[tuple[int, int, int, int]]:
    """Cut the outputs ``[0, n_out)`` of one window into segments ``(o0, o1, s0, s1)``: consecutive output ranges, each as long as its
    staged input frames ``[s0, s1)`` (``span_inputs``, the filter's halo of ``hpp - 1`` frames included) fit ``budget_bytes`` and at most
    ``max_out`` outputs.  The segments tile ``[0, n_out)`` without gaps or overlap."""
    n_in, n_out, up, down, hpp, pre = int(n_in), int(n_out), int(up), int(down), int(hpp), int(pre)
    frames_budget = int(budget_bytes) // int(frame_bytes)
    segs, o0 = [], 0
    while o0 < n_out:
        lo = span_inputs(o0, o0 + 1, n_in, up, down, hpp, pre)[0]
        if n_in - lo <= frames_budget:
            o1 = n_out
        else:
            last = lo + frames_budget - 1   # newest frame the budget can stage
            o1 = last + 1 if hpp == 0 else (last * up + up - 1) // down - pre + 1
        o1 = min(o1, n_out, o0 + int(max_out))
        if o1 <= o0:
            raise ValueError(f"a staging budget of {budget_bytes} bytes cannot hold the {hpp} input frames of one output")
        s0, s1 = span_inputs(o0, o1, n_in, up, down, hpp, pre)
        segs.append((o0, o1, s0, s1))
        o0 = o1
    return segs


def long_files(tab: "FileTable", sample_rate: int, slab_bytes: int) -> np.ndarray:
    """Files the pipeline streams in ``stream_long`` mode: the read window exceeds one slab, or its positions exceed what one
    ``bn_ingest_resample`` launch indexes (``(n_out + pre + 4096) * down`` or ``frames * up`` reach 2^32)."""
    out = np.zeros(len(tab.paths), bool)
    for i in np.flatnonzero(tab.kind >= 0):
        up, down, _hpp, pre = filter_geometry(int(tab.sr0[i]), sample_rate)
        too_far = (int(tab.n_out[i]) + pre + 4096) * down >= 1 << 32 or int(tab.frames[i]) * up >= 1 << 32
        out[i] = int(tab.nbytes[i]) > slab_bytes or too_far
    return out


def window_counts(total_frames: np.ndarray, sr0: np.ndarray, max_duration) -> np.ndarray:
    """Frames of the read window of ``load_audio_window`` (reference io.py:95-111 with ``random_offset=False``), vectorised; the
    same float64 operations as ``audio.ingest._window_frames`` so the counts agree exactly."""
    total = np.asarray(total_frames, np.int64)
    sr = np.asarray(sr0, np.int64)
    ok = (total > 0) & (sr > 0)
    safe_sr = np.where(ok, sr, 1).astype(np.float64)
    duration = total.astype(np.float64) / safe_sr
    want = np.minimum(float(max_duration), duration) if max_duration and max_duration > 0 else duration
    count = np.minimum(total.astype(np.float64), want * safe_sr).astype(np.int64)
    return np.where(ok, count, 0)


def resampled_lengths(frames: np.ndarray, sr0: np.ndarray, sample_rate: int) -> np.ndarray:
    """``len(resample_poly(x, up, down))`` = ceil(n * up / down) per window (identity at the target rate)."""
    frames = np.asarray(frames, np.int64)
    sr0 = np.asarray(sr0, np.int64)
    g = np.gcd(np.where(sr0 > 0, sr0, 1), int(sample_rate))
    up, down = int(sample_rate) // g, np.where(sr0 > 0, sr0, 1) // g
    n = frames * up
    return np.where(sr0 == sample_rate, frames, n // down + (n % down != 0))


def chunk_counts(n_out: np.ndarray, sample_rate: int, chunk_duration: float, chunk_overlap: float) -> np.ndarray:
    """``estimate_num_chunks`` (reference io.py:33-60) for an array of waveform lengths."""
    size = int(sample_rate * chunk_duration)
    step = _io._step(sample_rate, chunk_duration, chunk_overlap)
    n = np.asarray(n_out, np.int64)
    rest = np.maximum(n - size, 0)
    many = 1 + rest // step + (rest % step != 0)
    return np.where((n <= 0) | (size <= 0), 0, np.where(n <= size, 1, many)).astype(np.int64)


def chunk_table_arrays(n_out: np.ndarray, sample_rate: int, chunk_duration: float, chunk_overlap: float):
    """Vectorised ``audio.ingest.chunk_table``: ``(start within its window, valid samples, window index, chunks per window, size)``."""
    size = int(sample_rate * chunk_duration)
    step = _io._step(sample_rate, chunk_duration, chunk_overlap)
    n = np.asarray(n_out, np.int64)
    counts = chunk_counts(n, sample_rate, chunk_duration, chunk_overlap)
    total = int(counts.sum())
    owner = np.repeat(np.arange(n.shape[0], dtype=np.int64), counts)
    first = np.cumsum(counts) - counts
    j = np.arange(total, dtype=np.int64) - first[owner]
    n_own = n[owner]
    start = j * step
    tail = (j == counts[owner] - 1) & (n_own > size) & ((n_own - size) % step != 0)  # the uncovered end: one more chunk at len - size
    start = np.where(tail, n_own - size, start)
    valid = np.where(n_own <= size, n_own, size).astype(np.int32)
    return start, valid, owner.astype(np.int32), counts, size


@dataclass
class FileTable:
    """Per-file facts the pipeline plans with (arrays over the rank's file list)."""

    paths: list[str]
    kind: np.ndarray        # 0: plain WAV payload read by the C pool; 1: decoded on the host in the read stage; -1: unreadable / empty
    fmt: np.ndarray
    channels: np.ndarray
    sr0: np.ndarray
    frames: np.ndarray      # frames of the read window
    file_off: np.ndarray    # byte offset of the window in the file (kind 0)
    nbytes: np.ndarray      # bytes of the window in the slab
    n_out: np.ndarray       # samples after resampling
    n_chunks: np.ndarray
    decoded: dict = field(default_factory=dict)  # kind 1 windows that had to be decoded to learn their length

    def sub(self, lo: int, hi: int) -> "FileTable":
        """Files ``[lo, hi)`` as a table of their own."""
        arrays = ("kind", "fmt", "channels", "sr0", "frames", "file_off", "nbytes", "n_out", "n_chunks")
        return FileTable(self.paths[lo:hi], *(getattr(self, a)[lo:hi] for a in arrays), {i - lo: w for i, w in self.decoded.items() if lo <= i < hi})


def plan_files(paths: list[str], sample_rate: int, chunk_duration: float, chunk_overlap: float, max_duration=60,
               n_threads: int | None = None, keep_decoded: bool = True) -> FileTable:
    """Probe every file's container (threads, headers only) and derive window, resampled and chunk sizes.

    Plain WAV: exact, from the header.  FLAC: from STREAMINFO (the first 64 KB of the file); a stream that does not state its length,
    and every other container, is decoded now (``read_pcm_window``) and kept until its group is staged — unless ``keep_decoded`` is off
    (the weights pass of the sharded ``evaluate``: every rank needs every file's chunk COUNT, not its samples; holding the decoded windows of
    the whole data set on every rank only to throw them away was ADVICE r4)."""
    n = len(paths)
    lay = _pcmio.probe_wavs(paths, n_threads)
    kind = np.full(n, -1, np.int32)
    fmt = np.zeros(n, np.int32)
    ch = lay["channels"].astype(np.int64)
    sr0 = lay["sample_rate"].astype(np.int64)
    bits = lay["bits"].astype(np.int64)
    frames = np.zeros(n, np.int64)
    file_off = np.zeros(n, np.int64)
    is_wav_name = np.array([p.lower().endswith(".wav") for p in paths], bool) if n else np.zeros(0, bool)
    raw_fmt = np.full(n, -1, np.int32)
    for (code, b), f in _RAW_FORMATS.items():
        raw_fmt[(lay["format_tag"] == code) & (bits == b)] = f
    raw = is_wav_name & (lay["status"] == 0) & (raw_fmt >= 0) & (ch >= 1) & (sr0 > 0)
    frame_bytes = np.where(raw, (bits // 8) * ch, 1)
    total = np.where(raw, lay["data_bytes"] // frame_bytes, 0)
    cnt = window_counts(total, np.where(raw, sr0, 0), max_duration)
    raw &= cnt > 0
    kind[raw] = 0
    fmt[raw] = raw_fmt[raw]
    frames[raw] = cnt[raw]
    file_off[raw] = lay["data_offset"][raw]
    decoded: dict[int, object] = {}
    rest = [i for i in range(n) if not raw[i] and not (is_wav_name[i] and lay["status"][i] == 0 and cnt[i] <= 0 and raw_fmt[i] >= 0)]
    if rest:
        def slow(i):
            p = paths[i]
            if p.lower().endswith(".flac"):
                try:
                    from birdnet_stm32.audio import _flac

                    with open(p, "rb") as fh:
                        head = fh.read(65536)
                    fsr, fch, bps, ftotal = _flac.flac_info(head)
                    if ftotal > 0 and 1 <= fch and fsr > 0:
                        c = int(window_counts(np.array([ftotal]), np.array([fsr]), max_duration)[0])
                        return (PCM_S16 if bps == 16 else PCM_S32, fch, fsr, c, None) if c > 0 else None
                except Exception:
                    pass
            w = read_pcm_window(p, max_duration, chunk_duration, False)
            if w is None or w.frames <= 0:
                return None
            return (w.fmt, w.channels, w.sample_rate, w.frames, w)

        with ThreadPoolExecutor(max_workers=n_threads or _pcmio.default_threads()) as pool:
            for i, r in zip(rest, pool.map(slow, rest)):
                if r is None:
                    continue
                kind[i], fmt[i], ch[i], sr0[i], frames[i] = 1, r[0], r[1], r[2], r[3]
                if r[4] is not None and keep_decoded:
                    decoded[i] = r[4]
    good = kind >= 0
    ch = np.where(good, ch, 0)
    sr0 = np.where(good, sr0, 0)
    bps = np.array([_BYTES[int(f)] for f in fmt], np.int64) if n else np.zeros(0, np.int64)
    nbytes = np.where(good, frames * ch * bps, 0)
    n_out = np.where(good, resampled_lengths(frames, sr0, sample_rate), 0)
    n_chunks = chunk_counts(n_out, sample_rate, chunk_duration, chunk_overlap)
    return FileTable(list(paths), kind, fmt, ch, sr0, frames, file_off, nbytes, n_out, n_chunks, decoded)


def cut_groups(nbytes: np.ndarray, n_chunks: np.ndarray, slab_bytes: int, group_chunks: int, ramp: tuple = (8, 4, 2)) -> list[tuple[int, int]]:
    """Greedy contiguous groups of files: at most ``group_chunks`` chunks, ``slab_bytes`` bytes (with per-sub-group alignment slack)
    and ``MAX_WINDOWS_PER_GROUP`` files each; a single file larger than either limit forms its own group.  The first ``len(ramp)``
    groups are cut at ``slab_bytes / ramp[i]``: the copy stream has nothing to do until the first slab is read, so the pipeline starts
    on a small one (a full 256 MB slab costs ~4.5 ms of reading before the first byte crosses the bus)."""
    n = int(nbytes.shape[0])
    cb = np.concatenate([[0], np.cumsum(nbytes + _ALIGN)])
    cc = np.concatenate([[0], np.cumsum(n_chunks)])
    groups, a = [], 0
    while a < n:
        div = ramp[len(groups)] if len(groups) < len(ramp) else 1
        b = int(min(np.searchsorted(cb, cb[a] + slab_bytes // div, side="right") - 1, np.searchsorted(cc, cc[a] + group_chunks, side="right") - 1,
                    a + MAX_WINDOWS_PER_GROUP))
        b = max(b, a + 1)
        groups.append((a, b))
        a = b
    return groups


@dataclass
class ChunkSelection:
    """Which chunks of a file the pipeline keeps (the reference loader's ``max_chunks_per_file`` / ``snr_threshold`` /
    ``candidate_chunks_per_file``, data/generator.py:87-157; the remaining fields are the defaults of ``audio/activity.py``).

    A file with more grid chunks than ``candidate_chunks`` is cropped around its loudest stretches (``smart_crop``), any other keeps its
    grid; candidates are ranked by activity ratio, those under ``activity_threshold`` dropped (one is always kept), the first
    ``max_chunks_per_file`` taken.  ``exact_stft``: rank the bytes of ``bn_stft_mag_exact`` instead of the fast float32 STFT."""

    max_chunks_per_file: int
    activity_threshold: float = 0.1
    candidate_chunks: int | None = None
    k: float = 2.0
    max_active: float = 0.8
    subsample: int = 512
    energy_percentile: float = 75.0
    exact_stft: bool = False

    def __post_init__(self):
        if int(self.max_chunks_per_file) < 1:
            raise ValueError(f"max_chunks_per_file must be at least 1, got {self.max_chunks_per_file}")
        self.max_chunks_per_file = int(self.max_chunks_per_file)
        if self.candidate_chunks is None:
            self.candidate_chunks = min(8, max(4, 2 * self.max_chunks_per_file))
        self.candidate_chunks = int(self.candidate_chunks)
        if self.candidate_chunks < 1:
            raise ValueError(f"candidate_chunks must be at least 1, got {self.candidate_chunks}")
        if not 1 <= int(self.subsample) <= 512:
            raise ValueError(f"subsample={self.subsample}: bn_activity_counts takes the median over 1..512 elements")

    def crops(self, n_chunks) -> np.ndarray:
        """Per file: does it go through the smart crop (more grid chunks than candidates) or keep its grid?"""
        return np.asarray(n_chunks, np.int64) > self.candidate_chunks

    def candidate_counts(self, n_chunks) -> np.ndarray:
        """Upper bound of candidate rows per file (a crop may find fewer salient stretches than ``candidate_chunks``)."""
        return np.minimum(np.asarray(n_chunks, np.int64), self.candidate_chunks)

    def max_counts(self, n_chunks) -> np.ndarray:
        """Upper bound of selected rows per file."""
        return np.minimum(np.asarray(n_chunks, np.int64), self.max_chunks_per_file)


def selection_from_args(args, activity_threshold: float | None = None) -> ChunkSelection | None:
    """The selection the ``--max_chunks_per_file`` / ``--activity_threshold`` / ``--candidate_chunks`` flags of ``probe`` and ``embed`` ask for
    (``None`` when the first is 0 or absent)."""
    n = int(getattr(args, "max_chunks_per_file", 0) or 0)
    if n < 0:
        raise ValueError(f"--max_chunks_per_file must be >= 0, got {n}")
    if n == 0:
        return None
    cand = int(getattr(args, "candidate_chunks", 0) or 0)
    if cand < 0:
        raise ValueError(f"--candidate_chunks must be >= 0 (0 = the default min(8, max(4, 2 N))), got {cand}")
    thr = float(getattr(args, "activity_threshold", 0.1)) if activity_threshold is None else float(activity_threshold)
    return ChunkSelection(n, activity_threshold=thr, candidate_chunks=cand if cand > 0 else None)


STE_FRAME, STE_HOP = 1024, 512   # what bn_short_time_energy implements; smart_crop derives them for every chunk of >= 4096 samples


def ste_frame_counts(n_out, crop) -> np.ndarray:
    """Energy frames per window: ``1 + (n - 1024) // 512`` for the windows that are cropped, 0 for the others."""
    n = np.asarray(n_out, np.int64)
    return np.where(np.asarray(crop, bool) & (n >= STE_FRAME), 1 + (n - STE_FRAME) // STE_HOP, 0).astype(np.int64)


def candidate_table(n_out: np.ndarray, profiles: list, sel: ChunkSelection, sample_rate: int, chunk_duration: float):
    """Candidate chunks of a group's files, in file order: ``(start within the window, valid samples, owner file)`` arrays.

    ``profiles[j]`` is file j's short-time-energy profile when the file is cropped (its starts are then ``smart_crop``'s, off the grid), else
    ``None`` (it keeps the chunk grid without overlap, the reference's ``split_audio_into_chunks`` as its loader calls it).  Host only."""
    from birdnet_stm32.audio import activity

    size = int(sample_rate * chunk_duration)
    n_out = np.asarray(n_out, np.int64)
    start, valid, _owner, counts, _ = chunk_table_arrays(n_out, sample_rate, chunk_duration, 0.0)
    first = np.cumsum(counts) - counts
    starts, valids, owners = [], [], []
    for j, prof in enumerate(profiles):
        if prof is not None:
            st = np.asarray(activity._crop_starts(prof, int(n_out[j]), size, STE_HOP, sel.candidate_chunks, sel.energy_percentile), np.int64)
            va = np.full(st.shape[0], size, np.int32)
        else:
            st, va = start[first[j] : first[j] + counts[j]], valid[first[j] : first[j] + counts[j]]
        starts.append(st)
        valids.append(va)
        owners.append(np.full(st.shape[0], j, np.int64))
    if not starts:
        return np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64)
    return np.concatenate(starts).astype(np.int64), np.concatenate(valids).astype(np.int32), np.concatenate(owners)


def rank_rows(active: np.ndarray, n_feat: int, owner: np.ndarray, n_files: int, sel: ChunkSelection):
    """From the candidates' active-element counts to the rows that stay: ``(candidate indices per file in rank order, rows kept per file)``.
    Ratio, ``max_active``, ``np.argsort(r)[::-1]`` and the threshold in float64, as ``audio/activity.py`` does them.  Host only."""
    from birdnet_stm32.audio import activity

    ratios = np.array([activity.ratio_from_count(int(a), n_feat, sel.max_active) for a in active], np.float64)
    first = np.concatenate([[0], np.cumsum(np.bincount(np.asarray(owner, np.int64), minlength=n_files))]) if n_files else np.zeros(1, np.int64)
    rows, kept_per_file = [], np.zeros(n_files, np.int64)
    for j in range(n_files):
        a, b = int(first[j]), int(first[j + 1])
        if b > a:
            kept = activity.rank_by_activity(ratios[a:b], sel.activity_threshold)[: sel.max_chunks_per_file]
            rows.extend(a + r for r in kept)
            kept_per_file[j] = len(kept)
    return np.asarray(rows, np.int64), kept_per_file


@dataclass
class GroupLayout:
    """Where one group's windows lie in its slab and what its offset table holds (pure host data; see ``layout_group``)."""

    lo: int
    hi: int
    files: np.ndarray         # file indices (table order) that made it into the group, in file order
    counts: np.ndarray        # chunks per file of [lo, hi) (0 for files that dropped out)
    subs: list                # per sub-group: (slab byte offset, fmt, channels, sr0, first window, n windows, in_off word offset, max_in, max_out)
    n_windows: int
    n_chunks: int
    total_out: int            # resampled samples of all windows
    used: int                 # slab bytes
    tab_len: int              # table words (int64)
    off_out: int              # word offsets of the tables: resampled offsets [n_windows + 1],
    off_src: int              # chunk source positions [n_chunks] (int64),
    off_valid: int            # chunk valid lengths [n_chunks] (int32, two per word),
    off_owner: int            # chunk window indices [n_chunks] (int32)
    win_of_file: np.ndarray | None = None   # window index of files[j] (selection builds its own chunk tables from it)


def layout_group(tab: FileTable, lo: int, hi: int, base_ptr: int, capacity: int, table: np.ndarray, sample_rate: int, chunk_duration: float,
                 chunk_overlap: float, max_duration=60, n_threads: int | None = None, read_mode: str | None = None) -> GroupLayout:
    """Read the windows of files ``[lo, hi)`` into the slab at ``base_ptr`` and write the group's offset tables into ``table``.

    Windows are ordered by (format, channels, native rate) — each such *sub-group* is one ``bn_ingest_resample`` launch and lies
    back to back from a 256-byte aligned start — and keep file order inside a sub-group.  The chunk table is in FILE order, so the
    score rows of one file are contiguous and files follow the caller's order.  A file that fails now (it was readable when probed)
    drops out and the group is laid out again without it.  Host only: no GPU call in here.
    """
    alive = np.arange(lo, hi)[tab.kind[lo:hi] >= 0]
    while True:  # (repeats only when a file failed between probing and reading)
        key = (tab.fmt[alive].astype(np.int64) << 40) | (tab.channels[alive] << 32) | tab.sr0[alive]
        order = np.argsort(key, kind="stable")       # window w of the group = file alive[order[w]]
        wfile = alive[order]
        wkey = key[order]
        bounds = np.flatnonzero(np.concatenate([[True], wkey[1:] != wkey[:-1], [True]])) if wfile.size else np.array([0])
        nb = tab.nbytes[wfile]
        dst = np.zeros(wfile.shape[0], np.int64)
        subs_meta, pos = [], 0
        for s in range(len(bounds) - 1):
            w0, w1 = int(bounds[s]), int(bounds[s + 1])
            pos = -(-pos // _ALIGN) * _ALIGN
            csum = np.cumsum(nb[w0:w1])
            dst[w0:w1] = pos + csum - nb[w0:w1]
            subs_meta.append((pos, w0, w1))
            pos += int(csum[-1])
        used = pos
        if used > capacity:
            raise RuntimeError(f"evaluate pipeline: a group of {used} bytes outgrew its slab of {capacity}")
        raw_w = np.flatnonzero(tab.kind[wfile] == 0)
        status = _pcmio.read_windows([tab.paths[i] for i in wfile[raw_w]], tab.file_off[wfile[raw_w]], nb[raw_w], base_ptr, dst[raw_w], n_threads, read_mode)
        failed = set(wfile[raw_w][status != 0].tolist())
        host_w = np.flatnonzero(tab.kind[wfile] == 1)
        if host_w.size:
            def decode(w):
                i = int(wfile[w])
                win = tab.decoded.pop(i, None) or read_pcm_window(tab.paths[i], max_duration, chunk_duration, False)
                if win is None or win.fmt != tab.fmt[i] or win.channels != tab.channels[i] or win.sample_rate != tab.sr0[i] or win.payload.nbytes != nb[w]:
                    return None
                return np.ascontiguousarray(win.payload)

            with ThreadPoolExecutor(max_workers=n_threads or _pcmio.default_threads()) as pool:
                payloads = list(pool.map(decode, host_w))
            good = [j for j, p in enumerate(payloads) if p is not None]
            failed |= {int(wfile[host_w[j]]) for j, p in enumerate(payloads) if p is None}
            if good:
                _pcmio.copy_into([payloads[j] for j in good], base_ptr, dst[host_w[good]], n_threads)
        if not failed:
            break
        alive = np.array([i for i in alive if i not in failed], np.int64)
    n_windows = int(wfile.shape[0])
    n_chunks = int(tab.n_chunks[wfile].sum())
    half = -(-n_chunks // 2)
    need = (n_windows + len(subs_meta)) + (n_windows + 1) + n_chunks + 2 * half
    if need > table.shape[0]:
        raise RuntimeError(f"evaluate pipeline: a group's table of {need} words outgrew its buffer of {table.shape[0]}")
    n_out = tab.n_out[wfile]
    out_off = np.zeros(n_windows + 1, np.int64)
    np.cumsum(n_out, out=out_off[1:])
    cur = 0
    subs = []
    for pos, w0, w1 in subs_meta:
        fr = tab.frames[wfile[w0:w1]]
        table[cur] = 0
        np.cumsum(fr, out=table[cur + 1 : cur + 1 + (w1 - w0)])
        f0 = int(wfile[w0])
        subs.append((pos, int(tab.fmt[f0]), int(tab.channels[f0]), int(tab.sr0[f0]), w0, w1 - w0, cur, int(fr.max()), int(n_out[w0:w1].max())))
        cur += w1 - w0 + 1
    off_out = cur
    table[cur : cur + n_windows + 1] = out_off
    cur += n_windows + 1
    # chunk table in FILE order (the rows of one file contiguous, files in the caller's order)
    win_of_file = np.empty(n_windows, np.int64)
    win_of_file[order] = np.arange(n_windows)   # alive[j] is window win_of_file[j]
    start, valid, owner_f, counts_f, _ = chunk_table_arrays(tab.n_out[alive], sample_rate, chunk_duration, chunk_overlap)
    owner_w = win_of_file[owner_f]
    off_src = cur
    table[cur : cur + n_chunks] = start + out_off[owner_w]
    cur += n_chunks
    off_valid = cur
    table[cur : cur + half].view(np.int32)[:n_chunks] = valid
    cur += half
    off_owner = cur
    table[cur : cur + half].view(np.int32)[:n_chunks] = owner_w.astype(np.int32)
    cur += half
    counts = np.zeros(hi - lo, np.int64)
    counts[alive - lo] = counts_f
    return GroupLayout(lo, hi, alive, counts, subs, n_windows, n_chunks, int(out_off[-1]), used, cur, off_out, off_src, off_valid, off_owner, win_of_file)


@dataclass
class _Staged:
    """One group on its way to the GPU."""

    lay: GroupLayout
    slot: int                 # index into the device slab ring
    copied: object            # event: H2D of slab + table done
    h2d_events: tuple         # (start, stop) on the copy stream
    read_s: float


@dataclass
class _Segment:
    """One segment of a streamed file on its way to the GPU."""

    file: int                 # index into the run's file table
    seg: tuple                # (o0, o1, s0, s1)
    first: bool
    last: bool
    slot: int
    copied: object
    h2d_events: tuple
    read_s: float
    nbytes: int


# Page-locked slabs no pipeline holds at the moment: (address, bytes).  A process keeps them (page-locking costs ~65 us per MiB; every `evaluate`
# call builds its own EvaluatePipeline) until release_pinned_slabs().
_SLAB_POOL: list = []
_SLAB_LOCK = threading.Lock()
_COPY_STREAMS: dict = {}   # str(device) -> the H2D stream every pipeline of this process uses on that device


class _PinnedSlab:
    """``nbytes`` of page-locked host memory from the library (``bn_host_alloc_pinned``) seen as a uint8 CPU tensor.

    Not ``torch.empty(pin_memory=True)``: that call page-locks under the GIL (17 ms per 256 MiB on the timing box), and while the helper thread of
    ``_ensure_slabs`` sat in it neither the reader thread nor the caller's thread ran a line of Python (tools/_cold_trace.py).  Through ctypes
    the GIL is released; PyTorch recognises the memory as page-locked by its address (``is_pinned()``), so ``copy_(non_blocking=True)`` stays
    asynchronous."""

    def __init__(self, ctx, nbytes: int, torch):
        self.ctx = ctx
        self.ptr = 0
        with _SLAB_LOCK:
            for i, (ptr, size) in enumerate(_SLAB_POOL):
                if size >= nbytes:
                    self.ptr, self.nbytes = ptr, size
                    del _SLAB_POOL[i]
                    break
        if not self.ptr:
            self.ptr, self.nbytes = ctx.alloc_pinned(nbytes), int(nbytes)
        self.tensor = torch.frombuffer((ctypes.c_uint8 * self.nbytes).from_address(self.ptr), dtype=torch.uint8)

    @classmethod
    def fresh(cls, ctx, nbytes: int, torch):
        """A newly page-locked slab (never one taken from the pool): what tops the pool up."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self.ptr, self.nbytes = ctx.alloc_pinned(nbytes), int(nbytes)
        self.tensor = torch.frombuffer((ctypes.c_uint8 * self.nbytes).from_address(self.ptr), dtype=torch.uint8)
        return self

    def release(self) -> None:
        if self.ptr:
            with _SLAB_LOCK:
                _SLAB_POOL.append((self.ptr, self.nbytes))
            self.ptr, self.tensor = 0, None


_PREPARE: list = []   # helper threads of prepare_for_evaluate that may still be page-locking (a pipeline waits for them before it judges the pool)
_PRELOADED: set = set()   # str(device) whose code objects prepare_for_evaluate has loaded


def prepare_for_evaluate(ctx, torch, slabs: int = 3, slab_bytes: int = 256 << 20) -> None:
    """What a first ``evaluate`` call of a process otherwise does on its critical path, started NOW on a helper thread: the library's code objects
    loaded (``bn_preload_kernels``), ``slabs`` page-locked staging slabs put into the process-wide pool (19 ms each), the copy stream created.
    ``load_model_runner(..., prepare_pipeline=True)`` calls this as soon as it has a context — before it parses and lowers the model file, which
    takes longer than all of it — so a one-shot ``python -m birdnet_stm32 evaluate`` finds everything in place (the reference's counterpart is the
    interpreter's ``allocate_tensors()`` at load, models/runners.py:58).  Idempotent; ``release_pinned_slabs()`` gives the memory back."""
    dev = torch.device("cuda", ctx.device)

    def work():
        try:
            torch.cuda.set_device(dev)
            ctx.preload_kernels()
            _PRELOADED.add(str(dev))
            key = str(dev)
            with _SLAB_LOCK:
                if key not in _COPY_STREAMS:
                    _COPY_STREAMS[key] = torch.cuda.Stream(device=dev)
            for _ in range(slabs):
                with _SLAB_LOCK:
                    if sum(1 for _, size in _SLAB_POOL if size >= slab_bytes) >= slabs:
                        break
                _PinnedSlab.fresh(ctx, slab_bytes, torch).release()
        except Exception:  # pragma: no cover - the first evaluate call then does what is missing itself
            pass

    th = threading.Thread(target=work, name="bn-prepare-evaluate", daemon=True)
    _PREPARE.append(th)
    th.start()


def release_pinned_slabs() -> int:
    """Give the pooled page-locked slabs back to the system; returns the bytes freed."""
    with _SLAB_LOCK:
        pool, _SLAB_POOL[:] = list(_SLAB_POOL), []
    lib = _hip.load_library()
    for ptr, _ in pool:
        _hip.check(lib.bn_host_free_pinned(ctypes.c_void_p(ptr)))
    return sum(size for _, size in pool)


class EvaluatePipeline:
    """Runs files of one rank through read -> H2D -> ingest + inference; see the module docstring.

    ``run(paths)`` returns ``(scores [N, C] CUDA float32 with the chunks in file order, chunks per file, stats)``.
    """

    def __init__(self, runner, sample_rate: int, chunk_duration: float, chunk_overlap: float = 0.0, max_duration=60,
                 slab_bytes: int = 256 << 20, group_chunks: int | None = None, readers: int | None = None, pinned_slabs: int = 3,
                 ramp: tuple = (8, 4, 2), numa_pin: bool | None = None, read_mode: str | None = None, stream_long: bool = False,
                 mono_budget_bytes: int = MONO_BUDGET_BYTES, select: ChunkSelection | None = None):
        import torch

        self.torch = torch
        self.runner = runner
        self.ctx = runner.ctx
        self.dev = runner.device
        # Several ranks on one host (torch.distributed.run sets LOCAL_WORLD_SIZE / LOCAL_RANK): every rank keeps its reader threads and the
        # first touch of its page-locked slabs on the CPUs of ITS GPU's NUMA node and takes an even share of that node's CPUs — before the
        # first thread starts and before the slabs exist.  (numa_pin: None = only when ranks share the host, True / False = force.)
        n_local = _pcmio.local_world_size()
        self.numa = {"numa_node": -1, "cpus": 0, "pinned": False}
        if numa_pin if numa_pin is not None else n_local > 1:
            self.numa = _pcmio.pin_process_to_gpu_node(torch, int(os.environ.get("LOCAL_RANK", "0")), n_local)
        self.sr, self.cd, self.ov, self.max_duration = int(sample_rate), float(chunk_duration), float(chunk_overlap), max_duration
        self.slab_bytes = int(slab_bytes)
        self.ramp = tuple(ramp)  # first groups cut at slab_bytes / ramp[i] (cut_groups)
        self.group_chunks = int(group_chunks or max(runner.max_batch, 1024))
        self.readers = int(readers or _pcmio.default_threads())
        if read_mode is not None:   # "mmap" (library default) | "pread": process-wide switch of the reader (csrc/host/bn_pcmio.c)
            _pcmio.set_read_mode(read_mode)
        self.n_pinned = max(2, int(pinned_slabs))
        self._n_ring = self.n_pinned       # slabs in use by the current ring (a process's first call: 2, see _ensure_slabs)
        self._top_up = (0, 0)              # (bytes, count) of slabs to page-lock behind the call for the pool
        self.size = int(self.sr * self.cd)
        self._taps: dict[tuple[int, int], object] = {}
        self._pinned: list = []
        self._slabs: list = []         # the _PinnedSlab behind every tensor of _pinned
        self._pinned_free: list = []   # per pinned slab: the event of the last H2D that read it
        self._dslab: list = []
        self._dslab_free: list = []    # per device slab: the event behind the last kernels that read it
        self._mono = self._chunks = self._peak = None
        self._tab_pinned: list = []
        self._tab_dev: list = []
        self.copy_stream = None
        self._slot_ready = [threading.Semaphore(1), threading.Semaphore(1)]
        self._stop = threading.Event()
        self._trace = None
        self._t0 = 0.0
        self._preloaded = False
        # embedding output (evaluation/embeddings.py): None = scores only; "float32" / "int8" = run() also fills self.embeddings [N, D]
        self.emb_dtype: str | None = None
        self.embeddings = None
        # model inputs kept on the device (the augmented probe fit): run() also fills self.inputs [N, input_elems], the rows predict_device takes
        self.keep_inputs = False
        self.inputs = None
        self.inputs_into = None   # a caller's [>= rows, input_elems] CUDA tensor that run() fills instead of allocating (embed_files: one buffer for all blocks)
        self._inp = None
        self.inputs_budget_bytes = 32 << 30
        self._emb = None
        # long files (module docstring): off = every file goes through the grouped path and must fit one slab
        self.stream_long = bool(stream_long)
        self.mono_budget_bytes = int(mono_budget_bytes)
        self._long_mono = self._long_peak = None
        self._long_payload: dict = {}   # streamed host-decoded file -> its decoded window (producer thread)
        # chunk selection (module docstring): None = every grid chunk, the path every earlier caller takes
        self.select = select
        self.selected_rows: list = []   # per run(): (file index into paths, start sample within its window) of every output row, in row order
        self.select_stats: dict = {}
        if select is not None:
            from birdnet_stm32.models import _pack as pk

            if self.stream_long:
                raise ValueError("chunk selection and stream_long cannot be combined: a streamed file's samples are never on the device at once "
                                 "in the grouped form the selection works on; lower max_duration or drop one of the two")
            if runner.input_kind == pk.INPUT_MEL:
                raise ValueError("chunk selection ranks the hybrid frontend's spectrograms or the raw frontend's waveforms; models with a "
                                 "precomputed frontend (librosa / log_mel / mfcc) are not supported")
            if self.ov > 0.0:
                raise ValueError("chunk selection works on chunks without overlap, as the reference's loader cuts them (cropped files take their "
                                 f"chunks off the grid anyway); chunk_overlap={self.ov} given")
            if self.size < 4 * STE_FRAME:
                raise ValueError(f"chunk selection needs chunks of at least {4 * STE_FRAME} samples (bn_short_time_energy implements frames of "
                                 f"{STE_FRAME} at hops of {STE_HOP}); {self.size} given")

    def _mark(self, name: str) -> None:
        """Timeline of one run (``BN_PIPELINE_TRACE=1``: ``stats["trace"]`` = [(what, seconds since run() started, thread)]) — where a COLD call's
        time goes cannot be read off per-stage busy times (tools/_cold_probe.py)."""
        tr = self._trace
        if tr is not None:
            tr.append((name, round(time.perf_counter() - self._t0, 5), threading.current_thread().name))

    # -- buffers (grow only) ------------------------------------------------------------------------------------------------
    def _ensure_slabs(self, need: int, tab_words: int) -> None:
        torch = self.torch
        cap = max(self.slab_bytes, need)
        while _PREPARE:   # (prepare_for_evaluate still page-locking: its slabs are the ones this call wants)
            _PREPARE.pop().join()
        for e in getattr(self, "_pinned_ready", []):   # (a helper thread of an earlier call is still allocating: let it finish before judging the sizes)
            e.wait()
        if not self._tab_pinned or self._tab_pinned[0].numel() < tab_words:
            words = max(tab_words, 1 << 16)
            self._tab_pinned = [torch.empty(words, dtype=torch.int64, pin_memory=True) for _ in range(self.n_pinned)]
            self._tab_dev = [torch.empty(words, dtype=torch.int64, device=self.dev) for _ in range(2)]
        if not self._pinned or self._pinned[0] is None or self._pinned[0].numel() < cap:
            # Page-locking 3 x 256 MiB costs ~0.14 s the first time (a one-shot `evaluate` call pays it: BENCH_r04 cold read_s 0.18 against
            # 0.04 warm).  The slabs are allocated by a helper thread, in the order the producer needs them; the producer waits for slab k only
            # when it gets to group k — the first (small, ramped) groups are read and copied while the other slabs are still being pinned.
            self._release_slabs()
            # A process without pooled slabs (its first call) runs on a ring of TWO: the third one's 19 ms of page-locking sat in front of the first
            # H2D copy (the runtime serialises the two); it is page-locked behind the call instead and pooled for the next one (_top_up_pool).
            with _SLAB_LOCK:
                pooled = sum(1 for _, size in _SLAB_POOL if size >= cap)
            self._n_ring = self.n_pinned if pooled >= self.n_pinned else max(2, pooled)
            self._top_up = (cap, self.n_pinned - self._n_ring)
            self._pinned = [None] * self._n_ring
            self._slabs = [None] * self._n_ring
            self._pinned_ready = [threading.Event() for _ in range(self._n_ring)]
            self._pinned_free = [None] * self._n_ring

            def allocate():
                try:
                    torch.cuda.set_device(self.dev)
                    for k in range(self._n_ring):
                        self._slabs[k] = _PinnedSlab(self.ctx, cap, torch)
                        self._pinned[k] = self._slabs[k].tensor
                        self._pinned_ready[k].set()
                        self._mark(f"slab {k} page-locked")
                except BaseException as exc:  # noqa: BLE001 - surfaces in the producer
                    self._pinned_error = exc
                    for e in self._pinned_ready:
                        e.set()

            self._pinned_error = None
            # (device slabs first: behind the helper thread they wait for the runtime until every slab is page-locked — 44 ms of a cold call)
            self._dslab = [torch.empty(cap, dtype=torch.uint8, device=self.dev) for _ in range(2)]
            self._dslab_free = [None, None]
            threading.Thread(target=allocate, name="bn-pin-slabs", daemon=True).start()

    def _release_slabs(self) -> None:
        for e in getattr(self, "_pinned_ready", []):
            e.wait()
        for sl in self._slabs:
            if sl is not None:
                sl.release()
        self._slabs, self._pinned = [], []

    def close(self) -> None:
        """Hand the page-locked slabs back to the process-wide pool (the next pipeline takes them without page-locking anything)."""
        if self.copy_stream is not None:
            self.copy_stream.synchronize()
        self._release_slabs()
        cap, count = self._top_up
        self._top_up = (0, 0)
        if count > 0 and cap > 0:   # the slabs a first call did without: page-locked now, off everybody's critical path, for the next call's ring
            ctx, torch, want = self.ctx, self.torch, self.n_pinned

            def top_up():
                try:
                    for _ in range(count):
                        with _SLAB_LOCK:   # (an earlier call's top-up may have got there first)
                            if sum(1 for _, size in _SLAB_POOL if size >= cap) >= want:
                                return
                        slab = _PinnedSlab.fresh(ctx, cap, torch)
                        slab.release()
                except Exception:  # pragma: no cover - the next call simply runs on a shorter ring
                    pass

            threading.Thread(target=top_up, name="bn-pin-top-up", daemon=True).start()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass

    def _filter(self, sr0: int):
        """(device taps or None, up, down, taps per phase, leading outputs to drop) for one native rate."""
        if sr0 == self.sr:
            return None, 1, 1, 0, 0
        g = gcd(sr0, self.sr)
        up, down = self.sr // g, sr0 // g
        key = (up, down)
        if key not in self._taps:
            taps, per_phase, pre = polyphase_filter(up, down)
            self._taps[key] = (self.torch.from_numpy(taps).to(self.dev), per_phase, pre)
        d, per_phase, pre = self._taps[key]
        return d, up, down, per_phase, pre

    # -- stage 1 + 2: producer thread ----------------------------------------------------------------------------------------------
    def _stage_group(self, tab: FileTable, lo: int, hi: int, seq: int) -> _Staged:
        torch = self.torch
        t0 = time.perf_counter()
        k = seq % self._n_ring
        prev = self._pinned_free[k]
        if prev is not None:
            prev.synchronize()  # the H2D that last read this pinned slab has finished
        self._pinned_ready[k].wait()  # (the helper thread of _ensure_slabs has page-locked this slab)
        self._wait_s = getattr(self, "_wait_s", 0.0) + (time.perf_counter() - t0)   # (of read_s: waiting for a slab, not reading)
        if self._pinned_error is not None:
            raise self._pinned_error
        pinned = self._pinned[k]  # (sized for the largest group before the producer started: run())
        self._mark(f"group {seq}: slab ready")
        # While the helper thread of _ensure_slabs is still page-locking slabs the windows are taken with pread: registering a slab holds the
        # process's mmap lock (17 ms per 256 MiB), a mapping needs that lock for every file and pread needs it for none (tools/_cold_trace.py: the
        # first 32 MiB group of a cold call took 18 ms through mappings, 2 ms warm).
        pinning = not all(e.is_set() for e in self._pinned_ready)
        lay = layout_group(tab, lo, hi, pinned.data_ptr(), pinned.numel(), self._tab_pinned[k].numpy(), self.sr, self.cd, self.ov,
                           self.max_duration, self.readers, "pread" if pinning else None)
        read_s = time.perf_counter() - t0
        self._mark(f"group {seq}: read")
        # ---- H2D on the copy stream ----
        slot = seq % 2
        while not self._slot_ready[slot].acquire(timeout=0.1):  # the consumer has launched the group that used this device slab
            if self._stop.is_set():
                raise RuntimeError("evaluate pipeline stopped")
        with torch.cuda.device(self.dev), torch.cuda.stream(self.copy_stream):
            free = self._dslab_free[slot]
            if free is not None:
                self.copy_stream.wait_event(free)  # the kernels that read this device slab / table have run
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(self.copy_stream)
            if lay.used:
                self._dslab[slot][: lay.used].copy_(pinned[: lay.used], non_blocking=True)
            self._tab_dev[slot][: lay.tab_len].copy_(self._tab_pinned[k][: lay.tab_len], non_blocking=True)
            e1.record(self.copy_stream)
        self._pinned_free[k] = e1
        self._mark(f"group {seq}: H2D queued")
        return _Staged(lay, slot, e1, (e0, e1), read_s)

    def _stage_segment(self, tab: FileTable, i: int, seg: tuple, first: bool, last: bool, seq: int) -> _Segment:
        """Read input frames ``[s0, s1)`` of streamed file ``i`` into the next pinned slab and queue their H2D copy (the ring of
        ``_stage_group``; no offset table)."""
        torch = self.torch
        t0 = time.perf_counter()
        k = seq % self._n_ring
        prev = self._pinned_free[k]
        if prev is not None:
            prev.synchronize()
        self._pinned_ready[k].wait()
        self._wait_s = getattr(self, "_wait_s", 0.0) + (time.perf_counter() - t0)
        if self._pinned_error is not None:
            raise self._pinned_error
        pinned = self._pinned[k]
        _o0, _o1, s0, s1 = seg
        fb = _BYTES[int(tab.fmt[i])] * int(tab.channels[i])
        nbytes = (s1 - s0) * fb
        pieces = np.arange(0, nbytes, _READ_PIECE, dtype=np.int64)
        sizes = np.minimum(nbytes - pieces, _READ_PIECE)
        if int(tab.kind[i]) == 0:
            status = _pcmio.read_windows([tab.paths[i]] * pieces.shape[0], int(tab.file_off[i]) + s0 * fb + pieces, sizes, pinned.data_ptr(), pieces,
                                         self.readers)
            if np.any(status != 0):
                raise RuntimeError(f"{tab.paths[i]}: reading input frames [{s0}, {s1}) failed")
        else:
            payload = self._long_payload.get(i)
            if payload is None:
                win = tab.decoded.pop(i, None) or read_pcm_window(tab.paths[i], self.max_duration, self.cd, False)
                if win is None or win.fmt != tab.fmt[i] or win.channels != tab.channels[i] or win.frames != tab.frames[i]:
                    raise RuntimeError(f"{tab.paths[i]}: decoding its window again gave a different stream")
                payload = self._long_payload[i] = np.ascontiguousarray(win.payload)
            part = payload[s0 * fb : s1 * fb]
            _pcmio.copy_into([part[a : a + b] for a, b in zip(pieces.tolist(), sizes.tolist())], pinned.data_ptr(), pieces, self.readers)
            if last:
                del self._long_payload[i]
        read_s = time.perf_counter() - t0
        slot = seq % 2
        while not self._slot_ready[slot].acquire(timeout=0.1):
            if self._stop.is_set():
                raise RuntimeError("evaluate pipeline stopped")
        with torch.cuda.device(self.dev), torch.cuda.stream(self.copy_stream):
            free = self._dslab_free[slot]
            if free is not None:
                self.copy_stream.wait_event(free)
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(self.copy_stream)
            if nbytes:
                self._dslab[slot][:nbytes].copy_(pinned[:nbytes], non_blocking=True)
            e1.record(self.copy_stream)
        self._pinned_free[k] = e1
        return _Segment(i, seg, first, last, slot, e1, (e0, e1), read_s, nbytes)

    # -- stage 3: consumer (caller's thread and stream) -----------------------------------------------------------------------
    def _compute_group(self, st: _Staged, scores, row0: int, batch: int, lat_events: list | None, stats: dict, ftab: FileTable | None = None) -> None:
        torch = self.torch
        lib = self.ctx.lib
        cur = torch.cuda.current_stream(self.dev)
        g = st.lay
        cur.wait_event(st.copied)
        stream = ctypes.c_void_p(cur.cuda_stream)
        if self._mono is None or self._mono.numel() < max(g.total_out, 1):
            self._mono = torch.empty(max(g.total_out, 1) * 5 // 4 + 1024, dtype=torch.float32, device=self.dev)
        if self._peak is None or self._peak.numel() < max(g.n_windows, 1):
            self._peak = torch.empty(max(g.n_windows, 1) * 5 // 4 + 64, dtype=torch.float32, device=self.dev)
        if self._chunks is None or self._chunks.shape[0] < g.n_chunks:
            self._chunks = None
            self._chunks = torch.empty((max(g.n_chunks, self.group_chunks), self.size), dtype=torch.float32, device=self.dev)
        self._mark("compute: buffers")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record(cur)
        if g.n_windows:
            self._peak[: g.n_windows].zero_()
        slab = self._dslab[st.slot].data_ptr()
        tab = self._tab_dev[st.slot].data_ptr()
        for pos, fmt, ch, sr0, w0, nw, in_off, max_in, max_out in g.subs:
            d_taps, up, down, per_phase, pre = self._filter(sr0)
            _hip.check(lib.bn_ingest_resample(self.ctx.handle, slab + pos, fmt, ch, tab + 8 * in_off, tab + 8 * (g.off_out + w0), nw, max_in, max_out,
                                              d_taps.data_ptr() if d_taps is not None else None, up, down, per_phase, pre,
                                              self._mono.data_ptr(), self._peak.data_ptr() + 4 * w0, stream))
        keep = None
        if self.select is not None:
            keep = self._select_rows(g, ftab, tab_dev=tab, stream=stream)   # (rewrites g.counts / g.n_chunks)
        elif g.n_chunks:
            _hip.check(lib.bn_ingest_chunks(self.ctx.handle, self._mono.data_ptr(), self._peak.data_ptr(), tab + 8 * g.off_src, tab + 8 * g.off_valid,
                                            tab + 8 * g.off_owner, g.n_chunks, self.size, self._chunks.data_ptr(), stream))
        done = torch.cuda.Event()
        done.record(cur)
        self._dslab_free[st.slot] = done  # slab and table may be overwritten once these launches have run
        self._slot_ready[st.slot].release()
        ev[1].record(cur)
        self._mark("compute: ingest launched")
        n = g.n_chunks
        emb = self._emb
        if n:
            if lat_events is None and emb is not None:
                self.runner.infer_audio_device(self._chunks[:n], out=scores[row0 : row0 + n], return_embeddings=True, emb_dtype=self.emb_dtype,
                                               emb_out=emb[row0 : row0 + n])
            elif lat_events is None:
                self.runner.infer_audio_device(self._chunks[:n], out=scores[row0 : row0 + n])
            else:
                for b0 in range(0, n, batch):
                    nb = min(batch, n - b0)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(cur)
                    kw = {} if emb is None else dict(return_embeddings=True, emb_dtype=self.emb_dtype, emb_out=emb[row0 + b0 : row0 + b0 + nb])
                    self.runner.infer_audio_device(self._chunks[b0 : b0 + nb], out=scores[row0 + b0 : row0 + b0 + nb], **kw)
                    b.record(cur)
                    lat_events.append((a, b, nb))
        ev[2].record(cur)
        if n and self._inp is not None:   # (after the events: the inference time stays the inference's)
            mb = int(self.runner.max_batch)
            for b0 in range(0, n, mb):
                self._inp[row0 + b0 : row0 + min(b0 + mb, n)].copy_(self.runner.model_inputs_device(self._chunks[b0 : min(b0 + mb, n)]))
        self._mark("compute: inference launched")
        stats["_events"].append((st.h2d_events, ev, g.used + 8 * g.tab_len))
        if keep is not None:
            stats.setdefault("_keep", []).append(keep)   # (the second bn_ingest_chunks reads its tables asynchronously)

    def _select_rows(self, g: GroupLayout, tab: FileTable, tab_dev: int, stream) -> tuple:
        """Selection for one group whose windows are resampled on the stream (module docstring).  On return ``self._chunks[: g.n_chunks]`` holds the
        selected rows, per file in rank order, and ``g.counts`` / ``g.n_chunks`` describe them.  Two host synchronisations: the energies
        (``_energies``) and the counts (``_count_candidates``); the decisions between them are ``candidate_table`` and ``rank_rows``."""
        torch, lib, sel, dev = self.torch, self.ctx.lib, self.select, self.dev
        files, wof = g.files, g.win_of_file
        n_out = tab.n_out[files].astype(np.int64)
        by_window = np.zeros(g.n_windows, np.int64)
        by_window[wof] = n_out
        out_off = np.concatenate([[0], np.cumsum(by_window)])
        crop = sel.crops(tab.n_chunks[files])
        times = {}
        t0 = time.perf_counter()
        ste, frame_off = self._energies(g, by_window, crop, tab_dev, stream, times)
        t1 = time.perf_counter()
        profiles = [ste[frame_off[w] : frame_off[w + 1]] if c else None for w, c in zip(wof.tolist(), crop.tolist())]
        c_start, c_valid, c_owner = candidate_table(n_out, profiles, sel, self.sr, self.cd)
        n_cand = int(c_start.shape[0])
        if n_cand > self._chunks.shape[0]:
            raise RuntimeError("chunk selection: more candidates than the group's planned chunks")
        c_src = c_start + out_off[wof[c_owner]]
        c_win = wof[c_owner].astype(np.int32)
        t2 = time.perf_counter()
        active, n_feat = self._count_candidates(c_src, c_valid, c_win, stream, times)
        t3 = time.perf_counter()
        keep_rows, new_counts = rank_rows(active, n_feat, c_owner, files.shape[0], sel)
        n_sel = int(keep_rows.shape[0])
        keep = None
        if n_sel:   # the selected rows, cut again from the resampled windows in their final order (the bytes bn_ingest_chunks gave the candidates)
            keep = tuple(torch.from_numpy(np.ascontiguousarray(a[keep_rows])).to(dev) for a in (c_src, c_valid, c_win))
            _hip.check(lib.bn_ingest_chunks(self.ctx.handle, self._mono.data_ptr(), self._peak.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(),
                                            keep[2].data_ptr(), n_sel, self.size, self._chunks.data_ptr(), stream))
            self.selected_rows.extend(zip(files[c_owner[keep_rows]].tolist(), c_start[keep_rows].tolist()))
        t4 = time.perf_counter()
        counts_all = np.zeros(g.hi - g.lo, np.int64)
        counts_all[files - g.lo] = new_counts
        g.counts, g.n_chunks = counts_all, n_sel
        # wall seconds of the four steps, and inside the two device steps the kernels' own time from events: what is left of a step is its
        # launches, table uploads and the round trip to the host
        times.update(candidates=n_cand, selected=n_sel, cropped_files=int(crop.sum()), ste_s=t1 - t0, host_crop_s=t2 - t1, features_s=t3 - t2,
                     host_rank_s=t4 - t3)
        times["round_trip1_s"] = times["ste_s"] - times.get("ste_kernel_s", 0.0)
        times["round_trip2_s"] = times["features_s"] - times.get("cut_kernel_s", 0.0) - times.get("stft_kernel_s", 0.0) - times.get("count_kernel_s", 0.0)
        for key, v in times.items():
            self.select_stats[key] = self.select_stats.get(key, 0) + v
        return keep

    def _timed(self, what: str, pairs: list):
        """Bracket a launch with two events on the current stream; ``_elapsed`` adds them up once the stream has been synchronised."""
        torch = self.torch
        cur = torch.cuda.current_stream(self.dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        pairs.append((what, a, b))
        a.record(cur)
        return lambda: b.record(cur)

    @staticmethod
    def _elapsed(pairs: list, times: dict) -> None:
        for what, a, b in pairs:
            times[what] = times.get(what, 0.0) + a.elapsed_time(b) / 1e3

    def _energies(self, g: GroupLayout, by_window: np.ndarray, crop: np.ndarray, tab_dev: int, stream, times: dict):
        """Short-time energies of the cropped files: one ``bn_short_time_energy`` launch over the group's windows (the others get an empty slice of
        the output) and round trip 1, 4 bytes per 512 samples.  Returns ``(energies, frame offsets per window)``."""
        torch, dev = self.torch, self.dev
        frame_off = np.zeros(g.n_windows + 1, np.int64)
        if not crop.any():
            return np.zeros(0, np.float32), frame_off
        crop_w = np.zeros(g.n_windows, bool)
        crop_w[g.win_of_file] = crop
        np.cumsum(ste_frame_counts(by_window, crop_w), out=frame_off[1:])
        d_frame_off = torch.from_numpy(frame_off).to(dev)
        d_index = torch.arange(g.n_windows, dtype=torch.int32, device=dev)
        d_ste = torch.empty(max(int(frame_off[-1]), 1), dtype=torch.float32, device=dev)
        pairs: list = []
        done = self._timed("ste_kernel_s", pairs)
        _hip.check(self.ctx.lib.bn_short_time_energy(self.ctx.handle, self._mono.data_ptr(), self._peak.data_ptr(), tab_dev + 8 * g.off_out,
                                                     d_index.data_ptr(), d_frame_off.data_ptr(), g.n_windows, STE_FRAME, STE_HOP, d_ste.data_ptr(), stream))
        done()
        ste = d_ste.cpu().numpy()   # (synchronises)
        self._elapsed(pairs, times)
        return ste, frame_off

    def _count_candidates(self, c_src: np.ndarray, c_valid: np.ndarray, c_win: np.ndarray, stream, times: dict):
        """Cut the candidates into ``self._chunks``, compute their features (hybrid frontend: ``bn_stft_mag(normalize=1)`` in slices of ``max_batch``;
        raw frontend: the chunks themselves) and count the active elements per candidate; round trip 2, 4 bytes per candidate.
        Returns ``(counts, elements per feature map)``."""
        from birdnet_stm32.audio import activity
        from birdnet_stm32.models import _pack as pk
        from birdnet_stm32.models.runners import stft_device

        torch, lib, sel, dev = self.torch, self.ctx.lib, self.select, self.dev
        n_cand = int(c_src.shape[0])
        raw = self.runner.input_kind == pk.INPUT_WAVEFORM
        n_feat = self.size if raw else 257 * self.runner.spec_width
        if not n_cand:
            return np.zeros(0, np.int32), n_feat
        pairs: list = []
        d_src, d_valid, d_win = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (c_src, c_valid, c_win))
        done = self._timed("cut_kernel_s", pairs)
        _hip.check(lib.bn_ingest_chunks(self.ctx.handle, self._mono.data_ptr(), self._peak.data_ptr(), d_src.data_ptr(), d_valid.data_ptr(),
                                        d_win.data_ptr(), n_cand, self.size, self._chunks.data_ptr(), stream))
        done()
        d_active = torch.empty(n_cand, dtype=torch.int32, device=dev)
        d_idx = torch.from_numpy(activity.subsample_indices(n_feat, sel.subsample).astype(np.int32)).to(dev)
        step = n_cand if raw else self.runner.max_batch
        for b0 in range(0, n_cand, step):
            nb = min(step, n_cand - b0)
            feat = self._chunks[b0 : b0 + nb]
            if not raw:
                done = self._timed("stft_kernel_s", pairs)
                feat = stft_device(self.ctx, feat, 512, None, self.runner.spec_width, True, exact=sel.exact_stft)
                done()
            done = self._timed("count_kernel_s", pairs)
            _hip.check(lib.bn_activity_counts(self.ctx.handle, feat.data_ptr(), nb, n_feat, d_idx.data_ptr(), d_idx.numel(), float(sel.k),
                                              d_active.data_ptr() + 4 * b0, None, stream))
            done()
        active = d_active.cpu().numpy()   # (synchronises)
        self._elapsed(pairs, times)
        return active, n_feat

    def _compute_segment(self, sg: _Segment, tab: FileTable, stats: dict) -> None:
        """One ``bn_ingest_resample_span`` launch: outputs ``[o0, o1)`` of the streamed file into its mono buffer, its peak folded in."""
        torch = self.torch
        cur = torch.cuda.current_stream(self.dev)
        i = sg.file
        if sg.first:
            n_out = int(tab.n_out[i])
            if self._long_mono is None or self._long_mono.numel() < n_out:
                self._long_mono = None
                self._long_mono = torch.empty(n_out, dtype=torch.float32, device=self.dev)
            if self._long_peak is None:
                self._long_peak = torch.empty(1, dtype=torch.float32, device=self.dev)
            self._long_peak.zero_()
        cur.wait_event(sg.copied)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record(cur)
        d_taps, up, down, per_phase, pre = self._filter(int(tab.sr0[i]))
        o0, o1, s0, s1 = sg.seg
        _hip.check(self.ctx.lib.bn_ingest_resample_span(
            self.ctx.handle, self._dslab[sg.slot].data_ptr(), int(tab.fmt[i]), int(tab.channels[i]), s0, s1 - s0, int(tab.frames[i]), o0, o1,
            d_taps.data_ptr() if d_taps is not None else None, up, down, per_phase, pre, self._long_mono.data_ptr(), self._long_peak.data_ptr(),
            ctypes.c_void_p(cur.cuda_stream)))
        done = torch.cuda.Event()
        done.record(cur)
        self._dslab_free[sg.slot] = done
        self._slot_ready[sg.slot].release()
        ev[1].record(cur)
        ev[2].record(cur)
        stats["_events"].append((sg.h2d_events, ev, sg.nbytes))

    def _finish_stream(self, tab: FileTable, i: int, scores, row0: int, stats: dict) -> int:
        """Chunks of streamed file ``i`` (its resampled samples are complete on the stream) scored in slices of ``group_chunks``."""
        torch = self.torch
        lib = self.ctx.lib
        cur = torch.cuda.current_stream(self.dev)
        stream = ctypes.c_void_p(cur.cuda_stream)
        start, valid, _owner, counts, _size = chunk_table_arrays(np.array([int(tab.n_out[i])], np.int64), self.sr, self.cd, self.ov)
        n = int(counts[0])
        if not n:
            return 0
        d_src = torch.from_numpy(start.astype(np.int64)).to(self.dev)
        d_valid = torch.from_numpy(valid.astype(np.int32)).to(self.dev)
        d_owner = torch.zeros(n, dtype=torch.int32, device=self.dev)
        if self._chunks is None or self._chunks.shape[0] < self.group_chunks:
            self._chunks = None
            self._chunks = torch.empty((self.group_chunks, self.size), dtype=torch.float32, device=self.dev)
        for c0 in range(0, n, self.group_chunks):
            nc = min(self.group_chunks, n - c0)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record(cur)
            _hip.check(lib.bn_ingest_chunks(self.ctx.handle, self._long_mono.data_ptr(), self._long_peak.data_ptr(), d_src.data_ptr() + 8 * c0,
                                            d_valid.data_ptr() + 4 * c0, d_owner.data_ptr(), nc, self.size, self._chunks.data_ptr(), stream))
            ev[1].record(cur)
            kw = {} if self._emb is None else dict(return_embeddings=True, emb_dtype=self.emb_dtype, emb_out=self._emb[row0 + c0 : row0 + c0 + nc])
            self.runner.infer_audio_device(self._chunks[:nc], out=scores[row0 + c0 : row0 + c0 + nc], **kw)
            ev[2].record(cur)
            stats["_events"].append((None, ev, 0))
        stats.setdefault("_keep", []).append((d_src, d_valid, d_owner))   # (the launches read them asynchronously)
        return n

    def _plan_items(self, tab: FileTable, streamed: np.ndarray) -> list:
        """Work in file order: ``("group", lo, hi)`` for runs of grouped files and ``("stream", i, segments)`` for each streamed file.
        Refuses, before anything is read, a streamed file whose resampled samples exceed ``mono_budget_bytes``."""
        items, a, n = [], 0, len(tab.paths)
        for i in np.flatnonzero(streamed):
            need = 4 * int(tab.n_out[i])
            if need > self.mono_budget_bytes:
                raise ValueError(f"{tab.paths[i]}: its {int(tab.n_out[i])} resampled samples need {need / 2**30:.1f} GiB of device memory, more than "
                                 f"the budget of {self.mono_budget_bytes / 2**30:.1f} GiB (mono_budget_bytes); lower max_duration")
        for b in list(np.flatnonzero(streamed)) + [n]:
            b = int(b)
            if b > a:
                ramp = self.ramp if not items else ()
                items += [("group", a + lo, a + hi) for lo, hi in cut_groups(tab.nbytes[a:b], tab.n_chunks[a:b], self.slab_bytes, self.group_chunks, ramp)]
            if b < n:
                up, down, hpp, pre = filter_geometry(int(tab.sr0[b]), self.sr)
                fb = _BYTES[int(tab.fmt[b])] * int(tab.channels[b])
                items.append(("stream", b, plan_segments(int(tab.frames[b]), int(tab.n_out[b]), up, down, hpp, pre, fb, self.slab_bytes)))
            a = b + 1
        return items

    def run(self, paths: list[str], batch_size: int | None = None, measure_latency: bool = False, table: FileTable | None = None):
        """Score every chunk of ``paths``: ``(scores [N, C] CUDA, chunks per file (list), stats dict, per-chunk latencies in ms)``.

        ``batch_size`` only matters with ``measure_latency``: inference then runs in slices of that many chunks, each bracketed by
        events on the launch stream (the reference's accounting: time of one ``predict`` / its batch size, replicated per chunk,
        evaluation/metrics.py:130-136) — without a host synchronisation per slice.  Otherwise slices are the runner's ``max_batch``.

        ``table``: the ``plan_files`` result for ``paths`` when the caller has it already.  With ``emb_dtype`` set, ``self.embeddings``
        holds the ``[N, D]`` CUDA embeddings of the same rows afterwards; with ``keep_inputs`` set, ``self.inputs`` holds their model
        inputs ``[N, input_elems]`` (``runner.model_inputs_device`` of every chunk; with a selection the selected rows in their final order).
        """
        torch = self.torch
        t_start = time.perf_counter()
        stats: dict = {"_events": []}
        self._t0 = t_start
        self._trace = [] if os.environ.get("BN_PIPELINE_TRACE") else None
        with torch.cuda.device(self.dev):
            if self.copy_stream is None:
                # one copy stream per device and PROCESS: every `evaluate` call builds its own pipeline, and the first copy on a new stream waits
                # ~5 ms for its hardware queue (tools/_cold_trace.py: "group 0: H2D queued" of every warm call)
                key = str(self.dev)
                with _SLAB_LOCK:
                    if key not in _COPY_STREAMS:
                        _COPY_STREAMS[key] = torch.cuda.Stream(device=self.dev)
                    self.copy_stream = _COPY_STREAMS[key]
            tab = table if table is not None else plan_files(paths, self.sr, self.cd, self.ov, self.max_duration, self.readers)
            stats["probe_s"] = time.perf_counter() - t_start
            streamed = long_files(tab, self.sr, self.slab_bytes) if self.stream_long else np.zeros(len(tab.paths), bool)
            self.selected_rows, self.select_stats = [], {}
            if self.select is not None and measure_latency:
                raise ValueError("chunk selection synchronises with the host inside a group: per-chunk latencies are not measured with it")
            if streamed.any():
                items = self._plan_items(tab, streamed)
                groups = [(it[1], it[2]) for it in items if it[0] == "group"]
            else:
                groups = cut_groups(tab.nbytes, tab.n_chunks, self.slab_bytes, self.group_chunks, self.ramp)
                items = [("group", lo, hi) for lo, hi in groups]
            planned = int(tab.n_chunks.sum())
            self.inputs = self._inp = None
            inp_rows = int(self.select.max_counts(tab.n_chunks).sum()) if self.select is not None else planned   # (a selection keeps at most that many)
            if self.keep_inputs:
                check_inputs_budget(inp_rows, int(self.runner.input_elems), self.inputs_budget_bytes, self.stream_long, measure_latency)
            # size the rings for the largest group once, before the producer starts (nothing is reallocated while copies are in flight)
            cb = np.concatenate([[0], np.cumsum(tab.nbytes + _ALIGN)])
            cc = np.concatenate([[0], np.cumsum(tab.n_chunks)])
            need_bytes = max((int(cb[b] - cb[a]) for a, b in groups), default=0)
            need_words = max((3 * (b - a) + 2 * int(cc[b] - cc[a]) + 16 for a, b in groups), default=16)
            self._mark("planned")
            self._ensure_slabs(need_bytes, need_words)
            self._mark("device slabs")
            self._slot_ready = [threading.Semaphore(1), threading.Semaphore(1)]
            self._dslab_free = [None, None]
            self._pinned_free = [None] * self._n_ring
            self._stop.clear()
            scores = torch.empty((max(planned, 1), self.runner.num_classes), dtype=torch.float32, device=self.dev)
            self.embeddings = self._emb = None
            if self.emb_dtype is not None:
                D = self.runner.embedding_info()["dim"]
                self._emb = torch.empty((max(planned, 1), D), dtype=torch.int8 if self.emb_dtype == "int8" else torch.float32, device=self.dev)
            if self.keep_inputs and self.inputs_into is not None:
                if self.inputs_into.shape[0] < inp_rows or self.inputs_into.shape[1] != int(self.runner.input_elems) or not self.inputs_into.is_contiguous():
                    raise ValueError(f"inputs_into must be a contiguous [>= {inp_rows}, {int(self.runner.input_elems)}] tensor")
                self._inp = self.inputs_into
            elif self.keep_inputs:
                self._inp = torch.empty((max(inp_rows, 1), int(self.runner.input_elems)), dtype=torch.float32, device=self.dev)
            q: queue.Queue = queue.Queue(maxsize=max(1, self._n_ring - 1))
            stop = self._stop

            def producer():
                try:
                    torch.cuda.set_device(self.dev)
                    seq = 0
                    for it in items:
                        if stop.is_set():
                            break
                        if it[0] == "group":
                            q.put(self._stage_group(tab, it[1], it[2], seq))
                            seq += 1
                            continue
                        _, i, segs = it
                        for j, seg in enumerate(segs):
                            if stop.is_set():
                                break
                            q.put(self._stage_segment(tab, i, seg, j == 0, j == len(segs) - 1, seq))
                            seq += 1
                    q.put(None)
                except BaseException as exc:  # noqa: BLE001 - handed to the consumer
                    q.put(exc)

            th = threading.Thread(target=producer, name="bn-evaluate-reader", daemon=True)
            th.start()
            if str(self.dev) in _PRELOADED:
                self._preloaded = True
            if not self._preloaded:   # this thread has nothing to do until the first group is on the device: load the kernels' code objects meanwhile
                self.ctx.preload_kernels()
                torch.empty(64, dtype=torch.float32, device=self.dev).zero_()   # (and the one torch kernel of the compute stage: _peak.zero_())
                self._preloaded = True
                self._mark("kernels preloaded")
            counts = np.zeros(len(paths), np.int64)
            lat_events: list | None = [] if measure_latency else None
            row = 0
            read_s = 0.0
            self._wait_s = 0.0
            read_groups = []
            try:
                while True:
                    g = q.get()
                    if g is None:
                        break
                    if isinstance(g, BaseException):
                        raise g
                    if isinstance(g, _Segment):
                        self._compute_segment(g, tab, stats)
                        read_s += g.read_s
                        if g.last:
                            counts[g.file] = self._finish_stream(tab, g.file, scores, row, stats)
                            row += int(counts[g.file])
                        continue
                    self._compute_group(g, scores, row, int(batch_size or self.runner.max_batch), lat_events, stats, tab)
                    counts[g.lay.lo : g.lay.hi] = g.lay.counts
                    row += g.lay.n_chunks
                    read_s += g.read_s
                    read_groups.append(round(g.read_s, 4))
            finally:
                stop.set()
                while th.is_alive():  # let a blocked producer finish its put()
                    try:
                        q.get_nowait()
                    except queue.Empty:
                        th.join(timeout=0.05)
            self._mark("all launched")
            torch.cuda.current_stream(self.dev).synchronize()
            self._mark("stream drained")
            h2d_ms = ingest_ms = infer_ms = 0.0
            moved = 0
            stats.pop("_keep", None)
            for h2d, ev, nbytes in stats.pop("_events"):
                if h2d is not None:
                    h2d_ms += h2d[0].elapsed_time(h2d[1])
                ingest_ms += ev[0].elapsed_time(ev[1])
                infer_ms += ev[1].elapsed_time(ev[2])
                moved += nbytes
            lat: list[float] = []
            if lat_events:
                for a, b, nb in lat_events:
                    lat.extend([a.elapsed_time(b) / nb] * nb)
        stats.update(files=len(paths), readable=int((tab.kind >= 0).sum()), chunks=row, groups=len(groups), streamed=int(streamed.sum()), read_s=read_s, h2d_s=h2d_ms / 1e3,
                     h2d_bytes=moved, h2d_gbps=(moved / 1e9) / (h2d_ms / 1e3) if h2d_ms > 0 else 0.0, ingest_s=ingest_ms / 1e3,
                     infer_s=infer_ms / 1e3, wall_s=time.perf_counter() - t_start, readers=self.readers, slab_bytes=self.slab_bytes,
                     group_chunks=self.group_chunks, local_world=_pcmio.local_world_size(), numa=dict(self.numa), read_mode=_pcmio.set_read_mode(None), slab_wait_s=round(self._wait_s, 4),
                     read_s_per_group=read_groups[:32])
        if self.select is not None:
            stats["select"] = dict(self.select_stats)
        if self._trace is not None:
            stats["trace"] = list(self._trace)
        if self._emb is not None:
            self.embeddings, self._emb = self._emb[:row], None
        if self._inp is not None:
            self.inputs, self._inp = self._inp[:row], None
        return scores[:row], counts.tolist(), stats, lat


def check_inputs_budget(rows: int, input_elems: int, budget_bytes: int, stream_long: bool = False, measure_latency: bool = False) -> None:
    """The refusals of ``keep_inputs``, from the plan alone (nothing has been read yet): ``rows`` model-input rows of ``input_elems`` float32
    must fit ``budget_bytes`` of device memory, and neither streaming nor latency slices go with it."""
    if stream_long:
        raise ValueError("keep_inputs and stream_long cannot be combined: a streamed file's chunks are cut slice by slice into one buffer")
    if measure_latency:
        raise ValueError("keep_inputs and measure_latency cannot be combined: keeping the inputs adds work between the timed slices")
    row_bytes = 4 * int(input_elems)
    if int(rows) * row_bytes > int(budget_bytes):
        raise ValueError(f"keeping the model inputs of {int(rows)} rows needs {int(rows) * row_bytes / 2**30:.1f} GiB of device memory, more than the "
                         f"budget of {int(budget_bytes) / 2**30:.1f} GiB (inputs_budget_bytes): {int(budget_bytes) // row_bytes} rows would fit; "
                         "pass fewer files or a selection (max_chunks_per_file)")


def balanced_bounds(weights, world: int) -> list[int]:
    """Contiguous blocks of the file list with (nearly) equal total weight: ``bounds[r] .. bounds[r+1]`` belongs to rank r.

    ``weights[i]`` = chunks of file i (plus a twentieth of a chunk for the host's per-file work, so that runs of unreadable files
    still spread).  Deterministic: every rank derives the same bounds from the same headers."""
    w = np.asarray(weights, np.float64) + 0.05
    c = np.concatenate([[0.0], np.cumsum(w)])
    cuts = [0] * (world + 1)
    for r in range(1, world):
        target = c[-1] * r / world
        i = int(np.searchsorted(c, target, side="left"))  # first prefix at or above the target ...
        if i > 0 and i < len(c) and target - c[i - 1] < c[i] - target:
            i -= 1                                          # ... unless the prefix in front of it is nearer (a long file at the cut goes to the later rank)
        cuts[r] = min(i, len(w))
    cuts[-1] = len(w)
    for r in range(1, world + 1):
        cuts[r] = max(cuts[r], cuts[r - 1])
    return cuts
