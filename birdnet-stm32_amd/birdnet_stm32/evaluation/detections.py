"""Files -> detections: which classes the model finds in which chunk of each recording (the question ``analyze`` answers).

The reference firmware prints the top-k classes of every file it scores (reference firmware/Src/main.c:110-132, ``print_top_k``);
here every chunk of every file gets its scores and the ones above a threshold become detections with a time span.

``detect_files`` runs the evaluate pipeline (``audio.pipeline.EvaluatePipeline``) with ``stream_long=True``: a recording longer than
one staging slab is read, copied and resampled segment by segment, so hour-long field recordings go through the device path whole
(``max_duration=0``).  The ``[N, C]`` scores come back to the host once per block of files (``C * 4`` bytes per chunk: ~0.5 MB per
recorded hour at 3 s chunks); selection, times and merging run there on numpy.

Semantics:

* **audio**: ``max_duration=0`` reads the whole file, a positive value its first ``max_duration`` seconds (as ``evaluate``); channel
  mean, resampling, peak normalisation over the whole window, then ``split_audio_into_chunks``.
* **times**: a chunk starts at its first sample / ``sample_rate``; the last chunk of a file starts at ``n - size``; a chunk ends at
  ``min(start + chunk_duration, n / sample_rate)``.
* **selection**: ``score >= threshold`` (per class from ``class_thresholds``, else ``min_conf``); ``top_k`` keeps the best k of a chunk;
  rows are in file order, chunk order, then score descending and class index ascending.
* **merging** (``merge_consecutive``): detections of one class in consecutive chunks of one file whose spans touch or overlap become
  one event with the first start, the last end and the highest score.
"""

from __future__ import annotations

import csv
import os
from dataclasses import dataclass, field

import numpy as np

RAVEN_COLUMNS = ("Selection", "View", "Channel", "Begin Time (s)", "End Time (s)", "Low Freq (Hz)", "High Freq (Hz)", "Scientific Name",
                 "Common Name", "Confidence", "Begin Path")
CSV_COLUMNS = ("file", "start_s", "end_s", "scientific_name", "common_name", "class_index", "confidence")


@dataclass
class Detections:
    """Result of :func:`detect_files`: one entry per detection (``file_index`` .. ``score``), per input file (``paths``,
    ``chunks_per_file``, ``duration_s``: seconds of the analysed window, 0 for a skipped file) and, with ``return_scores``, per chunk
    (``scores`` ``[N, C]`` float32 in file then chunk order, ``chunk_file``, ``chunk_start_s``)."""

    file_index: np.ndarray
    start_s: np.ndarray
    end_s: np.ndarray
    class_index: np.ndarray
    score: np.ndarray
    paths: list
    chunks_per_file: np.ndarray
    duration_s: np.ndarray
    skipped: list = field(default_factory=list)
    scores: np.ndarray | None = None
    chunk_file: np.ndarray | None = None
    chunk_start_s: np.ndarray | None = None
    sample_rate: int = 22050
    chunk_duration: float = 3.0

    def __len__(self) -> int:
        return int(self.file_index.shape[0])


@dataclass
class ChunkTable:
    """Where every chunk of a set of windows lies: owner file, first sample, samples up to the chunk's end (clipped to the window)."""

    file: np.ndarray
    start: np.ndarray
    end: np.ndarray
    sample_rate: int

    @property
    def start_s(self) -> np.ndarray:
        return self.start.astype(np.float64) / float(self.sample_rate)

    @property
    def end_s(self) -> np.ndarray:
        return self.end.astype(np.float64) / float(self.sample_rate)


def chunk_table(n_out, sample_rate: int, chunk_duration: float, chunk_overlap: float) -> ChunkTable:
    """The chunks the pipeline cuts from windows of ``n_out`` resampled samples, in its row order (``split_audio_into_chunks``)."""
    from birdnet_stm32.audio.pipeline import chunk_table_arrays

    n = np.asarray(n_out, np.int64)
    start, _valid, owner, _counts, size = chunk_table_arrays(n, sample_rate, chunk_duration, chunk_overlap)
    owner = owner.astype(np.int64)
    return ChunkTable(owner, start.astype(np.int64), np.minimum(start + size, n[owner]).astype(np.int64), int(sample_rate))


def class_thresholds_vector(num_classes: int, min_conf: float, class_thresholds: dict | None = None, class_names=None) -> np.ndarray:
    """Per-class thresholds ``[C]`` float32: ``class_thresholds[name]`` for the classes it names, ``min_conf`` for the rest."""
    thr = np.full(int(num_classes), min_conf, np.float32)
    if class_thresholds:
        if class_names is None:
            raise ValueError("class_thresholds names classes: pass class_names")
        index = {str(n): i for i, n in enumerate(class_names)}
        unknown = sorted(str(k) for k in class_thresholds if str(k) not in index)
        if unknown:
            raise ValueError(f"class_thresholds names unknown classes: {', '.join(unknown)}")
        for k, v in class_thresholds.items():
            thr[index[str(k)]] = float(v)
    return thr


def select(scores: np.ndarray, thresholds: np.ndarray, top_k: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """``(row, class)`` of every score at or above its class threshold, the best ``top_k`` per row at most; rows ascending, within a row
    score descending then class ascending."""
    s = np.asarray(scores)
    if s.ndim != 2:
        raise ValueError("scores must be [N, C]")
    if top_k is not None and top_k < 1:
        raise ValueError("top_k must be at least 1")
    order = np.argsort(-s, axis=1, kind="stable")   # (stable: equal scores keep class order)
    keep = np.take_along_axis(s >= np.asarray(thresholds, s.dtype)[None, :], order, axis=1)
    if top_k is not None:
        keep[:, top_k:] = False
    rows, pos = np.nonzero(keep)
    return rows.astype(np.int64), order[rows, pos].astype(np.int64)


def merge_consecutive(rows: np.ndarray, classes: np.ndarray, scores: np.ndarray, chunks: ChunkTable) -> tuple[np.ndarray, ...]:
    """Join detections of one class in consecutive chunks of one file whose spans touch or overlap (in samples).

    ``rows`` index ``chunks``.  Returns ``(first row, class, start sample, end sample, max score)`` per event, ordered by file, start,
    then score descending and class ascending."""
    rows = np.asarray(rows, np.int64)
    classes = np.asarray(classes, np.int64)
    scores = np.asarray(scores, np.float32)
    if rows.size == 0:
        z = np.zeros(0, np.int64)
        return z, z, z, z, np.zeros(0, np.float32)
    by = np.lexsort((rows, classes, chunks.file[rows]))   # file, class, chunk
    r, c, sc = rows[by], classes[by], scores[by]
    f = chunks.file[r]
    start, end = chunks.start[r], chunks.end[r]
    joins = np.zeros(r.shape[0], bool)
    joins[1:] = (f[1:] == f[:-1]) & (c[1:] == c[:-1]) & (r[1:] == r[:-1] + 1) & (start[1:] <= end[:-1])
    first = np.flatnonzero(~joins)
    last = np.append(first[1:], r.shape[0]) - 1
    ev_row, ev_cls = r[first], c[first]
    ev_start, ev_end = start[first], end[last]
    ev_score = np.maximum.reduceat(sc, first)
    order = np.lexsort((ev_cls, -ev_score.astype(np.float64), ev_start, chunks.file[ev_row]))
    return ev_row[order], ev_cls[order], ev_start[order], ev_end[order], ev_score[order]


def detections_from_scores(scores: np.ndarray, n_out, paths: list, sample_rate: int, chunk_duration: float, chunk_overlap: float = 0.0,
                           min_conf: float = 0.25, top_k: int | None = None, class_thresholds: dict | None = None, class_names=None,
                           merge: bool = False, skipped=(), return_scores: bool = False) -> Detections:
    """Detections of the ``[N, C]`` chunk scores of windows of ``n_out`` resampled samples (rows in the pipeline's order)."""
    scores = np.asarray(scores, np.float32)
    n_out = np.asarray(n_out, np.int64)
    chunks = chunk_table(n_out, sample_rate, chunk_duration, chunk_overlap)
    if scores.shape[0] != chunks.file.shape[0]:
        raise ValueError(f"{scores.shape[0]} score rows for {chunks.file.shape[0]} chunks")
    thr = class_thresholds_vector(scores.shape[1], min_conf, class_thresholds, class_names)
    rows, cls = select(scores, thr, top_k)
    val = scores[rows, cls]
    if merge:
        rows, cls, start, end, val = merge_consecutive(rows, cls, val, chunks)
    else:
        start, end = chunks.start[rows], chunks.end[rows]
    sr = float(sample_rate)
    counts = np.bincount(chunks.file, minlength=len(paths)).astype(np.int64) if len(paths) else np.zeros(0, np.int64)
    res = Detections(chunks.file[rows], start.astype(np.float64) / sr, end.astype(np.float64) / sr, cls, val.astype(np.float32), list(paths),
                     counts, n_out.astype(np.float64) / sr, list(skipped), sample_rate=int(sample_rate), chunk_duration=float(chunk_duration))
    if return_scores:
        res.scores, res.chunk_file, res.chunk_start_s = scores, chunks.file, chunks.start_s
    return res


def detect_files(runner, paths: list[str], min_conf: float = 0.25, top_k: int | None = None, class_thresholds: dict | None = None,
                 chunk_overlap: float = 0.0, max_duration=0, merge_consecutive: bool = False, sample_rate: int = 22050,
                 chunk_duration: float = 3.0, pipeline_options: dict | None = None, return_scores: bool = False, class_names=None,
                 budget_bytes: int = 256 << 20, head=None) -> Detections:
    """Detections in every file of ``paths`` (see the module docstring).  ``class_names`` (needed for ``class_thresholds``): the model's
    classes in score order.  ``pipeline_options``: keyword arguments of ``EvaluatePipeline`` (``slab_bytes``, ``readers``, ...);
    long files are streamed.  Score rows come to the host in blocks of files whose scores fit ``budget_bytes``.

    ``head`` (a ``training.linear_probe.ProbeHead``): the pipeline also writes its float32 embeddings, the head is applied to them on the
    device per block, and its ``[N, C_head]`` scores take the place of the model's — ``class_names`` and thresholds are then the head's."""
    from birdnet_stm32.audio.pipeline import EvaluatePipeline, plan_files
    from birdnet_stm32.evaluation.embeddings import _to_host, embedding_blocks

    sr, cd, ov = int(sample_rate), float(chunk_duration), float(chunk_overlap)
    C = int(runner.num_classes)
    if head is not None:
        head.check_embedding_dim(runner.embedding_info()["dim"])   # (refused before any audio is read)
        C = int(head.num_classes)
    class_thresholds_vector(C, min_conf, class_thresholds, class_names)   # (an unknown class name fails before any audio is read)
    opts = dict(pipeline_options or {})
    opts.setdefault("stream_long", True)
    pipe = EvaluatePipeline(runner, sr, cd, ov, max_duration=max_duration, **opts)
    row_bytes = C * 4
    if head is not None:
        pipe.emb_dtype = "float32"
        row_bytes = (C + head.embedding_dim + int(runner.num_classes)) * 4
    paths = list(paths)
    try:
        tab = plan_files(paths, sr, cd, ov, max_duration, pipe.readers)
        counts = tab.n_chunks.astype(np.int64)
        parts = []
        for lo, hi in embedding_blocks(counts, row_bytes, budget_bytes):
            if int(counts[lo:hi].sum()) == 0:
                continue
            scores, got, _stats, _lat = pipe.run(paths[lo:hi], table=tab.sub(lo, hi))
            if list(got) != counts[lo:hi].tolist():
                raise RuntimeError("the pipeline cut a different number of chunks than it planned")
            if head is not None:
                scores = head.predict_device(pipe.embeddings.contiguous(), runner.ctx)
                pipe.embeddings = None
            parts.append(_to_host(scores.contiguous()))
    finally:
        pipe.close()
    scores = np.concatenate(parts) if parts else np.zeros((0, C), np.float32)
    skipped = [p for p, k in zip(paths, tab.kind) if k < 0]
    return detections_from_scores(scores, tab.n_out, paths, sr, cd, ov, min_conf, top_k, class_thresholds, class_names, merge_consecutive, skipped,
                                  return_scores)


# -- writers --------------------------------------------------------------------------------------------------------------------------
def split_name(name: str) -> tuple[str, str]:
    """``"Scientific name_Common name"`` -> (scientific, common); a name without ``_`` is both."""
    sci, sep, common = str(name).partition("_")
    return (sci, common) if sep else (sci, sci)


def _fmt_time(t: float) -> str:
    return f"{float(t):.6f}"


def _fmt_score(s) -> str:
    return f"{float(np.float32(s)):.9g}"   # (9 significant digits: the float32 value round-trips)


def write_csv(path: str, det: Detections, class_names) -> None:
    """One table of all detections: ``file,start_s,end_s,scientific_name,common_name,class_index,confidence``."""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(CSV_COLUMNS)
        for f, a, b, c, s in zip(det.file_index.tolist(), det.start_s.tolist(), det.end_s.tolist(), det.class_index.tolist(), det.score.tolist()):
            sci, common = split_name(class_names[c])
            w.writerow([det.paths[f], _fmt_time(a), _fmt_time(b), sci, common, c, _fmt_score(s)])


def raven_table_names(paths: list) -> list[str]:
    """File name of each input's selection table: ``<stem>.selections.txt``, prefixed with the input's index where stems repeat."""
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    seen: dict = {}
    for s in stems:
        seen[s] = seen.get(s, 0) + 1
    return [f"{s}.selections.txt" if seen[s] == 1 else f"{i:05d}_{s}.selections.txt" for i, s in enumerate(stems)]


def write_raven(out_dir: str, det: Detections, class_names) -> list[str]:
    """One Raven selection table (tab-separated) per analysed input file in ``out_dir``; returns the paths written."""
    os.makedirs(out_dir, exist_ok=True)
    names = raven_table_names(det.paths)
    skipped = set(det.skipped)
    rows_of: dict = {}
    for j, f in enumerate(det.file_index.tolist()):
        rows_of.setdefault(f, []).append(j)
    high = det.sample_rate / 2
    written = []
    for f, p in enumerate(det.paths):
        if p in skipped:
            continue
        out = os.path.join(out_dir, names[f])
        with open(out, "w", newline="") as fh:
            w = csv.writer(fh, delimiter="\t", lineterminator="\n")
            w.writerow(RAVEN_COLUMNS)
            for sel, j in enumerate(rows_of.get(f, []), start=1):
                c = int(det.class_index[j])
                sci, common = split_name(class_names[c])
                w.writerow([sel, "Spectrogram 1", 1, _fmt_time(det.start_s[j]), _fmt_time(det.end_s[j]), 0, f"{high:g}", sci, common,
                            _fmt_score(det.score[j]), p])
        written.append(out)
    return written


def write_npz(path: str, det: Detections, class_names) -> None:
    """The full per-chunk scores and what places them: ``scores``, ``file_index``, ``start_s``, ``paths``, ``chunks_per_file``,
    ``class_names`` (plus ``end_s``, ``duration_s``, ``sample_rate``, ``chunk_duration``).  Needs ``return_scores``."""
    if det.scores is None:
        raise ValueError("the npz output holds the per-chunk scores: run detect_files with return_scores=True")
    sr = float(det.sample_rate)
    dur = det.duration_s[det.chunk_file] if det.chunk_file.size else np.zeros(0)
    end_s = np.minimum(det.chunk_start_s + det.chunk_duration, dur)
    np.savez(path, scores=np.asarray(det.scores, np.float32), file_index=np.asarray(det.chunk_file, np.int64),
             start_s=np.asarray(det.chunk_start_s, np.float64), end_s=end_s.astype(np.float64),
             paths=np.asarray([str(p) for p in det.paths], dtype=np.str_), chunks_per_file=np.asarray(det.chunks_per_file, np.int64),
             duration_s=np.asarray(det.duration_s, np.float64), class_names=np.asarray([str(n) for n in class_names], dtype=np.str_),
             sample_rate=np.int64(sr), chunk_duration=np.float64(det.chunk_duration))
