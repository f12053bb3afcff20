"""Files -> embeddings: the pooled feature vector in front of the classifier head, per chunk or per file.

The embedding is what a user of the reference reads as the backbone output (reference training/linear_probe.py:57-68: the last
GlobalAveragePooling2D or the attention pool; TFLite tensor 127 of the shipped INT8 model).  It is used to cluster or search
recordings, to train a classifier on a frozen backbone and to compare recordings.

``embed_files`` runs the evaluate pipeline (``audio.pipeline.EvaluatePipeline``: readers -> page-locked slabs -> copy stream -> device
ingest -> inference) with its embedding output switched on; the fused head kernels store the vector from where they pool it, so the
scores computed alongside are the ones ``evaluate`` computes.  Device memory is bounded: files are processed in blocks whose embeddings fit
``budget_bytes`` and each block is copied to the host.  Per-file pooling (``pooling="avg" | "max"``) is ``bn_pool_scores`` with
``n_classes = D`` (mean / max in float32, the same values as numpy's); log-mean-exp is a score pooling and is refused for features.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

EMBED_POOLINGS = ("none", "avg", "max")


@dataclass
class FileEmbeddings:
    """Result of :func:`embed_files`.

    ``embeddings``: ``[N, D]`` per chunk (rows in file order) or ``[F, D]`` per file (``pooling`` != "none": one row per file with
    chunks, in file order); ``file_index`` / ``start_s``: owner file (index into ``paths``) and start of each chunk in seconds within its
    file's read window; ``chunks_per_file``: per path (0 = unreadable or empty, see ``skipped``).  With a selection the rows of a file are
    its selected chunks, most active first, and ``start_s`` need not lie on the chunk grid."""

    embeddings: np.ndarray
    file_index: np.ndarray
    start_s: np.ndarray
    paths: list
    chunks_per_file: np.ndarray
    pooling: str
    dtype: str
    scale: float
    zero_point: int
    skipped: list = field(default_factory=list)
    candidate_rows: int = 0   # with a selection: rows that were ranked (``embeddings`` holds the ones that were kept)
    inputs: object = None     # with ``keep_inputs``: the rows' model inputs, one CUDA float32 tensor ``[N, input_elems]`` (never copied to the host)


def chunk_starts(n_out: np.ndarray, sample_rate: int, chunk_duration: float, chunk_overlap: float) -> tuple[np.ndarray, np.ndarray]:
    """``(file index, start in seconds)`` of every chunk the pipeline cuts from windows of ``n_out`` resampled samples (the chunk
    table of ``audio.pipeline.chunk_table_arrays``, in the pipeline's row order)."""
    from birdnet_stm32.audio.pipeline import chunk_table_arrays

    start, _valid, owner, _counts, _size = chunk_table_arrays(np.asarray(n_out, np.int64), sample_rate, chunk_duration, chunk_overlap)
    return owner.astype(np.int64), (start.astype(np.float64) / float(sample_rate))


_PINNED: dict = {}   # per device: a page-locked host buffer the blocks are copied through (grown on demand, kept for the next call)


def _to_host(t) -> np.ndarray:
    """Copy a CUDA tensor to a fresh numpy array through a reused page-locked buffer: a copy into pageable memory runs through the
    runtime's staging buffer at a fraction of the page-locked rate (10 MB took up to 20 ms)."""
    import torch

    key = str(t.device)
    nbytes = t.numel() * t.element_size()
    buf = _PINNED.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _PINNED[key] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
    view = buf[:nbytes].view(t.dtype).view(t.shape)
    view.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return view.numpy().copy()


def embedding_blocks(n_chunks: np.ndarray, row_bytes: int, budget_bytes: int) -> list[tuple[int, int]]:
    """Contiguous file ranges ``[lo, hi)`` whose embeddings (``n_chunks`` rows of ``row_bytes`` each) fit ``budget_bytes``; a single
    file larger than the budget forms a block of its own."""
    blocks, lo, acc = [], 0, 0
    for i, c in enumerate(np.asarray(n_chunks, np.int64)):
        need = int(c) * int(row_bytes)
        if i > lo and acc + need > budget_bytes:
            blocks.append((lo, i))
            lo, acc = i, 0
        acc += need
    if lo < len(n_chunks):
        blocks.append((lo, len(n_chunks)))
    return blocks


def embed_files(runner, paths: list[str], chunk_overlap: float = 0.0, max_duration=60, pooling: str = "none", dtype: str | None = None,
                sample_rate: int = 22050, chunk_duration: float = 3.0, budget_bytes: int = 256 << 20,
                pipeline_options: dict | None = None, select=None, keep_inputs: bool = False, inputs_budget_bytes: int = 32 << 30) -> FileEmbeddings:
    """Embeddings of every chunk of ``paths`` (the chunks ``evaluate`` scores: first ``max_duration`` seconds, ``chunk_duration`` chunks
    with ``chunk_overlap`` seconds of overlap at ``sample_rate``).

    ``dtype``: "float32" (default) or "int8" (INT8 models: the MEAN / attention-pool bytes themselves; dequantise with the result's
    ``scale`` / ``zero_point``).  ``pooling``: "none" (per chunk), "avg" or "max" (per file, float32 only).

    ``select``: an ``audio.pipeline.ChunkSelection`` — only each file's most active chunks are embedded (long files are cropped around
    their loudest stretches first, as the reference's training loader does); ``None`` embeds every grid chunk.

    ``keep_inputs``: also keep every row's model inputs (``HipRunner.model_inputs_device`` of its chunk) on the device and return them as
    one tensor, ``inputs [N, input_elems]`` (per-chunk rows only); refused, before a file is read, when they exceed ``inputs_budget_bytes``."""
    from birdnet_stm32.audio.ingest import pool_scores_device
    from birdnet_stm32.audio.pipeline import EvaluatePipeline, check_inputs_budget, plan_files

    pooling = pooling.lower()
    if pooling in ("mean", "average"):
        pooling = "avg"
    if pooling not in EMBED_POOLINGS:
        raise ValueError(f"pooling must be one of {EMBED_POOLINGS} for embeddings (log-mean-exp pools scores, not features), not {pooling!r}")
    info = runner.embedding_info()
    dtype = dtype or "float32"
    if dtype not in ("float32", "int8"):
        raise ValueError(f"dtype must be 'float32' or 'int8', not {dtype!r}")
    if dtype == "int8" and info["dtype"] != "int8":
        raise ValueError("int8 embeddings need an INT8 (.tflite) model; float32 models give float32")
    if dtype == "int8" and pooling != "none":
        raise ValueError("per-file pooling works on float32 embeddings: pass dtype='float32' (the dequantised bytes)")
    if keep_inputs and pooling != "none":
        raise ValueError("keep_inputs keeps one row per chunk: pass pooling='none'")
    D = int(info["dim"])
    row_bytes = D * (1 if dtype == "int8" else 4)
    sr, cd, ov = int(sample_rate), float(chunk_duration), float(chunk_overlap)
    opts = dict(pipeline_options or {})
    if select is not None:
        opts["select"] = select
    pipe = EvaluatePipeline(runner, sr, cd, ov, max_duration=max_duration, **opts)
    sel_file, sel_start, candidates = [], [], 0
    pipe.emb_dtype = dtype
    pipe.keep_inputs, pipe.inputs_budget_bytes = bool(keep_inputs), int(inputs_budget_bytes)
    all_inputs, kept_rows = None, 0
    try:
        tab = plan_files(list(paths), sr, cd, ov, max_duration, pipe.readers)
        big = np.flatnonzero(tab.nbytes > pipe.slab_bytes)
        if big.size:
            i = int(big[0])
            raise ValueError(f"{paths[i]}: its read window of {int(tab.nbytes[i])} bytes exceeds one staging slab ({pipe.slab_bytes} bytes = "
                             f"{pipe.slab_bytes >> 20} MiB); lower max_duration (streaming longer recordings is not supported)")
        counts = tab.n_chunks.astype(np.int64)
        if keep_inputs:   # all blocks together stay resident (with a selection: its upper bound)
            rows = int((select.max_counts(counts) if select is not None else counts).sum())
            check_inputs_budget(rows, int(runner.input_elems), inputs_budget_bytes, bool(opts.get("stream_long")))
            import torch

            # one buffer for all blocks, allocated once: the budget bounds what stays resident (no per-block buffers, no joined copy)
            all_inputs = torch.empty((max(rows, 1), int(runner.input_elems)), dtype=torch.float32, device=runner.device)
        selected = np.zeros_like(counts)
        parts = []
        for lo, hi in embedding_blocks(counts, row_bytes, budget_bytes):
            if int(counts[lo:hi].sum()) == 0:
                continue
            if keep_inputs:
                pipe.inputs_into = all_inputs[kept_rows:]
            _scores, got, _stats, _lat = pipe.run(list(paths[lo:hi]), table=tab.sub(lo, hi))
            if select is not None:   # the planned grid count is an upper bound; the pipeline reports what it kept
                if np.any(np.asarray(got) > select.max_counts(counts[lo:hi])):
                    raise RuntimeError("the pipeline selected more chunks than the selection allows")
                sel_file += [lo + f for f, _ in pipe.selected_rows]
                sel_start += [s0 for _, s0 in pipe.selected_rows]
                candidates += int(pipe.select_stats.get("candidates", 0))
                selected[lo:hi] = got
            elif list(got) != counts[lo:hi].tolist():
                raise RuntimeError("the pipeline cut a different number of chunks than it planned")
            emb = pipe.embeddings
            if pooling != "none":
                nz = [c for c in got if c]
                emb = pool_scores_device(runner.ctx, emb.contiguous(), nz, pooling)
            parts.append(_to_host(emb.contiguous()))
            pipe.embeddings = None
            if keep_inputs:
                kept_rows += int(pipe.inputs.shape[0])
                pipe.inputs = pipe.inputs_into = None
    finally:
        pipe.close()
    out = np.concatenate(parts) if parts else np.zeros((0, D), np.int8 if dtype == "int8" else np.float32)
    file_index, start_s = chunk_starts(tab.n_out, sr, cd, ov)
    if select is not None:
        counts = selected
        file_index, start_s = np.asarray(sel_file, np.int64), np.asarray(sel_start, np.float64) / float(sr)
    if pooling != "none":
        file_index = np.flatnonzero(counts > 0).astype(np.int64)
        start_s = np.zeros(file_index.shape[0], np.float64)
    skipped = [p for p, k in zip(paths, tab.kind) if k < 0]
    res = FileEmbeddings(out, file_index, start_s, list(paths), counts, pooling, dtype, float(info["scale"]), int(info["zero_point"]), skipped, candidates)
    if keep_inputs:
        res.inputs = all_inputs[:kept_rows]   # (with a selection a view of the buffer sized for its upper bound, which the budget covered)
    return res


def save_embeddings_npz(path: str, res: FileEmbeddings) -> None:
    """Write ``embeddings``, ``file_index``, ``start_s``, ``paths``, ``chunks_per_file`` (and ``scale`` / ``zero_point`` for int8) to an
    ``.npz`` archive (plain numpy arrays: ``np.load(path)`` reads it without this package)."""
    arrays = {
        "embeddings": np.asarray(res.embeddings),
        "file_index": np.asarray(res.file_index, np.int64),
        "start_s": np.asarray(res.start_s, np.float64),
        "paths": np.asarray([str(p) for p in res.paths], dtype=np.str_),
        "chunks_per_file": np.asarray(res.chunks_per_file, np.int64),
    }
    if res.dtype == "int8":
        arrays["scale"] = np.float32(res.scale)
        arrays["zero_point"] = np.int32(res.zero_point)
    np.savez(path, **arrays)
