"""``birdnet-stm32 search`` — query by example: where else does this call occur?

The database is one or more ``.npz`` archives written by ``embed``; the queries are audio files (embedded with ``--model_path`` exactly as
``embed`` would, per chunk or one per file with ``--query_pooling``) or rows already embedded (``--query_npz``, no model needed).  The k
nearest database rows of every query by cosine or dot score are found on the GPU (``evaluation/search.py``) and written as CSV:

    query_path, query_start_s, rank, score, match_path, match_start_s, match_end_s

``match_end_s`` is ``match_start_s`` plus the chunk duration (the model config's, or ``--chunk_duration`` with ``--query_npz``).
``--exclude_same_file`` drops hits from the query's own recording (resolved paths are compared).
"""

from __future__ import annotations

import argparse
import csv
import os

CSV_COLUMNS = ("query_path", "query_start_s", "rank", "score", "match_path", "match_start_s", "match_end_s")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Find the nearest embeddings of query clips in archives written by `embed`.")
    p.add_argument("--model_path", type=str, default="", help="Path to .keras or .tflite model (needed with --query)")
    p.add_argument("--model_config", type=str, default="", help="Path to model config JSON (default: <model>_model_config.json)")
    p.add_argument("--database", type=str, nargs="+", required=True, help="One or more .npz archives written by `embed`")
    p.add_argument("--query", type=str, nargs="+", default=[], help="Query audio files and/or directories (walked recursively)")
    p.add_argument("--query_npz", type=str, default="", help="Queries already embedded: an .npz archive written by `embed` (instead of --query)")
    p.add_argument("--output", type=str, required=True, help="Output CSV path")
    p.add_argument("--top_k", type=int, default=10, help="Hits per query (1..128)")
    p.add_argument("--metric", type=str, default="cosine", choices=["cosine", "dot"])
    p.add_argument("--query_pooling", type=str, default="none", choices=["none", "avg", "max"], help="One query per chunk (none) or per file (float32 only)")
    p.add_argument("--min_score", type=float, default=None, help="Drop hits whose score is lower")
    p.add_argument("--exclude_same_file", action="store_true", default=False, help="Drop hits from the query's own recording")
    p.add_argument("--chunk_duration", type=float, default=0.0, help="With --query_npz and no model: seconds per database row, for match_end_s")
    p.add_argument("--overlap", type=float, default=0.0, help="Chunk overlap of the query files (seconds)")
    p.add_argument("--max_duration", type=float, default=60, help="Seconds read from the start of each query file")
    p.add_argument("--max_batch", type=int, default=4096, help="Workspace size in chunks = inference slice of the device pipeline")
    p.add_argument("--device", type=int, default=0, help="MI355X index")
    return p


def validate_args(args) -> None:
    """Everything that can be refused before a model or an archive is read."""
    from birdnet_stm32.evaluation.search import MAX_K

    if bool(args.query) == bool(args.query_npz):
        raise ValueError("give either --query (audio files) or --query_npz (rows already embedded)")
    if args.query and not args.model_path:
        raise ValueError("--query needs --model_path to embed the files")
    if not 1 <= args.top_k <= MAX_K:
        raise ValueError(f"--top_k {args.top_k} outside 1..{MAX_K}")
    if args.query_npz and args.query_pooling != "none":
        raise ValueError("--query_pooling pools the chunks of query files; the rows of --query_npz are searched as they are")
    if args.query_npz and not args.model_path and not args.chunk_duration > 0:
        raise ValueError("--query_npz without --model_path needs --chunk_duration (seconds per database row)")
    if args.chunk_duration < 0 or args.overlap < 0:
        raise ValueError("--chunk_duration and --overlap must be >= 0")
    for path in list(args.database) + ([args.query_npz] if args.query_npz else []):
        if not os.path.isfile(path):
            raise FileNotFoundError(f"archive not found: {path}")


def write_hits_csv(path: str, query_paths: list, query_start_s, result, chunk_duration: float, min_score: float | None = None) -> int:
    """One line per hit (rank 1 = best); unused slots and hits below ``min_score`` are left out.  Returns the number of lines."""
    n = 0
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS)
        for q, (qp, qs) in enumerate(zip(query_paths, query_start_s)):
            for r in range(result.idx.shape[1]):
                if result.idx[q, r] < 0 or (min_score is not None and result.score[q, r] < min_score):
                    continue
                start = float(result.match_start_s[q, r])
                w.writerow([qp, f"{float(qs):.3f}", r + 1, f"{float(result.score[q, r]):.7g}", result.match_path[q][r], f"{start:.3f}", f"{start + chunk_duration:.3f}"])
                n += 1
    return n


def main(argv=None, runner=None):
    args = build_parser().parse_args(argv)
    try:
        validate_args(args)
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"error: {exc}") from None
    from birdnet_stm32.evaluation.search import EmbeddingIndex, _load_archive, same_file_index, search_files

    cfg = None
    if args.model_path:
        from birdnet_stm32.cli.evaluate import resolve_config_path
        from birdnet_stm32.training.config import ModelConfig

        cfg = ModelConfig.load(resolve_config_path(args.model_path, args.model_config)).to_dict()
    chunk_duration = args.chunk_duration if args.chunk_duration > 0 else float(cfg["chunk_duration"])
    try:
        index = EmbeddingIndex.from_npz(*args.database)
    except ValueError as exc:
        raise SystemExit(f"error: {exc}") from None
    if args.query_npz:
        try:
            q = _load_archive(args.query_npz)
            if q["dtype"] != index.dtype or q["embeddings"].shape[1] != index.dim:
                raise ValueError(f"{args.query_npz}: {q['embeddings'].shape[1]} x {q['dtype']} does not match the database: {index.dim} x {index.dtype}")
            if index.dtype == "int8" and (q["zero_point"] != index.zero_point or abs(q["scale"] - index.scale) > 0):
                raise ValueError(f"{args.query_npz}: int8 scale / zero point differ from the database's: the bytes are not comparable")
            qfile = same_file_index(index.paths, q["paths"])[q["file_index"]] if args.exclude_same_file else None
            hits = index.search(q["embeddings"], k=args.top_k, metric=args.metric, query_file_index=qfile, exclude_same_file=args.exclude_same_file,
                                device=args.device)
        except ValueError as exc:
            raise SystemExit(f"error: {exc}") from None
        query_paths, query_start = [q["paths"][int(i)] for i in q["file_index"]], q["start_s"]
    else:
        from birdnet_stm32.cli.embed import collect_inputs
        from birdnet_stm32.models.frontend import normalize_frontend_name

        files = collect_inputs(args.query)
        if not files:
            raise SystemExit(f"error: no audio files found in {' '.join(args.query)}")
        if args.query_pooling != "none" and index.dtype == "int8":
            raise SystemExit("error: --query_pooling works on float32 embeddings; the database holds int8 bytes")
        if runner is None:
            from birdnet_stm32.models.runners import load_model_runner

            runner = load_model_runner(args.model_path, device=args.device, max_batch=args.max_batch, prepare_pipeline=True)
        frontend = normalize_frontend_name(cfg["audio_frontend"])
        if frontend not in ("hybrid", "raw"):
            runner.configure_precomputed(frontend, int(cfg["sample_rate"]), cfg.get("mag_scale", "none"), int(cfg["fft_length"]), int(cfg["num_mels"]),
                                         int(cfg.get("n_mfcc", 20)))
        overlap = max(0.0, min(float(cfg["chunk_duration"]) - 0.1, args.overlap))
        try:
            hits, res = search_files(runner, index, files, k=args.top_k, metric=args.metric, query_pooling=args.query_pooling,
                                     exclude_same_file=args.exclude_same_file, chunk_overlap=overlap, max_duration=args.max_duration,
                                     sample_rate=int(cfg["sample_rate"]), chunk_duration=float(cfg["chunk_duration"]))
        except ValueError as exc:
            raise SystemExit(f"error: {exc}") from None
        query_paths, query_start = [res.paths[int(i)] for i in res.file_index], res.start_s
    n = write_hits_csv(args.output, query_paths, query_start, hits, chunk_duration, args.min_score)
    print(f"Searched {len(index)} rows x {index.dim} ({index.dtype}) with {hits.idx.shape[0]} queries ({args.metric}, top {args.top_k}): {n} hits -> {args.output}")
    index.close()
    return hits


if __name__ == "__main__":
    main()
