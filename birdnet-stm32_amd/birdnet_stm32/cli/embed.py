"""``birdnet-stm32 embed`` — embeddings of audio files on the GPU, written to an ``.npz`` archive.

The embedding is the pooled feature vector in front of the classifier head (``evaluation/embeddings.py``).  The chunking follows the
model's ``<model>_model_config.json`` (``sample_rate``, ``chunk_duration``, ``audio_frontend``), as in ``evaluate``.  ``--input`` takes
files and directories; directories are walked recursively for ``data.dataset.SUPPORTED_AUDIO_EXTS``.

Output keys: ``embeddings`` ([N, D] per chunk, or [F, D] per file with ``--pooling avg|max``), ``file_index``, ``start_s``, ``paths``,
``chunks_per_file``; with ``--dtype int8`` also ``scale`` and ``zero_point`` (float value = (q - zero_point) * scale).
"""

from __future__ import annotations

import argparse
import os


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Write the embeddings (pooled features in front of the classifier) of audio files to an .npz file.")
    p.add_argument("--model_path", type=str, required=True, help="Path to .keras or .tflite model")
    p.add_argument("--model_config", type=str, default="", help="Path to model config JSON (default: <model>_model_config.json)")
    p.add_argument("--input", type=str, nargs="+", required=True, help="Audio files and/or directories (walked recursively)")
    p.add_argument("--output", type=str, required=True, help="Output .npz path")
    p.add_argument("--pooling", type=str, default="none", choices=["none", "avg", "max"], help="Per chunk (none) or one row per file")
    p.add_argument("--dtype", type=str, default="float32", choices=["float32", "int8"], help="int8: the raw bytes of an INT8 model")
    p.add_argument("--overlap", type=float, default=0.0, help="Chunk overlap (seconds)")
    p.add_argument("--max_duration", type=float, default=60, help="Seconds read from the start of each file")
    p.add_argument("--max_chunks_per_file", type=int, default=0,
                   help="Keep only each file's N most active chunks (long files are cropped around their loudest stretches first); 0 = off, every "
                        "chunk is used.  Needs --overlap 0.  The reference's `train` defaults to 3")
    p.add_argument("--activity_threshold", type=float, default=0.1, help="With --max_chunks_per_file: drop chunks whose activity ratio is lower (one per file is always kept)")
    p.add_argument("--candidate_chunks", type=int, default=0, help="With --max_chunks_per_file: chunks ranked per file (0 = min(8, max(4, 2 N)), as the reference)")
    p.add_argument("--max_batch", type=int, default=4096, help="Workspace size in chunks = inference slice of the device pipeline")
    p.add_argument("--device", type=int, default=0, help="MI355X index")
    p.add_argument("--skip_undecodable", action="store_true", default=False,
                   help="Embed the decodable files when the input holds containers this build cannot read (Ogg / MP3 / M4A without soundfile) instead of refusing")
    return p


def collect_inputs(inputs: list[str]) -> list[str]:
    """Files as given, directories walked recursively (sorted) for the supported audio extensions."""
    from birdnet_stm32.data.dataset import SUPPORTED_AUDIO_EXTS

    exts = tuple(e.lower() for e in SUPPORTED_AUDIO_EXTS)
    out: list[str] = []
    for item in inputs:
        if os.path.isdir(item):
            for root, dirs, files in os.walk(item):
                dirs.sort()
                out.extend(os.path.join(root, f) for f in sorted(files) if f.lower().endswith(exts))
        elif os.path.isfile(item):
            out.append(item)
        else:
            raise FileNotFoundError(f"input not found: {item}")
    return out


def main(argv=None, runner=None):
    from birdnet_stm32.audio.io import have_soundfile
    from birdnet_stm32.cli.evaluate import resolve_config_path
    from birdnet_stm32.audio.pipeline import selection_from_args
    from birdnet_stm32.evaluation.embeddings import embed_files, save_embeddings_npz
    from birdnet_stm32.models.frontend import normalize_frontend_name
    from birdnet_stm32.training.config import ModelConfig

    args = build_parser().parse_args(argv)
    try:
        select = selection_from_args(args)
    except ValueError as exc:
        raise SystemExit(f"error: {exc}") from None
    cfg = ModelConfig.load(resolve_config_path(args.model_path, args.model_config)).to_dict()
    files = collect_inputs(args.input)
    if not files:
        raise SystemExit(f"error: no audio files found in {' '.join(args.input)}")
    # the same decodability rule as `evaluate`: RIFF/WAVE and FLAC natively, other containers only through soundfile
    foreign: dict[str, int] = {}
    for path in files:
        ext = os.path.splitext(path)[1].lower()
        if ext not in (".wav", ".flac"):
            foreign[ext] = foreign.get(ext, 0) + 1
    if foreign and not have_soundfile():
        if not args.skip_undecodable:
            raise SystemExit("error: " + ", ".join(f"{n} x {e}" for e, n in sorted(foreign.items())) + f" of the {len(files)} input files cannot be "
                             "decoded: only RIFF/WAVE and FLAC are read natively and the `soundfile` package is not installed.  Convert them, install "
                             "soundfile, or pass --skip_undecodable to embed the remaining files")
        files = [p for p in files if os.path.splitext(p)[1].lower() in (".wav", ".flac")]
    if runner is None:
        from birdnet_stm32.models.runners import load_model_runner

        runner = load_model_runner(args.model_path, device=args.device, max_batch=args.max_batch, prepare_pipeline=True)
    frontend = normalize_frontend_name(cfg["audio_frontend"])
    if frontend not in ("hybrid", "raw"):
        runner.configure_precomputed(frontend, int(cfg["sample_rate"]), cfg.get("mag_scale", "none"), int(cfg["fft_length"]), int(cfg["num_mels"]),
                                     int(cfg.get("n_mfcc", 20)))
    overlap = max(0.0, min(float(cfg["chunk_duration"]) - 0.1, args.overlap))
    try:
        res = embed_files(runner, files, chunk_overlap=overlap, max_duration=args.max_duration, pooling=args.pooling, dtype=args.dtype,
                          sample_rate=int(cfg["sample_rate"]), chunk_duration=float(cfg["chunk_duration"]), select=select)
    except ValueError as exc:
        if select is None:
            raise
        raise SystemExit(f"error: {exc}") from None
    save_embeddings_npz(args.output, res)
    print(f"Embedded {len(files) - len(res.skipped)} files: {res.embeddings.shape[0]} rows x {res.embeddings.shape[1]} ({res.dtype}, pooling {res.pooling}) -> {args.output}")
    if select is not None:
        print(f"Selection kept {res.embeddings.shape[0] if res.pooling == 'none' else int(res.chunks_per_file.sum())} of {res.candidate_rows} candidate chunks")
    if res.skipped:
        print(f"Skipped {len(res.skipped)} unreadable or empty files:")
        for p in res.skipped:
            print(f"  {p}")
    return res


if __name__ == "__main__":
    main()
