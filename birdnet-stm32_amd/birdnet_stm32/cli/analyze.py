"""``birdnet-stm32 analyze`` — which classes are in these recordings, and when: per-chunk detections over whole files on the GPU.

``--input`` takes files and directories (walked recursively, as in ``embed``).  Files are analysed whole by default
(``--max_duration 0``); recordings longer than one staging slab are streamed through the device path segment by segment
(``evaluation/detections.py``).  The chunking follows the model's ``<model>_model_config.json``; class names come from its
``class_names`` ("Scientific name_Common name").  With ``--head`` (a head trained by ``probe``) the detections are of the head's classes:
it is applied on the device to the model's embeddings.

Outputs (``--format``, one or more):

* ``csv``: one table, ``file,start_s,end_s,scientific_name,common_name,class_index,confidence``;
* ``raven``: one tab-separated Raven selection table per input file, in a directory;
* ``npz``: the full per-chunk scores with ``file_index``, ``start_s``, ``paths``, ``chunks_per_file`` and ``class_names``.

With one format ``--output`` is that output (a file; a directory for raven); with several it is a directory that receives
``detections.csv``, ``detections.npz`` and the selection tables.
"""

from __future__ import annotations

import argparse
import json
import os

FORMATS = ("csv", "raven", "npz")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Detect the model's classes in audio files, per chunk, and write them as CSV, Raven tables or npz.")
    p.add_argument("--model_path", type=str, required=True, help="Path to .keras or .tflite model")
    p.add_argument("--model_config", type=str, default="", help="Path to model config JSON (default: <model>_model_config.json)")
    p.add_argument("--head", type=str, default="", help="A head trained by `probe` (<output>.npz): report its classes instead of the model's")
    p.add_argument("--input", type=str, nargs="+", required=True, help="Audio files and/or directories (walked recursively)")
    p.add_argument("--output", type=str, required=True, help="Output file (csv, npz), directory (raven, or several formats)")
    p.add_argument("--format", type=str, nargs="+", default=["csv"], choices=FORMATS, help="Output format(s)")
    p.add_argument("--min_conf", type=float, default=0.25, help="Score threshold of a detection")
    p.add_argument("--top_k", type=int, default=None, help="At most this many detections per chunk")
    p.add_argument("--thresholds", type=str, default="", help="Per-class thresholds: a JSON object (class name -> value) or a JSON file")
    p.add_argument("--overlap", type=float, default=0.0, help="Chunk overlap (seconds)")
    p.add_argument("--max_duration", type=float, default=0, help="Seconds read from the start of each file (0: the whole file)")
    p.add_argument("--merge_consecutive", action="store_true", default=False, help="Join a class's detections in consecutive chunks")
    p.add_argument("--max_batch", type=int, default=4096, help="Workspace size in chunks = inference slice of the device pipeline")
    p.add_argument("--device", type=int, default=0, help="MI355X index")
    p.add_argument("--skip_undecodable", action="store_true", default=False,
                   help="Analyse the decodable files when the input holds containers this build cannot read instead of refusing")
    return p


def load_thresholds(arg: str) -> dict | None:
    """``--thresholds``: a JSON object given inline or as a file path."""
    if not arg:
        return None
    text = open(arg).read() if os.path.isfile(arg) else arg
    val = json.loads(text)
    if not isinstance(val, dict):
        raise SystemExit("error: --thresholds must be a JSON object mapping class names to thresholds")
    return {str(k): float(v) for k, v in val.items()}


def output_paths(output: str, formats: list[str]) -> dict:
    """Where each format goes: ``output`` itself for a single format, fixed names inside the directory ``output`` for several."""
    formats = list(dict.fromkeys(formats))
    if len(formats) == 1:
        return {formats[0]: output}
    os.makedirs(output, exist_ok=True)
    names = {"csv": "detections.csv", "npz": "detections.npz", "raven": "raven"}
    return {f: os.path.join(output, names[f]) for f in formats}


def main(argv=None, runner=None):
    from birdnet_stm32.audio.io import have_soundfile
    from birdnet_stm32.cli.embed import collect_inputs
    from birdnet_stm32.cli.evaluate import resolve_config_path
    from birdnet_stm32.evaluation.detections import detect_files, write_csv, write_npz, write_raven
    from birdnet_stm32.models.frontend import normalize_frontend_name
    from birdnet_stm32.training.config import ModelConfig

    args = build_parser().parse_args(argv)
    cfg = ModelConfig.load(resolve_config_path(args.model_path, args.model_config)).to_dict()
    class_names = list(cfg.get("class_names") or [])
    head = None
    if args.head:
        from birdnet_stm32.training.linear_probe import ProbeHead

        if not os.path.isfile(args.head):
            raise SystemExit(f"error: head not found: {args.head}")
        head = ProbeHead.load(args.head)
        class_names = list(head.class_names)
    if not class_names:
        raise SystemExit("error: class_names missing in model config")
    thresholds = load_thresholds(args.thresholds)
    files = collect_inputs(args.input)
    if not files:
        raise SystemExit(f"error: no audio files found in {' '.join(args.input)}")
    foreign: dict[str, int] = {}
    for path in files:
        ext = os.path.splitext(path)[1].lower()
        if ext not in (".wav", ".flac"):
            foreign[ext] = foreign.get(ext, 0) + 1
    if foreign and not have_soundfile():
        if not args.skip_undecodable:
            raise SystemExit("error: " + ", ".join(f"{n} x {e}" for e, n in sorted(foreign.items())) + f" of the {len(files)} input files cannot be "
                             "decoded: only RIFF/WAVE and FLAC are read natively and the `soundfile` package is not installed.  Convert them, install "
                             "soundfile, or pass --skip_undecodable to analyse the remaining files")
        files = [p for p in files if os.path.splitext(p)[1].lower() in (".wav", ".flac")]
    if runner is None:
        from birdnet_stm32.models.runners import load_model_runner

        runner = load_model_runner(args.model_path, device=args.device, max_batch=args.max_batch, prepare_pipeline=True)
    if head is None and int(runner.num_classes) != len(class_names):
        raise SystemExit(f"error: the model scores {runner.num_classes} classes, its config names {len(class_names)}")
    frontend = normalize_frontend_name(cfg["audio_frontend"])
    if frontend not in ("hybrid", "raw"):
        runner.configure_precomputed(frontend, int(cfg["sample_rate"]), cfg.get("mag_scale", "none"), int(cfg["fft_length"]), int(cfg["num_mels"]),
                                     int(cfg.get("n_mfcc", 20)))
    overlap = max(0.0, min(float(cfg["chunk_duration"]) - 0.1, args.overlap))
    outs = output_paths(args.output, args.format)
    try:
        det = detect_files(runner, files, min_conf=args.min_conf, top_k=args.top_k, class_thresholds=thresholds, chunk_overlap=overlap,
                           max_duration=args.max_duration, merge_consecutive=args.merge_consecutive, sample_rate=int(cfg["sample_rate"]),
                           chunk_duration=float(cfg["chunk_duration"]), return_scores="npz" in outs, class_names=class_names, head=head)
    except ValueError as exc:
        raise SystemExit(f"error: {exc}") from None
    if "csv" in outs:
        write_csv(outs["csv"], det, class_names)
    if "raven" in outs:
        write_raven(outs["raven"], det, class_names)
    if "npz" in outs:
        write_npz(outs["npz"], det, class_names)
    hours = float(det.duration_s.sum()) / 3600.0
    print(f"Analysed {len(files) - len(det.skipped)} files ({hours:.2f} h, {int(det.chunks_per_file.sum())} chunks): {len(det)} detections -> "
          + ", ".join(f"{f} {p}" for f, p in outs.items()))
    if det.skipped:
        print(f"Skipped {len(det.skipped)} unreadable or empty files:")
        for p in det.skipped:
            print(f"  {p}")
    return det


if __name__ == "__main__":
    main()
