#!/usr/bin/env python3
"""Throughput of ``analyze``'s streamed path against the grouped ``evaluate`` pipeline on the same audio.

    python tools/analyze_bench.py [--hours 2] [--sr 48000] [--repeats 3] [--dir /dev/shm/bn_analyze_bench]

Writes ``--hours`` 1-hour mono PCM16 WAVs at ``--sr`` (tone sweeps + noise, distinct per file) and the same audio cut into 60 s
files, both on tmpfs.  Then, alternating, times

* **stream**: ``EvaluatePipeline(stream_long=True, max_duration=0)`` over the 1-hour files — every file is streamed segment by
  segment (``bn_ingest_resample_span``), its chunks cut behind the last segment and scored in slices;
* **grouped**: ``EvaluatePipeline(max_duration=60)`` over the 60 s files — the path ``evaluate`` runs.

For each: audio-hours/s, chunks/s, WAV GB/s (payload bytes over wall time) and the stage split (busy time of read, H2D,
resample + chunk cut, inference; the stages overlap).  One JSON object on stdout (the last line); progress on stderr.
"""

from __future__ import annotations

import argparse
import json
import os
import shutil
import struct
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "birdnet-stm32_amd"))

import numpy as np  # noqa: E402


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def _wav(path: str, pcm: np.ndarray, sr: int) -> None:
    payload = pcm.astype("<i2").tobytes()
    hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(payload), b"WAVE", b"fmt ", 16, 1, 1, sr, sr * 2, 2, 16, b"data", len(payload))
    with open(path, "wb") as fh:
        fh.write(hdr)
        fh.write(payload)


def write_audio(root: str, hours: int, sr: int) -> tuple[list[str], list[str], int]:
    """``hours`` 1-hour files and the same samples as 60 s files; returns (long paths, short paths, payload bytes of each set)."""
    os.makedirs(os.path.join(root, "long"), exist_ok=True)
    os.makedirs(os.path.join(root, "short"), exist_ok=True)
    long_paths, short_paths = [], []
    n = 3600 * sr
    for h in range(hours):
        rng = np.random.default_rng(h)
        t = np.arange(n, dtype=np.float32) / np.float32(sr)
        f = np.float32(1500 + 400 * h) + np.float32(1000) * np.sin(np.float32(2 * np.pi / 7.0) * t)
        x = np.float32(0.3) * np.sin(np.float32(2 * np.pi) * f * t) + np.float32(0.05) * rng.standard_normal(n, dtype=np.float32)
        pcm = np.clip(np.rint(x * 32767), -32768, 32767).astype(np.int16)
        p = os.path.join(root, "long", f"rec_{h:02d}.wav")
        _wav(p, pcm, sr)
        long_paths.append(p)
        for m in range(60):
            q = os.path.join(root, "short", f"rec_{h:02d}_{m:02d}.wav")
            _wav(q, pcm[m * 60 * sr : (m + 1) * 60 * sr], sr)
            short_paths.append(q)
        log(f"wrote hour {h + 1}/{hours}")
    return long_paths, short_paths, hours * n * 2


def run_once(pipe, paths, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scores, counts, stats, _ = pipe.run(paths)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return scores, counts, stats, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=int, default=2)
    ap.add_argument("--sr", type=int, default=48000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max_batch", type=int, default=4096)
    ap.add_argument("--dir", type=str, default="/dev/shm/bn_analyze_bench")
    ap.add_argument("--keep", action="store_true")
    args = ap.parse_args()

    import torch

    from birdnet_stm32.audio.pipeline import EvaluatePipeline
    from birdnet_stm32.models.runners import load_model_runner

    if not torch.cuda.is_available():
        raise SystemExit("analyze_bench needs a GPU")
    ckpt = os.path.join(REPO, "birdnet-stm32_amd", "checkpoints", "birdnet_stm32n6_100.tflite")
    sr_out, cd = 22050, 3.0
    try:
        long_paths, short_paths, nbytes = write_audio(args.dir, args.hours, args.sr)
        runner = load_model_runner(ckpt, max_batch=args.max_batch, prepare_pipeline=True)
        legs = {
            "stream": (EvaluatePipeline(runner, sr_out, cd, 0.0, max_duration=0, stream_long=True), long_paths),
            "grouped": (EvaluatePipeline(runner, sr_out, cd, 0.0, max_duration=60), short_paths),
        }
        for name, (pipe, paths) in legs.items():   # warm-up: code objects, slabs, buffers
            run_once(pipe, paths, torch)
        results = {k: [] for k in legs}
        for r in range(args.repeats):
            for name, (pipe, paths) in legs.items():
                _s, counts, st, wall = run_once(pipe, paths, torch)
                chunks = int(sum(counts))
                row = dict(wall_s=round(wall, 4), audio_hours_per_s=round(args.hours / wall, 3), chunks_per_s=round(chunks / wall, 1),
                           wav_gbps=round(nbytes / wall / 1e9, 3), chunks=chunks, read_s=round(st["read_s"], 4), h2d_s=round(st["h2d_s"], 4),
                           resample_s=round(st["ingest_s"], 4), infer_s=round(st["infer_s"], 4), streamed=st.get("streamed", 0), groups=st["groups"])
                results[name].append(row)
                log(name, r, row)
        for pipe, _ in legs.values():
            pipe.close()
        runner.close()
        best = {k: max(v, key=lambda x: x["wav_gbps"]) for k, v in results.items()}
        out = dict(hours=args.hours, sr=args.sr, wav_bytes=nbytes, best=best, runs=results,
                   stream_over_grouped=round(best["stream"]["wav_gbps"] / best["grouped"]["wav_gbps"], 3))
        print(json.dumps(out))
    finally:
        if not args.keep:
            shutil.rmtree(args.dir, ignore_errors=True)


if __name__ == "__main__":
    main()
