#!/usr/bin/env python3
"""Cost of the embedding output, measured with the variants alternating in one process.

    python tools/embed_bench.py [--batch 4096] [--rounds 12] [--steps 10] [--files 1024] [--seconds 30] [--dtype i8]

1. **Step**: ``infer_audio_device`` on ``--batch`` synthetic chunks, scores only vs scores + float32 embeddings (preallocated outputs),
   ``--rounds`` rounds of ``--steps`` steps each per variant, alternating; median and spread of the per-step time of each.
2. **Files**: ``evaluate`` (the ``tools/evaluate_bench.py`` data set: PCM16 WAVs on tmpfs) against ``embed_files`` on the same files,
   warm calls alternating; chunks per second of each and their ratio.

One JSON object on stdout (the last line); progress on stderr.
"""

from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "birdnet-stm32_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def step_bench(torch, runner, batch: int, rounds: int, steps: int) -> dict:
    dev = runner.device
    T = 72000
    g = torch.Generator(device=dev).manual_seed(0)
    audio = (0.1 * torch.randn((batch, T), generator=g, device=dev)).contiguous()
    scores = torch.empty((batch, runner.num_classes), dtype=torch.float32, device=dev)
    emb = torch.empty((batch, runner.embedding_info()["dim"]), dtype=torch.float32, device=dev)

    def run(with_emb: bool) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            if with_emb:
                runner.infer_audio_device(audio, out=scores, return_embeddings=True, emb_out=emb)
            else:
                runner.infer_audio_device(audio, out=scores)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / steps

    for v in (False, True, False, True):   # warm-up: code objects, LDS limits
        run(v)
    t = {False: [], True: []}
    for r in range(rounds):
        for v in ((False, True) if r % 2 == 0 else (True, False)):
            t[v].append(run(v))
    base, withe = statistics.median(t[False]), statistics.median(t[True])
    out = {"batch": batch, "rounds": rounds, "steps_per_round": steps,
           "scores_only_ms": {"median": round(base, 4), "min": round(min(t[False]), 4), "max": round(max(t[False]), 4)},
           "scores_plus_f32_emb_ms": {"median": round(withe, 4), "min": round(min(t[True]), 4), "max": round(max(t[True]), 4)},
           "ratio_median": round(withe / base, 4),
           "chunks_per_s_scores_only": round(batch / base * 1e3), "chunks_per_s_with_emb": round(batch / withe * 1e3)}
    log(json.dumps(out))
    return out


def files_bench(torch, runner, args) -> dict:
    from evaluate_bench import write_dataset

    from birdnet_stm32.evaluation.embeddings import embed_files
    from birdnet_stm32.evaluation.metrics import evaluate
    from birdnet_stm32.training.config import ModelConfig

    ckpt = os.path.join(REPO, "birdnet-stm32_amd", "checkpoints", "birdnet_stm32n6_100")
    cfg = ModelConfig.load(ckpt + "_model_config.json").to_dict()
    cfg.update(sample_rate=24000, hop_length=281)   # (as tools/evaluate_bench.py)
    classes = cfg["class_names"]
    paths, gen_s = write_dataset(args.dir, args.files, args.seconds, args.channels, args.sr, classes[:8], torch)
    log(f"{len(paths)} files written in {gen_s:.1f} s")
    try:
        ev_t, em_t = [], []
        chunks = None
        for r in range(args.repeats + 1):   # the first round is the cold call of each: not counted
            for kind in (("evaluate", "embed") if r % 2 == 0 else ("embed", "evaluate")):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if kind == "evaluate":
                    evaluate(runner, paths, classes, cfg, pooling="avg", batch_size=16)
                else:
                    res = embed_files(runner, paths, sample_rate=cfg["sample_rate"], chunk_duration=float(cfg["chunk_duration"]))
                    chunks = res.embeddings.shape[0]
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if r:
                    (ev_t if kind == "evaluate" else em_t).append(dt)
                log(f"round {r} {kind}: {dt:.3f} s")
    finally:
        shutil.rmtree(args.dir, ignore_errors=True)
    ev, em = statistics.median(ev_t), statistics.median(em_t)
    return {"files": len(paths), "seconds_per_file": args.seconds, "chunks": chunks, "evaluate_chunks_per_s": round(chunks / ev),
            "embed_files_chunks_per_s": round(chunks / em), "embed_over_evaluate": round(ev / em, 4),
            "evaluate_s": [round(x, 3) for x in ev_t], "embed_files_s": [round(x, 3) for x in em_t]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dtype", choices=["i8", "f32"], default="i8")
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--sr", type=int, default=24000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm/bn_embed_bench")
    ap.add_argument("--no_files", action="store_true", help="only the step measurement")
    args = ap.parse_args()
    import torch

    from birdnet_stm32.models.runners import load_model_runner

    ckpt = os.path.join(REPO, "birdnet-stm32_amd", "checkpoints", "birdnet_stm32n6_100")
    runner = load_model_runner(ckpt + (".tflite" if args.dtype == "i8" else ".keras"), max_batch=args.batch, prepare_pipeline=True)
    out = {"model": args.dtype, "step": step_bench(torch, runner, args.batch, args.rounds, args.steps)}
    if not args.no_files:
        out["files"] = files_bench(torch, runner, args)
    runner.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
