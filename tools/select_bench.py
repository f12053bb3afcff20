"""Cost of chunk selection: the evaluate pipeline with embeddings on N synthetic 30 s recordings, with and without
``ChunkSelection``, alternating and repeated (medians), how the selecting run's time splits (``last_run.select``: wall seconds of the
energy step, the host crop, the feature step and the host ranking; inside the two device steps ``ste_kernel_s``, ``cut_kernel_s``,
``stft_kernel_s`` and ``count_kernel_s`` from HIP events, the rest of each step being ``round_trip1_s`` / ``round_trip2_s``: launches, table
uploads, the wait and the copy to the host), and both kernels' HBM rate from HIP events.

    python tools/select_bench.py [--files 1024] [--seconds 30] [--repeats 5] [--dir /dev/shm/select_bench] [--max_chunks 3]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import wave

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "birdnet-stm32_amd")]


def make_files(d: str, n: int, seconds: float, sr: int) -> list[str]:
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(0)
    base = (rng.standard_normal(int(sr * seconds)) * 30).astype(np.int16)
    paths = []
    for i in range(n):
        p = os.path.join(d, f"f{i:05d}.wav")
        if not os.path.isfile(p):
            x = base.copy()
            for _ in range(3):   # three bursts of 1-2 s at file-specific places
                a, m = int(rng.integers(0, x.size - 2 * sr)), int(rng.integers(sr, 2 * sr))
                x[a : a + m] += (rng.standard_normal(m) * 6000 * np.hanning(m)).astype(np.int16)
            with wave.open(p, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(sr)
                w.writeframes(x.tobytes())
        paths.append(p)
    return paths


def kernel_rates(torch, ctx) -> dict:
    from birdnet_stm32 import _hip
    from birdnet_stm32.audio.activity import subsample_indices

    out = {}
    B, n = 4096, 65792
    x = torch.rand((B, n), device="cuda")
    idx = torch.from_numpy(subsample_indices(n).astype(np.int32)).cuda()
    act = torch.empty(B, dtype=torch.int32, device="cuda")
    run = lambda: _hip.check(ctx.lib.bn_activity_counts(ctx.handle, x.data_ptr(), B, n, idx.data_ptr(), 512, 2.0, act.data_ptr(), None, None))  # noqa: E731
    out["activity_count_kernel"] = _time(torch, run, B * n * 4)
    nw, ln = 1024, 30 * 22050
    mono = torch.rand(nw * ln, device="cuda")
    peak = torch.ones(nw, device="cuda")
    off = torch.arange(nw + 1, dtype=torch.int64, device="cuda") * ln
    nf = 1 + (ln - 1024) // 512
    fo = torch.arange(nw + 1, dtype=torch.int64, device="cuda") * nf
    wi = torch.arange(nw, dtype=torch.int32, device="cuda")
    ste = torch.empty(nw * nf, device="cuda")
    run = lambda: _hip.check(ctx.lib.bn_short_time_energy(ctx.handle, mono.data_ptr(), peak.data_ptr(), off.data_ptr(), wi.data_ptr(), fo.data_ptr(), nw,  # noqa: E731
                                                          1024, 512, ste.data_ptr(), None))
    out["ste_kernel"] = _time(torch, run, nw * ln * 4)
    return out


def _time(torch, run, nbytes: int, reps: int = 20) -> dict:
    for _ in range(3):
        run()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "read_TBps": round(nbytes / (med * 1e-3) / 1e12, 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default="/dev/shm/select_bench")
    ap.add_argument("--max_chunks", type=int, default=3)
    args = ap.parse_args()
    import torch

    from birdnet_stm32.audio.pipeline import ChunkSelection, EvaluatePipeline, plan_files
    from birdnet_stm32.models.runners import load_model_runner

    sr, cd = 22050, 3.0
    paths = make_files(args.dir, args.files, args.seconds, sr)
    runner = load_model_runner(os.path.join(REPO, "birdnet-stm32_amd", "checkpoints", "birdnet_stm32n6_100.tflite"), max_batch=4096)
    tab = plan_files(paths, sr, cd, 0.0, 60)
    walls, last = {"plain": [], "select": []}, {}
    for rep in range(args.repeats + 1):   # (the first pair warms up and is dropped)
        for name, sel in (("plain", None), ("select", ChunkSelection(args.max_chunks))):
            pipe = EvaluatePipeline(runner, sr, cd, 0.0, max_duration=60, select=sel)
            pipe.emb_dtype = "float32"
            _scores, counts, stats, _ = pipe.run(paths, table=tab)
            pipe.close()
            if rep:
                walls[name].append(stats["wall_s"])
            last[name] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in stats.items() if k in ("wall_s", "read_s", "h2d_s", "ingest_s", "infer_s", "chunks", "groups")}
            if "select" in stats:
                last[name]["select"] = {k: (round(v, 5) if isinstance(v, float) else v) for k, v in stats["select"].items()}
    res = {"files": args.files, "seconds": args.seconds, "repeats": args.repeats,
           "wall_s_median": {k: round(statistics.median(v), 4) for k, v in walls.items()}, "wall_s_all": {k: [round(x, 4) for x in v] for k, v in walls.items()},
           "last_run": last, "kernels": kernel_rates(torch, runner.ctx)}
    print(json.dumps(res))
    runner.close()


if __name__ == "__main__":
    main()
