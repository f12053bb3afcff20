"""Chunks per second of the acoustic indices on resident chunks: ``bn_stft_mag(normalize = 0)`` + ``bn_acoustic_indices``, and each alone.

    python tools/indices_bench.py [--chunks 4096] [--spec_width 256] [--reps 20] [--out indices_bench.json]

``--chunks`` chunks of 3 s at 22050 Hz lie on the device (white noise under two tones, peak 1, as the ingest leaves them).  Every figure
is the median over ``--reps`` launches, each between two HIP events behind three warm-up launches, all in this process:
  stft       one ``bn_stft_mag(normalize = 0)`` launch: the yardstick the issue names ("the indices should cost no more than that");
  indices    one ``bn_acoustic_indices`` launch over the spectrograms that launch left, with and without the per-bin block;
  both       the two behind each other, as ``indices_files`` issues them per slice.
The indices kernel reads every magnitude once: ``chunks * 257 * W * 4`` bytes, reported over its time as GB/s — the algorithm's traffic,
whichever cache served it (4096 chunks are 1.08 GB, four times the 256 MiB last-level cache).  Nothing here is a threshold.  Prints one
JSON line.
"""

import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "birdnet-stm32_amd")]


def timed(torch, run, reps: int) -> float:
    """Median seconds of ``run()`` between two events, behind three warm-up calls."""
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms) * 1e-3


def main():
    import torch

    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation import indices as IX

    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--spec_width", type=int, default=256)
    ap.add_argument("--sample_rate", type=int, default=22050)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("error: this benchmark measures the GPU path and no device is available")
    B, W, sr = args.chunks, args.spec_width, args.sample_rate
    T = sr * 3
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    t = torch.arange(T, device=dev, dtype=torch.float32) / sr
    audio = 0.3 * torch.randn((B, T), generator=gen, device=dev)
    audio += torch.sin(2 * torch.pi * 3000.0 * t) + 0.5 * torch.sin(2 * torch.pi * 1500.0 * t)
    audio /= audio.abs().amax(dim=1, keepdim=True)
    ctx = _hip.Context(0, B)
    lib, h = ctx.lib, ctx.handle
    spec = torch.empty((B, IX.N_BINS, W), dtype=torch.float32, device=dev)
    minmax = torch.empty((B, 2), dtype=torch.float32, device=dev)
    out = torch.empty((B, IX.N_SCALARS), dtype=torch.float32, device=dev)
    bins = torch.empty((B, 3, IX.N_BINS), dtype=torch.float32, device=dev)
    dp = IX.device_params(IX.IndexParams(), sr)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def stft():
        _hip.check(lib.bn_stft_mag(h, audio.data_ptr(), B, T, IX.N_FFT, T // W, W, 0, spec.data_ptr(), minmax.data_ptr(), stream))

    def indices(spectral=True):
        _hip.check(lib.bn_acoustic_indices(h, spec.data_ptr(), minmax.data_ptr(), B, IX.N_BINS, W, ctypes.byref(dp), out.data_ptr(),
                                           bins.data_ptr() if spectral else None, stream))

    def both():
        stft()
        indices()

    t_stft = timed(torch, stft, args.reps)
    t_idx = timed(torch, indices, args.reps)
    t_idx_scalars = timed(torch, lambda: indices(False), args.reps)
    t_both = timed(torch, both, args.reps)
    nbytes = B * IX.N_BINS * W * 4
    mean = out.double().mean(dim=0).cpu().tolist()
    res = {
        "what": "indices_bench", "chunks": B, "spec_width": W, "sample_rate": sr, "reps": args.reps, "device": torch.cuda.get_device_name(0),
        "stft_ms": round(t_stft * 1e3, 4), "indices_ms": round(t_idx * 1e3, 4), "indices_scalars_only_ms": round(t_idx_scalars * 1e3, 4),
        "stft_plus_indices_ms": round(t_both * 1e3, 4),
        "stft_chunks_per_s": round(B / t_stft), "indices_chunks_per_s": round(B / t_idx), "stft_plus_indices_chunks_per_s": round(B / t_both),
        "indices_over_stft": round(t_idx / t_stft, 3), "indices_bytes_read": nbytes, "indices_read_gb_per_s": round(nbytes / t_idx / 1e9, 1),
        "audio_hours_per_s": round(B * 3.0 / 3600.0 / t_both, 1),
        "mean_indices": {name: round(v, 6) for name, v in zip(IX.INDEX_COLUMNS, mean)},
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
