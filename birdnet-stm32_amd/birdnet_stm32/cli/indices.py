"""``birdnet-stm32 indices`` — how complex, how even, how biological, how busy is each minute of these recordings: acoustic indices on the GPU.

No model is involved.  ``--input`` takes files and directories (walked recursively, as in ``embed``); files are read whole by default
(``--max_duration 0``), resampled to ``--sample_rate``, peak-normalised and cut into chunks of ``--chunk_duration`` seconds on the device,
hour-long files streamed (``evaluation/indices.py``: the definitions, and where they depart from soundecology and scikit-maad).
``--model_config`` takes the three numbers from a model's config JSON instead, so the chunks are the ones ``analyze`` scores.

    <output>          file, start_s, end_s, chunks, aci, hf, ht, h, ndsi, bi, adi, aei     one line per window of --window_s seconds
    --spectral_out    npz: aci, ent, cvr [windows, 257] float32, file_index, start_s, freqs_hz [257], paths
    --ldfc_png        a false-colour long-duration spectrogram per input file (MAP_<n>.png when there are several): one column per
                      window, frequency upwards, R, G, B = ACI_f, ENT_f, CVR_f scaled between LDFC_BOUNDS

A line is the MEAN of the chunks whose start falls into the window (per-chunk indices averaged, not indices of the whole minute);
``--window_s 0`` writes one line per chunk.  Every index is unchanged when a recording is made louder or quieter.
"""

from __future__ import annotations

import argparse
import csv
import json
import math
import os
import struct
import zlib

CSV_COLUMNS = ("file", "start_s", "end_s", "chunks", "aci", "hf", "ht", "h", "ndsi", "bi", "adi", "aei")   # evaluation/indices.py: INDEX_COLUMNS
# The fixed bounds a false-colour channel is scaled between, (value shown as 0, value shown as 255): ACI_f and ENT_f as Towsey (2014)
# normalises them for long-duration spectrograms; CVR_f is a share of frames and takes its whole range.
LDFC_BOUNDS = {"aci": (0.4, 0.7), "ent": (0.0, 0.6), "cvr": (0.0, 1.0)}


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Acoustic indices (ACI, entropies, NDSI, BI, ADI, AEI) of audio files, per window, computed on the GPU.")
    p.add_argument("--input", type=str, nargs="+", required=True, help="Audio files and/or directories (walked recursively)")
    p.add_argument("--output", type=str, required=True, help="Output CSV path (one line per window)")
    p.add_argument("--window_s", type=float, default=60.0, help="Seconds per output line: the mean of the chunks starting in it (0: one line per chunk)")
    p.add_argument("--sample_rate", type=int, default=22050, help="Rate the files are resampled to")
    p.add_argument("--chunk_duration", type=float, default=3.0, help="Seconds per chunk")
    p.add_argument("--spec_width", type=int, default=256, help="STFT frames per chunk")
    p.add_argument("--model_config", type=str, default="", help="Take sample_rate, chunk_duration and spec_width from a model config JSON")
    p.add_argument("--overlap", type=float, default=0.0, help="Chunk overlap (seconds)")
    p.add_argument("--max_duration", type=float, default=0, help="Seconds read from the start of each file (0: the whole file)")
    p.add_argument("--anthro", type=float, nargs=2, default=[1000.0, 2000.0], metavar=("LO", "HI"), help="Anthrophony band of NDSI (Hz)")
    p.add_argument("--bio", type=float, nargs=2, default=[2000.0, 8000.0], metavar=("LO", "HI"), help="Biophony band of NDSI and BI (Hz)")
    p.add_argument("--db_threshold", type=float, default=-50.0, help="Cover threshold of ADI / AEI / CVR in dB below the chunk's maximum")
    p.add_argument("--band_hz", type=float, default=1000.0, help="Width of the ADI / AEI bands (Hz)")
    p.add_argument("--max_hz", type=float, default=10000.0, help="Upper end of the ADI / AEI bands (Hz)")
    p.add_argument("--spectral_out", type=str, default="", help="Write the per-bin indices per window as an npz as well")
    p.add_argument("--ldfc_png", type=str, default="", help="Write a false-colour long-duration spectrogram per input file")
    p.add_argument("--device", type=int, default=0, help="MI355X index")
    p.add_argument("--max_batch", type=int, default=4096, help="Chunks per STFT + indices launch")
    return p


def resolve_args(args):
    """``(sample_rate, chunk_duration, spec_width, overlap, IndexParams)`` of parsed arguments; everything that can be refused before a
    file is read raises ``ValueError``."""
    from birdnet_stm32.evaluation.indices import MAX_WIDTH, MIN_WIDTH, IndexParams

    sr, cd, width = args.sample_rate, args.chunk_duration, args.spec_width
    if args.model_config:
        if not os.path.isfile(args.model_config):
            raise ValueError(f"model config not found: {args.model_config}")
        with open(args.model_config) as f:
            cfg = json.load(f)
        try:
            sr, cd, width = int(cfg["sample_rate"]), float(cfg["chunk_duration"]), int(cfg["spec_width"])
        except (KeyError, TypeError, ValueError) as exc:
            raise ValueError(f"{args.model_config}: sample_rate, chunk_duration and spec_width are needed ({exc})") from None
    if sr < 1:
        raise ValueError(f"--sample_rate {sr} must be positive")
    if not (math.isfinite(cd) and cd > 0.0):
        raise ValueError(f"--chunk_duration {cd} must be positive")
    if not MIN_WIDTH <= width <= MAX_WIDTH:
        raise ValueError(f"--spec_width {width} must be {MIN_WIDTH} .. {MAX_WIDTH}")
    if int(sr * cd) // width < 1:
        raise ValueError(f"chunks of {int(sr * cd)} samples are too short for {width} frames")
    if not (math.isfinite(args.window_s) and args.window_s >= 0.0):
        raise ValueError(f"--window_s {args.window_s} must be >= 0")
    if not (math.isfinite(args.overlap) and 0.0 <= args.overlap < cd):
        raise ValueError(f"--overlap {args.overlap} must be >= 0 and shorter than a chunk")
    if not (math.isfinite(args.max_duration) and args.max_duration >= 0.0):
        raise ValueError(f"--max_duration {args.max_duration} must be >= 0")
    if args.max_batch < 1:
        raise ValueError(f"--max_batch {args.max_batch} must be >= 1")
    params = IndexParams(tuple(args.anthro), tuple(args.bio), args.db_threshold, args.band_hz, args.max_hz).validate(sr)
    return sr, cd, width, args.overlap, params


def _fmt(v: float) -> str:
    return f"{float(v):.7g}"


def write_indices_csv(path: str, table, paths: list) -> int:
    """One line per row of an ``IndexTable`` whose values start with the eight scalars (``CSV_COLUMNS``).  Returns the number of lines."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS)
        for i in range(len(table)):
            w.writerow([paths[int(table.file_index[i])], f"{table.start_s[i]:.3f}", f"{table.end_s[i]:.3f}", int(table.chunks[i])]
                       + [_fmt(v) for v in table.values[i, : len(CSV_COLUMNS) - 4]])
    return len(table)


def write_spectral_npz(path: str, table, paths: list, sample_rate: int) -> None:
    """``aci``, ``ent``, ``cvr`` ``[windows, 257]`` float32 of an ``IndexTable`` whose values hold the per-bin block behind the scalars."""
    import numpy as np

    from birdnet_stm32.evaluation.indices import N_BINS, N_SCALARS, SPECTRAL_COLUMNS, bin_frequencies

    bins = np.asarray(table.values[:, N_SCALARS:], np.float32).reshape(len(table), len(SPECTRAL_COLUMNS), N_BINS)
    np.savez(path, **{name: np.ascontiguousarray(bins[:, i]) for i, name in enumerate(SPECTRAL_COLUMNS)},
             file_index=np.asarray(table.file_index, np.int64), start_s=np.asarray(table.start_s, np.float64),
             freqs_hz=bin_frequencies(sample_rate), paths=np.array([str(p) for p in paths]))


def encode_png(rgb) -> bytes:
    """An 8-bit RGB PNG of ``rgb [H, W, 3]`` uint8 (row 0 on top), with the standard library's zlib and struct only."""
    import numpy as np

    a = np.ascontiguousarray(np.asarray(rgb, np.uint8))
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("rgb must be [H, W, 3] with H, W >= 1")
    h, w = a.shape[:2]
    raw = b"".join(b"\x00" + a[y].tobytes() for y in range(h))   # filter type 0 in front of every scanline

    def chunk(kind: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 9))
            + chunk(b"IEND", b""))


def ldfc_image(aci, ent, cvr):
    """The false-colour map ``[257, windows, 3]`` uint8 of per-window per-bin indices ``[windows, 257]``: time along x, frequency upwards
    (bin 256 is the top row), R, G, B = ACI_f, ENT_f, CVR_f, each ``round(255 * clip((v - lo) / (hi - lo), 0, 1))`` over ``LDFC_BOUNDS``."""
    import numpy as np

    planes = []
    for name, v in (("aci", aci), ("ent", ent), ("cvr", cvr)):
        lo, hi = LDFC_BOUNDS[name]
        x = np.clip((np.asarray(v, np.float64) - lo) / (hi - lo), 0.0, 1.0)
        planes.append(np.rint(255.0 * x).astype(np.uint8).T[::-1])
    return np.stack(planes, axis=-1)


def ldfc_paths(path: str, n_files: int) -> list[str]:
    """Where the map of each input file goes: ``path`` itself for one file, ``<stem>_<n><ext>`` for several."""
    if n_files == 1:
        return [path]
    stem, ext = os.path.splitext(path)
    return [f"{stem}_{i}{ext or '.png'}" for i in range(n_files)]


def write_ldfc(path: str, table, n_files: int) -> list[str]:
    """One PNG per input file that has a window.  Returns the files written."""
    import numpy as np

    from birdnet_stm32.evaluation.indices import N_BINS, N_SCALARS, SPECTRAL_COLUMNS

    bins = np.asarray(table.values[:, N_SCALARS:], np.float64).reshape(len(table), len(SPECTRAL_COLUMNS), N_BINS)
    written = []
    for i, out in enumerate(ldfc_paths(path, n_files)):
        rows = np.flatnonzero(table.file_index == i)
        if rows.size == 0:
            continue
        with open(out, "wb") as f:
            f.write(encode_png(ldfc_image(bins[rows, 0], bins[rows, 1], bins[rows, 2])))
        written.append(out)
    return written


def main(argv=None):
    args = build_parser().parse_args(argv)
    from birdnet_stm32.cli.embed import collect_inputs

    try:
        sr, cd, width, overlap, params = resolve_args(args)
        files = collect_inputs(args.input)
        if not files:
            raise ValueError(f"no audio files found in {' '.join(args.input)}")
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"error: {exc}") from None
    import numpy as np

    from birdnet_stm32.evaluation.indices import aggregate, indices_files

    spectral = bool(args.spectral_out or args.ldfc_png)
    try:
        res = indices_files(files, sr, cd, width, overlap, args.max_duration, spectral, params, args.device, args.max_batch)
    except ValueError as exc:
        raise SystemExit(f"error: {exc}") from None
    rows = res.scalars if not spectral else np.concatenate([res.scalars, res.spectral.reshape(len(res), -1)], axis=1)
    table = aggregate(rows, res.chunk_file, res.chunk_start_s, args.window_s, res.chunk_end_s)
    write_indices_csv(args.output, table, files)
    outs = [args.output]
    if args.spectral_out:
        write_spectral_npz(args.spectral_out, table, files, sr)
        outs.append(args.spectral_out)
    if args.ldfc_png:
        outs += write_ldfc(args.ldfc_png, table, len(files))
    hours = float(res.duration_s.sum()) / 3600.0
    print(f"Indices of {len(files) - len(res.skipped)} files ({hours:.2f} h, {len(res)} chunks) in {len(table)} windows -> " + ", ".join(outs))
    if res.skipped:
        print(f"Skipped {len(res.skipped)} unreadable or empty files:")
        for p in res.skipped:
            print(f"  {p}")
    return table


if __name__ == "__main__":
    main()
