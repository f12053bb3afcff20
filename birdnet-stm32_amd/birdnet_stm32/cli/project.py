"""``birdnet-stm32 project`` — what does this archive look like?

The database is one or more ``.npz`` archives written by ``embed``.  Their rows are laid out on a 2-D map by exact t-SNE on the GPU
(``evaluation/project.py``: k-nearest-neighbour affinities, all-pairs repulsion, scikit-learn's constants) and written as one CSV file:

    <output>    path, start_s, end_s, x, y      one line per row in the archive's order (x and y empty: a zero row)

so it joins line by line with ``cluster``'s CSV.  ``end_s`` is ``start_s`` plus ``--chunk_duration`` (the archive does not record it; 0
leaves ``end_s = start_s``).  ``--npz_out`` writes the map as ``xy`` [N, 2] float32 (NaN for a zero row) with the archive's ``file_index``,
``start_s`` and ``paths``, the final divergence ``kl`` and the rows' ``beta``.
"""

from __future__ import annotations

import argparse
import csv
import math
import os

CSV_COLUMNS = ("path", "start_s", "end_s", "x", "y")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Lay the rows of archives written by `embed` out on a 2-D map (exact t-SNE on the GPU).")
    p.add_argument("--database", type=str, nargs="+", required=True, help="One or more .npz archives written by `embed`")
    p.add_argument("--output", type=str, required=True, help="Output CSV path (one line per row)")
    p.add_argument("--perplexity", type=float, default=30.0, help="Effective number of neighbours (1..42)")
    p.add_argument("--n_iter", type=int, default=1000, help="Iterations")
    p.add_argument("--early_exaggeration", type=float, default=12.0, help="Factor on the affinities during the first iterations")
    p.add_argument("--exaggeration_iter", type=int, default=250, help="Iterations with early exaggeration")
    p.add_argument("--learning_rate", type=float, default=None, help="Step size (default: max(rows / early_exaggeration / 4, 50))")
    p.add_argument("--seed", type=int, default=42, help="Seed of the initial map (--init random)")
    p.add_argument("--init", type=str, default="random", choices=("random", "pca"),
                   help="Initial map: a seeded Gaussian, or the first two principal components (scikit-learn's default: maps keep their global arrangement)")
    p.add_argument("--chunk_duration", type=float, default=0.0, help="Seconds per row, for end_s")
    p.add_argument("--npz_out", type=str, default="", help="Write the map as an .npz archive as well")
    p.add_argument("--device", type=int, default=0, help="MI355X index")
    return p


def validate_args(args) -> None:
    """Everything that can be refused before an archive is read."""
    from birdnet_stm32.evaluation.search import MAX_K as SEARCH_MAX_K

    if not args.perplexity >= 1.0:
        raise ValueError(f"--perplexity {args.perplexity} must be >= 1")
    if 3.0 * args.perplexity > SEARCH_MAX_K:
        raise ValueError(f"--perplexity {args.perplexity} above {SEARCH_MAX_K // 3} (3 * perplexity neighbours, at most {SEARCH_MAX_K})")
    if args.n_iter < 0 or args.exaggeration_iter < 0:
        raise ValueError("--n_iter and --exaggeration_iter must be >= 0")
    if not (math.isfinite(args.early_exaggeration) and args.early_exaggeration >= 1.0):
        raise ValueError(f"--early_exaggeration {args.early_exaggeration} must be finite and >= 1")
    if args.learning_rate is not None and not (math.isfinite(args.learning_rate) and args.learning_rate > 0.0):
        raise ValueError(f"--learning_rate {args.learning_rate} must be finite and > 0")
    if args.chunk_duration < 0:
        raise ValueError("--chunk_duration must be >= 0")
    for path in args.database:
        if not os.path.isfile(path):
            raise FileNotFoundError(f"archive not found: {path}")


def write_map_csv(path: str, index, result, chunk_duration: float) -> int:
    """One line per row of the index.  Returns the number of lines."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS)
        for i in range(len(index)):
            start = float(index.start_s[i])
            x, y = (float(v) for v in result.xy[i])
            on_map = math.isfinite(x) and math.isfinite(y)
            w.writerow([index.paths[int(index.file_index[i])], f"{start:.3f}", f"{start + chunk_duration:.3f}", f"{x:.7g}" if on_map else "",
                        f"{y:.7g}" if on_map else ""])
    return len(index)


def write_map_archive(path: str, index, result) -> None:
    import numpy as np

    with open(path, "wb") as f:   # (np.savez would append .npz to a name without it)
        np.savez(f, xy=result.xy, file_index=index.file_index, start_s=index.start_s, paths=np.asarray(index.paths), kl=np.float64(result.kl),
                 beta=result.beta)


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        validate_args(args)
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"error: {exc}") from None
    from birdnet_stm32.evaluation.project import project_index
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    try:
        index = EmbeddingIndex.from_npz(*args.database)
        result = project_index(index, perplexity=args.perplexity, n_iter=args.n_iter, early_exaggeration=args.early_exaggeration,
                               exaggeration_iter=args.exaggeration_iter, learning_rate=args.learning_rate, seed=args.seed, device=args.device,
                               init=args.init)
    except ValueError as exc:
        raise SystemExit(f"error: {exc}") from None
    write_map_csv(args.output, index, result, args.chunk_duration)
    if args.npz_out:
        write_map_archive(args.npz_out, index, result)
    print(f"Projected {len(index)} rows x {index.dim} ({index.dtype}) onto a map: {result.n_iter} iterations at perplexity {args.perplexity:g}, "
          f"KL divergence {result.kl:.4f} -> {args.output}")
    index.close()
    return result


if __name__ == "__main__":
    main()
