"""``birdnet-stm32 density`` — which call types are in here when nobody knows how many, and what is only background?

The database is one or more ``.npz`` archives written by ``embed``.  Their rows are clustered by HDBSCAN over cosine scores, the spanning
tree on the GPU (``evaluation/density.py``), and written as two CSV files:

    <output>            path, start_s, end_s, cluster, score                    one line per row (cluster -1: noise or a zero row)
    <stem>_summary.csv  cluster, count, stability, exemplar_1, exemplar_2, ...  one line per cluster, exemplars as path@start_s

The first file has ``cluster``'s columns and lines up with ``cluster``'s and ``project``'s files for the same archives; ``score`` is the
membership (1 at a cluster's core, towards 0 at its rim, 0 for noise).  ``end_s`` is ``start_s`` plus ``--chunk_duration`` (the archive
does not record it; 0 leaves ``end_s = start_s``).  ``--exemplars`` are a cluster's densest members, found on the host, so int8 archives
have them too; sorted into class folders they feed ``probe``.

``--silhouette`` scores the clusters with the exact cosine silhouette (``evaluation/silhouette.py``), noise and zero rows excluded:
``<output>`` gets the columns ``silhouette`` and ``nearest_cluster`` (empty and -1 for noise), the summary a ``silhouette`` column behind
``stability``.  It needs at least 2 clusters and is refused, after the fit, where there are fewer.
"""

from __future__ import annotations

import argparse
import csv
import os

from birdnet_stm32.cli.cluster import CSV_COLUMNS, SILHOUETTE_COLUMNS, SUMMARY_SILHOUETTE_COLUMN, cluster_mean_cell, summary_path, write_clusters_csv

SUMMARY_COLUMNS = ("cluster", "count", "stability")

__all__ = ["CSV_COLUMNS", "SUMMARY_COLUMNS", "build_parser", "validate_args", "summary_path", "write_clusters_csv", "write_summary_csv", "main"]


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Density clustering (HDBSCAN, cosine) of the rows of archives written by `embed`: no K, a noise label.")
    p.add_argument("--database", type=str, nargs="+", required=True, help="One or more .npz archives written by `embed`")
    p.add_argument("--output", type=str, required=True, help="Output CSV path (one line per row); <stem>_summary.csv is written next to it")
    p.add_argument("--min_cluster_size", type=int, default=15, help="Fewest rows a cluster holds (>= 2)")
    p.add_argument("--min_samples", type=int, default=None, help="Rows, the row itself included, whose neighbourhood sets a row's density (1..129; default: --min_cluster_size)")
    p.add_argument("--exemplars", type=int, default=5, help="Densest members per cluster in the summary")
    p.add_argument("--silhouette", action="store_true", help="Add each clustered row's silhouette and nearest other cluster, and each cluster's mean silhouette")
    p.add_argument("--chunk_duration", type=float, default=0.0, help="Seconds per row, for end_s")
    p.add_argument("--device", type=int, default=0, help="MI355X index")
    return p


def validate_args(args) -> None:
    """Everything that can be refused before an archive is read."""
    from birdnet_stm32.evaluation.density import check_density_flags

    try:
        check_density_flags(args.min_cluster_size, args.min_samples, args.exemplars)
    except ValueError as exc:
        raise ValueError(f"--{exc}") from None
    if args.chunk_duration < 0:
        raise ValueError("--chunk_duration must be >= 0")
    for path in args.database:
        if not os.path.isfile(path):
            raise FileNotFoundError(f"archive not found: {path}")


def write_summary_csv(path: str, index, result, silhouette=None) -> int:
    """One line per cluster: its member count, its stability, with a ``SilhouetteResult`` its mean silhouette, and its exemplars as
    ``path@start_s``."""
    E = result.exemplar_idx.shape[1]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(SUMMARY_COLUMNS + ((SUMMARY_SILHOUETTE_COLUMN,) if silhouette is not None else ()) + tuple(f"exemplar_{e + 1}" for e in range(E)))
        for c in range(result.n_clusters):
            ex = [f"{index.paths[int(index.file_index[i])]}@{float(index.start_s[i]):.3f}" if i >= 0 else "" for i in result.exemplar_idx[c]]
            w.writerow([c, int((result.labels == c).sum()), f"{float(result.stability[c]):.7g}"]
                       + ([cluster_mean_cell(silhouette, c)] if silhouette is not None else []) + ex)
    return result.n_clusters


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        validate_args(args)
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"error: {exc}") from None
    from birdnet_stm32.evaluation.density import density_index
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    try:
        index = EmbeddingIndex.from_npz(*args.database)
        result = density_index(index, args.min_cluster_size, args.min_samples, exemplars=args.exemplars, device=args.device)
        silhouette = None
        if args.silhouette:
            if result.n_clusters < 2:
                raise ValueError(f"--silhouette needs at least 2 clusters; the fit found {result.n_clusters}")
            from birdnet_stm32.evaluation.silhouette import silhouette_index

            silhouette = silhouette_index(index, result.labels, result.n_clusters, device=args.device)
    except ValueError as exc:
        raise SystemExit(f"error: {exc}") from None
    write_clusters_csv(args.output, index, result, args.chunk_duration, silhouette)
    write_summary_csv(summary_path(args.output), index, result, silhouette)
    noise = int((result.labels < 0).sum())
    print(f"Clustered {len(index)} rows x {index.dim} ({index.dtype}) by density: {result.n_clusters} clusters, {noise} rows of noise, "
          f"spanning tree in {result.rounds} rounds" + (f", mean silhouette {silhouette.mean:.4f}" if silhouette is not None else "") + f" -> {args.output}")
    index.close()
    return result


if __name__ == "__main__":
    main()
