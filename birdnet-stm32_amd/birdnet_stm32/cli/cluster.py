"""``birdnet-stm32 cluster`` — which call types are in here, and which clips should I listen to first?

The database is one or more ``.npz`` archives written by ``embed``.  Their rows are clustered by spherical k-means on the GPU
(``evaluation/cluster.py``) and written as two CSV files:

    <output>            path, start_s, end_s, cluster, score                       one line per row (cluster -1: a zero row)
    <stem>_summary.csv  cluster, count, mean_score, exemplar_1, exemplar_2, ...    one line per cluster, exemplars as path@start_s

``end_s`` is ``start_s`` plus ``--chunk_duration`` (the archive does not record it; 0 leaves ``end_s = start_s``).  ``--exemplars`` are
the best rows per centroid, found by ``search`` (float32 archives only).  ``--centroids_out`` writes the centroids as an archive that
``search --query_npz`` takes as it stands; exemplars sorted into class folders feed ``probe``.

``--silhouette`` scores the fit with the exact cosine silhouette (``evaluation/silhouette.py``): ``<output>`` gets the columns
``silhouette`` and ``nearest_cluster`` (empty and -1 for a zero row), the summary a ``silhouette`` column behind ``mean_score``, and the
mean is printed.  ``--k_sweep K1 K2 ...`` fits ``--k`` and every further candidate with the same ``--max_iter``, ``--n_init`` and
``--seed``, writes

    <stem>_sweep.csv    k, silhouette, mean_score, n_iter, converged, smallest_cluster, largest_cluster    one line per candidate

and the usual files, with the silhouette columns, for the candidate with the highest mean silhouette (the lowest k among equal means).
"""

from __future__ import annotations

import argparse
import csv
import os

CSV_COLUMNS = ("path", "start_s", "end_s", "cluster", "score")
SUMMARY_COLUMNS = ("cluster", "count", "mean_score")
SILHOUETTE_COLUMNS = ("silhouette", "nearest_cluster")   # appended to CSV_COLUMNS by --silhouette
SUMMARY_SILHOUETTE_COLUMN = "silhouette"                 # behind SUMMARY_COLUMNS, before the exemplars
SWEEP_COLUMNS = ("k", "silhouette", "mean_score", "n_iter", "converged", "smallest_cluster", "largest_cluster")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Cluster the rows of archives written by `embed` (spherical k-means, cosine).")
    p.add_argument("--database", type=str, nargs="+", required=True, help="One or more .npz archives written by `embed`")
    p.add_argument("--k", type=int, required=True, help="Number of clusters (1..4096)")
    p.add_argument("--output", type=str, required=True, help="Output CSV path (one line per row); <stem>_summary.csv is written next to it")
    p.add_argument("--k_sweep", type=int, nargs="+", default=None, metavar="K",
                   help="Further candidates for k (2..4096): fit each and --k, keep the one with the highest mean silhouette; <stem>_sweep.csv holds the table")
    p.add_argument("--silhouette", action="store_true", help="Add each row's silhouette and nearest other cluster, and each cluster's mean silhouette")
    p.add_argument("--max_iter", type=int, default=25, help="Most centroid updates per restart")
    p.add_argument("--n_init", type=int, default=1, help="Restarts; the one with the highest mean score is kept")
    p.add_argument("--seed", type=int, default=42, help="Seed of the initial rows")
    p.add_argument("--exemplars", type=int, default=5, help="Best rows per centroid in the summary (0..128; float32 archives only)")
    p.add_argument("--centroids_out", type=str, default="", help="Write the centroids as an .npz archive (for `search --query_npz`)")
    p.add_argument("--chunk_duration", type=float, default=0.0, help="Seconds per row, for end_s")
    p.add_argument("--device", type=int, default=0, help="MI355X index")
    return p


def validate_args(args) -> None:
    """Everything that can be refused before an archive is read."""
    from birdnet_stm32.evaluation.cluster import MAX_K
    from birdnet_stm32.evaluation.search import MAX_K as SEARCH_MAX_K

    if not 1 <= args.k <= MAX_K:
        raise ValueError(f"--k {args.k} outside 1..{MAX_K}")
    if args.k_sweep is not None:
        for k in sweep_candidates(args):
            if not 2 <= k <= MAX_K:
                raise ValueError(f"--k_sweep: k={k} outside 2..{MAX_K} (a silhouette needs two clusters)")
    if args.max_iter < 0 or args.n_init < 1:
        raise ValueError("--max_iter must be >= 0 and --n_init >= 1")
    if not 0 <= args.exemplars <= SEARCH_MAX_K:
        raise ValueError(f"--exemplars {args.exemplars} outside 0..{SEARCH_MAX_K}")
    if args.chunk_duration < 0:
        raise ValueError("--chunk_duration must be >= 0")
    for path in args.database:
        if not os.path.isfile(path):
            raise FileNotFoundError(f"archive not found: {path}")


def sweep_candidates(args) -> list[int]:
    """The candidates of ``--k_sweep``: ``--k`` and the further values, each once, ascending."""
    return sorted({int(args.k), *(int(k) for k in args.k_sweep)})


def summary_path(output: str) -> str:
    stem, ext = os.path.splitext(output)
    return f"{stem}_summary{ext or '.csv'}"


def sweep_path(output: str) -> str:
    stem, ext = os.path.splitext(output)
    return f"{stem}_sweep{ext or '.csv'}"


def silhouette_cells(silhouette, i: int) -> list:
    """The two cells of ``SILHOUETTE_COLUMNS`` for row i: an empty silhouette and -1 for a row that took no part."""
    s = float(silhouette.silhouette[i])
    return ["" if s != s else f"{s:.7g}", int(silhouette.nearest[i])]


def write_clusters_csv(path: str, index, result, chunk_duration: float, silhouette=None) -> int:
    """One line per row of the index; with a ``SilhouetteResult`` the two columns of ``SILHOUETTE_COLUMNS`` behind the others.  Returns
    the number of lines."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS + (SILHOUETTE_COLUMNS if silhouette is not None else ()))
        for i in range(len(index)):
            start = float(index.start_s[i])
            w.writerow([index.paths[int(index.file_index[i])], f"{start:.3f}", f"{start + chunk_duration:.3f}", int(result.labels[i]),
                        f"{float(result.score[i]):.7g}"] + (silhouette_cells(silhouette, i) if silhouette is not None else []))
    return len(index)


def cluster_mean_cell(silhouette, c: int) -> str:
    """A cluster's mean silhouette as a summary cell, empty for a cluster without live rows."""
    m = float(silhouette.cluster_mean[c])
    return "" if m != m else f"{m:.7g}"


def write_summary_csv(path: str, index, result, silhouette=None) -> int:
    """One line per cluster: its member count, the mean score of its members, with a ``SilhouetteResult`` their mean silhouette, and its
    exemplars as ``path@start_s``."""
    import numpy as np

    K, E = result.centroids.shape[0], result.exemplar_idx.shape[1]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(SUMMARY_COLUMNS + ((SUMMARY_SILHOUETTE_COLUMN,) if silhouette is not None else ()) + tuple(f"exemplar_{e + 1}" for e in range(E)))
        for c in range(K):
            m = result.labels == c
            mean = float(result.score[m].astype(np.float64).mean()) if m.any() else 0.0
            ex = [f"{index.paths[int(index.file_index[i])]}@{float(index.start_s[i]):.3f}" if i >= 0 else "" for i in result.exemplar_idx[c]]
            w.writerow([c, int(m.sum()), f"{mean:.7g}"] + ([cluster_mean_cell(silhouette, c)] if silhouette is not None else []) + ex)
    return K


def write_sweep_csv(path: str, table) -> int:
    """One line per candidate of a sweep (``SWEEP_COLUMNS``)."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(SWEEP_COLUMNS)
        for row in table:
            w.writerow([int(row["k"]), f"{row['silhouette']:.7g}", f"{row['mean_score']:.7g}", int(row["n_iter"]), int(bool(row["converged"])),
                        int(row["smallest_cluster"]), int(row["largest_cluster"])])
    return len(table)


def write_centroid_archive(path: str, centroids) -> None:
    import numpy as np

    from birdnet_stm32.evaluation.cluster import centroid_archive

    with open(path, "wb") as f:   # (np.savez would append .npz to a name without it)
        np.savez(f, **centroid_archive(centroids))


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        validate_args(args)
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"error: {exc}") from None
    from birdnet_stm32.evaluation.cluster import cluster_index
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    try:
        index = EmbeddingIndex.from_npz(*args.database)
        if args.exemplars and index.dtype == "int8":
            raise ValueError("--exemplars are found by `search`, which needs queries of the database's dtype: the centroids of an int8 archive are "
                             "float32 (pass --exemplars 0, or cluster a float32 archive)")
        silhouette, table = None, None
        if args.k_sweep is not None:
            from birdnet_stm32.evaluation.silhouette import cluster_sweep

            result, silhouette, table = cluster_sweep(index, sweep_candidates(args), max_iter=args.max_iter, n_init=args.n_init, seed=args.seed,
                                                      exemplars=args.exemplars, device=args.device)
        else:
            result = cluster_index(index, args.k, max_iter=args.max_iter, n_init=args.n_init, seed=args.seed, exemplars=args.exemplars, device=args.device)
            if args.silhouette:
                from birdnet_stm32.evaluation.silhouette import silhouette_index

                silhouette = silhouette_index(index, result.labels, result.centroids.shape[0], device=args.device)
    except ValueError as exc:
        raise SystemExit(f"error: {exc}") from None
    k = int(result.centroids.shape[0])
    write_clusters_csv(args.output, index, result, args.chunk_duration, silhouette)
    write_summary_csv(summary_path(args.output), index, result, silhouette)
    if table is not None:
        write_sweep_csv(sweep_path(args.output), table)
        print("      k  silhouette  mean_score  updates  converged  smallest  largest")
        for row in table:
            print(f"{row['k']:7d}  {row['silhouette']:10.4f}  {row['mean_score']:10.4f}  {row['n_iter']:7d}  {str(bool(row['converged'])):>9}  "
                  f"{row['smallest_cluster']:8d}  {row['largest_cluster']:7d}{'   <- chosen' if row['k'] == k else ''}")
        print(f"Chose k = {k}: the highest mean silhouette of {len(table)} candidates -> {sweep_path(args.output)}")
    if args.centroids_out:
        write_centroid_archive(args.centroids_out, result.centroids)
    print(f"Clustered {len(index)} rows x {index.dim} ({index.dtype}) into {k} clusters: {result.n_iter} updates, "
          f"{'converged' if result.converged else 'not converged'}, mean score {result.mean_score:.4f}"
          + (f", mean silhouette {silhouette.mean:.4f}" if silhouette is not None else "") + f" -> {args.output}")
    index.close()
    return result


if __name__ == "__main__":
    main()
