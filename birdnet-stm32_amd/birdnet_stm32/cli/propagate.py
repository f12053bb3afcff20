"""``birdnet-stm32 propagate`` — I have labelled forty rows of this archive; what are the others?

The database is one or more ``.npz`` archives written by ``embed``.  The few labels given are spread over all its rows along the
nearest-neighbour graph on the GPU (``evaluation/propagate.py``: label spreading, scikit-learn's iteration) and written as

    <output>            row, path, start_s, label, score, seeded       one line per row in the archive's order, as ``cluster`` writes them
                                                                       (label empty: a zero row, a row no label reaches, or below --min_score)
    <stem>_summary.csv  class, seeds, rows, mean_score, holdout_recall one line per class
    <stem>_labels.txt   the class names, sorted, one per line

The labels come from ``--labels``, a CSV with a header and the columns ``path,label`` (every row of that file) or ``path,start_s,label``
(the row of that file that starts there), or from ``--labelled``, archives embedded from class folders (``probe``'s layout): their rows
join the database behind its own and take the name of their file's parent folder.  ``--holdout H`` hides that share of the labelled rows
first and reports how many of them come back right; what is written still uses every label.  ``--scores_out`` writes the label matrix
``F`` [N, C] float32 (NaN for a zero row) with the class names and the archive's ``file_index``, ``start_s`` and ``paths``.
"""

from __future__ import annotations

import argparse
import csv
import math
import os

CSV_COLUMNS = ("row", "path", "start_s", "label", "score", "seeded")
SUMMARY_COLUMNS = ("class", "seeds", "rows", "mean_score", "holdout_recall")
START_TOLERANCE_S = 5e-4   # start_s is written with three decimals


def build_parser() -> argparse.ArgumentParser:
    from birdnet_stm32.evaluation import propagate as P

    p = argparse.ArgumentParser(description="Spread a few labels over the rows of archives written by `embed` (label spreading on the GPU).")
    p.add_argument("--database", type=str, nargs="+", required=True, help="One or more .npz archives written by `embed`")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--labels", type=str, default="", help="CSV with a header: path,label or path,start_s,label")
    g.add_argument("--labelled", type=str, nargs="+", default=None, help="Archives embedded from class folders; their rows join the database")
    p.add_argument("--output", type=str, required=True, help="Output CSV path (one line per row); <stem>_summary.csv and <stem>_labels.txt go next to it")
    p.add_argument("--neighbours", type=int, default=P.DEFAULT_NEIGHBOURS, help="Nearest neighbours per row in the graph (1..128)")
    p.add_argument("--tau", type=float, default=P.DEFAULT_TAU, help="Width of the edge weight exp((cosine - 1) / tau)")
    p.add_argument("--alpha", type=float, default=P.DEFAULT_ALPHA, help="Share a row takes from its neighbours per update, in (0, 1)")
    p.add_argument("--max_iter", type=int, default=P.DEFAULT_MAX_ITER, help="Most updates")
    p.add_argument("--tol", type=float, default=P.DEFAULT_TOL, help="Stop when the label matrix changes by less (sum of absolute differences); 0: never")
    p.add_argument("--min_score", type=float, default=0.0, help="Rows whose score is below this are written without a label")
    p.add_argument("--holdout", type=float, default=0.0, help="Share of the labelled rows hidden to measure accuracy, in (0, 1); 0: none")
    p.add_argument("--holdout_seed", type=int, default=0, help="Seed of the hold-out split")
    p.add_argument("--scores_out", type=str, default="", help="Write the label matrix as an .npz archive as well")
    p.add_argument("--device", type=int, default=0, help="MI355X index")
    return p


def validate_args(args) -> None:
    """Everything that can be refused before an archive is read."""
    from birdnet_stm32.evaluation.search import MAX_K as SEARCH_MAX_K

    if not 1 <= args.neighbours <= SEARCH_MAX_K:
        raise ValueError(f"--neighbours {args.neighbours} outside 1..{SEARCH_MAX_K}")
    if not (math.isfinite(args.tau) and args.tau > 0.0):
        raise ValueError(f"--tau {args.tau} must be finite and > 0")
    if not 0.0 < args.alpha < 1.0:
        raise ValueError(f"--alpha {args.alpha} must lie in (0, 1)")
    if args.max_iter < 0 or not args.tol >= 0.0:
        raise ValueError("--max_iter and --tol must be >= 0")
    if not 0.0 <= args.min_score <= 1.0:
        raise ValueError(f"--min_score {args.min_score} outside 0..1")
    if not (args.holdout == 0.0 or 0.0 < args.holdout < 1.0):
        raise ValueError(f"--holdout {args.holdout} must be 0 or lie in (0, 1)")
    for path in list(args.database) + list(args.labelled or []) + ([args.labels] if args.labels else []):
        if not os.path.isfile(path):
            raise FileNotFoundError(f"file not found: {path}")


def read_labels_csv(path: str) -> list[tuple]:
    """The lines of a ``--labels`` file as ``(path, start_s or None, label)``."""
    with open(path, newline="") as f:
        reader = csv.DictReader(f)
        fields = tuple(name.strip() for name in (reader.fieldnames or ()))
        if fields not in (("path", "label"), ("path", "start_s", "label")):
            raise ValueError(f"{path}: the header must be path,label or path,start_s,label, not {','.join(fields)}")
        reader.fieldnames = list(fields)
        out = []
        for line, rec in enumerate(reader, start=2):
            name, label = (rec["path"] or "").strip(), (rec["label"] or "").strip()
            if not name or not label:
                raise ValueError(f"{path}:{line}: an empty path or label")
            start = None
            if "start_s" in fields:
                try:
                    start = float(rec["start_s"])
                except (TypeError, ValueError):
                    raise ValueError(f"{path}:{line}: start_s {rec['start_s']!r} is not a number") from None
            out.append((name, start, label))
    if not out:
        raise ValueError(f"{path}: no labels")
    return out


def seeds_from_records(index, records) -> tuple:
    """``(seed_label [N] int32, class names sorted)`` from the lines of a ``--labels`` file.  A path stands for the file of the archive
    with the same name or, failing that, the same resolved name; a line that matches no row, and a row given two labels, are errors."""
    import numpy as np

    names = sorted({label for _, _, label in records})
    by_name: dict = {}
    for i, p in enumerate(index.paths):
        by_name.setdefault(p, []).append(i)
    by_real: dict = {}
    for i, p in enumerate(index.paths):
        by_real.setdefault(os.path.realpath(p), []).append(i)
    seed = np.full(len(index), -1, np.int32)
    for name, start, label in records:
        files = by_name.get(name) or by_real.get(os.path.realpath(name)) or []
        rows = np.flatnonzero(np.isin(index.file_index, files))
        if start is not None:
            rows = rows[np.abs(index.start_s[rows] - start) < START_TOLERANCE_S]
        if rows.size == 0:
            raise ValueError(f"--labels: {name}" + (f" at {start:.3f} s" if start is not None else "") + " matches no row of the database")
        c = names.index(label)
        clash = rows[(seed[rows] >= 0) & (seed[rows] != c)]
        if clash.size:
            raise ValueError(f"--labels: {name} row {int(clash[0])} is labelled {names[int(seed[clash[0]])]} and {label}")
        seed[rows] = c
    return seed, names


def seeds_from_folders(index, first_row: int) -> tuple:
    """``(seed_label [N] int32, class names sorted)``: the rows from ``first_row`` on take the name of their file's parent folder."""
    import numpy as np

    folder = [os.path.basename(os.path.dirname(p)) for p in index.paths]
    files = np.unique(index.file_index[first_row:])
    missing = [index.paths[int(f)] for f in files if not folder[int(f)]]
    if missing:
        raise ValueError(f"--labelled: {missing[0]} has no parent folder to take a class name from")
    names = sorted({folder[int(f)] for f in files})
    seed = np.full(len(index), -1, np.int32)
    where = np.asarray([names.index(folder[i]) if folder[i] in names else -1 for i in range(len(folder))], np.int32)
    seed[first_row:] = where[index.file_index[first_row:]]
    return seed, names


def archive_rows(path: str) -> int:
    import numpy as np

    with np.load(path, allow_pickle=False) as z:
        if "file_index" not in z.files:
            raise ValueError(f"{path}: not an archive written by `embed` (no file_index)")
        return int(z["file_index"].shape[0])


def summary_path(output: str) -> str:
    stem, ext = os.path.splitext(output)
    return f"{stem}_summary{ext or '.csv'}"


def labels_path(output: str) -> str:
    return os.path.splitext(output)[0] + "_labels.txt"


def write_propagate_csv(path: str, index, labels, scores, seed_label, names) -> int:
    """One line per row of the index (``CSV_COLUMNS``).  Returns the number of lines."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS)
        for i in range(len(index)):
            s = float(scores[i])
            w.writerow([i, index.paths[int(index.file_index[i])], f"{float(index.start_s[i]):.3f}", names[int(labels[i])] if labels[i] >= 0 else "",
                        "" if s != s else f"{s:.7g}", int(seed_label[i] >= 0)])
    return len(index)


def write_summary_csv(path: str, labels, scores, seed_label, names, holdout=None) -> int:
    """One line per class: its seeds, the rows it won, their mean score and, after a hold-out, its recall on the hidden rows."""
    import numpy as np

    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(SUMMARY_COLUMNS)
        for c, name in enumerate(names):
            m = labels == c
            mean = float(np.asarray(scores)[m].astype(np.float64).mean()) if m.any() else 0.0
            r = float(holdout.recall[c]) if holdout is not None else math.nan
            w.writerow([name, int((seed_label == c).sum()), int(m.sum()), f"{mean:.7g}", "" if r != r else f"{r:.7g}"])
    return len(names)


def write_scores_archive(path: str, index, result, names) -> None:
    import numpy as np

    with open(path, "wb") as f:   # (np.savez would append .npz to a name without it)
        np.savez(f, F=result.F, labels=np.asarray(names), file_index=index.file_index, start_s=index.start_s, paths=np.asarray(index.paths))


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        validate_args(args)
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"error: {exc}") from None
    from birdnet_stm32.evaluation.propagate import apply_min_score, propagate_index
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    try:
        if args.labelled:
            first = sum(archive_rows(p) for p in args.database)
            index = EmbeddingIndex.from_npz(*args.database, *args.labelled)
            seed_label, names = seeds_from_folders(index, first)
        else:
            index = EmbeddingIndex.from_npz(*args.database)
            seed_label, names = seeds_from_records(index, read_labels_csv(args.labels))
        result = propagate_index(index, seed_label, len(names), neighbours=args.neighbours, tau=args.tau, alpha=args.alpha, max_iter=args.max_iter,
                                 tol=args.tol, holdout=args.holdout, seed=args.holdout_seed, device=args.device, keep_scores=bool(args.scores_out))
    except ValueError as exc:
        raise SystemExit(f"error: {exc}") from None
    written = apply_min_score(result.labels, result.scores, args.min_score)
    write_propagate_csv(args.output, index, written, result.scores, seed_label, names)
    write_summary_csv(summary_path(args.output), written, result.scores, seed_label, names, result.holdout)
    with open(labels_path(args.output), "w") as f:
        f.write("".join(name + "\n" for name in names))
    if args.scores_out:
        write_scores_archive(args.scores_out, index, result, names)
    held = f", hold-out accuracy {result.holdout.accuracy:.4f} on {result.holdout.rows.size} hidden rows" if result.holdout is not None else ""
    print(f"Spread {int((seed_label >= 0).sum())} labels of {len(names)} classes over {len(index)} rows x {index.dim} ({index.dtype}): "
          f"{result.n_iter} updates, {int((written >= 0).sum())} rows labelled{held} -> {args.output}")
    index.close()
    return result


if __name__ == "__main__":
    main()
