"""``birdnet-stm32 select`` — which rows of this archive should I listen to next?

The database is one or more ``.npz`` archives written by ``embed``.  ``--budget`` rows are chosen on the GPU by farthest-first traversal
(``evaluation/select.py``: k-centre greedy), each the row least like everything chosen so far, and written as

    <output>          rank, row, path, start_s, key, weight, guess, covers    one line per pick, in pick order
    --coverage_out    row, path, start_s, nearest_row, similarity, taken      one line per row in the archive's order, as ``cluster`` writes them
                                                                              (taken: 0 no, 1 picked, 2 labelled already)

Rows that are labelled already are where the traversal starts: ``--labels`` (a CSV ``path,label`` or ``path,start_s,label``) or
``--labelled`` (archives embedded from class folders, whose rows join the database behind its own) mean what they mean for ``propagate``.
Without either the first pick is ``--first`` or, failing that, the most central row.  ``--scores`` takes the label matrix that
``propagate --scores_out`` wrote for the same rows and weights every row's distance by how unsure that labelling is (``--uncertainty``);
``guess`` is then the row's best class.  ``covers`` counts the untaken rows whose nearest chosen row is this pick.  ``--min_key R`` ends the
list before the first pick whose key is below ``R``.
"""

from __future__ import annotations

import argparse
import csv
import math
import os

from birdnet_stm32.cli.propagate import archive_rows, read_labels_csv, seeds_from_folders, seeds_from_records

CSV_COLUMNS = ("rank", "row", "path", "start_s", "key", "weight", "guess", "covers")
COVERAGE_COLUMNS = ("row", "path", "start_s", "nearest_row", "similarity", "taken")
UNCERTAINTY_MODES = ("margin", "entropy", "least_confidence")   # evaluation/select.py: UNCERTAINTY_MODES


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Choose the rows of archives written by `embed` to label next (farthest-first traversal on the GPU).")
    p.add_argument("--database", type=str, nargs="+", required=True, help="One or more .npz archives written by `embed`")
    p.add_argument("--budget", type=int, required=True, help="Rows to choose")
    p.add_argument("--output", type=str, required=True, help="Output CSV path (one line per pick)")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--labels", type=str, default="", help="CSV with a header: path,label or path,start_s,label; its rows are chosen already")
    g.add_argument("--labelled", type=str, nargs="+", default=None, help="Archives embedded from class folders; their rows join the database, chosen already")
    p.add_argument("--scores", type=str, default="", help="The label matrix `propagate --scores_out` wrote for the same rows")
    p.add_argument("--uncertainty", type=str, default=None, choices=UNCERTAINTY_MODES, help="How --scores weights a row (default with --scores: margin)")
    p.add_argument("--first", type=int, default=None, help="Row to start from (default: the labelled rows or, without any, the most central row)")
    p.add_argument("--min_key", type=float, default=0.0, help="End the list before the first pick whose key is below this")
    p.add_argument("--coverage_out", type=str, default="", help="Write every row's nearest chosen row as a CSV as well")
    p.add_argument("--device", type=int, default=0, help="MI355X index")
    return p


def validate_args(args) -> None:
    """Everything that can be refused before an archive is read."""
    if args.budget < 1:
        raise ValueError(f"--budget {args.budget} must be >= 1")
    if args.first is not None and args.first < 0:
        raise ValueError(f"--first {args.first} must be a row number >= 0")
    if math.isnan(args.min_key):
        raise ValueError("--min_key is not a number")
    if args.uncertainty and not args.scores:
        raise ValueError("--uncertainty needs --scores")
    for path in list(args.database) + list(args.labelled or []) + [p for p in (args.labels, args.scores) if p]:
        if not os.path.isfile(path):
            raise FileNotFoundError(f"file not found: {path}")


def read_scores(path: str, index):
    """``(F [N, C] float32, class names)`` of a ``propagate --scores_out`` archive, refused unless it lines up with the database: the same
    number of rows, ``file_index`` and ``start_s``."""
    import numpy as np

    with np.load(path, allow_pickle=False) as z:
        missing = [key for key in ("F", "labels", "file_index", "start_s") if key not in z.files]
        if missing:
            raise ValueError(f"{path}: not an archive written by `propagate --scores_out` (no {', '.join(missing)})")
        F, names = np.asarray(z["F"], np.float32), [str(s) for s in z["labels"]]
        file_index, start_s = z["file_index"], z["start_s"]
    if F.ndim != 2 or F.shape[0] != len(index) or F.shape[1] != len(names) or F.shape[1] < 1:
        raise ValueError(f"--scores: {path} holds {F.shape} scores of {len(names)} classes, the database has {len(index)} rows")
    if not (np.array_equal(file_index, index.file_index) and np.array_equal(start_s, index.start_s)):
        raise ValueError(f"--scores: the rows of {path} are not the database's (file_index / start_s differ)")
    return F, names


def taken_flags(n_rows: int, result):
    """0 no, 1 picked, 2 chosen before the run (a seed, or the caller's first)."""
    import numpy as np

    taken = np.zeros(n_rows, np.int64)
    taken[result.picked] = 1
    taken[result.seeds] = 2
    return taken


def write_select_csv(path: str, index, result, weights=None, F=None, names=None) -> int:
    """One line per pick (``CSV_COLUMNS``).  Returns the number of lines."""
    import numpy as np

    taken = taken_flags(len(index), result)
    open_rows = (taken == 0) & (result.nearest >= 0)
    covers = np.bincount(result.nearest[open_rows], minlength=len(index))
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS)
        for rank, (row, key) in enumerate(zip(result.picked.tolist(), result.key.tolist())):
            guess = ""
            if F is not None and not np.isnan(F[row]).any():
                guess = names[int(np.argmax(F[row]))]
            w.writerow([rank, row, index.paths[int(index.file_index[row])], f"{float(index.start_s[row]):.3f}", f"{key:.7g}",
                        f"{1.0 if weights is None else float(weights[row]):.7g}", guess, int(covers[row])])
    return int(result.picked.size)


def write_coverage_csv(path: str, index, result) -> int:
    """One line per row of the index (``COVERAGE_COLUMNS``).  Returns the number of lines."""
    taken = taken_flags(len(index), result)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(COVERAGE_COLUMNS)
        for i in range(len(index)):
            s = float(result.similarity[i])
            w.writerow([i, index.paths[int(index.file_index[i])], f"{float(index.start_s[i]):.3f}", "" if result.nearest[i] < 0 else int(result.nearest[i]),
                        "" if s != s else f"{s:.7g}", int(taken[i])])
    return len(index)


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        validate_args(args)
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"error: {exc}") from None
    import numpy as np

    from birdnet_stm32.evaluation import select as S
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    try:
        seeds = None
        if args.labelled:
            first_row = sum(archive_rows(p) for p in args.database)
            index = EmbeddingIndex.from_npz(*args.database, *args.labelled)
            seeds = np.flatnonzero(seeds_from_folders(index, first_row)[0] >= 0)
        else:
            index = EmbeddingIndex.from_npz(*args.database)
            if args.labels:
                seeds = np.flatnonzero(seeds_from_records(index, read_labels_csv(args.labels))[0] >= 0)
        F = names = weights = None
        if args.scores:
            F, names = read_scores(args.scores, index)
            weights = S.uncertainty_reference(F, args.uncertainty or "margin")
        result = S.select_index(index, args.budget, seeds=seeds, weights=weights, first=args.first, min_key=args.min_key, device=args.device)
    except ValueError as exc:
        raise SystemExit(f"error: {exc}") from None
    write_select_csv(args.output, index, result, weights, F, names)
    if args.coverage_out:
        write_coverage_csv(args.coverage_out, index, result)
    print(f"Chose {result.picked.size} of {len(index)} rows x {index.dim} ({index.dtype}) after {result.seeds.size} chosen already"
          + (f", weighted by {args.uncertainty or 'margin'}" if weights is not None else "") + f" -> {args.output}")
    index.close()
    return result


if __name__ == "__main__":
    main()
