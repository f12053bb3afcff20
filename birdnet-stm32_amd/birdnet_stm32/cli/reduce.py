"""``birdnet-stm32 reduce`` — centre, rotate, shorten and optionally whiten the rows of archives written by ``embed``.

The database is one or more ``.npz`` archives written by ``embed``.  Their rows are projected onto their leading principal components
(``evaluation/reduce.py``; the sums over rows run on the GPU) and written as an ordinary archive of float32 ``[N, r]`` rows, which
``search``, ``cluster``, ``density`` and ``project`` take unchanged (it carries the model as extra ``pca_*`` keys, which they ignore):

    reduce --database DB.npz [DB2.npz ...] --output R.npz [--components 32 | --variance 0.95] [--whiten] [--model_out PCA.npz] [--variance_out V.csv]
    reduce --model PCA.npz --database Q.npz --output QR.npz

``--variance_out`` writes component, explained variance, ratio and cumulative ratio: how many dimensions the archive really has.
``--model`` applies a saved model to another archive — the way to search by example against a reduced database: ``embed`` the queries,
``reduce --model``, then ``search --query_npz``.  The default is ``--components 32``, or as many as the width and the live rows allow.
"""

from __future__ import annotations

import argparse
import csv
import os

VARIANCE_COLUMNS = ("component", "explained_variance", "ratio", "cumulative_ratio")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Principal components of the rows of archives written by `embed`: a reduced archive the other commands take.")
    p.add_argument("--database", type=str, nargs="+", required=True, help="One or more .npz archives written by `embed`")
    p.add_argument("--output", type=str, required=True, help="Output .npz archive of float32 [N, r] rows")
    p.add_argument("--components", type=int, default=None, help="Components to keep (default 32, or fewer where the width or the rows allow no more)")
    p.add_argument("--variance", type=float, default=None, help="Keep the fewest components that explain this share of the variance (0..1)")
    p.add_argument("--whiten", action="store_true", help="Scale every component to unit variance")
    p.add_argument("--model", type=str, default="", help="Apply a model written by --model_out instead of fitting one")
    p.add_argument("--model_out", type=str, default="", help="Write the fitted model as an .npz file")
    p.add_argument("--variance_out", type=str, default="", help="Write the explained-variance table as CSV")
    p.add_argument("--device", type=int, default=0, help="MI355X index")
    return p


def validate_args(args) -> None:
    """Everything that can be refused before an archive is read."""
    if args.components is not None and args.variance is not None:
        raise ValueError("--components and --variance are mutually exclusive")
    if args.components is not None and args.components < 1:
        raise ValueError(f"--components {args.components} must be >= 1")
    if args.variance is not None and not 0.0 < args.variance < 1.0:
        raise ValueError(f"--variance {args.variance} must be inside (0, 1)")
    if args.model and (args.components is not None or args.variance is not None or args.whiten or args.model_out):
        raise ValueError("--model applies a saved model: --components, --variance, --whiten and --model_out belong to the fit")
    if args.model and not os.path.isfile(args.model):
        raise FileNotFoundError(f"model not found: {args.model}")
    for path in args.database:
        if not os.path.isfile(path):
            raise FileNotFoundError(f"archive not found: {path}")


def requested_components(args, index, n_live: int):
    """What the fit is asked for: ``--variance``, ``--components``, or the default clipped to ``min(D, live rows - 1)``."""
    from birdnet_stm32.evaluation.reduce import DEFAULT_COMPONENTS

    if args.variance is not None:
        return float(args.variance)
    if args.components is not None:
        return int(args.components)
    return max(1, min(DEFAULT_COMPONENTS, index.dim, n_live - 1))


def write_variance_csv(path: str, model) -> int:
    ratio = model.explained_variance_ratio
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(VARIANCE_COLUMNS)
        cum = 0.0
        for k in range(model.n_components):
            cum += float(ratio[k])
            w.writerow([k, f"{float(model.explained_variance[k]):.9g}", f"{float(ratio[k]):.9g}", f"{cum:.9g}"])
    return model.n_components


def write_reduced_archive(path: str, reduced, model) -> None:
    import numpy as np

    with open(path, "wb") as f:   # (np.savez would append .npz to a name without it)
        np.savez(f, embeddings=reduced.embeddings, file_index=reduced.file_index, start_s=reduced.start_s, paths=np.asarray(reduced.paths),
                 **model.fields("pca_"))


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        validate_args(args)
    except (ValueError, FileNotFoundError) as exc:
        raise SystemExit(f"error: {exc}") from None
    import numpy as np

    from birdnet_stm32.evaluation.reduce import PcaModel, check_live, check_model_applies, fit_pca, reduce_index
    from birdnet_stm32.evaluation.search import EmbeddingIndex, inv_norms_reference

    try:   # every refusal comes before a file is written
        index = EmbeddingIndex.from_npz(*args.database)
        if args.model:
            model = PcaModel.load(args.model)
            check_model_applies(model, index)
        else:
            n_live = int(np.count_nonzero(inv_norms_reference(index.embeddings, index.zero_point)))
            check_live(n_live)
            model = fit_pca(index, requested_components(args, index, n_live), args.whiten, device=args.device)
        reduced, model = reduce_index(index, model, device=args.device)
    except ValueError as exc:
        raise SystemExit(f"error: {exc}") from None
    write_reduced_archive(args.output, reduced, model)
    if args.model_out:
        model.save(args.model_out)
    if args.variance_out:
        write_variance_csv(args.variance_out, model)
    share = float(model.explained_variance.sum() / model.total_variance)
    print(f"Reduced {len(index)} rows x {index.dim} ({index.dtype}) to {model.n_components} {'whitened ' if model.whiten else ''}components "
          f"({100 * share:.2f} % of the variance) -> {args.output}")
    index.close()
    return reduced, model


if __name__ == "__main__":
    main()
