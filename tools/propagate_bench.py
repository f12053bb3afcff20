"""Time of the graph build, of one update (``bn_propagate_step``) and of a whole ``propagate_index`` run, on planted rows.

    python tools/propagate_bench.py [--reps 20] [--sizes 32768 131072] [--classes 16 64 256] [--neighbours 15] [--dim 256] [--out table.md]

float32 rows drawn around as many normal centres as there are classes; one row in a hundred is labelled.  The graph is the run's own
(``device_neighbours``, ``build_graph``).  A cell is the median of ``--reps`` calls timed one by one with HIP events behind three warm-up
calls:
  step        ``bn_propagate_step`` without the change (the update alone);
  step+delta  the same with the float64 change, its fold included;
  torch       ``torch.sparse`` CSR ``mm`` of the same matrix with the same ``F`` on the same device, the product alone, without the
              ``alpha`` / seed term: for context.  It does not give the specification's fixed order of additions, so its bits are its own.
An update reads every entry's column and value (8 bytes) and ``C`` floats of ``F`` per entry, and reads and writes a row of ``F`` per
row: ``nnz (4 C + 8) + 8 n C`` bytes, reported over the step's time as GB/s.  The rows of ``F`` that the entries name are fetched
again and again (from the caches where they fit), so this is the algorithm's traffic, not the memory's; the card's peak for
comparison is 8 TB/s.  End to end is ``propagate_index`` with 30 updates at ``tol = 0``: the upload, the neighbour search, the host's
graph and the decision included.  Nothing here is a threshold.  Prints one JSON line per shape and a markdown table.
"""

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "birdnet-stm32_amd"), os.path.join(REPO, "tools")]


def step_bytes(nnz: int, n: int, C: int) -> int:
    return nnz * (4 * C + 8) + 8 * n * C


def planted_rows(n, D, centres, seed=1):
    import numpy as np

    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, D)).astype(np.float32)
    true = rng.integers(0, centres, n)
    rows = c[true] + 0.5 * rng.standard_normal((n, D)).astype(np.float32)
    seed_label = np.full(n, -1, np.int32)
    picked = rng.choice(n, max(centres, n // 100), replace=False)
    seed_label[picked] = true[picked]
    return rows, true, seed_label


def main():
    import numpy as np
    import torch
    from project_bench import timed

    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation import propagate as P
    from birdnet_stm32.evaluation.project import device_neighbours
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[32768, 131072])
    ap.add_argument("--classes", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--neighbours", type=int, default=P.DEFAULT_NEIGHBOURS)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("propagate_bench needs the device: a time taken elsewhere says nothing")
    ctx = _hip.Context(0, 1)
    lib, h = ctx.lib, ctx.handle
    table = []
    for n in args.sizes:
        for C in args.classes:
            x, true, seed_label = planted_rows(n, args.dim, C)
            t0 = time.perf_counter()
            d_idx, d_score = device_neighbours(ctx, x, 0, args.neighbours)
            idx, score = d_idx.cpu().numpy().astype(np.int64), d_score.cpu().numpy()
            t_search = time.perf_counter() - t0
            del d_idx, d_score
            t0 = time.perf_counter()
            rowptr, col, val, _ = P.build_graph(idx, score, n, P.DEFAULT_TAU)
            t_graph = time.perf_counter() - t0
            nnz = int(rowptr[-1])
            d_rowptr, d_col, d_val, d_seed = (torch.from_numpy(a).cuda() for a in (rowptr, col, val, seed_label))
            f = torch.from_numpy(P.initial_labels(seed_label, C)).cuda()
            g = torch.empty_like(f)
            delta = torch.zeros(1, dtype=torch.float64, device="cuda")

            def step(d):
                _hip.check(lib.bn_propagate_step(h, d_rowptr.data_ptr(), d_col.data_ptr(), d_val.data_ptr(), f.data_ptr(), d_seed.data_ptr(), n, C,
                                                 _hip.c_float(P.DEFAULT_ALPHA), g.data_ptr(), d, None))

            step(None)
            f.copy_(g)   # (a matrix with more than the seeds in it)
            t_step = timed(torch, lambda: step(None), args.reps)
            t_delta = timed(torch, lambda: step(delta.data_ptr()), args.reps)
            S = torch.sparse_csr_tensor(d_rowptr, d_col.to(torch.int64), d_val, size=(n, n))
            t_torch = timed(torch, lambda: torch.sparse.mm(S, f), args.reps)
            del S, d_rowptr, d_col, d_val, d_seed, f, g
            torch.cuda.empty_cache()
            index = EmbeddingIndex(x, np.zeros(n, np.int64), np.zeros(n), ["synthetic"])
            t0 = time.perf_counter()
            res = P.propagate_index(index, seed_label, C, neighbours=args.neighbours, tol=0.0, ctx=ctx)
            t_run = time.perf_counter() - t0
            nbytes = step_bytes(nnz, n, C)
            row = dict(n=n, D=args.dim, C=C, k=args.neighbours, nnz=nnz, search_s=t_search, graph_host_s=t_graph, step_ms=t_step * 1e3, step_delta_ms=t_delta * 1e3,
                       torch_sparse_mm_ms=t_torch * 1e3, step_bytes=nbytes, step_gb_per_s=nbytes / t_step * 1e-9, n_iter=res.n_iter, end_to_end_s=t_run,
                       accuracy=float((res.labels == true).mean()))
            table.append(row)
            print(json.dumps(row), flush=True)
            del index
    lines = ["| N | C | entries of S | neighbour search s | graph on the host s | step ms | step + delta ms | torch.sparse mm ms | bytes per step | GB/s | "
             "end to end s (30 updates) |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in table:
        lines.append(f"| {r['n']} | {r['C']} | {r['nnz']} | {r['search_s']:.2f} | {r['graph_host_s']:.2f} | {r['step_ms']:.3f} | {r['step_delta_ms']:.3f} | "
                     f"{r['torch_sparse_mm_ms']:.3f} | {r['step_bytes']:.3g} | {r['step_gb_per_s']:.0f} | {r['end_to_end_s']:.2f} |")
    text = "\n".join(lines)
    print("\n" + text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
