"""Time of one t-SNE iteration (``bn_tsne_gradient`` + ``bn_tsne_update``), split into repulsion, attraction and update, and of a whole
``project_index`` fit, on synthetic rows.

    python tools/project_bench.py [--reps 10] [--n_iter 1000] [--sizes 4096 32768 131072] [--out table.md] [--sklearn]

D = 256, float32 rows drawn around 64 normal centres, perplexity 30 (k = 90).  The neighbours, the affinities and the symmetrised matrix
are the fit's own (``device_affinities``, ``symmetrize``); the map is the fit's start scaled to unit size.  A cell is the median of ``--reps``
calls timed one by one with HIP events behind three warm-up calls:
  repulsion   ``bn_tsne_gradient`` with an empty matrix P: the all-pairs kernel, the fold of its column ranges, Z and the row pass;
  attraction  ``bn_tsne_gradient`` with the real P, minus the above;
  update      ``bn_tsne_update``.
Pairs per second are n (n - 1) over the repulsion time.  The repulsion kernel spends 13 float32 operations on a pair (two differences, two
fused multiply-adds for 1 + d^2, a reciprocal, a product, an addition and two fused accumulations), so its share of the card's float32
vector peak (157.3 TFLOP/s) is 13 * pairs per second / 157.3e12.  End to end is ``project_index`` with ``--n_iter`` iterations, the upload,
the neighbour search, the host's symmetrisation and the final divergence included.  ``--sklearn`` adds scikit-learn's
``TSNE(method="exact")`` on the host's CPUs at the smallest size, for context only.  Nothing here is a threshold.
Prints one JSON line per size and a markdown table.
"""

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "birdnet-stm32_amd")]

FP32_VECTOR_PEAK = 157.3e12   # flop per second
FLOPS_PER_PAIR = 13


def timed(torch, fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms) * 1e-3


def synthetic_rows(n, D=256, centres=64, seed=1):
    import numpy as np

    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, D)).astype(np.float32)
    return c[rng.integers(0, centres, n)] + 0.5 * rng.standard_normal((n, D)).astype(np.float32)


def main():
    import numpy as np
    import torch

    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation import project
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n_iter", type=int, default=1000)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 32768, 131072])
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--sklearn", action="store_true", help="also time scikit-learn's exact t-SNE on the host at the smallest size")
    args = ap.parse_args()
    ctx = _hip.Context(0, 1)
    lib, h = ctx.lib, ctx.handle
    perplexity, k = 30.0, 90
    rows = []
    for n in args.sizes:
        x = synthetic_rows(n)
        t0 = time.perf_counter()
        idx, p_cond, _ = project.device_affinities(ctx, x, 0, k, perplexity)
        t_aff = time.perf_counter() - t0
        t0 = time.perf_counter()
        rowptr, col, val = project.symmetrize(idx, p_cond, n)
        t_sym = time.perf_counter() - t0
        y = torch.from_numpy(project.initial_map(n, 42) * np.float32(1e4)).cuda()
        d_rowptr, d_col, d_val = (torch.from_numpy(a).cuda() for a in (rowptr, col, val))
        d_empty = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        grad, upd, gains = torch.zeros_like(y), torch.zeros_like(y), torch.ones_like(y)
        z = torch.zeros(1, dtype=torch.float64, device="cuda")
        y2 = y.clone()

        def gradient(rp):
            _hip.check(lib.bn_tsne_gradient(h, y.data_ptr(), n, rp.data_ptr(), d_col.data_ptr(), d_val.data_ptr(), 1.0, grad.data_ptr(), z.data_ptr(), None, None))

        t_rep = timed(torch, lambda: gradient(d_empty), args.reps)
        t_full = timed(torch, lambda: gradient(d_rowptr), args.reps)
        t_upd = timed(torch, lambda: _hip.check(lib.bn_tsne_update(h, y2.data_ptr(), grad.data_ptr(), upd.data_ptr(), gains.data_ptr(), n, 0.0, 0.5, None)), args.reps)
        del d_rowptr, d_col, d_val, d_empty, grad, upd, gains, y, y2
        torch.cuda.empty_cache()
        index = EmbeddingIndex(x, np.zeros(n, np.int64), np.zeros(n), ["synthetic"])
        t0 = time.perf_counter()
        res = project.project_index(index, perplexity=perplexity, n_iter=args.n_iter, ctx=ctx)
        t_fit = time.perf_counter() - t0
        pairs = n * (n - 1) / t_rep
        row = dict(n=n, D=256, nnz=int(rowptr[-1]), repulsion_ms=t_rep * 1e3, attraction_ms=(t_full - t_rep) * 1e3, update_ms=t_upd * 1e3,
                   iteration_ms=(t_full + t_upd) * 1e3, pairs_per_s=pairs, share_of_fp32_vector_peak=FLOPS_PER_PAIR * pairs / FP32_VECTOR_PEAK,
                   affinities_s=t_aff, symmetrize_s=t_sym, n_iter=args.n_iter, end_to_end_s=t_fit, kl=res.kl, sklearn_exact_s=None)
        if args.sklearn and n == min(args.sizes):
            from sklearn.manifold import TSNE

            t0 = time.perf_counter()
            TSNE(method="exact", perplexity=perplexity, max_iter=args.n_iter, init="random", random_state=0).fit_transform(x)
            row["sklearn_exact_s"] = time.perf_counter() - t0
        rows.append(row)
        print(json.dumps(row), flush=True)
        del index
    lines = ["| N | entries of P | repulsion ms | attraction ms | update ms | iteration ms | pairs / s | share of 157.3 TFLOP/s | "
             f"end to end s ({args.n_iter} iterations) | scikit-learn exact, host CPUs s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        sk = "-" if r["sklearn_exact_s"] is None else f"{r['sklearn_exact_s']:.0f}"
        lines.append(f"| {r['n']} | {r['nnz']} | {r['repulsion_ms']:.3f} | {r['attraction_ms']:.3f} | {r['update_ms']:.3f} | {r['iteration_ms']:.3f} | "
                     f"{r['pairs_per_s']:.3g} | {100 * r['share_of_fp32_vector_peak']:.0f} % | {r['end_to_end_s']:.1f} | {sk} |")
    table = "\n".join(lines)
    print("\n" + table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
