"""Time of a density fit (``density_index``): the rounds of ``bn_density_nearest``, the whole fit and the host's share of it, against the
arithmetic of a round and, for context, scikit-learn's HDBSCAN on the CPU.

    python tools/density_bench.py [--sizes 16384 65536 262144] [--sklearn 16384] [--out table.md]

Rectified Gaussian blobs with a tenth of scattered rows, D = 256, float32 and the same rows as int8 bytes; ``min_cluster_size`` 15,
``min_samples`` 5.  Per cell: the number of rounds, the median over the rounds of the device time of one ``bn_density_nearest`` call
(HIP events around the call; every round multiplies all pairs, whatever the number of components), the seconds of the core scores
(``bn_search_topk``), of the tree (rounds, copies and the host's share of Borůvka), of the host hierarchy and of the whole fit, and the
round's 2 n^2 D flop over its time next to the measured exact-float32 matrix-core rate (155 TFLOP/s).  A warm-up fit at the smallest size
comes first.  ``--sklearn N`` (0: skip) runs ``sklearn.cluster.HDBSCAN`` on the normalised float32 rows of that size on the CPU, with the
same two parameters.  Prints one JSON line per cell and a markdown table.
"""

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "birdnet-stm32_amd")]

MFMA_F32_RATE = 155e12   # flop per second, v_mfma_f32_16x16x4_f32
D, BLOBS, MIN_CLUSTER_SIZE, MIN_SAMPLES = 256, 64, 15, 5


def make_rows(n, seed=1):
    import numpy as np

    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((BLOBS, D)).astype(np.float32)
    lab = rng.integers(0, BLOBS, n)
    x = cent[lab] + np.float32(0.5) * rng.standard_normal((n, D), dtype=np.float32)
    scattered = rng.random(n) < 0.1
    x[scattered] = rng.standard_normal((int(scattered.sum()), D), dtype=np.float32)
    return np.maximum(x, 0, out=x)


def to_int8(x):
    import numpy as np

    scale = float(x.max()) / 255.0
    return np.clip(np.rint(x / scale) - 128, -128, 127).astype(np.int8), scale, -128


def main():
    import numpy as np
    import torch

    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation.density import density_index
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 14, 1 << 16, 1 << 18])
    ap.add_argument("--sklearn", type=int, default=1 << 14, help="rows of the scikit-learn run on the CPU (0: skip)")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("density_bench.py measures on the GPU; there is none")
    ctx = _hip.Context(0, 1)

    def fit(x, zp=0, scale=1.0):
        n = x.shape[0]
        index = EmbeddingIndex(x, np.zeros(n, np.int64), np.zeros(n), ["bench"], scale=scale, zero_point=zp, budget_bytes=1 << 40)
        t = {}
        t0 = time.perf_counter()
        res = density_index(index, MIN_CLUSTER_SIZE, MIN_SAMPLES, ctx=ctx, timings=t)
        t["fit_s"] = time.perf_counter() - t0
        return res, t

    fit(make_rows(min(args.sizes)))   # warm-up: code objects, workspaces
    lines = ["| rows | dtype | rounds | s / round (median) | TFLOP/s of a round | cores s | tree s | hierarchy s | fit s | clusters | noise |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in args.sizes:
        x = make_rows(n)
        for dtype in ("float32", "int8"):
            rows, scale, zp = (x, 1.0, 0) if dtype == "float32" else to_int8(x)
            res, t = fit(rows, zp, scale)
            per_round = statistics.median(t["round_s"])
            cell = dict(rows=n, D=D, dtype=dtype, rounds=res.rounds, round_s=per_round, round_tflops=2.0 * n * n * D / per_round / 1e12, cores_s=t["cores_s"],
                        tree_s=t["tree_s"], hierarchy_s=t["hierarchy_s"], fit_s=t["fit_s"], clusters=res.n_clusters, noise=int((res.labels < 0).sum()),
                        mfma_f32_rate_tflops=MFMA_F32_RATE / 1e12)
            print(json.dumps(cell), flush=True)
            lines.append(f"| {n} | {dtype} | {res.rounds} | {per_round:.4f} | {cell['round_tflops']:.1f} | {t['cores_s']:.3f} | {t['tree_s']:.3f} | {t['hierarchy_s']:.3f} | "
                         f"{t['fit_s']:.3f} | {res.n_clusters} | {cell['noise']} |")
    if args.sklearn:
        from sklearn.cluster import HDBSCAN

        x = make_rows(args.sklearn)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        t0 = time.perf_counter()
        sk = HDBSCAN(min_cluster_size=MIN_CLUSTER_SIZE, min_samples=MIN_SAMPLES).fit(x)
        cell = dict(rows=args.sklearn, D=D, sklearn_cpu_fit_s=time.perf_counter() - t0, clusters=int(sk.labels_.max()) + 1, noise=int((sk.labels_ < 0).sum()),
                    cpus=os.cpu_count())
        print(json.dumps(cell), flush=True)
        lines.append(f"\nscikit-learn {args.sklearn} rows on the CPU: {cell['sklearn_cpu_fit_s']:.1f} s, {cell['clusters']} clusters, {cell['noise']} rows of noise")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
