"""Time of one silhouette pass (``bn_kmeans_accumulate`` + ``bn_silhouette_means``) against its roofs, against the same quantities written
with PyTorch ops, and — at a row count the host can hold pairwise — against ``sklearn.metrics.silhouette_samples``, on the same machine.

    python tools/silhouette_bench.py [--reps 20] [--out table.md] [--small] [--sklearn_rows 16384]

Random rows, D = 256, float32 and int8, N in {2^18, 2^22}, K in {16, 256, 1024} (``--small``: N = 2^18 only), random labels.  A cell is the
median of ``--reps`` calls timed one by one with HIP events behind three warm-up calls; the inverse norms of the rows are computed once,
outside the timing, as an index does.  Compared with
  (a) the roofs: the rows streamed once at the card's measured copy rate (6.3 TB/s), and 2 N K D flops at the measured exact-float32
      matrix-core rate (155 TFLOP/s);
  (b) the pass a user would write without the kernels: normalised rows kept as float32, ``index_add_`` for the sums (whose float atomics
      are not reproducible run to run), ``bincount``, one matmul, a gather for ``own`` and a masked ``max`` for ``other``;
  (c) scikit-learn's O(N^2 D) ``silhouette_samples(metric="cosine")`` on ``--sklearn_rows`` rows of the float32 matrix, next to
      ``silhouette_index`` on the same rows (wall clock, upload and host finish included), with the largest difference of the two.
Prints one JSON line per cell and a markdown table.
"""

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "birdnet-stm32_amd")]

COPY_RATE = 6.3e12    # bytes per second
MFMA_F32_RATE = 155e12   # flop per second, v_mfma_f32_16x16x4_f32


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


def against_sklearn(ctx, n, D, K):
    import numpy as np
    from sklearn.metrics import silhouette_samples

    from birdnet_stm32.evaluation.search import EmbeddingIndex
    from birdnet_stm32.evaluation.silhouette import silhouette_index

    rng = np.random.default_rng(3)
    C = rng.standard_normal((K, D))
    lab = rng.integers(0, K, n)
    lab[:K] = np.arange(K)
    x = (C[lab] / np.linalg.norm(C[lab], axis=1, keepdims=True) + 0.5 * rng.standard_normal((n, D)) / np.sqrt(D)).astype(np.float32)
    index = EmbeddingIndex(x, np.zeros(n, np.int64), np.zeros(n), ["rows"])
    silhouette_index(index, lab, K, ctx=ctx)   # (warm: the block is resident afterwards, as it is behind a fit)
    t0 = time.perf_counter()
    got = silhouette_index(index, lab, K, ctx=ctx)
    t_ours = time.perf_counter() - t0
    xn = x.astype(np.float64)
    xn /= np.linalg.norm(xn, axis=1, keepdims=True)
    t0 = time.perf_counter()
    want = silhouette_samples(xn, lab, metric="cosine")
    t_sk = time.perf_counter() - t0
    return dict(sklearn_rows=n, D=D, K=K, silhouette_index_ms=t_ours * 1e3, sklearn_ms=t_sk * 1e3, sklearn_over_ours=t_sk / t_ours,
                max_abs_difference=float(np.abs(got.silhouette - want).max()))


def main():
    import torch

    from birdnet_stm32 import _hip

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--small", action="store_true", help="N = 2^18 only")
    ap.add_argument("--sklearn_rows", type=int, default=16384, help="rows of the scikit-learn comparison (0: skip it)")
    args = ap.parse_args()
    D = 256
    ctx = _hip.Context(0, 1)
    lib, h = ctx.lib, ctx.handle
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for dtype in ("float32", "int8"):
        code = _hip.DTYPE_I8 if dtype == "int8" else _hip.DTYPE_F32
        zp = -128 if dtype == "int8" else 0
        for N in ((1 << 18,) if args.small else (1 << 18, 1 << 22)):
            if dtype == "int8":
                x = torch.randint(-128, 128, (N, D), device="cuda", generator=g, dtype=torch.int8)
            else:
                x = torch.rand((N, D), device="cuda", generator=g)
            inv = torch.empty(N, device="cuda")
            _hip.check(lib.bn_search_inv_norms(h, x.data_ptr(), code, N, D, zp, inv.data_ptr(), None))
            ref = x.float() - zp if dtype == "int8" else x
            ref = ref / ref.norm(dim=1, keepdim=True).clamp_min(1e-30)   # the PyTorch side's own resident form (float32 either way)
            for K in (16, 256, 1024):
                label = torch.randint(0, K, (N,), device="cuda", generator=g, dtype=torch.int32)
                lab64 = label.long()
                sums = torch.empty((K, D), device="cuda")
                counts = torch.empty(K, dtype=torch.int64, device="cuda")
                own, other = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
                nearest = torch.empty(N, dtype=torch.int32, device="cuda")

                def accumulate():
                    _hip.check(lib.bn_kmeans_accumulate(h, x.data_ptr(), code, N, D, zp, inv.data_ptr(), label.data_ptr(), K, 0, sums.data_ptr(), counts.data_ptr(), None))

                accumulate()
                weight = (1.0 / counts.double().clamp_min(1)).float() * (counts > 0)

                def means():
                    _hip.check(lib.bn_silhouette_means(h, x.data_ptr(), code, N, D, zp, inv.data_ptr(), label.data_ptr(), sums.data_ptr(), weight.data_ptr(), K,
                                                       own.data_ptr(), other.data_ptr(), nearest.data_ptr(), None))

                def theirs():
                    acc = torch.zeros((K, D), device="cuda").index_add_(0, lab64, ref)
                    n = torch.bincount(lab64, minlength=K)
                    m = (ref @ acc.T) * ((1.0 / n.clamp_min(1)) * (n > 0))[None, :]
                    o = m.gather(1, lab64[:, None])[:, 0]
                    m.scatter_(1, lab64[:, None], float("-inf"))
                    m.masked_fill_((n == 0)[None, :], float("-inf"))
                    t, near = m.max(dim=1)
                    return o, t, near

                t_acc = timed(torch, accumulate, args.reps)
                t_means = timed(torch, means, args.reps)
                t_torch = timed(torch, theirs, max(3, args.reps // 2))
                o, t, near = theirs()
                agree = float((near == nearest.long()).float().mean())
                worst = float(torch.maximum((o - own).abs().max(), (t - other).abs().max()))
                del o, t, near
                stream = N * D * x.element_size() / COPY_RATE
                mfma = 2.0 * N * K * D / MFMA_F32_RATE
                total = t_acc + t_means
                row = dict(dtype=dtype, N=N, D=D, K=K, accumulate_ms=t_acc * 1e3, means_ms=t_means * 1e3, pass_ms=total * 1e3, stream_once_ms=stream * 1e3,
                           mfma_ms=mfma * 1e3, means_share_of_roof=max(stream, mfma) / t_means, torch_ms=t_torch * 1e3, torch_over_pass=t_torch / total,
                           nearest_agree=agree, max_abs_difference_to_torch=worst)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del x, inv, ref
            torch.cuda.empty_cache()
    lines = ["| dtype | N | K | accumulate ms | means ms | pass ms | stream-once ms | 2NKD at 155 TF ms | means / roof | PyTorch ms | PyTorch / pass |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['dtype']} | 2^{r['N'].bit_length() - 1} | {r['K']} | {r['accumulate_ms']:.3f} | {r['means_ms']:.3f} | {r['pass_ms']:.3f} | "
                     f"{r['stream_once_ms']:.3f} | {r['mfma_ms']:.3f} | {100 * r['means_share_of_roof']:.0f} % | {r['torch_ms']:.3f} | {r['torch_over_pass']:.2f} |")
    if args.sklearn_rows:
        sk = against_sklearn(ctx, args.sklearn_rows, D, 16)
        print(json.dumps(sk), flush=True)
        lines += ["", f"scikit-learn on {sk['sklearn_rows']} float32 rows, K = {sk['K']}: {sk['sklearn_ms']:.1f} ms; `silhouette_index` on the same rows "
                      f"{sk['silhouette_index_ms']:.2f} ms ({sk['sklearn_over_ours']:.0f}x); largest difference {sk['max_abs_difference']:.2g}"]
    table = "\n".join(lines)
    print("\n" + table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
