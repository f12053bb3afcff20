"""Time of the three calls of a reduction (``bn_pca_colsum``, ``bn_pca_gram``, ``bn_pca_transform``) and of a whole fit, against the
arithmetic and the bytes of the scatter matrix.

    python tools/reduce_bench.py [--sizes 16384 65536 262144] [--repeats 20] [--out table.md]

Rectified Gaussian rows around 64 centres, D = 256, r = 32, float32 and the same rows as int8 bytes, resident on the device.  Per cell: the
median, the smallest and the largest of ``--repeats`` device times of each call (HIP events around the call, behind three warm-up calls of
the same shape); the scatter matrix as ``n D^2`` multiply-adds per second next to the exact-float32 matrix-core rate it uses (155 TFLOP/s
measured = 77.5 T multiply-adds per second; the kernel multiplies the upper triangle of 64-feature tiles only, 10 of 16 at D = 256, so the
matrix cores see 5/8 of that count) and as the bytes of the rows read once per second next to HBM (8 TB/s by specification, 6.3 measured;
the kernel itself reads a row once per pair of macro tiles it takes part in, five times at D = 256); and the whole ``fit_pca`` by the host clock, copies
to the device and the eigen-decomposition included.  Prints one JSON line per cell and a markdown table.
"""

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "birdnet-stm32_amd")]

MFMA_F32_MACS = 77.5e12   # multiply-adds per second, v_mfma_f32_16x16x4_f32 (155 TFLOP/s measured)
HBM_BYTES = 8.0e12        # bytes per second by specification
D, R, BLOBS = 256, 32, 64


def make_rows(n, seed=1):
    import numpy as np

    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((BLOBS, D)).astype(np.float32)
    x = cent[rng.integers(0, BLOBS, n)] + np.float32(0.5) * rng.standard_normal((n, D), dtype=np.float32)
    return np.maximum(x, 0, out=x)


def to_int8(x):
    import numpy as np

    scale = float(x.max()) / 255.0
    return np.clip(np.rint(x / scale) - 128, -128, 127).astype(np.int8), scale, -128


def main():
    import numpy as np
    import torch

    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation.reduce import fit_pca
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 14, 1 << 16, 1 << 18])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reduce_bench.py measures on the GPU; there is none")
    ctx = _hip.Context(0, 1)
    lib, h = ctx.lib, ctx.handle

    def timed(call):
        """(median, min, max) seconds of ``--repeats`` calls by HIP events, behind three warm-up calls."""
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) / 1e3)
        return statistics.median(times), min(times), max(times)

    lines = ["| rows | dtype | colsum ms (min–max) | gram ms (min–max) | gram T multiply-adds/s (of 77.5) | gram TB/s of rows (of 8) | transform ms (min–max) | fit s |",
             "|---|---|---|---|---|---|---|---|"]
    for n in args.sizes:
        x = make_rows(n)
        for dtype in ("float32", "int8"):
            rows, scale, zp = (x, 1.0, 0) if dtype == "float32" else to_int8(x)
            code = _hip.DTYPE_I8 if dtype == "int8" else _hip.DTYPE_F32
            d_rows = torch.from_numpy(rows).cuda()
            d_sum = torch.empty(D, dtype=torch.float64, device="cuda")
            d_gram = torch.empty((D, D), dtype=torch.float64, device="cuda")
            d_mean = torch.from_numpy(rows.astype(np.float64).mean(axis=0).astype(np.float32) - np.float32(zp)).cuda()
            d_W = torch.from_numpy(np.linalg.qr(np.random.default_rng(2).standard_normal((D, R)))[0].T.astype(np.float32).copy()).cuda()
            d_out = torch.empty((n, R), dtype=torch.float32, device="cuda")
            gram_mean = d_mean.data_ptr() if dtype == "float32" else None
            col = timed(lambda: _hip.check(lib.bn_pca_colsum(h, d_rows.data_ptr(), code, n, D, zp, d_sum.data_ptr(), None)))
            gram = timed(lambda: _hip.check(lib.bn_pca_gram(h, d_rows.data_ptr(), code, n, D, zp, gram_mean, d_gram.data_ptr(), None)))
            tr = timed(lambda: _hip.check(lib.bn_pca_transform(h, d_rows.data_ptr(), code, n, D, zp, d_mean.data_ptr(), d_W.data_ptr(), R, d_out.data_ptr(), None)))
            index = EmbeddingIndex(rows, np.zeros(n, np.int64), np.zeros(n), ["bench"], scale=scale, zero_point=zp, budget_bytes=1 << 40)
            fit_pca(index, R, ctx=ctx)   # warm-up of the host side
            t0 = time.perf_counter()
            model = fit_pca(index, R, ctx=ctx)
            fit_s = time.perf_counter() - t0
            macs, byts = float(n) * D * D / gram[0], float(rows.nbytes) / gram[0]
            cell = dict(rows=n, D=D, r=R, dtype=dtype, repeats=args.repeats, colsum_s=col, gram_s=gram, transform_s=tr, gram_macs_per_s=macs,
                        gram_share_of_mfma_f32=macs / MFMA_F32_MACS, gram_row_bytes_per_s=byts, gram_share_of_hbm=byts / HBM_BYTES, fit_s=fit_s,
                        explained=float(model.explained_variance.sum() / model.total_variance))
            print(json.dumps(cell), flush=True)
            ms = lambda t: f"{1e3 * t[0]:.3f} ({1e3 * t[1]:.3f}–{1e3 * t[2]:.3f})"   # noqa: E731
            lines.append(f"| {n} | {dtype} | {ms(col)} | {ms(gram)} | {macs / 1e12:.1f} | {byts / 1e12:.2f} | {ms(tr)} | {fit_s:.3f} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
