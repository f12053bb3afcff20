"""Time of ``bn_head_i8_forward`` (the exported INT8 head over resident int8 embedding rows) next to ``bn_search_topk`` on the same rows.

    python tools/head_export_bench.py [--reps 20] [--batch 10] [--rows 1048576] [--out table.md]

Random int8 rows, D = 256, sigmoid heads of C in {16, 100, 1000} with random weights.  A cell is the median over ``--reps`` timed batches
of ``--batch`` back-to-back calls between one pair of HIP events (a single call is too short a window to time), divided by the batch,
behind three warm-up calls; the spread column is (max - min) / median over the batches.  Traffic = the rows read once per pass over the
classes plus the ``[n, C]`` float32 scores and (where asked for) the ``[n, C]`` logit bytes written; the rate is that traffic over the
time.  Next to it ``bn_search_topk`` (dot metric, 16 queries, k = 10; its score and merge kernels) over the same rows: a parent-commit
kernel with the same streamer and the same read traffic and next to nothing written.  It is a yardstick for the row stream only: what it
spends on its top-k lists is not the head's work.  Prints one JSON line per cell and a markdown table.
"""

import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "birdnet-stm32_amd")]


def timed(torch, fn, reps, batch):
    """(median seconds per call, (max - min) / median) over ``reps`` batches of ``batch`` calls, each batch between one pair of events."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / batch)
    med = statistics.median(ms)
    return med * 1e-3, (max(ms) - min(ms)) / med


def main():
    import numpy as np
    import torch

    from birdnet_stm32 import _hip
    from birdnet_stm32.conversion.head_export import quantize_head
    from birdnet_stm32.training.linear_probe import ProbeHead

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    N, D, s_in, z_in = args.rows, 256, 0.0159, -128
    ctx = _hip.Context(0, 1)
    lib, h = ctx.lib, ctx.handle
    g = torch.Generator(device="cuda").manual_seed(1)
    db = torch.randint(-128, 128, (N, D), device="cuda", generator=g, dtype=torch.int8)
    rows = []

    # the yardstick: 16 queries, dot metric
    Q, k = 16, 10
    q = db[torch.randint(0, N, (Q,), device="cuda", generator=g)].clone()
    idx = torch.empty((Q, k), dtype=torch.int32, device="cuda")
    score = torch.empty((Q, k), device="cuda")
    t, spread = timed(torch, lambda: _hip.check(lib.bn_search_topk(h, db.data_ptr(), _hip.DTYPE_I8, N, D, z_in, None, q.data_ptr(), Q, None, _hip.SEARCH_METRICS["dot"], None,
                                                            None, k, idx.data_ptr(), score.data_ptr(), None)), args.reps, args.batch)
    rows.append(dict(kernel="bn_search_topk, 16 queries", C=Q, logit_bytes=False, passes=1, ms=t * 1e3, spread=spread, rows_per_s=N / t, bytes=N * D,
                     gb_per_s=N * D / t * 1e-9))
    print(json.dumps(rows[-1]), flush=True)

    rng = np.random.default_rng(0)
    for C in (16, 100, 1000):
        head = ProbeHead(rng.normal(0, 0.1, (D, C)), rng.normal(0, 1, C), "sigmoid")
        qh = quantize_head(head, s_in, z_in, -12.0, 12.0)
        k_ = qh._constants(db.device)
        scores = torch.empty((N, C), dtype=torch.float32, device="cuda")
        logit = torch.empty((N, C), dtype=torch.int8, device="cuda")
        passes = -(-C // _hip.head_i8_pass_classes(D, C))
        for with_bytes in (False, True):
            def ours():
                _hip.check(lib.bn_head_i8_forward(h, db.data_ptr(), N, D, k_["w"].data_ptr(), k_["bias"].data_ptr(), k_["mult"].data_ptr(), k_["shift"].data_ptr(), C,
                                                  qh.z_out, k_["lut"].data_ptr(), 0, ctypes.c_float(qh.s_out), logit.data_ptr() if with_bytes else None,
                                                  scores.data_ptr(), None))

            t, spread = timed(torch, ours, args.reps, args.batch)
            traffic = N * D * passes + N * C * (5 if with_bytes else 4)
            rows.append(dict(kernel="bn_head_i8_forward", C=C, logit_bytes=with_bytes, passes=passes, ms=t * 1e3, spread=spread, rows_per_s=N / t, bytes=traffic,
                             gb_per_s=traffic / t * 1e-9))
            print(json.dumps(rows[-1]), flush=True)
        del scores, logit
        torch.cuda.empty_cache()
    lines = [f"| kernel (n = {N}, D = {D}) | C | logit bytes | class passes | ms | spread | M rows/s | GB read + written | GB/s |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['kernel']} | {r['C']} | {'yes' if r['logit_bytes'] else 'no'} | {r['passes']} | {r['ms']:.3f} | {100 * r['spread']:.1f} % | {r['rows_per_s'] * 1e-6:.0f} | "
                     f"{r['bytes'] * 1e-9:.2f} | {r['gb_per_s']:.0f} |")
    table = "\n".join(lines)
    print("\n" + table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
