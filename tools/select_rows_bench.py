"""Time per pick of ``bn_select_run`` and of the route the library offered before it, on planted rows.

    python tools/select_rows_bench.py [--reps 7] [--sizes 32768 131072 524288] [--budget 256] [--dim 256] [--out table.md]

float32 rows drawn around 64 normal centres (``propagate_bench.planted_rows``) and the same rows as int8 bytes (20 steps per unit, zero
point 3).  A run is the traversal from row 0 over ``--budget`` greedy picks; a cell is the median over ``--reps`` runs, each timed as a
whole with HIP events behind two warm-up runs, divided by the run's picks:
  fused     one ``bn_select_run``: a launch per pick, nothing read back;
  chained   per pick ``bn_kmeans_assign`` with one centroid gathered on the device (the row itself as float32, its inverse norm beside
            it), ``torch.maximum`` into ``m``, the taken row set to +inf, ``torch.argmax`` of ``1 - m``; the index stays on the device;
  .item()   the same with the per-pick ``.item()`` a straightforward caller would write, the gather a host-side slice.
The composed routes give the same picks where scores do not tie (``torch.argmax`` does not promise the lowest index among equals); the
tool prints how many of their picks equal the fused run's.  A pick reads every row once and reads and writes its state:
``n (D itemsize + 12)`` bytes, reported over the fused time as GB/s: the algorithm's traffic, whichever cache served it.  Nothing here is
a threshold.  Prints one JSON line per shape and a markdown table.
"""

import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "birdnet-stm32_amd"), os.path.join(REPO, "tools")]

ZERO_POINT = 3


def pick_bytes(n: int, D: int, itemsize: int) -> int:
    return n * (D * itemsize + 12)


def timed_runs(torch, run, reps):
    """Median seconds of ``run()``, whole runs between two events, behind two warm-up runs."""
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms) * 1e-3


def main():
    import numpy as np
    import torch
    from propagate_bench import planted_rows

    from birdnet_stm32 import _hip

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[32768, 131072, 524288])
    ap.add_argument("--budget", type=int, default=256)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("select_rows_bench needs the device: a time taken elsewhere says nothing")
    ctx = _hip.Context(0, 1)
    lib, h = ctx.lib, ctx.handle
    B, D = args.budget, args.dim
    table = []
    for n in args.sizes:
        x = planted_rows(n, D, 64)[0]
        for dtype in ("float32", "int8"):
            rows = x if dtype == "float32" else np.clip(np.rint(x * 20.0) + ZERO_POINT, -128, 127).astype(np.int8)
            code, zp = (_hip.DTYPE_F32, 0) if dtype == "float32" else (_hip.DTYPE_I8, ZERO_POINT)
            d_rows = torch.from_numpy(rows).cuda()
            d_inv = torch.empty(n, dtype=torch.float32, device="cuda")
            _hip.check(lib.bn_search_inv_norms(h, d_rows.data_ptr(), code, n, D, zp, d_inv.data_ptr(), None))
            d_m = torch.empty(n, dtype=torch.float32, device="cuda")
            d_nearest = torch.empty(n, dtype=torch.int32, device="cuda")
            d_picked = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
            d_key = torch.empty(B + 1, dtype=torch.float32, device="cuda")

            def fused():
                d_m.fill_(-math.inf)
                d_nearest.fill_(-1)
                d_picked[0] = 0
                _hip.check(lib.bn_select_run(h, d_rows.data_ptr(), code, n, D, zp, d_inv.data_ptr(), None, d_m.data_ptr(), d_nearest.data_ptr(),
                                             d_picked.data_ptr(), 1, B + 1, d_key.data_ptr(), None))

            d_label = torch.empty(n, dtype=torch.int32, device="cuda")
            d_score = torch.empty(n, dtype=torch.float32, device="cuda")
            d_changed = torch.zeros(1, dtype=torch.int64, device="cuda")
            trace = torch.zeros(B + 1, dtype=torch.int64, device="cuda")

            def composed(read_back):
                d_m.fill_(-math.inf)
                idx = torch.zeros(1, dtype=torch.int64, device="cuda")
                for t in range(B + 1):
                    if read_back:
                        c = int(idx.item())
                        cent, cinv = d_rows[c:c + 1], d_inv[c:c + 1]
                    else:
                        cent, cinv = d_rows.index_select(0, idx), d_inv.index_select(0, idx)
                    cent = cent.float() if dtype == "float32" else cent.float() - float(zp)
                    _hip.check(lib.bn_kmeans_assign(h, d_rows.data_ptr(), code, n, D, zp, d_inv.data_ptr(), cent.data_ptr(), cinv.data_ptr(), 1, None,
                                                    d_label.data_ptr(), d_score.data_ptr(), d_changed.data_ptr(), None))
                    torch.maximum(d_m, d_score, out=d_m)
                    d_m.index_fill_(0, idx, math.inf)
                    trace[t:t + 1] = idx
                    idx = torch.argmax(1.0 - d_m).view(1)

            t_fused = timed_runs(torch, fused, args.reps) / (B + 1)
            picks = d_picked.cpu().numpy().astype(np.int64)
            t_chain = timed_runs(torch, lambda: composed(False), args.reps) / (B + 1)
            agree = int((trace.cpu().numpy() == picks).sum())
            t_item = timed_runs(torch, lambda: composed(True), max(3, args.reps // 2)) / (B + 1)
            nbytes = pick_bytes(n, D, rows.dtype.itemsize)
            row = dict(n=n, D=D, dtype=dtype, budget=B, fused_us=t_fused * 1e6, chained_us=t_chain * 1e6, item_us=t_item * 1e6, pick_bytes=nbytes,
                       fused_gb_per_s=nbytes / t_fused * 1e-9, same_picks=agree, picks=B + 1)
            table.append(row)
            print(json.dumps(row), flush=True)
            del d_rows, d_inv, d_m, d_nearest, d_label, d_score
            torch.cuda.empty_cache()
    lines = ["| N | dtype | fused us / pick | chained us / pick | with .item() us / pick | bytes per pick | fused GB/s | composed picks equal |",
             "|---|---|---|---|---|---|---|---|"]
    for r in table:
        lines.append(f"| {r['n']} | {r['dtype']} | {r['fused_us']:.1f} | {r['chained_us']:.1f} | {r['item_us']:.1f} | {r['pick_bytes']:.3g} | "
                     f"{r['fused_gb_per_s']:.0f} | {r['same_picks']} / {r['picks']} |")
    text = "\n".join(lines)
    print("\n" + text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
