"""Time of ``bn_search_topk`` against the streaming roof and against the same search written with PyTorch ops on the same GPU.

    python tools/search_bench.py [--reps 20] [--out table.md]

Random rows, D = 256, float32 and int8, N in {2^18, 2^22}, Q in {1, 16, 64}, k = 10, cosine.  A cell is the median of ``--reps`` calls
timed one by one with HIP events behind three warm-up calls (the inverse norms of the database are computed once, outside the timing, as
an index does).  The roof is the time to read the database once at the measured copy rate of the card (6.3 TB/s).  The PyTorch side
is what a user would write without the kernel: normalise the queries, one matmul against the normalised rows kept as float32, ``topk``
(for int8 rows it dequantises first: there is no int8 matmul to call).  Prints one JSON line per cell and a markdown table.
"""

import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "birdnet-stm32_amd")]

COPY_RATE = 6.3e12   # bytes per second


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


def main():
    import torch

    from birdnet_stm32 import _hip

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    D, k = 256, 10
    ctx = _hip.Context(0, 1)
    lib, h = ctx.lib, ctx.handle
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for dtype in ("float32", "int8"):
        code = _hip.DTYPE_I8 if dtype == "int8" else _hip.DTYPE_F32
        zp = -128 if dtype == "int8" else 0
        for N in (1 << 18, 1 << 22):
            if dtype == "int8":
                db = torch.randint(-128, 128, (N, D), device="cuda", generator=g, dtype=torch.int8)
            else:
                db = torch.rand((N, D), device="cuda", generator=g)
            inv = torch.empty(N, device="cuda")
            _hip.check(lib.bn_search_inv_norms(h, db.data_ptr(), code, N, D, zp, inv.data_ptr(), None))
            t_norm = timed(torch, lambda: _hip.check(lib.bn_search_inv_norms(h, db.data_ptr(), code, N, D, zp, inv.data_ptr(), None)), args.reps)
            ref = db.float() - zp if dtype == "int8" else db
            ref = ref / ref.norm(dim=1, keepdim=True).clamp_min(1e-30)   # the PyTorch side's own resident form (float32 either way)
            roof = N * D * db.element_size() / COPY_RATE
            for Q in (1, 16, 64):
                q = db[torch.randint(0, N, (Q,), device="cuda", generator=g)].clone()
                qinv = torch.empty(Q, device="cuda")
                idx = torch.empty((Q, k), dtype=torch.int32, device="cuda")
                score = torch.empty((Q, k), device="cuda")

                def ours():
                    _hip.check(lib.bn_search_inv_norms(h, q.data_ptr(), code, Q, D, zp, qinv.data_ptr(), None))
                    _hip.check(lib.bn_search_topk(h, db.data_ptr(), code, N, D, zp, inv.data_ptr(), q.data_ptr(), Q, qinv.data_ptr(), 0, None, None, k,
                                                  idx.data_ptr(), score.data_ptr(), None))

                def theirs():
                    qf = q.float() - zp if dtype == "int8" else q
                    qf = qf / qf.norm(dim=1, keepdim=True).clamp_min(1e-30)
                    return torch.topk(qf @ ref.T, k, dim=1)

                a = timed(torch, ours, args.reps)
                b = timed(torch, theirs, args.reps)
                agree = float((theirs()[1][:, 0] == idx[:, 0].long()).float().mean())   # the best hit is the query's own row on both sides
                row = dict(dtype=dtype, N=N, D=D, Q=Q, k=k, search_ms=a * 1e3, roof_ms=roof * 1e3, share_of_roof=roof / a, torch_ms=b * 1e3, torch_over_search=b / a,
                           inv_norms_ms=t_norm * 1e3, top1_agree=agree)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del db, inv, ref
            torch.cuda.empty_cache()
    lines = ["| dtype | N | Q | search ms | stream-once ms | share of roof | PyTorch ms | PyTorch / search | norms ms |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['dtype']} | 2^{r['N'].bit_length() - 1} | {r['Q']} | {r['search_ms']:.3f} | {r['roof_ms']:.3f} | {100 * r['share_of_roof']:.0f} % | "
                     f"{r['torch_ms']:.3f} | {r['torch_over_search']:.2f} | {r['inv_norms_ms']:.3f} |")
    table = "\n".join(lines)
    print("\n" + table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
