"""Time of one k-means iteration (``bn_kmeans_assign`` + ``bn_kmeans_accumulate`` + ``bn_kmeans_centroids``) against its roofs, against
the same iteration written with PyTorch ops, and against ``bn_search_topk`` with the roles swapped, on the same GPU.

    python tools/cluster_bench.py [--reps 20] [--out table.md] [--small]

Random rows, D = 256, float32 and int8, N in {2^18, 2^22}, K in {16, 256, 1024} (``--small``: N = 2^18 only).  A cell is the median of
``--reps`` calls timed one by one with HIP events behind three warm-up calls; the inverse norms of the rows are computed once, outside the
timing, as an index does.  Compared with
  (a) the roofs: the rows streamed once at the card's measured copy rate (6.3 TB/s), and 2 N K D flops at the measured exact-float32
      matrix-core rate (155 TFLOP/s);
  (b) the iteration a user would write without the kernels: normalised rows kept as float32, one matmul, ``argmax``, ``index_add_`` (whose
      float atomics are not reproducible run to run), normalise;
  (c) for the assignment alone, ``bn_search_topk`` with the centroids as the database, the rows as the queries and k = 1 (float32 only:
      it wants both sides of one dtype).
Prints one JSON line per cell and a markdown table.
"""

import argparse
import json
import os
import statistics
import sys

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


def main():
    import torch

    from birdnet_stm32 import _hip

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--small", action="store_true", help="N = 2^18 only")
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
                C = ref[torch.randint(0, N, (K,), device="cuda", generator=g)].clone()
                cinv = torch.empty(K, device="cuda")
                _hip.check(lib.bn_search_inv_norms(h, C.data_ptr(), _hip.DTYPE_F32, K, D, 0, cinv.data_ptr(), None))
                label = torch.empty(N, dtype=torch.int32, device="cuda")
                prev = torch.zeros(N, dtype=torch.int32, device="cuda")
                score = torch.empty(N, device="cuda")
                changed = torch.zeros(1, dtype=torch.int64, device="cuda")
                sums = torch.empty((K, D), device="cuda")
                counts = torch.empty(K, dtype=torch.int64, device="cuda")
                C2, cinv2 = C.clone(), cinv.clone()

                def assign():
                    _hip.check(lib.bn_kmeans_assign(h, x.data_ptr(), code, N, D, zp, inv.data_ptr(), C.data_ptr(), cinv.data_ptr(), K, prev.data_ptr(), label.data_ptr(),
                                                    score.data_ptr(), changed.data_ptr(), None))

                def update():
                    _hip.check(lib.bn_kmeans_accumulate(h, x.data_ptr(), code, N, D, zp, inv.data_ptr(), label.data_ptr(), K, 0, sums.data_ptr(), counts.data_ptr(), None))
                    _hip.check(lib.bn_kmeans_centroids(h, sums.data_ptr(), counts.data_ptr(), K, D, C2.data_ptr(), cinv2.data_ptr(), None))

                def theirs():
                    s = ref @ C.T
                    best, lab = s.max(dim=1)
                    acc = torch.zeros((K, D), device="cuda").index_add_(0, lab, ref)
                    return lab, acc / acc.norm(dim=1, keepdim=True).clamp_min(1e-30)

                t_assign = timed(torch, assign, args.reps)
                t_update = timed(torch, update, args.reps)
                t_torch = timed(torch, theirs, args.reps)
                agree = float((theirs()[0] == label.long()).float().mean())
                t_swapped, swapped_agree = None, None
                if dtype == "float32":
                    idx = torch.empty((N, 1), dtype=torch.int32, device="cuda")
                    sc = torch.empty((N, 1), device="cuda")

                    def swapped():   # (2^20 queries per call: a call's query passes are one grid dimension)
                        for q0 in range(0, N, 1 << 20):
                            nq = min(1 << 20, N - q0)
                            _hip.check(lib.bn_search_topk(h, C.data_ptr(), code, K, D, 0, cinv.data_ptr(), x[q0:].data_ptr(), nq, inv[q0:].data_ptr(), 0, None, None, 1,
                                                          idx[q0:].data_ptr(), sc[q0:].data_ptr(), None))

                    t_swapped = timed(torch, swapped, max(3, args.reps // 4))
                    swapped_agree = float((idx[:, 0] == label).float().mean())
                    del idx, sc
                stream = N * D * x.element_size() / COPY_RATE
                mfma = 2.0 * N * K * D / MFMA_F32_RATE
                it = t_assign + t_update
                row = dict(dtype=dtype, N=N, D=D, K=K, assign_ms=t_assign * 1e3, update_ms=t_update * 1e3, iteration_ms=it * 1e3, stream_once_ms=stream * 1e3,
                           mfma_ms=mfma * 1e3, assign_share_of_roof=max(stream, mfma) / t_assign, torch_ms=t_torch * 1e3, torch_over_iteration=t_torch / it,
                           swapped_search_ms=None if t_swapped is None else t_swapped * 1e3, swapped_over_assign=None if t_swapped is None else t_swapped / t_assign,
                           label_agree=agree, swapped_agree=swapped_agree)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del x, inv, ref
            torch.cuda.empty_cache()
    lines = ["| dtype | N | K | assign ms | update ms | iteration ms | stream-once ms | 2NKD at 155 TF ms | assign / roof | PyTorch ms | PyTorch / iteration | "
             "swapped search ms | swapped / assign |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        sw = "-" if r["swapped_search_ms"] is None else f"{r['swapped_search_ms']:.3f}"
        so = "-" if r["swapped_over_assign"] is None else f"{r['swapped_over_assign']:.1f}"
        lines.append(f"| {r['dtype']} | 2^{r['N'].bit_length() - 1} | {r['K']} | {r['assign_ms']:.3f} | {r['update_ms']:.3f} | {r['iteration_ms']:.3f} | "
                     f"{r['stream_once_ms']:.3f} | {r['mfma_ms']:.3f} | {100 * r['assign_share_of_roof']:.0f} % | {r['torch_ms']:.3f} | {r['torch_over_iteration']:.2f} | {sw} | {so} |")
    table = "\n".join(lines)
    print("\n" + table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
