"""Time of ``bn_augment_inputs`` against a device-to-device copy of the same byte count and against the same augmentation written with
PyTorch ops, then probe epochs with and without augmentation.

    python tools/augment_bench.py [--reps 20] [--rows 4096] [--probe_rows 10000] [--out table.md]

Kernel: the three real row shapes (257 x 256 hybrid, 64 x 256 precomputed, 1 x 66 150 raw) at m = n_rows = ``--rows``; three mixes --
every row a copy, every row mixed from three sources, and the default mix (``augment_plan`` at the reference's defaults: a quarter of the
rows mixed, SpecAugment on the spectrogram shapes).  A cell is the median of ``--reps`` calls timed one by one with HIP events behind
three warm-up calls.  "Bytes moved" counts what the plan asks for: every source row read once per output row that uses it, every output
row written once (masked runs are counted as read: the figure is a lower bound on the rate where the kernel skips them).  The copy is
``dst.copy_(src)`` over tensors of half that byte count (read + write = the same traffic), timed in the same process.  The PyTorch side
is what a user would write without the kernel: masked fill per source table, ``index_select``, multiply, add.

Probe: ``fit_probe`` against ``fit_probe_augmented`` at the reference's defaults on ``--probe_rows`` synthetic rows through the shipped
INT8 model, seconds per epoch, with the share spent in plan + augmentation + backbone.  Prints one JSON line per cell and a markdown table.
"""

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "birdnet-stm32_amd")]

SHAPES = ((257, 256), (64, 256), (1, 66150))


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


def plans(np, n, F, W):
    from birdnet_stm32.training.augment import AugmentPlan, ProbeAugmentation, augment_plan

    own = np.arange(n, dtype=np.int32)
    copy = AugmentPlan(np.ones(n, np.int32), np.repeat(own[:, None], 3, 1), np.tile(np.array([1, 0, 0], np.float32), (n, 1)), None, None, F, W)
    rng = np.random.default_rng(0)
    src3 = np.stack([own, rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)], axis=1)
    three = AugmentPlan(np.full(n, 3, np.int32), src3, rng.dirichlet([0.2] * 3, n).astype(np.float32), None, None, F, W)
    default = augment_plan(n, F, W, ProbeAugmentation(mixup_probability=0.25, spec_augment=True), 1, 0)
    return (("all copy", copy), ("all 3-source", three), ("default mix", default))


def torch_augment(torch, x, plan, tabs, F, W):
    """The same rows from PyTorch ops (values, not bits: torch may fuse the multiply-add)."""
    n = x.shape[0]
    masked = x.view(n, F, W)
    if tabs[3] is not None or tabs[4] is not None:
        masked = masked.clone()
        f_idx, t_idx = torch.arange(F, device=x.device), torch.arange(W, device=x.device)
        for tab, idx, dim in ((tabs[3], f_idx, 1), (tabs[4], t_idx, 2)):
            if tab is None:
                continue
            for k in range(tab.shape[1]):
                hit = (idx[None, :] >= tab[:, k, 0:1]) & (idx[None, :] < tab[:, k, 0:1] + tab[:, k, 1:2])
                masked.masked_fill_(hit[:, :, None] if dim == 1 else hit[:, None, :], 0.0)
    masked = masked.view(n, -1)
    src, gain, nsrc = tabs[1].long(), tabs[2], tabs[0]
    out = masked.index_select(0, src[:, 0])
    mixed = nsrc > 1
    if bool(mixed.any()):
        rows = mixed.nonzero().squeeze(1)
        acc = masked.index_select(0, src[rows, 0]) * gain[rows, 0:1] + masked.index_select(0, src[rows, 1]) * gain[rows, 1:2]
        three = (nsrc[rows] > 2).float()[:, None]
        acc = acc + masked.index_select(0, src[rows, 2]) * (gain[rows, 2:3] * three)
        out[rows] = acc
    return out


def bench_kernel(torch, np, ctx, n, reps):
    from birdnet_stm32 import _hip

    rows = []
    for F, W in SHAPES:
        E = F * W
        x = torch.randn((n, E), device="cuda")
        out = torch.empty_like(x)
        for name, plan in plans(np, n, F, W):
            up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
            tabs = [up(a) for a in (plan.nsrc, plan.src, plan.gain, plan.fmask, plan.tmask)]
            nf, nt = (0 if a is None else a.shape[1] for a in (plan.fmask, plan.tmask))
            p = lambda t: None if t is None else t.data_ptr()  # noqa: E731

            def ours():
                _hip.check(ctx.lib.bn_augment_inputs(ctx.handle, x.data_ptr(), n, F, W, p(tabs[0]), p(tabs[1]), p(tabs[2]), p(tabs[3]), nf, p(tabs[4]), nt, n,
                                                     out.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))

            moved = (int(plan.nsrc.sum()) + n) * E * 4
            half = torch.empty(moved // 8, device="cuda")
            dst = torch.empty_like(half)
            a = timed(torch, ours, reps)
            c = timed(torch, lambda: dst.copy_(half), reps)
            t = timed(torch, lambda: torch_augment(torch, x, plan, tabs, F, W), reps)
            row = dict(shape=f"{F}x{W}", m=n, mix=name, bytes_moved=moved, kernel_ms=a * 1e3, kernel_TBps=moved / a / 1e12, copy_ms=c * 1e3,
                       copy_TBps=moved / c / 1e12, kernel_over_copy=a / c, torch_ms=t * 1e3, torch_over_kernel=t / a)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del half, dst
        del x, out
        torch.cuda.empty_cache()
    return rows


def bench_probe(torch, np, n, epochs=5):
    from birdnet_stm32.models.runners import load_model_runner
    from birdnet_stm32.training.augment import ProbeAugmentation
    from birdnet_stm32.training.linear_probe import fit_probe, fit_probe_augmented

    ckpt = os.path.join(REPO, "birdnet-stm32_amd", "checkpoints", "birdnet_stm32n6_100.tflite")
    runner = load_model_runner(ckpt, max_batch=4096)
    g = torch.Generator(device="cuda").manual_seed(2)
    inputs = torch.rand((n, runner.input_elems), device="cuda", generator=g)
    emb = torch.cat([runner.predict_device(inputs[b : b + 4096], return_embeddings=True)[1] for b in range(0, n, 4096)])
    Y = np.eye(10, dtype=np.float32)[np.random.default_rng(0).integers(0, 10, n)]
    kw = dict(epochs=epochs, batch_size=32, patience=epochs)
    out = {}
    for name, fn in (("plain", lambda: fit_probe(runner, emb, Y, **kw)),
                     ("augmented", lambda: fit_probe_augmented(runner, inputs, Y, augment=ProbeAugmentation(mixup_probability=0.25, spec_augment=True),
                                                               input_shape=runner.input_shape(), **kw))):
        fn()   # warm: code objects, workspaces
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        head = fn()
        torch.cuda.synchronize()
        out[name] = dict(epoch_ms=(time.perf_counter() - t0) / epochs * 1e3)
        aug_s = head.history.get("augment_seconds")
        if aug_s:
            out[name]["augment_reembed_ms"] = statistics.median(aug_s) * 1e3
    row = dict(probe_rows=n, epochs=epochs, **{f"{k}_{m}": v for k, d in out.items() for m, v in d.items()})
    print(json.dumps(row), flush=True)
    runner.close()
    return row


def main():
    import numpy as np
    import torch

    from birdnet_stm32 import _hip

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--probe_rows", type=int, default=10000, help="0 skips the probe epochs")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    ctx = _hip.Context(0, 1)
    rows = bench_kernel(torch, np, ctx, args.rows, args.reps)
    ctx.close()
    lines = ["| shape | mix | MB moved | kernel ms | kernel TB/s | copy ms | copy TB/s | kernel / copy | PyTorch ms | PyTorch / kernel |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['shape']} | {r['mix']} | {r['bytes_moved'] / 1e6:.0f} | {r['kernel_ms']:.3f} | {r['kernel_TBps']:.2f} | {r['copy_ms']:.3f} | "
                     f"{r['copy_TBps']:.2f} | {r['kernel_over_copy']:.2f} | {r['torch_ms']:.3f} | {r['torch_over_kernel']:.1f} |")
    if args.probe_rows > 0:
        pr = bench_probe(torch, np, args.probe_rows)
        lines += ["", f"probe, n = {pr['probe_rows']}, batch 32: plain epoch {pr['plain_epoch_ms']:.1f} ms; augmented epoch {pr['augmented_epoch_ms']:.1f} ms, of which "
                      f"plan + augment + re-embed {pr['augmented_augment_reembed_ms']:.1f} ms"]
    table = "\n".join(lines)
    print("\n" + table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
