"""Steps per second and seconds per epoch of ``fit_probe`` against the same training step written with PyTorch ops on the same GPU.

    python tools/probe_bench.py [--rows 262144] [--epochs 2]

D = 256, C in {12, 100, 1000}, batch in {32, 512, 4096}, random rows.  The PyTorch side is what a user would write without the device
fit: gather, dropout, ``torch.nn.functional.linear``, sigmoid + binary cross-entropy, backward, ``clip_grad_norm_``, ``torch.optim.Adam``
with a cosine schedule.  Both sides are timed over whole epochs (first epoch discarded as warm-up), synchronised at the epoch's end only.
Prints one JSON line per cell and a markdown table.

    python tools/probe_bench.py --loss focal [--focal_gamma 2.0] [--row_weights] [--skip_torch]

The same cells with the device fit on the focal loss and / or with one weight per row (uniform in [0.5, 4), ``bn_probe_epoch_weighted``):
the forward kernel's other instantiation (csrc/bn_probe_step.h, EXT = 1).  The PyTorch side stays the plain cross-entropy step, for
scale; ``--skip_torch`` leaves it out.

    python tools/probe_bench.py --sweep 4,16,64 [--rows 262144] [--repeats 3] [--classes 12,100,1000] [--batches 32,512,4096]

One sweep of T trials (``fit_probe_sweep``'s backend, ``bn_probe_sweep_*``) against T single fits one after another (``bn_probe_*``) in the
same process: per cell one warm-up epoch of each side, then ``--repeats`` timed epochs of each, alternating.  An epoch is timed from the
permutation's upload to the step losses on the host, as the fit runs it.  Reports the median and the spread (min .. max) of both sides and
the ratio of the medians.

    python tools/probe_bench.py --qat [--rows 262144] [--large_rows 16384] [--repeats 5]

An epoch of the quantisation-aware fine-tune (``fit_probe_qat``'s backend: ``bn_probe_set_qat`` with per-class weights and quantised logits,
DESIGN.md §5j) against the plain ``bn_probe_epoch`` on the same rows in the same process: D = 256, C in {16, 100, 1000}, batch 32 and 512,
and the largest head the device takes (D = 2048, C = 4096, over ``--large_rows`` rows), where the two weight kernels in front of every
forward pass over 8.4 M weights.  Per cell one warm-up epoch of each side, then ``--repeats`` timed epochs of each, alternating; median,
spread (min .. max) and the ratio of the medians.

    python tools/probe_bench.py --hidden 64 [--classes 12,100] [--batches 32,512] [--rows 262144] [--epochs 2]

The step of a head with one hidden layer of H units (``fit_probe(hidden_units=H)``'s backend, ``bn_probe_mlp_*``), timed as
the linear step is: whole epochs, first one discarded.  Next to it the same step in PyTorch ops (dropout, linear, ReLU, dropout, linear,
the rest as above) and, for context, the linear step (``bn_probe_*``) on the same rows in the same process.
"""

import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "birdnet-stm32_amd")]


def torch_epoch_fn(torch, X, Y, C, batch, total_steps, hidden=0):
    if hidden:
        return torch_mlp_epoch_fn(torch, X, Y, C, batch, total_steps, hidden)
    lin = torch.nn.Linear(X.shape[1], C, device=X.device)
    opt = torch.optim.Adam(lin.parameters(), lr=1e-3, eps=1e-7)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, total_steps)
    drop = torch.nn.Dropout(0.5)

    def epoch(perm):
        for s in range(0, X.shape[0], batch):
            idx = perm[s : s + batch]
            loss = torch.nn.functional.binary_cross_entropy(torch.sigmoid(torch.nn.functional.linear(drop(X[idx]), lin.weight, lin.bias)), Y[idx])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(lin.parameters(), 1.0)
            opt.step()
            sched.step()
        torch.cuda.synchronize()

    return epoch


def torch_mlp_epoch_fn(torch, X, Y, C, batch, total_steps, hidden):
    net = torch.nn.Sequential(torch.nn.Dropout(0.5), torch.nn.Linear(X.shape[1], hidden), torch.nn.ReLU(), torch.nn.Dropout(0.5),
                              torch.nn.Linear(hidden, C)).to(X.device)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, eps=1e-7)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, total_steps)

    def epoch(perm):
        for s in range(0, X.shape[0], batch):
            idx = perm[s : s + batch]
            loss = torch.nn.functional.binary_cross_entropy(torch.sigmoid(net(X[idx])), Y[idx])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
            opt.step()
            sched.step()
        torch.cuda.synchronize()

    return epoch


def sweep_main(args):
    import numpy as np
    import torch

    from birdnet_stm32 import _hip
    from birdnet_stm32.training import linear_probe as lp

    n, D = args.rows, 256
    ctx = _hip.Context(0, 1)
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.rand((n, D), device="cuda", generator=g)
    rows = []
    for C in [int(v) for v in args.classes.split(",")]:
        Y = torch.zeros((n, C), device="cuda")
        Y[torch.arange(n, device="cuda"), torch.randint(0, C, (n,), device="cuda", generator=g)] = 1.0
        for batch in [int(v) for v in args.batches.split(",")]:
            steps = math.ceil(n / batch)
            plan = lp._plan_fit(X, Y, None, device=True, activation="sigmoid", optimizer="adam", batch_size=batch, dropout=0.5, epochs=args.repeats + 1,
                                learning_rate=1e-3, weight_decay=0.0, clipnorm=1.0, seed=1)
            for T in [int(v) for v in args.sweep.split(",")]:
                trials = [lp.ProbeTrial(learning_rate=1e-3, optimizer="adam", dropout=0.5, clipnorm=1.0)] * T
                singles = [lp._DeviceBackend(ctx, X, Y, None, None, plan) for _ in range(T)]
                sweep = lp._SweepBackend(ctx, X, Y, None, None, plan, trials)
                active = np.ones(T, bool)
                seq, par = [], []
                for e in range(args.repeats + 1):
                    perm = lp.epoch_permutation(1, e, n)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for be in singles:
                        be.epoch(perm)
                    seq.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    losses = sweep.epoch(perm, active)
                    par.append(time.perf_counter() - t0)
                same = bool(np.array_equal(losses[:, 0], singles[0].step_loss.cpu().numpy()))
                for be in singles + [sweep]:
                    be.close()
                seq, par = sorted(seq[1:]), sorted(par[1:])
                row = dict(D=D, C=C, batch=batch, T=T, steps_per_epoch=steps, sequential_s=float(np.median(seq)), sequential_min=seq[0], sequential_max=seq[-1],
                           sweep_s=float(np.median(par)), sweep_min=par[0], sweep_max=par[-1], ratio=float(np.median(seq) / np.median(par)),
                           sweep_trial_steps_per_s=T * steps / float(np.median(par)), same_losses=same)
                rows.append(row)
                print(json.dumps(row), flush=True)
    print("\n| C | batch | T | T fits one by one, s/epoch (min .. max) | one sweep, s/epoch (min .. max) | ratio | trial-steps/s in the sweep |\n|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['C']} | {r['batch']} | {r['T']} | {r['sequential_s']:.3f} ({r['sequential_min']:.3f} .. {r['sequential_max']:.3f}) | "
              f"{r['sweep_s']:.3f} ({r['sweep_min']:.3f} .. {r['sweep_max']:.3f}) | {r['ratio']:.2f} | {r['sweep_trial_steps_per_s']:.0f} |")
    ctx.close()


def qat_main(args):
    import numpy as np
    import torch

    from birdnet_stm32 import _hip
    from birdnet_stm32.training import linear_probe as lp
    from birdnet_stm32.training import probe_qat as pq

    ctx = _hip.Context(0, 1)
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for D, C, n in [(256, 16, args.rows), (256, 100, args.rows), (256, 1000, args.rows), (2048, 4096, args.large_rows)]:
        X = torch.rand((n, D), device="cuda", generator=g)
        Y = torch.zeros((n, C), device="cuda")
        Y[torch.arange(n, device="cuda"), torch.randint(0, C, (n,), device="cuda", generator=g)] = 1.0
        head = lp.ProbeHead(*lp.init_head(D, C, 1))
        for batch in (32, 512):
            steps = math.ceil(n / batch)
            kw = dict(optimizer="adam", batch_size=batch, dropout=0.5, epochs=args.repeats + 1, learning_rate=1e-4, weight_decay=0.0, clipnorm=1.0, seed=1)
            plan = pq._plan_qat(X, Y, None, head, True, kw)
            plain = lp._DeviceBackend(ctx, X, Y, None, None, plan)
            qat = pq._QatDeviceBackend(ctx, X, Y, None, None, plan, False, True, 16.0 / 255.0, 0)   # logits in [-8, 8]
            a, b = [], []
            for e in range(args.repeats + 1):
                perm = lp.epoch_permutation(1, e, n)
                for be, times in ((plain, a), (qat, b)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    be.epoch(perm)   # (uploads the permutation, reads the step losses back: synchronises)
                    times.append(time.perf_counter() - t0)
            plain.close()
            qat.close()
            a, b = sorted(a[1:]), sorted(b[1:])
            row = dict(D=D, C=C, batch=batch, rows=n, steps_per_epoch=steps, plain_s=float(np.median(a)), plain_min=a[0], plain_max=a[-1],
                       qat_s=float(np.median(b)), qat_min=b[0], qat_max=b[-1], ratio=float(np.median(b) / np.median(a)),
                       plain_us_per_step=1e6 * float(np.median(a)) / steps, qat_us_per_step=1e6 * float(np.median(b)) / steps)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del X, Y
    print("\n| D | C | batch | plain epoch, s (min .. max) | QAT epoch, s (min .. max) | plain, us/step | QAT, us/step | ratio |\n|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['D']} | {r['C']} | {r['batch']} | {r['plain_s']:.3f} ({r['plain_min']:.3f} .. {r['plain_max']:.3f}) | "
              f"{r['qat_s']:.3f} ({r['qat_min']:.3f} .. {r['qat_max']:.3f}) | {r['plain_us_per_step']:.1f} | {r['qat_us_per_step']:.1f} | {r['ratio']:.2f} |")
    ctx.close()


def main():
    import numpy as np
    import torch

    from birdnet_stm32 import _hip
    from birdnet_stm32.training import linear_probe as lp

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--epochs", type=int, default=2, help="timed epochs per cell (one more runs first as warm-up)")
    ap.add_argument("--loss", type=str, default="auto", choices=["auto", "focal"], help="the device fit's loss (not with --sweep)")
    ap.add_argument("--focal_gamma", type=float, default=2.0)
    ap.add_argument("--row_weights", action="store_true", help="the device fit with one weight per row (not with --sweep)")
    ap.add_argument("--skip_torch", action="store_true", help="time the device fit only")
    ap.add_argument("--sweep", type=str, default="", help="trial counts, e.g. 4,16,64: time one sweep of T trials against T fits one after another")
    ap.add_argument("--repeats", type=int, default=3, help="with --sweep: timed epochs per side and cell (one more runs first as warm-up)")
    ap.add_argument("--classes", type=str, default="12,100,1000", help="with --sweep: class counts")
    ap.add_argument("--batches", type=str, default="32,512,4096", help="with --sweep: batch sizes")
    ap.add_argument("--qat", action="store_true", help="time an epoch of the quantisation-aware fine-tune against the plain epoch (uses --rows, --repeats)")
    ap.add_argument("--large_rows", type=int, default=16384, help="with --qat: rows of the D = 2048, C = 4096 cell")
    ap.add_argument("--hidden", type=int, default=0, help="time the step of a head with this many hidden units (cells: --classes x --batches)")
    args = ap.parse_args()
    if args.qat:
        return qat_main(args)
    if args.sweep:
        return sweep_main(args)
    n, D = args.rows, 256
    ctx = _hip.Context(0, 1)
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.rand((n, D), device="cuda", generator=g)
    weights = np.random.default_rng(1).uniform(0.5, 4.0, n).astype(np.float32) if args.row_weights else None
    rows = []
    cells_C, cells_batch = ([int(v) for v in a.split(",")] for a in (args.classes, args.batches)) if args.hidden else ((12, 100, 1000), (32, 512, 4096))
    for C in cells_C:
        Y = torch.zeros((n, C), device="cuda")
        Y[torch.arange(n, device="cuda"), torch.randint(0, C, (n,), device="cuda", generator=g)] = 1.0
        for batch in cells_batch:
            steps = math.ceil(n / batch)
            total = steps * (args.epochs + 1)
            plan = lp._plan_fit(X, Y, None, device=True, activation="sigmoid", optimizer="adam", batch_size=batch, dropout=0.5, epochs=args.epochs + 1,
                                learning_rate=1e-3, weight_decay=0.0, clipnorm=1.0, seed=1, loss=args.loss, focal_gamma=args.focal_gamma,
                                sample_weight=weights, hidden_units=args.hidden)
            be = (lp._MlpDeviceBackend if args.hidden else lp._DeviceBackend)(ctx, X, Y, None, None, plan)
            lin = lp._DeviceBackend(ctx, X, Y, None, None, lp._plan_fit(X, Y, None, device=True, activation="sigmoid", optimizer="adam", batch_size=batch,
                                                                       dropout=0.5, epochs=args.epochs + 1, seed=1)) if args.hidden else None
            ours, linear = [], []
            for e in range(args.epochs + 1):
                perm = lp.epoch_permutation(1, e, n)
                t0 = time.perf_counter()
                be.epoch(perm)   # (uploads the permutation, reads the step losses back: synchronises)
                ours.append(time.perf_counter() - t0)
                if lin is not None:
                    t0 = time.perf_counter()
                    lin.epoch(perm)
                    linear.append(time.perf_counter() - t0)
            be.close()
            if lin is not None:
                lin.close()
            ep = torch_epoch_fn(torch, X, Y, C, batch, total, args.hidden)
            theirs = []
            for e in range(0 if args.skip_torch else args.epochs + 1):
                perm = torch.from_numpy(lp.epoch_permutation(1, e, n).astype(np.int64)).cuda()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ep(perm)
                theirs.append(time.perf_counter() - t0)
            a, b = min(ours[1:]), min(theirs[1:]) if theirs else float("nan")
            row = dict(D=D, C=C, batch=batch, loss=args.loss, row_weights=bool(args.row_weights), steps_per_epoch=steps, fit_probe_s_per_epoch=a, fit_probe_steps_per_s=steps / a, torch_s_per_epoch=b,
                       torch_steps_per_s=steps / b, speedup=b / a)
            if args.hidden:
                row.update(hidden=args.hidden, linear_steps_per_s=steps / min(linear[1:]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    extra = ("H | ", "---|", " linear step, steps/s |", "---|") if args.hidden else ("", "", "", "")
    print(f"\n| {extra[0]}C | batch | fit_probe steps/s | s/epoch | PyTorch steps/s | s/epoch | ratio |{extra[2]}\n|{extra[1]}---|---|---|---|---|---|---|{extra[3]}")
    for r in rows:
        print((f"| {r['hidden']} " if args.hidden else "") + f"| {r['C']} | {r['batch']} | {r['fit_probe_steps_per_s']:.0f} | {r['fit_probe_s_per_epoch']:.3f} | "
              f"{r['torch_steps_per_s']:.0f} | {r['torch_s_per_epoch']:.3f} | {r['speedup']:.2f} |" + (f" {r['linear_steps_per_s']:.0f} |" if args.hidden else ""))
    ctx.close()


if __name__ == "__main__":
    main()
