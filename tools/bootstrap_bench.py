#!/usr/bin/env python3
"""Bootstrap AP intervals: ``metrics.bootstrap_ap_ci`` (scikit-learn per resample, the reference's path) against
``bootstrap.bootstrap_ap_ci_device`` (csrc/bn_bootstrap.hip) on the same arrays in the same process.

    python tools/bootstrap_bench.py [--sizes 4096x100x1000,...] [--host_resamples 20] [--repeats 5] [--host_repeats 3]

Scores are seeded and lie on the 1/256 lattice the INT8 model emits (long runs of equal scores); one positive class per row, as
``evaluate`` builds ``y_true``.  The host's time is linear in the resample count and, at the default 1000, two minutes per size, so it is
measured at ``--host_resamples`` and the device is measured twice: at that same count (the like-for-like ratio, and the two results are
compared there) and at the size's full count.  One warm-up call each, then the median of the repeats; the device calls end with their
results on the host, so the time includes the sort, the rejection scan, the copies and the percentiles.

One JSON object on stdout (the last line); a table on stderr.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "birdnet-stm32_amd"))

import numpy as np  # noqa: E402


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def make_inputs(rows: int, classes: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    label = rng.integers(0, classes, size=rows)
    y_true = np.zeros((rows, classes), np.float32)
    y_true[np.arange(rows), label] = 1.0
    raw = rng.random((rows, classes)) ** 4 * 0.6
    raw[np.arange(rows), label] += rng.random(rows) * 0.5
    return y_true, (np.floor(np.clip(raw, 0, 255 / 256) * 256) / 256).astype(np.float32)


def timed(fn, repeats: int) -> tuple[float, object]:
    out = fn()  # warm-up
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096x100x1000,1024x100x1000,16384x100x1000,32768x20x1000,4097x100x1000",
                    help="comma-separated rows x classes x resamples")
    ap.add_argument("--host_resamples", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host_repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation import bootstrap as bs
    from birdnet_stm32.evaluation.metrics import bootstrap_ap_ci

    warnings.simplefilter("ignore", UserWarning)
    ctx = _hip.Context(args.device, 1)
    rows_out = []
    log(f"{'rows x classes':>16} {'resamples':>9} {'host s':>9} {'device s':>9} {'ratio':>8}   {'full':>6} {'device s':>9} {'host s (scaled)':>15}  max|diff|")
    for spec in args.sizes.split(","):
        n, c, b = (int(v) for v in spec.split("x"))
        yt, ys = make_inputs(n, c)
        names = [f"c{i}" for i in range(c)]
        hb = min(b, args.host_resamples)
        t_host, want = timed(lambda: bootstrap_ap_ci(yt, ys, names, n_bootstrap=hb), args.host_repeats)
        t_dev, got = timed(lambda: bs.bootstrap_ap_ci_device(yt, ys, names, n_bootstrap=hb, ctx=ctx), args.repeats)
        diff = max(max(abs(g["ci_lower"] - w["ci_lower"]), abs(g["ci_upper"] - w["ci_upper"])) for g, w in zip(got, want))
        same_ap = all(g["ap"] == w["ap"] for g, w in zip(got, want))
        t_full, _ = timed(lambda: bs.bootstrap_ap_ci_device(yt, ys, names, n_bootstrap=b, ctx=ctx), args.repeats)
        rec = {"rows": n, "classes": c, "host_resamples": hb, "host_s": t_host, "device_s": t_dev, "ratio": t_host / t_dev, "resamples": b,
               "device_full_s": t_full, "host_full_s_scaled": t_host * b / hb, "max_abs_diff": diff, "tolerance": bs.ap_tolerance(n), "ap_equal": same_ap,
               "within_tolerance": bool(diff <= bs.ap_tolerance(n))}
        rows_out.append(rec)
        log(f"{n:>9} x {c:<4} {hb:>9} {t_host:>9.3f} {t_dev:>9.4f} {t_host / t_dev:>8.1f}   {b:>6} {t_full:>9.4f} {t_host * b / hb:>15.1f}  {diff:.2e}")
    ctx.close()
    print(json.dumps({"bench": "bootstrap_ap_ci", "repeats": args.repeats, "host_repeats": args.host_repeats, "sizes": rows_out}))


if __name__ == "__main__":
    main()
