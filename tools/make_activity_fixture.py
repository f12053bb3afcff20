"""Write tests/golden/reference_activity.json: what the reference project's ``birdnet_stm32/audio/activity.py`` returns for the seeded inputs of
tests/activity_cases.py.  Needs a checkout of the reference (``--reference DIR``); no test calls this script.

    python tools/make_activity_fixture.py --reference /path/to/reference
"""

from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import activity_cases as ac  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--output", default=os.path.join(REPO, "tests", "golden", "reference_activity.json"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_activity", os.path.join(args.reference, "birdnet_stm32", "audio", "activity.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {"numpy": np.__version__, "sample_rate": ac.SR, "chunk_duration": ac.CD, "crop": [], "activity": [], "sort": [], "ste": [], "random": []}
    for name, seed in ac.CROP_CASES:
        x = ac.crop_signal(name, seed)
        for max_chunks, pct in ((5, 75.0), (2, 75.0), (8, 90.0)):
            chunks = ref.smart_crop(x, ac.SR, ac.CD, max_chunks=max_chunks, energy_percentile=pct)
            out["crop"].append({"name": name, "seed": seed, "max_chunks": max_chunks, "energy_percentile": pct,
                                "starts": [ac.locate(c, x) for c in chunks]})
    for name, seed in ac.ACTIVITY_CASES:
        x = ac.activity_input(name, seed)
        for k, max_active, sub in ((2.0, 0.8, 512), (1.0, 0.1, 512), (3.0, 0.8, 128)):
            out["activity"].append({"name": name, "seed": seed, "k": k, "max_active": max_active, "subsample": sub,
                                    "ratio": float(ref.get_activity_ratio(x, k=k, max_active=max_active, subsample=sub))})
    for kind, seed in ac.SORT_CASES:
        samples = ac.sort_samples(seed, kind)
        for thr in (0.0, 0.05, 0.25, 2.0):
            got = ref.sort_by_activity(samples, threshold=thr)
            out["sort"].append({"fn": "sort_by_activity", "kind": kind, "seed": seed, "threshold": thr,
                                "order": [next(i for i, s in enumerate(samples) if s is g) for g in got]})
        for thr in (0.1, 0.9):
            got = ref.sort_by_s2n(samples, threshold=thr)
            out["sort"].append({"fn": "sort_by_s2n", "kind": kind, "seed": seed, "threshold": thr,
                                "order": [next(i for i, s in enumerate(samples) if s is g) for g in got]})
    for seed, n in ac.STE_CASES:
        e = ref._short_time_energy(ac.ste_signal(seed, n))
        out["ste"].append({"seed": seed, "n": n, "bits": np.asarray(e, np.float32).view(np.uint32).tolist()})
    samples = ac.sort_samples(21, "maps")
    for num, first in ((1, False), (3, False), (1, True), (4, True), (99, True)):
        np.random.seed(1234)
        got = ref.pick_random_samples(samples, num_samples=num, pick_first=first)
        got = got if isinstance(got, list) else [got]
        out["random"].append({"num_samples": num, "pick_first": first, "np_seed": 1234,
                              "picked": [next(i for i, s in enumerate(samples) if s is g) for g in got]})
    with open(args.output, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {args.output}: {os.path.getsize(args.output)} bytes")


if __name__ == "__main__":
    main()
