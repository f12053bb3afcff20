#!/usr/bin/env python3
"""Where i8_tail2_kernel's wave time goes: in-kernel time stamps per block and wave (the measurement build of the same sources).

    make -C birdnet-stm32_amd/csrc stamps        # lib/libbirdnet_hip_stamps.so (-DBN_TAIL_STAMPS), in the build container
    python tools/tail2_stamps.py > profiles/r05_i8_tail2_attribution.md      # on the GPU box
    python tools/tail2_stamps.py split > profiles/r06_mid2_tail2_barrier_split.md

``split``: both fused kernels in their STAGED forms (``i8_mid_split`` = 0 for ``i8_mid2_kernel``); a wave's wait at the middle and at the end
barrier of every block is divided into (a) until the last wave of its OWN chunk slot arrived and (b) from then until the last wave of the
workgroup arrived.  The stamped build puts a chunk barrier in front of each workgroup barrier and stamps between the two.
"""
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["BIRDNET_HIP_LIB"] = os.path.join(REPO, "birdnet-stm32_amd", "lib", "libbirdnet_hip_stamps.so")
sys.path[:0] = [REPO, os.path.join(REPO, "birdnet-stm32_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from birdnet_stm32 import _hip  # noqa: E402
from birdnet_stm32.models.runners import load_model_runner  # noqa: E402

B = 4096
dev = torch.device("cuda", 0)
r = load_model_runner(os.path.join(bench.PKG, "checkpoints", "birdnet_stm32n6_100.tflite"), max_batch=B)
lib = _hip.load_library()
lib.bn_debug_tail2_stamps.argtypes = [ctypes.c_void_p]
x = bench.synth_audio_device(torch, B, 0, dev, 42)
out = torch.empty((B, 100), device=dev)
for _ in range(3):
    r.infer_audio_device(x, hop=bench.HOP, out=out)
torch.cuda.synchronize()
WG, GRP, BLK, WAVES = 8, 4, 8, 8
buf = torch.zeros(WG * GRP * BLK * WAVES * 8, dtype=torch.int64, device=dev)
assert lib.bn_debug_tail2_stamps(buf.data_ptr()) == 0
SPLIT = len(sys.argv) > 1 and sys.argv[1] == "split"
if SPLIT:
    lib.bn_debug_mid2_stamps.argtypes = [ctypes.c_void_p]
    mbuf = torch.zeros(WG * GRP * BLK * WAVES * 8, dtype=torch.int64, device=dev)
    assert lib.bn_debug_mid2_stamps(mbuf.data_ptr()) == 0
    r.profile(True)
    with _hip.options(i8_mid_split=0):
        r.infer_audio_device(x, hop=bench.HOP, out=out)
    torch.cuda.synchronize()
    ms = {q["kind"]: q["ms"] for q in r.profile_collect() if q["launches"]}
    print("# Barrier waits of `i8_mid2_kernel` and `i8_tail2_kernel`, staged forms: own chunk against the rest of the workgroup\n")
    print(f"INT8 B = {B}, stamped build (`make stamps`, `tools/tail2_stamps.py split`), `i8_mid_split` = 0; launches: stage 2 {ms.get('i8_mid', 0):.3f} ms, tail {ms.get('i8_tail', 0):.3f} ms.")
    print("Means over 8 workgroups x 4 chunk groups x 8 waves, microseconds per wave and block.  wait = arrival at the barrier -> behind it;")
    print("(a) = arrival -> the last wave of the wave's own chunk slot has arrived; (b) = from then -> the last wave of the workgroup has arrived.\n")
    for title, b_, nblk, wpc in (("i8_mid2_kernel (2 chunk slots x 4 waves)", mbuf, 3, 4), ("i8_tail2_kernel (4 chunk slots x 2 waves)", buf, 6, 2)):
        t = b_.cpu().numpy().reshape(WG, GRP, BLK, WAVES, 8).astype(np.float64) * 0.01
        print(f"## {title}\n")
        print("| block | phase before (depthwise) | middle wait | (a) | (b) | phase before (pointwise) | end wait | (a) | (b) |")
        print("|---|---|---|---|---|---|---|---|---|")
        tot = np.zeros(8)
        for li in range(nblk):
            q = t[:, :, li]
            row = np.array([(q[..., 1] - q[..., 0]).mean(), (q[..., 4] - q[..., 1]).mean(), (q[..., 3] - q[..., 1]).mean(), (q[..., 4] - q[..., 3]).mean(),
                            (q[..., 2] - q[..., 4]).mean(), (q[..., 6] - q[..., 2]).mean(), (q[..., 5] - q[..., 2]).mean(), (q[..., 6] - q[..., 5]).mean()])
            tot += row
            print(f"| {li} | " + " | ".join(f"{v:.2f}" for v in row) + " |")
        print("| all | " + " | ".join(f"{v:.2f}" for v in tot) + " |")
        wait, a_, b__ = tot[1] + tot[5], tot[2] + tot[6], tot[3] + tot[7]
        print(f"\nPer chunk group: busy {tot[0] + tot[4]:.2f} us, waiting at barriers {wait:.2f} us = (a) {a_:.2f} + (b) {b__:.2f}; "
              f"(b) is {100 * b__ / max(wait, 1e-9):.0f} % of the wait.\n")
    r.close()
    sys.exit(0)
r.profile(True)
r.infer_audio_device(x, hop=bench.HOP, out=out)
torch.cuda.synchronize()
tail_ms = [q["ms"] for q in r.profile_collect() if q["kind"] == "i8_tail" and q["launches"]]
st = buf.cpu().numpy().reshape(WG, GRP, BLK, WAVES, 8).astype(np.float64) * 0.01  # microseconds
names = ["stage3_ds1 (64->128, s2, taps from HBM)", "stage3_ds2 (128->128 + ADD)", "stage3_ds3 (128->128 + ADD)", "stage3_ds4 (128->128 + ADD)",
         "stage4_ds1 (128->256, s2)", "stage4_ds2 (256->256 + ADD)", "head: MEAN (-> barrier), then FULLY_CONNECTED + scores (-> group's end barrier)"]
print("# `i8_tail2_kernel`: where a wave's time goes, per block (in-kernel stamps, `tools/tail2_stamps.py`)\n")
print(f"INT8 B = {B}, stamped build; tail launch {tail_ms[0]:.3f} ms.  Means over 8 workgroups x 4 chunk groups x 8 waves.\n")
print("| block | entry -> behind the middle barrier (depthwise phase) us | -> behind the end barrier (pointwise phase) us | block us |")
print("|---|---|---|---|")
tot = np.zeros(3)
for li, nm in enumerate(names):
    dw = (st[:, :, li, :, 4] - st[:, :, li, :, 0]).mean()
    pw = (st[:, :, li, :, 6] - st[:, :, li, :, 4]).mean()
    print(f"| {nm} | {dw:.2f} | {pw:.2f} | {dw + pw:.2f} |")
    tot += np.array([dw, pw, dw + pw])
print(f"| all six blocks + head | {tot[0]:.2f} | {tot[1]:.2f} | {tot[2]:.2f} |")
per_group = tail_ms[0] * 1e3 / (B / 4 / 256)
print(f"\nA chunk group takes {per_group:.1f} us of the launch; the six blocks account for {tot[2]:.1f} us of it, the rest is MEAN + FULLY_CONNECTED + head.")
# the group's full extent from the first block's entry to the next group's entry
g0 = st[:, :-1, 0, :, 0]
g1 = st[:, 1:, 0, :, 0]
print(f"\nEntry of a group's first block to the entry of the next group's: {(g1 - g0).mean():.2f} us.")
r.close()
