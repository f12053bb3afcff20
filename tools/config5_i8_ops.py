#!/usr/bin/env python3
"""Per-operator times of the configs[4] INT8 backbone (see config5_i8_bench.py): kind, shape, ms, algorithmic GB/s."""
import os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "birdnet-stm32_amd"))
import numpy as np
import torch
from birdnet_stm32.conversion.export import convert_netspec_to_int8
from birdnet_stm32.models import build_model
from birdnet_stm32.models._lower_i8 import lower_i8
from birdnet_stm32.models._tflite_reader import parse_tflite
from birdnet_stm32.models._tflite_writer import write_tflite
from birdnet_stm32.models.runners import HipRunner

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
spec = build_model("dscnn", num_mels=64, spec_width=256, sample_rate=24000, chunk_duration=3, embeddings_size=256, num_classes=100,
                   audio_frontend="hybrid", mag_scale="pcen", alpha=1.5, use_se=True, use_inverted_residual=True, randomize_bn=True, seed=42)
spec.frontend.attrs["norm"] = True
rng = np.random.default_rng(0)
cal = [rng.random((1, 257, 256, 1), dtype=np.float32) ** 4 for _ in range(8)]
model = parse_tflite(write_tflite(convert_netspec_to_int8(spec, lambda: ([c] for c in cal), frontend_norm=True)))
r = HipRunner(lower_i8(model), max_batch=B)
x = torch.randn((B, 72000), device="cuda")
x = x / x.abs().amax(dim=1, keepdim=True)
for _ in range(2):
    r.infer_audio_device(x)
torch.cuda.synchronize()
r.profile(True)
for _ in range(3):
    r.infer_audio_device(x)
torch.cuda.synchronize()
for q in r.profile_collect():
    if not q["launches"]:
        continue
    g = r.plan.ops[q["op"]].get if q["p"] else None  # field of the operator's record by name (the STFT stages have none)
    ms = q["ms"] / q["launches"]
    if q["kind"] == "i8_dwpw":
        desc = f"H{g('H')} W{g('W')} Cin{g('Cin')} s{g('sh')} -> OH{g('OH')} OW{g('OW')} Cout{g('Cout')} dw{g('has_dw')} add{g('has_add')} strip{g('strip')}"
        gb = B * (g("H") * g("W") * g("Cin") + g("OH") * g("OW") * g("Cout")) / ms / 1e6
    elif q["kind"] in ("i8_dw", "i8_stem"):
        C = g("C" if q["kind"] == "i8_dw" else "Cout")
        desc = f"H{g('H')} W{g('W')} C{C} s{g('sh')} -> OH{g('OH')} OW{g('OW')}"
        gb = B * (g("H") * g("W") * (C if q["kind"] == "i8_dw" else 1) + g("OH") * g("OW") * C) / ms / 1e6
    elif q["kind"] == "i8_scale":
        desc = f"P{g('P')} C{g('C')}"
        gb = B * 2 * g("P") * g("C") / ms / 1e6
    else:
        desc, gb = str(q["p"][:4]), 0.0
    print(f"{q['kind']:10s} {q['name']:6s} {ms:7.3f} ms  {gb:8.1f} GB/s  {desc}")
