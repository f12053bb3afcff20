"""Models, inputs and plan mutants of the float32 operator tests (tests/test_f32_plan_ref_host.py, tests/test_gpu_f32_ops.py).

A helper, not a test.  Seeded models go through :func:`liven`: with fresh BatchNorm statistics about half of the channels behind a ReLU are
identically zero on any input, so any negative pre-activation would be "correct" there.  ``liven`` changes the TEST's ``NetSpec`` (never the
product): layer by layer, with the oracle's own layer functions, it raises the BatchNorm ``beta`` of a channel whose pre-activation is
nowhere positive over the input set (and lowers one that sits at the ReLU6 clamp everywhere).  The shipped checkpoint is data and stays.
"""

from __future__ import annotations

import functools

import numpy as np

from conftest import KERAS_PATH, synth_chunks

BASE = dict(num_mels=64, spec_width=256, sample_rate=24000, chunk_duration=3, embeddings_size=256, num_classes=10, randomize_bn=True, seed=7)
GEOM = dict(BASE, seed=11)

# name -> (build_model arguments or None for the shipped archive, frontend norm override or None)
MODELS = {
    "shipped": (None, None),
    "ir_se_default": (dict(BASE), None),
    "ds_se_attnpool_emb": (dict(BASE, use_inverted_residual=False, use_se=True, embeddings_size=128, use_attention_pooling=True, class_activation="sigmoid"), None),
    "alpha1.5_pcen": (dict(BASE, alpha=1.5, mag_scale="pcen", num_classes=37), None),
    "mels32_w128_a0.75_2s": (dict(GEOM, num_mels=32, spec_width=128, alpha=0.75, chunk_duration=2), False),
    "mels40_w128_ds": (dict(GEOM, num_mels=40, spec_width=128, alpha=0.5, use_se=False, use_inverted_residual=False, class_activation="linear"), False),
    "raw_small_padded": (dict(num_mels=24, spec_width=96, sample_rate=8000, chunk_duration=1.0, embeddings_size=64, num_classes=7, alpha=0.5, audio_frontend="raw",
                              mag_scale="pwl", use_se=False, use_inverted_residual=False, randomize_bn=True, seed=3), None),
    "raw_pcen_a1.5_2s": (dict(num_mels=64, spec_width=256, sample_rate=24000, chunk_duration=2, embeddings_size=256, num_classes=100, audio_frontend="raw",
                              mag_scale="pcen", alpha=1.5, use_se=True, use_inverted_residual=True, randomize_bn=True, seed=42), None),
    "mels64_w320_ds_se_norm": (dict(GEOM, spec_width=320, use_inverted_residual=False, use_se=True), True),
}
BATCH3_ONLY = ("raw_pcen_a1.5_2s",)  # the one large model: batch of 3, default form and f32_pw_ws = 0


def raw_spec(name: str):
    """The model as built / loaded, before :func:`liven`."""
    args, norm = MODELS[name]
    if args is None:
        from birdnet_stm32.models._keras_loader import load_keras_archive

        return load_keras_archive(KERAS_PATH)
    from birdnet_stm32.models import build_model

    spec = build_model("dscnn", **args)
    if norm is not None:
        spec.frontend.attrs["norm"] = norm
    return spec


def model_inputs(spec) -> np.ndarray:
    """The six inputs of a model, float32 ``[6, ...]`` in the runner's input shape: two synthetic chunks, zeros, ones, single spikes at
    the four corners and the centre, dense uniform noise — spectrograms for the hybrid frontend, their waveform analogues for the raw one."""
    from oracle import stft

    fa = spec.frontend.attrs
    sr, cd, W = int(fa["sample_rate"]), float(fa["chunk_duration"]), int(fa["spec_width"])
    chunks = synth_chunks(2, sr=sr, seconds=cd, seed=4)
    rng = np.random.default_rng(17)
    if fa["mode"] == "raw":
        T = int(sr * cd)
        x = np.zeros((6, T), np.float32)
        x[:2] = chunks / (np.abs(chunks).max(axis=1, keepdims=True) + 1e-6)
        x[3] = 1.0
        x[4, [0, 1, T // 2, T - 2, T - 1]] = (1.0, -0.5, 0.75, -1.0, 0.5)
        x[5] = rng.uniform(-1, 1, T)
        return x[..., None]
    F = int(fa["fft_length"]) // 2 + 1
    x = np.zeros((6, F, W), np.float32)
    x[:2] = np.stack([stft.hybrid_spectrogram(a, int(fa["fft_length"]), W) for a in chunks])
    x[3] = 1.0
    for f, t in ((0, 0), (0, W - 1), (F - 1, 0), (F - 1, W - 1), (F // 2, W // 2)):
        x[4, f, t] = 1.0
    x[5] = rng.uniform(0, 1, (F, W))
    return x[..., None]


def click_and_silence(spec) -> np.ndarray:
    """Audio for the audio entry: two synthetic chunks, silence, one click."""
    fa = spec.frontend.attrs
    sr, cd = int(fa["sample_rate"]), float(fa["chunk_duration"])
    a = np.zeros((4, int(sr * cd)), np.float32)
    a[:2] = synth_chunks(2, sr=sr, seconds=cd, seed=4)
    a[3, 1000] = 1.0
    return a


def liven(spec, x: np.ndarray, margin_q: float = 0.75):
    """Adjust BatchNorm betas in place so that every channel behind a ReLU is positive somewhere over ``x`` and not at the ReLU6 clamp
    everywhere.  A dead channel's beta is raised until the ``margin_q`` quantile of its pre-activation is 1/16 (a quarter of its elements
    come out positive); a channel clamped everywhere is lowered until its median is 3.  Returns {relu layer: channels adjusted}."""
    from oracle import float_graph as fg

    dt = np.float64
    acts: dict[str, np.ndarray] = {}
    by_name = {ly.name: ly for ly in spec.layers}
    changed: dict[str, int] = {}
    for ly in spec.layers:
        k = ly.kind
        src = [acts[n] for n in ly.inputs]
        if k == "relu":
            # the BatchNorm whose beta shifts this pre-activation: back through identities and one Add
            chain, cur = [], by_name[ly.inputs[0]]
            while cur.kind in ("identity", "add"):
                chain.append(cur)
                if cur.kind == "add":
                    nxt = [by_name[n] for n in cur.inputs]
                    hit = [c for c in nxt if _leads_to_bn(c, by_name)]
                    cur = hit[-1]
                else:
                    cur = by_name[cur.inputs[0]]
            if cur.kind == "batchnorm":
                pre = src[0]
                flat = pre.reshape(-1, pre.shape[-1])
                delta = np.zeros(flat.shape[1])
                dead = flat.max(axis=0) <= 0
                # (+ 1/16: many elements of a dead channel share one value, the folded bias, which must not cancel to rounding noise)
                delta[dead] = 0.0625 - np.quantile(flat[:, dead], margin_q, axis=0) if dead.any() else 0.0
                if ly.attrs.get("max_value") is not None:
                    top = flat.min(axis=0) >= float(ly.attrs["max_value"])
                    delta[top] = 3.0 - np.median(flat[:, top], axis=0) if top.any() else 0.0
                    dead = dead | top
                if dead.any():
                    old = cur.weights["beta"].astype(np.float64)
                    cur.weights["beta"] = (old + delta).astype(np.float32)
                    real = cur.weights["beta"].astype(np.float64) - old  # (what the float32 beta moved by)
                    for c in [cur, *chain]:
                        acts[c.name] = acts[c.name] + real
                    src = [acts[n] for n in ly.inputs]
                    changed[ly.name] = int(dead.sum())
        if k == "input":
            y = np.asarray(x).astype(dt)
        elif k == "frontend":
            y = fg.frontend_forward(src[0], ly, dt)
        elif k == "conv2d":
            y = fg.conv2d_same(src[0], ly.weights["kernel"].astype(dt), ly.attrs["strides"])
        elif k == "dwconv2d":
            y = fg.dwconv2d_same(src[0], ly.weights["kernel"].astype(dt), ly.attrs["strides"])
        elif k == "batchnorm":
            w = ly.weights
            y = w["gamma"].astype(dt) * (src[0] - w["mean"].astype(dt)) / np.sqrt(w["var"].astype(dt) + dt(ly.attrs["eps"])) + w["beta"].astype(dt)
        elif k == "relu":
            y = np.maximum(src[0], 0)
            if ly.attrs.get("max_value") is not None:
                y = np.minimum(y, dt(ly.attrs["max_value"]))
        elif k == "add":
            y = src[0] + src[1]
        elif k == "multiply":
            y = src[0] * src[1]
        elif k == "gap":
            y = src[0].mean(axis=(1, 2), keepdims=bool(ly.attrs.get("keepdims")))
        elif k == "dense":
            y = src[0] @ ly.weights["kernel"].astype(dt)
            if "bias" in ly.weights:
                y = y + ly.weights["bias"].astype(dt)
            if ly.attrs.get("activation") == "relu":
                y = np.maximum(y, 0)
            elif ly.attrs.get("activation") == "sigmoid":
                y = 1.0 / (1.0 + np.exp(-y))
        elif k == "identity":
            y = src[0]
        else:
            break  # pooling and head: no ReLU behind them
        acts[ly.name] = y
    return changed


def _leads_to_bn(layer, by_name) -> bool:
    while layer.kind == "identity":
        layer = by_name[layer.inputs[0]]
    return layer.kind == "batchnorm"


def live_share(spec, acts: dict) -> dict:
    """{relu layer: (channels non-zero somewhere, channels, channels at the ReLU6 clamp everywhere)} from oracle activations."""
    out = {}
    for ly in spec.layers:
        if ly.kind != "relu":
            continue
        a = acts[ly.name].reshape(-1, acts[ly.name].shape[-1])
        mv = ly.attrs.get("max_value")
        out[ly.name] = (int((a.max(axis=0) > 0).sum()), a.shape[1], int((a.min(axis=0) >= float(mv)).sum()) if mv is not None else 0)
    return out


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(spec, inputs [6, ...]) of a model, seeded ones livened; cached for the session (the spec is not to be modified)."""
    spec = raw_spec(name)
    x = model_inputs(spec)
    if MODELS[name][0] is not None:
        liven(spec, x)
    return spec, x


# ------------------------------------------------------------------------------------------------------------------------- mutants
def reference_run(plan, x: np.ndarray) -> dict:
    """{operator index: result dict of f32_plan_ref.eval_op}: the float64 reference run from the model input, every operator reading the
    reference value of the one in front as if observed (each bound is that operator's own)."""
    import f32_plan_ref as fr

    return {oi: r for oi, _, r, _ in fr.walk_plan(plan, x, lambda oi: None, own=True)}


def _altered(plan, ti: int, index, fn):
    """A copy of ``plan`` whose tensor ``ti`` has ``fn(value)`` at ``index`` (float32, and different from before)."""
    import copy

    new = copy.copy(plan)
    new.tensors = list(plan.tensors)
    t = plan.tensors[ti].copy()
    t[index] = np.float32(fn(np.float64(t[index])))
    assert t[index] != plan.tensors[ti][index]
    new.tensors[ti] = t
    return new


def mutants(plan, ref: dict) -> dict:
    """The four altered plans of the sensitivity tests, {name: (plan, operator altered, operator whose output shows it, what)}.  ``ref``:
    :func:`reference_run` of the unaltered plan on the test inputs (it picks the live channel with the smallest peak)."""
    from birdnet_stm32.models import _pack as pk

    ops = plan.ops
    out = {}
    # one pointwise weight of the live output channel with the smallest peak relative to its map's (plain 1x1 operators: their input is readable)
    best = None
    for oi, r in ref.items():
        op = ops[oi]
        if op.kind != pk.F32_DWPW or op.get("has_dw"):
            continue
        peak = np.abs(r["out"].val).reshape(-1, op.get("Cout")).max(axis=0)
        rel = np.where(peak > 0, peak / peak.max(), np.inf)
        c = int(np.argmin(rel))
        if best is None or rel[c] < best[0]:
            best = (float(rel[c]), oi, c)
    rel, oi, c = best
    op = ops[oi]
    Cin = op.get("Cin")
    xin = np.abs(ref[oi]["in0"].val).reshape(ref[oi]["in0"].val.shape[0], -1, Cin)
    if ref[oi]["gate"] is not None:
        xin = xin * np.abs(ref[oi]["gate"].val).reshape(-1, 1, Cin)
    frag = plan.tensors[op.get("pw_w")]
    col = np.array([abs(float(frag[i // 16, c // 16, ((i % 16) // 4) * 16 + c % 16, i % 4])) for i in range(Cin)])
    terms = xin.reshape(-1, Cin) * col  # |w x| per (element, input channel): alter the weight with the largest share of its sum
    total = terms.sum(axis=1) + abs(float(plan.tensors[op.get("pw_b")][c]))
    if ref[oi]["in1"] is not None:
        total = total + np.abs(ref[oi]["in1"].val).reshape(-1, op.get("Cout"))[:, c]
    shows = np.abs(ref[oi]["out"].val).reshape(-1, op.get("Cout"))[:, c] > 0  # (elements the ReLU lets through)
    i = int(np.unravel_index(np.argmax(terms * shows[:, None] / (total[:, None] + 1e-300)), terms.shape)[1])
    out["pw_weight"] = (_altered(plan, op.get("pw_w"), (i // 16, c // 16, ((i % 16) // 4) * 16 + c % 16, i % 4), lambda v: v * (1 + 2.0 ** -10)), oi, oi,
                        f"{op.name}: weight [{i}][{c}] x (1 + 2^-10), channel peak {rel:.2e} of the map's")
    # one depthwise corner tap, one folded bias: the first stand-alone depthwise operator, the channel with the largest tap / bias
    di = next(oi for oi in ref if ops[oi].kind == pk.F32_DW)
    w = plan.tensors[ops[di].get("w")]
    ch = int(np.argmax(np.abs(w[0, 0])))
    out["dw_corner_tap"] = (_altered(plan, ops[di].get("w"), (0, 0, ch), lambda v: v * (1 + 2.0 ** -10)), di, di, f"{ops[di].name}: tap [0][0][{ch}] x (1 + 2^-10)")
    b = plan.tensors[ops[di].get("bias")]
    ch = int(np.argmax(np.abs(b)))
    out["folded_bias"] = (_altered(plan, ops[di].get("bias"), (ch,), lambda v: v * (1 + 2.0 ** -12)), di, di, f"{ops[di].name}: bias [{ch}] moved by 2^-12 of itself")
    # one band value of the mel mixer: the largest weight of the middle band
    mi = next(oi for oi in ref if ops[oi].kind == pk.F32_MEL)
    bands = plan.tensors[ops[mi].get("bands")]
    m = bands.shape[1] // 2
    vals = plan.tensors[ops[mi].get("wvals")]
    j = int(bands[2, m]) + int(np.argmax(vals[bands[2, m] : bands[2, m] + bands[1, m]]))
    shown = max(oj for oj in ref if ops[oj].out == ops[mi].out)  # (the in-place MAG behind it when the frontend normalises)
    out["mel_band_value"] = (_altered(plan, ops[mi].get("wvals"), (j,), lambda v: v * (1 + 2.0 ** -10)), mi, shown, f"mel band {m}: value {j} moved by one part in 2^10")
    return out
