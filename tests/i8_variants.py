"""Shapes other than the shipped checkpoint's for the fused back half of the INT8 graph: other class counts, a head without LOGISTIC,
shorter and longer chains of stage 3-4 blocks.

``tests/i8_mutants.py`` changes the numbers of the shipped graph and keeps its shape.  The builders here keep the numbers (as far as they
can) and change the shape that ``i8_tail2_kernel`` / ``i8_tail_kernel`` and their planners see: the class count NC (tile count, padded
rows, the LDS copy of the classifier, the edges NC = 128 | 129 and 256 | 257 between the kernels), the head's table, and the run of blocks
between stage 2 and the MEAN.  Every variant is a deterministic, seeded ``TfliteModel`` derived IN MEMORY from ``i8_mutants.shipped()``;
``build(name)`` makes one, ``VARIANTS`` says what the lowering must make of it, ``oracle(model, S)`` runs the numpy interpreter on it.
Plain helper module: no fixtures, no test functions.

``repeat_blocks`` and the 8-layer chain: the copy of a residual block reads its original's ADD output, whose scale differs from that of
the tensor the original reads.  With the original's own scales on the copy's three outputs the lowering keeps every fused form (``tail =
1``, matrix-core constants present) for one more res128 and one more res256 block, so no scale had to be adjusted; a ninth block makes
``_add_tail_op`` leave the tail unfused (``len(chain) > 8``).  The LIBRARY does not fuse the 8-layer chain, though: ``tail_plan`` finds no
LDS placement for it (TAIL_FORM below has the cause), so on the device these variants run the per-block kernels.
"""

from __future__ import annotations

import dataclasses
import functools

import numpy as np

import i8_mutants as im

N_INPUTS = 16
INPUT_SEED = 3
CLASS_COUNTS = (1, 15, 16, 17, 100, 128, 129, 252, 253, 256, 257, 1000)


# ------------------------------------------------------------------------------------------------ graph access
def blocks_of(model) -> list[dict]:
    """``i8_mutants.backbone`` for a graph whose stage 3-4 has any number of blocks: dict(dw, pw, add, stage, first, out) per block."""
    ops = model.ops
    i = next(k for k, o in enumerate(ops) if o.name == "CONV_2D" and tuple(model.tensors[o.inputs[1]].shape[1:3]) == (3, 3)) + 1
    blocks = []
    while i + 1 < len(ops) and ops[i].name == "DEPTHWISE_CONV_2D":
        dw, pw = ops[i], ops[i + 1]
        add = ops[i + 2] if ops[i + 2].name == "ADD" else None
        ow = int(model.tensors[pw.outputs[0]].shape[2])
        stage = "stage1" if ow == 64 else "stage2" if ow == 32 else "stage3-4"
        blocks.append(dict(dw=dw, pw=pw, add=add, stage=stage, first=dw.options["stride_w"] == 2, out=(add or pw).outputs[0]))
        i += 3 if add is not None else 2
    assert ops[i].name == "MEAN"
    return blocks


def tail_chain(model) -> list[dict]:
    return [b for b in blocks_of(model) if b["stage"] == "stage3-4"]


def head_ops(model) -> dict:
    """mean, fc, logistic (or None) and dequantize operators of the head."""
    by = {o.name: o for o in model.ops[-4:]}
    assert model.ops[-1].name == "DEQUANTIZE" and "FULLY_CONNECTED" in by and "MEAN" in by
    return dict(mean=by["MEAN"], fc=by["FULLY_CONNECTED"], logistic=by.get("LOGISTIC"), dequantize=by["DEQUANTIZE"])


def _renumber(model) -> None:
    for k, o in enumerate(model.ops):   # (the lowering and the oracle take op.index for the position)
        o.index = k


def _new_tensor(model, like: int, tag: str) -> int:
    t = model.tensors[like]
    assert t.data is None
    model.tensors.append(dataclasses.replace(t, index=len(model.tensors), name=f"{t.name}/{tag}", scale=t.scale.copy(), zero_point=t.zero_point.copy()))
    return len(model.tensors) - 1


# ------------------------------------------------------------------------------------------------ inputs and the oracle
@functools.lru_cache(maxsize=1)
def inputs() -> np.ndarray:
    """The 16 spectrograms every variant is run on (read-only)."""
    S = im.boundary_inputs(N_INPUTS, seed=INPUT_SEED)
    S.setflags(write=False)
    return S


_front_cache: dict = {}


def _front(S: np.ndarray) -> tuple[dict, int]:
    """(tensors of the shipped graph in front of stage 3-4 on ``S``, index of the first stage 3-4 operator): no builder here touches that part."""
    from oracle.int8_graph import Int8Interpreter

    key = (S.shape, hash(S.tobytes()))
    if key not in _front_cache:
        m = im.shipped()
        first = tail_chain(m)[0]["dw"]
        cut = dataclasses.replace(m, ops=m.ops[: first.index], outputs=[first.inputs[0]])
        _, env = Int8Interpreter(cut).invoke(S, return_all=True)
        _front_cache[key] = ({first.inputs[0]: env[first.inputs[0]]}, first.index)
    return _front_cache[key]


def oracle(model, S: np.ndarray):
    """``Int8Interpreter(model).invoke(S, return_all=True)`` with the operators in front of stage 3-4 (identical in every variant, checked) taken
    from one shared run of the shipped graph; the returned tensors are those from the stage-2 output on."""
    from oracle.int8_graph import Int8Interpreter

    env, k = _front(S)
    base = im._shipped_cached()
    assert [(o.name, o.inputs, o.outputs) for o in model.ops[:k]] == [(o.name, o.inputs, o.outputs) for o in base.ops[:k]]
    return Int8Interpreter(model).invoke(S, return_all=True, resume=(env, k))


def calibration_inputs() -> np.ndarray:
    return im.boundary_inputs(8, seed=5)[[0, 1, 7, 4, 2, 5]]


# ------------------------------------------------------------------------------------------------ builders
def resize_head(model, nc: int, seed: int = 0):
    """Classifier of ``nc`` classes: rows sampled with replacement from the shipped classifier (weights permuted within the row, the row's
    scale kept: sum |w| and the multipliers are the shipped ones, so the lowering's range checks hold as shipped), biases chosen so that the
    median accumulator of class j over six calibration chunks lands on a target byte t_j — evenly spaced over the part of the int8 range
    where the head's table moves (LOGISTIC), or over -100 .. 100 (no table) — in a shuffled order, so that neighbouring classes differ.

    Each bias is then raised by less than one output step so that the accumulator of ONE of the test inputs (input j mod 16 for class j)
    is the smallest one that still gives its output byte: any decrease moves that class's byte.  One more unit of a weight in the PACKED
    classifier (the folded bias ``b - zp sum w`` left alone) adds the raw pooled byte, which is negative for all but the largest activations
    (zero point -128), so it shows on that input.  (Without this a weight + 1 — at most 128 accumulator units against 2000 .. 6000 per
    output step — changes no byte of a class on any of the 16 inputs, and a comparison could not see a wrong classifier weight of that
    size.)"""
    from birdnet_stm32.models import _quant as qz

    rng = np.random.default_rng(21_000 + 131 * nc + seed)
    h = head_ops(model)
    fc = h["fc"]
    wt, bt = model.tensors[fc.inputs[1]], model.tensors[fc.inputs[2]]
    base_w = im._shipped_cached().tensors[fc.inputs[1]]
    assert wt.data.shape[1] == 256
    rows = rng.integers(0, base_w.data.shape[0], nc)
    wt.data = np.stack([base_w.data[r][rng.permutation(256)] for r in rows]).astype(np.int8)
    wt.shape = (nc, 256)
    wt.scale, wt.zero_point = base_w.scale[rows].copy(), np.zeros(nc, np.int64)
    s_in, z_in = im.qp(model, fc.inputs[0])
    s_out, z_out = im.qp(model, fc.outputs[0])
    bt.shape, bt.scale, bt.zero_point = (nc,), (np.float32(s_in) * wt.scale).astype(np.float32), np.zeros(nc, np.int64)
    if h["logistic"] is not None:
        lut = qz.logistic_table(s_out, z_out, *im.qp(model, h["logistic"].outputs[0])).astype(np.int64)
        moving = np.nonzero((lut > lut.min() + 1) & (lut < lut.max() - 1))[0] - 128
        t_lo, t_hi = int(moving.min()), int(moving.max())
    else:
        t_lo, t_hi = -100, 100
    target = np.linspace(t_lo, t_hi, nc)[rng.permutation(nc)] if nc > 1 else np.asarray([(t_lo + t_hi) / 2.0])
    bt.data = np.zeros(nc, np.int32)
    _, env = oracle(model, calibration_inputs())
    x = env[fc.inputs[0]].reshape(-1, 256).astype(np.int64) - z_in
    acc = x @ wt.data.astype(np.int64).T
    mult = np.float64(np.float32(s_in)) * wt.scale.astype(np.float64) / np.float64(np.float32(s_out))
    bias = np.rint((target - z_out) / mult - np.median(acc, axis=0)).astype(np.int64)
    _, env = oracle(model, inputs())
    xt = env[fc.inputs[0]].reshape(-1, 256).astype(np.int64) - z_in
    pick = np.arange(nc) % xt.shape[0]
    acc = (xt[pick] * wt.data.astype(np.int64)).sum(axis=1) + bias
    m, sh = qz.channel_multipliers(s_in, wt.scale, s_out, nc)
    byte = lambda a: np.clip(qz.requantize(a, m, sh) + z_out, -128, 127)   # noqa: E731  (monotone in the accumulator: bisect for the boundary)
    b0, lo, hi = byte(acc), np.zeros(nc, np.int64), np.ceil(1.5 / mult).astype(np.int64)
    assert (byte(acc + hi) != b0).all()
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        moved = byte(acc + mid) != b0
        lo, hi = np.where(moved, lo, mid), np.where(moved, mid, hi)
    im.set_b(model, fc, bias + hi)
    t = fc.outputs[0]
    while True:   # the classifier output and everything behind it
        model.tensors[t].shape = (1, nc)
        nxt = [o for o in model.ops if t in o.inputs]
        if not nxt:
            break
        t = nxt[0].outputs[0]
    return model


def drop_logistic(model):
    """FULLY_CONNECTED -> DEQUANTIZE: a head without a table (``g_hlut = -1``); the scores are the dequantised classifier output."""
    h = head_ops(model)
    assert h["logistic"] is not None
    h["dequantize"].inputs = [h["fc"].outputs[0]]
    model.ops.remove(h["logistic"])
    _renumber(model)
    return model


def drop_blocks(model, which):
    """Remove the residual blocks ``which`` (indices among the residual blocks of stage 3-4 in graph order: 0, 1, 2 = res128, 3 = res256);
    whoever read such a block's ADD output reads the block's input tensor instead."""
    res = [b for b in tail_chain(model) if b["add"] is not None]
    for k in sorted(which, reverse=True):
        b = res[k]
        src, out = b["dw"].inputs[0], b["add"].outputs[0]
        for o in (b["dw"], b["pw"], b["add"]):
            model.ops.remove(o)
        for o in model.ops:
            o.inputs = [src if t == out else t for t in o.inputs]
    _renumber(model)
    return model


def repeat_blocks(model, n128: int = 1, n256: int = 1):
    """Append ``n128`` / ``n256`` copies of the last residual block of stage 3 / stage 4 behind it: new activation tensors with the scales
    and zero points of the original's, the SAME weight, bias and scale tensors.  A copy reads its predecessor's ADD output."""
    for width, n in ((128, n128), (256, n256)):
        for rep in range(n):
            b = [b for b in tail_chain(model) if b["add"] is not None and model.tensors[b["out"]].shape[3] == width][-1]
            at = model.ops.index(b["add"]) + 1
            src = b["add"].outputs[0]
            t_dw, t_pw, t_add = (_new_tensor(model, o.outputs[0], f"copy{rep}") for o in (b["dw"], b["pw"], b["add"]))
            for o in model.ops[at:]:
                o.inputs = [t_add if t == src else t for t in o.inputs]
            dw = dataclasses.replace(b["dw"], inputs=[src] + list(b["dw"].inputs[1:]), outputs=[t_dw], options=dict(b["dw"].options))
            pw = dataclasses.replace(b["pw"], inputs=[t_dw] + list(b["pw"].inputs[1:]), outputs=[t_pw], options=dict(b["pw"].options))
            add = dataclasses.replace(b["add"], inputs=[src if t == b["dw"].inputs[0] else t_pw for t in b["add"].inputs], outputs=[t_add],
                                      options=dict(b["add"].options))
            model.ops[at:at] = [dw, pw, add]
            _renumber(model)
    return model


# ------------------------------------------------------------------------------------------------ the variants
# name -> what the lowering must make of it: NC, blocks of stage 3-4, a table behind the classifier, fused tail operator in the plan, its
# matrix-core constants present, and ``gpu``: the variant is run on the device (the 9-layer chain only pins that the plan has no tail)
def _v(nc, layers, table=True, tail=1, tail2=True, gpu=True, chain=None):
    return dict(nc=nc, layers=layers, table=table, tail=tail, tail2=tail2, gpu=gpu, chain=chain)


VARIANTS = {f"nc{n}": _v(n, 6, tail=int(n <= 256), tail2=n <= 256) for n in CLASS_COUNTS}   # (nc100 = the shipped 6-layer chain)
VARIANTS.update({
    "nolog100": _v(100, 6, table=False), "nolog17": _v(17, 6, table=False),
    "chain2": _v(100, 2, chain="drop0123"), "chain4": _v(100, 4, chain="drop12"), "chain5": _v(100, 5, chain="drop3"),
    "chain8": _v(100, 8, chain="rep11"), "chain9": _v(100, 9, tail=0, tail2=False, gpu=False, chain="rep21"),
    "chain2_nc252": _v(252, 2, chain="drop0123"), "chain2_nc17": _v(17, 2, chain="drop0123"),
    "chain8_nc128": _v(128, 8, chain="rep11"), "chain8_nc129": _v(129, 8, chain="rep11"),
})
GPU_VARIANTS = [n for n, v in VARIANTS.items() if v["gpu"]]
CHAIN_VARIANTS = [n for n, v in VARIANTS.items() if v["chain"]]
# ``runner.tail_form()[0]``: 2 = i8_tail2_kernel runs by default (i8_tail_kernel behind it), 1 = i8_tail_kernel only, 0 = per-block kernels.
# The library's host-side planners (csrc/bn_chain_plan.cpp) compute these values from the descriptor tables; tests/test_chain_plan_host.py
# asserts them on the CPU from the planners themselves, tests/test_gpu_i8_variants.py from the loaded model and from which kernel ran.
# Shipped chain: what the packer and the NC conditions of tail_plan / tail2_plan say.  The chains of 2, 4 and 5 blocks take the form their NC
# allows.  The 8-block chain is refused by tail_plan (and with it by tail2_plan, which only runs where the first form could): (0, 0), the
# per-block kernels run.  Its first fit puts the output map of the 128 -> 256 block at 67584 when that block's input sits at 0 — which an EVEN
# number of res128 blocks in front of it makes it do — and the 64 KB of pointwise weights of the first res256 block then fit neither below
# the maps nor above them (100864 + 65536 > 160 KB).  A fallback of the placement, not a wrong result: pinned here, so that a planner that
# starts to accept the chain shows up.
TAIL_FORM = {n: (0 if v["layers"] == 8 else 2 if v["nc"] <= 128 else 1 if v["nc"] <= 256 else 0) for n, v in VARIANTS.items() if v["gpu"]}


def build(name: str):
    v = VARIANTS[name]
    m = im.shipped()
    c = v["chain"]
    if c and c.startswith("drop"):
        drop_blocks(m, [int(d) for d in c[4:]])
    elif c:
        repeat_blocks(m, int(c[3]), int(c[4]))
    if not v["table"]:
        drop_logistic(m)
    return resize_head(m, v["nc"], seed=0)


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """Model and oracle results (cached: treat as read-only) on ``inputs()``: scores, classifier bytes ``fc``, their float32 form ``logits``, pooled bytes ``emb`` and
    their float32 form ``emb_f32``, all tensors ``env`` (from the stage-2 output on)."""
    model = build(name)
    scores, env = oracle(model, inputs())
    h = head_ops(model)
    s, z = im.qp(model, h["fc"].outputs[0])
    se, ze = im.qp(model, h["mean"].outputs[0])
    fc, emb = env[h["fc"].outputs[0]], env[h["mean"].outputs[0]].reshape(N_INPUTS, -1)
    return dict(model=model, scores=scores, env=env, fc=fc, logits=(fc.astype(np.float32) - np.float32(z)) * np.float32(s), emb=emb,
                emb_f32=(emb.astype(np.float32) - np.float32(ze)) * np.float32(se),
                score_bytes=env[h["logistic"].outputs[0]] if h["logistic"] is not None else None)


@functools.lru_cache(maxsize=None)
def plan(name: str):
    """The production plan of ``case(name)["model"]`` (cached for the host tests that only read it: treat as read-only)."""
    from birdnet_stm32.models._lower_i8 import lower_i8

    return lower_i8(case(name)["model"])


def weight_flips(c: dict, cls: int) -> np.ndarray:
    """Per input channel k: on how many test inputs the classifier byte of class ``cls`` changes when W[cls][k] grows by one in the packed
    constants of a plan, where the bias is stored folded (``b - zp sum w``) and stays as it is: the accumulator moves by the raw pooled
    byte.  In terms of the model that is W[cls][k] + 1 together with b[cls] + zp.  0 where the weight is 127.  ``_quant.requantize`` on the
    oracle's pooled bytes, checked against the oracle's classifier bytes first."""
    from birdnet_stm32.models import _quant as qz

    model = c["model"]
    fc = head_ops(model)["fc"]
    _, z_in = im.qp(model, fc.inputs[0])
    _, z_out = im.qp(model, fc.outputs[0])
    m, sh = im.fixed_point(model, fc)
    w = im.get_w(model, fc).astype(np.int64)
    raw = c["emb"].astype(np.int64)
    acc = (raw - z_in) @ w[cls] + im.get_b(model, fc)[cls]
    byte = lambda a: np.clip(qz.requantize(a, int(m[cls]), int(sh[cls])) + z_out, -128, 127)   # noqa: E731
    assert np.array_equal(byte(acc), c["fc"][:, cls].astype(np.int64)), "the classifier as restated here differs from the oracle"
    return (byte(acc[:, None] + raw) != byte(acc)[:, None]).sum(axis=0) * (w[cls] < 127)


def spread(c: dict) -> dict:
    """The figures the conditions on the inputs are stated in."""
    fc, emb = c["fc"], c["emb"]
    return dict(fc_distinct=int(np.unique(fc).size), fc_min_per_class=int(min(np.unique(fc[:, j]).size for j in range(fc.shape[1]))),
                fc_saturated=float(((fc == -128) | (fc == 127)).mean()),
                score_distinct=int(np.unique(c["score_bytes"]).size) if c["score_bytes"] is not None else None,
                emb_distinct=int(np.unique(emb).size), emb_rows_distinct=int(np.unique(emb, axis=0).shape[0]))
