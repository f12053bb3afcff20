"""Weight sets other than the shipped checkpoint's for the fused INT8 kernels, and a ledger of what they reach.

The fused kernels (``i8_front_strip_kernel``, ``i8_strip_mf_kernel``, ``i8_mid2_kernel``, ``i8_tail2_kernel``, behind them ``i8_tail_kernel``)
run requantisation forms that ``models/_lower_i8.py`` proves for the particular weights.  Every family here is a deterministic, seeded
``TfliteModel`` derived IN MEMORY from ``checkpoints/birdnet_stm32n6_100.tflite``: same operators and shapes, other ``.data`` / scales /
zero points of the backbone (stem, depthwise, pointwise; the classifier for ``perm`` / ``sign`` / ``dense``).  The mel mixer and the
element-wise frontend in front of the stem are never touched.  ``mutant(family, seed)`` builds one, ``ledger(model, S)`` counts what the
lowering chose for it and what one oracle run actually produced.  Plain helper module: no fixtures, no test functions.
"""

from __future__ import annotations

import copy
import functools

import numpy as np

from conftest import TFLITE_PATH, synth_chunks

FAMILIES = {"perm": (0, 1), "sign": (0, 1), "dense": (0, 1), "dead": (0,), "edge": (0,), "scale": (0,)}
STAGES = ("stage1", "stage2", "stage3-4")
DEAD_TINY = 0.75 * 2.0**-30   # effective multiplier of a dead channel whose output is the zero point (shift 30)
DEAD_CONST = 0.75 * 2.0**-23  # ... of one whose folded bias alone yields a non-zero constant (shift 23)


@functools.lru_cache(maxsize=1)
def _shipped_cached():
    from birdnet_stm32.models._tflite_reader import load_tflite

    return load_tflite(TFLITE_PATH)


def shipped():
    """A private copy of the shipped INT8 model."""
    return copy.deepcopy(_shipped_cached())


# ------------------------------------------------------------------------------------------------ graph access
def backbone(model) -> tuple[object, list[dict]]:
    """(stem operator, blocks) of the shipped topology: every block is ``dict(dw, pw, add, stage, first)`` — ``stage`` by the width of the
    block's output map (64: stage 1 = front block + strip kernel, 32: stage 2 = ``i8_mid2_kernel``, <= 16: stage 3-4 = the fused tail),
    ``first`` = the stride-2 block that opens the stage (the block whose taps come from memory in the two chain kernels)."""
    ops = model.ops
    i = next(k for k, o in enumerate(ops) if o.name == "CONV_2D" and tuple(model.tensors[o.inputs[1]].shape[1:3]) == (3, 3))
    stem, blocks = ops[i], []
    i += 1
    while i + 1 < len(ops) and ops[i].name == "DEPTHWISE_CONV_2D":
        dw, pw = ops[i], ops[i + 1]
        add = ops[i + 2] if ops[i + 2].name == "ADD" else None
        ow = int(model.tensors[pw.outputs[0]].shape[2])
        stage = "stage1" if ow == 64 else "stage2" if ow == 32 else "stage3-4"
        blocks.append(dict(dw=dw, pw=pw, add=add, stage=stage, first=dw.options["stride_w"] == 2 and ow in (64, 32, 16), out=(add or pw).outputs[0]))
        i += 3 if add is not None else 2
    assert ops[i].name == "MEAN" and len(blocks) == 11
    return stem, blocks


def conv_ops(model, with_fc: bool = False) -> list:
    stem, blocks = backbone(model)
    out = [stem] + [o for b in blocks for o in (b["dw"], b["pw"])]
    if with_fc:
        out.append(next(o for o in model.ops if o.name == "FULLY_CONNECTED"))
    return out


def get_w(model, op) -> np.ndarray:
    """Weights as ``[output channel][taps or input channels]`` (a copy)."""
    t = model.tensors[op.inputs[1]]
    if op.name == "DEPTHWISE_CONV_2D":
        return t.data.reshape(-1, t.shape[3]).T.copy()
    return t.data.reshape(t.shape[0], -1).copy()


def set_w(model, op, w) -> None:
    t = model.tensors[op.inputs[1]]
    w = np.asarray(w)
    assert np.abs(w).max() <= 127
    t.data = (w.T if op.name == "DEPTHWISE_CONV_2D" else w).reshape(t.shape).astype(np.int8)


def get_b(model, op) -> np.ndarray:
    return model.tensors[op.inputs[2]].data.astype(np.int64)


def set_b(model, op, b) -> None:
    b = np.asarray(b, np.int64)
    assert np.abs(b).max() < 2**31
    t = model.tensors[op.inputs[2]]
    t.data = b.astype(np.int32).reshape(t.shape)


def qp(model, ti) -> tuple[float, int]:
    t = model.tensors[ti]
    return float(t.scale[0]), int(t.zero_point[0])


def get_mult(model, op) -> np.ndarray:
    """Real per-channel multiplier ``s_in s_w[c] / s_out`` of a convolution."""
    s_in, _ = qp(model, op.inputs[0])
    s_out, _ = qp(model, op.outputs[0])
    ws = model.tensors[op.inputs[1]].scale.astype(np.float64)
    return s_in * ws / s_out


def set_mult(model, op, mult) -> None:
    """Set the weight scales so that the real multipliers become ``mult`` (to float32 precision)."""
    s_in, _ = qp(model, op.inputs[0])
    s_out, _ = qp(model, op.outputs[0])
    t = model.tensors[op.inputs[1]]
    t.scale = (np.asarray(mult, np.float64) * s_out / s_in).astype(np.float32)
    assert t.scale.shape == t.zero_point.shape and (t.scale > 0).all()


def fixed_point(model, op) -> tuple[np.ndarray, np.ndarray]:
    """(Q31 multiplier, shift) per channel, as the lowering and the oracle derive them."""
    from birdnet_stm32.models import _quant as qz

    s_in, _ = qp(model, op.inputs[0])
    s_out, _ = qp(model, op.outputs[0])
    t = model.tensors[op.inputs[1]]
    return qz.channel_multipliers(s_in, t.scale, s_out, t.scale.size)


def conv_acc(model, op, x: np.ndarray) -> np.ndarray:
    """int64 accumulators (bias included) of a backbone convolution on the int8 map ``x`` [B, H, W, C]: SAME padding, padded taps
    contribute nothing.  Plain numpy, independent of the oracle's own convolution."""
    _, zp = qp(model, op.inputs[0])
    w = get_w(model, op).astype(np.int64)
    s = op.options["stride_h"], op.options["stride_w"]
    xc = x.astype(np.int64) - zp
    if w.shape[1] != 9:   # 1 x 1
        return xc @ w.T + get_b(model, op)
    B, H, W, C = xc.shape
    dims = []
    for size, st in zip((H, W), s):
        o = -(-size // st)
        total = max((o - 1) * st + 3 - size, 0)
        dims.append((o, total // 2, total - total // 2))
    (oh, pt, pb), (ow, pl, pr) = dims
    xp = np.pad(xc, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
    acc = np.zeros((B, oh, ow, w.shape[0]), np.int64)
    for i in range(3):
        for j in range(3):
            patch = xp[:, i : i + (oh - 1) * s[0] + 1 : s[0], j : j + (ow - 1) * s[1] + 1 : s[1], :]
            acc += patch * w[:, 3 * i + j]   # (depthwise: channel by channel; the stem: one input channel broadcast over the filters)
    return acc + get_b(model, op)


def acc_bounds(model, op) -> tuple[np.ndarray, np.ndarray]:
    """The lowering's proven range ``[lo, hi]`` of a channel's accumulator over every int8 input (the unfolded view: ``x - zp`` in 0 .. 255
    for zp = -128 is what the folded bias of ``_lower_i8`` amounts to; for another zero point the span shifts accordingly)."""
    _, zp = qp(model, op.inputs[0])
    w = get_w(model, op).astype(np.int64)
    b = get_b(model, op)
    a, z = (-128 - zp) * w, (127 - zp) * w
    return np.minimum(a, z).sum(axis=1) + b, np.maximum(a, z).sum(axis=1) + b


def requant(model, op, acc) -> np.ndarray:
    from birdnet_stm32.models import _quant as qz

    m, s = fixed_point(model, op)
    return qz.requantize(acc, m, s)


def act_bounds(model, op) -> tuple[int, int]:
    from birdnet_stm32.models import _quant as qz

    return qz.activation_bounds(op.options["activation"], *qp(model, op.outputs[0]))


def add_params(model, blk):
    """``AddParams`` of a residual block with the residual as operand 1 and the block's own value as operand 2."""
    from birdnet_stm32.models import _quant as qz

    add, own = blk["add"], blk["pw"].outputs[0]
    res = next(t for t in add.inputs if t != own)
    return qz.AddParams(*qp(model, res), *qp(model, own), *qp(model, add.outputs[0]), add.options["activation"])


# ------------------------------------------------------------------------------------------------ inputs
def boundary_inputs(n: int, seed: int = 0) -> np.ndarray:
    """``n`` >= 8 spectrograms at the runner boundary, float32 [n, 257, 256, 1]: the mix of test_i8_runner_boundary_4096_spectrograms_bit_exact —
    silence, all ones, a single spike, values on the quantiser's steps, scaled and plain uniform noise, and spectrograms of ``synth_chunks``
    for the rest (at least a quarter)."""
    from oracle import stft

    assert n >= 8
    rng = np.random.default_rng(1000 + seed)
    S = np.empty((n, 257, 256, 1), np.float32)
    n_syn = max(n - 8, n // 4)
    S[:n_syn, :, :, 0] = np.stack([stft.hybrid_spectrogram(a) for a in synth_chunks(n_syn, seed=77 + seed)])
    k = n - n_syn
    S[n_syn:] = rng.random((k, 257, 256, 1), dtype=np.float32)
    fixed = [np.zeros((257, 256, 1), np.float32), np.ones((257, 256, 1), np.float32), np.zeros((257, 256, 1), np.float32)]
    fixed[2][40, 100, 0] = 1.0
    fixed.append((np.round(S[n_syn] * 255.0) / 255.0).astype(np.float32))
    fixed.append(S[n_syn] * np.float32(32.0 / 255.0))
    for j, v in enumerate(fixed[: max(k - 1, 0)]):   # (the last of the k stays plain uniform noise)
        S[n_syn + j] = v
    return S


# ------------------------------------------------------------------------------------------------ families
def perm(seed: int = 0):
    """Every output channel's weights permuted among themselves (input channels of a 1 x 1 convolution and of the classifier, the nine taps
    of a 3 x 3 kernel).  Sum |w| per channel is unchanged, so every range proof of the lowering holds as for the shipped weights: all fused
    forms are kept, the matrix-core tail included."""
    m, rng = shipped(), np.random.default_rng(11_000 + seed)
    for op in conv_ops(m, with_fc=True):
        w = get_w(m, op)
        set_w(m, op, np.stack([row[rng.permutation(row.size)] for row in w]))
    return m


def sign(seed: int = 0):
    """Random sign flips of every weight and every bias.  |w| is unchanged: all fused forms are kept."""
    m, rng = shipped(), np.random.default_rng(12_000 + seed)
    for op in conv_ops(m, with_fc=True):
        w = get_w(m, op)
        set_w(m, op, w * rng.choice((-1, 1), size=w.shape))
        b = get_b(m, op)
        set_b(m, op, b * rng.choice((-1, 1), size=b.shape))
    return m


def dense(seed: int = 0):
    """Uniform random weights in [-127, 127] (biases and scales as shipped).  The own terms of the residual blocks of stage 3-4 can then leave
    ``|v| < 2^11``: the plan keeps ``i8_mid2_kernel`` but carries no matrix-core constants for the tail and runs ``i8_tail_kernel``."""
    m, rng = shipped(), np.random.default_rng(13_000 + seed)
    for op in conv_ops(m, with_fc=True):
        w = get_w(m, op)
        set_w(m, op, rng.integers(-127, 128, size=w.shape))
    return m


def _dead_channels(live: np.ndarray, salt: int) -> tuple[list[int], list[int]]:
    """(channels that die to the zero point, channels that die to a non-zero constant) among the channels ``live`` as shipped: spread over the
    lane groups / channel tiles of the kernels (first, last, and two inside)."""
    n = live.size
    tiny = sorted({0, n - 1, (5 + 7 * salt) % n})
    const = sorted({(2 + 3 * salt) % n, (n // 2 + 1 + salt) % n} - set(tiny))
    return live[tiny].tolist(), live[const].tolist()


def dead(seed: int = 0):
    """Dead channels — weight scales so small that the requantisation shift exceeds ``STRIP_MAX_SHIFT`` (22), which the lowering rewrites to
    ``multiplier 0, e = 1, c1 = 1 + 2 q`` — in the stem and in the depthwise and the pointwise stage of EVERY block: stage 1 (front block and
    strip kernel), stage 2 and stage 3-4, the first block of each chain kernel and the later ones, pointwise stages with and without ADD.
    Two kinds per layer: shift 30 (the output is the zero point, q = 0) and shift 23 with the channel's weights cut to [-4, 4] and a large
    bias, so that the constant is q = 3 (or -3 / 5 for the own term of a residual block, which may be negative).  A shift beyond 31 is not
    expressible (``quantize_multiplier`` returns (0, 0), a shift of 0, which no strip form takes), hence 30 at most."""
    m = shipped()
    stem, blocks = backbone(m)
    layers = [(stem, False)] + [(o, b["add"] is not None and o is b["pw"]) for b in blocks for o in (b["dw"], b["pw"])]
    for k, (op, is_own) in enumerate(layers):
        mult, w, b = get_mult(m, op), get_w(m, op).astype(np.int64), get_b(m, op)
        _, zp_in = qp(m, op.inputs[0])
        tiny, const = _dead_channels(np.nonzero(mult >= 2.0**-23)[0], k + seed)
        mult[tiny] = DEAD_TINY
        for c in const:
            w[c] = np.clip(w[c], -4, 4)
            b[c] = 0
            mult[c] = DEAD_CONST
        set_w(m, op, w)
        set_b(m, op, b)
        lo, hi = acc_bounds(m, op)
        for j, c in enumerate(const):   # the centre of the proven range (at most 4 * 256 * 255 wide: 0.03 of a step) at q + 0.2
            q = 3 if not is_own else (-3, 5)[j % 2]
            b[c] = int(round((q + 0.2) / DEAD_CONST)) - int(lo[c] + hi[c]) // 2
        set_w(m, op, w)
        set_b(m, op, b)
        set_mult(m, op, mult)
    return m


def _calibration_maps(model) -> np.ndarray:
    """The stem's int8 input for a handful of calibration chunks (the frontend is the shipped one in every family)."""
    from oracle.int8_graph import Int8Interpreter

    stem, _ = backbone(model)
    _, env = Int8Interpreter(_shipped_cached()).invoke(boundary_inputs(8, seed=5)[[0, 1, 7, 4]], return_all=True)
    return env[stem.inputs[0]]


def edge(seed: int = 0):
    """Every backbone weight at +-127, multipliers and biases chosen layer by layer from accumulator statistics on four calibration chunks
    (own numpy forward, ``conv_acc``), so that the activations keep a spread instead of collapsing onto one clamp end:

    * depthwise: channels 4k all +127 and 4k + 1 all -127 (the rest random signs).  The all-positive ones keep bias 0 and map their whole
      proven range [0, 9 * 127 * 255] onto ~1.3 output ranges: an input patch pinned at the upper clamp puts the accumulator AT its bound.
      The others map the 10 % .. 90 % span of their accumulators onto ~1.6 output ranges around the middle (both clamp ends are reached);
    * pointwise without ADD and the stem: the same, with every eighth channel shifted to sit mostly at the upper / lower clamp;
    * pointwise with ADD (own term): the largest multiplier the lowering accepts — ``|v| < 2^11`` over the PROVEN accumulator range
      (``tail2_constants``) is the binding condition with weights of +-127, so the multiplier is 1900 / max(|lo|, |hi|): +-127 weights at the
      shipped scales are refused (the plan would lose the matrix-core forms), this is the nearest accepted choice.  Biases put channel 4k
      around own = -100 and 4k + 1 around +140, i.e. beyond the int8 clamp of the own value on either side, the rest around 0."""
    from birdnet_stm32.models import _quant as qz

    m, rng = shipped(), np.random.default_rng(15_000 + seed)
    stem, blocks = backbone(m)
    x = _calibration_maps(m)

    def spread_layer(op, x):
        C = get_w(m, op).shape[0]
        w = rng.choice((-127, 127), size=get_w(m, op).shape)
        dwise = op.name == "DEPTHWISE_CONV_2D"
        if dwise:
            w[0::4], w[1::4] = 127, -127
        set_w(m, op, w)
        set_b(m, op, np.zeros(C, np.int64))
        acc = conv_acc(m, op, x).reshape(-1, C)
        p10, p50, p90 = np.percentile(acc, (10, 50, 90), axis=0)
        lo, hi = act_bounds(m, op)
        _, z = qp(m, op.outputs[0])
        mult = 1.6 * (hi - lo) / np.maximum(p90 - p10, 1.0)
        centre = np.full(C, (lo + hi) / 2.0 - z)
        if not dwise:
            centre[7::8] += 0.6 * (hi - lo)
            centre[6::8] -= 0.6 * (hi - lo)
        bias = np.rint(centre / mult - p50)
        if dwise:
            blo, bhi = acc_bounds(m, op)
            mult[0::4] = 1.3 * (hi - lo) / bhi[0::4]
            bias[0::4] = 0
        mult = np.clip(mult, 2.0**-20, 0.45)
        set_mult(m, op, mult)
        set_b(m, op, bias)
        return np.clip(requant(m, op, conv_acc(m, op, x)) + z, lo, hi).astype(np.int8)

    x = spread_layer(stem, x)
    for blk in blocks:
        res = x
        x = spread_layer(blk["dw"], x)
        pw = blk["pw"]
        if blk["add"] is None:
            x = spread_layer(pw, x)
            continue
        C = get_w(m, pw).shape[0]
        set_w(m, pw, rng.choice((-127, 127), size=get_w(m, pw).shape))
        set_b(m, pw, np.zeros(C, np.int64))
        acc = conv_acc(m, pw, x).reshape(-1, C)
        lo0, hi0 = acc_bounds(m, pw)
        mult = 1900.0 / np.maximum(np.abs(lo0), np.abs(hi0))       # bias 0 first: the wanted offsets, then the multiplier with the bias in the bound
        want = np.zeros(C)
        want[0::4], want[1::4] = -100.0, 140.0
        bias = np.rint(want / mult - np.median(acc, axis=0))
        set_b(m, pw, bias)
        lo1, hi1 = acc_bounds(m, pw)
        set_mult(m, pw, 1900.0 / np.maximum(np.abs(lo1), np.abs(hi1)))
        _, z = qp(m, pw.outputs[0])
        own = np.clip(requant(m, pw, conv_acc(m, pw, x)) + z, -128, 127)
        x = add_params(m, blk).apply(res.astype(np.int64), own).astype(np.int8)
    assert qz is not None
    return m


# residual blocks in graph order: (own scale / residual scale, own zero point, divisor of the shipped pointwise multipliers)
_SCALE_DESIGN = (
    None,                    # stage 1 (strip kernel: the ADD is a table there, no rescale form) — as shipped
    (2.5, 0, 1.0),           # stage 2: e1 = 2, the smallest the lowering accepts
    (60000.0, -19, 64.0),    #          e1 = 16, the largest
    (3.0, -20, 1.0),         # stage 3: e1 = 2
    (64.0, -15, 8.0),        #          e1 = 6
    (1024.0, -4, 64.0),      #          e1 = 10
    (60000.0, -20, 64.0),    # stage 4: e1 = 16
)


def scale(seed: int = 0):
    """Scale and zero point of the residual blocks' own value moved so that the residual rescale shift ``e1`` (``tail2_constants``: ``R = 2^10 +
    2^(10 + e1)``) takes 2, 6, 10 and 16 in the two chain kernels — 16 is the largest the lowering takes (``-s1 > 16`` is refused), 2 the
    smallest: ``e1 = 0`` (own scale = residual scale, the branch where R has no second term) and ``e1 = 1`` (own scale up to twice the
    residual's) are refused for EVERY own zero point, because the proof that the unclamped own term saturates the sum needs an own step of
    more than two output steps.  So that branch of the lowering is unreachable with a fused plan, and this family takes the nearest values.
    The pointwise multipliers of those blocks are divided by up to 64 so that the own value stays a mix of zero and non-zero steps.
    In every depthwise stage and every pointwise stage without ADD, channels 16k + 3 get the multiplier 0.3 (shift 1, the smallest a strip
    form takes), 16k + 7 get 0.75 * 2^-22 (shift 22, the largest that is not dead) and 16k + 11 get 0.6 * 2^-18; pointwise stages WITH ADD
    get the two large shifts only — a shift of 1 there breaks ``|v| < 2^11`` for any channel with more than a few non-zero weights."""
    m = shipped()
    stem, blocks = backbone(m)
    k = 0
    for blk in blocks:
        if blk["add"] is None:
            continue
        design = _SCALE_DESIGN[k]
        k += 1
        if design is None:
            continue
        r, z_own, div = design
        pw, own = blk["pw"], m.tensors[blk["pw"].outputs[0]]
        mult = get_mult(m, pw)
        res = next(t for t in blk["add"].inputs if t != pw.outputs[0])
        own.scale = np.asarray([np.float32(qp(m, res)[0] * r)], np.float32)
        own.zero_point = np.asarray([z_own], np.int64)
        set_mult(m, pw, np.where(mult < 2.0**-23, mult, mult / div))   # (channels that are dead as shipped stay where they are)
    assert k == len(_SCALE_DESIGN)
    for op, is_own in [(stem, False)] + [(o, b["add"] is not None and o is b["pw"]) for b in blocks for o in (b["dw"], b["pw"])]:
        mult = get_mult(m, op)
        new = mult.copy()
        if not is_own:
            new[3::16] = 0.3
        new[7::16] = 0.75 * 2.0**-22
        new[11::16] = 0.6 * 2.0**-18
        set_mult(m, op, np.where(mult < 2.0**-23, mult, new))   # (channels dead as shipped carry biases beyond 2^30: they stay dead)
    return m


_BUILDERS = {"perm": perm, "sign": sign, "dense": dense, "dead": dead, "edge": edge, "scale": scale}


def mutant(family: str, seed: int = 0):
    return _BUILDERS[family](seed)


def all_mutants() -> list[tuple[str, int]]:
    return [(f, s) for f, seeds in FAMILIES.items() for s in seeds]


# ------------------------------------------------------------------------------------------------ what the plan chose
def plan_forms(plan) -> dict:
    """Kernel forms of a production plan: fused stage-2 operator, fused tail, its matrix-core constants, constant blocks of the front and
    strip kernels."""
    from birdnet_stm32.models import _pack as pk

    ops = plan.ops
    tail = [o for o in ops if o.kind == pk.I8_TAIL]
    front = [o for o in ops if o.kind == pk.I8_FRONT]
    strips = [o for o in ops if o.kind == pk.I8_DWPW and o.get("has_dw") == 1 and not o.p[pk.TAIL_TAG]]
    return dict(mid=sum(o.kind == pk.I8_MID for o in ops), tail=len(tail),
                tail2=bool(tail and tail[0].get("cst2") >= 0 and tail[0].get("desc2") >= 0),
                front_strip=bool(front and front[0].get("strip_cst") >= 0), strip=[bool(o.get("strip_cst") >= 0) for o in strips])


def ledger(model, S: np.ndarray) -> dict:
    """What the lowering's constants say and what ONE oracle run on the spectrograms ``S`` produced, per block of the backbone:

    ``dead[(stage, kind)]``  channels with a requantisation shift beyond 22 (kind: stem / dw / pw / pw+add);
    ``shifts``               (smallest, largest) shift among the live channels of the whole backbone;
    ``e1``                   residual rescale shift of every residual block, in graph order;
    ``blocks``               per block: stage, first, dead channels of its two stages, share of the output map at the lower / upper clamp, max |acc| / max(|lo|, |hi|) of the
                             depthwise and the pointwise stage, and for residual blocks the share of own terms outside the int8 clamp before
                             it acts (pointwise accumulator recomputed from the oracle's depthwise output, ``_quant.requantize``), the share
                             of negative own terms and the largest |v| relative to 2^11."""
    from oracle.int8_graph import Int8Interpreter

    _, env = Int8Interpreter(model).invoke(S, return_all=True)
    stem, blocks = backbone(model)
    dead_n: dict = {}
    live_e: list[int] = []

    def count(op, stage, kind) -> int:
        e = -fixed_point(model, op)[1].astype(np.int64)
        dead_n[(stage, kind)] = dead_n.get((stage, kind), 0) + int((e > 22).sum())
        live_e.extend(e[e <= 22].tolist())
        return int((e > 22).sum())

    def ratio(op):
        acc = conv_acc(model, op, env[op.inputs[0]])
        lo, hi = acc_bounds(model, op)
        assert (acc >= lo).all() and (acc <= hi).all(), "an accumulator outside the proven range"
        live = (-fixed_point(model, op)[1].astype(np.int64) <= 22) & (hi > lo)   # (dead and all-zero channels say nothing about the range)
        a = acc[..., live]
        top = float((np.abs(a) / np.maximum(np.abs(lo), np.abs(hi))[live]).max())
        pos = (a - lo[live]) / (hi - lo)[live]
        return acc, top, float(pos.min()), float(pos.max())

    count(stem, "stage1", "stem")
    rows, e1s = [], []
    for blk in blocks:
        dw, pw, add = blk["dw"], blk["pw"], blk["add"]
        n_dw = count(dw, blk["stage"], "dw")
        n_pw = count(pw, blk["stage"], "pw+add" if add is not None else "pw")
        out = env[blk["out"]]
        lo, hi = act_bounds(model, add if add is not None else pw)
        _, r_dw, dw_min, dw_max = ratio(dw)
        acc_pw, r_pw, _, _ = ratio(pw)
        row = dict(stage=blk["stage"], first=blk["first"], add=add is not None, at_lo=float((out == lo).mean()), at_hi=float((out == hi).mean()),
                   dw_ratio=r_dw, dw_pos=(dw_min, dw_max), pw_ratio=r_pw, dead_dw=n_dw, dead_pw=n_pw)
        if add is not None:
            _, z = qp(model, pw.outputs[0])
            v = requant(model, pw, acc_pw)
            assert np.array_equal(np.clip(v + z, -128, 127), env[pw.outputs[0]].astype(np.int64)), "own-term recomputation differs from the oracle"
            row.update(own_outside=float(((v + z < -128) | (v + z > 127)).mean()), own_negative=float((v < 0).mean()), v_max=float(np.abs(v).max() / 2048.0))
            e1 = -add_params(model, blk).sh1
            row["e1"] = e1
            e1s.append(e1)
        rows.append(row)
    return dict(dead=dead_n, shifts=(min(live_e), max(live_e)), e1=e1s, blocks=rows)


def format_ledger(name: str, forms: dict, led: dict) -> str:
    """One paragraph per model: the forms, the dead channels per stage and kind, one line per block."""
    dead_txt = ", ".join(f"{s}/{k} {n}" for (s, k), n in sorted(led["dead"].items()) if n) or "none"
    head = (f"{name}: mid={forms['mid']} tail={forms['tail']} tail2={int(forms['tail2'])} front_strip={int(forms['front_strip'])} "
            f"strip={[int(v) for v in forms['strip']]} | live shifts {led['shifts'][0]}..{led['shifts'][1]} | e1 {led['e1']} | dead: {dead_txt}")
    lines = [head]
    for i, r in enumerate(led["blocks"]):
        own = f" own_outside={r['own_outside']:.4f} own_neg={r['own_negative']:.3f} |v|/2^11={r['v_max']:.3f} e1={r['e1']}" if r["add"] else ""
        lines.append(f"  block {i:2d} {r['stage']:8s}{' first' if r['first'] else '      '} dead={r['dead_dw']}/{r['dead_pw']} at_lo={r['at_lo']:.3f} at_hi={r['at_hi']:.3f} "
                     f"dw|acc|/bound={r['dw_ratio']:.3f} dw_pos={r['dw_pos'][0]:.2f}..{r['dw_pos'][1]:.2f} pw|acc|/bound={r['pw_ratio']:.3f}{own}")
    return "\n".join(lines)
