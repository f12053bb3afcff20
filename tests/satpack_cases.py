"""Models for the tests of the packed shift-and-saturate epilogues (option ``i8_satpack``), derived in memory from the shipped INT8 graph,
and a numpy restatement of the instruction.  Plain helper module: no fixtures, no test functions.

``narrow_relu6()``  the ReLU6 output of the depthwise stage of the stride-2 block that opens stage 2 and of the one that opens stage 3 gets
                    its scale doubled: the upper clamp bound ``zp + 6 / scale`` falls from 127 to 0, a clamp the instruction's
                    saturation does not cover, in one block of each chain kernel.
``add_zero_point()`` the ADD output of the last residual block of stage 3 and of stage 4 gets zero point -120: behind the graph's fused ReLU6 the
                    lower bound of the stored byte is then -120.  (The consumers of these two tensors — a block that reads its taps from
                    LDS, and MEAN — take any zero point; a residual block behind it or the first block of a chain would not.)
"""
from __future__ import annotations

import numpy as np

import i8_mutants as im


def narrow_relu6():
    m = im.shipped()
    _, blocks = im.backbone(m)
    for stage in ("stage2", "stage3-4"):
        blk = next(b for b in blocks if b["stage"] == stage and b["first"])
        t = m.tensors[blk["dw"].outputs[0]]
        assert blk["dw"].options["activation"] == "relu6" and int(t.zero_point[0]) == -128
        t.scale = (t.scale.astype(np.float64) * 2.0).astype(np.float32)
        assert im.act_bounds(m, blk["dw"])[1] < 127
    return m


def add_zero_point(zp: int = -120):
    m = im.shipped()
    _, blocks = im.backbone(m)
    tail = [b for b in blocks if b["stage"] == "stage3-4" and b["add"] is not None]
    widths = sorted({int(m.tensors[b["out"]].shape[2]) for b in tail})
    for w in widths:   # the last residual block of stage 3 (16 wide) and of stage 4 (8 wide)
        blk = [b for b in tail if int(m.tensors[b["out"]].shape[2]) == w][-1]
        t = m.tensors[blk["out"]]
        assert int(t.zero_point[0]) == -128
        assert blk["add"].options["activation"] == "relu6"
        t.zero_point = np.asarray([zp], t.zero_point.dtype)
    return m


def chain_bounds(plan) -> dict:
    """form ('mid' / 'tail2') -> per block (dw_lo, dw_hi, pw_lo, pw_hi, add_lo, add_hi, has_add) from the descriptor tables of a lowered plan."""
    from birdnet_stm32.models import _pack as pk

    out = {}
    for o in plan.ops:
        if o.kind == pk.I8_MID:
            name, desc, nl = "mid", plan.tensors[o.get("desc")].reshape(-1), o.get("n_layers")
        elif o.kind == pk.I8_TAIL and o.get("desc2") >= 0:
            name, desc, nl = "tail2", plan.tensors[o.get("desc2")].reshape(-1), o.get("n_layers")
        else:
            continue
        out[name] = [tuple(int(v) for v in desc[32 * i + np.array([11, 12, 13, 14, 18, 19, 9])]) for i in range(nl)]
    return out


def bounds_full(rows) -> bool:
    """The library's predicate (``tail2_satpack_ok``) restated on ``chain_bounds`` rows."""
    return all((dl, dh) == (-128, 127) and ((al, ah) if add else (pl, ph)) == (-128, 127) for dl, dh, pl, ph, al, ah, add in rows)


# ------------------------------------------------------------------------------------------------ the instruction in numpy
def sat_i8(v):
    return np.clip(v, -128, 127)


def ashr_pk(a, b, s):
    """``v_ashr_pk_i8_i32``: the 16-bit result, byte 0 from ``a``, byte 1 from ``b``; ``s`` counts with its low five bits."""
    s = np.asarray(s, np.int64) & 31
    return (sat_i8(np.asarray(a, np.int64) >> s) & 0xFF) | ((sat_i8(np.asarray(b, np.int64) >> s) & 0xFF) << 8)


def perm(s0, s1, sel: int):
    """``v_perm_b32`` for selectors 0..7: byte k of the result = byte sel[k] of the 8 bytes (s1 = bytes 0-3, s0 = bytes 4-7)."""
    both = (np.asarray(s1, np.int64) & 0xFFFFFFFF) | ((np.asarray(s0, np.int64) & 0xFFFFFFFF) << 32)
    out = np.zeros_like(both)
    for k in range(4):
        idx = (sel >> (8 * k)) & 0xFF
        assert idx < 8
        out |= ((both >> (8 * idx)) & 0xFF) << (8 * k)
    return out
