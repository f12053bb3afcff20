"""Packed model blob writer — the Python side of ``csrc/bn_blob.h``.

``bn_model_load`` (include/birdnet_hip.h) takes one self-contained byte string: a header,
the activation-slot table, the tensor table, the operator table and 256-byte-aligned tensor
payloads.  The lowering passes (``_lower_f32`` for `.keras`, ``_lower_i8`` for `.tflite`)
describe a device plan through :class:`PlanBuilder`; this module lays it out.  Every constant
here mirrors ``bn_blob.h`` and is asserted against the library at load time through
``bn_version``/the blob version field.
"""

from __future__ import annotations

import struct
from dataclasses import dataclass, field

import numpy as np

BLOB_MAGIC = b"BNHIPM01"
BLOB_VERSION = 5

DTYPE_F32, DTYPE_I8 = 0, 1
INPUT_SPECTROGRAM, INPUT_WAVEFORM, INPUT_MEL = 0, 1, 2

SLOT_INPUT, SLOT_SCORES, SLOT_LOGITS, SLOT_AUDIO, SLOT_NONE = -1, -2, -3, -4, -9
OP_PATH, PATH_BOTH, PATH_INPUT, PATH_AUDIO = 39, 0, 1, 2

OP_NP, OP_NT, OP_NF = 40, 16, 8

# operator kinds (enum BnOpKind)
F32_MEL, F32_MAG, F32_RAWFE, F32_STEM, F32_DW, F32_PW = 1, 2, 3, 4, 5, 6
F32_SEGATE, F32_SCALE, F32_GAP, F32_DENSE, F32_ATTNPOOL, F32_DWPW, F32_STFTMEL, F32_MELFIN, F32_FRONT, F32_GAPDENSE = 7, 8, 9, 10, 11, 12, 13, 14, 15, 16
I8_QUANT, I8_MEL, I8_STEM, I8_DW, I8_PW, I8_MEAN, I8_FC, I8_HEAD, I8_DWPW, I8_FRONT, I8_TAIL, I8_SCALE, I8_MAXNORM, I8_RAWFE, I8_ATTNPOOL, I8_MID = 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35
TAIL_TAG = 38  # OpRec.p[TAIL_TAG] = TAIL_COVERED: the operator is covered by the plan's fused tail operator; TAIL_OP: it is that operator
TAIL_COVERED, TAIL_OP = 0x7A110001, 0x7A110002  # (bn_blob.h; values no other use of p[38] can take)
MID_COVERED, MID_OP = 0x7A11000E, 0x7A11000F    # the same for the fused stage-2 chain (i8_mid2_kernel)
EMB_TAG, EMB_DIM, EMB_ZP, EMB_SCALE = 36, 35, 34, 7  # OpRec.p[EMB_TAG] = EMB_OP: the operator's result is the embedding (bn_blob.h);
EMB_OP = 0x7A110010                                  # p[EMB_DIM] = D, INT8: p[EMB_ZP] = zero point, f[EMB_SCALE] = scale
EMB_KINDS = (25, 30, 34, 9, 11, 16)                  # I8_MEAN, I8_TAIL, I8_ATTNPOOL, F32_GAP, F32_ATTNPOOL, F32_GAPDENSE
FRONT2_HEAD, FRONT2_COVERED = 0x7A110003, 0x7A110004  # front block + the residual block FRONT2_DIST operators further on may run as one kernel
FRONT2_DIST = 37
PWDW8_HEAD, PWDW8_COVERED = 0x7A11000C, 0x7A11000D  # the INT8 counterpart (i8_pwdw_kernel)
PWDW_STEM = 0x7A11000B  # a stem convolution whose only reader is a PWDW pair: the fused kernel may compute the stem rows itself
PWDW_HEAD, PWDW_COVERED = 0x7A110009, 0x7A11000A  # expand 1x1 + the depthwise 3x3 behind it (inverted-residual blocks) may run as one kernel
SEGATE_HEAD, SEGATE_COVERED = 0x7A110007, 0x7A110008  # an I8_MEAN operator and the two I8_FC operators of a squeeze-excite gate behind it: may run as one kernel
SCALE_HEAD, SCALE_COVERED = 0x7A110005, 0x7A110006  # an I8_SCALE operator and the plain 1x1 convolution right behind it, its only reader: may run as one kernel

KIND_NAMES = {
    F32_MEL: "f32_mel", F32_MAG: "f32_mag", F32_RAWFE: "f32_rawfe", F32_STEM: "f32_stem", F32_DW: "f32_dw",
    F32_PW: "f32_pw", F32_SEGATE: "f32_segate", F32_SCALE: "f32_scale", F32_GAP: "f32_gap", F32_DENSE: "f32_dense",
    F32_ATTNPOOL: "f32_attnpool", F32_DWPW: "f32_dwpw", F32_STFTMEL: "f32_stftmel", F32_MELFIN: "f32_melfin", F32_FRONT: "f32_front", F32_GAPDENSE: "f32_gapdense", I8_QUANT: "i8_quant", I8_MEL: "i8_mel", I8_STEM: "i8_stem", I8_DW: "i8_dw",
    I8_PW: "i8_pw", I8_DWPW: "i8_dwpw", I8_FRONT: "i8_front", I8_MEAN: "i8_mean", I8_FC: "i8_fc", I8_HEAD: "i8_head", I8_TAIL: "i8_tail", I8_SCALE: "i8_scale", I8_MAXNORM: "i8_maxnorm", I8_RAWFE: "i8_rawfe", I8_ATTNPOOL: "i8_attnpool", I8_MID: "i8_mid",
}  # fmt: skip

# ---- operator-record fields: the Python mirror of csrc/bn_ops.h ---------------------------------------------------------------------
# OP_FIELDS[kind] = (names of p[0..], names of t[0..], names of f[0..]) in index order; tests/test_lowering_and_abi.py compares the table
# with the enumerators of bn_ops.h.  A kind's names are unique across its three arrays, so one name addresses one entry.  rsvN: an entry
# the kind leaves at its default.  The cross-kind entries (OP_PATH, TAIL_TAG, FRONT2_DIST, EMB_*) keep the fixed indices above.


def _geom(c: str, p5: str) -> tuple:
    """The ten conv-geometry fields STEM / DW / DWPW of both plans start with (bn_ops.h: BN_OP_GEOM)."""
    return ("H", "W", c, "sh", "sw", p5, "OH", "OW", "pt", "pl")


ADD_FIELDS = ("has_add", "add_z1", "add_m1", "add_s1", "add_m2", "add_s2", "add_mo", "add_so", "add_zo", "add_amin", "add_amax")  # bn_ops.h: BN_OP_ADD
_RQ = ("w", "bias", "mult", "shift")
_FRONT_T = ("stem_w", "stem_b", "dw_w", "dw_b", "pw_w", "pw_b")
_FRONT8_T = ("stem_w", "stem_b", "stem_mult", "stem_shift", "dw_w", "dw_b", "dw_mult", "dw_shift", "pw_w", "pw_b", "pw_mult", "pw_shift")
_CHAIN = ("n_layers", "H0", "W0", "C0", "P_last", "C_last")

OP_FIELDS = {
    F32_MEL: (("F", "W", "M", "mag", "norm"), ("wvals", "bands", "magp"), ()),
    F32_MAG: (("M", "W", "mag"), ("rsv0", "rsv1", "magp"), ()),
    F32_RAWFE: (("T", "W", "M", "stride", "pad_left", "mag"), ("fb", "bias", "magp"), ()),
    F32_STEM: (_geom("Cout", "act"), ("w", "bias"), ()),
    F32_DW: (_geom("C", "act"), ("w", "bias"), ()),
    F32_PW: (("P", "Cin", "Cout", "act", "has_res", "has_gate", "gate_slot"), ("w", "bias"), ()),
    F32_SEGATE: (("P", "C", "Cr"), ("w1", "w2"), ()),
    F32_SCALE: (("P", "C"), (), ()),
    F32_GAP: (("P", "C"), (), ()),
    F32_DENSE: (("Cin", "Cout", "act"), ("w", "bias"), ()),
    F32_ATTNPOOL: (("P", "C"), ("score",), ()),
    F32_DWPW: (_geom("Cin", "dw_act") + ("Cout", "pw_act", "has_res", "has_gate", "gate_slot", "has_dw", "TH", "TW", "NB"),
               ("dw_w", "dw_b", "pw_w", "pw_b"), ()),
    F32_STFTMEL: (("T", "W", "M"), ("wvals", "bands"), ()),
    F32_MELFIN: (("M", "W", "mag", "norm"), ("wsum", "rsv1", "magp"), ()),
    F32_FRONT: (("H0", "W0", "C", "N", "OH", "OW", "stem_act", "dw_act", "pw_act", "raw_mel", "mag"), _FRONT_T + ("wsum", "magp"), ()),
    F32_GAPDENSE: (("P", "Cin", "Cout", "act"), ("w", "bias"), ()),
    I8_QUANT: (("F", "W", "Kp", "zp", "fill"), (), ("scale",)),
    I8_MEL: (("W", "Kp", "M", "zp_out", "act_min", "act_max", "has_lut"), _RQ + ("lut",), ()),
    I8_STEM: (_geom("Cout", "rsv5") + ("zp_in", "zp_out", "act_min", "act_max"), _RQ, ()),
    I8_DW: (_geom("C", "rsv5") + ("zp_in", "zp_out", "act_min", "act_max"), _RQ, ()),
    I8_PW: (("P", "Cin", "Cout", "zp_out", "act_min", "act_max") + ADD_FIELDS, _RQ, ()),
    I8_MEAN: (("P", "C", "zp_in", "mult", "shift", "zp_out"), (), ()),
    I8_FC: (("Cin", "Cout", "zp_out", "act_min", "act_max", "has_lut"), _RQ + ("lut",), ()),
    I8_HEAD: (("C", "zp_fc", "zp_out", "has_lut", "softmax"), ("lut",), ("s_fc", "s_out", "beta")),
    I8_DWPW: (_geom("Cin", "qF") + ("dw_zp_in", "dw_zp_out", "dw_amin", "dw_amax", "Cout", "pw_zp_out", "pw_amin", "pw_amax") + ADD_FIELDS
              + ("has_dw", "transposed", "TH", "TW", "NB", "has_lut", "strip", "q_at_load", "qzp", "qfill"),
              ("dw_w", "dw_b", "dw_mult", "dw_shift", "pw_w", "pw_b", "pw_mult", "pw_shift", "lut", "strip_cst", "add_tab"), ("qscale",)),
    I8_FRONT: (("H0", "W0", "C", "N", "OH", "OW", "stem_zp_in", "stem_zp_out", "stem_amin", "stem_amax", "dw_zp_out", "dw_amin", "dw_amax",
                "pw_zp_out", "pw_amin", "pw_amax", "strip"), _FRONT8_T + ("strip_cst",), ()),
    I8_TAIL: (("in_bytes", "pw_macs", "dw_macs", "other_macs", "n_classes") + _CHAIN, ("cst", "desc", "cst2", "desc2"), ("s_fc", "s_head")),
    I8_SCALE: (("P", "C", "zp_x", "zp_gate", "mult", "shift", "zp_out", "act_min", "act_max"), (), ()),
    I8_MAXNORM: (("C", "W", "has_lut"), ("denom", "div", "lut"), ()),
    I8_RAWFE: (("T", "W", "M", "stride", "pad_left", "q_zp", "zp_out", "act_min", "act_max", "has_lut"), _RQ + ("lut",), ("q_scale",)),
    I8_ATTNPOOL: (("P", "C", "fc_bias", "fc_mult", "fc_shift", "fc_zo", "form", "zx", "za", "mul_mult", "mul_shift", "mul_zo", "mul_lo", "mul_hi",
                   "sum_mult", "sum_shift", "sum_zo"), ("score", "tables"), ()),
    I8_MID: (("in_bytes", "pw_macs", "dw_macs", "rsv3", "rsv4") + _CHAIN, ("cst", "desc"), ()),
}
for _k, _pf in OP_FIELDS.items():
    _all = _pf[0] + _pf[1] + _pf[2]
    assert len(set(_all)) == len(_all) and len(_pf[0]) <= OP_PATH and len(_pf[1]) <= OP_NT and len(_pf[2]) <= OP_NF, KIND_NAMES[_k]

ACT_CODES = {"none": 0, "linear": 0, "relu": 1, "relu6": 2}
MAG_CODES = {"none": 0, "pwl": 1, "pcen": 2, "db": 3}


@dataclass(frozen=True)
class PlanEmbedding:
    """Where a plan's embedding comes from: ``ops`` maps each entry path ("input": bn_forward, "audio": bn_infer_audio) to the marked
    operator that produces it with the default launcher options; ``marked`` lists every marked operator (an INT8 plan marks its unfused
    MEAN and the fused tail operator that covers it).  ``scale`` / ``zero_point`` dequantise the int8 form (1.0 / 0 on float32 plans)."""

    ops: dict
    marked: tuple
    dim: int
    dtype: str
    scale: float
    zero_point: int


def _align(n: int, a: int = 256) -> int:
    return (n + a - 1) // a * a


@dataclass
class PlanOp:
    """One device-plan operator plus what tests need to interpret its output."""

    kind: int
    in0: int
    in1: int
    out: int
    p: list[int]
    t: list[int]
    f: list[float]
    name: str = ""  # reference layer / tflite tensor this output corresponds to
    out_shape: tuple = ()  # per chunk
    out_dtype: str = "float32"

    def _entry(self, name: str) -> tuple[list, int]:
        for arr, names in zip((self.p, self.t, self.f), OP_FIELDS[self.kind]):
            if name in names:
                return arr, names.index(name)
        raise KeyError(f"{KIND_NAMES[self.kind]} has no field '{name}'")

    def get(self, name: str):
        """The entry of p / t / f that ``OP_FIELDS`` names ``name`` for this operator's kind."""
        arr, i = self._entry(name)
        return arr[i]

    def set(self, name: str, value) -> None:
        arr, i = self._entry(name)
        arr[i] = value


@dataclass
class Plan:
    """A lowered model: operators, constant tensors, slot sizes and header facts."""

    dtype: int
    input_kind: int
    input_elems: int
    fft_bins: int
    spec_width: int
    num_classes: int
    ops: list[PlanOp] = field(default_factory=list)
    tensors: list[np.ndarray] = field(default_factory=list)
    slot_bytes: list[int] = field(default_factory=list)
    meta: dict = field(default_factory=dict)

    def to_blob(self) -> bytes:
        return pack_plan(self)

    @property
    def embedding(self) -> PlanEmbedding | None:
        """The marked embedding operator(s) of this plan, or None when lowering found no pooled vector in front of a classifier."""
        marked = tuple(i for i, o in enumerate(self.ops) if o.p[EMB_TAG] == EMB_OP)
        if not marked:
            return None
        first = self.ops[marked[0]]
        i8 = self.dtype == DTYPE_I8
        ops = {}
        for name, path in (("input", PATH_INPUT), ("audio", PATH_AUDIO)):
            run = [i for i in marked if self.ops[i].p[OP_PATH] in (PATH_BOTH, path)]
            fused = [i for i in run if self.ops[i].p[TAIL_TAG] == TAIL_OP]   # the fused tail covers the MEAN whenever it runs
            ops[name] = (fused or run or [None])[0]
        return PlanEmbedding(ops, marked, int(first.p[EMB_DIM]), "int8" if i8 else "float32",
                             float(first.f[EMB_SCALE]) if i8 else 1.0, int(first.p[EMB_ZP]) if i8 else 0)


class PlanBuilder:
    """Collects operators over symbolic activation values, then maps values to slots.

    Lowering passes call :meth:`value` for every operator output and refer to values by id.
    :meth:`finalize` runs a linear scan over the operator list: with ``reuse=True`` a slot is
    recycled once the last reader of its value has run (an output never aliases a value that
    is still live, so no kernel runs in place unless its operator says so; ``_extra_uses`` keeps
    the inputs of an operator alive up to a later operator that may run fused with it); with
    ``reuse=False`` every value keeps its own slot so that tests can read each intermediate
    activation back through ``bn_debug_op_output``.
    """

    def __init__(self, plan: Plan):
        self.plan = plan
        self._value_bytes: list[int] = []
        self._gate_refs: list[tuple[int, int]] = []  # (op index, p index) holding a value id
        self._extra_uses: list[tuple[int, int]] = []  # (op index, value id): the value must stay live until that operator has run

    def tensor(self, arr: np.ndarray, dtype) -> int:
        a = np.ascontiguousarray(np.asarray(arr).astype(dtype))
        self.plan.tensors.append(a)
        return len(self.plan.tensors) - 1

    def value(self, nbytes: int) -> int:
        self._value_bytes.append(_align(int(nbytes), 256))
        return len(self._value_bytes) - 1

    def op(self, kind, in0, out, p=None, t=None, f=None, in1=SLOT_NONE, name="", out_shape=(), out_dtype="float32",
           value_params=(), path=PATH_BOTH, tag=0) -> PlanOp:
        """Append an operator.  ``p`` / ``t`` / ``f`` map field names of ``OP_FIELDS[kind]`` to values (entries left out keep 0 / -1 / 0.0);
        a name the kind does not have in that array raises.  ``value_params``: names of p entries that hold a value id; ``tag``: p[TAIL_TAG]."""
        names = OP_FIELDS[kind]

        def fill(given, which, n, default, conv):
            arr = [default] * n
            for k, v in (given or {}).items():
                if k not in names[which]:
                    raise ValueError(f"{KIND_NAMES[kind]}: '{k}' is not a field of {'ptf'[which]}")
                arr[names[which].index(k)] = conv(v)
            return arr

        pp, tt, ff = fill(p, 0, OP_NP, 0, int), fill(t, 1, OP_NT, -1, int), fill(f, 2, OP_NF, 0.0, float)
        pp[OP_PATH] = int(path)
        if tag:  # (I8_DWPW's qfill shares the index: see the stated exception in bn_ops.h)
            pp[TAIL_TAG] = int(tag)
        o = PlanOp(kind, int(in0), int(in1), int(out), pp, tt, ff, name, tuple(out_shape), out_dtype)
        for pn in value_params:
            self._gate_refs.append((len(self.plan.ops), names[0].index(pn)))
        self.plan.ops.append(o)
        return o

    def finalize(self, reuse: bool = True) -> Plan:
        ops = self.plan.ops
        refs: dict[int, list[int]] = {}
        for oi, pi in self._gate_refs:
            refs.setdefault(oi, []).append(pi)
        last_use: dict[int, int] = {}
        for oi, o in enumerate(ops):
            for v in [o.in0, o.in1, o.out] + [o.p[pi] for pi in refs.get(oi, [])]:
                if v >= 0:
                    last_use[v] = oi
        extra: dict[int, list[int]] = {}
        for oi, v in self._extra_uses:
            last_use[v] = max(last_use.get(v, oi), oi)
            extra.setdefault(oi, []).append(v)
        slot_of: dict[int, int] = {}
        slot_bytes: list[int] = []
        free: list[int] = []
        for oi, o in enumerate(ops):
            if o.out >= 0 and o.out not in slot_of:
                need = self._value_bytes[o.out]
                if reuse and free:
                    sid = min(free, key=lambda s: (slot_bytes[s] < need, abs(slot_bytes[s] - need)))
                    free.remove(sid)
                    slot_bytes[sid] = max(slot_bytes[sid], need)
                else:
                    slot_bytes.append(need)
                    sid = len(slot_bytes) - 1
                slot_of[o.out] = sid
            if reuse:
                for v in {o.in0, o.in1, o.out, *[o.p[pi] for pi in refs.get(oi, [])], *extra.get(oi, [])}:
                    if v >= 0 and last_use[v] == oi and v in slot_of and slot_of[v] not in free:
                        free.append(slot_of[v])
        for oi, o in enumerate(ops):
            o.in0 = slot_of[o.in0] if o.in0 >= 0 else o.in0
            o.in1 = slot_of[o.in1] if o.in1 >= 0 else o.in1
            o.out = slot_of[o.out] if o.out >= 0 else o.out
            for pi in refs.get(oi, []):
                o.p[pi] = slot_of[o.p[pi]]
        self.plan.slot_bytes = slot_bytes
        return self.plan


def mark_embedding(op: PlanOp, dim: int, scale: float = 0.0, zero_point: int = 0) -> None:
    """Tag ``op`` as the producer of the plan's embedding (see :class:`PlanEmbedding`)."""
    if op.kind not in EMB_KINDS:
        raise ValueError(f"operator kind {op.kind} cannot carry the embedding")
    op.p[EMB_TAG] = EMB_OP
    op.p[EMB_DIM] = int(dim)
    op.p[EMB_ZP] = int(zero_point)
    op.f[EMB_SCALE] = float(scale)


def pack_plan(plan: Plan) -> bytes:
    """Serialise ``plan`` into the byte layout ``bn_model_load`` parses."""
    n_slots, n_tensors, n_ops = len(plan.slot_bytes), len(plan.tensors), len(plan.ops)
    op_size = 16 + 4 * (OP_NP + OP_NT + OP_NF)
    slots_off = 64
    tensors_off = slots_off + 8 * n_slots
    ops_off = tensors_off + 16 * n_tensors
    data_off = _align(ops_off + op_size * n_ops)

    tensor_recs = []
    payload = bytearray()
    for arr in plan.tensors:
        off = data_off + len(payload)
        raw = arr.tobytes()
        tensor_recs.append((off, len(raw)))
        payload += raw
        payload += b"\x00" * (_align(len(payload)) - len(payload))

    out = bytearray()
    out += struct.pack(
        "<8s14I", BLOB_MAGIC, BLOB_VERSION, plan.dtype, plan.input_kind, plan.input_elems, plan.fft_bins,
        plan.spec_width, plan.num_classes, n_slots, n_tensors, n_ops, slots_off, tensors_off, ops_off, 0,
    )  # fmt: skip
    assert len(out) == 64
    for nb in plan.slot_bytes:
        out += struct.pack("<Q", nb)
    for off, nb in tensor_recs:
        out += struct.pack("<QQ", off, nb)
    for o in plan.ops:
        out += struct.pack(f"<4i{OP_NP}i{OP_NT}i{OP_NF}f", o.kind, o.in0, o.in1, o.out, *o.p, *o.t, *o.f)
    out += b"\x00" * (data_off - len(out))
    out += payload
    return bytes(out)
