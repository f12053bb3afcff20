"""A trained probe head as the classifier of an INT8 `.tflite`: quantise it, graft it onto the backbone's graph, write the file.

The reference's ``train --linear_probe`` ends in a model that ``convert`` quantises and ``deploy`` ships (reference:
birdnet_stm32/training/linear_probe.py, conversion/quantize.py).  Here ``probe`` trains its head on the embeddings of a frozen INT8
backbone, so nothing in front of the classifier changes: the exported file is the backbone's graph with the FULLY_CONNECTED behind the
pooling replaced by the new head, quantised by the rules of this build's own quantiser (``conversion/quantize.py``):

* weights ``[C, D]``: symmetric int8 per class row (one common scale with ``per_tensor``) — ``quantize_weights``;
* bias: int32 at ``float32(emb_scale) * s_w[c]``, clamped to +-2^30 — the bias rule of ``quantize_graph``;
* logit tensor: ``choose_activation_params`` of the range the caller observed; requantisation: ``channel_multipliers``;
* sigmoid heads: LOGISTIC with output 1 / 256, -128 as ``logistic_table``; softmax heads: DEQUANTIZE and a float32 SOFTMAX.

:func:`head_scores_i8_reference` is the numpy specification of what the exported tail computes; ``bn_head_i8_forward``
(csrc/bn_head_i8.hip, :meth:`QuantizedHead.predict_device`) computes the same bits over resident int8 embedding rows, so ``embed --dtype
int8`` archives are scored as the board will score them without running the backbone again.
"""

from __future__ import annotations

import copy
from dataclasses import dataclass, field

import numpy as np

from birdnet_stm32.conversion.quantize import choose_activation_params, quantize_weights
from birdnet_stm32.models import _quant as qz
from birdnet_stm32.models._tflite_reader import BUILTIN_NAMES, TfliteModel, TfliteOp, TfliteTensor

ACTIVATIONS = ("sigmoid", "softmax")
_LOGISTIC_OUT = (1.0 / 256.0, -128)   # TFLite fixes the int8 LOGISTIC's output parameters
_CODE_OF = {v: k for k, v in BUILTIN_NAMES.items()}


@dataclass
class QuantizedHead:
    """An INT8 classifier head over int8 embedding rows at ``(emb_scale, emb_zero_point)``; everything the exported tail is made of."""

    w: np.ndarray                 # int8 [C, D]
    w_scale: np.ndarray           # float32 [C] (equal entries with per_tensor)
    bias: np.ndarray              # int32 [C] at emb_scale * w_scale[c]
    s_out: float                  # the logit tensor's scale ...
    z_out: int                    # ... and zero point
    mult: np.ndarray              # int32 [C] Q31 multipliers of emb_scale * w_scale[c] / s_out
    shift: np.ndarray             # int32 [C] their exponents
    lut: np.ndarray | None        # int8 [256] LOGISTIC table by byte + 128 (sigmoid), None (softmax)
    activation: str
    class_names: list = field(default_factory=list)
    emb_scale: float = 1.0
    emb_zero_point: int = 0
    per_tensor: bool = False

    def __post_init__(self):
        self.w = np.ascontiguousarray(self.w, np.int8)
        self.w_scale, self.bias = np.ascontiguousarray(self.w_scale, np.float32), np.ascontiguousarray(self.bias, np.int32)
        self.mult, self.shift = np.ascontiguousarray(self.mult, np.int32), np.ascontiguousarray(self.shift, np.int32)
        self.lut = None if self.lut is None else np.ascontiguousarray(self.lut, np.int8)
        self.s_out, self.z_out = float(np.float32(self.s_out)), int(self.z_out)
        self.emb_scale, self.emb_zero_point, self.per_tensor = float(np.float32(self.emb_scale)), int(self.emb_zero_point), bool(self.per_tensor)
        self.class_names = [str(c) for c in self.class_names]
        C = self.w.shape[0]
        if self.w.ndim != 2 or any(a.shape != (C,) for a in (self.w_scale, self.bias, self.mult, self.shift)):
            raise ValueError("w must be [C, D] and the scales, bias, multipliers and shifts [C]")
        if self.activation not in ACTIVATIONS:
            raise ValueError(f"activation must be one of {ACTIVATIONS}, not {self.activation!r}")
        if (self.lut is not None) != (self.activation == "sigmoid") or (self.lut is not None and self.lut.shape != (256,)):
            raise ValueError("a sigmoid head carries its 256-entry LOGISTIC table, a softmax head none")
        if self.class_names and len(self.class_names) != C:
            raise ValueError(f"{len(self.class_names)} class names for {C} classes")
        self._device = {}   # per device index: [own context or None, constants on the device]

    @property
    def num_classes(self) -> int:
        return int(self.w.shape[0])

    @property
    def embedding_dim(self) -> int:
        return int(self.w.shape[1])

    def folded_bias(self) -> np.ndarray:
        """``bias - z_in * sum_k w[c, k]`` (int64): the bias the accumulators of the raw bytes take, as ``lower_i8`` folds it."""
        return self.bias.astype(np.int64) - self.emb_zero_point * self.w.astype(np.int64).sum(axis=1)

    def save(self, path: str) -> None:
        """A plain ``.npz`` (``np.load(path)`` reads it without this package)."""
        np.savez(path, w=self.w, w_scale=self.w_scale, bias=self.bias, s_out=np.float32(self.s_out), z_out=np.int64(self.z_out), mult=self.mult,
                 shift=self.shift, lut=self.lut if self.lut is not None else np.zeros(0, np.int8), activation=np.str_(self.activation),
                 class_names=np.asarray(self.class_names, dtype=np.str_), emb_scale=np.float32(self.emb_scale),
                 emb_zero_point=np.int64(self.emb_zero_point), per_tensor=np.bool_(self.per_tensor))

    @classmethod
    def load(cls, path: str) -> "QuantizedHead":
        with np.load(path, allow_pickle=False) as z:
            return cls(z["w"], z["w_scale"], z["bias"], float(z["s_out"]), int(z["z_out"]), z["mult"], z["shift"], z["lut"] if z["lut"].size else None,
                       str(z["activation"]), [str(c) for c in z["class_names"]], float(z["emb_scale"]), int(z["emb_zero_point"]), bool(z["per_tensor"]))

    # -- on the device ---------------------------------------------------------------------------------------------------------------
    def close(self) -> None:
        """Drop the device copies of the constants and close the contexts ``predict`` opened for itself (none when it was given one)."""
        for slot in self._device.values():
            if slot[0] is not None:
                slot[0].close()
        self._device = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _constants(self, device):
        import torch

        D = self.embedding_dim
        w_pad = np.zeros((self.num_classes, -(-D // 64) * 64), np.int8)   # the kernel's B operand: rows of whole 64-byte chunks, zero beyond D
        w_pad[:, :D] = self.w
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        return {"w": up(w_pad), "bias": up(self.folded_bias().astype(np.int32)), "mult": up(self.mult), "shift": up(self.shift),
                "lut": None if self.lut is None else up(self.lut)}

    def predict_device(self, rows_i8, ctx=None, return_logit_bytes: bool = False):
        """Scores ``[N, C]`` (CUDA float32) of a CUDA int8 tensor ``[N, D]`` of embedding bytes (``bn_head_i8_forward``); with
        ``return_logit_bytes`` also the requantised classifier output ``[N, C]`` int8.  ``rows_i8`` may be any view whose rows are
        contiguous and lie one behind the other.  ``ctx``: the caller's ``_hip.Context``; without one the head opens its own per device."""
        import ctypes

        import torch

        from birdnet_stm32 import _hip

        if not (rows_i8.is_cuda and rows_i8.dtype == torch.int8 and rows_i8.dim() == 2 and rows_i8.is_contiguous()):
            raise ValueError("rows must be a contiguous int8 CUDA tensor [N, D]")
        if int(rows_i8.shape[1]) != self.embedding_dim:
            raise ValueError(f"the head takes embeddings of width {self.embedding_dim}, the rows are {int(rows_i8.shape[1])} wide")
        dev = rows_i8.device.index or 0
        if dev not in self._device:
            self._device[dev] = [None, self._constants(rows_i8.device)]
        slot = self._device[dev]
        if ctx is None:
            ctx = slot[0] = slot[0] or _hip.Context(dev, 1)
        k = slot[1]
        n, C = int(rows_i8.shape[0]), self.num_classes
        scores = torch.empty((n, C), dtype=torch.float32, device=rows_i8.device)
        softmax = self.activation == "softmax"
        logit = torch.empty((n, C), dtype=torch.int8, device=rows_i8.device) if (softmax or return_logit_bytes) else None
        with torch.cuda.device(rows_i8.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(rows_i8.device).cuda_stream)
            _hip.check(ctx.lib.bn_head_i8_forward(ctx.handle, rows_i8.data_ptr(), n, self.embedding_dim, k["w"].data_ptr(), k["bias"].data_ptr(),
                                                  k["mult"].data_ptr(), k["shift"].data_ptr(), C, self.z_out, None if k["lut"] is None else k["lut"].data_ptr(),
                                                  _hip.PROBE_ACTIVATIONS[self.activation], ctypes.c_float(self.s_out),
                                                  None if logit is None else logit.data_ptr(), scores.data_ptr(), stream))
        return (scores, logit) if return_logit_bytes else scores

    def predict(self, rows, ctx=None, device: int = 0):
        """Scores of int8 embedding rows: a numpy array in gives a numpy array, a CUDA tensor a CUDA tensor.  Always on the device."""
        import torch

        if isinstance(rows, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(rows, np.int8)).to(f"cuda:{getattr(ctx, 'device', device)}")
            return self.predict_device(t, ctx).cpu().numpy()
        return self.predict_device(rows, ctx)


# -- quantise -------------------------------------------------------------------------------------------------------------------------
def quantize_head(head, emb_scale: float, emb_zero_point: int, logit_lo: float, logit_hi: float, per_tensor: bool = False, hidden_units=0) -> QuantizedHead:
    """Quantise ``head`` (a ``ProbeHead``: ``W [D, C]``, ``b [C]``) for int8 embeddings at ``(emb_scale, emb_zero_point)`` whose logits
    were seen in ``[logit_lo, logit_hi]``.  Deterministic: the same arguments give the same head.  A head with a hidden layer
    (``head.W1``, or ``hidden_units > 0``) is refused: the export is built for the linear head only."""
    from birdnet_stm32.models._lower_i8 import _expect_acc_range
    from birdnet_stm32.training.linear_probe import refuse_hidden

    refuse_hidden("quantize_head", hidden_units, head)
    if not (np.isfinite(logit_lo) and np.isfinite(logit_hi) and logit_lo <= logit_hi):
        raise ValueError(f"bad logit range [{logit_lo}, {logit_hi}]")
    if not (np.isfinite(emb_scale) and emb_scale > 0 and -128 <= int(emb_zero_point) <= 127):
        raise ValueError(f"bad embedding parameters: scale {emb_scale}, zero point {emb_zero_point}")
    W, b = np.asarray(head.W, np.float64), np.asarray(head.b, np.float64)
    if not (np.isfinite(W).all() and np.isfinite(b).all()):
        raise ValueError("the head's weights are not finite")
    C = W.shape[1]
    q, s_w = quantize_weights(W.T, 0, per_tensor)                                      # [C, D] int8, [C] float32
    s_b = np.float64(np.float32(emb_scale)) * s_w.astype(np.float64)                   # the bias rule of quantize_graph
    bias = np.clip(np.round(b / s_b), -(2**30), 2**30).astype(np.int32)
    s_out, z_out = choose_activation_params(logit_lo, logit_hi)
    mult, shift = qz.channel_multipliers(emb_scale, s_w, s_out, C)
    lut = qz.logistic_table(s_out, z_out, *_LOGISTIC_OUT) if head.activation == "sigmoid" else None
    qh = QuantizedHead(q, s_w, bias, s_out, z_out, mult, shift, lut, head.activation, list(head.class_names), emb_scale, emb_zero_point, per_tensor)
    try:
        _expect_acc_range(qh.w, qh.folded_bias(), 1, "the exported head", qh.mult, qh.shift)
    except NotImplementedError as exc:
        raise ValueError(f"the head cannot be exported: {exc}") from None
    return qh


def head_scores_i8_reference(qhead: QuantizedHead, rows_i8) -> tuple[np.ndarray, np.ndarray]:
    """The specification: ``(logit bytes [n, C] int8, scores [n, C] float32)`` of int8 embedding rows ``[n, D]``."""
    rows = np.asarray(rows_i8)
    if rows.dtype != np.int8 or rows.ndim != 2 or rows.shape[1] != qhead.embedding_dim:
        raise ValueError(f"rows must be int8 [n, {qhead.embedding_dim}]")
    acc = rows.astype(np.int64) @ qhead.w.astype(np.int64).T + qhead.folded_bias()[None, :]
    q = np.clip(qz.requantize(acc, qhead.mult.astype(np.int64)[None, :], qhead.shift.astype(np.int64)[None, :]) + qhead.z_out, -128, 127).astype(np.int8)
    if qhead.activation == "sigmoid":
        out = qhead.lut[q.astype(np.int32) + 128]
        return q, ((out.astype(np.int32) + 128).astype(np.float32) / np.float32(256.0)).astype(np.float32)
    logits = ((q.astype(np.int32) - qhead.z_out).astype(np.float32) * np.float32(qhead.s_out)).astype(np.float32)
    e = np.exp(logits - logits.max(axis=-1, keepdims=True), dtype=np.float32)
    return q, (e / e.sum(axis=-1, keepdims=True, dtype=np.float32)).astype(np.float32)


# -- graft ----------------------------------------------------------------------------------------------------------------------------
def find_classifier(model: TfliteModel) -> dict:
    """The classifier of an INT8 graph, found by data flow from the output backwards the way ``_mark_embedding`` finds the embedding:
    pooling -> FULLY_CONNECTED -> [LOGISTIC ->] DEQUANTIZE [-> SOFTMAX].  ``{"pool", "fc", "logistic", "dequantize", "softmax"}`` are
    operator positions (None where the head has none).  ``ValueError`` when the graph has no such tail."""
    writer = {o: i for i, op in enumerate(model.ops) for o in op.outputs}
    consumers: dict[int, list[int]] = {}
    for i, op in enumerate(model.ops):
        for k in op.inputs:
            consumers.setdefault(k, []).append(i)

    def refuse(why):
        raise ValueError(f"no classifier behind pooling in this graph ({why}): the head of an INT8 model this build's exporters write ends in "
                         "pooling -> FULLY_CONNECTED -> [LOGISTIC ->] DEQUANTIZE [-> SOFTMAX]")

    def producer(ti, names, what):
        i = writer.get(ti)
        if i is None or model.ops[i].name not in names:
            refuse(f"{what} expected in front of tensor {ti}")
        return i

    if len(model.outputs) != 1:
        refuse("more than one output")
    found = {"softmax": None, "logistic": None}
    at = producer(model.outputs[0], ("SOFTMAX", "DEQUANTIZE"), "DEQUANTIZE or SOFTMAX")
    if model.ops[at].name == "SOFTMAX":
        found["softmax"] = at
        at = producer(model.ops[at].inputs[0], ("DEQUANTIZE",), "DEQUANTIZE")
    found["dequantize"] = at
    at = producer(model.ops[at].inputs[0], ("LOGISTIC", "FULLY_CONNECTED"), "LOGISTIC or FULLY_CONNECTED")
    if model.ops[at].name == "LOGISTIC":
        if found["softmax"] is not None:
            refuse("LOGISTIC and SOFTMAX in one head")
        found["logistic"] = at
        at = producer(model.ops[at].inputs[0], ("FULLY_CONNECTED",), "FULLY_CONNECTED")
    found["fc"] = at
    fc = model.ops[at]
    if len(fc.inputs) < 3 or fc.inputs[2] < 0 or model.tensors[fc.inputs[1]].data is None or model.tensors[fc.inputs[2]].data is None:
        refuse("the FULLY_CONNECTED has no constant weights and bias")
    found["pool"] = producer(fc.inputs[0], ("MEAN", "SUM"), "MEAN or attention pooling")
    order = [found[k] for k in ("pool", "fc", "logistic", "dequantize", "softmax") if found[k] is not None]
    if order[1:] != list(range(order[1], len(model.ops))):
        refuse("operators between the classifier and the output")
    for i in order[1:-1]:   # the tail is a chain: each tensor of it feeds the next operator only
        if consumers.get(model.ops[i].outputs[0], []) != [i + 1]:
            refuse(f"tensor {model.ops[i].outputs[0]} has other consumers")
    return found


def int8_embedding_of(model: TfliteModel) -> tuple[float, int, int]:
    """``(scale, zero_point, width)`` of the pooled tensor the classifier of an INT8 graph reads.  ``ValueError`` for a graph without such a
    classifier (``find_classifier``) and for a float graph: its pooled tensor is not int8 with one scale."""
    pooled = model.tensors[model.ops[find_classifier(model)["fc"]].inputs[0]]
    if pooled.dtype != np.dtype(np.int8) or pooled.scale.size != 1:
        raise ValueError(f"not an INT8 model: the pooled tensor in front of the classifier is {pooled.dtype} with {pooled.scale.size} scales; the head is "
                         "grafted onto an INT8 .tflite (heads on float backbones are not exported)")
    return float(pooled.scale[0]), int(pooled.zero_point[0]), int(pooled.shape[-1])


def graft_head(backbone: TfliteModel, qhead: QuantizedHead) -> TfliteModel:
    """``backbone`` with its classifier replaced by ``qhead``: a new model; every tensor and operator in front of the classifier is the
    backbone's own, byte for byte."""
    f = find_classifier(backbone)
    new = copy.deepcopy(backbone)
    T, ops = new.tensors, new.ops
    fc = ops[f["fc"]]
    pooled = T[fc.inputs[0]]
    D, C = qhead.embedding_dim, qhead.num_classes
    if pooled.scale.size != 1 or int(pooled.shape[-1]) != D or int(np.prod(pooled.shape)) != D:
        raise ValueError(f"the head takes embeddings of width {D}, the model's pooled tensor is {tuple(pooled.shape)}")
    if float(np.float32(pooled.scale[0])) != float(np.float32(qhead.emb_scale)) or int(pooled.zero_point[0]) != qhead.emb_zero_point:
        raise ValueError(f"the head was quantised for embeddings at scale {qhead.emb_scale:.9g}, zero point {qhead.emb_zero_point}; the model's are at "
                         f"{float(pooled.scale[0]):.9g}, {int(pooled.zero_point[0])}")
    wt, bt, logit = T[fc.inputs[1]], T[fc.inputs[2]], T[fc.outputs[0]]
    n_ws = 1 if qhead.per_tensor else C
    wt.data, wt.shape, wt.scale, wt.zero_point, wt.quantized_dimension = qhead.w.copy(), (C, D), qhead.w_scale[:n_ws].copy(), np.zeros(n_ws, np.int64), 0
    s_b = (np.float64(np.float32(qhead.emb_scale)) * qhead.w_scale[:n_ws].astype(np.float64)).astype(np.float32)
    bt.data, bt.shape, bt.scale, bt.zero_point, bt.quantized_dimension = qhead.bias.copy(), (C,), s_b, np.zeros(n_ws, np.int64), 0
    fc.options = {**fc.options, "activation": "none"}
    lead = tuple(int(v) for v in logit.shape[:-1])
    logit.shape, logit.scale, logit.zero_point = lead + (C,), np.asarray([qhead.s_out], np.float32), np.asarray([qhead.z_out], np.int64)

    deq_op, deq_out = ops[f["dequantize"]], T[ops[f["dequantize"]].outputs[0]]
    final = T[backbone.outputs[0]]
    sigmoid = qhead.activation == "sigmoid"
    tail = [fc]
    drop: set[int] = set()
    if sigmoid:
        if f["logistic"] is not None:
            lg = ops[f["logistic"]]
            prob = T[lg.outputs[0]]
        else:   # a softmax backbone: a new int8 tensor between FC and DEQUANTIZE
            prob = TfliteTensor(len(T), logit.name + "/sigmoid", lead + (C,), np.dtype(np.int8), np.zeros(0, np.float32), np.zeros(0, np.int64), 0, None)
            T.append(prob)
            lg = TfliteOp(0, _CODE_OF["LOGISTIC"], "LOGISTIC", 0, [logit.index], [prob.index], {})
        prob.shape, prob.scale, prob.zero_point = lead + (C,), np.asarray([_LOGISTIC_OUT[0]], np.float32), np.asarray([_LOGISTIC_OUT[1]], np.int64)
        deq_op.inputs = [prob.index]
        tail += [lg, deq_op]
        if f["softmax"] is not None:   # the DEQUANTIZE now ends the graph and writes the output tensor
            drop.add(deq_out.index)
            deq_op.outputs = [final.index]
    else:
        deq_op.inputs = [logit.index]
        tail.append(deq_op)
        if f["logistic"] is not None:
            drop.add(ops[f["logistic"]].outputs[0])
        if f["softmax"] is not None:
            tail.append(ops[f["softmax"]])
        else:   # a sigmoid backbone: a new float32 tensor between DEQUANTIZE and SOFTMAX; the SOFTMAX writes the output tensor
            mid = TfliteTensor(len(T), final.name + "/dequantized", lead + (C,), np.dtype(np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), 0, None)
            T.append(mid)
            deq_op.outputs = [mid.index]
            tail.append(TfliteOp(0, _CODE_OF["SOFTMAX"], "SOFTMAX", 0, [mid.index], [final.index], {"beta": 1.0}))
    for t in (deq_out, final):
        if t.index not in drop:
            t.shape = lead + (C,)
    new.ops = ops[: f["fc"]] + tail
    for i, op in enumerate(new.ops):
        op.index = i
    if drop:   # a tensor that lost its operator leaves the table; the tail's tensors come last in the files this build reads, so nothing in front moves
        keep = [t for t in T if t.index not in drop]
        remap = {t.index: i for i, t in enumerate(keep)}
        if any(k >= min(drop) for op in new.ops[: f["fc"]] for k in op.inputs + op.outputs) or any(k >= min(drop) for k in new.inputs):
            raise ValueError("tensors behind the classifier's are used in front of it: the graft would renumber them")
        for op in new.ops[f["fc"]:]:
            op.inputs = [remap.get(k, k) for k in op.inputs]
            op.outputs = [remap[k] for k in op.outputs]
        for i, t in enumerate(keep):
            t.index = i
        new.tensors = keep
        new.outputs = [remap[k] for k in new.outputs]
    new.description = (backbone.description or "") + " | classifier head grafted from a linear probe (birdnet_stm32.conversion.head_export)"
    return new


# -- export ---------------------------------------------------------------------------------------------------------------------------
def float_logit_range(head, rows_i8, emb_scale: float, emb_zero_point: int, block: int = 1 << 16) -> tuple[float, float]:
    """Smallest and largest logit of the float head over the dequantised int8 rows (a CUDA tensor stays on its device; row blocks)."""
    import torch

    W = torch.from_numpy(np.ascontiguousarray(head.W, np.float32)).to(rows_i8.device)
    b = torch.from_numpy(np.ascontiguousarray(head.b, np.float32)).to(rows_i8.device)
    lo, hi = float("inf"), float("-inf")
    for r0 in range(0, int(rows_i8.shape[0]), block):
        z = ((rows_i8[r0 : r0 + block].to(torch.float32) - float(emb_zero_point)) * float(np.float32(emb_scale))) @ W + b
        lo, hi = min(lo, float(z.min())), max(hi, float(z.max()))
    return lo, hi


def export_head_tflite(head, backbone_path: str, rows_i8, out_path: str, per_tensor: bool = False, ctx=None, logit_range=None, hidden_units=0) -> dict:
    """Write ``head`` into a copy of the INT8 model at ``backbone_path`` as ``out_path``; ``rows_i8 [n, D]`` (int8 embedding bytes, CUDA
    tensor or numpy) calibrate the logit tensor.  ``logit_range = (lo, hi)`` replaces the range observed over ``rows_i8``: the range a
    head fine-tuned by ``training.probe_qat.fit_probe_qat`` was trained against, so that the file's logit parameters are those.  Returns ``{"qhead", "logit_range", "logit_scale", "logit_zero_point", "clipped_share",
    "path", ...}``; ``clipped_share`` is the share of logit bytes at -128 or 127 over ``rows_i8`` (``bn_head_i8_forward``).  A head with a
    hidden layer (``head.W1``, or ``hidden_units > 0``) is refused before anything is read."""
    import torch

    from birdnet_stm32.models._tflite_reader import load_tflite
    from birdnet_stm32.models._tflite_writer import write_tflite
    from birdnet_stm32.training.linear_probe import refuse_hidden

    refuse_hidden("export_head_tflite", hidden_units, head)
    if not str(backbone_path).endswith(".tflite"):
        raise ValueError(f"{backbone_path}: the head is grafted onto an INT8 .tflite (heads on float backbones are not exported)")
    backbone = load_tflite(backbone_path)
    emb_scale, emb_zp, _ = int8_embedding_of(backbone)
    if isinstance(rows_i8, np.ndarray):
        rows_i8 = torch.from_numpy(np.ascontiguousarray(rows_i8, np.int8)).to(f"cuda:{getattr(ctx, 'device', 0)}")
    if rows_i8.dtype != torch.int8 or rows_i8.dim() != 2 or int(rows_i8.shape[0]) < 1:
        raise ValueError("rows_i8 must be a non-empty int8 matrix [n, D]")
    head.check_embedding_dim(rows_i8.shape[1])
    lo, hi = float_logit_range(head, rows_i8, emb_scale, emb_zp) if logit_range is None else (float(logit_range[0]), float(logit_range[1]))
    qhead = quantize_head(head, emb_scale, emb_zp, lo, hi, per_tensor)
    raw = write_tflite(graft_head(backbone, qhead))
    with open(out_path, "wb") as fh:
        fh.write(raw)
    _, logit = qhead.predict_device(rows_i8.contiguous(), ctx, return_logit_bytes=True)
    clipped = float(((logit == -128) | (logit == 127)).to(torch.float32).mean())
    return {"qhead": qhead, "path": out_path, "bytes": len(raw), "rows": int(rows_i8.shape[0]), "per_tensor": bool(per_tensor), "logit_range": [lo, hi],
            "logit_scale": qhead.s_out, "logit_zero_point": qhead.z_out, "clipped_share": clipped}
