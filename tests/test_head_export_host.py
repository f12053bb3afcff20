"""Host tests of the head export (birdnet_stm32/conversion/head_export.py): the grafted graph against the numpy specification, bit for bit,
through the FlatBuffer writer and the lowering; nothing in front of the classifier moves; the specification's error against the float64
head stays inside the bound the roundings give; refusals; save / load.  No GPU."""
from __future__ import annotations

import copy
import dataclasses
import os

import numpy as np
import pytest

import i8_mutants as im
import i8_variants as iv

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIPPED = os.path.join(REPO, "birdnet-stm32_amd", "checkpoints", "birdnet_stm32n6_100")
EMB_TENSOR, FC_OP = 127, 53   # the shipped graph's pooled tensor and its classifier (tests/test_oracle_pinning.py pins both)


def make_head(D, C, activation="sigmoid", spread=0.1, seed=0):
    from birdnet_stm32.training.linear_probe import ProbeHead

    rng = np.random.default_rng([seed, D, C])
    return ProbeHead(rng.normal(0.0, spread, (D, C)), rng.normal(0.0, 1.0, C), activation, [f"class{j}" for j in range(C)])


def float_logits(head, rows, s_in, z_in):
    return ((rows.astype(np.float64) - z_in) * float(np.float32(s_in))) @ head.W.astype(np.float64) + head.b.astype(np.float64)


def quantized(head, rows, s_in, z_in, per_tensor=False):
    from birdnet_stm32.conversion.head_export import quantize_head

    z = float_logits(head, rows, s_in, z_in)
    return quantize_head(head, s_in, z_in, float(z.min()), float(z.max()), per_tensor)


@pytest.fixture(scope="module")
def shipped():
    m = im.shipped()
    t = m.tensors[EMB_TENSOR]
    assert m.ops[FC_OP].name == "FULLY_CONNECTED" and m.ops[FC_OP].inputs[0] == EMB_TENSOR
    return m, float(t.scale[0]), int(t.zero_point[0])


@pytest.fixture(scope="module")
def pooled(shipped):
    """The interpreter's own pooled bytes of the first four shared inputs (the classifier does not feed them: one run serves every head)."""
    _, env = iv.oracle(shipped[0], iv.inputs()[:4])
    return np.ascontiguousarray(env[EMB_TENSOR].reshape(4, -1)).astype(np.int8)


@pytest.mark.parametrize("per_tensor", [False, True], ids=["per_channel", "per_tensor"])
@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
@pytest.mark.parametrize("C", [1, 7, 100, 129])
def test_grafted_graph_equals_the_specification(shipped, pooled, C, activation, per_tensor):
    from birdnet_stm32.conversion.head_export import find_classifier, graft_head, head_scores_i8_reference
    from birdnet_stm32.models._lower_i8 import lower_i8
    from birdnet_stm32.models._tflite_reader import parse_tflite
    from birdnet_stm32.models._tflite_writer import write_tflite

    model, s_in, z_in = shipped
    head = make_head(256, C, activation, seed=C)
    cal = np.random.default_rng(C).integers(-128, 128, (64, 256)).astype(np.int8)
    qh = quantized(head, np.concatenate([cal, pooled]), s_in, z_in, per_tensor)
    assert (len(set(qh.w_scale.tolist())) == 1) == (per_tensor or C == 1)
    grafted = parse_tflite(write_tflite(graft_head(model, qh)))
    plan = lower_i8(grafted)
    assert plan.num_classes == C and len(plan.to_blob()) > 0
    f = find_classifier(grafted)
    assert (f["logistic"] is not None) == (activation == "sigmoid") and (f["softmax"] is not None) == (activation == "softmax")
    assert [o.index for o in grafted.ops] == list(range(len(grafted.ops)))

    out, env = iv.oracle(grafted, iv.inputs()[:4])
    assert np.array_equal(env[EMB_TENSOR].reshape(4, -1), pooled)
    want_bytes, want_scores = head_scores_i8_reference(qh, pooled)
    got_bytes = env[grafted.ops[f["fc"]].outputs[0]].reshape(4, C)
    assert np.array_equal(got_bytes, want_bytes)
    assert out.shape == (4, C) and out.dtype == np.float32
    assert np.array_equal(out, want_scores)   # (softmax: the float32 softmax of equal bytes, in the interpreter's own operations)
    # the numbers mean something: the INT8 scores follow the float head
    z = float_logits(head, pooled, s_in, z_in)
    ref = 1 / (1 + np.exp(-z)) if activation == "sigmoid" else np.exp(z - z.max(1, keepdims=True)) / np.exp(z - z.max(1, keepdims=True)).sum(1, keepdims=True)
    assert np.abs(out - ref).max() < 0.05


def test_grafts_onto_grafted_graphs(shipped, pooled):
    """Every pair of (backbone head, new head): the shipped graph has a sigmoid head, so the branches that start from a softmax head — LOGISTIC
    and its tensor put back, the DEQUANTIZE rewired to the output; softmax onto softmax — run on graphs grafted here.  Each step goes through
    the writer and the reader and must lower, equal the specification bit for bit and keep the tensor table free of leftovers."""
    from birdnet_stm32.conversion.head_export import find_classifier, graft_head, head_scores_i8_reference
    from birdnet_stm32.models._lower_i8 import lower_i8
    from birdnet_stm32.models._tflite_reader import parse_tflite
    from birdnet_stm32.models._tflite_writer import write_tflite

    model, s_in, z_in = shipped
    n_tensors = {"sigmoid": len(model.tensors), "softmax": len(model.tensors)}   # FC -> LOGISTIC -> DEQUANTIZE and FC -> DEQUANTIZE -> SOFTMAX: three tensors either way
    for step, (activation, C) in enumerate((("softmax", 7), ("sigmoid", 17), ("sigmoid", 3), ("softmax", 129), ("softmax", 5), ("sigmoid", 100))):
        qh = quantized(make_head(256, C, activation, seed=step), pooled, s_in, z_in, per_tensor=bool(step % 2))
        model = parse_tflite(write_tflite(graft_head(model, qh)))
        f = find_classifier(model)
        assert (f["logistic"] is not None) == (activation == "sigmoid") and (f["softmax"] is not None) == (activation == "softmax"), step
        assert len(model.tensors) == n_tensors[activation] and [t.index for t in model.tensors] == list(range(len(model.tensors)))
        used = {k for op in model.ops for k in op.inputs + op.outputs if k >= 0}
        assert used == set(range(len(model.tensors))), f"step {step}: tensors without an operator"
        assert lower_i8(model).num_classes == C
        out, env = iv.oracle(model, iv.inputs()[:4])
        want_bytes, want_scores = head_scores_i8_reference(qh, pooled)
        assert np.array_equal(env[model.ops[f["fc"]].outputs[0]].reshape(4, C), want_bytes), step
        assert np.array_equal(out, want_scores), step


@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
def test_nothing_in_front_of_the_classifier_moved(shipped, activation):
    from birdnet_stm32.conversion.head_export import graft_head
    from birdnet_stm32.models._tflite_reader import parse_tflite
    from birdnet_stm32.models._tflite_writer import write_tflite

    model, s_in, z_in = shipped
    before = copy.deepcopy(model)
    rows = np.random.default_rng(1).integers(-128, 128, (32, 256)).astype(np.int8)
    grafted = graft_head(model, quantized(make_head(256, 7, activation), rows, s_in, z_in))
    fc = model.ops[FC_OP]
    head_tensors = set(fc.inputs[1:3]) | {o for op in model.ops[FC_OP:] for o in op.outputs}
    for g in (grafted, parse_tflite(write_tflite(grafted))):
        for a, b in zip(model.ops[:FC_OP], g.ops[:FC_OP]):
            assert (a.index, a.name, a.inputs, a.outputs, a.options) == (b.index, b.name, b.inputs, b.outputs, b.options)
        for t in model.tensors:
            if t.index in head_tensors:
                continue
            u = g.tensors[t.index]
            assert (t.index, t.name, tuple(t.shape), t.dtype, t.quantized_dimension) == (u.index, u.name, tuple(u.shape), u.dtype, u.quantized_dimension)
            assert np.array_equal(t.scale, u.scale) and np.array_equal(t.zero_point, u.zero_point)
            assert (t.data is None) == (u.data is None) and (t.data is None or (t.data.dtype == u.data.dtype and np.array_equal(t.data, u.data)))
        assert g.inputs == model.inputs
    # and the backbone the caller handed in is untouched
    for a, b in zip(before.tensors, model.tensors):
        assert tuple(a.shape) == tuple(b.shape) and np.array_equal(a.scale, b.scale) and (a.data is None or np.array_equal(a.data, b.data))
    assert [(o.name, o.inputs, o.outputs) for o in before.ops] == [(o.name, o.inputs, o.outputs) for o in model.ops]


def test_error_against_the_float_head_stays_inside_the_roundings_bound():
    """Sigmoid scores of the specification against the float64 head.  Per element the bound is the sigmoid's largest slope (1/4) times the
    roundings of the logit — weights (half a step each, times |x_k|), bias (half a step at s_in s_w), the logit byte (half a step of
    s_out, 1 % for the Q31 multiplier) and the table's float32 argument — plus one step of the 1/256 output."""
    from birdnet_stm32.conversion.head_export import head_scores_i8_reference

    worst, cases = 0.0, 0
    for D in (16, 50, 64, 80, 256, 320):
        for C in (1, 15, 16, 17, 100, 129):
            for n in (1, 63, 65, 300):
                for spread in (0.02, 0.1, 0.5):
                    seed = cases
                    rng = np.random.default_rng(seed)
                    s_in, z_in = float(np.float32(rng.uniform(0.005, 0.05))), int(rng.choice([-128, -128, -20, 0, 37]))
                    rows = rng.integers(-128, 128, (n, D)).astype(np.int8)
                    rows.reshape(-1)[: min(256, rows.size)] = np.arange(-128, 128, dtype=np.int64)[: min(256, rows.size)].astype(np.int8)   # every byte value
                    head = make_head(D, C, "sigmoid", spread, seed)
                    qh = quantized(head, rows, s_in, z_in, per_tensor=bool(seed % 2))
                    _, got = head_scores_i8_reference(qh, rows)
                    want = 1.0 / (1.0 + np.exp(-float_logits(head, rows, s_in, z_in)))
                    x_abs = (np.abs(rows.astype(np.float64) - z_in) * s_in).sum(axis=1)[:, None]
                    s_w = qh.w_scale.astype(np.float64)[None, :]
                    bound = 0.25 * (x_abs * s_w / 2 + s_in * s_w / 2 + 1.01 * qh.s_out / 2 + qh.s_out * 2.0**-7) + 1.0 / 256
                    ratio = float((np.abs(got.astype(np.float64) - want) / bound).max())
                    worst, cases = max(worst, ratio), cases + 1
                    assert ratio <= 1.0, f"D={D} C={C} n={n} spread={spread}: error / bound = {ratio:.3f}"
    print(f"\n{cases} cases, worst error / bound = {worst:.3f}")


def test_refusals(shipped, tmp_path):
    from birdnet_stm32.conversion.head_export import export_head_tflite, find_classifier, graft_head, quantize_head
    from birdnet_stm32.training.linear_probe import ProbeHead

    model, s_in, z_in = shipped
    rows = np.random.default_rng(2).integers(-128, 128, (16, 256)).astype(np.int8)
    with pytest.raises(ValueError, match="INT8 .tflite"):   # a float backbone, before anything is read
        export_head_tflite(make_head(256, 3), SHIPPED + ".keras", rows, str(tmp_path / "x.tflite"))
    assert not os.path.exists(tmp_path / "x.tflite")
    narrow = np.random.default_rng(2).integers(-128, 128, (16, 128)).astype(np.int8)
    with pytest.raises(ValueError, match="width 128"):   # a head of another width
        graft_head(model, quantized(make_head(128, 3), narrow, s_in, z_in))
    with pytest.raises(ValueError, match="scale"):   # ... or quantised for other embedding parameters
        graft_head(model, quantized(make_head(256, 3), rows, s_in * 2, z_in))
    with pytest.raises(ValueError, match="zero point"):
        graft_head(model, quantized(make_head(256, 3), rows, s_in, z_in + 1))
    # graphs without a classifier behind pooling: cut at the embedding; a classifier that reads the map in front of the pooling
    cut = dataclasses.replace(copy.deepcopy(model), ops=copy.deepcopy(model.ops[:FC_OP]), outputs=[EMB_TENSOR])
    with pytest.raises(ValueError, match="no classifier behind pooling"):
        find_classifier(cut)
    moved = copy.deepcopy(model)
    moved.ops[FC_OP].inputs[0] = moved.ops[FC_OP - 1].inputs[0]
    with pytest.raises(ValueError, match="no classifier behind pooling"):
        graft_head(moved, quantized(make_head(256, 3), rows, s_in, z_in))
    # accumulators that can leave int32: a row of 70000 weights at +-127 next to a bias at the clamp (no device head is that wide; the rule is the lowering's)
    wide = ProbeHead(np.full((70000, 2), 0.5), np.array([1e9, -1e9]), "sigmoid", ["a", "b"])
    with pytest.raises(ValueError, match="overflow int32"):
        quantize_head(wide, 0.01, -128, -5.0, 5.0)
    with pytest.raises(ValueError, match="logit range"):
        quantize_head(make_head(256, 3), s_in, z_in, 1.0, float("nan"))


def test_probe_refuses_an_export_before_any_audio(shipped, tmp_path):
    """``check_export_args`` is what ``probe`` runs before it lists a folder: a ``.keras``, a ``.tflite`` whose pooled tensor is float32, and
    one without a classifier behind pooling are refused there; the shipped INT8 file and a command without the flag pass."""
    import argparse

    from birdnet_stm32.models._tflite_writer import write_tflite
    from birdnet_stm32.training.linear_probe import check_export_args

    model = shipped[0]
    ns = lambda path, on=True: argparse.Namespace(model_path=str(path), export_tflite=on, min_cosine_sim=0.95)  # noqa: E731
    assert check_export_args(ns(SHIPPED + ".tflite")) is True and check_export_args(ns(SHIPPED + ".keras", on=False)) is False
    with pytest.raises(ValueError, match="INT8 .tflite"):
        check_export_args(ns(SHIPPED + ".keras"))
    floaty = copy.deepcopy(model)   # the tail of a float graph: float32 tensors without quantisation from the pooling on
    for k in [EMB_TENSOR] + [o for op in floaty.ops[FC_OP:] for o in op.outputs]:
        t = floaty.tensors[k]
        t.dtype, t.scale, t.zero_point = np.dtype(np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64)
    path = tmp_path / "float_tail.tflite"
    path.write_bytes(write_tflite(floaty))
    with pytest.raises(ValueError, match="not an INT8 model"):
        check_export_args(ns(path))
    cut = dataclasses.replace(copy.deepcopy(model), ops=copy.deepcopy(model.ops[:FC_OP]), outputs=[EMB_TENSOR])
    path = tmp_path / "cut.tflite"
    path.write_bytes(write_tflite(cut))
    with pytest.raises(ValueError, match="no classifier behind pooling"):
        check_export_args(ns(path))
    bad = ns(SHIPPED + ".tflite")
    bad.min_cosine_sim = 1.5
    with pytest.raises(ValueError, match="min_cosine_sim"):
        check_export_args(bad)


@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
def test_save_and_load_round_trip(tmp_path, activation):
    from birdnet_stm32.conversion.head_export import QuantizedHead, head_scores_i8_reference

    rows = np.random.default_rng(3).integers(-128, 128, (40, 80)).astype(np.int8)
    qh = quantized(make_head(80, 17, activation), rows, 0.02, -128, per_tensor=activation == "softmax")
    path = str(tmp_path / "head_i8.npz")
    qh.save(path)
    back = QuantizedHead.load(path)
    for f in dataclasses.fields(QuantizedHead):
        a, b = getattr(qh, f.name), getattr(back, f.name)
        assert (a is None and b is None) or (isinstance(a, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)) or (not isinstance(a, np.ndarray) and a == b), f.name
    for x, y in zip(head_scores_i8_reference(qh, rows), head_scores_i8_reference(back, rows)):
        assert np.array_equal(x, y)
    with np.load(path, allow_pickle=False) as z:   # a plain archive
        assert z["w"].dtype == np.int8 and z["w"].shape == (17, 80)
