"""Host-side tests of the probe's optional hidden layer (no GPU): the numpy specification's gradient against central differences of its
own loss, ``hidden_units=0`` as the linear fit bit for bit, the head's file format, the refusals of what is not built for such a head,
and the command line."""

import argparse

import numpy as np
import pytest

from birdnet_stm32.training import linear_probe as lp

D, H, C, B = 7, 5, 3, 4


def _step_inputs(activation, seed):
    """One step's inputs in float64: the batch after drop1 with the ones column, drop2's mask, targets and a parameter vector."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B, D))
    xd = np.concatenate([X * lp.dropout_mask(3, 0, B, D, 0.5, np.float64), np.ones((B, 1))], axis=1)
    m2 = lp.dropout_mask(3 ^ lp.DROP2_SEED_XOR, 0, B, H, 0.5, np.float64)
    W1, b1, W2, b2 = lp.init_mlp_head(D, H, C, seed)
    b1 = b1 + 0.3 * rng.standard_normal(H)
    b2 = b2 + 0.1 * rng.standard_normal(C)
    params = np.concatenate([W1.ravel(), b1, W2.ravel(), b2]).astype(np.float64)
    if activation == "softmax":
        Y = np.eye(C)[rng.integers(0, C, B)]
    else:
        Y = (rng.random((B, C)) < 0.4).astype(np.float64)
    return params, xd, m2, Y, rng


@pytest.mark.parametrize("activation,loss_kw", [("sigmoid", {}), ("softmax", {}), ("sigmoid", {"loss": "focal", "focal_gamma": 2.0, "weighted": True})])
def test_step_gradient_against_central_differences(activation, loss_kw):
    """mlp_loss_and_gradient's analytic gradient against central differences (h = 1e-5) of its own float64 loss, every parameter perturbed
    on its own; the largest error is at most 1e-5 of the largest |g|.  ReLU has a kink at a = 0: the inputs keep min |a| far above what a
    perturbation of h can move a by (h times the largest |xd| row entry, 2 with dropout 0.5 on N(0, 1) rows of up to ~3), asserted."""
    h = 1e-5
    loss_kw = dict(loss_kw)
    params, xd, m2, Y, rng = _step_inputs(activation, seed=11)
    kw = dict(loss=loss_kw.get("loss", "auto"), focal_gamma=loss_kw.get("focal_gamma", 2.0),
              sample_weight=rng.uniform(0.2, 6.0, B) if loss_kw.get("weighted") else None)
    _, g, parts = lp.mlp_loss_and_gradient(params, xd, m2, Y, activation, **kw)
    assert np.abs(parts["a"]).min() > 100 * h * np.abs(xd).max(), "an element of a lies too close to the ReLU kink for this step"
    assert (parts["a"] > 0).any() and (parts["a"] < 0).any() and (m2 == 0).any() and (m2 > 0).any()
    assert g.shape == params.shape == ((D + 1) * H + (H + 1) * C,)
    num = np.empty_like(params)
    for i in range(params.size):
        up, dn = params.copy(), params.copy()
        up[i] += h
        dn[i] -= h
        num[i] = (lp.mlp_loss_and_gradient(up, xd, m2, Y, activation, **kw)[0] - lp.mlp_loss_and_gradient(dn, xd, m2, Y, activation, **kw)[0]) / (2 * h)
    err = np.abs(num - g).max()
    print(f"{activation} {loss_kw}: max |numeric - analytic| {err:.3e}, max |g| {np.abs(g).max():.3e}")
    assert err <= 1e-5 * np.abs(g).max()
    # ... and the gradient without the ReLU gate is another vector (what the device test's second condition relies on)
    _, g_open, _ = lp.mlp_loss_and_gradient(params, xd, m2, Y, activation, relu_gate=False, **kw)
    assert np.abs(g_open - g).max() > 1e-3 * np.abs(g).max()


def _rows(n=67, d=12, c=4, seed=2):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, c, n)
    X = np.maximum(np.random.default_rng(9).standard_normal((c, d))[lab] + rng.standard_normal((n, d)), 0).astype(np.float32)
    return X, np.eye(c, dtype=np.float32)[lab]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zero_hidden_units_is_the_linear_fit_bit_for_bit(dtype):
    X, Y = _rows()
    kw = dict(activation="sigmoid", epochs=3, batch_size=16, dropout=0.5, seed=5, dtype=dtype, label_smoothing=0.1)
    a = lp.fit_probe_reference(X, Y, X[:20], Y[:20], **kw)
    b = lp.fit_probe_reference(X, Y, X[:20], Y[:20], hidden_units=0, **kw)
    assert b.W1 is None and b.hidden_units == 0
    for k in ("W", "b", "step_loss"):
        assert np.array_equal(np.asarray(a.history[k]).view(np.uint8), np.asarray(b.history[k]).view(np.uint8)), k
    assert a.history["val_loss"] == b.history["val_loss"]


def test_reference_with_a_hidden_layer_trains_and_repeats():
    X, Y = _rows(n=200)
    kw = dict(activation="softmax", epochs=12, batch_size=16, learning_rate=1e-2, dropout=0.2, seed=5, hidden_units=9)
    a = lp.fit_probe_reference(X, Y, X[:40], Y[:40], **kw)
    b = lp.fit_probe_reference(X, Y, X[:40], Y[:40], **kw)
    assert a.W1.shape == (12, 9) and a.b1.shape == (9,) and a.W.shape == (9, 4) and a.b.shape == (4,)
    assert a.embedding_dim == 12 and a.hidden_units == 9 and a.num_classes == 4
    assert a.history["loss"][-1] < 0.7 * a.history["loss"][0]
    for k in ("W1", "b1", "W", "b", "step_loss"):
        assert np.array_equal(a.history[k], b.history[k]), k
    W1, b1, W2, b2 = lp.init_mlp_head(12, 9, 4, 5)
    assert np.array_equal(W1, lp.init_head(12, 9, 5)[0]) and np.array_equal(W2, lp.init_head(9, 4, 6)[0]) and not b1.any() and not b2.any()
    # the validation loss takes the raw targets, the steps the targets smoothed once
    s = lp.fit_probe_reference(X, Y, X[:40], Y[:40], label_smoothing=0.2, **{**kw, "epochs": 1})
    P = lp.mlp_forward(X[:40].astype(np.float64), s.history["W1"], s.history["b1"], s.history["W"], s.history["b"], "softmax")
    assert s.history["val_loss"][0] == float(lp.probe_loss(P, Y[:40].astype(np.float64), "softmax"))


def _mlp_head():
    W1, b1, W2, b2 = lp.init_mlp_head(6, 4, 3, 1)
    return lp.ProbeHead(W2, b2 + 0.5, "sigmoid", ["a", "b", "c"], {"loss": [1.0, 0.5], "val_loss": [0.9]}, W1, b1 - 0.25)


def test_save_load_round_trip(tmp_path):
    head = _mlp_head()
    path = str(tmp_path / "mlp.npz")
    head.save(path)
    back = lp.ProbeHead.load(path)
    for k in ("W", "b", "W1", "b1"):
        assert np.array_equal(getattr(head, k), getattr(back, k)), k
    assert (back.embedding_dim, back.hidden_units, back.num_classes, back.activation, back.class_names) == (6, 4, 3, "sigmoid", ["a", "b", "c"])
    assert back.history == {"loss": [1.0, 0.5], "val_loss": [0.9]}
    with np.load(path) as z:
        assert int(z["hidden_units"]) == 4 and int(z["embedding_dim"]) == 6
        fields = {k: z[k] for k in z.files}
    # a linear head's file has none of the new entries and loads as before
    W, b = lp.init_head(6, 3, 1)
    lin = str(tmp_path / "lin.npz")
    lp.ProbeHead(W, b, "softmax", ["a", "b", "c"]).save(lin)
    with np.load(lin) as z:
        assert not {"W1", "b1", "hidden_units"} & set(z.files)
    got = lp.ProbeHead.load(lin)
    assert got.W1 is None and got.b1 is None and got.hidden_units == 0 and got.embedding_dim == 6 and np.array_equal(got.W, W)
    # refused: an embedding_dim that is not W1's, hidden_units that is not W1's, half a hidden layer, shapes that do not chain
    for change, match in (({"embedding_dim": np.int64(4)}, "embedding_dim"), ({"hidden_units": np.int64(5)}, "hidden_units")):
        bad = str(tmp_path / "bad.npz")
        np.savez(bad, **{**fields, **change})
        with pytest.raises(ValueError, match=match):
            lp.ProbeHead.load(bad)
    bad = str(tmp_path / "half.npz")
    np.savez(bad, **{k: v for k, v in fields.items() if k != "b1"})
    with pytest.raises(ValueError, match="together"):
        lp.ProbeHead.load(bad)
    with pytest.raises(ValueError, match="W1 must be"):
        lp.ProbeHead(head.W, head.b, "sigmoid", [], {}, head.W1[:, :3], head.b1[:3])
    with pytest.raises(ValueError, match="width 6"):
        head.check_embedding_dim(4)


# -- what is not built for a hidden layer says so ----------------------------------------------------------------------------------------
def test_library_refusals():
    from birdnet_stm32.conversion.head_export import export_head_tflite, quantize_head
    from birdnet_stm32.training.probe_qat import fit_probe_qat

    X, Y = _rows()
    head, lin = _mlp_head(), lp.ProbeHead(*lp.init_head(6, 3, 1))
    msg = "hidden layer"
    with pytest.raises(ValueError, match=msg):
        lp.fit_probe_sweep(None, X, Y, trials=[lp.ProbeTrial()], hidden_units=8)
    with pytest.raises(ValueError, match=msg):
        lp.fit_probe_augmented(None, X, Y, augment=None, input_shape=(1, 12), hidden_units=8)
    with pytest.raises(ValueError, match=msg):
        fit_probe_qat(None, X, Y, head=lin, logit_range=(-1.0, 1.0), hidden_units=8)
    with pytest.raises(ValueError, match=msg):
        fit_probe_qat(None, X, Y, head=head, logit_range=(-1.0, 1.0))
    with pytest.raises(ValueError, match=msg):
        quantize_head(head, 0.1, 0, -1.0, 1.0)
    with pytest.raises(ValueError, match=msg):
        quantize_head(lin, 0.1, 0, -1.0, 1.0, hidden_units=8)
    with pytest.raises(ValueError, match=msg):
        export_head_tflite(head, "no_such_model.tflite", np.zeros((2, 6), np.int8), "out.tflite")
    with pytest.raises(ValueError, match=msg):
        export_head_tflite(lin, "no_such_model.tflite", np.zeros((2, 6), np.int8), "out.tflite", hidden_units=8)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="hidden_units"):
            lp.fit_probe_reference(X, Y, hidden_units=bad)


CLI = ["--model_path", "no_such_model.tflite", "--data_path_train", "no_such_folder", "--output", "out", "--hidden_units", "16"]


@pytest.mark.parametrize("extra,flag", [(["--tune"], "--tune"), (["--export_tflite"], "--export_tflite"),
                                        (["--export_tflite", "--qat_epochs", "2"], "--export_tflite"), (["--qat_epochs", "2"], "--qat_epochs"),
                                        (["--mixup_probability", "0.25"], "--mixup_probability"), (["--spec_augment"], "--spec_augment")])
def test_command_line_refusals_come_before_any_file_is_read(extra, flag):
    """Neither the model nor the folder exists: the refusal is raised before either is looked for, by the command and by run_linear_probe."""
    from birdnet_stm32.cli import probe

    args = probe.build_parser().parse_args(CLI + extra)
    with pytest.raises(ValueError, match=f"--hidden_units does not combine with {flag}"):
        lp.hidden_from_args(args)
    with pytest.raises(ValueError, match="--hidden_units does not combine"):
        lp.run_linear_probe(args)
    with pytest.raises(SystemExit, match="--hidden_units does not combine"):
        probe.main(CLI + extra)


def test_parser_takes_hidden_units():
    from birdnet_stm32.cli import probe

    p = probe.build_parser()
    base = ["--model_path", "m.keras", "--data_path_train", "d", "--output", "o"]
    assert p.parse_args(base).hidden_units == 0
    assert p.parse_args(base + ["--hidden_units", "64"]).hidden_units == 64
    assert lp.hidden_from_args(p.parse_args(base)) == 0 and lp.hidden_from_args(p.parse_args(base + ["--hidden_units", "64"])) == 64
    assert lp.hidden_from_args(argparse.Namespace()) == 0   # (an older namespace)
    with pytest.raises(ValueError, match="hidden_units"):
        lp.hidden_from_args(p.parse_args(base + ["--hidden_units", "-3"]))
    with pytest.raises(ValueError, match="hidden_units"):
        lp.hidden_from_args(p.parse_args(base + ["--hidden_units", "4096"]))
