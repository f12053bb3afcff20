"""CPU tests of the probe's hyperparameter sweep: the trials ``sample_trials`` draws, label smoothing in the numpy restatement, ``ProbeTrial``
validation and what ``probe --tune`` refuses before it loads anything."""

import numpy as np
import pytest

from birdnet_stm32.training import linear_probe as lp
from birdnet_stm32.training import tune


def test_sample_trials_are_deterministic_in_range_and_start_with_the_base():
    base = lp.ProbeTrial(learning_rate=2e-3, optimizer="sgd", clipnorm=0.5, dropout=0.1, label_smoothing=0.3)
    a, b = tune.sample_trials(64, 7, base), tune.sample_trials(64, 7, base)
    assert a == b and len(a) == 64 and a[0] is base
    assert tune.sample_trials(20, 7, base) == a[:20]                # a longer search extends a shorter one
    assert tune.sample_trials(64, 8, base)[1:] != a[1:]
    seen = {k: set() for k in ("dropout", "label_smoothing", "optimizer", "clipnorm")}
    for t in a[1:]:
        assert 1e-4 <= t.learning_rate <= 1e-2
        assert t.dropout in tune.DROPOUT_CHOICES and t.label_smoothing in tune.LABEL_SMOOTHING_CHOICES
        assert t.optimizer in ("adam", "adamw") and t.clipnorm in tune.GRAD_CLIP_CHOICES
        assert (1e-5 <= t.weight_decay <= 1e-2) if t.optimizer == "adamw" else t.weight_decay == 0.0
        for k in seen:
            seen[k].add(getattr(t, k))
    assert seen["dropout"] == set(tune.DROPOUT_CHOICES) and seen["label_smoothing"] == set(tune.LABEL_SMOOTHING_CHOICES)
    assert seen["optimizer"] == {"adam", "adamw"} and seen["clipnorm"] == set(tune.GRAD_CLIP_CHOICES)
    assert tune.sample_trials(1, 7, base) == [base]
    for n in (0, 65):
        with pytest.raises(ValueError, match="n_trials"):
            tune.sample_trials(n, 7, base)


def _rows(n=70, D=9, C=4):
    rng = np.random.default_rng(3)
    return rng.random((n, D)).astype(np.float32), np.eye(C, dtype=np.float32)[rng.integers(0, C, n)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
def test_reference_without_smoothing_is_unchanged_to_the_bit(activation, dtype):
    X, Y = _rows()
    kw = dict(activation=activation, epochs=3, batch_size=16, dtype=dtype, seed=4)
    a = lp.fit_probe_reference(X, Y, X[:20], Y[:20], **kw)
    b = lp.fit_probe_reference(X, Y, X[:20], Y[:20], label_smoothing=0.0, **kw)
    c = lp.fit_probe_reference(X, Y, X[:20], Y[:20], label_smoothing=0.1, **kw)
    assert np.array_equal(a.history["W"], b.history["W"]) and np.array_equal(a.history["b"], b.history["b"])
    assert np.array_equal(a.history["step_loss"], b.history["step_loss"]) and a.history["val_loss"] == b.history["val_loss"]
    assert not np.array_equal(a.history["W"], c.history["W"])
    sweep = lp.fit_probe_sweep_reference(X, Y, X[:20], Y[:20], [lp.ProbeTrial(), lp.ProbeTrial(label_smoothing=0.1)], **kw)
    assert np.array_equal(sweep.heads[0].history["W"], a.history["W"]) and np.array_equal(sweep.heads[1].history["W"], c.history["W"])
    best = [min(h.history["val_loss"]) for h in sweep.heads]
    assert sweep.best == int(np.argmin(best))


def test_smoothed_targets_and_loss_by_hand():
    """Y = [[1, 0, 0], [0, 1, 1]], eps = 0.1.  Sigmoid: 1 -> 0.95, 0 -> 0.05.  Softmax (C = 3): 1 -> 0.9 + 1/30, 0 -> 1/30.  With every
    probability 0.5 the binary cross-entropy is ln 2 whatever the targets; with uniform softmax probabilities the categorical one is
    ln 3 * (sum of the row's targets): row 0 sums to 1, row 1 to 0.9 * 2 + 0.1 = 1.9, the mean is 1.45 ln 3."""
    Y = np.array([[1, 0, 0], [0, 1, 1]], np.float64)
    s = lp.smooth_targets(Y, 0.1, "sigmoid")
    e = float(np.float32(0.1))
    assert np.allclose(s, [[0.95, 0.05, 0.05], [0.05, 0.95, 0.95]], atol=1e-8, rtol=0)
    assert np.array_equal(s, Y * (1.0 - e) + 0.5 * e)
    m = lp.smooth_targets(Y, 0.1, "softmax")
    assert np.allclose(m, [[0.9 + 1 / 30, 1 / 30, 1 / 30], [1 / 30, 0.9 + 1 / 30, 0.9 + 1 / 30]], atol=1e-8, rtol=0)
    assert abs(float(lp.probe_loss(np.full((2, 3), 0.5), s, "sigmoid")) - np.log(2)) < 1e-12
    assert abs(float(lp.probe_loss(np.full((2, 3), 1 / 3), m, "softmax")) - 1.45 * np.log(3)) < 1e-7
    # a non-trivial P: the sigmoid loss by hand
    P = np.array([[0.8, 0.3, 0.1], [0.2, 0.6, 0.9]])
    want = -np.mean(s * np.log(P) + (1 - s) * np.log(1 - P))
    assert abs(float(lp.probe_loss(P, s, "sigmoid")) - want) < 1e-15
    # float32: each operation rounded in float32, no fused multiply-add
    Y32 = Y.astype(np.float32)
    keep, add = np.float32(1) - np.float32(0.1), np.float32(0.5) * np.float32(0.1)
    assert np.array_equal(lp.smooth_targets(Y32, 0.1, "sigmoid"), (Y32 * keep).astype(np.float32) + add)
    assert lp.smooth_targets(Y32, 0.1, "softmax").dtype == np.float32
    assert np.array_equal(lp.smooth_targets(Y32, 0.1, "softmax")[0, 1:], np.full(2, np.float32(0.1) / np.float32(3)))


def test_device_step_sizes_restate_step_sizes():
    got = lp.device_step_sizes([1e-3, 2e-2], 7, 5, 40)
    assert got.shape == (5, 2, 2) and got.dtype == np.float32
    for i in range(5):
        for j, lr in enumerate((1e-3, 2e-2)):
            want = np.array(lp.step_sizes(lr, 7 + i, 40))
            assert np.all(np.abs(got[i, j] - want) <= 2.0 ** -23 * want)


def test_probe_trial_validation():
    lp.ProbeTrial()
    for kw, match in ((dict(optimizer="rmsprop"), "optimizer"), (dict(dropout=1.0), "dropout"), (dict(dropout=-0.1), "dropout"),
                      (dict(label_smoothing=1.0), "label_smoothing"), (dict(label_smoothing=-0.01), "label_smoothing"),
                      (dict(learning_rate=-1.0), "learning_rate"), (dict(weight_decay=float("nan")), "weight_decay")):
        with pytest.raises(ValueError, match=match):
            lp.ProbeTrial(**kw)
    X, Y = _rows()
    with pytest.raises(ValueError, match="label_smoothing"):
        lp.fit_probe_reference(X, Y, label_smoothing=1.0)
    with pytest.raises(ValueError, match="ProbeTrial"):
        lp.fit_probe_sweep_reference(X, Y, trials=[])
    with pytest.raises(ValueError, match="ProbeTrial"):
        lp.fit_probe_sweep_reference(X, Y, trials=[dict(dropout=0.5)])


@pytest.mark.parametrize("flags,match", [
    (["--tune", "--val_split", "0"], "val_split"),
    (["--tune", "--mixup_probability", "0.25"], "mixup"),
    (["--tune", "--spec_augment"], "spec_augment"),
    (["--tune", "--n_trials", "0"], "n_trials"),
    (["--tune", "--n_trials", "65"], "n_trials"),
    (["--label_smoothing", "1.0"], "label_smoothing"),
])
def test_probe_cli_refuses_before_loading_anything(tmp_path, flags, match):
    """The model path does not exist: a refusal that names the flag came before the model was looked for."""
    from birdnet_stm32.cli import probe as probe_cli

    with pytest.raises(SystemExit, match=match):
        probe_cli.main(["--model_path", str(tmp_path / "missing.tflite"), "--data_path_train", str(tmp_path), "--output", str(tmp_path / "head"), *flags])


def test_probe_cli_defaults():
    from birdnet_stm32.cli import probe as probe_cli

    args = probe_cli.build_parser().parse_args(["--model_path", "m", "--data_path_train", "d", "--output", "o"])
    assert args.label_smoothing == 0.0 and args.tune is False and args.n_trials == 20 and args.tune_seed is None
    assert "0.1" in " ".join(probe_cli.build_parser().format_help().split("--label_smoothing")[2][:400].split())   # the reference's default


def test_macro_roc_auc_by_hand():
    """Class 0: scores rank its positive first, AUC 1.  Class 1: the positive is ranked second of three, AUC 0.5.  Class 2 has no
    positive and is left out.  The mean is 0.75."""
    y = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]], np.float32)
    s = np.array([[0.9, 0.8, 0.1], [0.2, 0.5, 0.7], [0.1, 0.3, 0.2]], np.float32)
    assert tune.macro_roc_auc(y, s) == pytest.approx(0.75)
    assert np.isnan(tune.macro_roc_auc(np.zeros((3, 2), np.float32), s[:, :2]))
