"""Host-side tests of the linear probe (no GPU): the numpy restatement learns, its optimiser arithmetic matches torch.optim, the dropout
hash, targets from folders, the split, ProbeHead files, argument parsing and dispatch."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import CONFIG_PATH, PKG, TFLITE_PATH

from birdnet_stm32.training import linear_probe as lp


def _clusters(n, D, C, seed):
    cent = np.random.default_rng(77).standard_normal((C, D))
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, C, n)
    X = np.maximum(cent[lab] + 1.5 * rng.standard_normal((n, D)), 0).astype(np.float32)
    return X, np.eye(C, dtype=np.float32)[lab], lab


def test_reference_fit_learns_a_separable_problem():
    X, Y, _ = _clusters(4096, 256, 12, 1)
    Xv, Yv, lv = _clusters(1024, 256, 12, 2)
    head = lp.fit_probe_reference(X, Y, Xv, Yv, epochs=4, batch_size=32, learning_rate=1e-3, dropout=0.5, clipnorm=1.0, dtype=np.float64)
    h = head.history
    assert len(h["loss"]) == 4 and len(h["val_loss"]) == 4 and h["step_loss"].shape == (4 * 128,)
    assert h["step_loss"][0] > 1.0 and h["loss"][-1] < 0.15 and h["val_loss"][-1] < h["val_loss"][0]
    P = lp.head_scores(Xv.astype(np.float64), h["W"], h["b"], "sigmoid")
    assert (P.argmax(axis=1) == lv).mean() > 0.98
    again = lp.fit_probe_reference(X, Y, Xv, Yv, epochs=4, batch_size=32, dtype=np.float64)
    assert np.array_equal(again.history["W"], h["W"])
    sm = lp.fit_probe_reference(X, Y, activation="softmax", epochs=2, batch_size=64, dtype=np.float64)
    assert sm.history["loss"][-1] < sm.history["loss"][0] and sm.history["val_loss"] == []


@pytest.mark.parametrize("optimizer", ["adam", "adamw", "sgd"])
def test_optimizer_arithmetic_against_torch(optimizer):
    """Constant learning rate, eps = 0 on both sides and nonzero gradients: there Keras' and torch's definitions coincide."""
    import torch

    rng = np.random.default_rng(4)
    w0 = rng.standard_normal((7, 5))
    grads = [rng.standard_normal((7, 5)) + 0.1 for _ in range(6)]
    lr, wd = 1e-2, 0.05
    t = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    opt = {"adam": lambda: torch.optim.Adam([t], lr=lr, eps=0.0), "adamw": lambda: torch.optim.AdamW([t], lr=lr, eps=0.0, weight_decay=wd),
           "sgd": lambda: torch.optim.SGD([t], lr=lr, momentum=0.9)}[optimizer]()
    w, state = w0.copy(), {"m": np.zeros_like(w0), "v": np.zeros_like(w0)}
    for i, g in enumerate(grads):
        t.grad = torch.tensor(g)
        opt.step()
        alpha = lr * np.sqrt(1 - lp.BETA_2 ** (i + 1)) / (1 - lp.BETA_1 ** (i + 1))
        w = lp.optimizer_step(w, g, state, optimizer, lr, alpha, wd, eps=0.0)
        assert np.allclose(w, t.detach().numpy(), rtol=1e-12, atol=1e-14), (optimizer, i)


def test_adam_epsilon_sits_on_the_uncorrected_sqrt_v():
    """Two steps by hand, Keras placement: w -= alpha_t m / (sqrt(v) + 1e-7) with alpha_t = lr sqrt(1 - b2^t) / (1 - b1^t).  A gradient of
    1e-7 makes the placement visible: sqrt(v_1) = 1e-7 sqrt(0.001) is far below eps."""
    g, lr = 1e-7, 0.1
    state = {"m": np.zeros(1), "v": np.zeros(1)}
    w = np.ones(1)
    m1, v1 = 0.1 * g, 0.001 * g * g
    a1 = lr * np.sqrt(1 - 0.999) / (1 - 0.9)
    want1 = 1.0 - a1 * m1 / (np.sqrt(v1) + 1e-7)
    assert lp.step_sizes(lr, 0, 10**9)[1] == pytest.approx(a1, rel=1e-7)   # (the learning rate is the float32 the C ABI takes)
    w = lp.optimizer_step(w, np.full(1, g), state, "adam", lr, a1)
    assert abs(w[0] - want1) < 1e-15
    m2, v2 = m1 + 0.1 * (g - m1), v1 + 0.001 * (g * g - v1)
    a2 = lr * np.sqrt(1 - 0.999**2) / (1 - 0.9**2)
    want2 = want1 - a2 * m2 / (np.sqrt(v2) + 1e-7)
    w = lp.optimizer_step(w, np.full(1, g), state, "adam", lr, a2)
    assert abs(w[0] - want2) < 1e-15
    # torch's placement (eps added to the corrected sqrt) would have moved by lr * g / (g + 1e-7) = lr / 2 in step one
    assert abs((1.0 - want1) - lr / 2) > 0.01


def test_step_sizes_follow_the_cosine_schedule():
    assert lp.step_sizes(1e-3, 0, 100)[0] == pytest.approx(1e-3, rel=1e-6)
    assert lp.step_sizes(1e-3, 50, 100)[0] == pytest.approx(5e-4, rel=1e-6)
    assert lp.step_sizes(1e-3, 100, 100)[0] == pytest.approx(0.0, abs=1e-12) and lp.step_sizes(1e-3, 150, 100)[0] == pytest.approx(0.0, abs=1e-12)
    lr_t, alpha = lp.step_sizes(1e-3, 0, 100)
    assert alpha == pytest.approx(lr_t * np.sqrt(0.001) / 0.1)


def test_clip_and_losses():
    g = np.array([[3.0, 4.0]])
    assert np.allclose(lp.clip_by_global_norm(g, 1.0), g / 5) and lp.clip_by_global_norm(g, 10.0) is g and lp.clip_by_global_norm(g, 0.0) is g
    P, Y = np.array([[0.5, 1.0], [0.25, 0.0]]), np.array([[1.0, 1.0], [0.0, 0.0]])
    want = -(np.log(0.5) + np.log(1 - 1e-7) + np.log(0.75) + np.log(1 - 1e-7)) / 4
    assert lp.probe_loss(P, Y, "sigmoid") == pytest.approx(want, rel=1e-12)
    assert lp.probe_loss(np.array([[0.2, 0.8]]), np.array([[0.0, 1.0]]), "softmax") == pytest.approx(-np.log(0.8))


def test_dropout_hash():
    a, b = lp.dropout_hash(42, 7, 64, 256), lp.dropout_hash(42, 7, 64, 256)
    assert a.dtype == np.uint32 and a.shape == (64, 256) and np.array_equal(a, b) and a.max() < 1 << 24
    assert np.array_equal(lp.dropout_hash(42, 7, 16, 100), a[:16, :100])           # stateless: a counter, not a stream
    for other in (lp.dropout_hash(43, 7, 64, 256), lp.dropout_hash(42, 8, 64, 256)):
        assert 0.45 < (other >= (1 << 23)).mean() < 0.55 and (other == a).mean() < 0.01
    # one value by hand
    def fmix(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)

    h = fmix(42 ^ ((7 * 0x9E3779B1) & 0xFFFFFFFF))
    h = fmix(h ^ ((5 * 0x85EBCA77) & 0xFFFFFFFF))
    h = fmix(h ^ ((9 * 0xC2B2AE3D) & 0xFFFFFFFF))
    assert int(a[5, 9]) == h >> 8
    n = 512 * 256
    for p in (0.1, 0.5, 0.9):
        m = lp.dropout_mask(1, 3, 512, 256, p)
        kept = int((m > 0).sum())
        assert abs(kept - n * (1 - p)) < 5 * np.sqrt(n * p * (1 - p))               # 5 sigma of the binomial
        assert np.allclose(m[m > 0], 1 / (1 - p), rtol=1e-6)
    assert np.array_equal(lp.dropout_mask(1, 3, 8, 8, 0.0), np.ones((8, 8), np.float32)) and lp.dropout_threshold(0.0) == 0


def test_targets_split_and_head_files(tmp_path):
    paths = ["/d/owl/a.wav", "/d/noise/n.wav", "/d/wren/b.wav", "/d/owl/c.wav", "/d/other/o.wav"]
    classes = ["owl", "wren"]
    file_index = np.array([0, 0, 1, 2, 3, 3, 4])
    Y, keep = lp.targets_from_paths(paths, classes, file_index, "sigmoid")
    assert Y.tolist() == [[1, 0], [1, 0], [0, 0], [0, 1], [1, 0], [1, 0], [0, 0]] and keep.all()
    Y2, keep2 = lp.targets_from_paths(paths, classes, file_index, "softmax")
    assert np.array_equal(Y, Y2) and keep2.tolist() == [True, True, False, True, True, True, False]
    tr, va = lp.split_train_val(list("abcdefghij"), 0.2)
    assert tr == list("abcdefgh") and va == list("ij")
    assert lp.split_train_val(list("abc"), 0.0) == (list("abc"), [])

    rng = np.random.default_rng(0)
    head = lp.ProbeHead(rng.standard_normal((16, 2)), rng.standard_normal(2), "softmax", classes, {"loss": [1.0, 0.5], "val_loss": [0.9, 0.6], "step_loss": np.ones(3)})
    p = str(tmp_path / "h.npz")
    head.save(p)
    with np.load(p) as z:   # numpy alone reads it
        assert z["W"].dtype == np.float32 and z["W"].shape == (16, 2) and str(z["activation"]) == "softmax" and list(z["class_names"]) == classes
    back = lp.ProbeHead.load(p)
    assert np.array_equal(back.W, head.W) and np.array_equal(back.b, head.b) and back.activation == "softmax" and back.class_names == classes
    assert back.embedding_dim == 16 and back.num_classes == 2 and back.history["val_loss"] == [0.9, 0.6]
    with pytest.raises(ValueError, match="width 16"):
        back.check_embedding_dim(256)
    with pytest.raises(ValueError):
        lp.ProbeHead(np.zeros((4, 2)), np.zeros(3))
    with pytest.raises(ValueError):
        lp.ProbeHead(np.zeros((4, 2)), np.zeros(2), "relu")
    assert lp.probe_output_paths("x/y.npz") == lp.probe_output_paths("x/y") and lp.probe_output_paths("x/y")["config"] == "x/y_model_config.json"
    lp.write_history_csv(str(tmp_path / "h.csv"), {"loss": [1.0, 0.5], "val_loss": [0.9]})
    assert open(tmp_path / "h.csv").read().splitlines() == ["epoch,loss,val_loss", "1,1,0.9", "2,0.5,"]


def test_detect_files_refuses_a_head_of_another_width_before_reading_audio():
    from birdnet_stm32.evaluation.detections import detect_files

    class Runner:
        num_classes = 100

        def embedding_info(self):
            return {"dim": 256, "dtype": "float32", "scale": 1.0, "zero_point": 0}

    with pytest.raises(ValueError, match="width 128"):
        detect_files(Runner(), ["/nonexistent/a.wav"], head=lp.ProbeHead(np.zeros((128, 3)), np.zeros(3)))


def test_fit_args_are_checked():
    X, Y = np.zeros((8, 4), np.float32), np.zeros((8, 2), np.float32)
    for kw in (dict(activation="relu"), dict(optimizer="lamb"), dict(dropout=1.0), dict(batch_size=0), dict(epochs=0)):
        with pytest.raises(ValueError):
            lp.fit_probe_reference(X, Y, **kw)
    with pytest.raises(ValueError):
        lp.fit_probe_reference(X, Y[:7])


def test_probe_and_analyze_argument_parsing():
    from birdnet_stm32.cli import analyze, probe

    a = probe.build_parser().parse_args(["--model_path", "m.tflite", "--data_path_train", "d", "--output", "o"])
    assert (a.epochs, a.batch_size, a.learning_rate, a.optimizer, a.weight_decay, a.grad_clip, a.dropout, a.val_split, a.seed, a.activation, a.overlap) == \
        (50, 32, 1e-3, "adam", 0.0, 1.0, 0.5, 0.2, 42, "sigmoid", 0.0)
    a = probe.build_parser().parse_args(["--model_path", "m", "--data_path_train", "d", "--output", "o", "--optimizer", "adamw", "--weight_decay", "0.01",
                                         "--activation", "softmax", "--max_duration", "10", "--grad_clip", "0"])
    assert a.optimizer == "adamw" and a.weight_decay == 0.01 and a.activation == "softmax" and a.max_duration == 10 and a.grad_clip == 0
    with pytest.raises(SystemExit):
        probe.build_parser().parse_args(["--model_path", "m", "--data_path_train", "d", "--output", "o", "--optimizer", "lamb"])
    with pytest.raises(SystemExit, match="Pretrained model not found"):
        probe.main(["--model_path", "/nonexistent/m.tflite", "--data_path_train", "d", "--output", "o"])
    b = analyze.build_parser().parse_args(["--model_path", "m", "--input", "x.wav", "--output", "o.csv", "--head", "h.npz"])
    assert b.head == "h.npz" and analyze.build_parser().parse_args(["--model_path", "m", "--input", "x", "--output", "o"]).head == ""
    with pytest.raises(SystemExit, match="head not found"):
        analyze.main(["--model_path", TFLITE_PATH, "--model_config", CONFIG_PATH, "--input", "x.wav", "--output", "o.csv", "--head", "/nonexistent/h.npz"])


def test_main_dispatches_probe():
    import birdnet_stm32.__main__ as m

    assert "probe" in m.USAGE and "embed" in m.USAGE and "analyze" in m.USAGE
    env = dict(os.environ, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, "-m", "birdnet_stm32", "probe", "--help"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "--data_path_train" in r.stdout and "--grad_clip" in r.stdout
    r = subprocess.run([sys.executable, "-m", "birdnet_stm32", "train"], capture_output=True, text=True, env=env)
    assert r.returncode == 2 and "reference package" in r.stdout


def test_probe_config_is_the_base_config_with_the_new_classes(tmp_path):
    from dataclasses import replace

    from birdnet_stm32.training.config import ModelConfig

    cfg = ModelConfig.load(CONFIG_PATH)
    new = replace(cfg, num_classes=2, class_names=["a", "b"], dropout_rate=0.3)
    new.save(tmp_path / "c.json")
    d = json.load(open(tmp_path / "c.json"))
    assert d["num_classes"] == 2 and d["class_names"] == ["a", "b"] and d["dropout_rate"] == 0.3 and d["sample_rate"] == cfg.sample_rate
