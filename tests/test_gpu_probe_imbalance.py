"""GPU tests of the probe's tools for long-tailed training sets: the focal loss, row weights and ``rows`` in the forward kernel's epilogue
(csrc/bn_probe_step.h, EXT = 1) against the numpy restatement, in the single fit, the sweep and the augmented fit; the new ABI calls'
refusals; and ``probe --loss focal --class_weights balanced --upsample_ratio`` end to end.

The yardstick is tests/test_gpu_probe.py's: d32 = the distance of the float32 restatement from the float64 one, measured in the same
test; the device (float32 too, another summation order) must be within 8 d32 of float64."""

import ctypes
import json
import os
import wave

import numpy as np
import pytest

from conftest import CONFIG_PATH, TFLITE_PATH, synth_chunks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


@pytest.fixture(scope="module")
def ctx(torch_mod):
    from birdnet_stm32 import _hip

    c = _hip.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def runner(torch_mod):
    from birdnet_stm32.models.runners import load_model_runner

    r = load_model_runner(TFLITE_PATH, max_batch=64, prepare_pipeline=True)
    yield r
    r.close()


def _clusters(n, D, C, seed, multi_hot=False):
    """Rectified Gaussian clusters (the recipe of tests/test_gpu_probe.py), with class sizes that fall off: class c is drawn (c + 1)^-1.5 often."""
    cent = np.random.default_rng(1000 + D + C).standard_normal((C, D))
    rng = np.random.default_rng(seed)
    p = (np.arange(C) + 1.0) ** -1.5
    lab = rng.choice(C, n, p=p / p.sum())
    X = np.maximum(cent[lab] + 1.5 * rng.standard_normal((n, D)), 0).astype(np.float32)
    Y = np.eye(C, dtype=np.float32)[lab]
    if multi_hot:
        Y[::7] = 0.0                                           # "noise" rows
        Y[np.arange(3, n, 11), rng.integers(0, C, len(range(3, n, 11)))] = 1.0   # a second label
    return X, Y, lab


def _balanced(Y):
    """Row weights from balanced class weights, one file per row: total / (C * count), an empty class counting as 1."""
    from birdnet_stm32.training.linear_probe import row_weights

    pos = Y.max(axis=1) > 0
    count = np.bincount(np.argmax(Y[pos], axis=1), minlength=Y.shape[1])
    return row_weights(Y, pos.sum() / (Y.shape[1] * np.maximum(count, 1.0)))


def _upsampled(Y, seed, factor=1.5):
    """Row numbers with repeats, about ``factor`` times the rows: every row once and draws from the rows of the rarer half of the classes."""
    rng = np.random.default_rng(seed)
    rare = np.flatnonzero((np.argmax(Y, axis=1) >= Y.shape[1] // 2) & (Y.max(axis=1) > 0))
    return np.sort(np.concatenate([np.arange(len(Y)), rng.choice(rare, int((factor - 1) * len(Y)))])).astype(np.int32)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


def _params(head, key=None):
    W, b = (head.history["W"], head.history["b"]) if key else (head.W, head.b)
    return np.concatenate([W, b[None, :]]).astype(np.float64)


def _yardstick(what, dev, r32, r64, val=True):
    """Prints and returns the ratios device-to-float64 over float32-restatement-to-float64: weights, step losses, validation losses."""
    out = {}
    for name, d, a, b in [("weights", _params(dev), _params(r32, 1), _params(r64, 1)),
                          ("step losses", dev.history["step_loss"], r32.history["step_loss"], r64.history["step_loss"])] + \
                         ([("val losses", dev.history["val_loss"], r32.history["val_loss"], r64.history["val_loss"])] if val else []):
        d32, dd = _rel(a, b), _rel(d, b)
        out[name] = (dd, d32)
    print(f"{what}: " + "; ".join(f"{k} d32 {d32:.3e} device {dd:.3e} (ratio {dd / d32:.2f})" for k, (dd, d32) in out.items()))
    return out


N, D, C = 1027, 96, 13   # batch 32: a short last batch of 3 rows; C: a partial column tile; D: a partial tile of the gradient kernel

MANY = {
    "focal2":          dict(loss="focal", focal_gamma=2.0),
    "focal.5-multihot": dict(loss="focal", focal_gamma=0.5, multi_hot=True),
    "weights":         dict(weights=True),
    "all-three":       dict(loss="focal", focal_gamma=2.0, weights=True, rows=True),
    "batch96":         dict(loss="focal", focal_gamma=2.0, weights=True, rows=True, batch=96),   # several row groups: the reduce kernel runs
    "softmax-weights": dict(activation="softmax", weights=True),
}


@pytest.mark.parametrize("case", list(MANY))
def test_many_steps_track_the_float64_restatement(torch_mod, ctx, case):
    """3 epochs over 1027 rows (or about 1.5 x as many row numbers), dropout 0.5, clip 1, Adam, with validation rows."""
    from birdnet_stm32.training.linear_probe import fit_probe, fit_probe_reference

    cfg = dict(MANY[case])
    X, Y, _ = _clusters(N, D, C, seed=3, multi_hot=cfg.pop("multi_hot", False))
    Xv, Yv, _ = _clusters(200, D, C, seed=4)
    w = _balanced(Y) if cfg.pop("weights", False) else None
    rows = _upsampled(Y, seed=5) if cfg.pop("rows", False) else None
    kw = dict(epochs=3, batch_size=cfg.pop("batch", 32), learning_rate=1e-3, optimizer="adam", clipnorm=1.0, dropout=0.5, seed=42, sample_weight=w, rows=rows, **cfg)
    r64 = fit_probe_reference(X, Y, Xv, Yv, dtype=np.float64, **kw)
    r32 = fit_probe_reference(X, Y, Xv, Yv, dtype=np.float32, **kw)
    dev = fit_probe(ctx, X, Y, Xv, Yv, **kw)
    m = N if rows is None else len(rows)
    assert len(dev.history["step_loss"]) == 3 * -(-m // kw["batch_size"]) and (rows is None or (m > 1.45 * N and len(np.unique(rows)) == N))
    assert w is None or (w.max() > 3 * w.min())
    assert dev.history["best_epoch"] == r64.history["best_epoch"] and dev.history["loss"][-1] < dev.history["loss"][0]
    plain = fit_probe(ctx, X, Y, Xv, Yv, **{**kw, "loss": "auto", "sample_weight": None, "rows": None})
    assert not np.array_equal(plain.W, dev.W)                  # the arguments did something
    for name, (dd, d32) in _yardstick(case, dev, r32, r64).items():
        assert dd <= 8 * d32, name


@pytest.mark.parametrize("D,C,B", [(96, 7, 5), (255, 13, 33), (32, 2050, 40)])
def test_one_sgd_step_is_the_focal_weighted_gradient(torch_mod, ctx, D, C, B):
    """One SGD step with lr = 1 (momentum starts at zero), no dropout, no clip: W0 - W1 is the gradient, Xa^T probe_loss_gradient in
    float64, focal (gamma 2) and weights on.  C = 2050 is just over one pass of columns: the second pass's epilogue runs."""
    from birdnet_stm32.training.linear_probe import fit_probe, fit_probe_reference, head_scores, init_head, probe_loss, probe_loss_gradient

    X, Y, _ = _clusters(B, D, C, seed=5, multi_hot=True)
    X *= 0.25
    w = np.random.default_rng(6).uniform(0.3, 5.0, B).astype(np.float32)
    kw = dict(epochs=1, batch_size=B, learning_rate=1.0, optimizer="sgd", clipnorm=0.0, dropout=0.0, seed=9, loss="focal", focal_gamma=2.0, sample_weight=w)
    head = fit_probe(ctx, X, Y, **kw)
    r32 = fit_probe_reference(X, Y, dtype=np.float32, **kw)
    W0, b0 = init_head(D, C, 9)
    P0 = np.concatenate([W0, b0[None, :]]).astype(np.float64)
    P = head_scores(X.astype(np.float64), W0.astype(np.float64), b0.astype(np.float64), "sigmoid")
    lkw = dict(loss="focal", focal_gamma=2.0, sample_weight=w.astype(np.float64))
    want = np.concatenate([X.astype(np.float64), np.ones((B, 1))], axis=1).T @ probe_loss_gradient(P, Y.astype(np.float64), "sigmoid", **lkw)
    dd, d32 = _rel(P0 - _params(head), want), _rel(P0 - _params(r32, 1), want)
    loss64 = float(probe_loss(P, Y.astype(np.float64), "sigmoid", **lkw))
    print(f"D={D} C={C} B={B}: gradient d32 {d32:.3e} device {dd:.3e} (ratio {dd / d32:.2f}); loss {head.history['step_loss'][0]:.7f} vs {loss64:.7f}")
    assert dd <= 8 * d32
    assert abs(head.history["step_loss"][0] - loss64) <= 1e-5 * max(1.0, abs(loss64))   # (the bound of tests/test_gpu_probe.py's one-step test)


def test_validation_loss_is_the_focal_unweighted_one(torch_mod, ctx):
    from birdnet_stm32.training.linear_probe import fit_probe, fit_probe_reference, head_scores, probe_loss

    X, Y, _ = _clusters(300, D, C, seed=3)
    Xv, Yv, _ = _clusters(203, D, C, seed=4, multi_hot=True)
    kw = dict(epochs=3, batch_size=32, learning_rate=1e-2, dropout=0.2, seed=1, loss="focal", focal_gamma=2.0, sample_weight=_balanced(Y))
    dev = fit_probe(ctx, X, Y, Xv, Yv, **kw)
    r64, r32 = (fit_probe_reference(X, Y, Xv, Yv, dtype=dt, **kw) for dt in (np.float64, np.float32))
    dd, d32 = _yardstick("validation", dev, r32, r64)["val losses"]
    assert dd <= 8 * d32
    # ... and it is the focal loss of the returned weights, not the cross-entropy and not weighted: to the float32 of one evaluation
    P = head_scores(Xv.astype(np.float64), dev.W.astype(np.float64), dev.b.astype(np.float64), "sigmoid")
    best = dev.history["best_epoch"]
    focal, ce = float(probe_loss(P, Yv.astype(np.float64), "sigmoid", loss="focal", focal_gamma=2.0)), float(probe_loss(P, Yv.astype(np.float64), "sigmoid"))
    assert abs(dev.history["val_loss"][best] - focal) <= 1e-5 * max(1.0, focal) and abs(focal - ce) > 0.1 * focal   # (the one-step tests' loss bound)


def _assert_same_head(a, b, what):
    assert np.array_equal(a.W, b.W) and np.array_equal(a.b, b.b), f"{what}: weights differ, max {np.abs(a.W - b.W).max():.3e}"
    assert np.array_equal(a.history["step_loss"], b.history["step_loss"]), f"{what}: step losses differ"
    assert a.history["val_loss"] == b.history["val_loss"], f"{what}: validation losses differ"


@pytest.mark.parametrize("batch", [32, 96])
def test_sweep_trials_with_focal_weights_and_rows(torch_mod, ctx, batch):
    """Three trials, one of them smoothed: the un-smoothed ones have the bits of fit_probe with the same arguments, the smoothed one (the
    focal loss sees the smoothed target) meets the yardstick against the restatement."""
    from birdnet_stm32.training.linear_probe import ProbeTrial, fit_probe, fit_probe_reference, fit_probe_sweep

    X, Y, _ = _clusters(301, D, C, seed=8, multi_hot=True)
    Xv, Yv, _ = _clusters(100, D, C, seed=9)
    trials = [ProbeTrial(learning_rate=1e-3, optimizer="adam", dropout=0.5, clipnorm=1.0),
              ProbeTrial(learning_rate=3e-3, optimizer="adam", dropout=0.3, clipnorm=1.0, label_smoothing=0.1),
              ProbeTrial(learning_rate=1e-2, optimizer="sgd", dropout=0.0, clipnorm=2.0)]
    kw = dict(epochs=2, batch_size=batch, seed=11, loss="focal", focal_gamma=2.0, sample_weight=_balanced(Y), rows=_upsampled(Y, seed=2))
    sweep = fit_probe_sweep(ctx, X, Y, Xv, Yv, trials, **kw)
    for t in (0, 2):
        kwt = trials[t].fit_kwargs()
        assert kwt.pop("label_smoothing") == 0.0
        _assert_same_head(sweep.heads[t], fit_probe(ctx, X, Y, Xv, Yv, **kw, **kwt), f"trial {t}")   # label_smoothing absent: the single-fit kernels
    r64, r32 = (fit_probe_reference(X, Y, Xv, Yv, dtype=dt, **kw, **trials[1].fit_kwargs()) for dt in (np.float64, np.float32))
    for name, (dd, d32) in _yardstick(f"smoothed trial, batch {batch}", sweep.heads[1], r32, r64).items():
        assert dd <= 8 * d32, name
    _assert_same_head(sweep.heads[1], fit_probe(ctx, X, Y, Xv, Yv, **kw, **trials[1].fit_kwargs()), "fit_probe(label_smoothing) is the sweep of one")


def test_same_call_same_bits_and_the_defaults_are_the_call_without(torch_mod, ctx):
    from birdnet_stm32.training.linear_probe import fit_probe

    X, Y, _ = _clusters(500, D, C, seed=8)
    Xv, Yv, _ = _clusters(100, D, C, seed=9)
    base = dict(epochs=2, batch_size=96, optimizer="adamw", weight_decay=1e-3, seed=11)
    kw = dict(base, loss="focal", focal_gamma=1.5, sample_weight=_balanced(Y), rows=_upsampled(Y, seed=2))
    _assert_same_head(fit_probe(ctx, X, Y, Xv, Yv, **kw), fit_probe(ctx, X, Y, Xv, Yv, **kw), "twice")
    _assert_same_head(fit_probe(ctx, X, Y, Xv, Yv, **base), fit_probe(ctx, X, Y, Xv, Yv, loss="auto", focal_gamma=2.0, sample_weight=None, rows=None, **base), "defaults")
    ident = fit_probe(ctx, X, Y, Xv, Yv, rows=np.arange(500), **base)   # the same row numbers per epoch through the same kernels
    _assert_same_head(fit_probe(ctx, X, Y, Xv, Yv, **base), ident, "identity rows")


def test_augmented_fit_with_weights_and_rows(torch_mod, runner):
    """40 synthetic chunks through the shipped INT8 model (tests/test_gpu_augment.py's shapes: 3 epochs of batch 8): the identity
    augmentation with weights and rows is fit_probe with them, bit for bit; with mixup and SpecAugment on, the device fit tracks
    fit_probe_augmented_reference over the same backbone on the yardstick (the device augmentation has the restatement's bits)."""
    torch = torch_mod
    from birdnet_stm32.training.augment import ProbeAugmentation
    from birdnet_stm32.training.linear_probe import fit_probe, fit_probe_augmented, fit_probe_augmented_reference

    audio = torch.from_numpy(synth_chunks(40, seed=5)).cuda()
    inputs = runner.model_inputs_device(audio).contiguous()

    def embed(x):
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        return runner.predict_device(t.contiguous(), return_embeddings=True)[1].clone().cpu().numpy()

    emb = embed(inputs)
    rng = np.random.default_rng(0)
    Y = np.eye(3, dtype=np.float32)[rng.choice(3, 40, p=[0.7, 0.2, 0.1])]
    Y[::9] = 0.0
    tr, va = slice(0, 32), slice(32, 40)
    w, rows = _balanced(Y[tr]), np.sort(np.concatenate([np.arange(32), rng.integers(0, 32, 15)])).astype(np.int32)   # 47 row numbers: a last batch of 7
    kw = dict(epochs=3, batch_size=8, learning_rate=0.01, seed=7, loss="focal", focal_gamma=2.0, sample_weight=w, rows=rows)
    ident = ProbeAugmentation(mixup_probability=0.0, spec_augment=True, freq_mask_max=1, time_mask_max=1)
    plain = fit_probe(runner, emb[tr], Y[tr], emb[va], Y[va], **kw)
    aug = fit_probe_augmented(runner, inputs[tr].contiguous(), Y[tr], emb[va], Y[va], augment=ident, input_shape=runner.input_shape(), **kw)
    _assert_same_head(plain, aug, "identity augmentation")
    assert len(aug.history["step_loss"]) == 3 * 6

    on = ProbeAugmentation(mixup_alpha=0.2, mixup_probability=0.25, spec_augment=True)
    akw = dict(kw, augment=on, input_shape=runner.input_shape())
    dev = fit_probe_augmented(runner, inputs[tr].contiguous(), Y[tr], emb[va], Y[va], **akw)
    x_host = inputs[tr].cpu().numpy()
    r64, r32 = (fit_probe_augmented_reference(embed, x_host, Y[tr], emb[va], Y[va], dtype=dt, **akw) for dt in (np.float64, np.float32))
    assert not np.array_equal(dev.W, plain.W)
    for name, (dd, d32) in _yardstick("augmented", dev, r32, r64).items():
        assert dd <= 8 * d32, name


def test_new_abi_calls_refuse_bad_arguments(torch_mod, ctx):
    torch = torch_mod
    from birdnet_stm32 import _hip

    lib = ctx.lib
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    X, Y = torch.rand((64, 32), device="cuda"), torch.zeros((64, 5), device="cuda")
    Y[torch.arange(64), torch.arange(64) % 5] = 1.0
    W, b = torch.zeros((32, 5), device="cuda"), torch.zeros(5, device="cuda")
    rw = torch.linspace(0.5, 3.0, 64, device="cuda")
    perm = (torch.arange(80, dtype=torch.int32, device="cuda") * 7) % 64     # 80 row numbers into 64 rows: repeats
    loss = torch.full((8,), float("nan"), device="cuda")
    ERR = -1   # BN_ERR_ARG

    def err():
        return lib.bn_last_error().decode()

    ptr = lambda t: t.data_ptr()   # noqa: E731
    h, hs = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.bn_probe_create(ctx.handle, 32, 5, 0, 0, 1e-3, 0.0, 1.0, 0.5, 1, 10, ptr(W), ptr(b), ctypes.byref(h), stream) == 0
    assert lib.bn_probe_create(ctx.handle, 32, 5, 1, 0, 1e-3, 0.0, 1.0, 0.5, 1, 10, ptr(W), ptr(b), ctypes.byref(hs), stream) == 0
    trials = (_hip.ProbeTrialStruct * 2)(_hip.ProbeTrialStruct(0, 1e-3, 0.0, 1.0, 0.5, 0.0), _hip.ProbeTrialStruct(0, 1e-3, 0.0, 1.0, 0.5, 0.1))
    sw, sws = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.bn_probe_sweep_create(ctx.handle, 32, 5, 0, 2, trials, 1, 10, ptr(W), ptr(b), ctypes.byref(sw), stream) == 0
    assert lib.bn_probe_sweep_create(ctx.handle, 32, 5, 1, 2, trials, 1, 10, ptr(W), ptr(b), ctypes.byref(sws), stream) == 0
    sizes = torch.full((5, 2, 2), 1e-3, device="cuda")
    sloss = torch.full((5, 2), float("nan"), device="cuda")
    try:
        for set_loss, good, soft, what in ((lib.bn_probe_set_loss, h, hs, "probe"), (lib.bn_probe_sweep_set_loss, sw, sws, "sweep")):
            assert set_loss(None, _hip.PROBE_LOSSES["focal"], 2.0) == ERR and "null" in err(), what
            assert set_loss(soft, 1, 2.0) == ERR and "softmax" in err(), what
            assert set_loss(good, 2, 2.0) == ERR and "loss" in err(), what
            for gamma in (-0.5, float("nan"), float("inf")):
                assert set_loss(good, 1, gamma) == ERR and "focal_gamma" in err(), (what, gamma)
            assert set_loss(soft, 0, 0.0) == 0 and set_loss(good, 1, 2.0) == 0, what
        assert lib.bn_probe_epoch_weighted(None, ptr(X), ptr(Y), ptr(rw), ptr(perm), 80, 16, ptr(loss), stream) == ERR
        assert lib.bn_probe_epoch_weighted(h, None, ptr(Y), ptr(rw), ptr(perm), 80, 16, ptr(loss), stream) == ERR and "null" in err()
        assert lib.bn_probe_epoch_weighted(h, ptr(X), ptr(Y), ptr(rw), None, 80, 16, ptr(loss), stream) == ERR
        assert lib.bn_probe_epoch_weighted(h, ptr(X), ptr(Y), ptr(rw), ptr(perm), 80, 0, ptr(loss), stream) == ERR and "batch" in err()
        assert lib.bn_probe_sweep_epoch_weighted(None, ptr(X), ptr(Y), ptr(rw), ptr(perm), 80, 16, ptr(sizes), None, ptr(sloss), stream) == ERR
        assert lib.bn_probe_sweep_epoch_weighted(sw, ptr(X), None, ptr(rw), ptr(perm), 80, 16, ptr(sizes), None, ptr(sloss), stream) == ERR and "null" in err()
        assert lib.bn_probe_sweep_epoch_weighted(sw, ptr(X), ptr(Y), ptr(rw), ptr(perm), 80, 81, ptr(sizes), None, ptr(sloss), stream) == ERR
        torch.cuda.synchronize()
        assert torch.isnan(loss).all() and torch.isnan(sloss).all()   # nothing ran
        # ... and all four are still usable: 80 row numbers into 64 rows, weights null or not, focal on the sigmoid ones
        assert lib.bn_probe_epoch_weighted(h, ptr(X), ptr(Y), ptr(rw), ptr(perm), 80, 16, ptr(loss), stream) == 0
        assert lib.bn_probe_epoch_weighted(hs, ptr(X), ptr(Y), None, ptr(perm), 80, 16, ptr(loss), stream) == 0
        assert lib.bn_probe_sweep_epoch_weighted(sw, ptr(X), ptr(Y), ptr(rw), ptr(perm), 80, 16, ptr(sizes), None, ptr(sloss), stream) == 0
        assert lib.bn_probe_sweep_epoch_weighted(sws, ptr(X), ptr(Y), None, ptr(perm), 80, 16, ptr(sizes), None, ptr(sloss), stream) == 0
        assert lib.bn_probe_loss(h, ptr(X), ptr(Y), 64, ptr(loss) + 4 * 7, stream) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(loss[:5]).all() and torch.isfinite(loss[7]) and torch.isfinite(sloss).all()
    finally:
        lib.bn_probe_destroy(h)
        lib.bn_probe_destroy(hs)
        lib.bn_probe_sweep_destroy(sw)
        lib.bn_probe_sweep_destroy(sws)
    assert _hip.PROBE_LOSSES == {"auto": 0, "focal": 1}


# -- end to end -----------------------------------------------------------------------------------------------------------------------
SR = 24000
FOLDERS = {"common": (700.0, 12), "rare": (2300.0, 3), "noise": (None, 3)}


def _write_wav(path, x):
    pcm = np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(SR)
        w.writeframes(pcm.tobytes())


def test_probe_command_with_focal_weights_and_upsampling(torch_mod, runner, tmp_path, capsys):
    """12 files of one class, 3 of the other, 3 in a noise folder -> probe --loss focal --class_weights balanced --upsample_ratio 0.5: the
    saved head has the bits of fit_probe with the weights and rows the public helpers derive from the same file list; analyze --head
    takes it; --tune records the four settings."""
    from birdnet_stm32.cli import analyze as analyze_cli
    from birdnet_stm32.cli import probe as probe_cli
    from birdnet_stm32.data.dataset import load_file_paths_from_directory
    from birdnet_stm32.evaluation.embeddings import embed_files
    from birdnet_stm32.training import linear_probe as lp

    rng = np.random.default_rng(5)
    t = np.arange(3 * SR) / SR
    train_dir = tmp_path / "train"
    files = []
    for kind, (f0, count) in FOLDERS.items():
        os.makedirs(train_dir / kind)
        for i in range(count):
            x = 0.3 * rng.standard_normal(t.size) + (np.sin(2 * np.pi * f0 * (1 + 0.02 * rng.standard_normal()) * t) if f0 else 0.0)
            _write_wav(train_dir / kind / f"{i:02d}.wav", 0.8 * x / np.abs(x).max())
            files.append(str(train_dir / kind / f"{i:02d}.wav"))
    out = str(tmp_path / "tail")
    flags = ["--epochs", "6", "--batch_size", "8", "--learning_rate", "0.01", "--dropout", "0.3", "--seed", "3",
             "--loss", "focal", "--focal_gamma", "1.5", "--class_weights", "balanced", "--upsample_ratio", "0.5"]
    common = ["--model_path", TFLITE_PATH, "--model_config", CONFIG_PATH, "--data_path_train", str(train_dir)]
    head = probe_cli.main([*common, "--output", out, *flags], runner=runner)
    printed = capsys.readouterr().out
    for suffix in (".npz", "_labels.txt", "_model_config.json", "_history.csv"):
        assert os.path.isfile(out + suffix), suffix
    loaded = lp.ProbeHead.load(out + ".npz")
    assert loaded.class_names == ["common", "rare"] and np.array_equal(loaded.W, head.W) and np.array_equal(loaded.b, head.b)

    # the same file list through the public helpers, in the command's order: shuffle, split, upsample, count, embed once per file
    np.random.seed(3)
    paths, classes = load_file_paths_from_directory(str(train_dir))
    tr_paths, va_paths = lp.split_train_val(paths, 0.2)
    mult, upsampled = lp.upsample_multiplicity(tr_paths, classes, 0.5)
    cw = lp.balanced_class_weights(upsampled, classes)
    emb = embed_files(runner, tr_paths + va_paths, max_duration=30, sample_rate=22050, chunk_duration=3.0)
    assert len(emb.paths) == 18 and emb.embeddings.shape[0] == 18       # one row per distinct file: nothing embedded twice
    Y, _keep = lp.targets_from_paths(emb.paths, classes, emb.file_index, "sigmoid")
    is_tr = np.asarray(emb.file_index) < len(tr_paths)
    rows = lp.upsample_rows(np.asarray(emb.file_index)[is_tr], mult)
    n_rare, n_noise = (sum(f"/{k}/" in p for p in tr_paths) for k in ("rare", "noise"))
    n_common = len(tr_paths) - n_rare - n_noise
    assert 0 < n_rare < n_common // 2 and n_noise > 0                 # (a condition on the seed: the split leaves something to upsample)
    assert len(rows) == n_common + n_common // 2 + n_noise and mult[[("/noise/" in p) for p in tr_paths]].tolist() == [1] * n_noise
    assert f"{int(is_tr.sum())} training rows -> {len(rows)} rows per epoch" in printed
    assert f"Balanced class weights: min={cw.min():.2f}, max={cw.max():.2f}" in printed
    alone = lp.fit_probe(runner, emb.embeddings[is_tr], Y[is_tr], emb.embeddings[~is_tr], Y[~is_tr], epochs=6, batch_size=8, learning_rate=0.01, dropout=0.3,
                         seed=3, loss="focal", focal_gamma=1.5, sample_weight=lp.row_weights(Y[is_tr], cw), rows=rows)
    assert np.array_equal(alone.W, loaded.W) and np.array_equal(alone.b, loaded.b)
    plain = lp.fit_probe(runner, emb.embeddings[is_tr], Y[is_tr], emb.embeddings[~is_tr], Y[~is_tr], epochs=6, batch_size=8, learning_rate=0.01, dropout=0.3, seed=3)
    assert not np.array_equal(plain.W, loaded.W)

    det = analyze_cli.main([*common[:4], "--head", out + ".npz", "--input", *files[:6], "--output", str(tmp_path / "det.csv"), "--min_conf", "0.0",
                            "--top_k", "1"], runner=runner)
    assert len(det) >= 6 and os.path.isfile(tmp_path / "det.csv")

    tuned_out = str(tmp_path / "tuned")
    probe_cli.main([*common, "--output", tuned_out, *flags, "--tune", "--n_trials", "3", "--tune_seed", "9"], runner=runner)
    report = json.load(open(tuned_out + "_tune.json"))
    assert report["n_trials"] == 3 and len(report["trials"]) == 3
    assert (report["loss"], report["focal_gamma"], report["class_weights"], report["upsample_ratio"]) == ("focal", 1.5, "balanced", 0.5)
    assert all("loss" not in r["params"] and "focal_gamma" not in r["params"] for r in report["trials"])   # no part of the search space
    # trial 0 is the command line's own settings: the head of the run without --tune, bit for bit in its validation losses
    assert report["trials"][0]["val_loss"] == [float(v) for v in loaded.history["val_loss"]]
