"""GPU tests of the probe's hyperparameter sweep (csrc/bn_probe_sweep.hip, bn_probe_sweep_*): a trial has the bits of a single fit, label
smoothing tracks the float64 restatement, trials stop independently, determinism, refused calls, and probe --tune end to end."""

import ctypes
import json
import os
import wave

import numpy as np
import pytest

from conftest import CONFIG_PATH, TFLITE_PATH

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


def _clusters(n, D, C, seed, multi_hot=False):
    """Rectified Gaussian clusters: separable, non-negative like pooled ReLU features (the recipe of tests/test_gpu_probe.py)."""
    cent = np.random.default_rng(1000 + D + C).standard_normal((C, D))
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, C, n)
    X = np.maximum(cent[lab] + 1.5 * rng.standard_normal((n, D)), 0).astype(np.float32)
    Y = np.eye(C, dtype=np.float32)[lab]
    if multi_hot:
        Y[::7] = 0.0
        Y[np.arange(3, n, 11), rng.integers(0, C, len(range(3, n, 11)))] = 1.0
    return X, Y, lab


def _trials():
    from birdnet_stm32.training.linear_probe import ProbeTrial

    return [ProbeTrial(learning_rate=1e-3, optimizer="adam", dropout=0.5, clipnorm=1.0),
            ProbeTrial(learning_rate=3e-3, optimizer="adamw", weight_decay=1e-3, dropout=0.0, clipnorm=0.0),
            ProbeTrial(learning_rate=1e-2, optimizer="sgd", dropout=0.3, clipnorm=2.0)]


def _assert_same_head(a, b, what):
    assert np.array_equal(a.W, b.W) and np.array_equal(a.b, b.b), f"{what}: weights differ, max {np.abs(a.W - b.W).max():.3e}"
    assert np.array_equal(a.history["step_loss"], b.history["step_loss"]), f"{what}: step losses differ"
    assert a.history["val_loss"] == b.history["val_loss"], f"{what}: validation losses differ"
    assert a.history["best_epoch"] == b.history["best_epoch"] and a.history["stopped_epoch"] == b.history["stopped_epoch"]


@pytest.mark.parametrize("D,C,n,n_val,batch,T,epochs,activation", [
    (256, 40, 2000, 300, 96, 3, 2, "sigmoid"),    # several row groups (the reduce kernel runs), a short last batch
    (256, 40, 2000, 300, 96, 3, 2, "softmax"),
    (255, 13, 70, 20, 33, 2, 2, "sigmoid"),       # no tile multiples
    (64, 2100, 48, 16, 48, 2, 1, "softmax"),      # C > 2048: the two-pass forward
])
def test_a_trial_is_a_single_fit_bit_for_bit(torch_mod, ctx, D, C, n, n_val, batch, T, epochs, activation):
    from birdnet_stm32.training.linear_probe import fit_probe, fit_probe_sweep

    X, Y, _ = _clusters(n, D, C, seed=8)
    Xv, Yv, _ = _clusters(n_val, D, C, seed=9)
    trials = _trials()[:T]
    kw = dict(activation=activation, epochs=epochs, batch_size=batch, seed=11)
    sweep = fit_probe_sweep(ctx, X, Y, Xv, Yv, trials, **kw)
    assert len(sweep.heads) == T
    for t, trial in enumerate(trials):
        kwt = trial.fit_kwargs()
        assert kwt.pop("label_smoothing") == 0.0
        single = fit_probe(ctx, X, Y, Xv, Yv, **kw, **kwt)     # label_smoothing absent: the single-fit kernels
        _assert_same_head(sweep.heads[t], single, f"trial {t} ({trial.optimizer})")
        assert len(single.history["step_loss"]) == epochs * -(-n // batch)
    assert not np.array_equal(sweep.heads[0].W, sweep.heads[1].W)


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
def test_label_smoothing_tracks_the_float64_restatement(torch_mod, ctx, activation):
    """3 epochs of batch 32 over 1027 rows (a short last batch), dropout 0.5, clip 1, two trials with eps = 0.1 and 0.2.  The rule of
    test_many_steps_track_the_float64_restatement: d32 = distance of the float32 restatement from the float64 one, measured here; the
    device (float32 too, another summation order) must be within 8 d32 of float64, in weights and step losses."""
    from birdnet_stm32.training.linear_probe import ProbeTrial, fit_probe, fit_probe_sweep, fit_probe_sweep_reference

    X, Y, _ = _clusters(1027, 256, 12, seed=3)
    trials = [ProbeTrial(learning_rate=1e-3, dropout=0.5, clipnorm=1.0, label_smoothing=eps) for eps in (0.1, 0.2)]
    kw = dict(activation=activation, epochs=3, batch_size=32, seed=42)
    r64 = fit_probe_sweep_reference(X, Y, trials=trials, dtype=np.float64, **kw)
    r32 = fit_probe_sweep_reference(X, Y, trials=trials, dtype=np.float32, **kw)
    dev = fit_probe_sweep(ctx, X, Y, trials=trials, **kw)
    plain = fit_probe(ctx, X, Y, learning_rate=1e-3, dropout=0.5, clipnorm=1.0, **kw)
    ratios = []
    for t, trial in enumerate(trials):
        P64 = np.concatenate([r64.heads[t].history["W"], r64.heads[t].history["b"][None, :]])
        P32 = np.concatenate([r32.heads[t].history["W"], r32.heads[t].history["b"][None, :]]).astype(np.float64)
        Pd = np.concatenate([dev.heads[t].W, dev.heads[t].b[None, :]]).astype(np.float64)
        d32, dd = _rel(P32, P64), _rel(Pd, P64)
        l32 = _rel(r32.heads[t].history["step_loss"], r64.heads[t].history["step_loss"])
        ld = _rel(dev.heads[t].history["step_loss"], r64.heads[t].history["step_loss"])
        print(f"{activation} eps={trial.label_smoothing}: weights d32 {d32:.3e} device {dd:.3e} (ratio {dd / d32:.2f}); step losses d32 {l32:.3e} "
              f"device {ld:.3e} (ratio {ld / l32:.2f})")
        ratios.append((dd, d32, ld, l32))
        assert not np.array_equal(dev.heads[t].W, plain.W)     # the smoothing did something
    for dd, d32, ld, l32 in ratios:
        assert dd <= 8 * d32
        assert ld <= 8 * l32
    # ... and fit_probe(label_smoothing=eps) is the sweep of one trial
    one = fit_probe(ctx, X, Y, learning_rate=1e-3, dropout=0.5, clipnorm=1.0, label_smoothing=0.2, **kw)
    assert np.array_equal(one.W, dev.heads[1].W) and np.array_equal(one.history["step_loss"], dev.heads[1].history["step_loss"])


def test_trials_stop_independently(torch_mod, ctx):
    """A validation set with shuffled labels: the faster a trial fits the training set, the sooner its validation loss turns.  The
    reference (float64) gives each trial's best and stopped epoch — asserted here to be what the case was built for — the device must
    reproduce them, and each trial's head must be fit_probe's for that trial alone: a stopped trial's weights and snapshot never moved
    while the others trained on."""
    from birdnet_stm32.training.linear_probe import ProbeTrial, fit_probe, fit_probe_sweep, fit_probe_sweep_reference

    X, Y, _ = _clusters(512, 64, 6, seed=1)
    Xv, Yv, _ = _clusters(128, 64, 6, seed=2)
    Yv = Yv[np.random.default_rng(0).permutation(len(Yv))]
    trials = [ProbeTrial(learning_rate=2e-2, optimizer="adam", dropout=0.0),
              ProbeTrial(learning_rate=2e-3, optimizer="adamw", weight_decay=1e-2, dropout=0.5),
              ProbeTrial(learning_rate=3e-4, optimizer="adam", dropout=0.2)]
    kw = dict(epochs=30, batch_size=32, patience=3, seed=5)
    ref = fit_probe_sweep_reference(X, Y, Xv, Yv, trials, dtype=np.float64, **kw)
    want = [(h.history["best_epoch"], h.history["stopped_epoch"]) for h in ref.heads]
    print("reference (best, stopped):", want)
    assert want == [(0, 3), (2, 5), (29, None)]
    dev = fit_probe_sweep(ctx, X, Y, Xv, Yv, trials, **kw)
    got = [(h.history["best_epoch"], h.history["stopped_epoch"]) for h in dev.heads]
    print("device    (best, stopped):", got, "best-epoch val_loss", [min(h.history["val_loss"]) for h in dev.heads])
    assert got == want
    for t, trial in enumerate(trials):
        kwt = trial.fit_kwargs()
        kwt.pop("label_smoothing")
        _assert_same_head(dev.heads[t], fit_probe(ctx, X, Y, Xv, Yv, **kw, **kwt), f"trial {t}")
        assert len(dev.heads[t].history["val_loss"]) == (want[t][1] + 1 if want[t][1] is not None else 30)
    best = [min(h.history["val_loss"]) for h in dev.heads]
    assert dev.best == int(np.argmin(best)) and dev.best_head is dev.heads[dev.best]


def test_same_sweep_twice_same_bits(torch_mod, ctx):
    from birdnet_stm32.training.linear_probe import ProbeTrial, fit_probe_sweep

    X, Y, _ = _clusters(700, 256, 40, seed=8, multi_hot=True)
    Xv, Yv, _ = _clusters(100, 256, 40, seed=9)
    trials = _trials() + [ProbeTrial(learning_rate=2e-3, label_smoothing=0.1)]
    kw = dict(epochs=2, batch_size=96, seed=11)
    a = fit_probe_sweep(ctx, X, Y, Xv, Yv, trials, **kw)
    b = fit_probe_sweep(ctx, torch_mod.from_numpy(X).cuda(), torch_mod.from_numpy(Y).cuda(), Xv, Yv, trials, **kw)
    for t in range(len(trials)):
        _assert_same_head(a.heads[t], b.heads[t], f"trial {t}")
    assert a.best == b.best
    # the order of the trials does not matter to a trial
    c = fit_probe_sweep(ctx, X, Y, Xv, Yv, trials[::-1], **kw)
    for t in range(len(trials)):
        _assert_same_head(a.heads[t], c.heads[len(trials) - 1 - t], f"trial {t} reversed")


def test_sweep_abi_refuses_bad_calls(torch_mod, ctx):
    torch = torch_mod
    from birdnet_stm32 import _hip

    lib = ctx.lib
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    X, Y = torch.rand((64, 32), device="cuda"), torch.zeros((64, 5), device="cuda")
    W, b = torch.zeros((32, 5), device="cuda"), torch.zeros(5, device="cuda")
    perm = torch.arange(64, dtype=torch.int32, device="cuda")
    sizes = torch.full((4, 2, 2), 1e-3, device="cuda")
    active, loss = torch.ones(2, dtype=torch.uint8, device="cuda"), torch.full((4, 2), -1.0, device="cuda")

    def err():
        return lib.bn_last_error().decode()

    def rows(*trials):
        return (_hip.ProbeTrialStruct * len(trials))(*[_hip.ProbeTrialStruct(*t) for t in trials])

    ok = (0, 1e-3, 0.0, 1.0, 0.5, 0.0)
    h = ctypes.c_void_p()
    mk = lambda D, C, act, T, tr, total, w, bb: lib.bn_probe_sweep_create(ctx.handle, D, C, act, T, tr, 1, total, w, bb, ctypes.byref(h), stream)   # noqa: E731
    assert mk(32, 5, 0, 0, rows(ok), 10, W.data_ptr(), b.data_ptr()) == -1 and "T=0" in err()
    assert mk(32, 5, 0, 65, rows(*[ok] * 65), 10, W.data_ptr(), b.data_ptr()) == -1 and "T=65" in err()
    assert mk(32, 5, 0, 2, rows(ok, (0, 1e-3, 0.0, 1.0, 1.0, 0.0)), 10, W.data_ptr(), b.data_ptr()) == -1 and "trial 1" in err() and "dropout" in err()
    assert mk(32, 5, 0, 2, rows(ok, (0, 1e-3, 0.0, 1.0, 0.5, 1.0)), 10, W.data_ptr(), b.data_ptr()) == -1 and "label_smoothing" in err()
    assert mk(32, 5, 0, 1, rows((0, 1e-3, 0.0, 1.0, 0.5, -0.1)), 10, W.data_ptr(), b.data_ptr()) == -1 and "label_smoothing" in err()
    assert mk(32, 5, 0, 1, rows((3, 1e-3, 0.0, 1.0, 0.5, 0.0)), 10, W.data_ptr(), b.data_ptr()) == -1 and "optimizer" in err()
    assert mk(32, 5, 0, 2, None, 10, W.data_ptr(), b.data_ptr()) == -1 and "null" in err()
    assert mk(32, 5, 0, 2, rows(ok, ok), 10, None, b.data_ptr()) == -1 and "null" in err()
    assert mk(32, 5, 0, 2, rows(ok, ok), 0, W.data_ptr(), b.data_ptr()) == -1 and "total_steps" in err()
    assert mk(32, 5, 2, 2, rows(ok, ok), 10, W.data_ptr(), b.data_ptr()) == -1 and "activation" in err()
    assert mk(4096, 5, 0, 2, rows(ok, ok), 10, W.data_ptr(), b.data_ptr()) == -1
    # over the byte cap: the largest head, 64 trials; the message names the largest T that fits
    assert mk(2048, 4096, 0, 64, rows(*[ok] * 64), 10, W.data_ptr(), b.data_ptr()) == -4 and "largest T that fits is 15" in err() and not h.value
    assert lib.bn_probe_sweep_create(ctx.handle, 32, 5, 0, 2, rows(ok, ok), 1, 10, W.data_ptr(), b.data_ptr(), None, stream) == -1
    assert mk(32, 5, 0, 2, rows(ok, ok), 10, W.data_ptr(), b.data_ptr()) == 0 and h.value
    try:
        ep = lambda hh, x, y, p, n, batch, sz, ac, ls: lib.bn_probe_sweep_epoch(hh, x, y, p, n, batch, sz, ac, ls, stream)   # noqa: E731
        args = (X.data_ptr(), Y.data_ptr(), perm.data_ptr(), 64, 16, sizes.data_ptr(), active.data_ptr(), loss.data_ptr())
        assert ep(h, *args[:4], 0, *args[5:]) == -1 and "batch" in err()
        assert ep(h, *args[:4], 65, *args[5:]) == -1
        assert ep(h, args[0], None, *args[2:]) == -1 and "null" in err()
        assert ep(h, *args[:5], None, *args[6:]) == -1 and "null" in err()
        assert ep(None, *args) == -1
        assert lib.bn_probe_sweep_loss(h, X.data_ptr(), Y.data_ptr(), 0, None, loss.data_ptr(), stream) == -1
        assert lib.bn_probe_sweep_loss(h, X.data_ptr(), None, 64, None, loss.data_ptr(), stream) == -1
        assert lib.bn_probe_sweep_snapshot(h, None, stream) == -1 and lib.bn_probe_sweep_snapshot(None, active.data_ptr(), stream) == -1
        assert lib.bn_probe_sweep_get(h, 2, 0, W.data_ptr(), b.data_ptr(), stream) == -1 and "trial 2" in err()
        assert lib.bn_probe_sweep_get(h, 0, 2, W.data_ptr(), b.data_ptr(), stream) == -1
        assert lib.bn_probe_sweep_get(h, 0, 0, None, b.data_ptr(), stream) == -1
        torch.cuda.synchronize()
        assert bool((loss == -1.0).all())                       # nothing was launched
        # ... and the sweep is still usable; an inactive trial is left alone (its losses too)
        active[1] = 0
        assert ep(h, *args) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(loss[:, 0]).all() and bool((loss[:, 0] > 0).all()) and bool((loss[:, 1] == -1.0).all())
        W1, b1 = torch.full_like(W, 7.0), torch.full_like(b, 7.0)
        assert lib.bn_probe_sweep_get(h, 1, _hip.PROBE_SWEEP_CURRENT, W1.data_ptr(), b1.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert torch.equal(W1, W) and torch.equal(b1, b)        # trial 1 still has the initial weights
        assert lib.bn_probe_sweep_get(h, 0, _hip.PROBE_SWEEP_CURRENT, W1.data_ptr(), b1.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert not torch.equal(W1, W)
    finally:
        lib.bn_probe_sweep_destroy(h)
    from birdnet_stm32.training.linear_probe import ProbeTrial, fit_probe_sweep

    with pytest.raises(ValueError, match="at most 64"):
        fit_probe_sweep(ctx, X, Y, trials=[ProbeTrial()] * 65)
    assert _hip.PROBE_SWEEP_MAX_TRIALS == 64


# -- end to end -----------------------------------------------------------------------------------------------------------------------
SR = 24000
TONES = {"low": 700.0, "mid": 2300.0, "high": 5100.0}


def _write_wav(path, x):
    pcm = np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(SR)
        w.writeframes(pcm.tobytes())


def test_probe_tune_end_to_end(torch_mod, tmp_path):
    """Three class folders of 3 s tones in noise -> probe --tune --n_trials 4 -> the files; the saved head is the winning trial's, trial 0
    is the command line's own settings; analyze --head runs on the result."""
    from birdnet_stm32.cli import analyze as analyze_cli
    from birdnet_stm32.cli import probe as probe_cli
    from birdnet_stm32.data.dataset import load_file_paths_from_directory
    from birdnet_stm32.evaluation.embeddings import embed_files
    from birdnet_stm32.models.runners import load_model_runner
    from birdnet_stm32.training.linear_probe import ProbeHead, ProbeTrial, fit_probe, split_train_val, targets_from_paths
    from birdnet_stm32.training.tune import sample_trials

    rng = np.random.default_rng(5)
    t = np.arange(3 * SR) / SR
    train_dir = tmp_path / "train"
    files = []
    for kind, f0 in TONES.items():
        os.makedirs(train_dir / kind)
        for i in range(8):
            x = np.sin(2 * np.pi * f0 * (1 + 0.02 * rng.standard_normal()) * t) + 0.3 * rng.standard_normal(t.size)
            _write_wav(train_dir / kind / f"{i:02d}.wav", 0.8 * x / np.abs(x).max())
            files.append(str(train_dir / kind / f"{i:02d}.wav"))
    runner = load_model_runner(TFLITE_PATH, max_batch=64, prepare_pipeline=True)
    try:
        out = str(tmp_path / "tuned")
        flags = ["--epochs", "6", "--batch_size", "8", "--learning_rate", "0.005", "--dropout", "0.3", "--label_smoothing", "0.05", "--seed", "3"]
        head = probe_cli.main(["--model_path", TFLITE_PATH, "--model_config", CONFIG_PATH, "--data_path_train", str(train_dir), "--output", out,
                               "--tune", "--n_trials", "4", "--tune_seed", "9", *flags], runner=runner)
        for suffix in (".npz", "_labels.txt", "_model_config.json", "_history.csv", "_tune.json"):
            assert os.path.isfile(out + suffix), suffix
        report = json.load(open(out + "_tune.json"))
        base = ProbeTrial(learning_rate=0.005, dropout=0.3, label_smoothing=0.05)
        trials = sample_trials(4, 9, base)
        assert report["n_trials"] == 4 and len(report["trials"]) == 4 and report["objective"] == "val_loss"
        assert [r["params"] for r in report["trials"]] == [tr.fit_kwargs() for tr in trials] and report["trials"][0]["params"] == base.fit_kwargs()
        best_vals = [r["best_val_loss"] for r in report["trials"]]
        win = report["best_trial"]
        assert win == int(np.argmin(best_vals)) and 0.0 <= report["best_val_macro_roc_auc"] <= 1.0
        for r in report["trials"]:
            assert len(r["val_loss"]) >= 1 and r["best_val_loss"] == min(r["val_loss"]) and r["val_loss"][r["best_epoch"]] == r["best_val_loss"]
        loaded = ProbeHead.load(out + ".npz")
        assert loaded.class_names == sorted(TONES) and np.array_equal(loaded.W, head.W) and np.array_equal(loaded.b, head.b)
        assert loaded.history["val_loss"] == report["trials"][win]["val_loss"]
        lines = open(out + "_history.csv").read().strip().split("\n")
        assert len(lines) == 1 + len(report["trials"][win]["val_loss"])

        # the winning trial alone, on the command's split and embeddings, gives the saved head
        np.random.seed(3)
        paths, classes = load_file_paths_from_directory(str(train_dir))
        tr_paths, va_paths = split_train_val(paths, 0.2)
        emb = embed_files(runner, tr_paths + va_paths, max_duration=30, sample_rate=22050, chunk_duration=3.0)
        Y, _keep = targets_from_paths(emb.paths, classes, emb.file_index, "sigmoid")
        is_tr = emb.file_index < len(tr_paths)
        alone = fit_probe(runner, emb.embeddings[is_tr], Y[is_tr], emb.embeddings[~is_tr], Y[~is_tr], epochs=6, batch_size=8, seed=3, **trials[win].fit_kwargs())
        assert np.array_equal(alone.W, loaded.W) and np.array_equal(alone.b, loaded.b)

        det = analyze_cli.main(["--model_path", TFLITE_PATH, "--model_config", CONFIG_PATH, "--head", out + ".npz", "--input", *files[:6],
                                "--output", str(tmp_path / "det.csv"), "--min_conf", "0.0", "--top_k", "1"], runner=runner)
        assert len(det) >= 6 and os.path.isfile(tmp_path / "det.csv")
    finally:
        runner.close()
