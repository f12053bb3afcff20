"""GPU tests of the linear probe: the training step (csrc/bn_probe.hip) against the numpy restatement in float64, determinism, early
stopping, bn_head_forward against numpy and against the runner's own head, refused calls, and probe -> analyze --head end to end."""

import ctypes
import math
import os
import wave

import numpy as np
import pytest

from conftest import CONFIG_PATH, KERAS_PATH, TFLITE_PATH

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # unit roundoff of float32


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
    """Rectified Gaussian clusters: separable, non-negative like pooled ReLU features."""
    cent = np.random.default_rng(1000 + D + C).standard_normal((C, D))
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, C, n)
    X = np.maximum(cent[lab] + 1.5 * rng.standard_normal((n, D)), 0).astype(np.float32)
    Y = np.eye(C, dtype=np.float32)[lab]
    if multi_hot:
        Y[::7] = 0.0                                           # "noise" rows
        Y[np.arange(3, n, 11), rng.integers(0, C, len(range(3, n, 11)))] = 1.0   # a second label
    return X, Y, lab


def _prob_bound(X, W, b, activation):
    """Float64 probabilities P and a bound on the float32 device error of P.

    Logits: a length-D dot product accumulated in float32 (v_mfma_f32_16x16x4_f32 is an fmaf chain) plus the bias:
    |dz| <= (D + 2) u (|x| |W| + |b|).  Sigmoid 1 / (1 + expf(-z)): expf is within 1 ulp (ocml), the addition and the IEEE division
    half an ulp each, and d sigma / dz <= 1/4: |dP| <= dz / 4 + 4 u P.  Softmax expf(z - m) / sum: the subtraction, expf, the division
    and a sum of C terms added as at most 8 + 4 + 16 partial sums: |dP| <= P (2 max_row dz + 40 u)."""
    D = X.shape[0] and X.shape[1]
    X, W, b = X.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    z = X @ W + b
    dz = (D + 2) * U * (np.abs(X) @ np.abs(W) + np.abs(b))
    if activation == "softmax":
        e = np.exp(z - z.max(axis=1, keepdims=True))
        P = e / e.sum(axis=1, keepdims=True)
        return P, P * (2 * dz.max(axis=1, keepdims=True) + 40 * U)
    P = 1.0 / (1.0 + np.exp(-z))
    return P, dz / 4 + 4 * U * P


@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
@pytest.mark.parametrize("D,C,B", [(256, 100, 32), (96, 7, 5), (320, 1000, 512), (2048, 4096, 64), (255, 13, 33)])
def test_one_sgd_step_is_the_gradient(torch_mod, ctx, activation, D, C, B):
    """One SGD step with lr = 1 (momentum starts at zero), no dropout, no clip: W0 - W1 is the gradient, compared element by element with
    float64 under the float32 dot-product bound |err| <= (K + c) 2^-24 sum_k |a_k b_k|: K = D for the logits that feed G (propagated
    through the activation, see _prob_bound), K = B for dW = x^T G, plus one rounding of the stored W1 = fl(W0 - g)."""
    from birdnet_stm32.training.linear_probe import fit_probe, init_head

    X, Y, _ = _clusters(B, D, C, seed=5, multi_hot=activation == "sigmoid")
    X *= 0.25
    head = fit_probe(ctx, X, Y, activation=activation, epochs=1, batch_size=B, learning_rate=1.0, optimizer="sgd", clipnorm=0.0, dropout=0.0, seed=9)
    W0, b0 = init_head(D, C, 9)
    got = np.concatenate([W0.astype(np.float64) - head.W, (b0.astype(np.float64) - head.b)[None, :]])
    P, dP = _prob_bound(X, W0, b0, activation)
    scale = B if activation == "softmax" else B * C
    G = (P - Y) / scale
    dG = (dP + 2 * U * np.abs(P - Y)) / scale
    Xa = np.concatenate([X.astype(np.float64), np.ones((B, 1))], axis=1)
    want = Xa.T @ G
    bound = np.abs(Xa).T @ dG + (B + 2) * U * (np.abs(Xa).T @ np.abs(G)) + U * np.abs(np.concatenate([head.W, head.b[None, :]]))
    err = np.abs(got - want)
    print(f"{activation} D={D} C={C} B={B}: max err {err.max():.3e}, max err/bound {np.max(err / bound):.3f}, |g| max {np.abs(want).max():.3e}")
    assert np.all(err <= bound)
    loss64 = _loss64(P, Y, activation)
    assert abs(head.history["step_loss"][0] - loss64) <= 1e-5 * max(1.0, abs(loss64))


def _loss64(P, Y, activation):
    from birdnet_stm32.training.linear_probe import probe_loss

    return float(probe_loss(P, Y.astype(np.float64), activation))


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("optimizer,C,activation", [("adam", 12, "sigmoid"), ("adam", 100, "sigmoid"), ("adamw", 12, "sigmoid"), ("sgd", 12, "sigmoid"),
                                                    ("adam", 12, "softmax")])
def test_many_steps_track_the_float64_restatement(torch_mod, ctx, optimizer, C, activation):
    """4 epochs of batch 32 over 4099 rows (a short last batch), dropout 0.5, clip 1.  d32 = distance of the float32 restatement from the
    float64 one, measured here; the device (float32 too, another summation order) must be within 8 d32 of float64, weights and losses."""
    from birdnet_stm32.training.linear_probe import fit_probe, fit_probe_reference

    X, Y, _ = _clusters(4099, 256, C, seed=3)
    kw = dict(activation=activation, epochs=4, batch_size=32, learning_rate=1e-3, optimizer=optimizer, weight_decay=1e-2 if optimizer == "adamw" else 0.0,
              clipnorm=1.0, dropout=0.5, seed=42)
    r64 = fit_probe_reference(X, Y, dtype=np.float64, **kw)
    r32 = fit_probe_reference(X, Y, dtype=np.float32, **kw)
    dev = fit_probe(ctx, X, Y, **kw)
    P64 = np.concatenate([r64.history["W"], r64.history["b"][None, :]])
    P32 = np.concatenate([r32.history["W"], r32.history["b"][None, :]]).astype(np.float64)
    Pd = np.concatenate([dev.W, dev.b[None, :]]).astype(np.float64)
    d32, dd = _rel(P32, P64), _rel(Pd, P64)
    l32, ld = _rel(r32.history["step_loss"], r64.history["step_loss"]), _rel(dev.history["step_loss"], r64.history["step_loss"])
    print(f"{optimizer} C={C} {activation}: weights d32 {d32:.3e} device {dd:.3e} (ratio {dd / d32:.2f}); step losses d32 {l32:.3e} device {ld:.3e} "
          f"(ratio {ld / l32:.2f}); loss {dev.history['loss'][0]:.4f} -> {dev.history['loss'][-1]:.4f}")
    assert dev.history["loss"][-1] < 0.5 * dev.history["loss"][0]
    assert dd <= 8 * d32
    assert ld <= 8 * l32


@pytest.mark.parametrize("D,C,batch,tail", [(256, 12, 4096, 1632), (256, 100, 1000, 816)])
def test_short_last_batch_with_more_row_groups_than_the_full_batch(torch_mod, ctx, D, C, batch, tail):
    """The rows per group are rounded up to a multiple of 4, so the group count is not monotone in the batch: at D = 256, C = 12 a
    full batch of 4096 has 94 groups (44 rows each), a last batch of 1632 has 102 (16 rows each); at C = 100, 1000 rows have 50 groups and
    816 rows have 51.  The workspace must hold the larger count.  Two epochs against the restatement, bound as above."""
    from birdnet_stm32.training.linear_probe import fit_probe, fit_probe_reference

    X, Y, _ = _clusters(batch + tail, D, C, seed=21)
    kw = dict(epochs=2, batch_size=batch, learning_rate=1e-2, optimizer="adam", clipnorm=1.0, dropout=0.5, seed=4)
    r64 = fit_probe_reference(X, Y, dtype=np.float64, **kw)
    r32 = fit_probe_reference(X, Y, dtype=np.float32, **kw)
    dev = fit_probe(ctx, X, Y, **kw)
    again = fit_probe(ctx, X, Y, **kw)
    P64 = np.concatenate([r64.history["W"], r64.history["b"][None, :]])
    d32 = _rel(np.concatenate([r32.history["W"], r32.history["b"][None, :]]).astype(np.float64), P64)
    dd = _rel(np.concatenate([dev.W, dev.b[None, :]]).astype(np.float64), P64)
    l32, ld = _rel(r32.history["step_loss"], r64.history["step_loss"]), _rel(dev.history["step_loss"], r64.history["step_loss"])
    print(f"D={D} C={C} batch={batch}+{tail}: weights d32 {d32:.3e} device {dd:.3e}; step losses d32 {l32:.3e} device {ld:.3e}")
    assert np.array_equal(dev.W, again.W) and np.array_equal(dev.b, again.b)
    assert dd <= 8 * d32 and ld <= 8 * l32


def test_same_seed_same_bits(torch_mod, ctx):
    torch = torch_mod
    from birdnet_stm32.training.linear_probe import fit_probe

    X, Y, _ = _clusters(2000, 256, 40, seed=8)
    Xv, Yv, _ = _clusters(300, 256, 40, seed=9)
    kw = dict(epochs=2, batch_size=96, optimizer="adamw", weight_decay=1e-3)   # 96 rows: several row groups, the reduce kernel runs
    a = fit_probe(ctx, X, Y, Xv, Yv, seed=11, **kw)
    b = fit_probe(ctx, torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), Xv, Yv, seed=11, **kw)
    c = fit_probe(ctx, X, Y, Xv, Yv, seed=12, **kw)
    assert torch.equal(torch.from_numpy(a.W), torch.from_numpy(b.W)) and torch.equal(torch.from_numpy(a.b), torch.from_numpy(b.b))
    assert np.array_equal(a.history["step_loss"], b.history["step_loss"]) and a.history["val_loss"] == b.history["val_loss"]
    assert not np.array_equal(a.W, c.W)


def test_early_stopping_restores_the_best_epoch(torch_mod, ctx):
    """A validation set with shuffled labels: the validation loss rises once the head fits the training set.  The returned weights are
    those of the best epoch: equal to a run of the same schedule stopped there."""
    from birdnet_stm32.training import linear_probe as lp

    X, Y, _ = _clusters(512, 64, 6, seed=1)
    Xv, Yv, _ = _clusters(128, 64, 6, seed=2)
    Yv = Yv[np.random.default_rng(0).permutation(len(Yv))]
    kw = dict(epochs=30, batch_size=32, learning_rate=2e-2, dropout=0.0, seed=5)
    head = lp.fit_probe(ctx, X, Y, Xv, Yv, patience=3, **kw)
    h = head.history
    best = h["best_epoch"]
    print("val_loss", [round(v, 4) for v in h["val_loss"]], "best", best, "stopped", h["stopped_epoch"])
    assert h["stopped_epoch"] is not None and h["stopped_epoch"] == best + 3 and best == int(np.argmin(h["val_loss"]))
    plan = lp._plan_fit(X, Y, None, device=True, activation="sigmoid", optimizer="adam", batch_size=32, dropout=0.0, epochs=30, learning_rate=2e-2,
                        weight_decay=0.0, clipnorm=1.0, seed=5)
    be = lp._DeviceBackend(ctx, X, Y, None, None, plan)
    try:
        for epoch in range(best + 1):
            be.epoch(lp.epoch_permutation(5, epoch, 512))
        W, b = be.get()
        assert np.array_equal(W.cpu().numpy(), head.W) and np.array_equal(b.cpu().numpy(), head.b)
    finally:
        be.close()


@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
@pytest.mark.parametrize("n,D,C", [(1000, 256, 100), (37, 96, 7), (129, 2048, 4096), (16, 1, 1)])
def test_head_forward_against_numpy(torch_mod, ctx, activation, n, D, C):
    from birdnet_stm32.training.linear_probe import ProbeHead

    rng = np.random.default_rng(n + C)
    X = np.maximum(rng.standard_normal((n, D)), 0).astype(np.float32)
    W = (rng.standard_normal((D, C)) / math.sqrt(D)).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    head = ProbeHead(W, b, activation)
    got = head.predict(X, ctx)
    P, dP = _prob_bound(X, W, b, activation)
    err = np.abs(got - P)
    print(f"{activation} n={n} D={D} C={C}: max err {err.max():.3e}, max err/bound {np.max(err / dP):.3f}")
    assert got.shape == (n, C) and got.dtype == np.float32 and np.all(err <= dP + U * P)   # (+ the rounding of the stored float32)
    d = torch_mod.from_numpy(X).cuda()
    assert torch_mod.equal(head.predict(d, ctx).cpu(), torch_mod.from_numpy(got))


def test_head_forward_matches_the_runners_own_head(torch_mod, ctx):
    """The shipped float32 model's dense kernel and bias as a head on that model's float32 embeddings give the runner's scores: the head
    path and the fused head kernels agree within the dot-product bound (both sum 256 float32 products, in different orders)."""
    from conftest import synth_chunks

    from birdnet_stm32.models._keras_loader import load_keras_archive
    from birdnet_stm32.models.runners import load_model_runner
    from birdnet_stm32.training.linear_probe import ProbeHead

    spec = load_keras_archive(KERAS_PATH)
    dense = spec.layers[-1]
    W, b = np.asarray(dense.weights["kernel"], np.float32), np.asarray(dense.weights["bias"], np.float32)
    act = dense.attrs.get("activation")
    assert act in ("sigmoid", "softmax") and W.shape[0] == 256
    runner = load_model_runner(KERAS_PATH, max_batch=32)
    try:
        audio = torch_mod.from_numpy(synth_chunks(24, seed=4)).cuda()
        scores, emb = runner.infer_audio_device(audio, return_embeddings=True)
        got = ProbeHead(W, b, act).predict(emb.contiguous(), runner.ctx).cpu().numpy()
        _P, dP = _prob_bound(emb.cpu().numpy(), W, b, act)
        err = np.abs(got.astype(np.float64) - scores.cpu().numpy())
        print(f"runner head vs bn_head_forward: max err {err.max():.3e}, max err/bound {np.max(err / (2 * dP + 2 * U)):.3f}")
        assert np.all(err <= 2 * dP + 2 * U)   # each side is within dP of the exact value
    finally:
        runner.close()


def test_probe_abi_refuses_bad_calls(torch_mod, ctx):
    torch = torch_mod
    from birdnet_stm32 import _hip

    lib = ctx.lib
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    X, Y = torch.rand((64, 32), device="cuda"), torch.zeros((64, 5), device="cuda")
    W, b = torch.zeros((32, 5), device="cuda"), torch.zeros(5, device="cuda")
    out, perm = torch.empty((64, 5), device="cuda"), torch.arange(64, dtype=torch.int32, device="cuda")
    loss = torch.empty(64, device="cuda")

    def err():
        return lib.bn_last_error().decode()

    assert lib.bn_head_forward(ctx.handle, None, 64, 32, W.data_ptr(), b.data_ptr(), 5, 0, out.data_ptr(), stream) == -1 and "null" in err()
    assert lib.bn_head_forward(ctx.handle, X.data_ptr(), 64, 0, W.data_ptr(), b.data_ptr(), 5, 0, out.data_ptr(), stream) == -1 and "D=0" in err()
    assert lib.bn_head_forward(ctx.handle, X.data_ptr(), 64, 2049, W.data_ptr(), b.data_ptr(), 5, 0, out.data_ptr(), stream) == -1
    assert lib.bn_head_forward(ctx.handle, X.data_ptr(), 64, 32, W.data_ptr(), b.data_ptr(), 4097, 0, out.data_ptr(), stream) == -1 and "C=4097" in err()
    assert lib.bn_head_forward(ctx.handle, X.data_ptr(), 64, 32, W.data_ptr(), b.data_ptr(), 5, 2, out.data_ptr(), stream) == -1 and "activation" in err()
    assert lib.bn_head_forward(None, X.data_ptr(), 64, 32, W.data_ptr(), b.data_ptr(), 5, 0, out.data_ptr(), stream) == -1
    h = ctypes.c_void_p()
    mk = lambda *a: lib.bn_probe_create(ctx.handle, *a, ctypes.byref(h), stream)   # noqa: E731
    assert mk(32, 5, 0, 3, 1e-3, 0.0, 1.0, 0.5, 1, 10, W.data_ptr(), b.data_ptr()) == -1 and "optimizer" in err()
    assert mk(32, 5, 0, 0, 1e-3, 0.0, 1.0, 1.0, 1, 10, W.data_ptr(), b.data_ptr()) == -1 and "dropout" in err()
    assert mk(32, 5, 0, 0, 1e-3, 0.0, 1.0, 0.5, 1, 0, W.data_ptr(), b.data_ptr()) == -1 and "total_steps" in err()
    assert mk(32, 5, 0, 0, 1e-3, 0.0, 1.0, 0.5, 1, 10, None, b.data_ptr()) == -1 and "null" in err()
    assert mk(4096, 5, 0, 0, 1e-3, 0.0, 1.0, 0.5, 1, 10, W.data_ptr(), b.data_ptr()) == -1 and not h.value
    assert mk(32, 5, 0, 0, 1e-3, 0.0, 1.0, 0.5, 1, 10, W.data_ptr(), b.data_ptr()) == 0 and h.value
    try:
        assert lib.bn_probe_epoch(h, X.data_ptr(), Y.data_ptr(), perm.data_ptr(), 64, 0, loss.data_ptr(), stream) == -1 and "batch" in err()
        assert lib.bn_probe_epoch(h, X.data_ptr(), Y.data_ptr(), perm.data_ptr(), 64, 65, loss.data_ptr(), stream) == -1
        assert lib.bn_probe_epoch(h, X.data_ptr(), None, perm.data_ptr(), 64, 16, loss.data_ptr(), stream) == -1 and "null" in err()
        assert lib.bn_probe_epoch(None, X.data_ptr(), Y.data_ptr(), perm.data_ptr(), 64, 16, loss.data_ptr(), stream) == -1
        assert lib.bn_probe_loss(h, X.data_ptr(), Y.data_ptr(), 0, loss.data_ptr(), stream) == -1
        assert lib.bn_probe_get(h, None, b.data_ptr(), stream) == -1 and lib.bn_probe_set(h, W.data_ptr(), None, stream) == -1
        # ... and the probe is still usable
        assert lib.bn_probe_epoch(h, X.data_ptr(), Y.data_ptr(), perm.data_ptr(), 64, 16, loss.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(loss[:4]).all()
    finally:
        lib.bn_probe_destroy(h)
    with pytest.raises(ValueError, match="width 32"):
        from birdnet_stm32.training.linear_probe import ProbeHead

        ProbeHead(W.cpu().numpy(), b.cpu().numpy()).predict(np.zeros((3, 31), np.float32), ctx)
    assert _hip.PROBE_MAX_D == 2048 and _hip.PROBE_MAX_C == 4096


# -- end to end -----------------------------------------------------------------------------------------------------------------------
SR = 24000
# class folder -> family of tools/signal_families.py (3 s chunks with random parameters); white noise is the negative folder
FAMILY_OF = {"harmonic_stack": 6, "sparse_impulses": 8, "brown_noise": 10, "chirp": 3, "noise": 2}
CLASSES = tuple(k for k in FAMILY_OF if k != "noise")


def _family_audio(torch, kind: str, n_chunks: int, g) -> np.ndarray:
    """``n_chunks`` chunks of the family, each peak-normalised (the families span four decades of level, PCM16 does not), end to end."""
    import importlib.util

    from conftest import REPO

    spec = importlib.util.spec_from_file_location("signal_families", os.path.join(REPO, "tools", "signal_families.py"))
    fam = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fam)
    x = fam.family_batch(torch, FAMILY_OF[kind], n_chunks, g, "cuda").cpu().numpy().astype(np.float64)
    return (0.9 * x / np.abs(x).max(axis=1, keepdims=True)).reshape(-1)


def _write_wav(path, x):
    pcm = np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(SR)
        w.writeframes(pcm.tobytes())


def test_probe_then_analyze_with_the_head(torch_mod, tmp_path):
    """Class folders of chunks from tools/signal_families.py -> probe -> analyze --head, against the float64 restatement on the same embeddings."""
    from birdnet_stm32.cli import analyze as analyze_cli
    from birdnet_stm32.cli import probe as probe_cli
    from birdnet_stm32.evaluation.detections import detect_files
    from birdnet_stm32.evaluation.embeddings import embed_files
    from birdnet_stm32.models.runners import load_model_runner
    from birdnet_stm32.training.linear_probe import ProbeHead, fit_probe_reference, head_scores, targets_from_paths

    torch = torch_mod
    g = torch.Generator(device="cuda").manual_seed(7)
    train_dir, held_dir = tmp_path / "train", tmp_path / "held"
    held = []
    for kind in CLASSES + ("noise",):
        for d in (train_dir, held_dir):
            os.makedirs(d / kind)
        for i in range(24):
            _write_wav(train_dir / kind / f"{i:02d}.wav", _family_audio(torch, kind, 2, g))
        for i in range(6):
            _write_wav(held_dir / kind / f"{i:02d}.wav", _family_audio(torch, kind, 1, g))
            held.append(str(held_dir / kind / f"{i:02d}.wav"))
    # a long file: 9 s spans (three chunks) of each class in turn with 6 s of noise in front of each; every border is a multiple of the
    # 3 s chunk, and 3 s are 72000 samples in and 66150 out, so the chunks of the analysis are the chunks placed here
    spans, parts, pos = [], [], 0.0
    for kind in CLASSES:
        parts += [_family_audio(torch, "noise", 2, g), _family_audio(torch, kind, 3, g)]
        spans.append((kind, pos + 6.0, pos + 15.0))
        pos += 15.0
    long_path = tmp_path / "long.wav"
    _write_wav(long_path, np.concatenate(parts))

    runner = load_model_runner(TFLITE_PATH, max_batch=64, prepare_pipeline=True)
    try:
        out = str(tmp_path / "myhead")
        head = probe_cli.main(["--model_path", TFLITE_PATH, "--model_config", CONFIG_PATH, "--data_path_train", str(train_dir), "--output", out,
                               "--epochs", "30", "--batch_size", "32", "--learning_rate", "0.01", "--seed", "3"], runner=runner)
        for suffix in (".npz", "_labels.txt", "_model_config.json", "_history.csv"):
            assert os.path.isfile(out + suffix), suffix
        loaded = ProbeHead.load(out + ".npz")
        assert loaded.class_names == sorted(CLASSES) and np.array_equal(loaded.W, head.W) and loaded.embedding_dim == runner.embedding_info()["dim"]
        classes = loaded.class_names

        # the same embeddings -> the float64 restatement, with the command's split and settings
        np.random.seed(3)
        from birdnet_stm32.data.dataset import load_file_paths_from_directory
        from birdnet_stm32.training.linear_probe import split_train_val

        paths, _ = load_file_paths_from_directory(str(train_dir))
        tr_paths, va_paths = split_train_val(paths, 0.2)
        emb = embed_files(runner, tr_paths + va_paths, max_duration=30, sample_rate=22050, chunk_duration=3.0)
        Y, keep = targets_from_paths(emb.paths, classes, emb.file_index, "sigmoid")
        is_tr = emb.file_index < len(tr_paths)
        ref = fit_probe_reference(emb.embeddings[is_tr], Y[is_tr], emb.embeddings[~is_tr], Y[~is_tr], epochs=30, batch_size=32, learning_rate=0.01, seed=3)

        def label(scores):   # per file: the best class, or "noise" below 0.5
            return [classes[int(np.argmax(s))] if s.max() >= 0.5 else "noise" for s in scores]

        he = embed_files(runner, held, max_duration=3, sample_rate=22050, chunk_duration=3.0)
        assert he.embeddings.shape[0] == len(held)
        truth = [os.path.basename(os.path.dirname(p)) for p in held]
        lab_ref = label(head_scores(he.embeddings.astype(np.float64), ref.history["W"], ref.history["b"], "sigmoid"))
        lab_dev = label(loaded.predict(he.embeddings, runner.ctx))
        acc = np.mean([a == b for a, b in zip(lab_ref, truth)])
        differ = sum(a != b for a, b in zip(lab_ref, lab_dev))
        print(f"held-out: restatement accuracy {acc:.3f}, device/restatement labels differ on {differ} of {len(held)} files")
        assert differ <= 1                      # (a)
        assert acc >= 0.9                       # (b) a condition on the inputs

        # analyze --head on the held-out files: the detections carry the head's classes and agree with predict()
        det = analyze_cli.main(["--model_path", TFLITE_PATH, "--model_config", CONFIG_PATH, "--head", out + ".npz", "--input", *held,
                                "--output", str(tmp_path / "held.csv"), "--min_conf", "0.5", "--top_k", "1"], runner=runner)
        got = {int(f): classes[int(c)] for f, c in zip(det.file_index, det.class_index)}
        assert [got.get(i, "noise") for i in range(len(held))] == lab_dev
        text = open(tmp_path / "held.csv").read()
        assert any(c in text for c in classes)

        # (c) the long file, streamed (a slab smaller than the file)
        det = detect_files(runner, [str(long_path)], min_conf=0.5, top_k=1, sample_rate=22050, chunk_duration=3.0, class_names=classes, head=loaded,
                           pipeline_options=dict(slab_bytes=1 << 20, stream_long=True), return_scores=True)
        assert det.scores.shape == (5 * len(CLASSES), len(classes)) and len(det) >= len(CLASSES)
        seen = set()
        for c, s0, s1 in zip(det.class_index, det.start_s, det.end_s):
            name = classes[int(c)]
            assert any(k == name and s0 >= a and s1 <= b for k, a, b in spans), f"{name} detected at {s0}-{s1} s, outside its span"
            seen.add(name)
        assert seen == set(CLASSES)

        # (d) head=None is the plain path
        a = detect_files(runner, held[:8], sample_rate=22050, chunk_duration=3.0, return_scores=True)
        b = detect_files(runner, held[:8], sample_rate=22050, chunk_duration=3.0, return_scores=True, head=None)
        assert np.array_equal(a.scores, b.scores) and np.array_equal(a.class_index, b.class_index) and np.array_equal(a.score, b.score)
        with pytest.raises(ValueError, match="width"):
            detect_files(runner, held[:2], head=ProbeHead(np.zeros((128, 3), np.float32), np.zeros(3, np.float32)))
    finally:
        runner.close()
