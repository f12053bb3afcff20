"""GPU tests of the quantisation-aware fine-tune of a probe head (csrc/bn_probe_step.h EXT = 2, the two weight kernels of csrc/bn_probe.hip,
``bn_probe_set_qat`` / ``bn_probe_get_quantized`` / ``bn_probe_scores``, training/probe_qat.py): the fake-quantised weights bit for bit, one
SGD step against float64 on an exact lattice and from a trained head, the loss of the fake-quantised forward, determinism, refused calls
and ``probe --export_tflite --qat_epochs`` end to end.

The many-step trajectory of a QAT fit is not compared with the float64 restatement: a single logit that rounds the other way moves it by
a whole step of the grid, and no margin for that can be derived.  The one-step and forward-only tests cover the arithmetic instead."""
from __future__ import annotations

import ctypes
import json
import os

import numpy as np
import pytest

import i8_variants as iv
from conftest import CONFIG_PATH, TFLITE_PATH
from test_gpu_head_export import _tone_file
from test_gpu_probe import U, _clusters

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; the product has no CPU path to fall back to")
    return torch


@pytest.fixture(scope="module")
def ctx(torch_mod):
    from birdnet_stm32 import _hip

    c = _hip.Context(0, 1)
    yield c
    c.close()


def _backend(ctx, head, X, Y, per_tensor=False, quantize_logits=True, logit_range=(-1.0, 1.0), Xv=None, Yv=None, **fit_kw):
    """A probe holding ``head`` with QAT set (training/probe_qat.py's own backend)."""
    from birdnet_stm32.conversion.quantize import choose_activation_params
    from birdnet_stm32.training import probe_qat as pq

    kw = dict(optimizer="sgd", batch_size=len(X), dropout=0.0, epochs=1, learning_rate=1.0, clipnorm=0.0)
    kw.update(fit_kw)
    plan = pq._plan_qat(X, Y, Xv, head, True, kw)
    return pq._QatDeviceBackend(ctx, X, Y, Xv, Yv, plan, per_tensor, quantize_logits, *choose_activation_params(*logit_range)), plan


# -- the weights ------------------------------------------------------------------------------------------------------------------------
def _weights_with_edges(D, C, seed):
    """Every class's largest weight is 1.0 (row 0), so one step is 1 / 127 per class and per tensor alike; 0.5 (row 1) is 63.5 steps, a tie;
    the last class of two or more is all zero: the 5e-7 floor per class."""
    W = np.clip(np.random.default_rng([seed, D, C]).normal(0.0, 0.3, (D, C)), -0.9, 0.9).astype(np.float32)
    W[0] = 1.0
    if D > 1:
        W[1, ::2] = 0.5
        W[1, 1::2] = -0.5
    if C > 1:
        W[:, -1] = 0.0
    return W


WEIGHT_SHAPES = [(D, C) for D in (1, 3, 255, 256, 2048) for C in (1, 15, 16, 17, 100, 129)] + [(2048, 4096)]


@pytest.mark.parametrize("per_tensor", [False, True], ids=["per_class", "per_tensor"])
def test_fake_quantized_weights_bit_for_bit(torch_mod, ctx, per_tensor):
    """``bn_probe_get_quantized`` against ``q * s_w`` of ``quantize_weights``: every D at which the row slices of the first kernel and the
    row chunks of the second end differently, C below, at and above a wave and two waves of columns, and the largest head."""
    from birdnet_stm32.training.linear_probe import ProbeHead
    from birdnet_stm32.training.probe_qat import fake_quantize_head_weights

    for D, C in WEIGHT_SHAPES:
        W = _weights_with_edges(D, C, seed=7)
        b = np.random.default_rng(C).normal(0.0, 1.0, C).astype(np.float32)
        be, _ = _backend(ctx, ProbeHead(W, b), np.zeros((1, D), np.float32), np.zeros((1, C), np.float32), per_tensor=per_tensor, quantize_logits=False)
        try:
            got = be.quantized().cpu().numpy()
            W_back, b_back = (t.cpu().numpy() for t in be.get())
        finally:
            be.close()
        want = fake_quantize_head_weights(W, per_tensor)
        bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        assert bad == 0, f"D={D} C={C}: {bad} of {want.size} weights differ"
        assert np.array_equal(W_back, W) and np.array_equal(b_back, b)   # the shadow parameters are untouched
        if D > 1:   # the tie: 63.5 steps round to 64, the even one
            assert got[1, 0] == np.float32(64) * np.float32(1.0 / 127.0)
        if C > 1:    # the zero class
            assert not got[:, -1].any() and not np.signbit(got[:, -1]).any()


# -- one step on an exact lattice -------------------------------------------------------------------------------------------------------
def _lattice(D, C, B, activation, seed):
    """X in multiples of 2^-4, W = k 2^-10 with |k| <= 127 and +127 in every class (row 0), b in multiples of 2^-14: every product is a
    multiple of 2^-14 and every partial sum stays below 2^10, so a logit is exact in float32 in any order, and W_q = W (one step is
    exactly 2^-10).  Row 0 of X is 8 at feature 0 and 0 elsewhere, row 1 its negative: their logits are +-127/128 + b in every class, outside
    the range the grid is given, so all their codes clamp (high and low); the other rows stay small and mostly inside."""
    rng = np.random.default_rng([seed, D, C, B])
    X = rng.integers(-4, 5, (B, D)).astype(np.float32) / np.float32(16.0)
    X[0], X[1 % B] = 0.0, 0.0
    X[0, 0] = 8.0
    if B > 1:
        X[1, 0] = -8.0
    W = rng.integers(-127, 128, (D, C)).astype(np.float32) / np.float32(1024.0)
    W[0] = np.float32(127.0 / 1024.0)
    b = rng.integers(-1024, 1025, C).astype(np.float32) / np.float32(16384.0)
    lab = rng.integers(0, C, B)
    Y = np.eye(C, dtype=np.float32)[lab]
    if activation == "sigmoid":
        Y[::7] = 0.0
    return X, Y, W, b


def _act64(z, activation):
    if activation == "softmax":
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)
    return 1.0 / (1.0 + np.exp(-z))


def _step_check(head0, head1, X, Y, zq32, ok, extra_G, what):
    """``W0 - W1`` of one SGD step at lr 1 against ``Xa^T G`` in float64, with the bound of test_one_sgd_step_is_the_gradient for logits
    that are known exactly (``zq32``, the float32 the device computes too: dz = 0), plus ``extra_G``, what an element's G may be off by for
    another reason."""
    B, C = Y.shape
    act = head0.activation
    P = _act64(zq32.astype(np.float64), act)
    dP = P * 40 * U if act == "softmax" else 4 * U * P
    scale = B if act == "softmax" else B * C
    G = (P - Y) * ok / scale
    dG = (dP + 2 * U * np.abs(P - Y)) * ok / scale + extra_G
    Xa = np.concatenate([X.astype(np.float64), np.ones((B, 1))], axis=1)
    got = np.concatenate([head0.W.astype(np.float64) - head1.W, (head0.b.astype(np.float64) - head1.b)[None, :]])
    want = Xa.T @ G
    bound = np.abs(Xa).T @ dG + (B + 2) * U * (np.abs(Xa).T @ np.abs(G)) + U * np.abs(np.concatenate([head1.W, head1.b[None, :]]))
    err = np.abs(got - want)
    print(f"{what}: max err {err.max():.3e}, max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, |g| max {np.abs(want).max():.3e}, "
          f"{int((~ok).sum())} of {ok.size} codes clamped")
    assert np.all(err <= bound)
    return P


@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
@pytest.mark.parametrize("D,C,B", [(96, 7, 5), (255, 13, 33), (256, 100, 32)])
def test_one_sgd_step_on_an_exact_lattice(torch_mod, ctx, activation, D, C, B):
    from birdnet_stm32.conversion.quantize import choose_activation_params
    from birdnet_stm32.training.linear_probe import ProbeHead, probe_loss
    from birdnet_stm32.training.probe_qat import fake_quantize_head_weights, fake_quantize_logits, fit_probe_qat, qat_logit_codes

    X, Y, W, b = _lattice(D, C, B, activation, seed=5)
    head0 = ProbeHead(W, b, activation)
    assert np.array_equal(fake_quantize_head_weights(W), W)
    z = (X.astype(np.float64) @ W.astype(np.float64) + b).astype(np.float32)
    assert np.array_equal(z.astype(np.float64), X.astype(np.float64) @ W.astype(np.float64) + b)   # exact
    rng = (-0.45, 0.6)
    s_out, z_out = choose_activation_params(*rng)
    zq, codes, ok = fake_quantize_logits(z, s_out, z_out)
    assert not ok[0].any() and (codes[0] == 127).all() and (B == 1 or (not ok[1].any() and (codes[1] == -128).all())) and ok[2:].mean() > 0.5

    got_codes = qat_logit_codes(ctx, head0, X, rng)
    assert got_codes.dtype == np.int8 and np.array_equal(got_codes, codes)

    kw = dict(head=head0, logit_range=rng, epochs=1, batch_size=B, learning_rate=1.0, optimizer="sgd", clipnorm=0.0, dropout=0.0, seed=9)
    head1 = fit_probe_qat(ctx, X, Y, **kw)
    P = _step_check(head0, head1, X, Y, zq, ok, 0.0, f"lattice {activation} D={D} C={C} B={B}")
    loss64 = float(probe_loss(P, Y.astype(np.float64), activation))
    assert abs(head1.history["step_loss"][0] - loss64) <= 1e-5 * max(1.0, abs(loss64))
    # a row whose codes all clamp contributes exactly nothing: other targets for it, the same weights bit for bit
    Y2 = Y.copy()
    Y2[0] = np.roll(Y[0], 1) if activation == "softmax" else 1.0 - Y[0]
    assert not np.array_equal(Y2[0], Y[0])
    head2 = fit_probe_qat(ctx, X, Y2, **kw)
    assert np.array_equal(head2.W, head1.W) and np.array_equal(head2.b, head1.b)
    if activation == "sigmoid":   # (the loss does see the row; a softmax row of equal codes is uniform, whatever its target)
        assert head2.history["step_loss"][0] != head1.history["step_loss"][0]


# -- one step from a trained head -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
@pytest.mark.parametrize("D,C,B", [(255, 13, 33), (256, 100, 32)])
def test_one_sgd_step_from_a_trained_head(torch_mod, ctx, activation, D, C, B):
    """Off the lattice the float32 logit is within dz = (D + 2) u (|x| |W_q| + |b|) of the float64 one (_prob_bound's bound), so the code is
    the float64 one unless z / s_out lies within dz / s_out (plus the division's own rounding) of a rounding boundary.  Such an element
    may have the other code: its quantised logit is off by s_out, its probability by at most s_out / 4 (no derivative of the sigmoid or of
    a softmax output by a logit exceeds 1/4), so G by s_out / (4 scale) — for softmax in every column of that row, since every output of
    the row moves.  Where the two candidates straddle a clamp (127 | 128 or -129 | -128) the logit is the same and the mask flips: G is
    off by at most 1 / scale.  Each goes into the bound times |x_b|; no element is left out."""
    from birdnet_stm32.conversion.quantize import choose_activation_params
    from birdnet_stm32.training.linear_probe import fit_probe
    from birdnet_stm32.training.probe_qat import fake_quantize_head_weights, fit_probe_qat

    Xt, Yt, _ = _clusters(600, D, C, seed=4, multi_hot=activation == "sigmoid")
    Xt *= 0.25
    head0 = fit_probe(ctx, Xt, Yt, activation=activation, epochs=3, batch_size=32, learning_rate=1e-2, dropout=0.0, seed=2)
    X, Y = Xt[:B], Yt[:B]
    Wq = fake_quantize_head_weights(head0.W).astype(np.float64)
    X64, b64 = X.astype(np.float64), head0.b.astype(np.float64)
    z = X64 @ Wq + b64
    dz = (D + 2) * U * (np.abs(X64) @ np.abs(Wq) + np.abs(b64))
    rng = (float(np.quantile(z, 0.02)), float(np.quantile(z, 0.98)))   # narrower than the logits: codes clamp
    s_out, z_out = choose_activation_params(*rng)
    t = z / np.float64(np.float32(s_out))
    k = np.rint(t) + z_out
    kc = np.clip(k, -128, 127)
    ok = k == kc
    zq32 = ((kc.astype(np.float32) - np.float32(z_out)) * np.float32(s_out)).astype(np.float32)
    near = np.abs(t - np.floor(t) - 0.5) <= dz / s_out + 2 * U * (np.abs(t) + 1)
    lo_code = np.floor(t) + z_out                                   # the candidates are lo_code and lo_code + 1
    at_clamp = near & ((lo_code == 127) | (lo_code == -129))
    inside = near & (lo_code >= -128) & (lo_code <= 126)
    scale = B if activation == "softmax" else B * C
    extra = at_clamp / scale + (inside.sum(axis=1, keepdims=True) * np.ones((1, C)) if activation == "softmax" else inside) * (s_out / (4 * scale))
    head1 = fit_probe_qat(ctx, X, Y, head=head0, logit_range=rng, epochs=1, batch_size=B, learning_rate=1.0, optimizer="sgd", clipnorm=0.0, dropout=0.0,
                          seed=9)
    print(f"{int(near.sum())} of {near.size} logits next to a rounding boundary, {int(at_clamp.sum())} of them at a clamp; s_out {s_out:.4g}")
    assert (~ok).any()
    _step_check(head0, head1, X, Y, zq32, ok, extra, f"trained {activation} D={D} C={C} B={B}")


# -- the forward alone, determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
def test_loss_of_the_fake_quantised_forward(torch_mod, ctx, activation):
    """``bn_probe_loss`` in QAT mode after 3 epochs against the float64 loss of the fake-quantised forward of the device's own final
    weights: the float tolerance of the plain fit's loss test, plus for every logit next to a rounding boundary (counted as above) what
    the other code moves the mean by: |dloss/dz| <= 1 per element, so s_out / (n C) (sigmoid) or s_out / n (softmax: the mean is over rows)."""
    from birdnet_stm32.conversion.quantize import choose_activation_params
    from birdnet_stm32.training.linear_probe import ProbeHead, epoch_permutation, fit_probe, probe_loss
    from birdnet_stm32.training.probe_qat import fake_quantize_head_weights

    D, C, n = 256, 40, 2000
    X, Y, _ = _clusters(n, D, C, seed=8)
    Xv, Yv, _ = _clusters(300, D, C, seed=9)
    head0 = fit_probe(ctx, X, Y, activation=activation, epochs=1, batch_size=96, seed=11)
    z0 = X.astype(np.float64) @ head0.W + head0.b
    rng = (float(z0.min()), float(z0.max()))
    s_out, z_out = choose_activation_params(*rng)
    be, plan = _backend(ctx, head0, X, Y, logit_range=rng, Xv=Xv, Yv=Yv, optimizer="adam", batch_size=96, dropout=0.5, epochs=3, learning_rate=1e-3,
                        clipnorm=1.0, seed=11)
    try:
        for epoch in range(3):
            be.epoch(epoch_permutation(11, epoch, n))
        got = be.val_loss()
        W, b = (t.cpu().numpy() for t in be.get())
        Wq_dev = be.quantized().cpu().numpy()
    finally:
        be.close()
    Wq = fake_quantize_head_weights(W)
    assert np.array_equal(Wq_dev, Wq) and not np.array_equal(W, head0.W)
    Xv64 = Xv.astype(np.float64)
    z = Xv64 @ Wq.astype(np.float64) + b
    dz = (D + 2) * U * (np.abs(Xv64) @ np.abs(Wq).astype(np.float64) + np.abs(b))
    t = z / np.float64(np.float32(s_out))
    kc = np.clip(np.rint(t) + z_out, -128, 127)
    zq = ((kc.astype(np.float32) - np.float32(z_out)) * np.float32(s_out)).astype(np.float64)
    lo_code = np.floor(t) + z_out
    near = (np.abs(t - np.floor(t) - 0.5) <= dz / s_out + 2 * U * (np.abs(t) + 1)) & (lo_code >= -128) & (lo_code <= 126)
    want = float(probe_loss(_act64(zq, activation), Yv.astype(np.float64), activation))
    tol = 1e-5 * max(1.0, abs(want)) + int(near.sum()) * s_out / (len(Xv) if activation == "softmax" else len(Xv) * C)
    print(f"{activation}: QAT loss {got:.7f} vs float64 {want:.7f} (|diff| {abs(got - want):.2e}, tolerance {tol:.2e}, {int(near.sum())} boundary logits)")
    assert abs(got - want) <= tol
    assert ProbeHead(W, b, activation).num_classes == C


def test_same_seed_same_bits_and_the_loss_falls(torch_mod, ctx):
    from birdnet_stm32.training.linear_probe import fit_probe
    from birdnet_stm32.training.probe_qat import fit_probe_qat

    X, Y, _ = _clusters(2000, 256, 40, seed=8)
    Xv, Yv, _ = _clusters(300, 256, 40, seed=9)
    head0 = fit_probe(ctx, X, Y, epochs=1, batch_size=96, seed=11)
    z0 = X.astype(np.float64) @ head0.W + head0.b
    kw = dict(head=head0, logit_range=(float(z0.min()), float(z0.max())), epochs=3, batch_size=96, learning_rate=1e-3, seed=11)
    a = fit_probe_qat(ctx, X, Y, Xv, Yv, **kw)
    b = fit_probe_qat(ctx, torch_mod.from_numpy(X).cuda(), torch_mod.from_numpy(Y).cuda(), Xv, Yv, **kw)
    c = fit_probe_qat(ctx, X, Y, Xv, Yv, **{**kw, "per_tensor": True})
    assert np.array_equal(a.W, b.W) and np.array_equal(a.b, b.b)
    assert np.array_equal(a.history["step_loss"], b.history["step_loss"]) and a.history["val_loss"] == b.history["val_loss"]
    assert not np.array_equal(a.W, c.W) and c.history["qat"]["per_tensor"] and not a.history["qat"]["per_tensor"]
    print("QAT loss per epoch", [round(v, 5) for v in a.history["loss"]], "val", [round(v, 5) for v in a.history["val_loss"]])
    assert a.history["loss"][-1] < a.history["loss"][0] and len(a.history["loss"]) == 3 == a.history["qat"]["epochs"]


# -- refused calls ----------------------------------------------------------------------------------------------------------------------
def test_set_qat_refuses_bad_arguments_and_changes_nothing(torch_mod, ctx):
    from birdnet_stm32.training import linear_probe as lp

    torch, lib = torch_mod, ctx.lib
    X, Y, _ = _clusters(200, 64, 6, seed=1)
    plan = lp._plan_fit(X, Y, None, device=True, activation="sigmoid", optimizer="adam", batch_size=32, dropout=0.5, epochs=1, seed=5)
    touched, plain = lp._DeviceBackend(ctx, X, Y, None, None, plan), lp._DeviceBackend(ctx, X, Y, None, None, plan)

    def err():
        return lib.bn_last_error().decode()

    try:
        h = touched.handle
        assert lib.bn_probe_set_qat(None, 1, 1, 0.05, 0) == -1 and "null probe" in err()
        assert lib.bn_probe_set_qat(h, 3, 0, 0.05, 0) == -1 and "weight mode 3" in err()
        assert lib.bn_probe_set_qat(h, -1, 0, 0.05, 0) == -1
        for s_out in (0.0, -0.05, float("nan"), float("inf")):
            assert lib.bn_probe_set_qat(h, 1, 1, s_out, 0) == -1 and "logit scale" in err(), s_out
        for z_out in (128, -129):
            assert lib.bn_probe_set_qat(h, 1, 1, 0.05, z_out) == -1 and "zero point" in err(), z_out
        assert lib.bn_probe_set_qat(h, 0, 0, float("nan"), 999) == 0   # (without quantize_logits the grid is not looked at)
        out, codes = torch.empty((200, 6), device="cuda"), torch.empty((200, 6), dtype=torch.int8, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.bn_probe_scores(h, touched.X.data_ptr(), 200, out.data_ptr(), codes.data_ptr(), stream) == -1 and "d_codes" in err()
        assert lib.bn_probe_scores(h, None, 200, out.data_ptr(), None, stream) == -1 and "null" in err()
        assert lib.bn_probe_scores(h, touched.X.data_ptr(), 0, out.data_ptr(), None, stream) == -1 and "row count" in err()
        assert lib.bn_probe_get_quantized(h, None, stream) == -1 and "null" in err()
        assert lib.bn_probe_scores(h, touched.X.data_ptr(), 200, out.data_ptr(), None, stream) == 0   # QAT off: the plain scores
        W0, b0 = touched.get()
        assert torch.equal(out, lp.ProbeHead(W0.cpu().numpy(), b0.cpu().numpy()).predict(touched.X, ctx))
        perm = lp.epoch_permutation(5, 0, 200)
        la, lb = touched.epoch(perm), plain.epoch(perm)
        assert np.array_equal(la, lb)
        for u, v in zip(touched.get(), plain.get()):
            assert torch.equal(u, v)
    finally:
        touched.close()
        plain.close()


# -- end to end -------------------------------------------------------------------------------------------------------------------------
def test_probe_export_with_qat_epochs(torch_mod, tmp_path):
    from birdnet_stm32.cli import probe as probe_cli
    from birdnet_stm32.conversion.head_export import find_classifier, quantize_head
    from birdnet_stm32.conversion.quantize import choose_activation_params
    from birdnet_stm32.models._tflite_reader import load_tflite
    from birdnet_stm32.models.runners import load_model_runner
    from birdnet_stm32.training.linear_probe import ProbeHead

    data = tmp_path / "data"
    for kind, f0 in (("high_tone", 2800.0), ("low_tone", 500.0)):
        os.makedirs(data / kind)
        for i in range(8):
            _tone_file(data / kind / f"{i:02d}.wav", f0, seed=int(f0) + i)
    out = str(tmp_path / "tones")
    S = iv.inputs()
    runner = load_model_runner(TFLITE_PATH, max_batch=64, prepare_pipeline=True)
    try:
        probe_cli.main(["--model_path", TFLITE_PATH, "--model_config", CONFIG_PATH, "--data_path_train", str(data), "--output", out, "--epochs", "3",
                        "--learning_rate", "0.01", "--export_tflite", "--qat_epochs", "2"], runner=runner)
        info = runner.embedding_info()
        rows = runner.embed(S.reshape(iv.N_INPUTS, -1), dtype="int8")
    finally:
        runner.close()
    rep = json.load(open(out + "_export.json"))
    qat = rep["qat"]
    print(json.dumps(qat))
    print(f"code_agreement {qat['code_agreement']:.4f}")
    assert qat["epochs"] == 2 and qat["kept"] in ("float", "qat") and 0.0 <= qat["code_agreement"] <= 1.0
    assert qat["kept"] == ("qat" if qat["qat"]["loss_int8"] < qat["float"]["loss_int8"] else "float")
    assert np.isfinite([qat[k][m] for k in ("float", "qat") for m in ("loss_int8", "loss_float", "cosine_mean")]).all()
    assert rep["loss_int8"] == qat[qat["kept"]]["loss_int8"] and rep["cosine_mean"] >= 0.95   # the report and the gate are the written head's
    # the file's logit parameters are the ones trained against
    trained = choose_activation_params(*qat["logit_range"])
    assert (qat["logit_scale"], qat["logit_zero_point"]) == trained and rep["logit_range"] == qat["logit_range"]
    written = load_tflite(out + ".tflite")
    logit = written.tensors[written.ops[find_classifier(written)["fc"]].outputs[0]]
    assert (float(logit.scale[0]), int(logit.zero_point[0])) == trained == (rep["logit_scale"], rep["logit_zero_point"])
    # the written file is the saved head, quantised with that range
    qh = quantize_head(ProbeHead.load(out + ".npz"), info["scale"], info["zero_point"], *qat["logit_range"])
    exported = load_model_runner(out + ".tflite", max_batch=iv.N_INPUTS)
    try:
        assert exported.num_classes == 2
        got = exported.predict(S.reshape(iv.N_INPUTS, -1))
        own = qh.predict_device(torch_mod.from_numpy(rows).cuda(), exported.ctx).cpu().numpy()
        qh.close()
    finally:
        exported.close()
    assert np.array_equal(got, own)
