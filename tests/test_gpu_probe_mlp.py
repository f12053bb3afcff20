"""GPU tests of the probe's hidden layer (csrc/bn_probe_mlp.hip, bn_probe_mlp_*, bn_head_mlp_forward): one step against the float64
specification under a derived float32 bound, many steps against the float64 restatement, row groups, determinism, scoring, the loss
options, refused calls, and probe --hidden_units -> analyze --head end to end."""

import ctypes
import os
import wave
from dataclasses import replace

import numpy as np
import pytest

from conftest import CONFIG_PATH, TFLITE_PATH

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
        Y[::7] = 0.0
        Y[np.arange(3, n, 11), rng.integers(0, C, len(range(3, n, 11)))] = 1.0
    return X, Y, lab


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def _vec(h, hist=False):
    """The four arrays of a head as one float64 vector, in the order of the parameter vector."""
    src = h.history if hist else {"W1": h.W1, "b1": h.b1, "W": h.W, "b": h.b}
    return np.concatenate([np.asarray(src[k], np.float64).ravel() for k in ("W1", "b1", "W", "b")])


def _prob_bound(z, dz, activation):
    """Float64 probabilities of logits z and the bound on the float32 device error of P when the device's logits are within dz of z
    (tests/test_gpu_probe.py: _prob_bound).  Sigmoid 1 / (1 + expf(-z)): expf within 1 ulp, the addition and the IEEE division half an
    ulp each, d sigma / dz <= 1/4: |dP| <= dz / 4 + 4 u P.  Softmax expf(z - m) / sum: the subtraction, expf, the division and a sum of C
    terms added as at most 8 + 4 + 16 partial sums: |dP| <= P (2 max_row dz + 40 u)."""
    if activation == "softmax":
        e = np.exp(z - z.max(axis=1, keepdims=True))
        P = e / e.sum(axis=1, keepdims=True)
        return P, P * (2 * dz.max(axis=1, keepdims=True) + 40 * U)
    P = 1.0 / (1.0 + np.exp(-z))
    return P, dz / 4 + 4 * U * P


def _forward_bound(xd, W1, b1, m2, W2, b2, activation):
    """The forward in float64 with, per element, a bound on the float32 device error; all inputs exact float32 values as float64.
    A length-K dot product accumulated in float32 (v_mfma_f32_16x16x4_f32 is an fmaf chain; any order) plus the bias add:
    |err| <= (K + 2) u (|x| |W| + |b|).  ReLU is 1-Lipschitz, so the error of relu(a) is that of a whatever the gate does; drop2's scale is
    a power of two here (asserted by the caller), so hd = relu(a) m2 carries da m2 and no rounding of its own."""
    D, H = W1.shape
    a = xd @ W1 + b1
    da = (D + 2) * U * (np.abs(xd) @ np.abs(W1) + np.abs(b1))
    hd, dhd = np.maximum(a, 0) * m2, da * m2
    z = hd @ W2 + b2
    dz = (H + 2) * U * ((np.abs(hd) + dhd) @ np.abs(W2) + np.abs(b2)) + dhd @ np.abs(W2)
    P, dP = _prob_bound(z, dz, activation)
    return a, da, hd, dhd, P, dP


def _device_step(lp, ctx, X, Y, W1, b1, W2, b2, activation, dropout, seed):
    """One SGD step with lr = 1 (momentum starts at zero), no clip, over all rows in order, from the given parameters: what the device
    returns is the parameters minus the gradient.  Returns (W1, b1, W2, b2 after the step, the step's loss)."""
    B, D = X.shape
    plan = lp._plan_fit(X, Y, None, device=True, activation=activation, optimizer="sgd", batch_size=B, dropout=dropout, epochs=1, learning_rate=1.0,
                        weight_decay=0.0, clipnorm=0.0, seed=seed, hidden_units=W1.shape[1])
    be = lp._MlpDeviceBackend(ctx, X, Y, None, None, replace(plan, W1_0=W1, b1_0=b1, W0=W2, b0=b2))
    try:
        losses = be.epoch(np.arange(B, dtype=np.int32))
        return tuple(t.cpu().numpy() for t in be.get()), float(losses[0])
    finally:
        be.close()


SHAPES = [(96, 24, 7, 5), (255, 100, 13, 33), (256, 64, 12, 32), (320, 512, 100, 256), (64, 2048, 5, 16), (2048, 1024, 100, 64)]


@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
@pytest.mark.parametrize("D,H,C,B", SHAPES)
def test_one_sgd_step_is_the_gradient(torch_mod, ctx, activation, D, H, C, B):
    """P0 - P1 of one SGD step (lr 1, no clip, dropout 0.5 on both layers) is the gradient, compared element by element with the float64
    specification (mlp_loss_and_gradient) under a float32 bound propagated through the step:

    * forward: _forward_bound (K = D for a, K = H for the logits), then the activation (_prob_bound);
    * G = (P - Y) / scale: dG = (dP + 2 u |P - Y|) / scale (the subtraction and the scaling);
    * dW2 = [hd, 1]^T G, K = B: (B + 2) u |hd^|^T |G^| + |hd^|^T dG + dhd^T |G|, hats the largest device values (|hd| + dhd, |G| + dG);
    * G W2^T, K = C: dGW = (C + 2) u |G^| |W2|^T + dG |W2|^T; dA = (G W2^T) m2 [a > 0] with m2's scale a power of two;
    * an element of a whose float64 value lies within its own bound da of zero is undecided: the device may gate it either way, so
      its dA is within |G W2^T| m2 + dGW m2 of the reference's.  That widens dW1 by |xd|^T of it; dW2 needs nothing more, because the
      error of relu(a) is at most da on either side of the gate, which dhd^T |G| already holds.  Nothing is excluded;
    * dW1 = xd^T dA, K = B: (B + 2) u |xd|^T |dA^| + |xd|^T ddA;
    * one rounding of the stored parameter P1 = fl(P0 - g): u |P1|.

    Conditions on the reference alone: at most 1 % of the B H elements of a are undecided (0.23 % at most was measured on the CPU for N(0, 1)
    rows, Glorot W1, small b1, dropout 0.5 and seeds 1-3, at D = 2048, H = 1024); and the float64 gradient without the ReLU gate violates
    the bound, so the bound can tell a wrong gate from rounding."""
    from birdnet_stm32.training import linear_probe as lp

    seed, p = 7, 0.5
    rng = np.random.default_rng(100 + D + H)
    X = rng.standard_normal((B, D)).astype(np.float32)
    lab = rng.integers(0, C, B)
    Y = np.eye(C, dtype=np.float32)[lab]
    if activation == "sigmoid":
        Y[::7] = 0.0
        Y[np.arange(B), rng.integers(0, C, B)] = 1.0
    W1, _, W2, _ = lp.init_mlp_head(D, H, C, seed)
    b1, b2 = (0.05 * rng.standard_normal(H)).astype(np.float32), (0.05 * rng.standard_normal(C)).astype(np.float32)
    (W1n, b1n, W2n, b2n), loss_dev = _device_step(lp, ctx, X, Y, W1, b1, W2, b2, activation, p, seed)
    P0 = np.concatenate([W1.ravel(), b1, W2.ravel(), b2]).astype(np.float64)
    P1 = np.concatenate([W1n.ravel(), b1n, W2n.ravel(), b2n]).astype(np.float64)
    got = P0 - P1

    m1, m2 = lp.dropout_mask(seed, 0, B, D, p, np.float64), lp.dropout_mask(seed ^ lp.DROP2_SEED_XOR, 0, B, H, p, np.float64)
    assert set(np.unique(m1)) <= {0.0, 2.0} and set(np.unique(m2)) <= {0.0, 2.0}   # the scale is a power of two: x m is exact
    xd = np.concatenate([X.astype(np.float64) * m1, np.ones((B, 1))], axis=1)
    Y64, W1_, b1_, W2_, b2_ = (v.astype(np.float64) for v in (Y, W1, b1, W2, b2))
    loss64, want, parts = lp.mlp_loss_and_gradient(P0, xd, m2, Y64, activation)
    a, da, hd, dhd, P, dP = _forward_bound(xd[:, :D], W1_, b1_, m2, W2_, b2_, activation)
    assert np.array_equal(a, parts["a"]) and np.array_equal(P, parts["P"])
    scale = B if activation == "softmax" else B * C
    G, GW = parts["G"], parts["GW"]
    dG = (dP + 2 * U * np.abs(P - Y64)) / scale
    Gh = np.abs(G) + dG
    hd1, dhd1 = np.concatenate([np.abs(hd) + dhd, np.ones((B, 1))], axis=1), np.concatenate([dhd, np.zeros((B, 1))], axis=1)
    bound2 = (B + 2) * U * (hd1.T @ Gh) + hd1.T @ dG + dhd1.T @ np.abs(G)
    dGW = (C + 2) * U * (Gh @ np.abs(W2_).T) + dG @ np.abs(W2_).T
    undecided = np.abs(a) <= da
    on = (a > da) | undecided                                    # the device's gate may be open
    ddA = m2 * (dGW * on + np.abs(GW) * undecided)
    dAh = np.abs(parts["dA"]) + ddA
    bound1 = (B + 2) * U * (np.abs(xd).T @ dAh) + np.abs(xd).T @ ddA
    bound = np.concatenate([bound1.ravel(), bound2.ravel()]) + U * np.abs(P1)
    err = np.abs(got - want)
    share = float(undecided.mean())
    _, open_gate, _ = lp.mlp_loss_and_gradient(P0, xd, m2, Y64, activation, relu_gate=False)
    beyond = int((np.abs(open_gate - want) > bound).sum())
    E1 = (D + 1) * H
    print(f"{activation} D={D} H={H} C={C} B={B}: max err {err.max():.3e}, max err/bound {np.max(err / bound):.3f} (layer 1 {np.max(err[:E1] / bound[:E1]):.3f}, "
          f"layer 2 {np.max(err[E1:] / bound[E1:]):.3f}), |g| max {np.abs(want).max():.3e}, undecided {int(undecided.sum())} of {B * H} "
          f"({100 * share:.3f} %), open-gate gradient beyond the bound in {beyond} elements")
    assert share <= 0.01                # a condition on the inputs
    assert beyond > 0                   # ... and on the bound: a wrong gate is no rounding
    assert np.all(err <= bound)
    # the loss: d loss / d z = G, the element losses carry a few roundings of their own (logf within 1 ulp, two products, one sum), and
    # the B C (or B) of them are added in float32 in some order
    dz = (H + 2) * U * ((np.abs(hd) + dhd) @ np.abs(W2_) + np.abs(b2_)) + dhd @ np.abs(W2_)
    n_sum = B * C
    loss_bound = float((np.abs(G) * dz).sum()) * 1.01 + (n_sum + 8) * U * abs(loss64)
    print(f"    loss {loss_dev:.7f} vs {loss64:.7f}: err {abs(loss_dev - loss64):.3e}, bound {loss_bound:.3e}")
    assert abs(loss_dev - loss64) <= loss_bound + U * abs(loss64)


@pytest.fixture(scope="module")
def long_fit_rows():
    return _clusters(4099, 256, 12, seed=3)


@pytest.mark.parametrize("optimizer,activation", [("adam", "sigmoid"), ("adamw", "sigmoid"), ("sgd", "sigmoid"), ("adam", "softmax")])
def test_many_steps_track_the_float64_restatement(torch_mod, ctx, long_fit_rows, optimizer, activation):
    """4 epochs of batch 32 over 4099 rows (a short last batch), D = 256, H = 64, dropout 0.5, clip 1.  d32 = distance of the float32
    restatement from the float64 one over all four arrays, measured here; the device (float32 too, another summation order) must be
    within 8 d32 of float64, weights and step losses."""
    from birdnet_stm32.training.linear_probe import fit_probe, fit_probe_reference

    X, Y, _ = long_fit_rows
    kw = dict(activation=activation, epochs=4, batch_size=32, learning_rate=1e-3, optimizer=optimizer, weight_decay=1e-2 if optimizer == "adamw" else 0.0,
              clipnorm=1.0, dropout=0.5, seed=42, hidden_units=64)
    r64 = fit_probe_reference(X, Y, dtype=np.float64, **kw)
    r32 = fit_probe_reference(X, Y, dtype=np.float32, **kw)
    dev = fit_probe(ctx, X, Y, **kw)
    assert dev.W1.shape == (256, 64) and dev.W.shape == (64, 12) and dev.hidden_units == 64
    P64 = _vec(r64, hist=True)
    d32, dd = _rel(_vec(r32, hist=True), P64), _rel(_vec(dev), P64)
    l32, ld = _rel(r32.history["step_loss"], r64.history["step_loss"]), _rel(dev.history["step_loss"], r64.history["step_loss"])
    print(f"{optimizer} {activation}: weights d32 {d32:.3e} device {dd:.3e} (ratio {dd / d32:.2f}); step losses d32 {l32:.3e} device {ld:.3e} "
          f"(ratio {ld / l32:.2f}); loss {dev.history['loss'][0]:.4f} -> {dev.history['loss'][-1]:.4f}")
    assert dev.history["loss"][-1] < 0.7 * dev.history["loss"][0]
    assert dd <= 8 * d32
    assert ld <= 8 * l32


def test_row_groups_and_a_short_last_batch(torch_mod, ctx):
    """Batch 4096 with a last batch of 1632 rows, H = 64: both gradient launches split the batch into row groups (69 for the full batch,
    68 for the short one) and the reduce kernel adds them over the whole parameter vector.  Two epochs against the restatement, 8 x rule."""
    from birdnet_stm32.training.linear_probe import fit_probe, fit_probe_reference

    X, Y, _ = _clusters(4096 + 1632, 256, 12, seed=21)
    kw = dict(epochs=2, batch_size=4096, learning_rate=1e-2, optimizer="adam", clipnorm=1.0, dropout=0.5, seed=4, hidden_units=64)
    r64 = fit_probe_reference(X, Y, dtype=np.float64, **kw)
    r32 = fit_probe_reference(X, Y, dtype=np.float32, **kw)
    dev = fit_probe(ctx, X, Y, **kw)
    again = fit_probe(ctx, X, Y, **kw)
    P64 = _vec(r64, hist=True)
    d32, dd = _rel(_vec(r32, hist=True), P64), _rel(_vec(dev), P64)
    l32, ld = _rel(r32.history["step_loss"], r64.history["step_loss"]), _rel(dev.history["step_loss"], r64.history["step_loss"])
    print(f"batch 4096+1632: weights d32 {d32:.3e} device {dd:.3e} (ratio {dd / d32:.2f}); step losses d32 {l32:.3e} device {ld:.3e} (ratio {ld / l32:.2f})")
    assert np.array_equal(_vec(dev), _vec(again))
    assert dd <= 8 * d32 and ld <= 8 * l32


def test_same_seed_same_bits(torch_mod, ctx):
    torch = torch_mod
    from birdnet_stm32.training.linear_probe import fit_probe

    X, Y, _ = _clusters(2000, 256, 40, seed=8)
    Xv, Yv, _ = _clusters(300, 256, 40, seed=9)
    kw = dict(epochs=2, batch_size=96, optimizer="adamw", weight_decay=1e-3, hidden_units=48, label_smoothing=0.1)   # 96 rows: several row groups
    a = fit_probe(ctx, X, Y, Xv, Yv, seed=11, **kw)
    b = fit_probe(ctx, torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), Xv, Yv, seed=11, **kw)
    c = fit_probe(ctx, X, Y, Xv, Yv, seed=12, **kw)
    assert np.array_equal(_vec(a).view(np.uint64), _vec(b).view(np.uint64))
    assert np.array_equal(a.history["step_loss"], b.history["step_loss"]) and a.history["val_loss"] == b.history["val_loss"]
    assert not np.array_equal(a.W1, c.W1) and not np.array_equal(a.W, c.W)


def test_validation_loss_and_best_weights(torch_mod, ctx):
    """bn_probe_mlp_loss is the loss of the returned weights over the raw validation targets (the training targets are smoothed), and the
    head returned after early stopping is the one of the best epoch."""
    from birdnet_stm32.training import linear_probe as lp

    X, Y, _ = _clusters(512, 64, 6, seed=1)
    Xv, Yv, _ = _clusters(128, 64, 6, seed=2)
    Yv = Yv[np.random.default_rng(0).permutation(len(Yv))]
    head = lp.fit_probe(ctx, X, Y, Xv, Yv, patience=3, epochs=30, batch_size=32, learning_rate=2e-2, dropout=0.0, seed=5, hidden_units=16, label_smoothing=0.1)
    h = head.history
    best = h["best_epoch"]
    print("val_loss", [round(v, 4) for v in h["val_loss"]], "best", best, "stopped", h["stopped_epoch"])
    assert h["stopped_epoch"] is not None and h["stopped_epoch"] == best + 3 and best == int(np.argmin(h["val_loss"]))
    P = lp.mlp_forward(Xv.astype(np.float64), *(v.astype(np.float64) for v in (head.W1, head.b1, head.W, head.b)), "sigmoid")
    want = float(lp.probe_loss(P, Yv.astype(np.float64), "sigmoid"))
    assert abs(h["val_loss"][best] - want) <= 1e-5 * want   # (float32 scores of 64- and 16-term dot products, a float32 mean)


@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
@pytest.mark.parametrize("n,D,H,C", [(37, 96, 24, 7), (1000, 256, 64, 100), (16, 1, 1, 1)])
def test_head_mlp_forward_against_numpy(torch_mod, ctx, activation, n, D, H, C):
    """bn_head_mlp_forward against float64 under the forward bound (no dropout: m2 = 1), plus the rounding of the stored float32."""
    from birdnet_stm32.training.linear_probe import ProbeHead, mlp_forward

    rng = np.random.default_rng(n + C)
    X = np.maximum(rng.standard_normal((n, D)), 0).astype(np.float32)
    W1 = (rng.standard_normal((D, H)) / np.sqrt(D)).astype(np.float32)
    W2 = (rng.standard_normal((H, C)) / np.sqrt(H)).astype(np.float32)
    b1, b2 = rng.standard_normal(H).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    head = ProbeHead(W2, b2, activation, [], {}, W1, b1)
    got = head.predict(X, ctx)
    X64, W1_, b1_, W2_, b2_ = (v.astype(np.float64) for v in (X, W1, b1, W2, b2))
    _a, _da, hd, _dhd, P, dP = _forward_bound(X64, W1_, b1_, np.ones((n, H)), W2_, b2_, activation)
    assert np.array_equal(P, mlp_forward(X64, W1_, b1_, W2_, b2_, activation)) and (hd > 0).any()
    err = np.abs(got - P)
    print(f"{activation} n={n} D={D} H={H} C={C}: max err {err.max():.3e}, max err/bound {np.max(err / (dP + U * P)):.3f}")
    assert got.shape == (n, C) and got.dtype == np.float32 and np.all(err <= dP + U * P)
    d = torch_mod.from_numpy(X).cuda()
    assert torch_mod.equal(head.predict(d, ctx).cpu(), torch_mod.from_numpy(got))
    assert head.predict(np.zeros((0, D), np.float32), ctx).shape == (0, C)   # n == 0 launches nothing
    head.close()


def test_focal_loss_row_weights_and_rows(torch_mod, ctx):
    """Focal loss with row weights and `rows` (upsampling: repeats inside a batch) on one small case, 8 x rule."""
    from birdnet_stm32.training.linear_probe import fit_probe, fit_probe_reference

    X, Y, lab = _clusters(300, 64, 5, seed=13, multi_hot=True)
    rng = np.random.default_rng(3)
    w = rng.uniform(0.3, 4.0, 300).astype(np.float32)
    rows = np.sort(np.concatenate([np.arange(300), np.repeat(np.flatnonzero(lab == 0), 3)])).astype(np.int32)   # class 0 four times
    kw = dict(activation="sigmoid", epochs=4, batch_size=64, learning_rate=1e-2, dropout=0.5, seed=6, hidden_units=24, loss="focal", focal_gamma=2.0,
              sample_weight=w, rows=rows)
    r64 = fit_probe_reference(X, Y, X[:50], Y[:50], dtype=np.float64, **kw)
    r32 = fit_probe_reference(X, Y, X[:50], Y[:50], dtype=np.float32, **kw)
    dev = fit_probe(ctx, X, Y, X[:50], Y[:50], **kw)
    assert len(dev.history["step_loss"]) == 4 * int(np.ceil(len(rows) / 64)) and len(rows) > 300
    P64 = _vec(r64, hist=True)
    d32, dd = _rel(_vec(r32, hist=True), P64), _rel(_vec(dev), P64)
    l32, ld = _rel(r32.history["step_loss"], r64.history["step_loss"]), _rel(dev.history["step_loss"], r64.history["step_loss"])
    v32, vd = _rel(r32.history["val_loss"], np.asarray(r64.history["val_loss"])), _rel(dev.history["val_loss"], np.asarray(r64.history["val_loss"]))
    print(f"focal + weights + rows: weights d32 {d32:.3e} device {dd:.3e} (ratio {dd / d32:.2f}); step losses d32 {l32:.3e} device {ld:.3e} "
          f"(ratio {ld / l32:.2f}); val losses d32 {v32:.3e} device {vd:.3e}")
    assert dd <= 8 * d32 and ld <= 8 * l32 and vd <= 8 * v32


def test_mlp_abi_refuses_bad_calls(torch_mod, ctx):
    torch = torch_mod
    lib = ctx.lib
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    z = lambda *s: torch.zeros(s, device="cuda")   # noqa: E731
    X, Y = torch.rand((64, 32), device="cuda"), z(64, 5)
    W1, b1, W2, b2 = 0.1 * torch.randn((32, 8), device="cuda"), z(8), 0.1 * torch.randn((8, 5), device="cuda"), z(5)
    out, perm, loss = torch.empty((64, 5), device="cuda"), torch.arange(64, dtype=torch.int32, device="cuda"), torch.empty(64, device="cuda")
    P = [t.data_ptr() for t in (W1, b1, W2, b2)]

    def err():
        return lib.bn_last_error().decode()

    fwd = lambda emb, n, D, H, C, act: lib.bn_head_mlp_forward(ctx.handle, emb, n, D, P[0], P[1], H, P[2], P[3], C, act, out.data_ptr(), stream)   # noqa: E731
    assert fwd(None, 64, 32, 8, 5, 0) == -1 and "null" in err()
    assert fwd(X.data_ptr(), 64, 32, 0, 5, 0) == -1 and "H=0" in err()
    assert fwd(X.data_ptr(), 64, 32, 2049, 5, 0) == -1 and "H=2049" in err()
    assert fwd(X.data_ptr(), 64, 0, 8, 5, 0) == -1 and "D=0" in err()
    assert fwd(X.data_ptr(), 64, 32, 8, 4097, 0) == -1 and "C=4097" in err()
    assert fwd(X.data_ptr(), 64, 32, 8, 5, 2) == -1 and "activation" in err()
    assert fwd(X.data_ptr(), -1, 32, 8, 5, 0) == -1 and "row count" in err()
    assert fwd(None, 0, 32, 8, 5, 0) == 0   # n == 0: nothing to read
    assert lib.bn_head_mlp_forward(ctx.handle, X.data_ptr(), 64, 32, P[0], None, 8, P[2], P[3], 5, 0, out.data_ptr(), stream) == -1 and "null" in err()
    h = ctypes.c_void_p()
    mk = lambda D, H, C, act, opt, drop, total, *p: lib.bn_probe_mlp_create(ctx.handle, D, H, C, act, opt, 1e-3, 0.0, 1.0, drop, 1, total, *p,   # noqa: E731
                                                                            ctypes.byref(h), stream)
    assert mk(32, 0, 5, 0, 0, 0.5, 10, *P) == -1 and "H=0" in err() and not h.value
    assert mk(32, 4096, 5, 0, 0, 0.5, 10, *P) == -1 and "H=4096" in err()
    assert mk(32, 8, 5, 0, 3, 0.5, 10, *P) == -1 and "optimizer" in err()
    assert mk(32, 8, 5, 0, 0, 1.0, 10, *P) == -1 and "dropout" in err()
    assert mk(32, 8, 5, 0, 0, 0.5, 0, *P) == -1 and "total_steps" in err()
    assert mk(32, 8, 5, 0, 0, 0.5, 10, P[0], P[1], None, P[3]) == -1 and "null" in err() and not h.value
    assert lib.bn_probe_mlp_create(ctx.handle, 32, 8, 5, 0, 0, 1e-3, 0.0, 1.0, 0.5, 1, 10, *P, None, stream) == -1 and "out" in err()
    assert mk(32, 8, 5, 1, 0, 0.5, 10, *P) == 0 and h.value
    try:
        assert lib.bn_probe_mlp_set_loss(h, 1, 2.0) == -1 and "softmax" in err()   # focal is the sigmoid head's
    finally:
        lib.bn_probe_mlp_destroy(h)
    h = ctypes.c_void_p()
    assert mk(32, 8, 5, 0, 0, 0.5, 10, *P) == 0 and h.value
    try:
        ep = lambda hh, x, y, n, batch: lib.bn_probe_mlp_epoch_weighted(hh, x, y, None, perm.data_ptr(), n, batch, loss.data_ptr(), stream)   # noqa: E731
        assert ep(h, X.data_ptr(), Y.data_ptr(), 64, 0) == -1 and "batch" in err()
        assert ep(h, X.data_ptr(), Y.data_ptr(), 64, 65) == -1 and "batch" in err()
        assert ep(h, X.data_ptr(), None, 64, 16) == -1 and "null" in err()
        assert ep(None, X.data_ptr(), Y.data_ptr(), 64, 16) == -1 and "null probe" in err()
        assert lib.bn_probe_mlp_loss(h, X.data_ptr(), Y.data_ptr(), 0, loss.data_ptr(), stream) == -1 and "row count" in err()
        assert lib.bn_probe_mlp_loss(h, X.data_ptr(), None, 64, loss.data_ptr(), stream) == -1 and "null" in err()
        assert lib.bn_probe_mlp_get(h, P[0], None, P[2], P[3], stream) == -1 and lib.bn_probe_mlp_set(h, P[0], P[1], P[2], None, stream) == -1
        assert lib.bn_probe_mlp_set_loss(h, 7, 2.0) == -1 and "unknown loss" in err()
        assert lib.bn_probe_mlp_set_loss(h, 1, -1.0) == -1 and "focal_gamma" in err()
        assert lib.bn_probe_mlp_set_loss(None, 1, 2.0) == -1
        # ... and the probe is still usable
        assert ep(h, X.data_ptr(), Y.data_ptr(), 64, 16) == 0
        assert lib.bn_probe_mlp_loss(h, X.data_ptr(), Y.data_ptr(), 64, loss[4:].data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(loss[:5]).all()
    finally:
        lib.bn_probe_mlp_destroy(h)
    lib.bn_probe_mlp_destroy(None)


def test_oversized_workspace_is_refused(torch_mod, ctx):
    """The largest head at a batch of 8192 rows: hd, dA, G and the batch's targets alone take 8192 * (2 * 2048 + 2 * 4096) floats = 384 MiB,
    over BN_PROBE_WORKSPACE_BYTES (256 MiB).  Refused before anything is launched; a batch of 64 of the same head runs."""
    torch = torch_mod
    lib = ctx.lib
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    D, H, C, n = 2048, 2048, 4096, 8192
    X, Y = torch.zeros((n, D), device="cuda"), torch.zeros((n, C), device="cuda")
    W1, b1, W2, b2 = torch.zeros((D, H), device="cuda"), torch.zeros(H, device="cuda"), torch.zeros((H, C), device="cuda"), torch.zeros(C, device="cuda")
    perm, loss = torch.arange(n, dtype=torch.int32, device="cuda"), torch.full((n,), float("nan"), device="cuda")
    h = ctypes.c_void_p()
    assert lib.bn_probe_mlp_create(ctx.handle, D, H, C, 0, 0, 1e-3, 0.0, 1.0, 0.5, 1, 10, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr(),
                                   ctypes.byref(h), stream) == 0
    try:
        rc = lib.bn_probe_mlp_epoch_weighted(h, X.data_ptr(), Y.data_ptr(), None, perm.data_ptr(), n, n, loss.data_ptr(), stream)
        msg = lib.bn_last_error().decode()
        assert rc == -4 and "workspace" in msg and "over the cap" in msg, (rc, msg)   # BN_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert torch.isnan(loss).all()   # nothing ran
        assert lib.bn_probe_mlp_epoch_weighted(h, X.data_ptr(), Y.data_ptr(), None, perm.data_ptr(), 64, 64, loss.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert abs(float(loss[0]) - np.log(2.0)) < 1e-6   # all-zero parameters: every score is 1/2
    finally:
        lib.bn_probe_mlp_destroy(h)
    with pytest.raises(ValueError, match="hidden_units <= 2048"):
        from birdnet_stm32.training.linear_probe import fit_probe

        fit_probe(ctx, np.zeros((4, 8), np.float32), np.zeros((4, 2), np.float32), hidden_units=2049)


# -- end to end -----------------------------------------------------------------------------------------------------------------------
SR = 24000
FAMILY_OF = {"harmonic_stack": 6, "chirp": 3, "noise": 2}   # class folder -> family of tools/signal_families.py; white noise is the negative folder


def _family_audio(torch, kind, n_chunks, g):
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


def test_probe_hidden_units_then_analyze_with_the_head(torch_mod, tmp_path):
    """A handful of synthetic WAVs in class folders -> probe --hidden_units 32 -> analyze --head: the detections carry the scores of
    ProbeHead.predict on the same files' embeddings."""
    import json

    from birdnet_stm32.cli import analyze as analyze_cli
    from birdnet_stm32.cli import probe as probe_cli
    from birdnet_stm32.evaluation.detections import detect_files
    from birdnet_stm32.evaluation.embeddings import embed_files
    from birdnet_stm32.models.runners import load_model_runner
    from birdnet_stm32.training.linear_probe import ProbeHead, mlp_forward

    torch = torch_mod
    g = torch.Generator(device="cuda").manual_seed(7)
    train_dir, held_dir = tmp_path / "train", tmp_path / "held"
    held = []
    for kind in FAMILY_OF:
        for d in (train_dir, held_dir):
            os.makedirs(d / kind)
        for i in range(8):
            _write_wav(train_dir / kind / f"{i:02d}.wav", _family_audio(torch, kind, 1, g))
        for i in range(2):
            _write_wav(held_dir / kind / f"{i:02d}.wav", _family_audio(torch, kind, 1, g))
            held.append(str(held_dir / kind / f"{i:02d}.wav"))
    runner = load_model_runner(TFLITE_PATH, max_batch=64, prepare_pipeline=True)
    try:
        out = str(tmp_path / "mlphead")
        head = probe_cli.main(["--model_path", TFLITE_PATH, "--model_config", CONFIG_PATH, "--data_path_train", str(train_dir), "--output", out,
                               "--epochs", "20", "--batch_size", "8", "--learning_rate", "0.01", "--seed", "3", "--hidden_units", "32"], runner=runner)
        for suffix in (".npz", "_labels.txt", "_model_config.json", "_history.csv"):
            assert os.path.isfile(out + suffix), suffix
        loaded = ProbeHead.load(out + ".npz")
        dim = runner.embedding_info()["dim"]
        assert loaded.hidden_units == 32 and loaded.embedding_dim == dim and loaded.W1.shape == (dim, 32) and loaded.W.shape == (32, 2)
        assert loaded.class_names == ["chirp", "harmonic_stack"] and all(np.array_equal(getattr(loaded, k), getattr(head, k)) for k in ("W1", "b1", "W", "b"))
        assert json.load(open(out + "_model_config.json"))["num_classes"] == 2
        assert len(open(out + "_history.csv").read().splitlines()) == 1 + len(head.history["loss"])
        assert head.history["loss"][-1] < head.history["loss"][0]

        he = embed_files(runner, held, max_duration=3, sample_rate=22050, chunk_duration=3.0)
        assert he.embeddings.shape[0] == len(held)
        want = loaded.predict(he.embeddings, runner.ctx)
        ref = mlp_forward(he.embeddings.astype(np.float64), *(v.astype(np.float64) for v in (loaded.W1, loaded.b1, loaded.W, loaded.b)), "sigmoid")
        assert np.abs(want - ref).max() <= 1e-5   # (the bound itself is test_head_mlp_forward_against_numpy's business)
        det = detect_files(runner, held, min_conf=0.0, top_k=2, sample_rate=22050, chunk_duration=3.0, class_names=loaded.class_names, head=loaded,
                           return_scores=True)
        assert np.array_equal(det.scores, want)
        det = analyze_cli.main(["--model_path", TFLITE_PATH, "--model_config", CONFIG_PATH, "--head", out + ".npz", "--input", *held,
                                "--output", str(tmp_path / "held.csv"), "--min_conf", "0.0", "--top_k", "1"], runner=runner)
        assert len(det) == len(held)
        for f, c, s in zip(det.file_index, det.class_index, det.score):
            assert int(c) == int(np.argmax(want[int(f)])) and np.float32(s) == want[int(f), int(c)]
        text = open(tmp_path / "held.csv").read()
        assert any(c in text for c in loaded.class_names)
    finally:
        runner.close()
