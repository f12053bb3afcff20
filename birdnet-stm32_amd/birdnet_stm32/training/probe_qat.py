"""Quantisation-aware fine-tuning of a probe head for the INT8 export (reference: ``train --qat``, birdnet_stm32/training/qat.py).

``probe --export_tflite`` quantises the trained float head after the fact (``conversion/head_export.py``).  When that costs too much, a
short fine-tune lets the head see both kinds of quantisation the export applies:

* the weights as ``conversion.quantize.quantize_weights`` will write them (``fake_quantize_head_weights``): the forward reads
  ``q * s_w`` while the gradient and the optimiser act on the full-precision shadow weights, the plain straight-through estimator;
* the logits on the grid ``choose_activation_params(*logit_range)`` gives the exported logit tensor (``fake_quantize_logits``), with
  TensorFlow's fake-quant gradient: zero where the code clamps.

``fit_probe_qat`` is the device fit (``bn_probe_set_qat`` on ``fit_probe``'s backend, ``csrc/bn_probe_step.h`` EXT = 2),
``fit_probe_qat_reference`` the same procedure in numpy.  The export must then be given the same ``logit_range``
(``export_head_tflite(..., logit_range=)``), so that the file's logit parameters are the ones trained against.

Not modelled in training: the int32 bias grid, the Q31 requantisation multiplier and the sigmoid's 1/256 output grid.  Label smoothing
and the augmented fit are no part of the QAT phase (the reference's QAT trains without augmentation).
"""

from __future__ import annotations

import ctypes
from dataclasses import replace

import numpy as np

from birdnet_stm32.conversion.quantize import choose_activation_params, quantize_weights
from birdnet_stm32.training import linear_probe as lp


def fake_quantize_head_weights(W, per_tensor: bool = False) -> np.ndarray:
    """``W [D, C]`` as the exported head holds it: ``q.astype(float32) * s_w`` of ``quantize_weights(W.T, 0, per_tensor)``, as ``[D, C]``
    float32.  ``bn_probe_get_quantized`` gives the same bits."""
    q, s_w = quantize_weights(np.asarray(W).T, 0, per_tensor)
    return np.ascontiguousarray((q.astype(np.float32) * s_w[:, None]).T)


def _fake_quantize_logits(z: np.ndarray, s_out, z_out, dt):
    s, zp = dt(np.float32(s_out)), dt(int(z_out))
    k = np.rint(z.astype(dt) / s) + zp
    kc = np.clip(k, dt(-128.0), dt(127.0))
    return (kc - zp) * s, kc.astype(np.int8), k == kc


def fake_quantize_logits(z, s_out: float, z_out: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(zq, codes, pass)`` of float32 logits on the int8 grid ``(s_out, z_out)``, every operation rounded to float32 (the statements of
    ``probe_fake_quant``, ``csrc/bn_probe_step.h``): ``k = rint(z / s_out) + z_out``, ``kc = clip(k, -128, 127)``, ``zq = (kc - z_out) * s_out``,
    ``codes = kc`` as int8 and ``pass = (k == kc)``: False exactly where the unclamped code leaves ``[-128, 127]``."""
    return _fake_quantize_logits(np.asarray(z, np.float32), s_out, z_out, np.float32)


def _scores_of_logits(z: np.ndarray, activation: str) -> np.ndarray:
    if activation == "softmax":
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def _check_qat_args(head, logit_range, label_smoothing, augment) -> tuple[float, float, float, int]:
    """``(lo, hi, s_out, z_out)``; label smoothing and augmentation are refused by name."""
    if label_smoothing:
        raise ValueError("label_smoothing is no part of the QAT phase: fine-tune without it")
    if augment is not None:
        raise ValueError("augment is no part of the QAT phase: the fine-tune runs on the embeddings as they are (fit_probe_augmented comes first)")
    if not isinstance(head, lp.ProbeHead):
        raise ValueError("head must be the ProbeHead to fine-tune")
    try:
        lo, hi = (float(v) for v in logit_range)
    except (TypeError, ValueError):
        raise ValueError(f"logit_range must be (lowest, highest) logit, got {logit_range!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise ValueError(f"bad logit range [{lo}, {hi}]")
    s_out, z_out = choose_activation_params(lo, hi)
    return lo, hi, s_out, z_out


def _plan_qat(X, Y, X_val, head, device: bool, fit_kw: dict):
    plan = lp._plan_fit(X, Y, X_val, device=device, activation=head.activation, **fit_kw)
    if (plan.D, plan.C) != (head.embedding_dim, head.num_classes):
        raise ValueError(f"the head is [{head.embedding_dim}, {head.num_classes}], the rows are X [*, {plan.D}] and Y [*, {plan.C}]")
    return replace(plan, W0=head.W.copy(), b0=head.b.copy())


def _finish(fitted, head, class_names, lo, hi, s_out, z_out, per_tensor, quantize_logits):
    fitted.class_names = list(class_names if class_names is not None else head.class_names)
    fitted.history["qat"] = {"logit_range": [lo, hi], "logit_scale": s_out, "logit_zero_point": z_out, "per_tensor": bool(per_tensor),
                             "quantize_logits": bool(quantize_logits), "epochs": len(fitted.history["loss"])}
    return fitted


class _QatNumpyBackend(lp._NumpyBackend):
    """``_NumpyBackend`` with the fake-quantised forward; the update acts on the shadow parameters ``self.P``."""

    def __init__(self, X, Y, X_val, Y_val, plan, dtype, per_tensor, quantize_logits, s_out, z_out):
        super().__init__(X, Y, X_val, Y_val, plan, dtype)
        self.per_tensor, self.quantize_logits, self.s_out, self.z_out = bool(per_tensor), bool(quantize_logits), s_out, z_out

    def forward(self, x):
        """``(probabilities, pass)`` of rows ``x [*, D]``."""
        D = self.P.shape[0] - 1
        z = x @ fake_quantize_head_weights(self.P[:D], self.per_tensor).astype(self.dt) + self.P[D]
        ok = True
        if self.quantize_logits:
            z, _, ok = _fake_quantize_logits(z, self.s_out, self.z_out, self.dt)
        return _scores_of_logits(z, self.plan.activation), ok

    def epoch(self, perm):
        c, dt, D = self.plan, self.dt, self.X.shape[1]
        losses = []
        for s in range(0, len(perm), c.batch):
            idx = perm[s : s + c.batch]
            B = len(idx)
            xd = np.concatenate([self.X[idx] * lp.dropout_mask(c.seed, self.t, B, D, c.dropout, dt), np.ones((B, 1), dt)], axis=1)
            P, ok = self.forward(xd[:, :D])
            y = self.Y[idx]
            w = None if self.w is None else self.w[idx]
            losses.append(float(lp.probe_loss(P, y, c.activation, sample_weight=w, **self.loss_kw)))
            G = lp.probe_loss_gradient(P, y, c.activation, sample_weight=w, **self.loss_kw) * ok
            g = lp.clip_by_global_norm(xd.T @ G, c.clipnorm)
            lr_t, alpha_t = lp.step_sizes(c.lr, self.t, c.total)
            self.P = lp.optimizer_step(self.P, g, self.state, c.optimizer, np.float32(lr_t), np.float32(alpha_t), np.float32(c.weight_decay))
            self.t += 1
        return losses

    def val_loss(self):
        return lp.probe_loss(self.forward(self.Xv)[0], self.Yv, self.plan.activation, **self.loss_kw)


class _QatDeviceBackend(lp._DeviceBackend):
    """``_DeviceBackend`` with ``bn_probe_set_qat`` applied: every step and ``val_loss`` run the fake-quantised forward."""

    def __init__(self, ctx, X, Y, X_val, Y_val, plan, per_tensor, quantize_logits, s_out, z_out):
        super().__init__(ctx, X, Y, X_val, Y_val, plan)
        try:
            self.hip.check(ctx.lib.bn_probe_set_qat(self.handle, self.hip.PROBE_QAT_WEIGHTS["per_tensor" if per_tensor else "per_class"],
                                                    int(bool(quantize_logits)), ctypes.c_float(s_out), int(z_out)))
        except Exception:
            self.close()
            raise
        self.quantize_logits = bool(quantize_logits)

    def quantized(self):
        """The weights ``[D, C]`` the next forward reads (``bn_probe_get_quantized``), a CUDA tensor."""
        Wq = self.torch.empty_like(self.W)
        with self.torch.cuda.device(self.dev):
            self.hip.check(self.ctx.lib.bn_probe_get_quantized(self.handle, Wq.data_ptr(), self._stream()))
        return Wq

    def scores(self, X):
        """``(scores [n, C] float32, logit codes [n, C] int8 or None)`` of rows ``X`` under the QAT setting (``bn_probe_scores``)."""
        X = self._dev(X)
        n = int(X.shape[0])
        out = self.torch.empty((n, self.C), dtype=self.torch.float32, device=self.dev)
        codes = self.torch.empty((n, self.C), dtype=self.torch.int8, device=self.dev) if self.quantize_logits else None
        with self.torch.cuda.device(self.dev):
            self.hip.check(self.ctx.lib.bn_probe_scores(self.handle, X.data_ptr(), n, out.data_ptr(), self._ptr(codes), self._stream()))
            self.torch.cuda.current_stream(self.dev).synchronize()   # (X may be a temporary of this call)
        return out, codes


def qat_logit_codes(ctx_or_runner, head, X, logit_range, per_tensor: bool = False) -> np.ndarray:
    """The int8 logit codes ``[n, C]`` the fake-quantised forward of ``head`` gives rows ``X`` (``bn_probe_scores``): what the fine-tune
    saw, to hold against the bytes of the exported head (``bn_head_i8_forward``)."""
    lo, hi, s_out, z_out = _check_qat_args(head, logit_range, 0.0, None)
    X0, Y0 = np.zeros((1, head.embedding_dim), np.float32), np.zeros((1, head.num_classes), np.float32)   # (a backend holds training rows; none are used)
    plan = _plan_qat(X0, Y0, None, head, True, dict(optimizer="sgd", batch_size=1, dropout=0.0, epochs=1, learning_rate=0.0))
    be = _QatDeviceBackend(getattr(ctx_or_runner, "ctx", ctx_or_runner), X0, Y0, None, None, plan, per_tensor, True, s_out, z_out)
    try:
        return be.scores(X)[1].cpu().numpy()
    finally:
        be.close()


def fit_probe_qat(ctx_or_runner, X, Y, X_val=None, Y_val=None, *, head, logit_range, per_tensor=False, quantize_logits=True, epochs=10,
                  learning_rate=1e-4, batch_size=32, optimizer="adam", weight_decay=0.0, clipnorm=1.0, dropout=0.5, patience=10, seed=42,
                  class_names=None, loss="auto", focal_gamma=2.0, sample_weight=None, rows=None, label_smoothing=0.0, augment=None,
                  hidden_units=0) -> lp.ProbeHead:
    """Fine-tune ``head`` on the device with the forward the INT8 export will compute: weights fake-quantised per class (one scale with
    ``per_tensor``), logits on the grid of ``choose_activation_params(*logit_range)`` (``quantize_logits``).  ``logit_range`` is the range
    the export will be given (``float_logit_range`` of the float head over the calibration rows).  The other keywords are ``fit_probe``'s;
    the procedure is ``fit_probe``'s too, starting from ``head`` instead of a fresh one, so the validation loss and early stopping are on
    the fake-quantised forward.  Returns a ``ProbeHead`` of the full-precision shadow weights, for ``quantize_head`` /
    ``export_head_tflite`` with the same ``logit_range``; ``history["qat"]`` holds the range, scale, zero point and flags.
    ``label_smoothing`` and ``augment`` are refused: they are no part of the QAT phase; so is a head with a hidden layer."""
    lp.refuse_hidden("fit_probe_qat", hidden_units, head)
    lo, hi, s_out, z_out = _check_qat_args(head, logit_range, label_smoothing, augment)
    plan = _plan_qat(X, Y, X_val, head, True, dict(optimizer=optimizer, batch_size=batch_size, dropout=dropout, epochs=epochs, learning_rate=learning_rate,
                                                   weight_decay=weight_decay, clipnorm=clipnorm, patience=patience, seed=seed, loss=loss,
                                                   focal_gamma=focal_gamma, sample_weight=sample_weight, rows=rows))
    be = _QatDeviceBackend(getattr(ctx_or_runner, "ctx", ctx_or_runner), X, Y, X_val, Y_val, plan, per_tensor, quantize_logits, s_out, z_out)
    return _finish(lp._device_fit(be, plan, None), head, class_names, lo, hi, s_out, z_out, per_tensor, quantize_logits)


def fit_probe_qat_reference(X, Y, X_val=None, Y_val=None, *, head, logit_range, per_tensor=False, quantize_logits=True, epochs=10, learning_rate=1e-4,
                            batch_size=32, optimizer="adam", weight_decay=0.0, clipnorm=1.0, dropout=0.5, patience=10, seed=42, class_names=None,
                            loss="auto", focal_gamma=2.0, sample_weight=None, rows=None, label_smoothing=0.0, augment=None,
                            dtype=np.float64) -> lp.ProbeHead:
    """The procedure of ``fit_probe_qat`` in numpy, the arithmetic in ``dtype`` (the weight rule is ``quantize_weights`` itself, float64
    inside, its result cast to ``dtype``).  ``history["W"]`` / ``["b"]`` keep the shadow weights in ``dtype``."""
    lo, hi, s_out, z_out = _check_qat_args(head, logit_range, label_smoothing, augment)
    X, Y = np.asarray(X), np.asarray(Y)
    plan = _plan_qat(X, Y, X_val, head, False, dict(optimizer=optimizer, batch_size=batch_size, dropout=dropout, epochs=epochs, learning_rate=learning_rate,
                                                    weight_decay=weight_decay, clipnorm=clipnorm, patience=patience, seed=seed, loss=loss,
                                                    focal_gamma=focal_gamma, sample_weight=sample_weight, rows=rows))
    be = _QatNumpyBackend(X, Y, X_val, Y_val, plan, dtype, per_tensor, quantize_logits, s_out, z_out)
    return _finish(lp._reference_fit(be, plan, None), head, class_names, lo, hi, s_out, z_out, per_tensor, quantize_logits)
