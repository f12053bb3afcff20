"""Linear probe: train a new classifier head on frozen embeddings (reference: birdnet_stm32/training/linear_probe.py).

The reference freezes the backbone, puts ``Dropout -> Dense(len(classes))`` behind the pooled vector and lets Keras train that, running
the backbone on every batch of every epoch.  Here the backbone runs once (``evaluation.embeddings.embed_files``) and the head is trained
on the ``[N, D]`` matrix, which stays on the device for the whole fit (``csrc/bn_probe.hip``, C ABI ``bn_probe_*``).

* ``fit_probe``            the device fit,
* ``fit_probe_reference``  the same procedure in numpy: the specification the device code is tested against,
* ``fit_probe_sweep``      many heads with different hyperparameters trained at once on the device (``csrc/bn_probe_sweep.hip``, C ABI
  ``bn_probe_sweep_*``; ``training/tune.py`` draws the trials), and ``fit_probe_sweep_reference``, a loop of ``fit_probe_reference``,
* ``fit_probe_augmented``  the device fit on fresh embeddings per epoch: mixup and SpecAugment over resident model inputs
  (``training/augment.py``, ``csrc/bn_augment.hip``), and ``fit_probe_augmented_reference``, the same loop in numpy,
* ``ProbeHead``            the result: ``W [D, C]``, ``b [C]``, activation, class names; ``save`` / ``load`` (plain ``.npz``), ``predict``,
* ``hidden_units = H > 0`` of ``fit_probe`` / ``fit_probe_reference``: one ReLU layer between embedding and classes, with dropout in front
  of both layers (``csrc/bn_probe_mlp.hip``, C ABI ``bn_probe_mlp_*``; ``mlp_loss_and_gradient`` is the step's definition),
* ``run_linear_probe``     class folders -> embeddings -> head -> files on disk (the ``probe`` command).

The procedure (both implementations): Glorot-uniform ``W`` from ``default_rng(seed)``, zero ``b``; per epoch a permutation from
``default_rng([seed, epoch])`` cut into batches (the last one short); per step dropout by a counter-based hash, logits, sigmoid + binary
cross-entropy or softmax + categorical cross-entropy (Keras definitions, probabilities clipped to ``[1e-7, 1 - 1e-7]`` in the loss only;
with ``label_smoothing`` the training loss and its gradient see ``smooth_targets``, the validation loss the targets as they are),
clip by global norm, Adam / AdamW / SGD-with-momentum (Keras definitions) under a cosine schedule to zero; validation loss per epoch,
early stopping with the best weights restored (Keras ``EarlyStopping(patience, restore_best_weights=True)``).

For long-tailed class folders every fit takes ``loss="focal"`` / ``focal_gamma`` (the reference's ``training/losses.py: BinaryFocalLoss``),
``sample_weight`` (its balanced ``class_weight``: ``balanced_class_weights``, ``row_weights``) and ``rows`` (its ``--upsample_ratio``:
``data.dataset.upsample_minority_classes``, ``upsample_rows``); all off by default, ``probe_loss`` / ``probe_loss_gradient`` are their
definition.
"""

from __future__ import annotations

import csv
import json
import math
import os
from dataclasses import dataclass, field

import numpy as np

ACTIVATIONS = ("sigmoid", "softmax")
OPTIMIZERS = ("adam", "adamw", "sgd")
LOSSES = ("auto", "focal")   # "auto": the activation's cross-entropy
NOISE_CLASSES = ("noise", "silence", "background", "other")
BETA_1, BETA_2, ADAM_EPS, MOMENTUM, LOSS_EPS = 0.9, 0.999, 1e-7, 0.9, 1e-7


# -- the dropout mask ---------------------------------------------------------------------------------------------------------------
def _fmix(h: np.ndarray) -> np.ndarray:
    """The murmur3 finaliser on uint32 arrays (multiplications wrap)."""
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def dropout_hash(seed: int, step: int, n_rows: int, n_cols: int) -> np.ndarray:
    """The 24-bit draw of every (row in batch, column) of global step ``step``: ``[n_rows, n_cols]`` uint32 in ``[0, 2^24)``.
    Stateless; ``probe_drop_hash`` of ``csrc/bn_probe.hip`` is the same function."""
    with np.errstate(over="ignore"):
        h0 = _fmix(np.array([(int(seed) ^ (int(step) * 0x9E3779B1)) & 0xFFFFFFFF], np.uint32))
        rows = _fmix(h0 ^ (np.arange(n_rows, dtype=np.uint32) * np.uint32(0x85EBCA77)))
        h = _fmix(rows[:, None] ^ (np.arange(n_cols, dtype=np.uint32) * np.uint32(0xC2B2AE3D))[None, :])
    return h >> np.uint32(8)


def dropout_threshold(p: float) -> int:
    """An element is kept iff its draw is >= this (``p`` as the float32 the C ABI takes)."""
    return int(math.ceil(float(np.float32(p)) * 16777216.0)) if p > 0 else 0


def dropout_mask(seed: int, step: int, n_rows: int, n_cols: int, p: float, dtype=np.float32) -> np.ndarray:
    """``keep / (1 - p)`` of one step."""
    if not p > 0:
        return np.ones((n_rows, n_cols), dtype)
    scale = np.float32(1.0 / (1.0 - float(np.float32(p))))
    return (dropout_hash(seed, step, n_rows, n_cols) >= dropout_threshold(p)).astype(dtype) * np.asarray(scale, dtype)


# -- pieces of the procedure --------------------------------------------------------------------------------------------------------
def init_head(D: int, C: int, seed: int) -> tuple[np.ndarray, np.ndarray]:
    """Glorot-uniform ``W [D, C]`` (Keras' Dense default) and zero ``b``, float32."""
    limit = math.sqrt(6.0 / (D + C))
    W = np.random.default_rng(seed).uniform(-limit, limit, (D, C)).astype(np.float32)
    return W, np.zeros(C, np.float32)


DROP2_SEED_XOR = 0x48494444   # the hidden layer's dropout draws: ``dropout_mask(seed ^ DROP2_SEED_XOR, t, B, H, p)``


def init_mlp_head(D: int, H: int, C: int, seed: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``(W1 [D, H], b1 [H], W2 [H, C], b2 [C])`` of a head with ``H`` hidden units: ``init_head(D, H, seed)`` and ``init_head(H, C, seed + 1)``."""
    return (*init_head(D, H, seed), *init_head(H, C, seed + 1))


def refuse_hidden(what: str, hidden_units=0, head=None) -> None:
    """The paths that are not built for a hidden layer say so: none of them drops the layer silently."""
    if int(hidden_units or 0) > 0 or (head is not None and getattr(head, "W1", None) is not None):
        raise ValueError(f"{what} is not built for a head with a hidden layer (hidden_units > 0): train such a head with fit_probe / "
                         "`probe --hidden_units` alone, or drop the hidden layer")


def check_hidden_units(hidden_units, device: bool = False) -> int:
    H = int(hidden_units)
    if H != hidden_units or H < 0:
        raise ValueError(f"hidden_units must be an integer >= 0 (0 = no hidden layer), got {hidden_units!r}")
    if device and H > 0:
        from birdnet_stm32 import _hip

        if H > _hip.PROBE_MAX_D:
            raise ValueError(f"the device path takes hidden_units <= {_hip.PROBE_MAX_D}, got {H}")
    return H


def mlp_forward(X: np.ndarray, W1: np.ndarray, b1: np.ndarray, W2: np.ndarray, b2: np.ndarray, activation: str) -> np.ndarray:
    """Scores of a head with a hidden layer, without dropout: ``act(relu(X W1 + b1) W2 + b2)``."""
    return head_scores(np.maximum(X @ W1 + b1, X.dtype.type(0)), W2, b2, activation)


def mlp_loss_and_gradient(params: np.ndarray, xd: np.ndarray, m2: np.ndarray, y: np.ndarray, activation: str, *, loss="auto", focal_gamma=2.0,
                          sample_weight=None, relu_gate: bool = True):
    """One training step of the head with a hidden layer, before clip and optimiser, in ``params``' dtype.  ``params``: the vector
    ``[(D + 1) H | (H + 1) C]`` (``W1`` then ``b1`` as row ``D``; ``W2`` then ``b2`` as row ``H``); ``xd [B, D + 1]``: the batch after
    ``drop1`` with the column of ones; ``m2 [B, H]``: ``drop2``'s mask (``keep / (1 - p)``).  Returns ``(loss, gradient vector, parts)``:

        a = xd [W1; b1];  hd = relu(a) m2;  z = [hd, 1] [W2; b2];  G = dLoss/dz (probe_loss_gradient)
        dW2 = [hd, 1]^T G;  dA = (G W2^T) m2 [a > 0];  dW1 = xd^T dA

    ``parts``: ``a``, ``hd``, ``P``, ``G``, ``GW`` (``G W2^T``), ``dA``.  ``relu_gate=False`` leaves ``[a > 0]`` out of ``dA``: the gradient of no
    loss, there for tests that must tell a wrong gate from rounding."""
    dt = params.dtype.type
    B, D1 = xd.shape
    H, C = m2.shape[1], y.shape[1]
    P1, P2 = params[: D1 * H].reshape(D1, H), params[D1 * H :].reshape(H + 1, C)
    a = xd[:, : D1 - 1] @ P1[: D1 - 1] + P1[D1 - 1]
    hd = np.concatenate([np.maximum(a, dt(0)) * m2, np.ones((B, 1), params.dtype)], axis=1)
    P = head_scores(hd[:, :H], P2[:H], P2[H], activation)
    value = probe_loss(P, y, activation, loss=loss, focal_gamma=focal_gamma, sample_weight=sample_weight)
    G = probe_loss_gradient(P, y, activation, loss=loss, focal_gamma=focal_gamma, sample_weight=sample_weight)
    GW = G @ P2[:H].T
    dA = GW * m2 * (a > 0) if relu_gate else GW * m2
    g = np.concatenate([(xd.T @ dA).ravel(), (hd.T @ G).ravel()])
    return value, g, {"a": a, "hd": hd[:, :H], "P": P, "G": G, "GW": GW, "dA": dA}


def epoch_permutation(seed: int, epoch: int, n: int) -> np.ndarray:
    return np.random.default_rng([int(seed), int(epoch)]).permutation(n).astype(np.int32)


def step_sizes(learning_rate: float, t: int, total_steps: int) -> tuple[float, float]:
    """``(lr_t, alpha_t)`` of global step ``t`` (0-based): cosine decay to zero over ``total_steps`` (Keras ``CosineDecay(alpha=0)``) and
    Adam's step size with the bias correction folded in.  Computed in float64 (the device code does the same on the host).  This is the
    restatement's schedule; ``device_step_sizes`` below is its twin with the operations in ``bn_probe_epoch``'s order, which a sweep uploads:
    the two agree to the last bit or two of the float64, and a change to the schedule goes into both (and into ``bn_probe_epoch``)."""
    lr_t = float(np.float32(learning_rate)) * 0.5 * (1.0 + math.cos(math.pi * min(t, total_steps) / total_steps))
    return lr_t, lr_t * math.sqrt(1.0 - BETA_2 ** (t + 1)) / (1.0 - BETA_1 ** (t + 1))


def device_step_sizes(learning_rates, t0: int, steps: int, total_steps: int) -> np.ndarray:
    """``[steps, T, 2]`` float32: ``(lr_t, alpha_t)`` of global steps ``t0 .. t0 + steps - 1`` for ``T`` learning rates, the table a sweep
    uploads per epoch.  ``step_sizes`` with the operations in the order ``bn_probe_epoch`` has them on the host (``pi * (t / total)`` where
    ``step_sizes`` has ``(pi * t) / total``: the two can differ in the last bit of the float64, and a sweep's trial must have a single
    fit's bits, not just its procedure).  ``cos``, ``pow`` and ``sqrt`` are the C library's through ``math``, one call per step."""
    lr = np.asarray([float(np.float32(v)) for v in learning_rates], np.float64) * 0.5
    cosf, num, den = np.empty(steps), np.empty(steps), np.empty(steps)
    for i in range(steps):
        t = t0 + i
        cosf[i] = 1.0 + math.cos(math.pi * (float(min(t, total_steps)) / float(total_steps)))
        num[i] = math.sqrt(1.0 - math.pow(BETA_2, float(t + 1)))
        den[i] = 1.0 - math.pow(BETA_1, float(t + 1))
    lr_t = lr[None, :] * cosf[:, None]
    return np.stack([lr_t, lr_t * num[:, None] / den[:, None]], axis=2).astype(np.float32)


def smooth_targets(Y: np.ndarray, label_smoothing: float, activation: str) -> np.ndarray:
    """Keras' label smoothing in ``Y``'s dtype: ``y (1 - eps) + 0.5 eps`` (sigmoid) or ``y (1 - eps) + eps / C`` (softmax), with ``eps`` the
    float32 the C ABI takes.  The operation order is the forward kernel's (``csrc/bn_probe_step.h``): ``keep = 1 - eps`` and
    ``add = 0.5 * eps`` or ``eps / C`` first, then ``(y * keep) + add``, each operation rounded in the dtype (no fused multiply-add)."""
    dt = Y.dtype.type
    eps = dt(np.float32(label_smoothing))
    keep = dt(1.0) - eps
    add = eps / dt(Y.shape[1]) if activation == "softmax" else dt(0.5) * eps
    return Y * keep + add


def head_scores(X: np.ndarray, W: np.ndarray, b: np.ndarray, activation: str) -> np.ndarray:
    z = X @ W + b
    if activation == "softmax":
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def _check_loss(loss, focal_gamma, activation) -> tuple[str, float]:
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES}, not {loss!r}")
    gamma = float(focal_gamma)
    if not (math.isfinite(gamma) and gamma >= 0.0):
        raise ValueError(f"focal_gamma must be finite and >= 0, got {focal_gamma!r}")
    if loss == "focal" and activation != "sigmoid":
        raise ValueError("loss='focal' is the sigmoid head's loss: not with activation='softmax'")
    return loss, gamma


def _loss_elements(P, Y, activation, loss, focal_gamma):
    """Per element: the loss and its derivative by the logit, before weights and the mean's scale.  The operations, and their order, are
    ``probe_loss_elem``'s (``csrc/bn_probe_step.h``).  Focal, with ``pc`` the clipped probability: ``bce = -(y log pc + (1 - y) log(1 - pc))``,
    ``q = 1 - (y pc + (1 - y)(1 - pc))``, ``f = exp(gamma log q)``, loss ``f bce``, derivative ``f (p - y) - gamma (f / q) (2 y - 1) pc (1 - pc) bce``.
    ``gamma = 0`` is not special-cased: ``f`` is exactly 1 and the second term exactly 0."""
    dt = P.dtype.type
    one = dt(1.0)
    Pc = np.clip(P, dt(LOSS_EPS), one - dt(LOSS_EPS))
    g = P - Y
    if activation == "softmax":
        return -(Y * np.log(Pc)), g
    bce = -(Y * np.log(Pc) + (one - Y) * np.log(one - Pc))
    if loss != "focal":
        return bce, g
    gamma = dt(np.float32(focal_gamma))
    q = one - (Y * Pc + (one - Y) * (one - Pc))
    f = np.exp(gamma * np.log(q))
    return f * bce, f * g - gamma * (f / q) * (dt(2.0) * Y - one) * Pc * (one - Pc) * bce


def probe_loss(P: np.ndarray, Y: np.ndarray, activation: str, *, loss="auto", focal_gamma=2.0, sample_weight=None):
    """Keras' loss on probabilities: mean binary cross-entropy over rows x classes, or mean categorical cross-entropy over rows.
    ``loss="focal"`` (sigmoid only): the focal form of the element loss (``_loss_elements``).  ``sample_weight [rows]`` multiplies the
    elements of its row; the mean still divides by rows x classes (or rows): Keras' ``sum_over_batch_size``, not the sum of the weights."""
    one = P.dtype.type(1.0)
    if loss == "auto" and sample_weight is None:
        Pc = np.clip(P, P.dtype.type(LOSS_EPS), one - P.dtype.type(LOSS_EPS))
        if activation == "softmax":
            return -(Y * np.log(Pc)).sum() / P.dtype.type(P.shape[0])
        return -(Y * np.log(Pc) + (one - Y) * np.log(one - Pc)).sum() / P.dtype.type(P.size)
    loss, focal_gamma = _check_loss(loss, focal_gamma, activation)
    elem, _ = _loss_elements(P, Y, activation, loss, focal_gamma)
    if sample_weight is not None:
        elem = elem * np.asarray(sample_weight, P.dtype)[:, None]
    return elem.sum() / P.dtype.type(P.shape[0] if activation == "softmax" else P.size)


def probe_loss_gradient(P: np.ndarray, Y: np.ndarray, activation: str, *, loss="auto", focal_gamma=2.0, sample_weight=None) -> np.ndarray:
    """``dLoss/dlogits [rows, C]`` of ``probe_loss`` with the same arguments, the mean's scale applied: what the forward kernel writes
    as ``G``.  (Cross-entropy: ``p - y``, which for softmax is the derivative when the targets of a row sum to 1.)"""
    scale = P.dtype.type(P.shape[0] if activation == "softmax" else P.size)
    if loss == "auto" and sample_weight is None:
        return (P - Y) / scale
    loss, focal_gamma = _check_loss(loss, focal_gamma, activation)
    _, g = _loss_elements(P, Y, activation, loss, focal_gamma)
    if sample_weight is not None:
        g = g * np.asarray(sample_weight, P.dtype)[:, None]
    return g / scale


def balanced_class_weights(paths: list, classes: list) -> np.ndarray:
    """The reference's balanced class weights (cli/train.py): ``total / (len(classes) * count)`` over the files of ``paths`` whose folder
    is a class, float64 ``[C]``.  A class without a file counts as 1, as the reference's ``label_counts.get(i, 1)`` does."""
    col = {c: i for i, c in enumerate(classes)}
    counts = np.zeros(len(classes), np.int64)
    for p in paths:
        i = col.get(os.path.basename(os.path.dirname(p)), -1)
        if i >= 0:
            counts[i] += 1
    return float(counts.sum()) / (len(classes) * np.maximum(counts, 1).astype(np.float64))


def row_weights(Y: np.ndarray, class_weights: np.ndarray) -> np.ndarray:
    """One weight per row, float32 ``[N]``: ``class_weights[argmax(Y[i])]`` for rows with a positive target (the first maximum, as
    Keras' ``class_weight`` takes it), ``1.0`` for all-zero rows (the noise folders).  A departure from Keras, which takes ``argmax`` of
    an all-zero row too and so gives the noise rows class 0's weight by accident."""
    Y = np.asarray(Y)
    w = np.asarray(class_weights, np.float64)[np.argmax(Y, axis=1)]
    return np.where(Y.max(axis=1) > 0, w, 1.0).astype(np.float32)


def upsample_rows(file_index: np.ndarray, multiplicity: np.ndarray) -> np.ndarray:
    """Row numbers for ``rows=``: every row repeated by the multiplicity of its file, in ascending row order (int32)."""
    file_index = np.asarray(file_index, np.int64)
    return np.repeat(np.arange(file_index.shape[0], dtype=np.int32), np.asarray(multiplicity, np.int64)[file_index])


def _check_weights_rows(n: int, sample_weight, rows) -> tuple:
    """``sample_weight`` as float32 ``[n]`` and ``rows`` as int32 ``[M]`` (or ``None`` each), refused when of another shape or out of range."""
    if sample_weight is not None:
        sample_weight = np.asarray(sample_weight)
        if sample_weight.shape != (n,) or sample_weight.dtype.kind not in "fiu":
            raise ValueError(f"sample_weight must be one number per row of X, shape ({n},), got {sample_weight.shape}")
        sample_weight = np.ascontiguousarray(sample_weight, np.float32)
        if not (np.isfinite(sample_weight).all() and (sample_weight >= 0).all()):
            raise ValueError("sample_weight must be finite and >= 0")
    if rows is not None:
        rows = np.asarray(rows)
        if rows.ndim != 1 or rows.shape[0] < 1 or rows.dtype.kind not in "iu":
            raise ValueError(f"rows must be a non-empty 1-D integer array of row numbers into X, got shape {rows.shape} of {rows.dtype}")
        if rows.min() < 0 or rows.max() >= n:
            raise ValueError(f"rows must lie in 0..{n - 1}")
        if rows.shape[0] > 0x7FFFFFFF:
            raise ValueError("rows is too long")
        rows = np.ascontiguousarray(rows, np.int32)
    return sample_weight, rows


def optimizer_step(params: np.ndarray, g: np.ndarray, state: dict, optimizer: str, lr_t, alpha_t, weight_decay=0.0, eps=ADAM_EPS) -> np.ndarray:
    """One update of ``params`` (any shape) in their dtype; ``state`` holds ``m`` / ``v`` (zeros at the start)."""
    dt = params.dtype.type
    if optimizer == "sgd":
        state["m"] = dt(MOMENTUM) * state["m"] - dt(lr_t) * g
        return params + state["m"]
    if optimizer == "adamw":
        params = params - dt(lr_t) * dt(weight_decay) * params
    # 1 - beta is formed in float64 and then cast (0.1, 0.001 to the nearest value of the dtype, as the kernel's constants are):
    # 1 - 0.999 formed in float32 would be 1.3e-5 off, a bias that is no rounding of the procedure
    state["m"] = state["m"] + (g - state["m"]) * dt(1.0 - BETA_1)
    state["v"] = state["v"] + (g * g - state["v"]) * dt(1.0 - BETA_2)
    return params - state["m"] * dt(alpha_t) / (np.sqrt(state["v"]) + dt(eps))


def clip_by_global_norm(g: np.ndarray, clipnorm: float) -> np.ndarray:
    if not clipnorm > 0:
        return g
    norm = np.sqrt((g * g).sum())
    return g * (g.dtype.type(clipnorm) / norm) if norm > g.dtype.type(clipnorm) else g


def _check_fit_args(X, Y, activation, optimizer, batch_size, dropout, epochs):
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be one of {ACTIVATIONS}, not {activation!r}")
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer must be one of {OPTIMIZERS}, not {optimizer!r}")
    if len(X.shape) != 2 or len(Y.shape) != 2 or X.shape[0] != Y.shape[0] or X.shape[0] < 1:
        raise ValueError(f"X must be [N, D] and Y [N, C] with the same N >= 1, got {tuple(X.shape)} and {tuple(Y.shape)}")
    if not 1 <= int(batch_size):
        raise ValueError("batch_size must be >= 1")
    if not 0.0 <= float(dropout) < 1.0:
        raise ValueError("dropout must be in [0, 1)")
    if int(epochs) < 1:
        raise ValueError("epochs must be >= 1")


def _check_label_smoothing(label_smoothing):
    if not 0.0 <= float(label_smoothing) < 1.0:
        raise ValueError("label_smoothing must be in [0, 1)")
    return float(label_smoothing)


def _epoch_rows(seed: int, epoch: int, n: int, rows) -> np.ndarray:
    """The row numbers of epoch ``epoch`` in training order: a permutation of ``0 .. n-1``, or of the entries of ``rows`` (``n = len(rows)``)."""
    perm = epoch_permutation(seed, epoch, n)
    return perm if rows is None else np.ascontiguousarray(rows[perm])


@dataclass(frozen=True)
class _FitPlan:
    """What every fit knows once its arguments are checked (``_plan_fit``)."""

    activation: str
    optimizer: str      # a sweep: the first trial's, like ``dropout``; its trials carry their own hyperparameters
    lr: float
    weight_decay: float
    clipnorm: float
    dropout: float
    label_smoothing: float
    loss: str
    focal_gamma: float
    sample_weight: np.ndarray | None   # float32 [n]
    rows: np.ndarray | None            # int32 [m]
    n: int              # rows of X
    D: int
    C: int
    m: int              # the length of an epoch: n, or len(rows)
    batch: int
    epochs: int
    patience: int
    seed: int
    total: int          # steps of the schedule
    has_val: bool
    W0: np.ndarray | None   # the initial head; None in the plan of a fit that hands over to a sweep
    b0: np.ndarray | None
    hidden: int = 0         # hidden units; > 0: W0 / b0 are the output layer [hidden, C], W1_0 / b1_0 the hidden layer [D, hidden]
    W1_0: np.ndarray | None = None
    b1_0: np.ndarray | None = None


def _plan_fit(X, Y, X_val, *, device: bool, activation, optimizer, batch_size, dropout, epochs, learning_rate=1e-3, weight_decay=0.0, clipnorm=1.0,
              patience=10, seed=42, label_smoothing=0.0, loss="auto", focal_gamma=2.0, sample_weight=None, rows=None, hidden_units=0) -> _FitPlan:
    """The checks every fit runs, in one order, and what follows from the arguments.  ``X``: anything with the ``shape`` of the training
    rows.  ``device``: the fit runs on the device, which takes D and C up to ``_hip.PROBE_MAX_D`` / ``PROBE_MAX_C`` and ``clipnorm`` as the
    Python float; the numpy fits round ``clipnorm`` through float32, as the C ABI does."""
    _check_fit_args(X, Y, activation, optimizer, batch_size, dropout, epochs)
    if not device:
        label_smoothing = _check_label_smoothing(label_smoothing)
    loss, focal_gamma = _check_loss(loss, focal_gamma, activation)
    n, D, C = int(X.shape[0]), int(X.shape[1]), int(Y.shape[1])
    sample_weight, rows = _check_weights_rows(n, sample_weight, rows)
    W0 = b0 = W1_0 = b1_0 = None
    H = check_hidden_units(hidden_units, device)
    if device:
        from birdnet_stm32 import _hip

        label_smoothing = _check_label_smoothing(label_smoothing)
    # A single device fit with smoothing runs as a sweep of one trial, which makes its own plan: the D/C refusal and the head are that one's
    # (with a hidden layer it does not: the targets are smoothed once on the host)
    if H > 0 or not (device and label_smoothing > 0):
        if device and not (1 <= D <= _hip.PROBE_MAX_D and 1 <= C <= _hip.PROBE_MAX_C):
            raise ValueError(f"the device path takes 1 <= D <= {_hip.PROBE_MAX_D} and 1 <= C <= {_hip.PROBE_MAX_C}, got D={D} C={C}")
        if H > 0:
            W1_0, b1_0, W0, b0 = init_mlp_head(D, H, C, seed)
        else:
            W0, b0 = init_head(D, C, seed)
    m = n if rows is None else len(rows)
    batch = min(int(batch_size), m)
    return _FitPlan(activation=activation, optimizer=optimizer, lr=float(learning_rate), weight_decay=float(weight_decay),
                    clipnorm=float(clipnorm) if device else float(np.float32(clipnorm)), dropout=float(dropout), label_smoothing=label_smoothing,
                    loss=loss, focal_gamma=focal_gamma, sample_weight=sample_weight, rows=rows, n=n, D=D, C=C, m=m, batch=batch, epochs=int(epochs),
                    patience=int(patience), seed=int(seed), total=int(epochs) * math.ceil(m / batch), has_val=X_val is not None and len(X_val) > 0,
                    W0=W0, b0=b0, hidden=H, W1_0=W1_0, b1_0=b1_0)


class _EarlyStopping:
    """Keras' ``EarlyStopping(patience)`` on the validation loss of one head, and the ``history`` its fit returns."""

    def __init__(self, patience: int):
        self.patience, self.best, self.wait = patience, math.inf, 0
        self.history = {"loss": [], "val_loss": [], "step_loss": [], "best_epoch": None, "stopped_epoch": None}

    def add_epoch(self, step_losses) -> None:
        losses = np.ascontiguousarray(step_losses, np.float64)
        self.history["step_loss"].append(losses)
        self.history["loss"].append(float(losses.mean()))

    def update(self, epoch: int, val: float) -> tuple[bool, bool]:
        """``(improved, stop)`` after epoch ``epoch`` gave the validation loss ``val``."""
        self.history["val_loss"].append(val)
        if val < self.best:
            self.best, self.wait, self.history["best_epoch"] = val, 0, epoch
            return True, False
        self.wait += 1
        stop = self.wait >= self.patience and epoch > 0
        if stop:
            self.history["stopped_epoch"] = epoch
        return False, stop

    def finish(self) -> dict:
        self.history["step_loss"] = np.concatenate(self.history["step_loss"])
        return self.history


def _fit_loop(backend, plan: _FitPlan) -> dict:
    """Epochs, validation and early stopping with the best weights restored, shared by the device and the numpy fit.  ``backend``:
    ``epoch(perm) -> step losses``, ``val_loss()``, ``get() -> (W, b)``, ``set(W, b)``."""
    stopping, best_weights = _EarlyStopping(plan.patience), None
    for epoch in range(plan.epochs):
        stopping.add_epoch(backend.epoch(_epoch_rows(plan.seed, epoch, plan.m, plan.rows)))
        if not plan.has_val:
            continue
        improved, stop = stopping.update(epoch, float(backend.val_loss()))
        if improved:
            best_weights = backend.get()
        if stop:
            break
    if best_weights is not None:
        backend.set(*best_weights)
    return stopping.finish()


# -- the result -----------------------------------------------------------------------------------------------------------------------
@dataclass
class ProbeHead:
    """A trained head: ``scores = act(x W + b)`` over embedding rows of width ``embedding_dim``.  With a hidden layer (``W1 [D, H]``,
    ``b1 [H]``; ``hidden_units = H``): ``scores = act(relu(x W1 + b1) W + b)``, and ``W [H, C]``, ``b`` are the output layer."""

    W: np.ndarray
    b: np.ndarray
    activation: str = "sigmoid"
    class_names: list = field(default_factory=list)
    history: dict = field(default_factory=dict)
    W1: np.ndarray | None = None
    b1: np.ndarray | None = None

    def __post_init__(self):
        self.W = np.ascontiguousarray(self.W, np.float32)
        self.b = np.ascontiguousarray(self.b, np.float32)
        if self.W.ndim != 2 or self.b.shape != (self.W.shape[1],):
            raise ValueError(f"W must be [D, C] and b [C], got {self.W.shape} and {self.b.shape}")
        if (self.W1 is None) != (self.b1 is None):
            raise ValueError("a hidden layer is W1 and b1 together")
        if self.W1 is not None:
            self.W1 = np.ascontiguousarray(self.W1, np.float32)
            self.b1 = np.ascontiguousarray(self.b1, np.float32)
            if self.W1.ndim != 2 or self.b1.shape != (self.W1.shape[1],) or self.W1.shape[1] != self.W.shape[0]:
                raise ValueError(f"W1 must be [D, H], b1 [H] and W [H, C], got {self.W1.shape}, {self.b1.shape} and {self.W.shape}")
        if self.activation not in ACTIVATIONS:
            raise ValueError(f"activation must be one of {ACTIVATIONS}, not {self.activation!r}")
        self.class_names = [str(c) for c in self.class_names]
        if self.class_names and len(self.class_names) != self.W.shape[1]:
            raise ValueError(f"{len(self.class_names)} class names for {self.W.shape[1]} classes")
        self._device = {}   # per device index: [own context or None, W, b (, W1, b1) on the device]; they are fixed once the head exists

    @property
    def embedding_dim(self) -> int:
        return int((self.W if self.W1 is None else self.W1).shape[0])

    @property
    def hidden_units(self) -> int:
        return 0 if self.W1 is None else int(self.W1.shape[1])

    @property
    def num_classes(self) -> int:
        return int(self.W.shape[1])

    def check_embedding_dim(self, dim: int) -> None:
        if int(dim) != self.embedding_dim:
            raise ValueError(f"the head was trained on embeddings of width {self.embedding_dim}, the model's are {int(dim)} wide")

    def save(self, path: str) -> None:
        """A plain ``.npz`` (``np.load(path)`` reads it without this package)."""
        hist = {k: np.asarray(v, np.float64) for k, v in self.history.items() if k in ("loss", "val_loss")}
        hidden = {} if self.W1 is None else {"W1": self.W1, "b1": self.b1, "hidden_units": np.int64(self.hidden_units)}
        np.savez(path, W=self.W, b=self.b, activation=np.str_(self.activation), class_names=np.asarray(self.class_names, dtype=np.str_),
                 embedding_dim=np.int64(self.embedding_dim), **hidden, **{f"history_{k}": v for k, v in hist.items()})

    @classmethod
    def load(cls, path: str) -> "ProbeHead":
        with np.load(path, allow_pickle=False) as z:
            hist = {k[len("history_"):]: z[k].tolist() for k in z.files if k.startswith("history_")}
            hidden = ("W1" in z.files, "b1" in z.files, "hidden_units" in z.files)
            if any(hidden) and not all(hidden):
                raise ValueError(f"{path}: a hidden layer is W1, b1 and hidden_units together")
            head = cls(z["W"], z["b"], str(z["activation"]), [str(c) for c in z["class_names"]], hist, *((z["W1"], z["b1"]) if all(hidden) else ()))
            if all(hidden) and int(z["hidden_units"]) != head.hidden_units:
                raise ValueError(f"{path}: hidden_units {int(z['hidden_units'])} does not match W1 {head.W1.shape}")
            if "embedding_dim" in z.files and int(z["embedding_dim"]) != head.embedding_dim:
                raise ValueError(f"{path}: embedding_dim {int(z['embedding_dim'])} does not match {'W' if head.W1 is None else 'W1'} "
                                 f"{(head.W if head.W1 is None else head.W1).shape}")
        return head

    def close(self) -> None:
        """Drop the device copies of ``W`` / ``b`` and close the contexts ``predict`` opened for itself (none when it was given one)."""
        for slot in self._device.values():
            if slot[0] is not None:
                slot[0].close()
        self._device = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def predict_device(self, emb, ctx=None):
        """Scores ``[N, C]`` of a contiguous float32 CUDA tensor ``[N, D]`` (``bn_head_forward``; with a hidden layer
        ``bn_head_mlp_forward``), as a CUDA tensor.  ``ctx``: the
        caller's ``_hip.Context`` (a runner's ``ctx``); without one the head opens its own per device and keeps it until ``close()``."""
        import ctypes

        import torch

        from birdnet_stm32 import _hip

        if not (emb.is_cuda and emb.dtype == torch.float32 and emb.dim() == 2 and emb.is_contiguous()):
            raise ValueError("embeddings must be a contiguous float32 CUDA tensor [N, D]")
        self.check_embedding_dim(emb.shape[1])
        dev = emb.device.index or 0
        if dev not in self._device:
            self._device[dev] = [None, *(torch.from_numpy(a).to(emb.device) for a in ((self.W, self.b) if self.W1 is None else (self.W, self.b, self.W1, self.b1)))]
        slot = self._device[dev]
        if ctx is None:
            ctx = slot[0] = slot[0] or _hip.Context(dev, 1)
        out = torch.empty((emb.shape[0], self.num_classes), dtype=torch.float32, device=emb.device)
        with torch.cuda.device(emb.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(emb.device).cuda_stream)
            if self.W1 is not None:
                _hip.check(ctx.lib.bn_head_mlp_forward(ctx.handle, emb.data_ptr(), emb.shape[0], self.embedding_dim, slot[3].data_ptr(), slot[4].data_ptr(),
                                                       self.hidden_units, slot[1].data_ptr(), slot[2].data_ptr(), self.num_classes,
                                                       _hip.PROBE_ACTIVATIONS[self.activation], out.data_ptr(), stream))
                return out
            _hip.check(ctx.lib.bn_head_forward(ctx.handle, emb.data_ptr(), emb.shape[0], self.embedding_dim, slot[1].data_ptr(), slot[2].data_ptr(),
                                               self.num_classes, _hip.PROBE_ACTIVATIONS[self.activation], out.data_ptr(), stream))
        return out

    def predict(self, embeddings, ctx=None, device: int = 0):
        """Scores of embedding rows: a numpy array in gives a numpy array, a CUDA tensor a CUDA tensor.  Always on the device."""
        import torch

        if isinstance(embeddings, np.ndarray):
            emb = torch.from_numpy(np.ascontiguousarray(embeddings, np.float32)).to(f"cuda:{getattr(ctx, 'device', device)}")
            return self.predict_device(emb, ctx).cpu().numpy()
        return self.predict_device(embeddings, ctx)


# -- the specification ----------------------------------------------------------------------------------------------------------------
class _NumpyBackend:
    def __init__(self, X, Y, X_val, Y_val, plan, dtype):
        cast = lambda a: None if a is None else np.asarray(a).astype(dtype)  # noqa: E731
        self.X, self.Y, self.plan, self.dt = cast(X), cast(Y), plan, np.dtype(dtype).type
        self.Xv, self.Yv = (cast(X_val), cast(Y_val)) if plan.has_val else (None, None)
        self.w = cast(plan.sample_weight)   # [rows of X], indexed like Y
        self.loss_kw = dict(loss=plan.loss, focal_gamma=plan.focal_gamma)
        self.set(plan.W0, plan.b0)
        self.state = {"m": np.zeros_like(self.P), "v": np.zeros_like(self.P)}
        self.t = 0

    def epoch(self, perm):
        c, dt, D = self.plan, self.dt, self.X.shape[1]
        losses = []
        for s in range(0, len(perm), c.batch):
            idx = perm[s : s + c.batch]
            B = len(idx)
            xd = np.concatenate([self.X[idx] * dropout_mask(c.seed, self.t, B, D, c.dropout, dt), np.ones((B, 1), dt)], axis=1)
            P = head_scores(xd[:, :D], self.P[:D], self.P[D], c.activation)
            y = self.Y[idx]
            if c.label_smoothing > 0:
                y = smooth_targets(y, c.label_smoothing, c.activation)
            w = None if self.w is None else self.w[idx]
            losses.append(float(probe_loss(P, y, c.activation, sample_weight=w, **self.loss_kw)))
            G = probe_loss_gradient(P, y, c.activation, sample_weight=w, **self.loss_kw)
            g = clip_by_global_norm(xd.T @ G, c.clipnorm)
            lr_t, alpha_t = step_sizes(c.lr, self.t, c.total)
            self.P = optimizer_step(self.P, g, self.state, c.optimizer, np.float32(lr_t), np.float32(alpha_t), np.float32(c.weight_decay))
            self.t += 1
        return losses

    def val_loss(self):   # the loss that was asked for, never weighted, never smoothed
        D = self.P.shape[0] - 1
        return probe_loss(head_scores(self.Xv, self.P[:D], self.P[D], self.plan.activation), self.Yv, self.plan.activation, **self.loss_kw)

    def get(self):
        return self.P[:-1].copy(), self.P[-1].copy()

    def set(self, W, b):
        self.P = np.concatenate([W, b[None, :]]).astype(self.dt)


class _NumpyMlpBackend(_NumpyBackend):
    """The head with a hidden layer: the parameters are one vector ``[(D + 1) H | (H + 1) C]``, so clip and optimiser see one norm and one
    schedule; a step is ``mlp_loss_and_gradient``.  The training targets are smoothed once, here; the validation loss takes them raw."""

    def __init__(self, X, Y, X_val, Y_val, plan, dtype):
        cast = lambda a: None if a is None else np.asarray(a).astype(dtype)  # noqa: E731
        self.X, self.Y, self.plan, self.dt = cast(X), cast(Y), plan, np.dtype(dtype).type
        self.Xv, self.Yv = (cast(X_val), cast(Y_val)) if plan.has_val else (None, None)
        self.w = cast(plan.sample_weight)
        self.loss_kw = dict(loss=plan.loss, focal_gamma=plan.focal_gamma)
        self.Yt = smooth_targets(self.Y, plan.label_smoothing, plan.activation) if plan.label_smoothing > 0 else self.Y
        self.D, self.H, self.C = self.X.shape[1], plan.hidden, self.Y.shape[1]
        self.set(plan.W1_0, plan.b1_0, plan.W0, plan.b0)
        self.state = {"m": np.zeros_like(self.P), "v": np.zeros_like(self.P)}
        self.t = 0

    def epoch(self, perm):
        c, dt, D, H = self.plan, self.dt, self.D, self.H
        losses = []
        for s in range(0, len(perm), c.batch):
            idx = perm[s : s + c.batch]
            B = len(idx)
            xd = np.concatenate([self.X[idx] * dropout_mask(c.seed, self.t, B, D, c.dropout, dt), np.ones((B, 1), dt)], axis=1)
            m2 = dropout_mask(c.seed ^ DROP2_SEED_XOR, self.t, B, H, c.dropout, dt)
            w = None if self.w is None else self.w[idx]
            value, g, _ = mlp_loss_and_gradient(self.P, xd, m2, self.Yt[idx], c.activation, sample_weight=w, **self.loss_kw)
            losses.append(float(value))
            g = clip_by_global_norm(g, c.clipnorm)
            lr_t, alpha_t = step_sizes(c.lr, self.t, c.total)
            self.P = optimizer_step(self.P, g, self.state, c.optimizer, np.float32(lr_t), np.float32(alpha_t), np.float32(c.weight_decay))
            self.t += 1
        return losses

    def val_loss(self):   # the loss that was asked for, never weighted, never smoothed
        return probe_loss(mlp_forward(self.Xv, *self.get(), self.plan.activation), self.Yv, self.plan.activation, **self.loss_kw)

    def get(self):
        D, H, C = self.D, self.H, self.C
        P1, P2 = self.P[: (D + 1) * H].reshape(D + 1, H), self.P[(D + 1) * H :].reshape(H + 1, C)
        return P1[:D].copy(), P1[D].copy(), P2[:H].copy(), P2[H].copy()

    def set(self, W1, b1, W2, b2):
        self.P = np.concatenate([np.asarray(W1).ravel(), np.asarray(b1).ravel(), np.asarray(W2).ravel(), np.asarray(b2).ravel()]).astype(self.dt)


def fit_probe_reference(X, Y, X_val=None, Y_val=None, *, activation="sigmoid", epochs=50, batch_size=32, learning_rate=1e-3, optimizer="adam",
                        weight_decay=0.0, clipnorm=1.0, dropout=0.5, patience=10, seed=42, dtype=np.float64, class_names=None,
                        label_smoothing=0.0, loss="auto", focal_gamma=2.0, sample_weight=None, rows=None, hidden_units=0) -> ProbeHead:
    """The procedure of ``fit_probe`` in numpy, all arithmetic in ``dtype``.  ``history["W"]`` / ``["b"]`` keep the result in ``dtype``
    (with ``hidden_units > 0`` also ``["W1"]`` / ``["b1"]``).  ``loss`` / ``focal_gamma`` / ``sample_weight`` / ``rows`` / ``hidden_units``: see
    ``fit_probe``."""
    X, Y = np.asarray(X), np.asarray(Y)
    plan = _plan_fit(X, Y, X_val, device=False, activation=activation, optimizer=optimizer, batch_size=batch_size, dropout=dropout, epochs=epochs,
                     learning_rate=learning_rate, weight_decay=weight_decay, clipnorm=clipnorm, patience=patience, seed=seed,
                     label_smoothing=label_smoothing, loss=loss, focal_gamma=focal_gamma, sample_weight=sample_weight, rows=rows,
                     hidden_units=hidden_units)
    if plan.hidden > 0:
        be = _NumpyMlpBackend(X, Y, X_val, Y_val, plan, dtype)
        history = _fit_loop(be, plan)
        W1, b1, W, b = be.get()
        history.update(W1=W1, b1=b1, W=W, b=b)
        return ProbeHead(W, b, plan.activation, list(class_names or []), history, W1, b1)
    return _reference_fit(_NumpyBackend(X, Y, X_val, Y_val, plan, dtype), plan, class_names)


def _reference_fit(be, plan: _FitPlan, class_names) -> ProbeHead:
    history = _fit_loop(be, plan)
    W, b = be.get()
    history["W"], history["b"] = W, b
    return ProbeHead(W, b, plan.activation, list(class_names or []), history)


# -- the device fit -------------------------------------------------------------------------------------------------------------------
class _DeviceBackend:
    """``bn_probe_*`` over resident ``X`` / ``Y``.  ``self.n`` is the number of rows of ``X``, ``self.m`` the length of an epoch: the two
    differ when the epoch runs over ``rows`` with repeats (``plan.m``).  ``per_trial``: ``()``, or ``(T,)`` in a sweep: the shape of one
    step's loss and of the validation loss."""

    SET_LOSS, DESTROY = "bn_probe_set_loss", "bn_probe_destroy"

    def __init__(self, ctx, X, Y, X_val, Y_val, plan, per_trial=()):
        import ctypes

        import torch

        from birdnet_stm32 import _hip

        self.torch, self.hip, self.ctx, self.plan = torch, _hip, ctx, plan
        self.dev = torch.device(f"cuda:{ctx.device}")
        self.X, self.Y = self._dev(X), self._dev(Y)
        self.Xv, self.Yv = (self._dev(X_val), self._dev(Y_val)) if plan.has_val else (None, None)
        self.W, self.b, self.w = self._dev(plan.W0), self._dev(plan.b0), self._dev(plan.sample_weight)
        self.n, self.D = self.X.shape
        self.C, self.m = self.Y.shape[1], plan.m
        if self.w is not None and tuple(self.w.shape) != (self.n,):
            raise ValueError(f"sample_weight must have shape ({self.n},), got {tuple(self.w.shape)}")
        self.steps = math.ceil(self.m / plan.batch)
        self.step_loss = torch.empty((self.steps, *per_trial), dtype=torch.float32, device=self.dev)
        self.val = torch.empty(per_trial or 1, dtype=torch.float32, device=self.dev)
        self.handle = ctypes.c_void_p()
        with torch.cuda.device(self.dev):
            _hip.check(self._create(ctypes.byref(self.handle)))
        if plan.loss != "auto":   # (the default is the handle's own: nothing to set)
            try:
                _hip.check(getattr(ctx.lib, self.SET_LOSS)(self.handle, _hip.PROBE_LOSSES[plan.loss], plan.focal_gamma))
            except Exception:
                self.close()
                raise

    def _create(self, out):
        c, hip = self.plan, self.hip
        return self.ctx.lib.bn_probe_create(self.ctx.handle, self.D, self.C, hip.PROBE_ACTIVATIONS[c.activation], hip.PROBE_OPTIMIZERS[c.optimizer], c.lr,
                                            c.weight_decay, c.clipnorm, c.dropout, c.seed & 0xFFFFFFFF, c.total, self.W.data_ptr(), self.b.data_ptr(),
                                            out, self._stream())

    def _dev(self, a):
        if a is None:
            return None
        if isinstance(a, np.ndarray):
            a = self.torch.from_numpy(np.ascontiguousarray(a, np.float32))
        return a.to(self.dev, self.torch.float32).contiguous()

    def _stream(self):
        import ctypes

        return ctypes.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    @staticmethod
    def _ptr(t):
        return None if t is None else t.data_ptr()

    def _check_perm(self, perm):
        if perm.shape != (self.m,) or perm.dtype != np.int32:
            raise ValueError(f"an epoch takes {self.m} int32 row numbers, got {perm.shape} of {perm.dtype}")

    def epoch(self, perm):
        self._check_perm(perm)
        with self.torch.cuda.device(self.dev):
            d_perm = self.torch.from_numpy(perm).to(self.dev)
            self.hip.check(self.ctx.lib.bn_probe_epoch_weighted(self.handle, self.X.data_ptr(), self.Y.data_ptr(), self._ptr(self.w), d_perm.data_ptr(),
                                                                self.m, self.plan.batch, self.step_loss.data_ptr(), self._stream()))
            return self.step_loss.cpu().numpy()   # (synchronises: d_perm outlives the epoch)

    def val_loss(self):
        with self.torch.cuda.device(self.dev):
            self.hip.check(self.ctx.lib.bn_probe_loss(self.handle, self.Xv.data_ptr(), self.Yv.data_ptr(), self.Xv.shape[0], self.val.data_ptr(), self._stream()))
            return float(self.val.item())

    def get(self):
        W, b = self.torch.empty_like(self.W), self.torch.empty_like(self.b)
        with self.torch.cuda.device(self.dev):
            self.hip.check(self.ctx.lib.bn_probe_get(self.handle, W.data_ptr(), b.data_ptr(), self._stream()))
        return W, b

    def set(self, W, b):
        with self.torch.cuda.device(self.dev):
            self.hip.check(self.ctx.lib.bn_probe_set(self.handle, W.data_ptr(), b.data_ptr(), self._stream()))
            self.torch.cuda.current_stream(self.dev).synchronize()

    def close(self):
        if self.handle:
            self.torch.cuda.synchronize(self.dev)
            getattr(self.ctx.lib, self.DESTROY)(self.handle)
            self.handle = None


class _MlpDeviceBackend(_DeviceBackend):
    """``bn_probe_mlp_*`` over resident ``X`` / ``Y``: ``self.W`` / ``self.b`` are the output layer, ``self.W1`` / ``self.b1`` the hidden one.
    ``Y`` is what the steps train on (smoothed by the caller when asked for), ``Y_val`` the raw validation targets."""

    SET_LOSS, DESTROY = "bn_probe_mlp_set_loss", "bn_probe_mlp_destroy"

    def _create(self, out):
        c, hip = self.plan, self.hip
        self.W1, self.b1 = self._dev(c.W1_0), self._dev(c.b1_0)
        return self.ctx.lib.bn_probe_mlp_create(self.ctx.handle, self.D, c.hidden, self.C, hip.PROBE_ACTIVATIONS[c.activation],
                                                hip.PROBE_OPTIMIZERS[c.optimizer], c.lr, c.weight_decay, c.clipnorm, c.dropout, c.seed & 0xFFFFFFFF, c.total,
                                                self.W1.data_ptr(), self.b1.data_ptr(), self.W.data_ptr(), self.b.data_ptr(), out, self._stream())

    def epoch(self, perm):
        self._check_perm(perm)
        with self.torch.cuda.device(self.dev):
            d_perm = self.torch.from_numpy(perm).to(self.dev)
            self.hip.check(self.ctx.lib.bn_probe_mlp_epoch_weighted(self.handle, self.X.data_ptr(), self.Y.data_ptr(), self._ptr(self.w), d_perm.data_ptr(),
                                                                    self.m, self.plan.batch, self.step_loss.data_ptr(), self._stream()))
            return self.step_loss.cpu().numpy()   # (synchronises: d_perm outlives the epoch)

    def val_loss(self):
        with self.torch.cuda.device(self.dev):
            self.hip.check(self.ctx.lib.bn_probe_mlp_loss(self.handle, self.Xv.data_ptr(), self.Yv.data_ptr(), self.Xv.shape[0], self.val.data_ptr(),
                                                          self._stream()))
            return float(self.val.item())

    def get(self):
        out = [self.torch.empty_like(t) for t in (self.W1, self.b1, self.W, self.b)]
        with self.torch.cuda.device(self.dev):
            self.hip.check(self.ctx.lib.bn_probe_mlp_get(self.handle, *(t.data_ptr() for t in out), self._stream()))
        return tuple(out)

    def set(self, W1, b1, W, b):
        with self.torch.cuda.device(self.dev):
            self.hip.check(self.ctx.lib.bn_probe_mlp_set(self.handle, W1.data_ptr(), b1.data_ptr(), W.data_ptr(), b.data_ptr(), self._stream()))
            self.torch.cuda.current_stream(self.dev).synchronize()


def _mlp_device_fit(ctx, X, Y, X_val, Y_val, plan: _FitPlan, class_names) -> ProbeHead:
    """``fit_probe`` with a hidden layer: the targets smoothed once on the host, then epochs, the best weights, the head."""
    if plan.label_smoothing > 0:
        import torch

        Y = smooth_targets(np.ascontiguousarray(Y.cpu().numpy() if isinstance(Y, torch.Tensor) else Y, np.float32), plan.label_smoothing, plan.activation)
    be = _MlpDeviceBackend(ctx, X, Y, X_val, Y_val, plan)
    try:
        history = _fit_loop(be, plan)
        W1, b1, W, b = (t.cpu().numpy() for t in be.get())
    finally:
        be.close()
    return ProbeHead(W, b, plan.activation, list(class_names or []), history, W1, b1)


def _device_fit(be, plan: _FitPlan, class_names) -> ProbeHead:
    """The fit on a device backend made for ``plan``, which it closes: epochs, the best weights, the head."""
    try:
        history = _fit_loop(be, plan)
        W, b = be.get()
        W, b = W.cpu().numpy(), b.cpu().numpy()
    finally:
        be.close()
    return ProbeHead(W, b, plan.activation, list(class_names or []), history)


def fit_probe(ctx_or_runner, X, Y, X_val=None, Y_val=None, *, activation="sigmoid", epochs=50, batch_size=32, learning_rate=1e-3, optimizer="adam",
              weight_decay=0.0, clipnorm=1.0, dropout=0.5, patience=10, seed=42, class_names=None, label_smoothing=0.0, loss="auto", focal_gamma=2.0,
              sample_weight=None, rows=None, hidden_units=0) -> ProbeHead:
    """Train ``scores = act(dropout(x) W + b)`` on embedding rows ``X [N, D]`` with targets ``Y [N, C]`` (float: one-hot, multi-hot or
    all-zero rows) on the device.  ``X`` / ``Y`` may be numpy arrays or CUDA tensors; they stay on the device for the whole fit, per epoch
    the host uploads one permutation and reads back the per-step losses.  The defaults are the reference CLI's.  The same inputs and seed
    give the same bits on every run.  ``label_smoothing > 0`` (``smooth_targets``) trains through the sweep's kernels as a sweep of one trial.

    For long-tailed sets, all off by default (the defaults run the launches, and give the bits, of a call without them):

    * ``loss="focal"`` with ``focal_gamma >= 0``: the focal form of the sigmoid head's loss (``probe_loss``), in training and in the
      validation loss.  Smoothing comes first: the focal loss sees the smoothed target.  Not with softmax.
    * ``sample_weight``: float ``[N]``, one weight per row of ``X`` (``row_weights``), multiplied into the training loss and its gradient;
      the means still divide by rows x classes (or rows).  The validation loss is never weighted.
    * ``rows``: int ``[M]``, row numbers into ``X``, repeats allowed (``upsample_rows``).  An epoch then runs over
      ``rows[epoch_permutation(seed, e, M)]``; the steps per epoch and the short last batch follow ``M``.  ``X``, ``Y`` and
      ``sample_weight`` are indexed through it and nothing is duplicated on the device.  The dropout draw is per position in the batch,
      so two copies of a row in one batch get different masks.

    ``hidden_units = H > 0`` trains ``scores = act(dropout2(relu(dropout(x) W1 + b1)) W2 + b2)`` instead (``bn_probe_mlp_*``): one ReLU layer of
    ``H`` units, ``1 <= H <= _hip.PROBE_MAX_D``, dropout at the same rate in front of both layers (the second mask is drawn with
    ``seed ^ DROP2_SEED_XOR``), one global norm and one schedule over all four arrays.  Everything above composes; label smoothing is
    applied to the training targets once on the host.  The head's ``W`` / ``b`` are then the output layer, ``W1`` / ``b1`` the hidden one."""
    plan = _plan_fit(X, Y, X_val, device=True, activation=activation, optimizer=optimizer, batch_size=batch_size, dropout=dropout, epochs=epochs,
                     learning_rate=learning_rate, weight_decay=weight_decay, clipnorm=clipnorm, patience=patience, seed=seed,
                     label_smoothing=label_smoothing, loss=loss, focal_gamma=focal_gamma, sample_weight=sample_weight, rows=rows,
                     hidden_units=hidden_units)
    if plan.hidden > 0:
        return _mlp_device_fit(getattr(ctx_or_runner, "ctx", ctx_or_runner), X, Y, X_val, Y_val, plan, class_names)
    if plan.label_smoothing > 0:
        trial = ProbeTrial(learning_rate=learning_rate, optimizer=optimizer, weight_decay=weight_decay, clipnorm=clipnorm, dropout=dropout,
                           label_smoothing=label_smoothing)
        return fit_probe_sweep(ctx_or_runner, X, Y, X_val, Y_val, [trial], activation=activation, epochs=epochs, batch_size=batch_size, patience=patience,
                               seed=seed, class_names=class_names, loss=plan.loss, focal_gamma=plan.focal_gamma, sample_weight=plan.sample_weight,
                               rows=plan.rows).heads[0]
    return _device_fit(_DeviceBackend(getattr(ctx_or_runner, "ctx", ctx_or_runner), X, Y, X_val, Y_val, plan), plan, class_names)


# -- many trials at once ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ProbeTrial:
    """The hyperparameters that differ between the trials of a sweep (the reference's search space, training/tuner.py)."""

    learning_rate: float = 1e-3
    optimizer: str = "adam"
    weight_decay: float = 0.0
    clipnorm: float = 1.0
    dropout: float = 0.5
    label_smoothing: float = 0.0

    def __post_init__(self):
        if self.optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {OPTIMIZERS}, not {self.optimizer!r}")
        if not float(self.learning_rate) >= 0 or not float(self.weight_decay) >= 0 or not float(self.clipnorm) >= 0:
            raise ValueError("learning_rate, weight_decay and clipnorm must be >= 0")
        if not 0.0 <= float(self.dropout) < 1.0:
            raise ValueError("dropout must be in [0, 1)")
        _check_label_smoothing(self.label_smoothing)

    def fit_kwargs(self) -> dict:
        """The trial as keyword arguments of ``fit_probe`` / ``fit_probe_reference``."""
        return dict(learning_rate=float(self.learning_rate), optimizer=self.optimizer, weight_decay=float(self.weight_decay), clipnorm=float(self.clipnorm),
                    dropout=float(self.dropout), label_smoothing=float(self.label_smoothing))


@dataclass
class SweepResult:
    """One ``ProbeHead`` per trial (``history`` as ``fit_probe``'s) and ``best``: the trial with the smallest best-epoch validation loss,
    the lower index on a tie; ``None`` without validation rows."""

    heads: list
    trials: list
    best: int | None = None

    @property
    def best_head(self) -> ProbeHead:
        return self.heads[self.best if self.best is not None else 0]


def _best_trial(heads: list) -> int | None:
    vals = [min(h.history["val_loss"]) if h.history.get("best_epoch") is not None else math.inf for h in heads]
    return int(np.argmin(vals)) if vals and min(vals) < math.inf else None


def _check_trials(trials) -> list:
    trials = list(trials)
    if not trials or not all(isinstance(t, ProbeTrial) for t in trials):
        raise ValueError("trials must be a non-empty list of ProbeTrial")
    return trials


class _SweepBackend(_DeviceBackend):
    """``bn_probe_sweep_*`` over resident ``X`` / ``Y``: every trial of the sweep takes the same step in the same launches."""

    SET_LOSS, DESTROY = "bn_probe_sweep_set_loss", "bn_probe_sweep_destroy"

    def __init__(self, ctx, X, Y, X_val, Y_val, plan, trials):
        self.trials, self.T, self.t = trials, len(trials), 0
        super().__init__(ctx, X, Y, X_val, Y_val, plan, per_trial=(self.T,))

    def _create(self, out):
        c, hip = self.plan, self.hip
        rows = (hip.ProbeTrialStruct * self.T)(*[hip.ProbeTrialStruct(hip.PROBE_OPTIMIZERS[t.optimizer], t.learning_rate, t.weight_decay, t.clipnorm,
                                                                      t.dropout, t.label_smoothing) for t in self.trials])
        return self.ctx.lib.bn_probe_sweep_create(self.ctx.handle, self.D, self.C, hip.PROBE_ACTIVATIONS[c.activation], self.T, rows, c.seed & 0xFFFFFFFF,
                                                  c.total, self.W.data_ptr(), self.b.data_ptr(), out, self._stream())

    def _mask(self, mask):
        return self.torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(self.dev)

    def epoch(self, perm, active):
        """One epoch of the active trials: step losses ``[steps, T]`` float32 (columns of inactive trials are not written)."""
        self._check_perm(perm)
        sizes = device_step_sizes([t.learning_rate for t in self.trials], self.t, self.steps, self.plan.total)
        with self.torch.cuda.device(self.dev):
            d_perm, d_sizes, d_active = self.torch.from_numpy(perm).to(self.dev), self.torch.from_numpy(sizes).to(self.dev), self._mask(active)
            self.hip.check(self.ctx.lib.bn_probe_sweep_epoch_weighted(self.handle, self.X.data_ptr(), self.Y.data_ptr(), self._ptr(self.w), d_perm.data_ptr(),
                                                                      self.m, self.plan.batch, d_sizes.data_ptr(), d_active.data_ptr(),
                                                                      self.step_loss.data_ptr(), self._stream()))
            self.t += self.steps
            return self.step_loss.cpu().numpy()   # (synchronises: the uploads outlive the epoch)

    def val_loss(self, active):
        with self.torch.cuda.device(self.dev):
            d_active = self._mask(active)
            self.hip.check(self.ctx.lib.bn_probe_sweep_loss(self.handle, self.Xv.data_ptr(), self.Yv.data_ptr(), self.Xv.shape[0], d_active.data_ptr(),
                                                            self.val.data_ptr(), self._stream()))
            return self.val.cpu().numpy()

    def snapshot(self, mask):
        with self.torch.cuda.device(self.dev):
            d_mask = self._mask(mask)
            self.hip.check(self.ctx.lib.bn_probe_sweep_snapshot(self.handle, d_mask.data_ptr(), self._stream()))
            self.torch.cuda.current_stream(self.dev).synchronize()

    def get(self, trial, snapshot=False):
        W, b = self.torch.empty_like(self.W), self.torch.empty_like(self.b)
        with self.torch.cuda.device(self.dev):
            self.hip.check(self.ctx.lib.bn_probe_sweep_get(self.handle, int(trial), self.hip.PROBE_SWEEP_SNAPSHOT if snapshot else self.hip.PROBE_SWEEP_CURRENT,
                                                           W.data_ptr(), b.data_ptr(), self._stream()))
        return W.cpu().numpy(), b.cpu().numpy()


def fit_probe_sweep(ctx_or_runner, X, Y, X_val=None, Y_val=None, trials=(), *, activation="sigmoid", epochs=50, batch_size=32, patience=10, seed=42,
                    class_names=None, loss="auto", focal_gamma=2.0, sample_weight=None, rows=None, hidden_units=0) -> SweepResult:
    """``fit_probe`` for every ``ProbeTrial`` of ``trials`` at once (at most ``_hip.PROBE_SWEEP_MAX_TRIALS``).  The trials share the rows, the
    initial weights, the permutations and the dropout draws; one training step of all of them is the launches of a single fit's step with
    the trial as one more grid axis, which is what makes a sweep cheap where one fit is launch-bound.  Early stopping is ``fit_probe``'s
    rule per trial: a stopped trial goes inactive (its weights and its best-epoch snapshot, kept on the device, no longer move) and the
    others go on.  A trial without label smoothing gives the bits of ``fit_probe`` with its hyperparameters: weights, bias, step losses
    and validation losses.  The validation loss is never smoothed, so trials compare.  ``loss`` / ``focal_gamma`` / ``sample_weight`` /
    ``rows`` are ``fit_probe``'s and shared by all trials (no part of a ``ProbeTrial``): a trial's smoothing comes first, the focal loss
    sees the smoothed target; the validation loss is the focal one, unweighted, unsmoothed."""
    from birdnet_stm32 import _hip

    refuse_hidden("fit_probe_sweep", hidden_units)
    trials = _check_trials(trials)
    if len(trials) > _hip.PROBE_SWEEP_MAX_TRIALS:
        raise ValueError(f"{len(trials)} trials: a sweep takes at most {_hip.PROBE_SWEEP_MAX_TRIALS}")
    # shapes, activation, batch and epochs; every trial's own fields were checked when it was made (ProbeTrial.__post_init__)
    plan = _plan_fit(X, Y, X_val, device=True, activation=activation, optimizer=trials[0].optimizer, batch_size=batch_size, dropout=trials[0].dropout,
                     epochs=epochs, patience=patience, seed=seed, loss=loss, focal_gamma=focal_gamma, sample_weight=sample_weight, rows=rows)
    T = len(trials)
    stopping, active = [_EarlyStopping(plan.patience) for _ in range(T)], np.ones(T, bool)
    be = _SweepBackend(getattr(ctx_or_runner, "ctx", ctx_or_runner), X, Y, X_val, Y_val, plan, trials)
    try:
        for epoch in range(plan.epochs):
            if not active.any():
                break
            running = np.flatnonzero(active)
            losses = be.epoch(_epoch_rows(plan.seed, epoch, plan.m, plan.rows), active)
            for t in running:
                stopping[t].add_epoch(losses[:, t])
            if not plan.has_val:
                continue
            vals = be.val_loss(active)
            improved = np.zeros(T, bool)
            for t in running:   # a stopped trial goes inactive
                improved[t], stop = stopping[t].update(epoch, float(vals[t]))
                active[t] = not stop
            if improved.any():
                be.snapshot(improved)
        heads = []
        for t in range(T):
            history = stopping[t].finish()
            W, b = be.get(t, snapshot=history["best_epoch"] is not None)
            heads.append(ProbeHead(W, b, activation, list(class_names or []), history))
    finally:
        be.close()
    return SweepResult(heads, trials, _best_trial(heads))


def fit_probe_sweep_reference(X, Y, X_val=None, Y_val=None, trials=(), *, activation="sigmoid", epochs=50, batch_size=32, patience=10, seed=42,
                              dtype=np.float64, class_names=None, loss="auto", focal_gamma=2.0, sample_weight=None, rows=None) -> SweepResult:
    """The specification of ``fit_probe_sweep``: ``fit_probe_reference`` once per trial."""
    trials = _check_trials(trials)
    heads = [fit_probe_reference(X, Y, X_val, Y_val, activation=activation, epochs=epochs, batch_size=batch_size, patience=patience, seed=seed, dtype=dtype,
                                 class_names=class_names, loss=loss, focal_gamma=focal_gamma, sample_weight=sample_weight, rows=rows, **t.fit_kwargs())
             for t in trials]
    return SweepResult(heads, trials, _best_trial(heads))


# -- the fit on augmented inputs ------------------------------------------------------------------------------------------------------
def _check_augmented_args(augment, activation, input_shape, n_elems):
    """The refusals of the augmented fit that need no model: raised before anything is loaded or uploaded."""
    from birdnet_stm32.training.augment import ProbeAugmentation

    if not isinstance(augment, ProbeAugmentation):
        raise ValueError("augment must be a ProbeAugmentation")
    if not augment.active:
        raise ValueError("the augmentation is off (no mixup, no SpecAugment): call fit_probe on the embeddings instead")
    if augment.mixup and activation == "softmax":
        raise ValueError("mixup takes the union of its sources' labels, which is no distribution: use activation='sigmoid' "
                         "(the reference switches to sigmoid whenever mixup is on)")
    F, W = (int(v) for v in input_shape)
    if F < 1 or W < 1 or (n_elems is not None and F * W != int(n_elems)):
        raise ValueError(f"input_shape {F} x {W} does not match rows of {n_elems} elements")
    return F, W


class _Shape:
    def __init__(self, *shape):
        self.shape = shape


def augmented_embeddings(runner, inputs, plan, out=None, slice_buf=None):
    """Embeddings ``[plan.rows, D]`` (CUDA float32) of the plan's augmented rows: in slices of ``runner.max_batch``, ``bn_augment_inputs``
    into one slice buffer and the backbone over it.  ``inputs``: the resident un-augmented model inputs ``[n, F * W]``."""
    import ctypes

    import torch

    from birdnet_stm32 import _hip
    from birdnet_stm32.training.augment import check_plan

    n, E = int(inputs.shape[0]), int(inputs.shape[1])
    if not (inputs.is_cuda and inputs.dtype == torch.float32 and inputs.is_contiguous() and E == int(plan.F) * int(plan.W)):
        raise ValueError(f"inputs must be a contiguous float32 CUDA tensor [n, {int(plan.F) * int(plan.W)}]")
    check_plan(plan, n)
    m, mb = plan.rows, int(runner.max_batch)
    dev = inputs.device
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_nsrc, d_src, d_gain, d_f, d_t = (up(a) for a in (plan.nsrc, plan.src, plan.gain, plan.fmask, plan.tmask))
    nf, nt = (0 if t is None else int(t.shape[1]) for t in (plan.fmask, plan.tmask))
    D = int(runner.embedding_info()["dim"])
    if out is None:
        out = torch.empty((m, D), dtype=torch.float32, device=dev)
    if slice_buf is None:
        slice_buf = torch.empty((min(mb, max(m, 1)), E), dtype=torch.float32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for b0 in range(0, m, mb):
            nb = min(mb, m - b0)
            _hip.check(runner.ctx.lib.bn_augment_inputs(runner.ctx.handle, inputs.data_ptr(), n, int(plan.F), int(plan.W), d_nsrc[b0:].data_ptr(),
                                                        d_src[b0:].data_ptr(), d_gain[b0:].data_ptr(), ptr(d_f), nf, ptr(d_t), nt, nb,
                                                        slice_buf.data_ptr(), stream))
            runner.predict_device(slice_buf[:nb], return_embeddings=True, emb_out=out[b0 : b0 + nb])
        torch.cuda.current_stream(dev).synchronize()   # (the tables are freed on return)
    return out


class _AugmentedDeviceBackend(_DeviceBackend):
    """The device fit over rows that change per epoch: ``epoch`` first builds that epoch's ``X`` / ``Y`` in place, then runs the plain epoch."""

    def __init__(self, runner, inputs, Y, X_val, Y_val, plan, augment, F, W_in):
        import time

        import torch

        self.runner, self.inputs, self.aug, self.F, self.W_in, self.time = runner, inputs, augment, F, W_in, time
        self.Y_host = np.ascontiguousarray(Y, np.float32)
        super().__init__(runner.ctx, torch.zeros((plan.n, plan.D), dtype=torch.float32, device=inputs.device), self.Y_host, X_val, Y_val, plan)
        self.slice_buf = torch.empty((min(int(runner.max_batch), plan.n), int(inputs.shape[1])), dtype=torch.float32, device=inputs.device)
        self.epochs_done, self.augment_seconds = 0, []

    def epoch(self, perm):
        from birdnet_stm32.training.augment import augment_plan, mixed_targets

        t0 = self.time.perf_counter()
        plan = augment_plan(self.n, self.F, self.W_in, self.aug, self.plan.seed, self.epochs_done)
        augmented_embeddings(self.runner, self.inputs, plan, out=self.X, slice_buf=self.slice_buf)
        self.Y.copy_(self.torch.from_numpy(mixed_targets(self.Y_host, plan)))
        self.torch.cuda.current_stream(self.dev).synchronize()
        self.augment_seconds.append(self.time.perf_counter() - t0)
        self.epochs_done += 1
        return super().epoch(perm)


def fit_probe_augmented(runner, inputs, Y, X_val=None, Y_val=None, *, augment, input_shape, activation="sigmoid", epochs=50, batch_size=32,
                        learning_rate=1e-3, optimizer="adam", weight_decay=0.0, clipnorm=1.0, dropout=0.5, patience=10, seed=42,
                        class_names=None, loss="auto", focal_gamma=2.0, sample_weight=None, rows=None, hidden_units=0) -> ProbeHead:
    """``fit_probe`` on fresh embeddings per epoch (reference: training/linear_probe.py:112-125, whose training loader masks and mixes).

    ``inputs [N, F * W]``: the un-augmented model inputs of the training rows (``HipRunner.model_inputs_device``; a CUDA tensor stays
    where it is, a numpy array is uploaded once), ``input_shape = (F, W)`` (the raw frontend: ``(1, T)``).  Epoch ``e`` builds
    ``training.augment.augment_plan(N, F, W, augment, seed, e)``, augments on the device (``bn_augment_inputs``), embeds the rows again with
    the frozen backbone and runs the plain epoch (same permutation, same dropout draws) on them with ``mixed_targets``.  ``X_val`` are
    embeddings of un-augmented validation rows, computed once by the caller.  ``history["augment_seconds"]`` holds the per-epoch time of
    plan + augmentation + backbone.  The same inputs and seed give the same bits on every run.

    ``loss`` / ``focal_gamma`` / ``sample_weight`` / ``rows``: as ``fit_probe``.  The plan of an epoch is drawn per row of ``inputs``, not
    per entry of ``rows``: every row is augmented and embedded once per epoch, and the copies of a row that ``rows`` repeats share that
    epoch's augmentation (their dropout masks still differ).  A mixed row's weight is its own: ``sample_weight[i]`` of the row it is
    built on, whatever rows were mixed into it."""
    import torch

    refuse_hidden("fit_probe_augmented", hidden_units)
    F, W_in = _check_augmented_args(augment, activation, input_shape, inputs.shape[1] if len(inputs.shape) == 2 else None)
    if not hasattr(runner, "predict_device"):
        raise ValueError("fit_probe_augmented needs the model's runner: the backbone runs every epoch")
    if len(inputs.shape) != 2:
        raise ValueError(f"inputs must be [N, F * W], got {tuple(inputs.shape)}")
    plan = _plan_fit(_Shape(int(inputs.shape[0]), int(runner.embedding_info()["dim"])), Y, X_val, device=True, activation=activation, optimizer=optimizer,
                     batch_size=batch_size, dropout=dropout, epochs=epochs, learning_rate=learning_rate, weight_decay=weight_decay, clipnorm=clipnorm,
                     patience=patience, seed=seed, loss=loss, focal_gamma=focal_gamma, sample_weight=sample_weight, rows=rows)
    if int(inputs.shape[1]) != int(runner.input_elems):
        raise ValueError(f"inputs have {int(inputs.shape[1])} elements per row, the model takes {runner.input_elems}")
    if isinstance(inputs, np.ndarray):
        inputs = torch.from_numpy(np.ascontiguousarray(inputs, np.float32)).to(runner.device)
    if isinstance(Y, torch.Tensor):
        Y = Y.cpu().numpy()
    be = _AugmentedDeviceBackend(runner, inputs.contiguous(), Y, X_val, Y_val, plan, augment, F, W_in)
    head = _device_fit(be, plan, class_names)
    head.history["augment_seconds"] = list(be.augment_seconds)
    return head


class _AugmentedNumpyBackend(_NumpyBackend):
    def __init__(self, embed, inputs, Y, X_val, Y_val, plan, dtype, augment, F, W_in):
        self.embed, self.inputs, self.Y_host, self.aug, self.F, self.W_in, self.epochs_done = embed, inputs, Y, augment, F, W_in, 0
        super().__init__(None, None, X_val, Y_val, plan, dtype)

    def epoch(self, perm):
        from birdnet_stm32.training.augment import augment_plan, augment_reference, mixed_targets

        plan = augment_plan(self.inputs.shape[0], self.F, self.W_in, self.aug, self.plan.seed, self.epochs_done)
        self.X = np.asarray(self.embed(augment_reference(self.inputs, plan))).astype(self.dt)
        self.Y = mixed_targets(self.Y_host, plan).astype(self.dt)
        self.epochs_done += 1
        return super().epoch(perm)


def fit_probe_augmented_reference(embed, inputs, Y, X_val=None, Y_val=None, *, augment, input_shape, activation="sigmoid", epochs=50, batch_size=32,
                                  learning_rate=1e-3, optimizer="adam", weight_decay=0.0, clipnorm=1.0, dropout=0.5, patience=10, seed=42,
                                  dtype=np.float64, class_names=None, loss="auto", focal_gamma=2.0, sample_weight=None, rows=None) -> ProbeHead:
    """The procedure of ``fit_probe_augmented`` in numpy over a caller-supplied ``embed(inputs [N, F * W] float32) -> X [N, D]``."""
    inputs, Y = np.ascontiguousarray(inputs, np.float32), np.asarray(Y)
    F, W_in = _check_augmented_args(augment, activation, input_shape, inputs.shape[1] if inputs.ndim == 2 else None)
    D = int(np.asarray(embed(inputs[:1])).shape[1])
    plan = _plan_fit(_Shape(inputs.shape[0], D), Y, X_val, device=False, activation=activation, optimizer=optimizer, batch_size=batch_size, dropout=dropout,
                     epochs=epochs, learning_rate=learning_rate, weight_decay=weight_decay, clipnorm=clipnorm, patience=patience, seed=seed, loss=loss,
                     focal_gamma=focal_gamma, sample_weight=sample_weight, rows=rows)
    return _reference_fit(_AugmentedNumpyBackend(embed, inputs, Y, X_val, Y_val, plan, dtype, augment, F, W_in), plan, class_names)


# -- from class folders to a head on disk ---------------------------------------------------------------------------------------------
def split_train_val(paths: list, val_split: float) -> tuple[list, list]:
    """The first ``1 - val_split`` of the (already shuffled) list trains, the rest validates (reference: linear_probe.py, cli/train.py)."""
    k = int(len(paths) * (1 - float(val_split)))
    return list(paths[:k]), list(paths[k:])


def targets_from_paths(paths: list, classes: list, file_index: np.ndarray, activation: str = "sigmoid") -> tuple[np.ndarray, np.ndarray]:
    """One-hot targets ``[rows, len(classes)]`` of embedding rows from the parent folder of each row's file, and the mask of rows to
    keep: files of folders that are not classes (the noise-like ones) give all-zero rows under sigmoid and are dropped under softmax."""
    col = {c: i for i, c in enumerate(classes)}
    label = np.array([col.get(os.path.basename(os.path.dirname(p)), -1) for p in paths], np.int64)
    row_label = label[np.asarray(file_index, np.int64)] if len(paths) else np.zeros(0, np.int64)
    Y = np.zeros((row_label.shape[0], len(classes)), np.float32)
    known = row_label >= 0
    Y[np.flatnonzero(known), row_label[known]] = 1.0
    keep = known if activation == "softmax" else np.ones_like(known)
    return Y, keep


def probe_output_paths(output: str) -> dict:
    stem = output[:-4] if output.endswith(".npz") else output
    return {"head": stem + ".npz", "labels": stem + "_labels.txt", "config": stem + "_model_config.json", "history": stem + "_history.csv",
            "tune": stem + "_tune.json", "tflite": stem + ".tflite", "export": stem + "_export.json"}


def write_history_csv(path: str, history: dict) -> None:
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["epoch", "loss", "val_loss"])
        val = history.get("val_loss") or []
        for i, loss in enumerate(history.get("loss", [])):
            w.writerow([i + 1, f"{loss:.8g}", f"{val[i]:.8g}" if i < len(val) else ""])


def _join_embeddings(a, b):
    """Two ``FileEmbeddings`` (per chunk) as one over ``a.paths + b.paths``."""
    from dataclasses import replace

    return replace(a, embeddings=np.concatenate([a.embeddings, b.embeddings]), file_index=np.concatenate([a.file_index, b.file_index + len(a.paths)]),
                   start_s=np.concatenate([a.start_s, b.start_s]), paths=list(a.paths) + list(b.paths),
                   chunks_per_file=np.concatenate([a.chunks_per_file, b.chunks_per_file]), skipped=list(a.skipped) + list(b.skipped),
                   candidate_rows=a.candidate_rows + b.candidate_rows)


def augmentation_from_args(args):
    """The ``ProbeAugmentation`` the ``--mixup_*`` / ``--spec_augment`` / ``--*_mask_max`` flags of ``probe`` ask for, ``None`` when both are
    off or absent (older namespaces); bad values and mixup with softmax are refused here, before anything is loaded."""
    from birdnet_stm32.training.augment import ProbeAugmentation

    aug = ProbeAugmentation(mixup_alpha=float(getattr(args, "mixup_alpha", 0.2)), mixup_probability=float(getattr(args, "mixup_probability", 0.0) or 0.0),
                            spec_augment=bool(getattr(args, "spec_augment", False)), freq_mask_max=int(getattr(args, "freq_mask_max", 8)),
                            time_mask_max=int(getattr(args, "time_mask_max", 25)))
    if not aug.active:
        return None
    _check_augmented_args(aug, getattr(args, "activation", "sigmoid"), (1, 1), None)
    return aug


def imbalance_from_args(args) -> dict:
    """``--loss`` / ``--focal_gamma`` / ``--class_weights`` / ``--upsample_ratio`` of ``probe`` as a dict (absent in older namespaces: all
    off); bad values and focal with softmax are refused here, before anything is loaded."""
    loss, gamma = _check_loss(getattr(args, "loss", "auto"), getattr(args, "focal_gamma", 2.0), getattr(args, "activation", "sigmoid"))
    class_weights = getattr(args, "class_weights", "none")
    if class_weights not in ("none", "balanced"):
        raise ValueError(f"--class_weights must be none or balanced, not {class_weights!r}")
    ratio = float(getattr(args, "upsample_ratio", 0.0) or 0.0)
    if not 0.0 <= ratio <= 1.0:   # (NaN fails too)
        raise ValueError(f"--upsample_ratio must be 0 (off) or in (0, 1], got {ratio}")
    return {"loss": loss, "focal_gamma": gamma, "class_weights": class_weights, "upsample_ratio": ratio}


def hidden_from_args(args) -> int:
    """``--hidden_units`` of ``probe`` (absent in older namespaces: 0, no hidden layer); refused, before anything is loaded, with what is
    not built for such a head: ``--tune``, ``--export_tflite`` / ``--qat_epochs``, ``--mixup_probability`` / ``--spec_augment``."""
    H = check_hidden_units(getattr(args, "hidden_units", 0) or 0, device=True)
    if H == 0:
        return 0
    for flag, on in (("--tune", getattr(args, "tune", False)), ("--export_tflite", getattr(args, "export_tflite", False)),
                     ("--qat_epochs", int(getattr(args, "qat_epochs", 0) or 0) > 0),
                     ("--mixup_probability", float(getattr(args, "mixup_probability", 0.0) or 0.0) > 0), ("--spec_augment", getattr(args, "spec_augment", False))):
        if on:
            raise ValueError(f"--hidden_units does not combine with {flag}: that path is not built for a head with a hidden layer")
    return H


def upsample_multiplicity(train_paths: list, classes: list, ratio: float) -> tuple[np.ndarray, list]:
    """How often each file of ``train_paths`` trains per epoch under ``--upsample_ratio`` (int64 ``[len(train_paths)]``), and the
    upsampled list of class files the counts come from.  Only the files whose folder is a class go through
    ``data.dataset.upsample_minority_classes`` (which, like the reference's, drops the others); the files of noise folders keep
    multiplicity 1.  ``train_paths`` must hold every file once."""
    from collections import Counter

    from birdnet_stm32.data.dataset import upsample_minority_classes

    known = set(classes)
    upsampled = upsample_minority_classes([p for p in train_paths if os.path.basename(os.path.dirname(p)) in known], classes, ratio)
    count = Counter(upsampled)
    return np.array([count.get(p, 1) for p in train_paths], np.int64), upsampled


def check_export_args(args) -> bool:
    """``--export_tflite`` of ``probe`` (absent in older namespaces: off): refused unless ``--model_path`` is an INT8 ``.tflite`` — the head
    must be trained on the embeddings the board computes — by its suffix and by the graph itself (an int8 pooled tensor in front of a
    classifier), before any audio file is read."""
    if not getattr(args, "export_tflite", False):
        return False
    if not str(args.model_path).lower().endswith(".tflite"):
        raise ValueError(f"--export_tflite needs --model_path to be an INT8 .tflite, not {args.model_path}: the exported head must be trained on the "
                         "embeddings the board computes, and heads on float backbones are not exported")
    if os.path.isfile(args.model_path):   # (a missing file is reported as such by the command); a float .tflite, or one without a classifier behind pooling
        from birdnet_stm32.conversion.head_export import int8_embedding_of
        from birdnet_stm32.models._tflite_reader import load_tflite

        try:
            int8_embedding_of(load_tflite(args.model_path))
        except ValueError as exc:
            raise ValueError(f"--export_tflite: {args.model_path}: {exc}") from None
    cos = float(getattr(args, "min_cosine_sim", 0.95))
    if not 0.0 <= cos <= 1.0:   # (NaN fails too)
        raise ValueError(f"--min_cosine_sim must be in [0, 1] (0 disables the check), got {cos}")
    return True


def check_qat_args(args) -> int:
    """``--qat_epochs`` / ``--qat_learning_rate`` of ``probe`` (absent in older namespaces: off): the epochs of the quantisation-aware
    fine-tune in front of the export, 0 when off; refused without ``--export_tflite`` and with bad values, before anything is loaded."""
    epochs = int(getattr(args, "qat_epochs", 0) or 0)
    if epochs < 0:
        raise ValueError(f"--qat_epochs must be >= 0 (0 = off), got {epochs}")
    if epochs == 0:
        return 0
    if not getattr(args, "export_tflite", False):
        raise ValueError("--qat_epochs needs --export_tflite: the fine-tune prepares the head for the INT8 export and is of no use without it")
    lr = float(getattr(args, "qat_learning_rate", 1e-4))
    if not (math.isfinite(lr) and lr > 0):
        raise ValueError(f"--qat_learning_rate must be finite and > 0, got {lr}")
    return epochs


def qat_for_export(head, runner, X, Y, train_rows, val_rows, report_rows, per_tensor: bool, epochs: int, fit_kw: dict, loss_kw: dict):
    """``probe --export_tflite --qat_epochs``: fine-tune ``head`` against the export's own quantisation (``training.probe_qat.fit_probe_qat``
    on the rows ``train_rows`` of ``X`` / ``Y``, validated on ``val_rows``), quantise the float head and the fine-tuned one with the float
    head's logit range over all of ``X``, and keep the one whose INT8 scores (``QuantizedHead.predict``) have the lower loss over
    ``report_rows``.  Returns ``(the kept head, logit_range, the "qat" object of <output>_export.json)``."""
    import torch

    from birdnet_stm32.conversion.head_export import float_logit_range, quantize_head
    from birdnet_stm32.conversion.validate import cosine_similarity
    from birdnet_stm32.training.probe_qat import fit_probe_qat, qat_logit_codes

    info = runner.embedding_info()
    if info["dtype"] != "int8":
        raise ValueError("--export_tflite needs an INT8 model: this one's embeddings are float32")
    rows = embedding_bytes_device(X, info["scale"], info["zero_point"], runner.device)
    lo, hi = float_logit_range(head, rows, info["scale"], info["zero_point"])
    tuned = fit_probe_qat(runner, X[train_rows], Y[train_rows], X[val_rows] if val_rows.any() else None, Y[val_rows] if val_rows.any() else None,
                          head=head, logit_range=(lo, hi), per_tensor=per_tensor, epochs=epochs, **fit_kw)
    rep_rows = rows[torch.from_numpy(np.flatnonzero(report_rows)).to(rows.device)].contiguous()
    X_rep, Y_rep = np.ascontiguousarray(X[report_rows]), Y[report_rows]
    side = {}
    for name, h in (("float", head), ("qat", tuned)):
        with quantize_head(h, info["scale"], info["zero_point"], lo, hi, per_tensor) as qh:
            P_q, logit = qh.predict_device(rep_rows, runner.ctx, return_logit_bytes=True)
        P_q, P_f = P_q.cpu().numpy(), h.predict(X_rep, runner.ctx)
        side[name] = {"loss_int8": float(probe_loss(P_q, Y_rep, h.activation, **loss_kw)), "loss_float": float(probe_loss(P_f, Y_rep, h.activation, **loss_kw)),
                      "cosine_mean": float(np.mean([cosine_similarity(u, v) for u, v in zip(P_f.astype(np.float64), P_q.astype(np.float64))]))}
        h.close()
        side[name + "_logit"] = logit.cpu().numpy()
    codes = qat_logit_codes(runner.ctx, tuned, X_rep, (lo, hi), per_tensor)
    kept = "qat" if side["qat"]["loss_int8"] < side["float"]["loss_int8"] else "float"
    report = {"epochs": tuned.history["qat"]["epochs"], "learning_rate": float(fit_kw["learning_rate"]), "logit_range": [lo, hi],
              "logit_scale": tuned.history["qat"]["logit_scale"], "logit_zero_point": tuned.history["qat"]["logit_zero_point"],
              "float": side["float"], "qat": side["qat"], "kept": kept, "code_agreement": float(np.mean(codes == side["qat_logit"]))}
    print(f"[probe] QAT fine-tune, {report['epochs']} epochs at lr {report['learning_rate']:g}: INT8 loss {side['float']['loss_int8']:.4f} (float head) vs "
          f"{side['qat']['loss_int8']:.4f} (fine-tuned), cosine {side['float']['cosine_mean']:.6f} vs {side['qat']['cosine_mean']:.6f}; the {kept} head is "
          f"written; {100 * report['code_agreement']:.2f} % of the fine-tune's logit codes are the INT8 head's bytes")
    return (tuned if kept == "qat" else head), (lo, hi), report


def embedding_bytes_device(X, scale: float, zero_point: int, device):
    """The int8 bytes behind float32 embeddings ``X [n, D]`` of an INT8 runner, ``round(x / scale) + zero_point``, as a CUDA int8 tensor; the
    round trip ``(q - zero_point) * scale == x`` is asserted on the device for every element."""
    import torch

    x = torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(device)
    s = torch.tensor(np.float32(scale), dtype=torch.float32, device=x.device)
    q = torch.round(x / s) + float(zero_point)
    if not bool(((q >= -128) & (q <= 127) & ((q - float(zero_point)) * s == x)).all()):
        raise RuntimeError("the embeddings are not the dequantised bytes of this model: (q - zero_point) * scale does not give them back")
    return q.to(torch.int8)


def export_probe_tflite(head, runner, model_path: str, X, Y, report_rows, out: dict, activation: str, per_tensor: bool, min_cosine_sim: float,
                        loss_kw: dict, logit_range=None, qat: dict | None = None) -> dict:
    """``probe --export_tflite``: ``head`` into ``out["tflite"]`` (``conversion.head_export.export_head_tflite``, calibrated on all rows
    ``X``), the report of float head against INT8 head (``bn_head_i8_forward``) over ``report_rows`` into ``out["export"]``; raises below
    ``min_cosine_sim`` as ``convert`` does.  ``logit_range`` / ``qat``: what ``qat_for_export`` returned for ``head``; the range then replaces
    the observed one and the report gains the ``"qat"`` object."""
    from birdnet_stm32.conversion.head_export import export_head_tflite
    from birdnet_stm32.conversion.validate import cosine_similarity, pearson_correlation

    info = runner.embedding_info()
    if info["dtype"] != "int8":
        raise ValueError("--export_tflite needs an INT8 model: this one's embeddings are float32")
    rows = embedding_bytes_device(X, info["scale"], info["zero_point"], runner.device)
    rep = export_head_tflite(head, model_path, rows, out["tflite"], per_tensor=per_tensor, ctx=runner.ctx, logit_range=logit_range)
    qhead = rep.pop("qhead")
    import torch

    sel = torch.from_numpy(np.flatnonzero(report_rows)).to(rows.device)
    P_q, logit = qhead.predict_device(rows[sel].contiguous(), runner.ctx, return_logit_bytes=True)
    P_q, logit = P_q.cpu().numpy(), logit.cpu().numpy()
    qhead.close()
    P_f = head.predict(X[report_rows], runner.ctx)
    a, b = P_f.astype(np.float64), P_q.astype(np.float64)
    rep.update({"model_path": model_path, "activation": activation, "classes": int(head.num_classes), "report_rows": int(report_rows.sum()),
                "cosine_mean": float(np.mean([cosine_similarity(u, v) for u, v in zip(a, b)])),
                "mse_mean": float(np.mean((a - b) ** 2)), "mae_mean": float(np.mean(np.abs(a - b))),
                "pearson_mean": float(np.mean([pearson_correlation(u, v) for u, v in zip(a, b)])),
                "loss_float": float(probe_loss(P_f, Y[report_rows], activation, **loss_kw)),
                "loss_int8": float(probe_loss(P_q, Y[report_rows], activation, **loss_kw)),
                "report_clipped_share": float(np.mean((logit == -128) | (logit == 127))), "min_cosine_sim": float(min_cosine_sim)})
    if qat is not None:
        rep["qat"] = qat
    with open(out["export"], "w") as fh:
        json.dump(rep, fh, indent=1)
    print(f"[probe] exported {out['tflite']} ({rep['bytes']} bytes, {rep['classes']} classes, {'per-tensor' if per_tensor else 'per-channel'} weights): logits "
          f"[{rep['logit_range'][0]:.3f}, {rep['logit_range'][1]:.3f}] at scale {rep['logit_scale']:.5f}, {100 * rep['clipped_share']:.2f} % of the logit bytes at "
          f"a clamp; float vs INT8 head over {rep['report_rows']} rows: cosine {rep['cosine_mean']:.6f}, MSE {rep['mse_mean']:.3e}, Pearson "
          f"{rep['pearson_mean']:.6f}, loss {rep['loss_float']:.4f} -> {rep['loss_int8']:.4f}")
    if min_cosine_sim > 0 and rep["cosine_mean"] < min_cosine_sim:
        raise RuntimeError(f"Quantization quality check failed: mean cosine similarity {rep['cosine_mean']:.6f} < threshold {min_cosine_sim:.4f}.")
    return rep


def run_linear_probe(args, runner=None) -> ProbeHead:
    """The ``probe`` command: ``args.data_path_train/<class>/*`` -> embeddings (the backbone runs once) -> ``fit_probe`` ->
    ``<output>.npz``, ``<output>_labels.txt``, ``<output>_model_config.json`` and ``<output>_history.csv``.  With ``args.hidden_units = H > 0``
    the head has one ReLU layer of ``H`` units (``hidden_from_args``: on its own only).  With ``args.tune``:
    ``training.tune.sample_trials`` -> ``fit_probe_sweep``; the files are the winning trial's, ``<output>_tune.json`` lists all trials.
    With ``args.export_tflite`` (INT8 ``.tflite`` backbones): the written head also goes into ``<output>.tflite``, an ordinary model next
    to the labels and config written here, with ``<output>_export.json`` (``export_probe_tflite``); with ``args.qat_epochs`` the head is
    first fine-tuned against the export's quantisation and the better of the two heads as INT8 is the one written (``qat_for_export``).

    For long-tailed folders (``imbalance_from_args``), in the reference's order: ``--upsample_ratio`` first repeats training files of the
    small classes (``upsample_multiplicity``; the validation split is never upsampled, and every distinct file is embedded once: the
    repeats are row numbers, ``upsample_rows``), then ``--class_weights balanced`` counts the upsampled list (``balanced_class_weights``,
    ``row_weights``), and ``--loss focal`` picks the element loss.  All three go to the plain fit, the sweep of ``--tune`` (shared by
    every trial) and the augmented fit alike."""
    import time
    from dataclasses import replace

    from birdnet_stm32.cli.evaluate import resolve_config_path
    from birdnet_stm32.data.dataset import load_file_paths_from_directory
    from birdnet_stm32.evaluation.embeddings import embed_files
    from birdnet_stm32.training.config import ModelConfig

    from birdnet_stm32.training.tune import check_tune_args

    hidden = hidden_from_args(args)
    augment = augmentation_from_args(args)
    imb = imbalance_from_args(args)
    check_tune_args(args)
    export = check_export_args(args)
    qat_epochs = check_qat_args(args)
    label_smoothing = _check_label_smoothing(getattr(args, "label_smoothing", 0.0))
    if augment is not None and label_smoothing > 0:
        raise ValueError("--label_smoothing does not combine with --mixup_probability or --spec_augment")
    if not os.path.isfile(args.model_path):
        raise FileNotFoundError(f"Pretrained model not found: {args.model_path}")
    cfg = ModelConfig.load(resolve_config_path(args.model_path, getattr(args, "model_config", "")))
    np.random.seed(int(args.seed))   # load_file_paths_from_directory shuffles with numpy.random
    paths, classes = load_file_paths_from_directory(args.data_path_train)
    if not classes:
        raise ValueError("No classes found in the training data.")
    if not 1 <= len(classes) <= 4096:
        raise ValueError(f"{len(classes)} classes: the device path takes at most 4096")
    train_paths, val_paths = split_train_val(paths, args.val_split)
    print(f"[probe] {len(classes)} target classes, {len(train_paths)} training and {len(val_paths)} validation files")
    multiplicity, counted = None, train_paths
    if imb["upsample_ratio"] > 0:   # (before the model is loaded: the draws follow the shuffle's on numpy's global generator)
        multiplicity, counted = upsample_multiplicity(train_paths, classes, imb["upsample_ratio"])
    class_weights = None
    if imb["class_weights"] == "balanced":
        class_weights = balanced_class_weights(counted, classes)
        print(f"Balanced class weights: min={class_weights.min():.2f}, max={class_weights.max():.2f}")
    if runner is None:
        from birdnet_stm32.models.runners import load_model_runner

        runner = load_model_runner(args.model_path, device=getattr(args, "device", 0), max_batch=getattr(args, "max_batch", 4096), prepare_pipeline=True)
    overlap = max(0.0, min(float(cfg.chunk_duration) - 0.1, float(args.overlap)))
    t0 = time.perf_counter()
    from birdnet_stm32.audio.pipeline import selection_from_args

    kw = dict(chunk_overlap=overlap, max_duration=args.max_duration, pooling="none", dtype="float32", sample_rate=int(cfg.sample_rate),
              chunk_duration=float(cfg.chunk_duration))
    select = selection_from_args(args)
    train_inputs = None
    if augment is not None:
        # training files keep their model inputs on the device; validation files take the plain path (with a selection at 0.5, as below)
        emb = embed_files(runner, train_paths, select=select, keep_inputs=True, **kw)
        train_inputs = emb.inputs
        if val_paths:
            emb = _join_embeddings(emb, embed_files(runner, val_paths, select=selection_from_args(args, 0.5), **kw))
    elif select is None:
        emb = embed_files(runner, train_paths + val_paths, **kw)
    else:
        # the reference's loader (data/generator.py:87-157): training files at --activity_threshold, validation files at 0.5 (its linear probe's
        # validation generator, training/linear_probe.py), hence one pass per split
        emb = embed_files(runner, train_paths, select=select, **kw)
        if val_paths:
            emb = _join_embeddings(emb, embed_files(runner, val_paths, select=selection_from_args(args, 0.5), **kw))
    if select is not None:
        print(f"[probe] selection: {emb.candidate_rows} candidate rows -> {emb.embeddings.shape[0]} rows (at most {select.max_chunks_per_file} per file, "
              f"{select.candidate_chunks} candidates)")
    t_embed = time.perf_counter() - t0
    Y, keep = targets_from_paths(emb.paths, classes, emb.file_index, args.activation)
    is_train = np.asarray(emb.file_index) < len(train_paths)
    tr, va = keep & is_train, keep & ~is_train
    if not tr.any():
        raise ValueError("no training rows: every training file was unreadable, empty or of a noise folder")
    n_fit = int(tr.sum())
    # the fits see the training rows X[tr] / Y[tr]: weights per such row, and the upsampled epoch as row numbers into them
    imb_kw = dict(loss=imb["loss"], focal_gamma=imb["focal_gamma"],
                  sample_weight=None if class_weights is None else row_weights(Y[tr], class_weights),
                  rows=None if multiplicity is None else upsample_rows(np.asarray(emb.file_index)[tr], multiplicity))
    if multiplicity is not None:
        print(f"[probe] upsampling at ratio {imb['upsample_ratio']:g}: {n_fit} training rows -> {len(imb_kw['rows'])} rows per epoch")
    t0 = time.perf_counter()
    fit_kw = dict(activation=args.activation, epochs=args.epochs, batch_size=args.batch_size, learning_rate=args.learning_rate,
                  optimizer=args.optimizer, weight_decay=args.weight_decay, clipnorm=args.grad_clip, dropout=args.dropout,
                  patience=getattr(args, "patience", 10), seed=args.seed, class_names=classes)
    tuned = None
    if getattr(args, "tune", False):
        from birdnet_stm32.training.tune import macro_roc_auc, sample_trials, tune_report

        if not va.any():
            raise ValueError("--tune needs validation rows: the validation split came out empty")
        base = ProbeTrial(learning_rate=args.learning_rate, optimizer=args.optimizer, weight_decay=args.weight_decay, clipnorm=args.grad_clip,
                          dropout=args.dropout, label_smoothing=label_smoothing)
        tune_seed = args.seed if getattr(args, "tune_seed", None) is None else args.tune_seed
        tuned = fit_probe_sweep(runner, emb.embeddings[tr], Y[tr], emb.embeddings[va], Y[va], sample_trials(args.n_trials, tune_seed, base),
                                activation=args.activation, epochs=args.epochs, batch_size=args.batch_size, patience=getattr(args, "patience", 10),
                                seed=args.seed, class_names=classes, **imb_kw)
        head = tuned.best_head
        auc = macro_roc_auc(Y[va], head.predict(emb.embeddings[va], runner.ctx))
        tuned = {**tune_report(tuned, auc), **imb}   # shared by every trial, no part of the search space
    elif augment is None:
        head = fit_probe(runner, emb.embeddings[tr], Y[tr], emb.embeddings[va] if va.any() else None, Y[va] if va.any() else None,
                         label_smoothing=label_smoothing, **fit_kw, **imb_kw, **({"hidden_units": hidden} if hidden else {}))
    else:
        import torch

        n_train = int(is_train.sum())   # the kept inputs are the training rows, in row order
        if train_inputs.shape[0] != n_train:
            raise RuntimeError("the kept model inputs do not match the training rows")
        rows = tr[:n_train]
        inputs = train_inputs if rows.all() else train_inputs[torch.from_numpy(np.flatnonzero(rows)).to(train_inputs.device)]
        head = fit_probe_augmented(runner, inputs, Y[tr], emb.embeddings[va] if va.any() else None, Y[va] if va.any() else None, augment=augment,
                                   input_shape=runner.input_shape(), **fit_kw, **imb_kw)
        del train_inputs, inputs
    qat_range = qat_report = None
    if export and qat_epochs:   # after whichever fit was asked for; the head with the lower INT8 loss is the one written below
        kept = tr | va
        qat_kw = {**{k: fit_kw[k] for k in ("batch_size", "optimizer", "weight_decay", "clipnorm", "dropout", "patience", "seed")},
                  "learning_rate": float(getattr(args, "qat_learning_rate", 1e-4)), **imb_kw}
        if tuned is not None:   # the winner's own settings, where the search covers them
            qat_kw.update({k: tuned["trials"][tuned["best_trial"]]["params"][k] for k in ("optimizer", "weight_decay", "clipnorm", "dropout")})
        head, qat_range, qat_report = qat_for_export(head, runner, emb.embeddings[kept], Y[kept], tr[kept], va[kept], (va if va.any() else tr)[kept],
                                                     bool(getattr(args, "per_tensor", False)), qat_epochs, qat_kw,
                                                     dict(loss=imb["loss"], focal_gamma=imb["focal_gamma"]))
    t_fit = time.perf_counter() - t0
    out = probe_output_paths(args.output)
    os.makedirs(os.path.dirname(os.path.abspath(out["head"])), exist_ok=True)
    head.save(out["head"])
    with open(out["labels"], "w") as fh:
        fh.write("\n".join(classes) + "\n")
    dropout_used = tuned["trials"][tuned["best_trial"]]["params"]["dropout"] if tuned else args.dropout   # the written head's own
    replace(cfg, num_classes=len(classes), class_names=list(classes), dropout_rate=float(dropout_used)).save(out["config"])
    write_history_csv(out["history"], head.history)
    if tuned is not None:
        with open(out["tune"], "w") as fh:
            json.dump(tuned, fh, indent=1)
        win = tuned["trials"][tuned["best_trial"]]
        print(f"[probe] tuned over {tuned['n_trials']} trials: trial {tuned['best_trial']} wins with val_loss {win['best_val_loss']:.4f} "
              f"(macro ROC-AUC {tuned['best_val_macro_roc_auc']:.4f}; trial 0, the untuned settings: {tuned['trials'][0]['best_val_loss']:.4f}) {win['params']}")
    if export:   # calibrated on all kept rows, reported over the validation rows (all rows when there are none)
        kept = tr | va
        export_probe_tflite(head, runner, args.model_path, emb.embeddings[kept], Y[kept], (va if va.any() else tr)[kept], out, args.activation,
                            bool(getattr(args, "per_tensor", False)), float(getattr(args, "min_cosine_sim", 0.95)),
                            dict(loss=imb["loss"], focal_gamma=imb["focal_gamma"]), logit_range=qat_range, qat=qat_report)
    head.history["seconds"] = {"embed": t_embed, "fit": t_fit}
    val = head.history["val_loss"]
    aug_s = head.history.get("augment_seconds")
    aug_note = f" of which augment + re-embed {sum(aug_s):.2f} s = {1e3 * sum(aug_s) / len(aug_s):.1f} ms per epoch" if aug_s else ""
    print(f"[probe] {int(tr.sum())} training rows x {head.embedding_dim}: embeddings {t_embed:.2f} s, fit {t_fit:.2f} s{aug_note} ({len(head.history['loss'])} epochs, "
          f"loss {head.history['loss'][-1]:.4f}" + (f", best val_loss {min(val):.4f}" if val else "") + f") -> {out['head']}")
    if emb.skipped:
        print(f"[probe] skipped {len(emb.skipped)} unreadable or empty files")
    return head
