"""Hyperparameter search for the probe's head (reference: ``train --tune --n_trials N``, training/tuner.py, which uses Optuna).

The reference trains its trials one after another and lets a sampler steer them.  Here all trials are drawn up front and trained at once
on the device (``linear_probe.fit_probe_sweep``, ``csrc/bn_probe_sweep.hip``): one fit is launch-bound at small batches, so the trials
share its launches.  Measured at batch 32: 16 trials take 1.00 x (C = 12) to 1.21 x (C = 1000) the time of 4, and are 12.8
to 15.7 x faster than 16 fits in a row; the gain shrinks as batch and class count fill the GPU.
No Optuna: the draws are independent, from numpy's generator, reproducible from a seed.

* ``sample_trials``  the trials of a search over the reference's space,
* ``tune_report``    what ``probe --tune`` writes as ``<output>_tune.json``.

The objective is the validation loss, not the reference's validation ROC-AUC: on small separable sets the AUC saturates at 1 and ties,
and the loss is what early stopping already ranks epochs by.  The winner's macro ROC-AUC is reported next to it.
"""

from __future__ import annotations

import math

import numpy as np

from birdnet_stm32.training.linear_probe import ProbeTrial, SweepResult

TUNE_STREAM = 0x74756E65   # "tune": the second word of the generator's seed, so the draws share nothing with the fit's own streams
LEARNING_RATE_RANGE = (1e-4, 1e-2)                      # log-uniform
DROPOUT_CHOICES = (0.2, 0.3, 0.4, 0.5, 0.6, 0.7)
LABEL_SMOOTHING_CHOICES = (0.0, 0.05, 0.1, 0.15, 0.2)
OPTIMIZER_CHOICES = ("adam", "adamw")
WEIGHT_DECAY_RANGE = (1e-5, 1e-2)                       # log-uniform, adamw only
GRAD_CLIP_CHOICES = (0.0, 1.0, 2.0, 3.0, 4.0, 5.0)
MAX_TRIALS = 64                                         # BN_PROBE_SWEEP_MAX_TRIALS


def _log_uniform(rng, lo: float, hi: float) -> float:
    return float(10.0 ** rng.uniform(math.log10(lo), math.log10(hi)))


def sample_trials(n: int, seed: int, base: ProbeTrial) -> list:
    """``n`` trials.  Trial 0 is ``base`` (the caller's own settings), so the search never returns worse than the untuned run on the
    validation set.  Trials 1 .. n-1 come from ``default_rng([seed, TUNE_STREAM])``, six draws per trial in this order, all six always
    taken so that one trial's choices never shift the next trial's draws:

    1. ``learning_rate``    log-uniform in ``LEARNING_RATE_RANGE``,
    2. ``dropout``          one of ``DROPOUT_CHOICES``,
    3. ``label_smoothing``  one of ``LABEL_SMOOTHING_CHOICES``,
    4. ``optimizer``        one of ``OPTIMIZER_CHOICES``,
    5. ``weight_decay``     log-uniform in ``WEIGHT_DECAY_RANGE``; kept for adamw, 0 otherwise,
    6. ``clipnorm``         one of ``GRAD_CLIP_CHOICES`` (the reference's ``grad_clip``).
    """
    n = int(n)
    if not 1 <= n <= MAX_TRIALS:
        raise ValueError(f"n_trials must be in 1..{MAX_TRIALS}, got {n}")
    if not isinstance(base, ProbeTrial):
        raise ValueError("base must be a ProbeTrial")
    rng = np.random.default_rng([int(seed), TUNE_STREAM])
    trials = [base]
    for _ in range(n - 1):
        lr = _log_uniform(rng, *LEARNING_RATE_RANGE)
        dropout = DROPOUT_CHOICES[int(rng.integers(len(DROPOUT_CHOICES)))]
        smoothing = LABEL_SMOOTHING_CHOICES[int(rng.integers(len(LABEL_SMOOTHING_CHOICES)))]
        optimizer = OPTIMIZER_CHOICES[int(rng.integers(len(OPTIMIZER_CHOICES)))]
        decay = _log_uniform(rng, *WEIGHT_DECAY_RANGE)
        clip = GRAD_CLIP_CHOICES[int(rng.integers(len(GRAD_CLIP_CHOICES)))]
        trials.append(ProbeTrial(learning_rate=lr, optimizer=optimizer, weight_decay=decay if optimizer == "adamw" else 0.0, clipnorm=clip, dropout=dropout,
                                 label_smoothing=smoothing))
    return trials


def check_tune_args(args) -> None:
    """The refusals of ``probe --tune`` that need no model: raised before anything is loaded."""
    if not getattr(args, "tune", False):
        return
    if not 1 <= int(args.n_trials) <= MAX_TRIALS:
        raise ValueError(f"--n_trials must be in 1..{MAX_TRIALS}, got {args.n_trials}")
    if not float(args.val_split) > 0:
        raise ValueError("--tune ranks the trials by their validation loss: it needs --val_split > 0")
    if float(getattr(args, "mixup_probability", 0.0) or 0.0) > 0 or getattr(args, "spec_augment", False):
        raise ValueError("--tune trains on fixed embeddings: it does not combine with --mixup_probability or --spec_augment")


def macro_roc_auc(y_true: np.ndarray, y_scores: np.ndarray) -> float:
    """The mean over classes of the per-class ROC-AUC (``evaluation._ranking.roc_auc_desc``, the curve ``ranking_metrics`` integrates),
    over the classes that have both positives and negatives among the rows; NaN when no class has."""
    from birdnet_stm32.evaluation._ranking import roc_auc_desc

    truth, scores = np.asarray(y_true) == 1, np.asarray(y_scores)
    aucs = []
    for c in range(scores.shape[1]):
        order = np.argsort(-scores[:, c], kind="stable")
        aucs.append(roc_auc_desc(truth[order, c], scores[order, c]))
    aucs = [a for a in aucs if not math.isnan(a)]
    return float(np.mean(aucs)) if aucs else float("nan")


def tune_report(result: SweepResult, roc_auc: float) -> dict:
    """Every trial's parameters, validation losses per epoch, best and stopped epoch and best validation loss; the winner and its
    validation macro ROC-AUC (``macro_roc_auc``)."""
    rows = []
    for i, (trial, head) in enumerate(zip(result.trials, result.heads)):
        h = head.history
        rows.append({"trial": i, "params": trial.fit_kwargs(), "val_loss": [float(v) for v in h["val_loss"]], "best_epoch": h["best_epoch"],
                     "stopped_epoch": h["stopped_epoch"], "best_val_loss": float(min(h["val_loss"])) if h["best_epoch"] is not None else None})
    return {"objective": "val_loss", "n_trials": len(rows), "best_trial": result.best, "best_val_macro_roc_auc": float(roc_auc), "trials": rows}
