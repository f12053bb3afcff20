"""Probe augmentation: per-epoch plans for mixup and SpecAugment, and the numpy specification of ``bn_augment_inputs``.

The reference's linear probe trains on augmented samples (reference: training/linear_probe.py:112-125): its loader masks every sample
with SpecAugment (data/generator.py:169-170, audio/augmentation.py:74-120) and then mixes 2-3 samples of each batch with Dirichlet gains,
taking the union of their labels (data/generator.py:406-418, audio/augmentation.py:10-71).  Here the un-augmented model inputs stay on the
device, a *plan* says per epoch which rows are masked where and which are mixed from which, ``csrc/bn_augment.hip`` builds the augmented
inputs from it, and the frozen backbone embeds them again (``training.linear_probe.fit_probe_augmented``).

Host only, numpy only:

* ``ProbeAugmentation``   the settings (the reference CLI's names; everything off by default here),
* ``augment_plan``        the plan of one epoch from ``default_rng([seed, epoch])``,
* ``mixed_targets``       the label rows of a plan: the element-wise maximum over each row's sources,
* ``augment_reference``   what ``bn_augment_inputs`` computes, rounding for rounding: the specification the kernel is tested against.

Two differences from the reference, both on purpose:

1. The reference draws a row's partners from the same *batch* and mixes ``int(batch * p)`` rows of every batch.  Here partners come from
   the whole training set and ``int(n * p)`` rows are mixed per epoch: the rows are resident, and the epoch's batches are cut afterwards.
2. The reference's loop mixes *in place* (audio/augmentation.py:50-64), so a row mixed earlier in a batch can be a later row's partner
   and carries its mix and its labels along.  Here every source is an un-mixed, masked row: one parallel pass over the rows cannot
   reproduce that chain.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MAX_MASKS = 4   # BN_AUGMENT_MAX_MASKS (include/birdnet_hip.h): masks per axis and row
MIN_MIXUP_ALPHA = 0.01


@dataclass(frozen=True)
class ProbeAugmentation:
    """Mixup and SpecAugment settings.  The reference's CLI has ``mixup_probability=0.25`` and SpecAugment on; here both are off unless
    asked for, so that a plain ``probe`` run stays what it was."""

    mixup_alpha: float = 0.2
    mixup_probability: float = 0.0
    spec_augment: bool = False
    freq_mask_max: int = 8
    time_mask_max: int = 25
    num_freq_masks: int = 2
    num_time_masks: int = 2

    def __post_init__(self):
        p = float(self.mixup_probability)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"mixup_probability must be in [0, 1], not {self.mixup_probability}")
        if p > 0 and not float(self.mixup_alpha) >= MIN_MIXUP_ALPHA:
            raise ValueError(f"mixup_alpha must be >= {MIN_MIXUP_ALPHA} while mixup is on (the gamma draws behind the Dirichlet gains underflow "
                             f"to 0/0 below that), not {self.mixup_alpha}")
        for name in ("freq_mask_max", "time_mask_max", "num_freq_masks", "num_time_masks"):
            if int(getattr(self, name)) < 0:
                raise ValueError(f"{name} must be >= 0, not {getattr(self, name)}")
        for name in ("num_freq_masks", "num_time_masks"):
            if int(getattr(self, name)) > MAX_MASKS:
                raise ValueError(f"{name} must be <= {MAX_MASKS}, not {getattr(self, name)}")

    @property
    def mixup(self) -> bool:
        return float(self.mixup_probability) > 0

    @property
    def active(self) -> bool:
        return self.mixup or bool(self.spec_augment)


@dataclass
class AugmentPlan:
    """One epoch's augmentation of ``n`` rows of ``F * W`` elements.

    ``nsrc [n]`` int32 in 1..3; ``src [n, 3]`` int32 source rows (slot 0 is the row itself in ``augment_plan``'s plans; slots past ``nsrc``
    repeat it and are not read); ``gain [n, 3]`` float32 (``1, 0, 0`` on copy rows); ``fmask [n_rows, nf, 2]`` / ``tmask [n_rows, nt, 2]``
    int32 ``(start, width)`` per SOURCE row, or ``None``."""

    nsrc: np.ndarray
    src: np.ndarray
    gain: np.ndarray
    fmask: np.ndarray | None
    tmask: np.ndarray | None
    F: int = 1
    W: int = 0

    @property
    def rows(self) -> int:
        return int(self.nsrc.shape[0])

    def touched(self) -> np.ndarray:
        """Mask of output rows that can differ from their un-augmented row: mixed, or with a source whose masks are not all empty."""
        hit = self.nsrc > 1
        for tab in (self.fmask, self.tmask):
            if tab is not None and tab.shape[1]:
                hit = hit | (tab[self.src[:, 0], :, 1] > 0).any(axis=1)
        return hit


def check_plan(plan: AugmentPlan, n_rows: int) -> None:
    """What the device cannot check for itself: counts in 1..3, sources in ``[0, n_rows)``, table shapes, starts and widths >= 0."""
    m = plan.rows
    if plan.nsrc.dtype != np.int32 or plan.src.dtype != np.int32 or plan.gain.dtype != np.float32:
        raise ValueError("nsrc and src must be int32, gain float32")
    if plan.src.shape != (m, 3) or plan.gain.shape != (m, 3):
        raise ValueError(f"src and gain must be [{m}, 3], got {plan.src.shape} and {plan.gain.shape}")
    if m and not (plan.nsrc.min() >= 1 and plan.nsrc.max() <= 3):
        raise ValueError("nsrc must be in 1..3")
    if m and not (plan.src.min() >= 0 and plan.src.max() < n_rows):
        raise ValueError(f"src must be in [0, {n_rows})")
    if int(plan.F) < 1 or int(plan.W) < 1:
        raise ValueError(f"bad row shape {plan.F} x {plan.W}")
    for name, tab in (("fmask", plan.fmask), ("tmask", plan.tmask)):
        if tab is None:
            continue
        if tab.dtype != np.int32 or tab.ndim != 3 or tab.shape[0] != n_rows or tab.shape[2] != 2 or not 1 <= tab.shape[1] <= MAX_MASKS:
            raise ValueError(f"{name} must be int32 [{n_rows}, 1..{MAX_MASKS}, 2], got {tab.dtype} {tab.shape}")
        if tab.min() < 0:
            raise ValueError(f"{name}: starts and widths must be >= 0")


def _draw_masks(rng, n: int, count: int, max_width: int, size: int) -> np.ndarray | None:
    """``[n, count, 2]`` (start, width): width = integers(0, max(1, min(max_width, size))), start = integers(0, max(1, size - width))
    (reference: audio/augmentation.py:107-116, the same two formulas on both axes; the upper ends are exclusive)."""
    if count == 0:
        return None
    width = rng.integers(0, max(1, min(int(max_width), size)), size=(n, count))
    start = rng.integers(0, np.maximum(1, size - width))
    return np.stack([start, width], axis=2).astype(np.int32)


def augment_plan(n: int, F: int, W: int, aug: ProbeAugmentation, seed: int, epoch: int) -> AugmentPlan:
    """The plan of epoch ``epoch`` for ``n`` rows of ``F x W`` elements (the raw frontend: ``F = 1``).

    Every draw comes from ``np.random.default_rng([seed, epoch])``, in this order:

    1. masks for all rows (only with ``spec_augment`` and ``F > 1``: the reference masks the four spectrogram frontends, never the raw
       one, data/generator.py:169): the frequency widths ``[n, num_freq_masks]`` in one call, the frequency starts, the time widths
       ``[n, num_time_masks]``, the time starts;
    2. the mixed rows (only with ``mixup_probability > 0``): ``choice(n, int(n * p), replace=False)`` (reference:
       audio/augmentation.py:44-48), then for each of them in ascending row order: the number of sources ``integers(2, 4)`` (:52), the
       partners ``choice(n, k - 1, replace=False)`` (:53; distinct from each other, possibly the row itself, as there), the gains
       ``dirichlet([alpha] * k)`` cast to float32 (:57).

    The module docstring states the two differences from the reference (partners from the whole set; no chained mixes)."""
    n, F, W = int(n), int(F), int(W)
    if n < 1 or F < 1 or W < 1:
        raise ValueError(f"need n >= 1 rows of F x W >= 1 x 1 elements, got n={n} F={F} W={W}")
    rng = np.random.default_rng([int(seed), int(epoch)])
    fmask = tmask = None
    if aug.spec_augment and F > 1:
        fmask = _draw_masks(rng, n, int(aug.num_freq_masks), aug.freq_mask_max, F)
        tmask = _draw_masks(rng, n, int(aug.num_time_masks), aug.time_mask_max, W)
    own = np.arange(n, dtype=np.int32)
    nsrc = np.ones(n, np.int32)
    src = np.repeat(own[:, None], 3, axis=1)
    gain = np.zeros((n, 3), np.float32)
    gain[:, 0] = 1.0
    num_mix = int(n * float(aug.mixup_probability)) if aug.mixup else 0
    if num_mix > 0:
        alpha = float(aug.mixup_alpha)
        for r in np.sort(rng.choice(n, size=num_mix, replace=False)):
            k = int(rng.integers(2, 4))
            if k - 1 > n:   # fewer rows than partners: as many as there are
                k = n + 1
            nsrc[r] = k
            src[r, 1:k] = rng.choice(n, size=k - 1, replace=False)
            gain[r, :k] = rng.dirichlet([alpha] * k).astype(np.float32)
    return AugmentPlan(nsrc, src, gain, fmask, tmask, F, W)


def mixed_targets(Y: np.ndarray, plan: AugmentPlan) -> np.ndarray:
    """Label rows of the plan's output: the element-wise maximum over each row's sources (reference: audio/augmentation.py:64, the
    multi-label union)."""
    Y = np.asarray(Y)
    out = Y[plan.src[:, 0]].copy()
    for s in (1, 2):
        rows = np.flatnonzero(plan.nsrc > s)
        out[rows] = np.maximum(out[rows], Y[plan.src[rows, s]])
    return out


def masked_rows(x: np.ndarray, plan: AugmentPlan) -> np.ndarray:
    """``x [n_rows, F * W]`` with every row's own masks set to ``+0.0`` (a copy, float32 ``[n_rows, F, W]``)."""
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise ValueError("x must be float32")
    out = x.reshape(x.shape[0], int(plan.F), int(plan.W)).copy()
    for s in range(out.shape[0]):
        if plan.fmask is not None:
            for f0, w in plan.fmask[s]:
                out[s, f0 : f0 + w, :] = 0.0
        if plan.tmask is not None:
            for t0, w in plan.tmask[s]:
                out[s, :, t0 : t0 + w] = 0.0
    return out


def augment_reference(x: np.ndarray, plan: AugmentPlan) -> np.ndarray:
    """What ``bn_augment_inputs`` writes for ``x [n_rows, F * W]`` float32: ``[plan.rows, F * W]`` float32.

    Masks belong to the source row; a copy row is the masked source bit for bit; a mixed row is ``fl(fl(g0 v0) + fl(g1 v1))`` and, with
    three sources, ``fl(that + fl(g2 v2))``, every product and sum rounded to float32 — numpy's
    ``np.sum(gains[:, None] * masked[src], axis=0)``, whose reduction over the outer axis adds row by row.  numpy starts that reduction
    from its additive identity ``+0.0``, which changes one case only: a mix whose products are all ``-0.0`` is ``+0.0``, not ``-0.0``.
    The sum is written out here with that start, and the kernel adds in the same order."""
    x = np.asarray(x)
    check_plan(plan, x.shape[0])
    masked = masked_rows(x, plan).reshape(x.shape[0], -1)
    out = masked[plan.src[:, 0]]   # (fancy indexing copies)
    g = plan.gain
    for k in (2, 3):
        rows = np.flatnonzero(plan.nsrc == k)
        if not rows.size:
            continue
        acc = (np.float32(0.0) + g[rows, 0, None] * masked[plan.src[rows, 0]]) + g[rows, 1, None] * masked[plan.src[rows, 1]]
        if k == 3:
            acc = acc + g[rows, 2, None] * masked[plan.src[rows, 2]]
        out[rows] = acc
    return out
