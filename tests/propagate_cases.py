"""Inputs shared by test_propagate_host.py and test_gpu_propagate.py: the planted rows of the propagate tests and the matrices the step
kernel is held to bit for bit."""

import functools

import numpy as np

N, D, C, K, SEEDS = 240, 16, 5, 7, 20
TAU, ALPHA = 0.1, 0.2


@functools.lru_cache(maxsize=None)
def planted():
    """``(X [240, 16] float32, true [240], seed_label [240] int32)``: five noisy centres, twenty labelled rows."""
    rng = np.random.default_rng(0)
    cent = rng.standard_normal((C, D))
    true = rng.integers(0, C, N)
    X = np.abs(cent[true] + 0.6 * rng.standard_normal((N, D))).astype(np.float32)
    seeds = rng.choice(N, SEEDS, replace=False)
    seed_label = np.full(N, -1, np.int32)
    seed_label[seeds] = true[seeds]
    for a in (X, true, seed_label):
        a.setflags(write=False)
    return X, true, seed_label


def quantised(X, zero_point: int):
    """The planted rows as int8 bytes around ``zero_point``."""
    scale = float(np.abs(X).max()) / 100.0
    return np.clip(np.rint(X / scale) + zero_point, -128, 127).astype(np.int8)


def step_matrix(n: int, seed: int):
    """``(rowptr int64, col int32, val float32)`` for the step kernel at ``n`` rows: about six entries per row in ascending columns, values
    in (0, 1) that are no lattice (every product rounds), and from n = 17 on an empty row, a one-entry row, a hub of n - 1 entries and a
    column out of range on either side."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        m = int(min(n, rng.integers(1, 12)))
        rows.append(np.sort(rng.choice(n, m, replace=False)).astype(np.int64))
    if n >= 17:
        rows[3] = np.zeros(0, np.int64)
        rows[4] = np.asarray([n - 1], np.int64)
        rows[5] = np.asarray([j for j in range(n) if j != 5], np.int64)
        rows[6] = np.asarray([-3, 2, 9, n, n + 7], np.int64)   # (stored order; the outsiders contribute nothing)
    rowptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32) if rowptr[-1] else np.zeros(0, np.int32)
    val = (rng.random(col.size) * 0.5 + 0.01).astype(np.float32)
    return rowptr, col, val


def step_labels(n: int, classes: int, seed: int):
    """``(F [n, C] float32, seed_label [n] int32)``: values in [0, 1) with zeros among them, and labels that cover -1, every class now and
    then, and a class only one row holds."""
    rng = np.random.default_rng(seed + 1000)
    F = rng.random((n, classes)).astype(np.float32)
    F[rng.random((n, classes)) < 0.2] = 0.0
    lab = rng.integers(-1, classes, n).astype(np.int32)
    lab[0] = classes - 1
    if n > 1:
        lab[1] = -1
    return F, lab
