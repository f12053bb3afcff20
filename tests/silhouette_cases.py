"""Inputs and written-out bounds shared by test_silhouette_host.py and test_gpu_silhouette.py."""

import numpy as np

U = 2.0 ** -24   # unit roundoff of float32
SEGMENT_ROWS = 256   # BN_KMEANS_SEGMENT_ROWS (include/birdnet_hip.h)

# (N, D, K) of the oracle tests
ORACLE_SHAPES = [(300, 8, 3), (1000, 96, 100), (4099, 255, 17)]


def planted(N, D, K, seed=7, noise=0.5):
    """Rows around K planted unit directions, every cluster with at least one row (the first N clusters where N < K):
    ``(x float32 [N, D], lab int64 [N])``."""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((K, D))
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    lab = rng.integers(0, K, N)
    lab[:min(N, K)] = np.arange(min(N, K))
    x = (C[lab] + noise * rng.standard_normal((N, D)) / np.sqrt(D)).astype(np.float32)
    return x, lab.astype(np.int64)


def quantised(x, zero_point):
    """The planted rows as int8 bytes around ``zero_point`` (the scale uses the whole range)."""
    scale = min(127 - zero_point, 128 + zero_point) / np.abs(x).max()
    return np.clip(np.rint(x.astype(np.float64) * scale) + zero_point, -128, 127).astype(np.int8)


def as_float64(rows, zero_point=0):
    rows = np.asarray(rows)
    return rows.astype(np.float64) - zero_point if rows.dtype == np.int8 else rows.astype(np.float64)


def abs_means(rows, zero_point, inv, sums, weight):
    """``A[i, c] = sum_d |x_id| |S_cd| inv_i w_c`` in float64: what every rounding of a mean cosine is relative to."""
    x = np.abs(as_float64(rows, zero_point))
    return (x @ np.abs(np.asarray(sums, np.float64)).T) * np.asarray(inv, np.float64)[:, None] * np.asarray(weight, np.float64)[None, :]


def mean_cosine_bound(rows, zero_point, inv, sums, weight):
    """``|m - m64| <= (D + 3) u A[i, c]`` for m computed in float32 from the given float32 sums, weights and inverse norms: the dot
    product in any order is within D u of A (a fused chain rounds once per term; separate products and sums round every product once,
    relative to its own term, and D - 1 sums), the two factors round once each, and one u covers the second-order terms."""
    return (rows.shape[1] + 3) * U * abs_means(rows, zero_point, inv, sums, weight)


def separated_rows(m64, bound, lab):
    """Rows whose best and second-best other cluster the float64 means separate by more than the two bounds.  ``m64`` / ``bound`` [N, K]
    with -inf / 0 where a cluster is no candidate; rows with a single candidate are separated."""
    order = np.argsort(-m64, axis=1, kind="stable")
    r = np.arange(m64.shape[0])
    best, second = order[:, 0], order[:, 1] if m64.shape[1] > 1 else order[:, 0]
    gap = m64[r, best] - m64[r, second]
    return (lab >= 0) & ((gap > bound[r, best] + bound[r, second]) | ~np.isfinite(m64[r, second]))


def candidate_means(rows, zero_point, inv, sums, weight, lab):
    """Float64 means ``m64 [N, K]`` of the live rows against every cluster, and the same with -inf at the row's own cluster and at the
    clusters of weight 0: the candidates for ``other``."""
    x = as_float64(rows, zero_point)
    w = np.asarray(weight, np.float64)
    m = (x @ np.asarray(sums, np.float64).T) * np.asarray(inv, np.float64)[:, None] * w[None, :]
    cand = np.where(w[None, :] != 0, m, -np.inf)
    live = lab >= 0
    cand[np.flatnonzero(live), lab[live]] = -np.inf
    return m, cand
