"""Silhouette: how well does every row sit in its cluster, and was ``k`` a good one?  Scores any labelling of the rows of ``embed`` archives.

``silhouette_reference`` is the specification in numpy; ``silhouette_index`` runs the same pass on the device (``csrc/bn_silhouette.hip``,
C ABI ``bn_silhouette_means``, after one pass of ``bn_kmeans_accumulate``).  Both finish in ``silhouette_from_means``.  The distance is
the cosine distance ``d(i, j) = 1 - x^_i . x^_j`` of the normalised rows; Euclidean distance is out of scope, as it is for ``cluster``.

The identity.  With ``S_c`` the sum of the normalised members of cluster c and ``n_c`` their number,
``sum_{j in c} d(i, j) = n_c - x^_i . S_c``: the exact silhouette needs every row against the K sums once, not against every other row.

Rows.  The ``[N, D]`` rows are float32, or int8 bytes with a zero point, exactly as in ``cluster.py``; ``inv[i]`` is
``search.inv_norms_reference(rows, zero_point)``.

Live rows.  A row is live when ``inv[i] != 0`` and ``0 <= label[i] < K``.  Every other row — a zero row, ``density``'s noise label -1, a
label outside the range — takes no part in sums, counts or means and comes back with ``silhouette = NaN`` and ``nearest = -1``.

Sums, counts, weights.  ``S [K, D]`` and ``n [K]`` are ``cluster.update_reference`` over the live rows.  ``w[c] = float32(1 / n[c])``,
computed in float64 and rounded once; ``w[c] = 0`` for an empty cluster.

Mean cosines.  ``m[i, c] = fl(fl(dot(x_i, S_c) * inv[i]) * w[c])`` with a float32 dot product whose summation order is free: the
assignment's score formula with ``S`` as the centroids and ``w`` as their inverse norms.  Per live row ``own[i] = m[i, label[i]]``;
``other[i]`` is the highest ``m[i, c]`` over ``c != label[i]`` with ``n[c] > 0`` and ``nearest[i]`` that c, the lowest index among equal
values (non-live rows: ``own = other = 0``; a live row without another non-empty cluster: ``other = 0``, ``nearest = -1``).

Silhouette.  In float64 on the host, from the float32 ``own`` and ``other``: ``a = (1 - own) n_A / (n_A - 1)`` with ``n_A`` the count of
the row's own cluster — the term ``d(i, i)`` is taken as exactly 0, that is ``x^_i . x^_i := 1`` whatever the rounded product would be —
``b = 1 - other``, ``s = (b - a) / max(a, b)``; ``s = 0`` when ``n_A = 1`` or ``max(a, b) = 0`` (scikit-learn's conventions).

Refused: fewer than 2 non-empty clusters among the live rows, ``K`` outside 1..MAX_K, ``D`` outside 1..MAX_D, labels not of length N, rows
that are not finite.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from birdnet_stm32.evaluation.cluster import MAX_D, MAX_K, _as_float, _inv_norms, update_reference

SWEEP_MIN_K = 2
SWEEP_COLUMNS = ("k", "silhouette", "mean_score", "n_iter", "converged", "smallest_cluster", "largest_cluster")


@dataclass
class SilhouetteResult:
    """``silhouette`` [N] float64 (NaN for a row that is not live), ``own`` / ``other`` [N] the mean cosines to the row's own and its
    nearest other cluster, ``nearest`` [N] int64 that cluster (-1 for a row that is not live), ``cluster_mean`` [K] float64 over a
    cluster's live rows (NaN for an empty cluster), ``mean`` over all live rows, ``n_live``, ``counts`` [K] live members."""

    silhouette: np.ndarray
    own: np.ndarray
    other: np.ndarray
    nearest: np.ndarray
    cluster_mean: np.ndarray
    mean: float
    n_live: int
    counts: np.ndarray


def weights_from_counts(counts) -> np.ndarray:
    """``w[c] = float32(1 / n[c])``, 0 for an empty cluster."""
    n = np.asarray(counts, np.float64)
    return np.divide(1.0, n, out=np.zeros_like(n), where=n > 0).astype(np.float32)


def check_labelling(n_rows: int, D: int, labels, K) -> tuple[np.ndarray, int]:
    """Everything refused before a row is read: ``(labels int64 [N], K)``."""
    labels = np.asarray(labels)
    if labels.shape != (int(n_rows),):
        raise ValueError(f"labels must be [{n_rows}], got {labels.shape}")
    if not 1 <= D <= MAX_D:
        raise ValueError(f"embedding width {D} outside 1..{MAX_D}")
    labels = labels.astype(np.int64)
    K = int(labels.max()) + 1 if K is None and labels.size else int(K or 0)
    if not 1 <= K <= MAX_K:
        raise ValueError(f"K={K} outside 1..{MAX_K}")
    return labels, K


def live_labels(labels, inv, K: int) -> np.ndarray:
    """The labels with -1 on every row that is not live."""
    labels = np.asarray(labels, np.int64)
    return np.where((np.asarray(inv) != 0) & (labels >= 0) & (labels < K), labels, -1)


def means_reference(rows, labels, sums, weight, zero_point: int = 0, dtype=np.float32, inv=None):
    """``(own, other [N] dtype, nearest [N] int64)`` of the module docstring for given sums ``[K, D]`` and weights ``[K]`` (a cluster with
    weight 0 counts as empty).  ``inv``: the rows' inverse norms where the caller has them."""
    rows, S, w = np.asarray(rows), np.asarray(sums).astype(dtype), np.asarray(weight).astype(dtype)
    K, N = S.shape[0], rows.shape[0]
    inv = _inv_norms(rows, zero_point, dtype) if inv is None else np.asarray(inv).astype(dtype)
    lab = live_labels(labels, inv, K)
    x = _as_float(rows, zero_point, dtype)
    own, other, nearest = np.zeros(N, dtype), np.zeros(N, dtype), np.full(N, -1, np.int64)
    step = max(1, (1 << 22) // K)
    for lo in range(0, N, step):
        l = lab[lo:lo + step]
        r = np.arange(l.size)
        m = (((x[lo:lo + step] @ S.T).astype(dtype) * inv[lo:lo + step, None]).astype(dtype) * w[None, :]).astype(dtype)
        live = l >= 0
        own[lo:lo + step][live] = m[r[live], l[live]]
        cand = np.broadcast_to(w != 0, m.shape).copy()
        cand[r[live], l[live]] = False
        cand[~live] = False
        masked = np.where(cand, m, -np.inf)
        best = np.argmax(masked, axis=1)   # (the first of equal maxima: the lowest index)
        has = cand.any(axis=1)
        other[lo:lo + step][has] = m[r[has], best[has]]
        nearest[lo:lo + step][has] = best[has]
    return own, other, nearest


def silhouette_from_means(own, other, nearest, labels, counts) -> SilhouetteResult:
    """The silhouette of the module docstring in float64 from the mean cosines; the reference and the device path share it.  A row is
    live when it has a nearest other cluster (``nearest >= 0``), which every live row has once two clusters are non-empty."""
    own, other = np.asarray(own), np.asarray(other)
    nearest, labels, counts = np.asarray(nearest, np.int64), np.asarray(labels, np.int64), np.asarray(counts, np.int64)
    K = counts.shape[0]
    if int((counts > 0).sum()) < 2:
        raise ValueError(f"a silhouette needs at least 2 non-empty clusters among the live rows, got {int((counts > 0).sum())}")
    live = (nearest >= 0) & (labels >= 0) & (labels < K)
    n_a = counts[np.where(live, labels, 0)].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = (1.0 - own.astype(np.float64)) * n_a / (n_a - 1.0)
        b = 1.0 - other.astype(np.float64)
        top = np.maximum(a, b)
        s = (b - a) / top
    s[(n_a == 1) | (top == 0)] = 0.0
    s[~live] = np.nan
    lab = np.where(live, labels, K)
    tot = np.bincount(lab, weights=np.where(live, s, 0.0), minlength=K + 1)[:K]
    num = np.bincount(lab, minlength=K + 1)[:K]
    cluster_mean = np.divide(tot, num, out=np.full(K, np.nan), where=num > 0)
    n_live = int(live.sum())
    return SilhouetteResult(s, own, other, np.where(live, nearest, -1), cluster_mean, float(s[live].sum() / max(n_live, 1)), n_live, counts)


def _checked_rows(rows) -> np.ndarray:
    rows = np.asarray(rows)
    if rows.ndim != 2:
        raise ValueError(f"rows must be [N, D], got {rows.shape}")
    if rows.dtype != np.int8:
        rows = rows.astype(np.float32)
        if not np.isfinite(rows).all():
            raise ValueError("the rows hold values that are not finite")
    return rows


def silhouette_reference(rows, labels, K=None, zero_point: int = 0, dtype=np.float32) -> SilhouetteResult:
    """The silhouette of the module docstring in numpy; ``K=None`` means ``max(label) + 1``.  ``dtype=np.float64``: norms, sums, weights
    and mean cosines in float64, the reference of the bound tests."""
    rows = _checked_rows(rows)
    labels, K = check_labelling(rows.shape[0], rows.shape[1], labels, K)
    inv = _inv_norms(rows, zero_point, dtype)
    lab = live_labels(labels, inv, K)
    S, counts = update_reference(rows, lab, K, zero_point, dtype)
    if int((counts > 0).sum()) < 2:
        raise ValueError(f"a silhouette needs at least 2 non-empty clusters among the live rows, got {int((counts > 0).sum())}")
    n = counts.astype(np.float64)
    w = weights_from_counts(counts) if dtype == np.float32 else np.divide(1.0, n, out=np.zeros_like(n), where=n > 0)
    own, other, nearest = means_reference(rows, lab, S, w, zero_point, dtype, inv)
    return silhouette_from_means(own, other, nearest, lab, counts)


# ---------------------------------------------------------------------------------------------------------------------- device
def silhouette_index(index, labels, K=None, ctx=None, device: int = 0) -> SilhouetteResult:
    """The silhouette of ``labels`` over the rows of an ``EmbeddingIndex`` on the device: one pass of ``bn_kmeans_accumulate`` for the sums
    and counts, the weights on the host, one pass of ``bn_silhouette_means``.  The rows go through ``index.device_block`` as they do for
    ``cluster_index``: a resident block is reused and left behind, an index larger than its budget is streamed."""
    import ctypes

    import torch

    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation.search import inv_norms_reference

    labels, K = check_labelling(len(index), index.dim, labels, K)
    lab = live_labels(labels, inv_norms_reference(index.embeddings, index.zero_point), K)
    if len(np.unique(lab[lab >= 0])) < 2:
        raise ValueError(f"a silhouette needs at least 2 non-empty clusters among the live rows, got {len(np.unique(lab[lab >= 0]))}")
    ctx = index.context(ctx, device)
    N, D, code, zp = len(index), index.dim, index.dtype_code, index.zero_point
    dev = torch.device("cuda", ctx.device)
    blocks = [(lo, hi) for lo, hi in index.block_ranges() if hi > lo]
    lib, h = ctx.lib, ctx.handle
    with torch.cuda.device(dev):
        sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        d_label = torch.from_numpy(lab.astype(np.int32)).to(dev)
        d_sums = torch.zeros((K, D), dtype=torch.float32, device=dev)
        d_counts = torch.zeros(K, dtype=torch.int64, device=dev)
        d_own = torch.zeros(N, dtype=torch.float32, device=dev)
        d_other = torch.zeros(N, dtype=torch.float32, device=dev)
        d_nearest = torch.full((N,), -1, dtype=torch.int32, device=dev)
        for j, (lo, hi) in enumerate(blocks):
            d_rows, d_inv = index.device_block(ctx, lo, hi, sp)[:2]
            _hip.check(lib.bn_kmeans_accumulate(h, d_rows.data_ptr(), code, hi - lo, D, zp, d_inv.data_ptr(), d_label[lo:].data_ptr(), K, int(j > 0),
                                                d_sums.data_ptr(), d_counts.data_ptr(), sp))
        counts = d_counts.cpu().numpy()
        d_weight = torch.from_numpy(weights_from_counts(counts)).to(dev)
        for lo, hi in blocks:
            d_rows, d_inv = index.device_block(ctx, lo, hi, sp)[:2]
            _hip.check(lib.bn_silhouette_means(h, d_rows.data_ptr(), code, hi - lo, D, zp, d_inv.data_ptr(), d_label[lo:].data_ptr(), d_sums.data_ptr(),
                                               d_weight.data_ptr(), K, d_own[lo:].data_ptr(), d_other[lo:].data_ptr(), d_nearest[lo:].data_ptr(), sp))
        own, other, nearest = d_own.cpu().numpy(), d_other.cpu().numpy(), d_nearest.cpu().numpy().astype(np.int64)
    return silhouette_from_means(own, other, nearest, lab, counts)


# ----------------------------------------------------------------------------------------------------------------------- sweep
def check_sweep_ks(ks) -> list[int]:
    """The candidates of a sweep: ``sorted(set(ks))``, each in 2..MAX_K."""
    ks = sorted({int(k) for k in ks})
    if not ks:
        raise ValueError("a sweep needs at least one k")
    for k in ks:
        if not SWEEP_MIN_K <= k <= MAX_K:
            raise ValueError(f"k={k} outside {SWEEP_MIN_K}..{MAX_K}: a silhouette needs two clusters")
    return ks


def sweep(ks, fit, score):
    """``fit(k) -> ClusterResult`` and ``score(ClusterResult) -> SilhouetteResult`` for every candidate: ``(best ClusterResult, best
    SilhouetteResult, table)`` with the highest mean silhouette, the lowest k among equal means; ``table`` holds one dict of
    ``SWEEP_COLUMNS`` per candidate."""
    best, table = None, []
    for k in check_sweep_ks(ks):
        res = fit(k)
        sil = score(res)
        table.append(dict(k=k, silhouette=sil.mean, mean_score=res.mean_score, n_iter=res.n_iter, converged=res.converged,
                          smallest_cluster=int(res.counts.min()), largest_cluster=int(res.counts.max())))
        if best is None or sil.mean > best[1].mean:
            best = (res, sil)
    return best[0], best[1], table


def cluster_sweep(index, ks, max_iter: int = 25, n_init: int = 1, seed: int = 42, exemplars: int = 0, ctx=None, device: int = 0):
    """Fit every candidate k on the device with the same ``max_iter``, ``n_init`` and ``seed`` and score each with ``silhouette_index``:
    ``(best ClusterResult, best SilhouetteResult, table)``.  ``exemplars`` are found for the winner only."""
    from birdnet_stm32.evaluation.cluster import cluster_index
    from birdnet_stm32.evaluation.search import MAX_K as SEARCH_MAX_K

    ks, exemplars = check_sweep_ks(ks), int(exemplars)
    if exemplars < 0 or exemplars > SEARCH_MAX_K:
        raise ValueError(f"exemplars={exemplars} outside 0..{SEARCH_MAX_K}")
    if exemplars and index.dtype == "int8":
        raise ValueError("exemplars are found by `search`, which needs queries of the database's dtype: the centroids of an int8 index are "
                         "float32 (cluster a float32 archive, or pass exemplars=0)")
    ctx = index.context(ctx, device)
    res, sil, table = sweep(ks, lambda k: cluster_index(index, k, max_iter=max_iter, n_init=n_init, seed=seed, ctx=ctx),
                            lambda r: silhouette_index(index, r.labels, r.centroids.shape[0], ctx=ctx))
    if exemplars:
        hits = index.search(res.centroids, k=exemplars, metric="cosine", ctx=ctx)
        res.exemplar_idx, res.exemplar_score = hits.idx, hits.score
    return res, sil, table
