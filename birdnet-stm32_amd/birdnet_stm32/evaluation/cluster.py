"""Clustering: spherical k-means over the rows of archives written by ``embed`` — which call types are in here?

``kmeans_reference`` is the specification in numpy; ``cluster_index`` runs the same fit on the device (``csrc/bn_kmeans.hip``, C ABI
``bn_kmeans_assign`` / ``bn_kmeans_accumulate`` / ``bn_kmeans_centroids``).  Both run the same host loop (``_lloyd``) and the same
``repair_empty_clusters``.  The metric is the cosine; Euclidean distance is out of scope, as it is for ``search``.

Rows.  The ``[N, D]`` rows are float32, or int8 bytes with a zero point; an int8 row means ``float32(byte - zero_point)``, which is exact,
and everything after that is float32.  ``inv[i]`` is ``search.inv_norms_reference(rows, zero_point)``: correctly rounded square root and
division, the sum of squares exact in int32 for int8 rows, 0 for a zero row.  Centroids ``C [K, D]`` are float32 with
``inv_c = inv_norms_reference(C)``.

Assignment.  ``score[i, c] = fl(fl(dot(x_i, C_c) * inv[i]) * inv_c[c])`` with a float32 dot product whose summation order is free;
``label[i]`` is the centroid with the highest score, the lowest index among equal scores.  For float32 rows that is
``search_reference(C, X, k=1, "cosine")`` with the centroids as the database, and ``assign_reference`` calls it (int8 rows take the same
formula with their exact ``inv``: ``search`` wants queries of the database's dtype).  One exception: a zero row gets label -1 and score 0
and takes no part in sums, counts or the changed count.

Update.  ``S_c`` is the float32 sum over the members of c of ``fl(inv[i] * x_i)`` (the summation order is the implementation's: the device
adds members in ascending row order, in segments); ``count[c]`` the member count; ``C_c = fl(S_c * inv_norm(S_c))`` where ``count[c] > 0``.
A cluster without members keeps its centroid and goes through ``repair_empty_clusters``.

Fit.  Assign; stop when no label changed; otherwise update, repair and go on, up to ``max_iter`` updates; after the last update one more
assignment, so labels and scores always belong to the returned centroids.  Seeded initialisation takes the rows
``np.sort(default_rng([seed, restart]).choice(nonzero_rows, K, replace=False))``, normalised; with ``n_init > 1`` the restart with the
highest mean score of the non-zero rows (summed in float64 on the host) is kept, the lowest restart index among equal means.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from birdnet_stm32.evaluation.search import inv_norms_reference, search_reference

MAX_K, MAX_D = 4096, 2048   # BN_KMEANS_MAX_K / BN_KMEANS_MAX_D (include/birdnet_hip.h)
REPAIR_EPS = np.float32(1.0 / 1024.0)


def _as_float(rows: np.ndarray, zero_point: int, dtype=np.float32) -> np.ndarray:
    rows = np.asarray(rows)
    if rows.dtype == np.int8:
        return (rows.astype(np.int32) - int(zero_point)).astype(dtype)
    return rows.astype(dtype)


def _inv_norms(rows: np.ndarray, zero_point: int, dtype) -> np.ndarray:
    if dtype == np.float32:
        return inv_norms_reference(rows, zero_point)
    x = _as_float(rows, zero_point, np.float64)
    n = np.sqrt((x * x).sum(axis=1))
    return np.divide(1.0, n, out=np.zeros_like(n), where=n > 0)


def assign_reference(rows, centroids, zero_point: int = 0, dtype=np.float32):
    """``(label [N] int64, score [N] dtype)`` of the module docstring; ``dtype=np.float64`` is the reference of the bound tests."""
    rows, C = np.asarray(rows), np.asarray(centroids)
    if rows.ndim != 2 or C.ndim != 2 or rows.shape[1] != C.shape[1]:
        raise ValueError(f"rows {rows.shape} and centroids {C.shape} must be [N, D] and [K, D]")
    inv = _inv_norms(rows, zero_point, dtype)
    if dtype == np.float32 and rows.dtype != np.int8:
        idx, sc = search_reference(C.astype(np.float32), rows.astype(np.float32), 1, "cosine")
        label, score = idx[:, 0].copy(), sc[:, 0].copy()
    else:
        x, c = _as_float(rows, zero_point, dtype), C.astype(dtype)
        inv_c = _inv_norms(c, 0, dtype)
        label, score = np.empty(rows.shape[0], np.int64), np.empty(rows.shape[0], dtype)
        step = max(1, (1 << 22) // max(C.shape[0], 1))
        for lo in range(0, rows.shape[0], step):
            s = ((x[lo:lo + step] @ c.T).astype(dtype) * inv[lo:lo + step, None]).astype(dtype) * inv_c[None, :]
            label[lo:lo + step] = np.argmax(s, axis=1)   # (the first of equal maxima: the lowest index)
            score[lo:lo + step] = s[np.arange(s.shape[0]), label[lo:lo + step]]
    zero = inv == 0
    label[zero], score[zero] = -1, 0
    return label, score


def update_reference(rows, labels, K: int, zero_point: int = 0, dtype=np.float32):
    """``(S [K, D] dtype, count [K] int64)``: sums of ``fl(inv[i] * x_i)`` over the members of every cluster, in ascending row order."""
    x = _as_float(rows, zero_point, dtype)
    inv = _inv_norms(rows, zero_point, dtype)
    labels = np.asarray(labels)
    S = np.zeros((K, x.shape[1]), dtype)
    counts = np.zeros(K, np.int64)
    order = np.argsort(labels, kind="stable")
    bounds = np.searchsorted(labels[order], np.arange(K + 1))
    for c in range(K):
        m = order[bounds[c]:bounds[c + 1]]
        counts[c] = m.size
        if m.size:
            S[c] = (x[m] * inv[m, None]).astype(dtype).sum(axis=0, dtype=dtype)
    return S, counts


def centroids_from_sums(S, counts, old, dtype=np.float32) -> np.ndarray:
    """``C_c = fl(S_c * inv_norm(S_c))`` where the cluster has members, the old centroid elsewhere."""
    S = np.asarray(S, dtype)
    C = np.array(old, dtype)
    has = np.asarray(counts) > 0
    C[has] = (S * _inv_norms(S, 0, dtype)[:, None]).astype(dtype)[has]
    return C


def repair_empty_clusters(centroids, counts):
    """Give every cluster without members half of the largest one: ``(centroids float32, counts int64, repaired)``.

    The empty clusters j in ascending order; L the cluster with the largest count (lowest index among ties).  With ``counts[L] < 2`` j is
    left alone.  Otherwise ``C_j`` becomes ``C_L`` with even dimensions times ``1 + 1/1024`` and odd dimensions times ``1 - 1/1024``,
    ``C_L`` the mirror image, both renormalised; ``counts[j] = counts[L] // 2`` and ``counts[L] -= counts[j]``.  float32 numpy on the
    host: the specification and the device fit share its bits."""
    C = np.array(centroids, np.float32)
    counts = np.array(counts, np.int64)
    up = np.where(np.arange(C.shape[1]) % 2 == 0, np.float32(1) + REPAIR_EPS, np.float32(1) - REPAIR_EPS).astype(np.float32)
    down = np.where(np.arange(C.shape[1]) % 2 == 0, np.float32(1) - REPAIR_EPS, np.float32(1) + REPAIR_EPS).astype(np.float32)
    repaired = 0
    for j in np.flatnonzero(counts == 0):
        L = int(np.argmax(counts))
        if counts[L] < 2:
            continue
        pair = np.stack([C[L] * up, C[L] * down]).astype(np.float32)
        pair = (pair * inv_norms_reference(pair)[:, None]).astype(np.float32)
        C[j], C[L] = pair[0], pair[1]
        counts[j] = counts[L] // 2
        counts[L] -= counts[j]
        repaired += 1
    return C, counts, repaired


def seeded_rows(inv: np.ndarray, K: int, seed: int, restart: int) -> np.ndarray:
    """The K distinct non-zero rows a seeded fit starts from, ascending."""
    nonzero = np.flatnonzero(np.asarray(inv) != 0)
    return np.sort(np.random.default_rng([int(seed), int(restart)]).choice(nonzero, int(K), replace=False))


def seeded_centroids(rows, zero_point: int, K: int, seed: int, restart: int, inv=None) -> np.ndarray:
    """The seeded start: the rows of ``seeded_rows``, normalised (``inv``: the rows' inverse norms where the caller has them)."""
    if inv is None:
        inv = inv_norms_reference(rows, zero_point)
    pick = seeded_rows(inv, K, seed, restart)
    return (_as_float(np.asarray(rows)[pick], zero_point) * inv[pick, None]).astype(np.float32)


def check_fit_args(n_rows: int, D: int, n_nonzero: int, k: int, max_iter: int, n_init: int, init_centroids=None):
    """Everything a fit refuses; returns ``init_centroids`` as float32 [K, D] or None."""
    k, max_iter, n_init = int(k), int(max_iter), int(n_init)
    if not 1 <= D <= MAX_D:
        raise ValueError(f"embedding width {D} outside 1..{MAX_D}")
    if k < 1:
        raise ValueError(f"k={k} must be >= 1")
    if k > MAX_K:
        raise ValueError(f"k={k} above the {MAX_K} clusters a fit holds")
    if k > n_nonzero:
        raise ValueError(f"k={k} above the number of non-zero rows ({n_nonzero} of {n_rows})")
    if max_iter < 0 or n_init < 1:
        raise ValueError("max_iter must be >= 0 and n_init >= 1")
    if init_centroids is None:
        return None
    C = np.ascontiguousarray(init_centroids, np.float32)
    if C.shape != (k, D):
        raise ValueError(f"init_centroids must be [{k}, {D}], got {C.shape}")
    if not np.isfinite(C).all():
        raise ValueError("init_centroids hold values that are not finite")
    return C


def mean_score(score: np.ndarray, labels: np.ndarray) -> float:
    """Mean score of the rows that have a cluster, summed in float64."""
    m = np.asarray(labels) >= 0
    return float(np.asarray(score)[m].astype(np.float64).sum() / max(int(m.sum()), 1))


def _lloyd(backend, max_iter: int):
    """The fit's loop over a backend with ``assign() -> changed`` and ``update()``: ``(n_iter, converged)``."""
    n_iter = 0
    while True:
        if backend.assign() == 0:
            return n_iter, True
        if n_iter >= max_iter:
            return n_iter, False
        backend.update()
        n_iter += 1


@dataclass
class ClusterResult:
    """``labels`` [N] (-1 for a zero row), ``score`` [N], ``centroids`` [K, D] float32, ``counts`` [K] members under the returned labels,
    ``mean_score`` over the rows with a cluster, ``n_iter`` updates taken, ``converged``, and per centroid its ``exemplars`` best rows
    (``exemplar_idx`` -1 / ``exemplar_score`` -inf where the index has fewer)."""

    labels: np.ndarray
    score: np.ndarray
    centroids: np.ndarray
    counts: np.ndarray
    mean_score: float
    n_iter: int
    converged: bool
    exemplar_idx: np.ndarray
    exemplar_score: np.ndarray
    restart: int = 0


class _NumpyBackend:
    def __init__(self, rows, zero_point, centroids, dtype):
        self.rows, self.zp, self.dtype = rows, zero_point, dtype
        self.C = np.array(centroids, np.float32)
        self.labels = None
        self.score = None

    def result(self):
        return self.labels, self.score, self.C

    def assign(self) -> int:
        prev = self.labels
        self.labels, self.score = assign_reference(self.rows, self.C, self.zp, self.dtype)
        live = self.labels >= 0
        return int(live.sum()) if prev is None else int((self.labels[live] != prev[live]).sum())

    def update(self) -> None:
        S, counts = update_reference(self.rows, self.labels, self.C.shape[0], self.zp, self.dtype)
        C = centroids_from_sums(S, counts, self.C, self.dtype).astype(np.float32)
        self.C, _, _ = repair_empty_clusters(C, counts)


def _finish(labels, score, C, n_iter, converged, restart) -> ClusterResult:
    K = C.shape[0]
    counts = np.bincount(labels[labels >= 0], minlength=K).astype(np.int64)
    none_i, none_s = np.zeros((K, 0), np.int64), np.zeros((K, 0), np.float32)
    return ClusterResult(labels.astype(np.int64), np.asarray(score), C, counts, mean_score(score, labels), int(n_iter), bool(converged), none_i, none_s, restart)


def _fit(make_backend, inv, rows, zero_point, k, max_iter, n_init, seed, init) -> ClusterResult:
    best = None
    for restart in range(1 if init is not None else int(n_init)):
        C0 = init if init is not None else seeded_centroids(rows, zero_point, k, seed, restart, inv)
        b = make_backend(C0)
        n_iter, converged = _lloyd(b, int(max_iter))
        labels, score, C = b.result()
        res = _finish(labels, score, C, n_iter, converged, restart)
        if best is None or res.mean_score > best.mean_score:
            best = res
    return best


def kmeans_reference(rows, k: int, max_iter: int = 25, n_init: int = 1, seed: int = 42, init_centroids=None, zero_point: int = 0,
                     dtype=np.float32) -> ClusterResult:
    """The fit of the module docstring in numpy (``dtype=np.float64``: scores, sums and norms in float64; the centroids stay float32)."""
    rows = np.asarray(rows)
    if rows.ndim != 2:
        raise ValueError(f"rows must be [N, D], got {rows.shape}")
    if rows.dtype != np.int8:
        rows = rows.astype(np.float32)
        if not np.isfinite(rows).all():
            raise ValueError("the rows hold values that are not finite")
    inv = inv_norms_reference(rows, zero_point)
    init = check_fit_args(rows.shape[0], rows.shape[1], int((inv != 0).sum()), k, max_iter, n_init, init_centroids)
    return _fit(lambda C0: _NumpyBackend(rows, zero_point, C0, dtype), inv, rows, zero_point, int(k), max_iter, n_init, seed, init)


# ---------------------------------------------------------------------------------------------------------------------- device
class _DeviceBackend:
    """The rows of an ``EmbeddingIndex`` on the device: resident when they fit the index's budget (the block ``search`` keeps is reused
    and left behind for it), streamed block by block per iteration otherwise.  Labels, scores and centroids stay on the device; per
    iteration the host reads the changed count and the K counts, and the centroids only when a cluster came out empty."""

    def __init__(self, index, ctx, centroids):
        import ctypes

        import torch

        from birdnet_stm32 import _hip

        self.torch, self.hip, self.index, self.ctx = torch, _hip, index, ctx
        self.dev = torch.device("cuda", ctx.device)
        self.code = index.dtype_code
        self.N, self.D, self.K = len(index), index.dim, int(centroids.shape[0])
        self.blocks = index.block_ranges()
        with torch.cuda.device(self.dev):
            self.stream = torch.cuda.current_stream(self.dev)
            self.sp = ctypes.c_void_p(self.stream.cuda_stream)
            self.d_label = [torch.full((max(self.N, 1),), -1, dtype=torch.int32, device=self.dev) for _ in range(2)]
            self.d_score = torch.zeros(max(self.N, 1), dtype=torch.float32, device=self.dev)
            self.d_changed = torch.zeros(1, dtype=torch.int64, device=self.dev)
            self.d_sums = torch.zeros((self.K, self.D), dtype=torch.float32, device=self.dev)
            self.d_counts = torch.zeros(self.K, dtype=torch.int64, device=self.dev)
            self.d_cinv = torch.empty(self.K, dtype=torch.float32, device=self.dev)
        self.cur, self.have_prev = 0, False
        self.set_centroids(centroids)

    def set_centroids(self, C) -> None:
        torch = self.torch
        with torch.cuda.device(self.dev):
            self.d_C = torch.from_numpy(np.ascontiguousarray(C, np.float32)).to(self.dev)
            self.hip.check(self.ctx.lib.bn_search_inv_norms(self.ctx.handle, self.d_C.data_ptr(), self.hip.DTYPE_F32, self.K, self.D, 0, self.d_cinv.data_ptr(), self.sp))

    def _block(self, lo, hi):
        """Rows lo .. hi and their inverse norms on the device (the index's own upload and cache)."""
        return self.index.device_block(self.ctx, lo, hi, self.sp)[:2]

    def assign(self) -> int:
        torch, lib, h = self.torch, self.ctx.lib, self.ctx.handle
        new, old = self.d_label[self.cur ^ 1], self.d_label[self.cur]
        changed = 0
        with torch.cuda.device(self.dev):
            for lo, hi in self.blocks:
                if hi == lo:
                    continue
                d_rows, d_inv = self._block(lo, hi)
                self.hip.check(lib.bn_kmeans_assign(h, d_rows.data_ptr(), self.code, hi - lo, self.D, self.index.zero_point, d_inv.data_ptr(), self.d_C.data_ptr(),
                                                    self.d_cinv.data_ptr(), self.K, old[lo:].data_ptr() if self.have_prev else None, new[lo:].data_ptr(),
                                                    self.d_score[lo:].data_ptr(), self.d_changed.data_ptr(), self.sp))
                changed += int(self.d_changed.item())
        self.cur ^= 1
        self.have_prev = True
        return changed

    def update(self) -> None:
        torch, lib, h = self.torch, self.ctx.lib, self.ctx.handle
        label = self.d_label[self.cur]
        with torch.cuda.device(self.dev):
            first = True
            for lo, hi in self.blocks:
                if hi == lo:
                    continue
                d_rows, d_inv = self._block(lo, hi)
                self.hip.check(lib.bn_kmeans_accumulate(h, d_rows.data_ptr(), self.code, hi - lo, self.D, self.index.zero_point, d_inv.data_ptr(),
                                                        label[lo:].data_ptr(), self.K, 0 if first else 1, self.d_sums.data_ptr(), self.d_counts.data_ptr(), self.sp))
                first = False
            self.hip.check(lib.bn_kmeans_centroids(h, self.d_sums.data_ptr(), self.d_counts.data_ptr(), self.K, self.D, self.d_C.data_ptr(), self.d_cinv.data_ptr(),
                                                   self.sp))
            counts = self.d_counts.cpu().numpy()
            if (counts == 0).any():
                C, _, repaired = repair_empty_clusters(self.d_C.cpu().numpy(), counts)
                if repaired:
                    self.set_centroids(C)

    def result(self):
        labels = self.d_label[self.cur][:self.N].cpu().numpy().astype(np.int64)
        return labels, self.d_score[:self.N].cpu().numpy(), self.d_C.cpu().numpy()


def cluster_index(index, k: int, max_iter: int = 25, n_init: int = 1, seed: int = 42, init_centroids=None, exemplars: int = 0, ctx=None,
                  device: int = 0) -> ClusterResult:
    """Spherical k-means over the rows of an ``EmbeddingIndex`` on the device; ``exemplars`` > 0 adds the best rows per centroid, which
    is ``index.search(centroids, k=exemplars)`` (float32 indexes only: ``search`` needs queries of the database's dtype)."""
    from birdnet_stm32.evaluation.search import MAX_K as SEARCH_MAX_K

    exemplars = int(exemplars)
    if exemplars < 0 or exemplars > SEARCH_MAX_K:
        raise ValueError(f"exemplars={exemplars} outside 0..{SEARCH_MAX_K}")
    if exemplars and index.dtype == "int8":
        raise ValueError("exemplars are found by `search`, which needs queries of the database's dtype: the centroids of an int8 index are "
                         "float32 (cluster a float32 archive, or pass exemplars=0)")
    inv = inv_norms_reference(index.embeddings, index.zero_point)
    init = check_fit_args(len(index), index.dim, int((inv != 0).sum()), k, max_iter, n_init, init_centroids)
    ctx = index.context(ctx, device)
    res = _fit(lambda C0: _DeviceBackend(index, ctx, C0), inv, index.embeddings, index.zero_point, int(k), max_iter, n_init, seed, init)
    if exemplars:
        hits = index.search(res.centroids, k=exemplars, metric="cosine", ctx=ctx)
        res.exemplar_idx, res.exemplar_score = hits.idx, hits.score
    return res


def centroid_archive(centroids: np.ndarray) -> dict:
    """The centroids as the keys of an ``embed`` archive: one row per path ``cluster_000``, ``cluster_001``, ... with ``start_s`` 0, so
    ``search --query_npz`` and ``EmbeddingIndex.from_npz`` take it as it stands."""
    C = np.ascontiguousarray(centroids, np.float32)
    K = C.shape[0]
    return dict(embeddings=C, file_index=np.arange(K, dtype=np.int64), start_s=np.zeros(K, np.float64), paths=np.asarray([f"cluster_{c:03d}" for c in range(K)]))
