"""Projection: a 2-D t-SNE map of the rows of archives written by ``embed`` — every chunk a point, call types as islands.

``tsne_reference`` is the specification in numpy (float64 gradient over dense pairs, for small N); ``project_index`` runs the same fit on
the device (``csrc/bn_tsne.hip``, C ABI ``bn_tsne_perplexity`` / ``bn_tsne_gradient`` / ``bn_tsne_update``; neighbours from
``bn_search_topk``).  Both share every host-side step: the argument checks, ``symmetrize``, the start and the schedule (``_descend``).  It
is exact t-SNE with sparse (k-nearest-neighbour) affinities and exact all-pairs repulsion: van der Maaten's formulas, the constants of
scikit-learn 1.7's ``sklearn.manifold.TSNE``; no Barnes-Hut, no FFT.

1. Rows.  ``[N, D]`` float32, or int8 bytes with a zero point, with ``search``'s meaning.  Zero rows (``inv_norms_reference`` gives 0) take
   no part and come back as NaN coordinates; ``n`` is the number of the others, and fewer than 2 is refused.
2. Neighbours.  ``k = min(n - 1, floor(3 * perplexity))``; ``perplexity < 1``, ``perplexity >= n`` and ``3 * perplexity > 128``
   (``BN_SEARCH_MAX_K``) are refused.  The neighbours of a row are its ``k`` best cosine scores ``s`` among the other non-zero rows
   (``search`` of the rows against themselves, every row its own group), and ``d2 = max(0, fl(2 - 2 s))`` in float32.
3. Conditional affinities, float64.  For a row with distances ``d2_j`` and ``m = min d2``: ``p_j = exp(-beta (d2_j - m))``, ``S = sum p_j``,
   ``H = log S + beta sum (d2_j - m) p_j / S``.  ``beta`` starts at 1 and follows scikit-learn's ``_binary_search_perplexity``: doubled or
   halved while that side of its interval is unbounded, bisected afterwards, until ``|H - log(perplexity)| <= 1e-5`` or 100 values have
   been tried; the last value tried stands.  ``P_cond[i, j] = p_j / S``, stored as float32.
4. Symmetrisation (host).  ``P = (P_cond + P_cond^T) / (2 n)`` over the union of the two patterns, float64, stored as float32 in CSR with
   ascending columns; a row holds anything from 0 to n - 1 entries.
5. Start.  ``Y = float32(1e-4 * default_rng([seed]).standard_normal((n, 2)))``, update 0, gains 1 (``init="random"``, the default).  With
   ``init="pca"`` (scikit-learn's own default) the start is the first two principal-component scores of the non-zero rows, unwhitened
   (``evaluation/reduce.py``), scaled by scikit-learn's rule ``Y = float32(scores / std(scores[:, 0]) * 1e-4)``, the standard deviation with
   ddof 0 in float64 (``initial_map_pca``); it needs at least 3 non-zero rows and two components of positive variance.
6. Gradient.  With ``w_ij = 1 / (1 + |y_i - y_j|^2)`` and exaggeration E: ``A_i = sum_{j in row i of P} p_ij w_ij (y_i - y_j)``,
   ``R_i = sum_{j != i} w_ij^2 (y_i - y_j)``, ``Z = sum_i sum_{j != i} w_ij``, ``grad_i = 4 (E A_i - R_i / Z)``.  Summation orders and the
   reciprocal are the implementation's; Z is a float64 sum of float32 row sums on the device.  ``kl_i = sum_j p_ij log(p_ij / w_ij)`` over
   the entries with ``p_ij > 0``; the divergence of the unexaggerated P is ``sum_i kl_i + (sum_ij p_ij) log Z``, summed in float64 on the host
   (``sum_ij p_ij`` is 1 up to the float32 storage of P).
7. Update (scikit-learn's ``_gradient_descent``), element-wise in float32, every operation rounded, nothing fused:
   ``inc = update * grad < 0``; ``gains = inc ? gains + 0.2 : gains * 0.8``; ``gains = max(gains, 0.01)``;
   ``update = momentum * update - lr * (gains * grad)``; ``Y += update``.
8. Schedule.  ``n_iter`` iterations; E = ``early_exaggeration`` and momentum 0.5 for the first ``exaggeration_iter`` of them, then E = 1 and
   momentum 0.8; ``lr = max(n / early_exaggeration / 4, 50)`` unless given.  No early stopping.  The final map is centred on its mean in
   float64 on the host.  "KL at iteration t" is the divergence of the map after t updates.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from birdnet_stm32.evaluation.search import MAX_K as SEARCH_MAX_K
from birdnet_stm32.evaluation.search import inv_norms_reference, search_reference

PERPLEXITY_TOL, PERPLEXITY_STEPS = 1e-5, 100
MAX_N = 1 << 21   # BN_TSNE_MAX_N (include/birdnet_hip.h)


def neighbour_count(n: int, perplexity: float) -> int:
    return min(int(n) - 1, int(math.floor(3.0 * float(perplexity))))


def check_project_args(n: int, perplexity, n_iter, early_exaggeration, exaggeration_iter, learning_rate, kl_every=0) -> None:
    """Everything a fit over ``n`` non-zero rows refuses."""
    if n < 2:
        raise ValueError(f"a map needs at least 2 non-zero rows, the archive holds {n}")
    if not (float(perplexity) >= 1.0):
        raise ValueError(f"perplexity {perplexity} must be >= 1")
    if float(perplexity) >= n:
        raise ValueError(f"perplexity {perplexity} must be below the number of non-zero rows ({n})")
    if 3.0 * float(perplexity) > SEARCH_MAX_K:
        raise ValueError(f"perplexity {perplexity} above {SEARCH_MAX_K // 3}: 3 * perplexity neighbours must fit the {SEARCH_MAX_K} `search` returns")
    if int(n_iter) < 0 or int(exaggeration_iter) < 0 or int(kl_every) < 0:
        raise ValueError("n_iter, exaggeration_iter and kl_every must be >= 0")
    if not (math.isfinite(float(early_exaggeration)) and float(early_exaggeration) >= 1.0):
        raise ValueError(f"early_exaggeration {early_exaggeration} must be finite and >= 1")
    if learning_rate is not None and not (math.isfinite(float(learning_rate)) and float(learning_rate) > 0.0):
        raise ValueError(f"learning_rate {learning_rate} must be finite and > 0")


def default_learning_rate(n: int, early_exaggeration: float) -> float:
    return max(n / float(early_exaggeration) / 4.0, 50.0)


def squared_distances(score) -> np.ndarray:
    """``d2 = max(0, fl(2 - 2 s))`` in float32."""
    s = np.asarray(score, np.float32)
    return np.maximum(np.float32(0), np.float32(2) - np.float32(2) * s).astype(np.float32)


def row_entropy(d2, beta):
    """``(p [n, k] float64, H [n])`` of item 3 for given ``beta`` [n]."""
    d = np.asarray(d2, np.float64)
    d = d - d.min(axis=1, keepdims=True)
    p = np.exp(-np.asarray(beta, np.float64)[:, None] * d)
    S = p.sum(axis=1)
    H = np.log(S) + beta * (d * p).sum(axis=1) / S
    return p / S[:, None], H


def conditional_p_reference(score, perplexity: float):
    """``(P_cond [n, k] float64, beta [n] float64)`` from the cosine scores ``[n, k]`` of every row's neighbours."""
    d2 = squared_distances(score)
    n = d2.shape[0]
    target = math.log(float(perplexity))
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    active = np.ones(n, bool)
    for step in range(PERPLEXITY_STEPS):
        rows = np.flatnonzero(active)
        if rows.size == 0:
            break
        _, H = row_entropy(d2[rows], beta[rows])
        diff = H - target
        stop = (np.abs(diff) <= PERPLEXITY_TOL) | (step == PERPLEXITY_STEPS - 1)
        up, down = rows[~stop & (diff > 0)], rows[~stop & ~(diff > 0)]
        lo[up] = beta[up]
        beta[up] = np.where(np.isinf(hi[up]), beta[up] * 2.0, (beta[up] + hi[up]) / 2.0)
        hi[down] = beta[down]
        beta[down] = np.where(np.isinf(lo[down]), beta[down] / 2.0, (beta[down] + lo[down]) / 2.0)
        active[rows[stop]] = False
    p, _ = row_entropy(d2, beta)
    return p, beta


def symmetrize(idx, p_cond, n: int):
    """``(rowptr [n + 1] int64, col int32, val float32)``: ``(P_cond + P_cond^T) / (2 n)`` in CSR with ascending columns.  ``idx [n, k]`` are
    the neighbours' row numbers (an entry < 0 or on the diagonal is dropped), ``p_cond [n, k]`` their conditional affinities."""
    idx = np.asarray(idx, np.int64)
    p = np.asarray(p_cond, np.float64)
    if idx.shape != p.shape or idx.ndim != 2 or idx.shape[0] != n:
        raise ValueError(f"idx {idx.shape} and p_cond {p.shape} must both be [{n}, k]")
    i = np.repeat(np.arange(n, dtype=np.int64), idx.shape[1])
    j = idx.ravel()
    keep = (j >= 0) & (j < n) & (j != i)
    i, j, v = i[keep], j[keep], p.ravel()[keep]
    keys = np.concatenate([i * n + j, j * n + i])
    vals = np.concatenate([v, v])
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    if keys.size == 0:
        return np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)
    uniq, first = np.unique(keys, return_index=True)
    sums = np.add.reduceat(vals, first)   # (at most two terms per entry: one order)
    rowptr = np.searchsorted(uniq // n, np.arange(n + 1)).astype(np.int64)
    return rowptr, (uniq % n).astype(np.int32), (sums / (2.0 * n)).astype(np.float32)


@dataclass
class GradientReference:
    """``grad [n, 2]``, ``A``, ``R`` [n, 2], ``z_rows [n]``, ``Z``, ``kl_rows [n]`` in float64, and per row (and component) the sums of the
    absolute values of the terms of A, R and kl (``abs_A``, ``abs_R`` [n, 2], ``abs_kl`` [n]): what the device's error bounds are written against."""

    grad: np.ndarray
    A: np.ndarray
    R: np.ndarray
    z_rows: np.ndarray
    Z: float
    kl_rows: np.ndarray
    abs_A: np.ndarray
    abs_R: np.ndarray
    abs_kl: np.ndarray
    p_sum: float

    @property
    def kl(self) -> float:
        return kl_from_rows(self.kl_rows, self.p_sum, self.Z)


def kl_from_rows(kl_rows, p_sum: float, Z: float) -> float:
    """``sum_i kl_i + (sum_ij p_ij) log Z`` in float64."""
    return float(np.asarray(kl_rows, np.float64).sum() + float(p_sum) * math.log(float(Z)))


def gradient_reference(Y, rowptr, col, val, exaggeration: float = 1.0) -> GradientReference:
    """Item 6 in float64 over dense pairs."""
    y = np.asarray(Y, np.float64)
    n = y.shape[0]
    rowptr, col, p = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(val, np.float64)
    R, abs_R, z_rows = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n)
    step = max(1, (1 << 22) // n)
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        diff = y[lo:hi, None, :] - y[None, :, :]
        w = 1.0 / (1.0 + (diff * diff).sum(axis=2))
        w[np.arange(hi - lo), np.arange(lo, hi)] = 0.0
        z_rows[lo:hi] = w.sum(axis=1)
        t = (w * w)[:, :, None] * diff
        R[lo:hi], abs_R[lo:hi] = t.sum(axis=1), np.abs(t).sum(axis=1)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    diff = y[row] - y[col]
    d2 = 1.0 + (diff * diff).sum(axis=1)
    t = (p / d2)[:, None] * diff
    A, abs_A, kl_rows, abs_kl = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n), np.zeros(n)
    pos = p > 0
    tk = np.zeros(p.shape)
    tk[pos] = p[pos] * np.log(p[pos] * d2[pos])
    for c in range(2):
        A[:, c] = np.bincount(row, t[:, c], n)
        abs_A[:, c] = np.bincount(row, np.abs(t[:, c]), n)
    kl_rows, abs_kl = np.bincount(row, tk, n), np.bincount(row, np.abs(tk), n)
    Z = float(z_rows.sum())
    return GradientReference(4.0 * (float(exaggeration) * A - R / Z), A, R, z_rows, Z, kl_rows, abs_A, abs_R, abs_kl, float(p.sum()))


def update_reference(Y, grad, update, gains, lr: float, momentum: float):
    """Item 7: ``(Y, update, gains)`` after one step, float32, every operation rounded."""
    y, g, u, gains = (np.array(a, np.float32) for a in (Y, grad, update, gains))
    inc = (u * g) < np.float32(0)
    gains = np.where(inc, gains + np.float32(0.2), gains * np.float32(0.8)).astype(np.float32)
    gains = np.maximum(gains, np.float32(0.01))
    u = (np.float32(momentum) * u - np.float32(lr) * (gains * g)).astype(np.float32)
    return (y + u).astype(np.float32), u, gains


def initial_map(n: int, seed: int) -> np.ndarray:
    return (1e-4 * np.random.default_rng([int(seed)]).standard_normal((n, 2))).astype(np.float32)


INITS = ("random", "pca")


def check_init(init: str) -> str:
    if init not in INITS:
        raise ValueError(f"init must be one of {INITS}, not {init!r}")
    return init


def initial_map_pca(scores) -> np.ndarray:
    """scikit-learn's ``init="pca"`` start from the first two unwhitened scores ``[n, >= 2]``: ``scores / std(scores[:, 0]) * 1e-4``, the
    standard deviation with ddof 0, all in float64, rounded to float32 once."""
    s = np.asarray(scores, np.float64)
    if s.ndim != 2 or s.shape[0] < 3 or s.shape[1] < 2:
        raise ValueError(f"a PCA start needs at least 3 non-zero rows and 2 components, got scores of shape {s.shape}")
    s = s[:, :2]
    std = s.std(axis=0)
    if not (np.isfinite(std).all() and (std > 0).all()):
        raise ValueError("a PCA start needs two components of positive variance")
    return (s / std[0] * 1e-4).astype(np.float32)


def _pca_model_for_start(fit, n: int):
    """The two-component model of a PCA start from ``fit(n_components)``, its refusals worded for the map."""
    if n < 3:
        raise ValueError(f"init='pca' needs at least 3 non-zero rows, the archive holds {n}")
    from birdnet_stm32.evaluation.reduce import WHITEN_FLOOR

    model = fit(2)
    if not model.explained_variance[1] > WHITEN_FLOOR * model.explained_variance[0]:   # (anything below is the rounding noise of the spectrum)
        raise ValueError("init='pca' needs two components of positive variance")
    return model


@dataclass
class ProjectionResult:
    """``xy`` [N, 2] float32 (NaN for a zero row), ``kl`` of the final map, ``kl_history`` as (iteration, kl) pairs (every ``kl_every``
    iterations, and the last), ``beta`` [N] float64 (NaN for a zero row), ``n_iter``; ``trajectory`` holds the uncentred maps of the
    non-zero rows after the iterations asked for with ``snapshots``."""

    xy: np.ndarray
    kl: float
    kl_history: list
    beta: np.ndarray
    n_iter: int
    trajectory: dict = field(default_factory=dict)


def _descend(backend, n: int, n_iter: int, early_exaggeration: float, exaggeration_iter: int, lr: float, kl_every: int, snapshots=()):
    """The schedule over a backend with ``gradient(E, want_kl) -> kl or None``, ``update(lr, momentum)`` and ``map()``:
    ``(kl, kl_history, trajectory)``."""
    history, trajectory = [], {}
    snapshots = {int(s) for s in snapshots}
    for it in range(int(n_iter)):
        early = it < int(exaggeration_iter)
        want = bool(kl_every) and it > 0 and it % int(kl_every) == 0
        if it in snapshots:
            trajectory[it] = backend.map()
        kl = backend.gradient(float(early_exaggeration) if early else 1.0, want)
        if want:
            history.append((it, kl))
        backend.update(lr, 0.5 if early else 0.8)
    if int(n_iter) in snapshots:
        trajectory[int(n_iter)] = backend.map()
    kl = backend.gradient(1.0, True)
    history.append((int(n_iter), kl))
    return kl, history, trajectory


def _finish(N, nonzero, Y, beta, kl, history, trajectory, n_iter) -> ProjectionResult:
    xy = np.full((N, 2), np.nan, np.float32)
    y = np.asarray(Y, np.float64)
    xy[nonzero] = (y - y.mean(axis=0)).astype(np.float32)
    b = np.full(N, np.nan)
    b[nonzero] = beta
    return ProjectionResult(xy, float(kl), history, b, int(n_iter), trajectory)


class _NumpyBackend:
    def __init__(self, csr, Y0):
        self.csr = csr
        self.Y = np.array(Y0, np.float32)
        self.u, self.gains = np.zeros_like(self.Y), np.ones_like(self.Y)
        self.grad = None

    def map(self):
        return self.Y.copy()

    def gradient(self, E, want_kl):
        g = gradient_reference(self.Y, *self.csr, exaggeration=E)
        self.grad = g.grad.astype(np.float32)
        return g.kl if want_kl else None

    def update(self, lr, momentum):
        self.Y, self.u, self.gains = update_reference(self.Y, self.grad, self.u, self.gains, lr, momentum)


def _rows_and_nonzero(rows, zero_point):
    rows = np.asarray(rows)
    if rows.ndim != 2:
        raise ValueError(f"rows must be [N, D], got {rows.shape}")
    if rows.dtype != np.int8:
        rows = rows.astype(np.float32)
        if not np.isfinite(rows).all():
            raise ValueError("the rows hold values that are not finite")
    return rows, np.flatnonzero(inv_norms_reference(rows, zero_point) != 0)


def neighbours_reference(rows, k: int, zero_point: int = 0):
    """``(idx [n, k], score [n, k])``: every row's ``k`` best cosine scores among the other rows."""
    groups = np.arange(rows.shape[0])
    return search_reference(rows, rows, k, "cosine", zero_point=zero_point, db_group=groups, query_group=groups)


def tsne_reference(rows, perplexity: float = 30, n_iter: int = 1000, early_exaggeration: float = 12, exaggeration_iter: int = 250, learning_rate=None,
                   seed: int = 42, kl_every: int = 0, zero_point: int = 0, snapshots=(), init: str = "random") -> ProjectionResult:
    """The fit of the module docstring in numpy, float64 gradient over dense pairs: for small N."""
    check_init(init)
    rows, nonzero = _rows_and_nonzero(rows, zero_point)
    n = int(nonzero.size)
    check_project_args(n, perplexity, n_iter, early_exaggeration, exaggeration_iter, learning_rate, kl_every)
    live = np.ascontiguousarray(rows[nonzero])
    if init == "pca":
        from birdnet_stm32.evaluation.reduce import pca_reference, transform_reference

        model = _pca_model_for_start(lambda r: pca_reference(live, zero_point, 1.0, r)[0], n)
        Y0 = initial_map_pca(transform_reference(live, model))
    else:
        Y0 = initial_map(n, seed)
    idx, score = neighbours_reference(live, neighbour_count(n, perplexity), zero_point)
    p_cond, beta = conditional_p_reference(score, perplexity)
    csr = symmetrize(idx, p_cond.astype(np.float32), n)
    lr = default_learning_rate(n, early_exaggeration) if learning_rate is None else float(learning_rate)
    b = _NumpyBackend(csr, Y0)
    kl, history, trajectory = _descend(b, n, n_iter, early_exaggeration, exaggeration_iter, lr, kl_every, snapshots)
    return _finish(rows.shape[0], nonzero, b.Y, beta, kl, history, trajectory, n_iter)


# ---------------------------------------------------------------------------------------------------------------------- device
class _DeviceBackend:
    """Map, gradient, update and gains stay on the device; the host reads n float64 values where the divergence is asked for."""

    def __init__(self, ctx, csr, Y0):
        import ctypes

        import torch

        from birdnet_stm32 import _hip

        self.torch, self.hip, self.ctx = torch, _hip, ctx
        self.dev = torch.device("cuda", ctx.device)
        self.n = int(Y0.shape[0])
        rowptr, col, val = csr
        with torch.cuda.device(self.dev):
            self.sp = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
            self.d_rowptr = torch.from_numpy(np.ascontiguousarray(rowptr, np.int64)).to(self.dev)
            self.d_col = torch.from_numpy(np.ascontiguousarray(col, np.int32)).to(self.dev)
            self.d_val = torch.from_numpy(np.ascontiguousarray(val, np.float32)).to(self.dev)
            if self.d_col.numel() == 0:   # (an empty tensor has no address; the kernels read no entry)
                self.d_col, self.d_val = torch.zeros(1, dtype=torch.int32, device=self.dev), torch.zeros(1, dtype=torch.float32, device=self.dev)
            self.d_y = torch.from_numpy(np.ascontiguousarray(Y0, np.float32)).to(self.dev)
            self.d_grad = torch.zeros_like(self.d_y)
            self.d_update = torch.zeros_like(self.d_y)
            self.d_gains = torch.ones_like(self.d_y)
            self.d_z = torch.zeros(1, dtype=torch.float64, device=self.dev)
            self.d_kl = torch.zeros(self.n, dtype=torch.float64, device=self.dev)
        self.p_sum = float(np.asarray(val, np.float64).sum())

    def map(self):
        return self.d_y.cpu().numpy()

    def gradient(self, E, want_kl):
        with self.torch.cuda.device(self.dev):
            self.hip.check(self.ctx.lib.bn_tsne_gradient(self.ctx.handle, self.d_y.data_ptr(), self.n, self.d_rowptr.data_ptr(), self.d_col.data_ptr(),
                                                         self.d_val.data_ptr(), self.hip.c_float(E), self.d_grad.data_ptr(), self.d_z.data_ptr(),
                                                         self.d_kl.data_ptr() if want_kl else None, self.sp))
            if not want_kl:
                return None
            return kl_from_rows(self.d_kl.cpu().numpy(), self.p_sum, float(self.d_z.item()))

    def update(self, lr, momentum):
        with self.torch.cuda.device(self.dev):
            self.hip.check(self.ctx.lib.bn_tsne_update(self.ctx.handle, self.d_y.data_ptr(), self.d_grad.data_ptr(), self.d_update.data_ptr(),
                                                       self.d_gains.data_ptr(), self.n, self.hip.c_float(lr), self.hip.c_float(momentum), self.sp))


def device_bytes_needed(n: int, D: int, itemsize: int, k: int) -> int:
    """What a fit keeps on the device at its largest: rows and their scores, then the matrix P and the gradient's workspace."""
    from birdnet_stm32 import _hip

    search = n * D * itemsize + n * 12 + 2 * n * k * 4 + n * k * 4 + n * 8 + (128 << 20)
    splits = -(-n // _hip.TSNE_SPLIT_J)
    fit = 2 * n * k * 8 + (n + 1) * 8 + splits * n * 16 + n * 12 + 5 * n * 8 + n * 8
    return max(search, fit)


def device_neighbours(ctx, rows: np.ndarray, zero_point: int, k: int):
    """``(idx [n, k] int32, score [n, k] float32)``, tensors on ``ctx``'s device, of the non-zero rows ``rows``: ``bn_search_topk`` of the rows
    against themselves, every row its own group."""
    import ctypes

    import torch

    from birdnet_stm32 import _hip

    n, D = rows.shape
    dev = torch.device("cuda", ctx.device)
    code = _hip.DTYPE_I8 if rows.dtype == np.int8 else _hip.DTYPE_F32
    lib, h = ctx.lib, ctx.handle
    with torch.cuda.device(dev):
        sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        d_rows = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
        d_inv = torch.empty(n, dtype=torch.float32, device=dev)
        d_grp = torch.arange(n, dtype=torch.int32, device=dev)
        d_idx = torch.empty((n, k), dtype=torch.int32, device=dev)
        d_score = torch.empty((n, k), dtype=torch.float32, device=dev)
        _hip.check(lib.bn_search_inv_norms(h, d_rows.data_ptr(), code, n, D, zero_point, d_inv.data_ptr(), sp))
        _hip.check(lib.bn_search_topk(h, d_rows.data_ptr(), code, n, D, zero_point, d_inv.data_ptr(), d_rows.data_ptr(), n, d_inv.data_ptr(),
                                      _hip.SEARCH_METRICS["cosine"], d_grp.data_ptr(), d_grp.data_ptr(), k, d_idx.data_ptr(), d_score.data_ptr(), sp))
    return d_idx, d_score


def device_affinities(ctx, rows: np.ndarray, zero_point: int, k: int, perplexity: float):
    """``(idx [n, k] int64, p_cond [n, k] float32, beta [n] float64)`` of the non-zero rows ``rows``: their neighbours
    (``device_neighbours``), then ``bn_tsne_perplexity``."""
    import ctypes

    import torch

    from birdnet_stm32 import _hip

    n = rows.shape[0]
    d_idx, d_score = device_neighbours(ctx, rows, zero_point, k)
    dev = d_idx.device
    with torch.cuda.device(dev):
        sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        d_p = torch.empty((n, k), dtype=torch.float32, device=dev)
        d_beta = torch.empty(n, dtype=torch.float64, device=dev)
        _hip.check(ctx.lib.bn_tsne_perplexity(ctx.handle, d_score.data_ptr(), n, k, ctypes.c_double(perplexity), d_p.data_ptr(), d_beta.data_ptr(), sp))
        return d_idx.cpu().numpy().astype(np.int64), d_p.cpu().numpy(), d_beta.cpu().numpy()


def device_pca_scores(index, nonzero, ctx) -> np.ndarray:
    """The first two unwhitened principal-component scores ``[n, 2]`` of the non-zero rows, fitted and projected on the device."""
    from birdnet_stm32.evaluation.reduce import fit_pca, transform_index

    model = _pca_model_for_start(lambda r: fit_pca(index, r, ctx=ctx), int(nonzero.size))
    return transform_index(index, model, ctx=ctx)[nonzero]


def device_initial_map_pca(index, nonzero, ctx) -> np.ndarray:
    return initial_map_pca(device_pca_scores(index, nonzero, ctx))


def project_index(index, perplexity: float = 30, n_iter: int = 1000, early_exaggeration: float = 12, exaggeration_iter: int = 250, learning_rate=None,
                  seed: int = 42, kl_every: int = 0, device: int = 0, ctx=None, init: str = "random", snapshots=()) -> ProjectionResult:
    """The t-SNE map of the rows of an ``EmbeddingIndex`` on the device.  The non-zero rows go to the device in one piece, whatever the
    index's block budget: an archive that does not fit is refused.  ``snapshots`` asks for the uncentred maps after those iterations
    (``ProjectionResult.trajectory``; 0 is the start)."""
    import torch

    check_init(init)
    rows, zp = index.embeddings, index.zero_point
    nonzero = np.flatnonzero(inv_norms_reference(rows, zp) != 0)
    n = int(nonzero.size)
    check_project_args(n, perplexity, n_iter, early_exaggeration, exaggeration_iter, learning_rate, kl_every)
    if n > MAX_N:
        raise ValueError(f"{n} non-zero rows: a map holds at most {MAX_N}")
    k = neighbour_count(n, perplexity)
    ctx = index.context(ctx, device)
    need = device_bytes_needed(n, index.dim, rows.dtype.itemsize, k)
    free, _ = torch.cuda.mem_get_info(ctx.device)
    if need > free:
        raise ValueError(f"the archive does not fit on the device in one piece: {n} rows x {index.dim} need about {need >> 20} MiB, "
                         f"{free >> 20} MiB are free (archives larger than device memory are out of scope)")
    live = rows if n == len(index) else np.ascontiguousarray(rows[nonzero])
    idx, p_cond, beta = device_affinities(ctx, live, zp, k, float(perplexity))
    csr = symmetrize(idx, p_cond, n)
    lr = default_learning_rate(n, early_exaggeration) if learning_rate is None else float(learning_rate)
    b = _DeviceBackend(ctx, csr, device_initial_map_pca(index, nonzero, ctx) if init == "pca" else initial_map(n, seed))
    kl, history, trajectory = _descend(b, n, n_iter, early_exaggeration, exaggeration_iter, lr, kl_every, snapshots)
    return _finish(len(index), nonzero, b.map(), beta, kl, history, trajectory, n_iter)
