"""Reduction: principal components of the rows of archives written by ``embed`` — centred, rotated, shortened and optionally whitened rows.

``pca_reference`` is the specification in numpy; ``fit_pca`` / ``transform_index`` run the sums over rows on the device (``csrc/bn_pca.hip``,
C ABI ``bn_pca_colsum`` / ``bn_pca_gram`` / ``bn_pca_transform``).  Both share every host-side step from the scatter matrix on
(``model_from_scatter``), so the two paths differ only where the kernels do.  The result matches scikit-learn 1.7's
``PCA(svd_solver="full")`` up to the float32 centring (checked in tests/test_reduce_host.py).

1. Rows.  ``[N, D]``; float32 rows are used as they are, an int8 row is ``x = byte - zero_point`` as integers.  Zero rows (the rows whose
   ``inv_norms_reference`` is 0) take no part in the fit and their transformed row is all zeros, so every downstream tool still sees them
   as zero rows.  ``n`` is the number of the others, the live rows; fewer than 2 is a ``ValueError``.
2. Mean.  ``mu = sum(x) / n`` in float64, ``mu32 = float32(mu)``.
3. Scatter matrix.  float32: ``c_i = fl32(x_i - mu32)``, one rounding per element, and ``G = sum_i c_i c_i^T``.  int8:
   ``G_raw = sum_i x_i x_i^T`` and ``s = sum_i x_i`` as exact integers, then ``G = G_raw - outer(s, s) / n`` in float64.  float32 is centred
   BEFORE the products, not after: the mean of pooled ReLU6 features is several standard deviations, and an uncentred float32 Gram matrix
   loses the small eigenvalues to the cancellation in ``G_raw - outer(s, s) / n``.  (The int8 sums are exact integers, so there the
   subtraction only costs float64 roundings.)  The device forms the float32 products in the matrix cores: they accumulate in float32 for
   runs of ``BN_PCA_RUN_ROWS`` rows and the runs are added in float64, so per entry
   ``|G_device - G| <= (BN_PCA_RUN_ROWS + 1) 2^-24 sum_i |c_ia c_ib|`` whatever ``n`` (``gram_entry_bound``).
4. Spectrum.  ``numpy.linalg.eigh(G)`` in float64, eigenvalues descending with a stable order among equal values (negative ones, which
   are rounding noise, count as 0).  Sign: the entry of largest magnitude of each component is positive, the first such entry on a tie
   (scikit-learn 1.7's ``svd_flip(u_based_decision=False)``).  ``explained_variance = lambda / (n - 1)``, times ``scale^2`` for int8 (real
   units); ``total_variance`` is the sum over all ``D`` eigenvalues and ``explained_variance_ratio = explained_variance / total_variance``.
5. ``n_components``.  An int in ``1 .. min(D, n - 1)``; or a float in ``(0, 1)``: the smallest ``r`` whose cumulative ratio exceeds it
   (scikit-learn's ``searchsorted(cumsum, v, side="right") + 1``), at most ``min(D, n - 1)``.
6. Weights.  ``W = components`` for float32, ``W = components * scale`` for int8; with ``whiten`` each row of ``W`` is divided by
   ``sqrt(explained_variance_k)``.  ``W`` is formed in float64 from the unrounded eigenvectors and rounded to float32 once (the model keeps
   it as ``weights``).  Whitening a component whose variance is not above ``2^-40`` of the first is refused; the message names the component.
7. Transform.  ``y_i = W c_i`` with ``c_i = fl32(x_i - mu32)`` for both dtypes (the int8 ``x`` is first made float32, which is exact).  The
   specification computes it in float64 and rounds once to float32; the device's fused float32 chain over ``d`` stays within
   ``(D + 2) 2^-24 sum_d |W_kd c_id|`` of the float64 value (``transform_bound``).
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from birdnet_stm32.evaluation.search import MAX_D, inv_norms_reference

RUN_ROWS = 256   # BN_PCA_RUN_ROWS (include/birdnet_hip.h)
WHITEN_FLOOR = 2.0 ** -40
DEFAULT_COMPONENTS = 32
MODEL_KEYS = ("mean", "components", "weights", "explained_variance", "total_variance", "n_rows", "whiten", "dtype", "scale", "zero_point")


@dataclass
class PcaModel:
    """``mean`` [D] float64 (of ``x``: integer units for int8), ``components`` [r, D] float32 (unit rows), ``weights`` [r, D] float32 (item 6),
    ``explained_variance`` [r] float64, ``total_variance``, ``n_rows`` (live rows of the fit), ``whiten`` and the source's ``dtype``,
    ``scale`` and ``zero_point``."""

    mean: np.ndarray
    components: np.ndarray
    weights: np.ndarray
    explained_variance: np.ndarray
    total_variance: float
    n_rows: int
    whiten: bool
    dtype: str
    scale: float
    zero_point: int

    @property
    def dim(self) -> int:
        return int(self.components.shape[1])

    @property
    def n_components(self) -> int:
        return int(self.components.shape[0])

    @property
    def explained_variance_ratio(self) -> np.ndarray:
        return self.explained_variance / self.total_variance

    @property
    def mean32(self) -> np.ndarray:
        return self.mean.astype(np.float32)

    def check(self) -> None:
        """Raise ``ValueError`` unless the fields fit together."""
        if self.dtype not in ("float32", "int8"):
            raise ValueError(f"model dtype {self.dtype!r}: 'float32' or 'int8' expected")
        c, w, m, ev = self.components, self.weights, self.mean, self.explained_variance
        if c.ndim != 2 or c.dtype != np.float32 or not 1 <= c.shape[0] <= c.shape[1] or not 1 <= c.shape[1] <= MAX_D:
            raise ValueError(f"components must be float32 [r, D] with 1 <= r <= D <= {MAX_D}, got {c.dtype} {c.shape}")
        if w.shape != c.shape or w.dtype != np.float32:
            raise ValueError(f"weights {w.dtype} {w.shape} do not match components {c.shape}")
        if m.shape != (c.shape[1],) or m.dtype != np.float64:
            raise ValueError(f"mean must be float64 [{c.shape[1]}], got {m.dtype} {m.shape}")
        if ev.shape != (c.shape[0],) or ev.dtype != np.float64:
            raise ValueError(f"explained_variance must be float64 [{c.shape[0]}], got {ev.dtype} {ev.shape}")
        if not (np.isfinite(c).all() and np.isfinite(w).all() and np.isfinite(m).all() and np.isfinite(ev).all()):
            raise ValueError("the model holds values that are not finite")
        if (ev < 0).any() or (np.diff(ev) > 0).any():
            raise ValueError("explained_variance must be non-negative and descending")
        if not (math.isfinite(self.total_variance) and self.total_variance >= float(ev.sum()) * (1 - 1e-9) and self.total_variance > 0):
            raise ValueError(f"total_variance {self.total_variance} below the components' own {float(ev.sum())}")
        if self.n_rows < 2 or c.shape[0] > self.n_rows - 1:
            raise ValueError(f"{c.shape[0]} components from {self.n_rows} rows")
        if not (math.isfinite(self.scale) and self.scale > 0) or not -128 <= self.zero_point <= 127:
            raise ValueError(f"scale {self.scale} / zero point {self.zero_point} out of range")
        if self.dtype == "float32" and (self.scale != 1.0 or self.zero_point != 0):
            raise ValueError("a float32 model has scale 1 and zero point 0")

    def save(self, path: str) -> None:
        self.check()
        with open(path, "wb") as f:   # (np.savez would append .npz to a name without it)
            np.savez(f, **self.fields())

    def fields(self, prefix: str = "") -> dict:
        """The model as arrays without pickled objects, keys ``prefix + name``."""
        d = dict(mean=self.mean, components=self.components, weights=self.weights, explained_variance=self.explained_variance,
                 total_variance=np.float64(self.total_variance), n_rows=np.int64(self.n_rows), whiten=np.bool_(self.whiten), dtype=np.asarray(self.dtype),
                 scale=np.float64(self.scale), zero_point=np.int64(self.zero_point))
        return {prefix + k: v for k, v in d.items()}

    @classmethod
    def load(cls, path: str) -> "PcaModel":
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in MODEL_KEYS if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a model written by `reduce` (no {', '.join(missing)})")
            try:
                m = cls(z["mean"], z["components"], z["weights"], z["explained_variance"], float(z["total_variance"]), int(z["n_rows"]), bool(z["whiten"]),
                        str(z["dtype"]), float(z["scale"]), int(z["zero_point"]))
                m.check()
            except (ValueError, TypeError) as exc:
                raise ValueError(f"{path}: {exc}") from None
        return m


# ------------------------------------------------------------------------------------------------------------------ host steps
def live_rows(rows, zero_point: int = 0):
    """``(rows, live)``: the rows as float32 or int8 ``[N, D]`` and the indices of the rows that are not zero rows."""
    rows = np.asarray(rows)
    if rows.ndim != 2:
        raise ValueError(f"rows must be [N, D], got {rows.shape}")
    if rows.dtype != np.int8:
        rows = rows.astype(np.float32)
        if not np.isfinite(rows).all():
            raise ValueError("the rows hold values that are not finite")
    return rows, np.flatnonzero(inv_norms_reference(rows, zero_point) != 0)


def check_live(n: int) -> None:
    if n < 2:
        raise ValueError(f"a fit needs at least 2 non-zero rows, the archive holds {n}")


def centred(rows, mean32, zero_point: int = 0) -> np.ndarray:
    """``c = fl32(x - mu32)`` of items 3 and 7, float32."""
    rows = np.asarray(rows)
    x = (rows.astype(np.int32) - int(zero_point)).astype(np.float32) if rows.dtype == np.int8 else rows.astype(np.float32)
    return x - np.asarray(mean32, np.float32)[None, :]


def scatter_from_raw(G_raw, s, n: int) -> np.ndarray:
    """``G_raw - outer(s, s) / n`` in float64 (int8, item 3); the arguments hold exact integers."""
    s = np.asarray(s, np.float64)
    return np.asarray(G_raw, np.float64) - np.outer(s, s) / float(n)


def scatter_reference(live, zero_point: int = 0):
    """``(mean [D] float64, G [D, D] float64)`` of items 2 and 3 over the live rows."""
    n = live.shape[0]
    if live.dtype == np.int8:
        x = live.astype(np.int64) - int(zero_point)
        s = x.sum(axis=0)
        return s.astype(np.float64) / n, scatter_from_raw(x.T @ x, s, n)
    mean = live.astype(np.float64).sum(axis=0) / n
    c = centred(live, mean.astype(np.float32)).astype(np.float64)
    return mean, c.T @ c


def flip_signs(V) -> np.ndarray:
    """Every row of ``V`` with its entry of largest magnitude positive, the first such entry on a tie (item 4)."""
    V = np.asarray(V, np.float64)
    big = np.argmax(np.abs(V), axis=1)   # (the first of equal magnitudes)
    sign = np.sign(V[np.arange(V.shape[0]), big])
    sign[sign == 0] = 1.0
    return V * sign[:, None]


def spectrum(G):
    """``(lambda [D] descending, clipped at 0; V [D, D] float64, rows = components with item 4's sign)``."""
    G = np.asarray(G, np.float64)
    w, v = np.linalg.eigh(G)
    order = np.argsort(-w, kind="stable")
    return np.maximum(w[order], 0.0), flip_signs(v[:, order].T)


def resolve_components(n_components, ratio, D: int, n: int) -> int:
    """Item 5."""
    limit = min(int(D), int(n) - 1)
    if isinstance(n_components, (bool, np.bool_)):
        raise ValueError(f"n_components {n_components!r}: an int >= 1 or a float in (0, 1) expected")
    if isinstance(n_components, (int, np.integer)):
        if not 1 <= int(n_components) <= limit:
            raise ValueError(f"n_components {int(n_components)} outside 1..{limit} (min(D, live rows - 1))")
        return int(n_components)
    v = float(n_components)
    if not 0.0 < v < 1.0:
        raise ValueError(f"n_components {n_components!r}: an int >= 1 or a float in (0, 1) expected")
    return min(int(np.searchsorted(np.cumsum(ratio), v, side="right")) + 1, limit)


def model_from_scatter(G, mean, n: int, dtype: str, scale: float = 1.0, zero_point: int = 0, n_components=DEFAULT_COMPONENTS, whiten: bool = False) -> PcaModel:
    """Items 4 to 6: what both the specification and the device fit do once they hold the scatter matrix."""
    check_live(n)
    scale = float(scale) if dtype == "int8" else 1.0
    lam, V = spectrum(G)
    D = V.shape[1]
    var = lam / (n - 1) * scale * scale
    total = float(var.sum())
    if not total > 0.0:
        raise ValueError("the rows are all equal: there is no variance to explain")
    r = resolve_components(n_components, var / total, D, n)
    W = V[:r] * scale
    if whiten:
        low = np.flatnonzero(~(var[:r] > WHITEN_FLOOR * var[0]))
        if low.size:
            raise ValueError(f"component {int(low[0])} has variance {var[low[0]]:.3g}, not above 2^-40 of the first ({var[0]:.3g}): it cannot be whitened; "
                             f"ask for at most {int(low[0])} components")
        W = W / np.sqrt(var[:r])[:, None]
    model = PcaModel(np.asarray(mean, np.float64), V[:r].astype(np.float32), W.astype(np.float32), var[:r].copy(), total, int(n), bool(whiten), dtype, scale,
                     int(zero_point) if dtype == "int8" else 0)
    model.check()
    return model


def transform_reference(rows, model: PcaModel) -> np.ndarray:
    """Item 7 over all rows: float32 ``[N, r]``, zeros for a zero row."""
    rows, live = live_rows(rows, model.zero_point)
    out = np.zeros((rows.shape[0], model.n_components), np.float32)
    c = centred(rows[live], model.mean32, model.zero_point).astype(np.float64)
    out[live] = (c @ model.weights.astype(np.float64).T).astype(np.float32)
    return out


def pca_reference(rows, zero_point: int = 0, scale: float = 1.0, n_components=DEFAULT_COMPONENTS, whiten: bool = False):
    """``(PcaModel, scores [N, r] float32)``: the specification of the module docstring."""
    rows, live = live_rows(rows, zero_point)
    check_live(int(live.size))
    mean, G = scatter_reference(np.ascontiguousarray(rows[live]), zero_point)
    dtype = "int8" if rows.dtype == np.int8 else "float32"
    model = model_from_scatter(G, mean, int(live.size), dtype, scale, zero_point, n_components, whiten)
    return model, transform_reference(rows, model)


def gram_entry_bound(c) -> np.ndarray:
    """``(RUN_ROWS + 1) 2^-24 sum_i |c_ia c_ib|`` [D, D]: what a device scatter matrix may differ by from the float64 product of the same
    centred float32 rows ``c`` (item 3)."""
    a = np.abs(np.asarray(c, np.float64))
    return (RUN_ROWS + 1) * 2.0 ** -24 * (a.T @ a)


def transform_bound(c, weights) -> np.ndarray:
    """``(D + 2) 2^-24 sum_d |W_kd c_id|`` [n, r] (item 7): D roundings of the fused chain, one of the float32 store of the reference, one spare."""
    a, w = np.abs(np.asarray(c, np.float64)), np.abs(np.asarray(weights, np.float64))
    return (a.shape[1] + 2) * 2.0 ** -24 * (a @ w.T)


def check_model_applies(model: PcaModel, index) -> None:
    """Refuse an index the model was not fitted for: another width or dtype, for int8 another scale or zero point."""
    if index.dim != model.dim or index.dtype != model.dtype:
        raise ValueError(f"the model was fitted on {model.dim} x {model.dtype} rows, the archive holds {index.dim} x {index.dtype}")
    if model.dtype == "int8" and (np.float32(index.scale) != np.float32(model.scale) or int(index.zero_point) != model.zero_point):
        raise ValueError(f"the model's int8 scale / zero point ({model.scale}, {model.zero_point}) differ from the archive's "
                         f"({index.scale}, {index.zero_point}): the bytes are not comparable")


# ---------------------------------------------------------------------------------------------------------------------- device
def _live_blocks(index, live_mask):
    """The live rows of every block of ``index.block_ranges()``, compacted on the host; blocks without one are left out."""
    for lo, hi in index.block_ranges():
        m = live_mask[lo:hi]
        if m.all():
            block = index.embeddings[lo:hi]
        else:
            block = np.ascontiguousarray(index.embeddings[lo:hi][m])
        if block.shape[0]:
            yield block


def device_scatter(index, live_mask, ctx):
    """``(s [D] float64, mean32, G [D, D] float64)``: column sums, then the scatter matrix (float32: of the centred rows; int8: the exact
    ``G_raw``), block by block, the blocks' results added on the host in float64 in block order."""
    import ctypes

    import torch

    from birdnet_stm32 import _hip

    D, zp, code = index.dim, index.zero_point, index.dtype_code
    n = int(live_mask.sum())
    dev = torch.device("cuda", ctx.device)
    lib, h = ctx.lib, ctx.handle
    s, G = np.zeros(D), np.zeros((D, D))
    with torch.cuda.device(dev):
        sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        d_sum = torch.empty(D, dtype=torch.float64, device=dev)
        d_gram = torch.empty((D, D), dtype=torch.float64, device=dev)
        for block in _live_blocks(index, live_mask):
            d_rows = torch.from_numpy(block).to(dev)
            _hip.check(lib.bn_pca_colsum(h, d_rows.data_ptr(), code, block.shape[0], D, zp, d_sum.data_ptr(), sp))
            s += d_sum.cpu().numpy()
        mean32 = (s / n).astype(np.float32)
        d_mean = torch.from_numpy(mean32).to(dev) if index.dtype == "float32" else None
        for block in _live_blocks(index, live_mask):
            d_rows = torch.from_numpy(block).to(dev)
            _hip.check(lib.bn_pca_gram(h, d_rows.data_ptr(), code, block.shape[0], D, zp, d_mean.data_ptr() if d_mean is not None else None,
                                       d_gram.data_ptr(), sp))
            G += d_gram.cpu().numpy()
    return s, mean32, G


def fit_pca(index, n_components=DEFAULT_COMPONENTS, whiten: bool = False, ctx=None, device: int = 0) -> PcaModel:
    """The model of the live rows of an ``EmbeddingIndex``; the sums over rows run on the device, block by block."""
    live_mask = inv_norms_reference(index.embeddings, index.zero_point) != 0
    n = int(live_mask.sum())
    check_live(n)
    ctx = index.context(ctx, device)
    s, _, G = device_scatter(index, live_mask, ctx)
    if index.dtype == "int8":
        G = scatter_from_raw(G, s, n)
    return model_from_scatter(G, s / n, n, index.dtype, index.scale, index.zero_point, n_components, whiten)


def transform_index(index, model: PcaModel, ctx=None, device: int = 0) -> np.ndarray:
    """``[N, r]`` float32: every row of the index through the model on the device, zero rows as zeros."""
    import ctypes

    import torch

    from birdnet_stm32 import _hip

    check_model_applies(model, index)
    ctx = index.context(ctx, device)
    N, D, r = len(index), index.dim, model.n_components
    out = np.zeros((N, r), np.float32)
    dev = torch.device("cuda", ctx.device)
    with torch.cuda.device(dev):
        sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        d_mean = torch.from_numpy(model.mean32).to(dev)
        d_W = torch.from_numpy(np.ascontiguousarray(model.weights)).to(dev)
        for lo, hi in index.block_ranges():
            if hi == lo:
                continue
            d_rows = torch.from_numpy(index.embeddings[lo:hi]).to(dev)
            d_out = torch.empty((hi - lo, r), dtype=torch.float32, device=dev)
            _hip.check(ctx.lib.bn_pca_transform(ctx.handle, d_rows.data_ptr(), index.dtype_code, hi - lo, D, index.zero_point, d_mean.data_ptr(),
                                                d_W.data_ptr(), r, d_out.data_ptr(), sp))
            out[lo:hi] = d_out.cpu().numpy()
    out[inv_norms_reference(index.embeddings, index.zero_point) == 0] = 0.0
    return out


def reduce_index(index, model_or_n_components=DEFAULT_COMPONENTS, whiten: bool = False, ctx=None, device: int = 0):
    """``(EmbeddingIndex, PcaModel)``: the reduced index is float32 ``[N, r]`` and carries the source's ``file_index``, ``start_s`` and
    ``paths``.  A ``PcaModel`` is applied as it is; anything else is ``n_components`` of a fresh fit."""
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    if isinstance(model_or_n_components, PcaModel):
        model = model_or_n_components
        check_model_applies(model, index)
    else:
        model = fit_pca(index, model_or_n_components, whiten, ctx=ctx, device=device)
    scores = transform_index(index, model, ctx=ctx, device=device)
    return EmbeddingIndex(scores, index.file_index, index.start_s, index.paths, "float32", budget_bytes=index.budget_bytes), model
