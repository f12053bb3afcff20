"""Inputs the CPU and GPU tests of ``reduce`` share: rectified rows with a planted spectrum, lattice rows, int8 bytes, three separated
clusters and a writer of ``embed``-style archives."""

import functools

import numpy as np

PLANTED_STD = (8.0, 6.0, 4.5, 3.2, 2.2, 1.5, 1.0, 0.7)   # the leading components; the others have 0.05
PLANTED_REST = 0.05


@functools.lru_cache(maxsize=8)
def _planted(n: int, D: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    std = np.full(D, PLANTED_REST)
    k = min(D, len(PLANTED_STD))
    std[:k] = PLANTED_STD[:k]
    q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    z = (rng.standard_normal((n, D)) * std) @ q.T
    # offsets in 1..5: the mean is many standard deviations of the small components away from 0, as pooled ReLU6 features have it
    return np.maximum(z + rng.uniform(1.0, 5.0, D), 0.0).astype(np.float32)


def planted_rows(n: int = 1000, D: int = 40, seed: int = 3) -> np.ndarray:
    """``[n, D]`` float32, non-negative: normal rows with standard deviations ``PLANTED_STD`` then ``PLANTED_REST`` along a random
    orthonormal basis, shifted by a positive offset per feature and rectified."""
    return _planted(n, D, seed).copy()


def real_rows(n: int, D: int, seed: int) -> np.ndarray:
    """Real-valued float32 rows of mixed sign and a mean away from 0."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, D)) * rng.uniform(0.1, 3.0, D) + rng.uniform(-2.0, 4.0, D)).astype(np.float32)


def lattice_rows(n: int, D: int, seed: int, mean: int = 0) -> np.ndarray:
    """Small integers around an integer mean as float32: every sum and product of the kernels is exact on them."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-8, 9, (n, D)) + mean).astype(np.float32)


def int8_rows(n: int, D: int, seed: int) -> np.ndarray:
    """Bytes over the whole range, mixed signs."""
    return np.random.default_rng(seed).integers(-128, 128, (n, D)).astype(np.int8)


def int8_features(n: int, D: int, seed: int, scale: float, zero_point: int) -> np.ndarray:
    """The bytes of rectified planted rows under ``(scale, zero_point)``."""
    x = planted_rows(n, D, seed)
    return np.clip(np.rint(x / scale) + zero_point, -128, 127).astype(np.int8)


def three_clusters(per: int = 40, D: int = 24, seed: int = 0, spread: float = 0.05):
    """``(rows [3 * per, D] float32, cluster [3 * per])``: three normal centres shifted to be positive, every row its centre plus
    ``spread`` times normal noise."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((3, D)) + 3.0
    rows = np.concatenate([centres[c] + spread * rng.standard_normal((per, D)) for c in range(3)]).astype(np.float32)
    return rows, np.arange(3 * per) // per


def write_archive(path: str, rows: np.ndarray, scale=None, zero_point=None, files: int = 4) -> None:
    """An archive as ``embed`` writes it: rows dealt to ``files`` files in order."""
    n = rows.shape[0]
    per = -(-n // files)
    arrays = dict(embeddings=rows, file_index=np.arange(n) // per, start_s=3.0 * (np.arange(n) % per), paths=np.asarray([f"clip{j}.wav" for j in range(files)]))
    if rows.dtype == np.int8:
        arrays.update(scale=np.float32(scale), zero_point=np.int32(zero_point))
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def same_cluster_share(points: np.ndarray, cluster: np.ndarray, cosine: bool = False) -> float:
    """Share of the rows whose nearest other row (Euclidean, or by cosine) comes from their own cluster."""
    y = np.asarray(points, np.float64)
    if cosine:
        y = y / np.linalg.norm(y, axis=1, keepdims=True)
        d = -(y @ y.T)
    else:
        d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    return float((cluster[d.argmin(axis=1)] == cluster).mean())


def fit_bounds(rows: np.ndarray, n_test: int = 8):
    """For the float32 fit on ``rows``: ``(reference model, sine bounds [n_test], variance bounds [n_test])``.  With ``B`` the matrix of
    entry bounds of the device's scatter matrix (``gram_entry_bound``), Davis-Kahan gives ``sin(angle_k) <= 2 ||B||_F / gap_k`` with
    ``gap_k`` the distance of ``lambda_k`` to its nearest other eigenvalue, and Weyl ``|dlambda_k| <= ||B||_2``."""
    from birdnet_stm32.evaluation import reduce as R

    model, _ = R.pca_reference(rows, n_components=n_test)
    c = R.centred(rows, model.mean32)
    B = R.gram_entry_bound(c)
    lam, _ = R.spectrum(c.astype(np.float64).T @ c.astype(np.float64))
    gaps = np.array([min(abs(lam[k] - lam[j]) for j in range(lam.size) if j != k) for k in range(n_test)])
    return model, 2.0 * np.linalg.norm(B, "fro") / gaps, np.linalg.norm(B, 2) / lam[:n_test]
