"""Inputs the CPU and GPU tests of ``project`` share: three well-separated clusters and the reference's fit on them (computed once per process)."""

import functools

import numpy as np

CLUSTERS, PER_CLUSTER, DIM, ITERATIONS = 3, 100, 32, 500
SNAPSHOTS = (100, 250, 500)


def three_clusters(seed: int = 0, spread: float = 0.05) -> np.ndarray:
    """3 x 100 rows, D = 32: three normal centres, every row its centre plus ``spread`` times normal noise (the centres are about
    sqrt(2 * 32) apart, the noise about 0.05 * sqrt(32) long: the reference alone puts every row next to one of its own cluster)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((CLUSTERS, DIM))
    return np.concatenate([centres[c] + spread * rng.standard_normal((PER_CLUSTER, DIM)) for c in range(CLUSTERS)]).astype(np.float32)


def cluster_of_rows() -> np.ndarray:
    return np.arange(CLUSTERS * PER_CLUSTER) // PER_CLUSTER


@functools.lru_cache(maxsize=1)
def reference_fit():
    """``tsne_reference`` on ``three_clusters()``: 500 iterations, the divergence at 250 and 500, the maps after 100, 250 and 500 updates."""
    from birdnet_stm32.evaluation.project import tsne_reference

    return tsne_reference(three_clusters(), n_iter=ITERATIONS, kl_every=250, snapshots=SNAPSHOTS)


def same_cluster_share(xy: np.ndarray, cluster: np.ndarray) -> float:
    """Share of the points whose nearest neighbour in the map comes from their own cluster."""
    y = np.asarray(xy, np.float64)
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    return float((cluster[d.argmin(axis=1)] == cluster).mean())
