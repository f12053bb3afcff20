"""Shared builders of the select tests (test_select_host.py, test_gpu_select.py): inputs on which the specification has one value
whatever the summation order, the clusters of the bounded test with its restated score bound, and a synthetic archive for the CLI."""

import numpy as np

U = 2.0 ** -24   # unit roundoff of float32


def lattice_rows(N, D, seed, int8_zp=None):
    """Rows on the lattice {0..15}/16 (every product and partial sum of a dot is exact in float32 for D <= 256), or int8 bytes over the
    full range; with duplicated rows (ties) and, from 15 rows on, two zero rows."""
    rng = np.random.default_rng(seed)
    if int8_zp is None:
        X = (rng.integers(0, 16, (N, D)) / 16.0).astype(np.float32)
        X[X.sum(axis=1) == 0, 0] = 0.5
        zero = 0.0
    else:
        X = rng.integers(-128, 128, (N, D)).astype(np.int8)
        X[(X == int8_zp).all(axis=1), 0] = int8_zp + (1 if int8_zp < 127 else -1)
        zero = int8_zp
    if N >= 8:
        src = rng.integers(0, N, max(1, N // 8))
        X[rng.integers(0, N, src.size)] = X[src]   # duplicated rows tie
    if N >= 15:
        X[[N // 2, N - 2]] = zero
    return X


def unit_rows(N, D, seed):
    """Rows with exactly sixteen entries of +-1/4: inverse norm 1, every dot a multiple of 1/16."""
    rng = np.random.default_rng(seed)
    X = np.zeros((N, D), np.float32)
    for i in range(N):
        X[i, rng.choice(D, 16, replace=False)] = rng.choice([-1, 1], 16) * 0.25
    return X


def weights(N, seed, zeros=True):
    """float32 weights in [0, 1) with, on request, every seventh one 0."""
    w = np.random.default_rng(seed).random(N).astype(np.float32)
    if zeros:
        w[3::7] = 0
    return w


def normal_clusters(N, D, K, spread, seed):
    """``C[r.integers] + spread * normal`` of the bounded test."""
    r = np.random.default_rng(seed)
    C = r.standard_normal((K, D))
    lab = r.integers(0, K, N)
    return (C[lab] + spread * r.standard_normal((N, D))).astype(np.float32)


def score_bound(X, c):
    """``_score_bound`` of test_gpu_cluster.py (derived in test_gpu_search.py) restated for one centre, row ``c`` of ``X``: the float64
    scores S [N] of the float32 rows against it and a bound on the float32 device error of each,
    |d S| <= (D + 2) u sum |x_j c_j| inv_x inv_c + |S| (D + 8) u, and 1 % on top."""
    D = X.shape[1]
    X64 = X.astype(np.float64)
    y = X64[c]
    dot, adot = X64 @ y, np.abs(X64) @ np.abs(y)
    nx = np.sqrt((X64 * X64).sum(axis=1))
    ix = np.divide(1.0, nx, out=np.zeros_like(nx), where=nx > 0)
    S = dot * ix * ix[c]
    return S, 1.01 * ((D + 2) * U * adot * ix * ix[c] + np.abs(S) * (D + 8) * U)


def key_bound(u, m, Bm):
    """The float64 keys ``u (1 - m)`` and a bound on the device's float32 ``fl(u fl(1 - m'))`` with ``|m' - m| <= Bm``: the error of m,
    the rounding of m to float32 and of the difference (2 U |1 - m| to first order, m' being within Bm of m), and the product's rounding:
    ``u (Bm + 2 U |1 - m|) + U |key|``."""
    key = u * (1.0 - m)
    return key, u * (Bm + 2 * U * np.abs(1.0 - m)) + U * np.abs(key)


def forced_trajectory(X, u, steps, start=0):
    """The float64 traversal of the rows ``X`` (weights ``u`` float64) from the taken row ``start``: per step the float32 state handed to
    the device (``m32``, ``nearest``), the float64 state and its bound (``m64``, ``Bm``), the reference's pick, the rows that may win
    under the key bound and whether the reference alone leaves one (a clean step)."""
    N = X.shape[0]
    live = np.abs(X).sum(axis=1) > 0
    m = np.full(N, -np.inf)
    Bm = np.zeros(N)
    nearest = np.full(N, -1, np.int32)

    def take(c):
        S, B = score_bound(X, c)
        better = live & (m != np.inf) & (S > m)
        better[c] = False
        m[better], Bm[better], nearest[better] = S[better], B[better], c
        m[c], Bm[c], nearest[c] = np.inf, 0.0, c

    take(start)
    out = []
    for _ in range(steps):
        open_ = live & (m != np.inf)
        key, Bk = key_bound(u, np.where(open_, m, 0.0), Bm)
        key, Bk = np.where(open_, key, -np.inf), np.where(open_, Bk, 0.0)
        best = int(np.argmax(key))
        may = np.flatnonzero(open_ & (key + Bk >= key[best] - Bk[best]))
        out.append(dict(m32=np.where(m == np.inf, np.inf, m).astype(np.float32), nearest=nearest.copy(), m64=m.copy(), Bm=Bm.copy(), pick=best,
                        may=may, clean=may.size == 1))
        take(best)
    return out


def synthetic_archive(path, X, files=4, **extra):
    """An archive as ``embed`` writes it: the rows of ``X`` dealt to ``files`` recordings, three seconds apart."""
    N = X.shape[0]
    file_index = (np.arange(N) * files // N).astype(np.int64)
    start_s = np.zeros(N)
    for f in range(files):
        rows = np.flatnonzero(file_index == f)
        start_s[rows] = 3.0 * np.arange(rows.size)
    paths = np.asarray([f"rec/file_{f}.wav" for f in range(files)])
    with open(path, "wb") as fh:
        np.savez(fh, embeddings=X, file_index=file_index, start_s=start_s, paths=paths, **extra)
    return file_index, start_s, [str(p) for p in paths]
