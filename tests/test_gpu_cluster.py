"""GPU tests of clustering (csrc/bn_kmeans.hip, evaluation/cluster.py, cli/cluster.py) against the numpy specification.

Equality tests use inputs on which the specification has one value whatever the summation order: rows and centroids on the lattice
{0, 1/16, ..., 15/16} (every product and partial sum is exact in float32 for D <= 256), INT8 bytes against lattice centroids (products
are multiples of 1/16 below 2^16), and for the update unit rows of sixteen entries +-1/4 (inverse norm exactly 1, sums exact).
Real-valued rows are held to written-out error bounds along a teacher-forced trajectory: at every iteration the device gets the
reference's float32 centroids and, for the update, the reference's labels; labels must be equal on every row the float64 reference alone
separates by more than the two bounds (at least 99 % of the rows, computed before the device output is looked at)."""

import csv
import os
import wave

import numpy as np
import pytest

from conftest import CONFIG_PATH, KERAS_PATH, TFLITE_PATH

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # unit roundoff of float32
NAN_BITS = 0x7FC0BEEF


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a ROCm device; there is no CPU fallback to fall back to")
    return torch


@pytest.fixture(scope="module")
def ctx(torch_mod):
    from birdnet_stm32 import _hip

    c = _hip.Context(0, 1)
    yield c
    c.close()


def _inv_norms(torch, ctx, rows, zp=0, off=False):
    from birdnet_stm32 import _hip

    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    if off:   # the same rows in a flat buffer one element longer, from its element 1: +4 bytes for float32, +1 byte for int8
        flat = torch.empty(rows.size + 1, dtype=d.dtype, device="cuda")
        flat[1:] = d.view(-1)
        d = flat[1:].view(rows.shape)
        assert d.data_ptr() % 16 == rows.itemsize
    out = torch.empty(rows.shape[0], dtype=torch.float32, device="cuda")
    code = _hip.DTYPE_I8 if rows.dtype == np.int8 else _hip.DTYPE_F32
    _hip.check(ctx.lib.bn_search_inv_norms(ctx.handle, d.data_ptr(), code, rows.shape[0], rows.shape[1], zp, out.data_ptr(), None))
    return d, out


def _assign(torch, ctx, rows, C, zp=0, prev=None, off=False):
    """bn_kmeans_assign through the C ABI: (label int64, score float32, changed) on the host.  ``off``: the rows off the 16-byte boundary."""
    from birdnet_stm32 import _hip

    d_rows, d_inv = _inv_norms(torch, ctx, rows, zp, off)
    d_C, d_cinv = _inv_norms(torch, ctx, np.ascontiguousarray(C, np.float32))
    n, K = rows.shape[0], C.shape[0]
    label = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    score = torch.full((n,), 3.0, dtype=torch.float32, device="cuda")
    changed = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    d_prev = torch.from_numpy(np.asarray(prev, np.int32)).cuda() if prev is not None else None
    code = _hip.DTYPE_I8 if rows.dtype == np.int8 else _hip.DTYPE_F32
    _hip.check(ctx.lib.bn_kmeans_assign(ctx.handle, d_rows.data_ptr(), code, n, rows.shape[1], zp, d_inv.data_ptr(), d_C.data_ptr(), d_cinv.data_ptr(), K,
                                        d_prev.data_ptr() if d_prev is not None else None, label.data_ptr(), score.data_ptr(), changed.data_ptr(), None))
    torch.cuda.synchronize()
    assert np.array_equal(d_rows.cpu().numpy(), rows) and np.array_equal(d_C.cpu().numpy(), C), "an input changed"
    return label.cpu().numpy().astype(np.int64), score.cpu().numpy(), int(changed.item())


def _accumulate(torch, ctx, rows, labels, K, zp=0, halves=False):
    """bn_kmeans_accumulate between guard rows of a NaN pattern: (sums [K, D] float32, counts [K] int64)."""
    from birdnet_stm32 import _hip

    n, D = rows.shape
    d_rows, d_inv = _inv_norms(torch, ctx, rows, zp)
    d_lab = torch.from_numpy(np.asarray(labels, np.int32)).cuda()
    sums = torch.full((K + 2, D), NAN_BITS, dtype=torch.int32, device="cuda")
    counts = torch.full((K + 2,), -99, dtype=torch.int64, device="cuda")
    code = _hip.DTYPE_I8 if rows.dtype == np.int8 else _hip.DTYPE_F32
    cuts = [0, n // 2, n] if halves else [0, n]
    for j, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        _hip.check(ctx.lib.bn_kmeans_accumulate(ctx.handle, d_rows[lo:].data_ptr(), code, hi - lo, D, zp, d_inv[lo:].data_ptr(), d_lab[lo:].data_ptr(), K, int(j > 0),
                                                sums[1:].data_ptr(), counts[1:].data_ptr(), None))
    torch.cuda.synchronize()
    s, c = sums.cpu().numpy(), counts.cpu().numpy()
    assert (s[0] == NAN_BITS).all() and (s[K + 1] == NAN_BITS).all() and c[0] == -99 and c[K + 1] == -99, "a guard row was written"
    assert np.array_equal(d_rows.cpu().numpy(), rows) and np.array_equal(d_lab.cpu().numpy(), np.asarray(labels, np.int32)), "an input changed"
    return s[1:K + 1].view(np.float32), c[1:K + 1]


def _tile_crossing_k():
    """One centroid more than an LDS tile holds at D = 256, from the header's constants."""
    from birdnet_stm32 import _hip

    tile = _hip.kmeans_tile_centroids(256, _hip.KMEANS_MAX_K)
    assert tile == min(_hip.KMEANS_MAX_TILE, _hip.KMEANS_LDS_BYTES // ((256 + 4) * 4) // 16 * 16)
    return tile + 1


# (N, D, K): every N of {1, 15, 17, 1000, 4099}, every D of {8, 96, 255, 256} and every K of {1, 2, 15, 16, 17, 100} at least once; a K that
# crosses a centroid tile at D = 256; K = 1024 at D = 8 (eight tiles).  A fourth entry "off": the rows start one element behind a 16-byte
# boundary while D is a multiple of 16, so every chunk of every row takes the loader's slow path (one full 16-row tile, one ragged tile,
# one chunk group)
SHAPES = [(1, 256, 1), (15, 96, 2), (17, 255, 15), (1000, 8, 16), (4099, 256, 17), (1000, 96, 100), (4099, 255, 16), (17, 8, 100), (1000, 256, "tile"),
          (1000, 8, 1024), (17, 256, 2, "off")]


def _shape(s):
    N, D, K = s[:3]
    return N, D, (_tile_crossing_k() if K == "tile" else K), len(s) > 3


def _shape_id(s):
    return "N{}-D{}-K{}".format(*s) + "-off" * (len(s) > 3)


def _lattice(N, D, K, seed, int8_zp=None):
    """Rows (lattice values, or int8 bytes over the full range) and lattice centroids with duplicates (ties), rows that are centroids and a
    few zero rows."""
    rng = np.random.default_rng(seed)
    C = (rng.integers(0, 16, (K, D)) / 16.0).astype(np.float32)
    C[C.sum(axis=1) == 0, 0] = 0.5
    if K >= 2:
        C[rng.integers(0, K, max(1, K // 4))] = C[rng.integers(0, K, max(1, K // 4))]   # duplicated centroids tie
    if int8_zp is None:
        X = (rng.integers(0, 16, (N, D)) / 16.0).astype(np.float32)
        take = min(N, K, 8)
        X[:take] = C[rng.integers(0, K, take)]
        zero = 0.0
    else:
        X = rng.integers(-128, 128, (N, D)).astype(np.int8)
        zero = int8_zp
    if N >= 15:
        X[[N // 2, N - 2]] = zero
    return X, C


def _check_assignment(torch, ctx, X, C, zp, what, off=False):
    from birdnet_stm32.evaluation.cluster import assign_reference

    wl, ws = assign_reference(X, C, zero_point=zp)
    gl, gs, changed = _assign(torch, ctx, X, C, zp, off=off)
    assert np.array_equal(gl, wl), f"{what}: labels differ on {int((gl != wl).sum())} of {len(wl)} rows"
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), f"{what}: scores differ"
    assert changed == int((wl >= 0).sum()), f"{what}: without previous labels every non-zero row counts"
    assert _assign(torch, ctx, X, C, zp, prev=gl, off=off)[2] == 0, f"{what}: the result as the previous labels"
    live = np.flatnonzero(wl >= 0)
    if live.size and C.shape[0] > 1:
        prev = gl.copy()
        prev[live[live.size // 2]] = (prev[live[live.size // 2]] + 1) % C.shape[0]
        l2, s2, ch = _assign(torch, ctx, X, C, zp, prev=prev, off=off)
        assert ch == 1 and np.array_equal(l2, gl) and np.array_equal(s2.view(np.uint32), gs.view(np.uint32)), f"{what}: one label altered by hand"
    return gl, gs


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_assignment_of_lattice_rows_equals_the_reference_bit_for_bit(torch_mod, ctx, shape):
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    N, D, K, off = _shape(shape)
    X, C = _lattice(N, D, K, 7 + N + D + K)
    gl, gs = _check_assignment(torch_mod, ctx, X, C, 0, shape, off)
    if N >= 15:
        assert (gl == -1).sum() == 2
    if N >= 1000 and K >= 15:
        dup = {i for i in range(K) if any(np.array_equal(C[i], C[j]) for j in range(i))}
        assert dup and not np.isin(gl, sorted(dup)).any(), "a duplicated centroid ties with its first copy and loses"
    # the existing search kernel with the roles swapped (centroids as the database, rows as the queries, k = 1) gives the same assignment
    swapped = EmbeddingIndex(C, np.zeros(K, np.int64), np.zeros(K), ["c"]).search(X, k=1, ctx=ctx)
    live = gl >= 0
    assert np.array_equal(swapped.idx[live, 0], gl[live]) and np.array_equal(swapped.score[live, 0].view(np.uint32), gs[live].view(np.uint32))


@pytest.mark.parametrize("zp", [-128, 0, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_assignment_of_int8_rows_equals_the_reference_bit_for_bit(torch_mod, ctx, shape, zp):
    N, D, K, off = _shape(shape)
    X, C = _lattice(N, D, K, 1000 + N + D + K + zp, int8_zp=zp)
    _check_assignment(torch_mod, ctx, X, C, zp, (shape, zp), off)


# ----------------------------------------------------------------------------------------------------------------------- update
def _unit_rows(N, D, seed, int8_zp=None):
    """Rows with exactly sixteen non-zero entries: +-1/4 (float32, inverse norm 1) or +-4 around the zero point (int8, inverse norm 1/16,
    so every term fl(inv * x) is +-1/4): sums of thousands of them are exact in float32."""
    rng = np.random.default_rng(seed)
    X = np.zeros((N, D), np.float32 if int8_zp is None else np.int8)
    if int8_zp is not None:
        X[:] = int8_zp
    for i in range(N):
        d = rng.choice(D, 16, replace=False)
        sign = rng.choice([-1, 1], 16)
        X[i, d] = sign * 0.25 if int8_zp is None else int8_zp + 4 * sign
    return X


def _segment_labels(seed):
    """Member counts of 1, segment - 1, segment and segment + 1 and two segments and a bit, two empty clusters, five rows without one."""
    from birdnet_stm32 import _hip

    seg = _hip.KMEANS_SEGMENT_ROWS
    counts = [1, seg - 1, 0, seg, seg + 1, 2 * seg + 3, 0]
    lab = np.concatenate([np.full(m, c) for c, m in enumerate(counts)] + [np.full(5, -1)])
    return np.random.default_rng(seed).permutation(lab), len(counts)


@pytest.mark.parametrize("D", [16, 96, 255, 256])
@pytest.mark.parametrize("case", ["segments", "one_cluster", "many_clusters", "int8"])
def test_update_sums_and_counts_are_exact(torch_mod, ctx, D, case):
    from birdnet_stm32.evaluation.cluster import update_reference

    zp = 5 if case == "int8" else None
    if case in ("segments", "int8"):
        labels, K = _segment_labels(D)
    elif case == "one_cluster":
        labels, K = np.full(1000, 1), 3
        labels[[3, 500]] = -1
    else:   # more clusters than one thread of the segment scan holds, with empty ones, and labels that are no cluster
        K = 300
        labels = np.random.default_rng(D).integers(-1, K + 2, 4099)
        labels[np.isin(labels, (0, 16, 17, 255, 256, 299))] = 1
    X = _unit_rows(len(labels), D, 3 + D, zp)
    ws, wc = update_reference(X, np.where(labels < K, labels, -1), K, zero_point=zp or 0)
    assert np.array_equal(ws, update_reference(X, np.where(labels < K, labels, -1), K, zero_point=zp or 0, dtype=np.float64)[0]), "the sums should be exact"
    for halves in (False, True):   # accumulate = 1 over two halves equals one call
        gs, gc = _accumulate(torch_mod, ctx, X, labels, K, zp or 0, halves)
        assert np.array_equal(gc, wc), (case, halves)
        assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (case, halves)
    assert (wc == 0).any() and wc.sum() == int(((labels >= 0) & (labels < K)).sum())


# ---------------------------------------------------------------------------------------------------------------------- bounded
def _clusters(n, D, C, seed, spread):
    """Rectified Gaussian clusters (as test_gpu_search.py makes them): non-negative like pooled ReLU features."""
    cent = np.random.default_rng(1000 + D + C).standard_normal((C, D))
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, C, n)
    return np.maximum(cent[lab] + spread * rng.standard_normal((n, D)), 0).astype(np.float32)


def _score_bound(X, C):
    """Float64 scores S [N, K] of float32 rows against float32 centroids and a bound on the float32 device error of each (the bound of
    test_gpu_search.py, derived there): |d S| <= (D + 2) u sum |x_j c_j| inv_x inv_c + |S| (D + 8) u, and 1 % on top."""
    D = X.shape[1]
    X, Y = X.astype(np.float64), C.astype(np.float64)
    dot, adot = X @ Y.T, np.abs(X) @ np.abs(Y).T
    nx, ny = np.sqrt((X * X).sum(axis=1)), np.sqrt((Y * Y).sum(axis=1))
    ix = np.divide(1.0, nx, out=np.zeros_like(nx), where=nx > 0)
    iy = np.divide(1.0, ny, out=np.zeros_like(ny), where=ny > 0)
    S = dot * ix[:, None] * iy[None, :]
    return S, 1.01 * ((D + 2) * U * adot * ix[:, None] * iy[None, :] + np.abs(S) * (D + 8) * U)


def _sum_bound(X, labels, K):
    """Float64 sums S [K, D] of inv_i x_i over the members and a bound on the float32 device error of each element.  The device's inverse
    norm is within ((D + 2) / 2 + 2) u (test_gpu_search.py), the product adds u, and a float32 sum of m terms in any order is within
    (m - 1) u sum |t|: |d S| <= ((D + 2) / 2 + 3 + (m - 1)) u sum |inv_i x_i|, and 1 % on top for the products of these terms."""
    D = X.shape[1]
    X64 = X.astype(np.float64)
    n = np.sqrt((X64 * X64).sum(axis=1))
    T = X64 * np.divide(1.0, n, out=np.zeros_like(n), where=n > 0)[:, None]
    S, A, m = np.zeros((K, D)), np.zeros((K, D)), np.bincount(labels[labels >= 0], minlength=K)
    for c in range(K):
        S[c], A[c] = T[labels == c].sum(axis=0), np.abs(T[labels == c]).sum(axis=0)
    return S, 1.01 * ((D + 2) / 2 + 3 + np.maximum(m - 1, 0))[:, None] * U * A, m


def _second_best_gap(S, B):
    """Per row the reference's label, and whether the float64 scores alone separate it from every centroid that is not a copy of it by
    more than the two bounds (copies of a centroid score the same bits on the device, and the lowest index wins on both sides)."""
    N = S.shape[0]
    best = np.argmax(S, axis=1)
    sb, bb = S[np.arange(N), best], B[np.arange(N), best]
    other = np.where(S == sb[:, None], -np.inf, S + B)   # (a copy of the best centroid has the same float64 score)
    return best, (sb - bb) > other.max(axis=1, initial=-np.inf)


def _teacher_forced(torch, ctx, X, C0, iters, min_clean):
    """The trajectory of the float64 reference from the float32 centroids C0; at every iteration the device's assignment of the
    reference's centroids and its update of the reference's labels are held to the bounds.  Returns per iteration (clean share, repaired)."""
    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation.cluster import centroids_from_sums, repair_empty_clusters

    K, D = C0.shape
    C = np.array(C0, np.float32)
    live = np.abs(X).sum(axis=1) > 0
    out, prev = [], None
    for it in range(iters):
        S, B = _score_bound(X, C)
        ref, clean = _second_best_gap(S, B)
        clean &= live
        share = float(clean[live].mean())
        print(f"iteration {it}: clean share {share:.4f}")
        assert share >= min_clean, "change the input, not the cap"
        gl, gs, _ = _assign(torch, ctx, X, C)
        assert (gl[~live] == -1).all() and (gs[~live] == 0).all() and (gl[live] >= 0).all() and (gl[live] < K).all()
        rows = np.flatnonzero(live)
        err = np.abs(gs[rows].astype(np.float64) - S[rows, gl[rows]])
        assert (err <= B[rows, gl[rows]]).all(), f"iteration {it}: largest score error / bound {float((err / B[rows, gl[rows]]).max()):.3f}"
        assert np.array_equal(gl[clean], ref[clean]), f"iteration {it}: labels differ on {int((gl[clean] != ref[clean]).sum())} clean rows"
        labels = np.where(live, ref, -1)
        if prev is not None and np.array_equal(labels, prev):
            break
        prev = labels
        S64, SB, m = _sum_bound(X, labels, K)
        gsum, gcount = _accumulate(torch, ctx, X, labels, K)
        assert np.array_equal(gcount, m)
        assert (np.abs(gsum.astype(np.float64) - S64) <= SB).all(), f"iteration {it}: a sum is outside its bound"
        # the device's centroids of its own sums: within the sums' relative bound twice (the sum and its norm) and the norm's and product's roundings
        d_s = torch.from_numpy(gsum).cuda()
        d_n = torch.from_numpy(gcount).cuda()
        d_c = torch.from_numpy(C).cuda()
        d_i = torch.empty(K, dtype=torch.float32, device="cuda")
        _hip.check(ctx.lib.bn_kmeans_centroids(ctx.handle, d_s.data_ptr(), d_n.data_ptr(), K, D, d_c.data_ptr(), d_i.data_ptr(), None))
        torch.cuda.synchronize()
        Cref = centroids_from_sums(S64, m, C, np.float64)
        rel = 1.01 * (2 * ((D + 2) / 2 + 3 + np.maximum(m - 1, 0)) + (D + 2) / 2 + 3) * U
        if (X >= 0).all():   # (non-negative terms: the sums' bounds are relative, so the bound carries over to the normalised centroid)
            assert (np.abs(d_c.cpu().numpy().astype(np.float64) - Cref) <= rel[:, None] * np.abs(Cref)).all(), f"iteration {it}: a centroid is outside its bound"
        assert np.array_equal(d_c.cpu().numpy()[m == 0], C[m == 0]), "a cluster without members keeps its centroid"
        C, _, repaired = repair_empty_clusters(Cref.astype(np.float32), m)
        out.append((share, repaired))
    return out


@pytest.mark.parametrize("N,D,K,spread,seed", [(4099, 256, 16, 0.3, 5), (4099, 256, 24, 0.6, 0), (1000, 96, 8, 0.3, 42), (4099, 255, 12, 0.5, 42),
                                               (1000, 8, 4, 0.2, 42), (4099, 256, 16, 1.0, 42)])
def test_teacher_forced_trajectory_within_the_bounds(torch_mod, ctx, N, D, K, spread, seed):
    """Twelve rectified Gaussian clusters fitted with K centroids from a seeded start, five iterations.  Clean shares of the float64
    reference on the CPU, the worst over the iterations: 99.63 %, 99.66 %, 100 %, 99.85 %, 100 %, 99.85 % in the order of the parameters.
    The starts are ones after which no cluster comes out empty: the halves of a repaired cluster lie 1/1024 apart and their members are
    not clean (the repair has a test of its own below); with 24 centroids the spread is 0.6, since at 0.3 the blobs are cut into pieces
    whose borders leave 98.6 % clean under this bound."""
    from birdnet_stm32.evaluation.cluster import seeded_centroids

    X = _clusters(N, D, 12, 5, spread)
    X[N // 3] = 0
    steps = _teacher_forced(torch_mod, ctx, X, seeded_centroids(X, 0, K, seed, 0), 5, 0.99)
    assert len(steps) >= 3 and not any(r for _, r in steps)


# -------------------------------------------------------------------------------------------------------------------- whole fit
def _blocks(N, D, K, seed=0):
    """Row i belongs to block i mod K: values in [1, 1.5] on the D // K dimensions of its block, 0.05 |N(0, 1)| elsewhere."""
    rng = np.random.default_rng(seed)
    x = 0.05 * np.abs(rng.standard_normal((N, D)))
    w = D // K
    for i in range(N):
        c = i % K
        x[i, c * w:(c + 1) * w] = rng.uniform(1.0, 1.5, w)
    return x.astype(np.float32)


def _index(x, **kw):
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    n = x.shape[0]
    return EmbeddingIndex(x, np.arange(n) // 50, np.zeros(n), [f"f{i}.wav" for i in range(n // 50 + 1)], **kw)


@pytest.mark.parametrize("N,D,K", [(1000, 96, 8), (4099, 256, 16), (4099, 255, 15), (17, 8, 2)])
def test_fit_of_separated_blocks_equals_the_reference(torch_mod, ctx, N, D, K):
    from birdnet_stm32.evaluation.cluster import centroids_from_sums, cluster_index, kmeans_reference

    x = _blocks(N, D, K)
    want = kmeans_reference(x, K, init_centroids=x[:K])
    assert want.n_iter == 1 and want.converged and np.array_equal(want.labels, np.arange(N) % K)
    # every row is clean at both assignments by at least nine times the bound, so the device has no choice
    S64, SB, m = _sum_bound(x, want.labels, K)
    C1 = centroids_from_sums(S64, m, x[:K], np.float64)
    for C in (x[:K], C1.astype(np.float32)):
        S, B = _score_bound(x, C)
        top = np.sort(S, axis=1)[:, ::-1]
        assert (np.argmax(S, axis=1) == want.labels).all() and ((top[:, 0] - top[:, 1]) > 9 * 2 * B.max(axis=1)).all()
    index = _index(x)
    got = cluster_index(index, K, init_centroids=x[:K], ctx=ctx)
    assert np.array_equal(got.labels, want.labels) and np.array_equal(got.counts, want.counts) and got.n_iter == 1 and got.converged
    rel = 1.01 * (2 * ((D + 2) / 2 + 3 + (m - 1)) + (D + 2) / 2 + 3) * U   # (as in _teacher_forced: the rows are non-negative)
    assert (np.abs(got.centroids.astype(np.float64) - C1) <= rel[:, None] * np.abs(C1)).all()
    S, B = _score_bound(x, got.centroids)
    err = np.abs(got.score.astype(np.float64) - S[np.arange(N), got.labels])
    assert (err <= B[np.arange(N), got.labels]).all() and abs(got.mean_score - got.score.astype(np.float64).mean()) < 1e-12
    # a budget that streams three blocks per iteration gives the labels of the resident run
    if N >= 1000:
        small = _index(x, budget_bytes=-(-N // 3) * D * 4)
        assert len(small.block_ranges()) == 3
        parts = cluster_index(small, K, init_centroids=x[:K], ctx=ctx)
        assert np.array_equal(parts.labels, got.labels) and np.array_equal(parts.counts, got.counts) and parts.n_iter == 1 and parts.converged
        assert (np.abs(parts.centroids.astype(np.float64) - C1) <= rel[:, None] * np.abs(C1)).all()
        # exemplars are index.search(centroids): the best rows of a block's centroid are rows of that block
        ex = cluster_index(index, K, init_centroids=x[:K], exemplars=3, ctx=ctx)
        assert ex.exemplar_idx.shape == (K, 3) and (ex.exemplar_idx % K == np.arange(K)[:, None]).all()
        hits = index.search(ex.centroids, k=3, ctx=ctx)
        assert np.array_equal(hits.idx, ex.exemplar_idx) and np.array_equal(hits.score, ex.exemplar_score)


def _repair64(C, counts):
    """repair_empty_clusters in float64, for the bound: (centroids, the clusters it wrote)."""
    C, counts, touched = np.array(C, np.float64), np.array(counts), []
    sign = np.where(np.arange(C.shape[1]) % 2 == 0, 1.0, -1.0) / 1024
    for j in np.flatnonzero(counts == 0):
        L = int(np.argmax(counts))
        if counts[L] < 2:
            continue
        up, down = C[L] * (1 + sign), C[L] * (1 - sign)
        C[j], C[L] = up / np.linalg.norm(up), down / np.linalg.norm(down)
        counts[j] = counts[L] // 2
        counts[L] -= counts[j]
        touched += [int(j), L]
    return C, touched


@pytest.mark.parametrize("N,D,true,K,spread,seed", [(1000, 32, 8, 24, 0.5, 8), (2000, 64, 12, 32, 0.7, 0)])
def test_seeded_fit_with_a_duplicated_initial_row_goes_through_the_repair(torch_mod, ctx, N, D, true, K, spread, seed):
    """Every row twice, and a seed whose draw takes both copies of one row: the second copy ties with the first at every row, loses and
    comes out empty, so the device fit's own update reads the counts back, repairs the centroids on the host and uploads them again.  One
    teacher-forced step through ``cluster_index`` (the reference's start, ``max_iter = 1``): every row is clean at the first assignment
    (copies of a centroid left out: they score the same bits and the lowest index wins on both sides), so the device has no choice of
    labels and its centroids behind the repair must lie within the update's bound of the float64 reference's; the labels it returns must
    belong to the centroids it returns, where at least 99 % of the rows are clean (99.8 % and 99.5 % with the reference on the CPU: the
    narrow rows keep the bound well under the 1/1024 that parts the halves of the split cluster)."""
    from birdnet_stm32.evaluation.cluster import centroids_from_sums, cluster_index, repair_empty_clusters, seeded_centroids, seeded_rows
    from birdnet_stm32.evaluation.search import inv_norms_reference

    x = _clusters(N, D, true, 8, spread)
    x[1::2] = x[0::2]
    inv = inv_norms_reference(x)
    assert (inv != 0).all() and (np.diff(seeded_rows(inv, K, seed, 0) // 2) == 0).any(), "the draw should hold a row twice"
    C0 = seeded_centroids(x, 0, K, seed, 0, inv)
    S, B = _score_bound(x, C0)
    ref0, clean0 = _second_best_gap(S, B)
    assert clean0.all(), "change the input: every row should be clean at the first assignment"
    S64, SB, m = _sum_bound(x, ref0, K)
    assert (m == 0).sum() >= 1 and m.max() >= 2
    C1, touched = _repair64(centroids_from_sums(S64, m, C0, np.float64), m)
    _, counts1, repaired = repair_empty_clusters(C0, m)
    assert repaired >= 1 and len(set(touched)) == 2 * repaired

    got = cluster_index(_index(x), K, init_centroids=C0, max_iter=1, ctx=ctx)
    assert got.n_iter == 1
    # the sums' relative bound twice (the sum and its norm) and the norm's and product's roundings, as in _teacher_forced; a repaired
    # centroid is scaled (one rounding) and normalised again on top of its source's error (its source's member count rules its bound)
    r_sum = ((D + 2) / 2 + 3 + np.maximum(m - 1, 0)) * U
    rel = 2 * r_sum + ((D + 2) / 2 + 3) * U
    src = np.arange(K)
    for pair in np.asarray(touched, int).reshape(-1, 2):
        src[pair[0]] = src[pair[1]]   # (cluster j takes its centroid from L, which may itself have been repaired from another)
    rel_rep = 2 * (rel[src] + U) + ((D + 2) / 2 + 3) * U
    bound = 1.01 * np.where(np.isin(np.arange(K), touched), rel_rep, rel)
    err = np.abs(got.centroids.astype(np.float64) - C1)
    assert (err <= bound[:, None] * np.abs(C1)).all(), f"largest centroid error / bound {float((err / np.maximum(bound[:, None] * np.abs(C1), 1e-300)).max()):.3f}"
    assert len({c.tobytes() for c in got.centroids}) == K, "the repair should have parted the copies"
    # the returned labels and scores belong to the returned centroids
    S, B = _score_bound(x, got.centroids)
    ref1, clean1 = _second_best_gap(S, B)
    print(f"behind the repair: clean share {clean1.mean():.4f}")
    assert clean1.mean() >= 0.99, "change the input, not the cap"
    assert np.array_equal(got.labels[clean1], ref1[clean1]), f"labels differ on {int((got.labels[clean1] != ref1[clean1]).sum())} clean rows"
    err = np.abs(got.score.astype(np.float64) - S[np.arange(N), got.labels])
    assert (err <= B[np.arange(N), got.labels]).all()
    assert np.array_equal(got.counts, np.bincount(got.labels, minlength=K)) and (got.counts[(m == 0)] > 0).all(), "the repaired clusters should have members now"


def test_library_names_the_clustering_kernels(ctx):
    names = ctx.lib.bn_kernel_names().decode().split("\n")
    assert {"kmeans_assign_kernel", "kmeans_keys_kernel", "kmeans_offsets_kernel", "kmeans_segments_kernel", "kmeans_partial_kernel", "kmeans_fold_kernel",
            "kmeans_scale_kernel"} <= set(names)


def test_same_seed_same_bits_other_seed_other_centroids_and_the_best_restart(torch_mod, ctx):
    from birdnet_stm32.evaluation.cluster import cluster_index, seeded_centroids

    x = _clusters(1000, 96, 8, 5, 0.5)
    x[7] = 0
    index = _index(x)
    a = cluster_index(index, 8, max_iter=6, seed=3, ctx=ctx)
    b = cluster_index(index, 8, max_iter=6, seed=3, ctx=ctx)
    for f in ("labels", "counts"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(a.centroids.view(np.uint32), b.centroids.view(np.uint32)) and np.array_equal(a.score.view(np.uint32), b.score.view(np.uint32))
    assert a.labels[7] == -1 and a.score[7] == 0 and a.counts.sum() == 999 and a.n_iter >= 1
    assert np.array_equal(a.counts, np.bincount(a.labels[a.labels >= 0], minlength=8))
    c = cluster_index(index, 8, max_iter=6, seed=4, ctx=ctx)
    assert not np.array_equal(a.centroids, c.centroids)
    # n_init = 3 returns the restart the float64 means select
    singles = [cluster_index(index, 8, max_iter=3, init_centroids=seeded_centroids(x, 0, 8, 3, r), ctx=ctx) for r in range(3)]
    means = [float(s.score[s.labels >= 0].astype(np.float64).sum() / (s.labels >= 0).sum()) for s in singles]
    assert [s.mean_score for s in singles] == means and len(set(means)) == 3
    best = cluster_index(index, 8, max_iter=3, n_init=3, seed=3, ctx=ctx)
    want = int(np.argmax(means))
    assert best.restart == want and best.mean_score == means[want]
    assert np.array_equal(best.centroids.view(np.uint32), singles[want].centroids.view(np.uint32)) and np.array_equal(best.labels, singles[want].labels)
    # int8 bytes: the fit runs on float32(byte - zero_point)
    b8 = np.clip(np.rint(x * 20) - 100, -128, 127).astype(np.int8)
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    i8 = EmbeddingIndex(b8, np.zeros(1000, np.int64), np.zeros(1000), ["a.wav"], "int8", 0.05, -100)
    r8 = cluster_index(i8, 8, max_iter=3, seed=3, ctx=ctx)
    assert r8.labels[7] == -1 and r8.counts.sum() == int((b8 != -100).any(axis=1).sum())
    S, B = _score_bound(b8.astype(np.float32) + 100, r8.centroids)
    live = r8.labels >= 0
    err = np.abs(r8.score[live].astype(np.float64) - S[live, r8.labels[live]])
    assert (err <= B[live, r8.labels[live]]).all()


def test_refused_calls(torch_mod, ctx):
    from birdnet_stm32 import _hip

    torch = torch_mod
    rows = torch.zeros((32, 16), dtype=torch.float32, device="cuda")
    inv = torch.ones(32, dtype=torch.float32, device="cuda")
    cent = torch.ones((4, 16), dtype=torch.float32, device="cuda")
    label = torch.full((33,), -7, dtype=torch.int32, device="cuda")
    prev = torch.zeros(32, dtype=torch.int32, device="cuda")
    score = torch.full((32,), 3.0, dtype=torch.float32, device="cuda")
    changed = torch.full((2,), -5, dtype=torch.int64, device="cuda")
    sums = torch.full((4, 16), 9.0, dtype=torch.float32, device="cuda")
    counts = torch.full((4,), -9, dtype=torch.int64, device="cuda")
    ok = dict(rows=rows.data_ptr(), dtype=_hip.DTYPE_F32, n=32, D=16, zp=0, inv=inv.data_ptr(), cent=cent.data_ptr(), cinv=inv.data_ptr(), K=4, prev=prev.data_ptr(),
              label=label.data_ptr(), score=score.data_ptr(), changed=changed.data_ptr(), sums=sums.data_ptr(), counts=counts.data_ptr())

    def assign(**kw):
        a = dict(ok, **kw)
        return ctx.lib.bn_kmeans_assign(ctx.handle, a["rows"], a["dtype"], a["n"], a["D"], a["zp"], a["inv"], a["cent"], a["cinv"], a["K"], a["prev"], a["label"],
                                        a["score"], a["changed"], None)

    def accumulate(**kw):
        a = dict(ok, **kw)
        return ctx.lib.bn_kmeans_accumulate(ctx.handle, a["rows"], a["dtype"], a["n"], a["D"], a["zp"], a["inv"], a["label"], a["K"], 0, a["sums"], a["counts"], None)

    shape = [dict(K=0), dict(K=_hip.KMEANS_MAX_K + 1), dict(D=0), dict(D=_hip.KMEANS_MAX_D + 1), dict(dtype=2), dict(dtype=-1), dict(n=-1), dict(n=1 << 31),
             dict(rows=None), dict(inv=None), dict(label=None), dict(rows=rows.data_ptr() + 2), dict(dtype=_hip.DTYPE_I8, zp=128)]
    for kw in shape + [dict(cent=None), dict(cinv=None), dict(score=None), dict(changed=None), dict(prev=label.data_ptr()), dict(changed=changed.data_ptr() + 4)]:
        assert assign(**kw) == -1 and ctx.lib.bn_last_error(), kw   # BN_ERR_ARG
    for kw in shape + [dict(sums=None), dict(counts=None), dict(counts=counts.data_ptr() + 4)]:
        assert accumulate(**kw) == -1 and ctx.lib.bn_last_error(), kw
    assert ctx.lib.bn_kmeans_centroids(ctx.handle, None, counts.data_ptr(), 4, 16, cent.data_ptr(), inv.data_ptr(), None) == -1
    assert ctx.lib.bn_kmeans_centroids(ctx.handle, sums.data_ptr(), counts.data_ptr(), 0, 16, cent.data_ptr(), inv.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert bool((label == -7).all()) and bool((score == 3.0).all()) and bool((changed == -5).all()) and bool((sums == 9.0).all()) and bool((counts == -9).all())
    assert bool((inv == 1.0).all()) and bool((cent == 1.0).all()), "a refused call wrote to its outputs"
    assert assign(prev=None) == 0   # the previous labels may be NULL
    torch.cuda.synchronize()
    # every score is 0 (the rows hold zeros; the inverse norms handed in are ones, so they count as rows): centroid 0, by index
    assert label.cpu().numpy().tolist() == [0] * 32 + [-7] and bool((score == 0.0).all()) and changed.cpu().numpy().tolist() == [32, -5]


# ------------------------------------------------------------------------------------------------------------------- end to end
SR = 22050   # the shipped model's config


def _write_wav(path, x):
    pcm = np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(SR)
        w.writeframes(pcm.tobytes())


def _tone(freq, gain, seconds=3.0):
    t = np.arange(int(SR * seconds)) / SR
    return gain * (0.5 * np.sin(2 * np.pi * freq * t) + 0.02 * np.sin(2 * np.pi * 3.1 * freq * t))


@pytest.mark.parametrize("model,dtype", [(TFLITE_PATH, "int8"), (KERAS_PATH, "float32")], ids=["int8", "float32"])
def test_embed_then_cluster_end_to_end(torch_mod, tmp_path, model, dtype):
    from birdnet_stm32.cli import cluster as cluster_cli
    from birdnet_stm32.cli import embed as embed_cli
    from birdnet_stm32.cli import search as search_cli
    from birdnet_stm32.evaluation.cluster import seeded_rows
    from birdnet_stm32.evaluation.search import EmbeddingIndex, inv_norms_reference
    from birdnet_stm32.models.runners import load_model_runner

    paths = []
    for kind, freq in enumerate((700.0, 2000.0, 4800.0)):   # three kinds of clip, eight of each: the tone a little off and louder or softer
        for j in range(8):
            paths.append(str(tmp_path / f"kind{kind}_{j}.wav"))
            _write_wav(paths[-1], _tone(freq * (1 + 0.004 * (j - 4)), 0.6 + 0.1 * j))
    ext = os.path.splitext(model)[1]
    ckpt = tmp_path / ("m" + ext)
    ckpt.write_bytes(open(model, "rb").read())
    (tmp_path / "m_model_config.json").write_text(open(CONFIG_PATH).read())
    runner = load_model_runner(str(ckpt), max_batch=64)
    db_npz = str(tmp_path / "db.npz")
    try:
        embed_cli.main(["--model_path", str(ckpt), "--input", *paths, "--output", db_npz, "--dtype", dtype], runner=runner)
    finally:
        runner.close()
    index = EmbeddingIndex.from_npz(db_npz)
    assert len(index) == 24 and index.dtype == dtype
    kind = np.asarray([int(os.path.basename(index.paths[int(f)])[4]) for f in index.file_index])
    # k-means keeps what its start gives it: the test takes a seed whose three initial rows are of three kinds
    inv = inv_norms_reference(index.embeddings, index.zero_point)
    assert (inv != 0).all()
    seed = next(s for s in range(100) if len(set(kind[seeded_rows(inv, 3, s, 0)])) == 3)
    out, cent = str(tmp_path / "clusters.csv"), str(tmp_path / "C.npz")
    ex = "2" if dtype == "float32" else "0"
    res = cluster_cli.main(["--database", db_npz, "--k", "3", "--output", out, "--seed", str(seed), "--exemplars", ex, "--centroids_out", cent, "--chunk_duration", "3"])
    assert res.converged and sorted(res.counts.tolist()) == [8, 8, 8]
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == cluster_cli.CSV_COLUMNS and len(rows) == 25 and all(float(r[2]) == float(r[1]) + 3.0 for r in rows[1:])
    by_kind = {}
    for r in rows[1:]:
        by_kind.setdefault(os.path.basename(r[0])[4], set()).add(r[3])
    assert all(len(v) == 1 for v in by_kind.values()) and len(set.union(*by_kind.values())) == 3, "every clip of a kind shares a cluster"
    with open(cluster_cli.summary_path(out), newline="") as f:
        summary = list(csv.reader(f))
    assert len(summary) == 4 and [r[1] for r in summary[1:]] == ["8", "8", "8"] and len(summary[0]) == 3 + int(ex)
    if dtype == "float32":
        for r in summary[1:]:   # a cluster's exemplars are clips of its kind
            assert {os.path.basename(e.split("@")[0])[4] for e in r[3:]} == {k for k, v in by_kind.items() if v == {r[0]}}
        hits_csv = str(tmp_path / "hits.csv")
        search_cli.main(["--database", db_npz, "--query_npz", cent, "--chunk_duration", "3", "--output", hits_csv, "--top_k", "2"])
        with open(hits_csv, newline="") as f:
            hits = list(csv.reader(f))[1:]
        assert len(hits) == 6 and [h[0] for h in hits[::2]] == ["cluster_000", "cluster_001", "cluster_002"]
        assert [h[4] + "@" + h[5] for h in hits] == [e for r in summary[1:] for e in r[3:]]
    else:
        assert EmbeddingIndex.from_npz(cent).dtype == "float32" and len(EmbeddingIndex.from_npz(cent)) == 3
        with pytest.raises(SystemExit, match="int8"):
            cluster_cli.main(["--database", db_npz, "--k", "3", "--output", out, "--exemplars", "2"])
    with pytest.raises(SystemExit, match="non-zero rows"):
        cluster_cli.main(["--database", db_npz, "--k", "25", "--output", out, "--exemplars", "0"])
