"""GPU tests of projection (csrc/bn_tsne.hip, evaluation/project.py, cli/project.py) against the numpy specification.

The error bounds are counted from the kernels' code, in units of u = 2^-24 (v = 2^-53 for the float64 parts), with
gamma(c) = c u / (1 - c u) for a chain of c roundings:

  per pair, both gradient kernels:  dx, dy one rounding each; d2 = fma(dy, dy, fma(dx, dx, 1)) sees 2 u from dx^2 (dy^2) and rounds twice:
      4 u; w = v_rcp_f32(d2), 1 ulp = 2 u: w carries 6 u.
  A_i:  pw = fl(p w) 7 u, the term pw dx 8 u = C_A; the product's rounding inside fma(pw, dx, acc) and every later addition (the lane's
      chain, then the tree over 16 lanes, where adding a zero is exact) are at most m roundings for a row of m entries.
  R_i:  w2 = fl(w w) 13 u, the term w2 dx 14 u = C_R; the fused accumulations over a column range (two chains, even and odd columns, added
      at the end) and the addition of the ranges are at most m = n - 1 roundings on any term's way (a chain holds at most
      BN_TSNE_SPLIT_J / 2 terms, and the left-out j = i adds an exact zero).
  Z:    z_i is a chain of n - 1 additions of terms with 6 u each, Z their float64 sum: eps_Z = gamma(n + 5) + n v.  (The test of Z itself
      asks for n u, as the issue states it: the 6 u of a single w are the worst case and do not add up in the same direction.)
  grad: fl(E A) one rounding, R / Z a float64 division rounded once to float32, the difference one rounding, the factor 4 exact:
      |grad - ref| <= 4 (1 + 1e-3) [(gamma(C_A + m_A) + 2 u) E abs_A + (gamma(C_R + n - 1) + eps_Z + 2 u) abs_R / Z]
      with abs_A, abs_R the sums of the absolute values of the terms (``gradient_reference``); the factor 1 + 1e-3 covers the products of
      the (1 + gamma) factors, all below 1 + 3e-4 at these sizes.  A missed or doubled tile is an error of the order of abs_R / Z itself.
  kl_i: float64 throughout: the differences, two fused multiply-adds and p d2 put 5 v on the logarithm's argument, an absolute 5 v p on
      the term; the logarithm (2 ulp allowed) and the product 5 v relative; m additions:
      |kl_i - ref| <= (1 + 1e-3) [5 v sum_j p_ij + (5 + m) v abs_kl].
"""

import csv
import functools
import math

import numpy as np
import pytest

import project_cases as cases

pytestmark = pytest.mark.gpu

U, V = 2.0 ** -24, 2.0 ** -53
C_A, C_R = 8, 14
NAN_BITS = 0x7FC0BEEF
NAN64_BITS = 0x7FF80000DEADBEEF
BN_ERR_ARG = -1


def gamma(c):
    return c * U / (1 - c * U)


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


def test_library_names_the_projection_kernels(ctx):
    names = ctx.lib.bn_kernel_names().decode().split("\n")
    assert {"tsne_perplexity_kernel", "tsne_repulsion_kernel", "tsne_fold_kernel", "tsne_z_kernel", "tsne_attraction_kernel", "tsne_update_kernel"} <= set(names)


# ------------------------------------------------------------------------------------------------------------------ perplexity
def _scores(n, k, seed, duplicates):
    """[n, k] cosine scores of random unit rows against their k best others, descending; row 0 with all neighbours at one distance, the
    last row with ``duplicates`` exact duplicates among its neighbours (score 1: d2 = 0; its entropy cannot fall below log(duplicates))."""
    rng = np.random.default_rng(seed)
    m = max(n, k + 1) + 1
    x = rng.standard_normal((m, 16)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    s = x[:n] @ x.T
    s[np.arange(n), np.arange(n)] = -np.inf
    s = -np.sort(-s, axis=1)[:, :k]
    s[0] = np.float32(0.375)
    if n > 1:
        s[n - 1, :duplicates] = 1.0
    return np.ascontiguousarray(s, np.float32)


def _perplexity(torch, ctx, score, perplexity):
    from birdnet_stm32 import _hip

    n, k = score.shape
    d_s = torch.from_numpy(score).cuda()
    p = torch.full((n + 2, k), NAN_BITS, dtype=torch.int32, device="cuda")
    beta = torch.full((n + 2,), NAN64_BITS, dtype=torch.int64, device="cuda")
    _hip.check(ctx.lib.bn_tsne_perplexity(ctx.handle, d_s.data_ptr(), n, k, perplexity, p[1:].data_ptr(), beta[1:].data_ptr(), None))
    torch.cuda.synchronize()
    ph, bh = p.cpu().numpy(), beta.cpu().numpy()
    assert (ph[0] == NAN_BITS).all() and (ph[n + 1] == NAN_BITS).all() and bh[0] == NAN64_BITS and bh[n + 1] == NAN64_BITS, "a guard row was written"
    assert np.array_equal(d_s.cpu().numpy(), score), "an input changed"
    return ph[1:n + 1].view(np.float32), bh[1:n + 1].view(np.float64)


@pytest.mark.parametrize("n", [1, 15, 17, 1000])
@pytest.mark.parametrize("k", [1, 5, 90, 126])
def test_conditional_affinities(torch_mod, ctx, n, k):
    """Property, in float64 from the device's float32 p: a row sums to 1 within u (every p_j carries at most u p_j, and they sum to 1) plus
    (k + 16) v for the two float64 sums; its entropy H = -sum p log p moves by at most sum |dp_j| |log p_j + 1| <= u (H + 1) <= u (log k + 1)
    <= k u under that storage error, on top of the 1e-5 the search stops at.  Value: with the device's beta, p is the float64 expression
    rounded once (u p, plus (k + 16) v p for the two float64 evaluations, plus the smallest subnormal)."""
    from birdnet_stm32.evaluation.project import squared_distances

    perplexity = 1.0 if k == 1 else min(30.0, k / 3.0)
    score = _scores(n, k, 100 * n + k, max(1, min(3, int(perplexity))))
    p, beta = _perplexity(torch_mod, ctx, score, perplexity)
    assert np.isfinite(p).all() and (p >= 0).all() and np.isfinite(beta).all() and (beta > 0).all()
    p64 = p.astype(np.float64)
    assert np.abs(p64.sum(axis=1) - 1).max() <= U + (k + 16) * V + k * 2.0 ** -149
    H = -(p64 * np.log(np.where(p64 > 0, p64, 1))).sum(axis=1)
    searched = np.ones(n, bool)
    if k > 1:
        searched[0] = False   # equidistant neighbours: H = log k whatever beta, uniform
        assert np.array_equal(p[0], np.full(k, np.float32(1.0 / k)))
    print("largest entropy error", np.abs(H - math.log(perplexity))[searched].max() if searched.any() else 0.0, "bound", 1e-5 + k * U)
    assert (np.abs(H - math.log(perplexity))[searched] <= 1e-5 + k * U).all()
    d = squared_distances(score).astype(np.float64)
    d -= d.min(axis=1, keepdims=True)
    want = np.exp(-beta[:, None] * d)
    want /= want.sum(axis=1, keepdims=True)
    assert (np.abs(p64 - want) <= (U + (k + 16) * V) * want + 2.0 ** -149).all()


# -------------------------------------------------------------------------------------------------------------------- gradient
def _gradient(torch, ctx, Y, csr, E, want_kl):
    """bn_tsne_gradient between guard rows: (grad [n, 2] float32, Z float64, kl_rows [n] float64 or None)."""
    from birdnet_stm32 import _hip

    n = Y.shape[0]
    rowptr, col, val = csr
    d_y = torch.from_numpy(np.ascontiguousarray(Y, np.float32)).cuda()
    d_rp = torch.from_numpy(np.ascontiguousarray(rowptr, np.int64)).cuda()
    d_col = torch.from_numpy(np.ascontiguousarray(np.append(col, 0), np.int32)).cuda()   # (one spare entry: an empty matrix still has an address)
    d_val = torch.from_numpy(np.ascontiguousarray(np.append(val, 0), np.float32)).cuda()
    grad = torch.full((n + 2, 2), NAN_BITS, dtype=torch.int32, device="cuda")
    z = torch.full((3,), NAN64_BITS, dtype=torch.int64, device="cuda")
    kl = torch.full((n + 2,), NAN64_BITS, dtype=torch.int64, device="cuda")
    _hip.check(ctx.lib.bn_tsne_gradient(ctx.handle, d_y.data_ptr(), n, d_rp.data_ptr(), d_col.data_ptr(), d_val.data_ptr(), E, grad[1:].data_ptr(), z[1:].data_ptr(),
                                        kl[1:].data_ptr() if want_kl else None, None))
    torch.cuda.synchronize()
    g, zh, kh = grad.cpu().numpy(), z.cpu().numpy(), kl.cpu().numpy()
    assert (g[0] == NAN_BITS).all() and (g[n + 1] == NAN_BITS).all() and zh[0] == NAN64_BITS and zh[2] == NAN64_BITS, "a guard row was written"
    assert kh[0] == NAN64_BITS and kh[n + 1] == NAN64_BITS and (want_kl or (kh == NAN64_BITS).all()), "a guard row was written"
    assert np.array_equal(d_y.cpu().numpy(), Y) and np.array_equal(d_rp.cpu().numpy(), rowptr) and np.array_equal(d_col.cpu().numpy()[:-1], col)
    assert np.array_equal(d_val.cpu().numpy()[:-1], val), "an input changed"
    return g[1:n + 1].view(np.float32), float(zh[1:2].view(np.float64)[0]), (kh[1:n + 1].view(np.float64) if want_kl else None)


def _check_gradient(torch, ctx, Y, csr, what):
    """E = 1 (with the divergence's rows) and E = 12 against ``gradient_reference`` under the bounds of the module docstring."""
    from birdnet_stm32.evaluation.project import gradient_reference

    Y = np.ascontiguousarray(Y, np.float32)
    n = Y.shape[0]
    rowptr, col, val = csr
    ref = gradient_reference(Y, rowptr, col, val, 1.0)
    m_A = np.diff(rowptr).astype(np.float64)[:, None]
    eps_Z = gamma(n + 5) + n * V
    p_rows = np.bincount(np.repeat(np.arange(n), np.diff(rowptr)), val.astype(np.float64), n)
    for E in (1.0, 12.0):
        grad, Z, kl = _gradient(torch, ctx, Y, csr, E, E == 1.0)
        want = 4.0 * (E * ref.A - ref.R / ref.Z)
        bound = 4.0 * (1 + 1e-3) * ((gamma(C_A + m_A) + 2 * U) * E * ref.abs_A + (gamma(C_R + n - 1) + eps_Z + 2 * U) * ref.abs_R / ref.Z) + 2.0 ** -149
        err = np.abs(grad.astype(np.float64) - want)
        print(f"{what} n={n} E={E}: largest gradient error / bound {np.max(err / bound):.3g}, Z error {abs(Z - ref.Z) / ref.Z / U:.3g} u (asked: {n} u)")
        assert np.isfinite(grad).all() and (err <= bound).all(), (what, n, E, float(np.max(err / bound)))
        assert abs(Z - ref.Z) <= n * U * ref.Z, (what, n, abs(Z - ref.Z) / ref.Z / U)
        if kl is not None:
            kbound = (1 + 1e-3) * (5 * V * p_rows + (5 + m_A[:, 0]) * V * ref.abs_kl) + 1e-300
            kerr = np.abs(kl - ref.kl_rows)
            print(f"{what} n={n}: largest divergence-row error / bound {np.max(kerr / kbound):.3g}")
            assert (kerr <= kbound).all(), (what, n, float(np.max(kerr / kbound)))


def _split_crossing_n():
    """One column more than a column range of the repulsion holds, from the header's constants."""
    from birdnet_stm32 import _hip

    assert _hip.TSNE_SPLIT_J % _hip.TSNE_TILE_J == 0 and _hip.TSNE_TILE_I == 256
    return _hip.TSNE_SPLIT_J + 1


@functools.lru_cache(maxsize=None)
def _knn_matrix(n):
    """The symmetrised kNN matrix of n random rows (D = 8), k = min(n - 1, 15)."""
    from birdnet_stm32.evaluation.project import conditional_p_reference, neighbours_reference, symmetrize

    rows = np.random.default_rng(n).standard_normal((n, 8)).astype(np.float32)
    k = min(n - 1, 15)
    idx, score = neighbours_reference(rows, k)
    p, _ = conditional_p_reference(score, max(1.0, min(5.0, k / 3.0)))
    return symmetrize(idx, p.astype(np.float32), n)


def _map(n, kind):
    rng = np.random.default_rng(7 * n + len(kind))
    if kind == "start":       # all w ~ 1: heavy cancellation in R
        return (1e-4 * rng.standard_normal((n, 2))).astype(np.float32)
    if kind == "duplicates":  # exact duplicate points: w = 1, no force between them
        y = (3.0 * rng.standard_normal((n, 2))).astype(np.float32)
        y[n // 2:] = y[:n - n // 2]
        return y
    assert kind == "far"      # coordinates of magnitude 10^3
    return (1e3 * rng.standard_normal((n, 2))).astype(np.float32)


GRADIENT_N = [2, 3, 17, 255, 256, 257, 1000, 4099, "split"]


@pytest.mark.parametrize("kind", ["start", "duplicates", "far"])
@pytest.mark.parametrize("n", GRADIENT_N)
def test_gradient_within_the_bounds(torch_mod, ctx, n, kind):
    n = _split_crossing_n() if n == "split" else n
    _check_gradient(torch_mod, ctx, _map(n, kind), _knn_matrix(n), kind)


@functools.lru_cache(maxsize=1)
def _cluster_matrix():
    from birdnet_stm32.evaluation.project import conditional_p_reference, neighbour_count, neighbours_reference, symmetrize

    rows = cases.three_clusters()
    idx, score = neighbours_reference(rows, neighbour_count(rows.shape[0], 30))
    p, _ = conditional_p_reference(score, 30)
    return symmetrize(idx, p.astype(np.float32), rows.shape[0])


@pytest.mark.parametrize("it", cases.SNAPSHOTS)
def test_gradient_along_the_references_trajectory(torch_mod, ctx, it):
    _check_gradient(torch_mod, ctx, cases.reference_fit().trajectory[it], _cluster_matrix(), f"iteration {it}")


@pytest.mark.parametrize("n", [17, 300, 1000])
def test_gradient_of_a_hand_made_matrix(torch_mod, ctx, n):
    """Row 0 empty, row 1 one entry, row 2 a hub of n - 1 entries, an entry that is 0, rows of 3 elsewhere; no symmetry."""
    rng = np.random.default_rng(n)
    cols = [np.zeros(0, np.int64), np.array([n - 1]), np.delete(np.arange(n), 2)]
    cols += [np.sort(rng.choice(np.delete(np.arange(n), i), 3, replace=False)) for i in range(3, n)]
    rowptr = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
    col = np.concatenate(cols).astype(np.int32)
    val = (rng.random(col.size) / col.size).astype(np.float32)
    val[rowptr[2] + 5] = 0.0
    assert rowptr[1] == 0 and rowptr[2] == 1 and rowptr[3] == n
    for kind in ("start", "duplicates"):
        _check_gradient(torch_mod, ctx, _map(n, kind), (rowptr, col, val), "hand-made " + kind)


# ---------------------------------------------------------------------------------------------------------------------- update
@pytest.mark.parametrize("n", [1, 255, 4099])
def test_update_equals_the_reference_bit_for_bit(torch_mod, ctx, n):
    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation.project import update_reference

    torch = torch_mod
    rng = np.random.default_rng(n)
    Y = rng.standard_normal((n, 2)).astype(np.float32)
    grad = (rng.standard_normal((n, 2)) * 10.0 ** rng.integers(-8, 1, (n, 2))).astype(np.float32)
    update = (rng.standard_normal((n, 2)) * 10.0 ** rng.integers(-6, 2, (n, 2))).astype(np.float32)
    gains = rng.uniform(0.01, 4.0, (n, 2)).astype(np.float32)
    for a, value in ((update, 0.0), (grad, 0.0), (gains, np.float32(0.01))):   # update * grad == 0 both ways, gains at the floor
        a.ravel()[rng.integers(0, 2 * n, max(1, n // 8))] = value
    prod = update * grad
    if n > 1:
        assert (prod < 0).any() and (prod > 0).any() and (prod == 0).any() and (gains == np.float32(0.01)).any()
    for lr, momentum in ((200.0, 0.5), (85.4, 0.8)):
        bufs = [torch.full((n + 2, 2), NAN_BITS, dtype=torch.int32, device="cuda") for _ in range(3)]
        for b, a in zip(bufs, (Y, update, gains)):
            b[1:n + 1] = torch.from_numpy(a.view(np.int32)).cuda()
        d_grad = torch.from_numpy(grad).cuda()
        _hip.check(ctx.lib.bn_tsne_update(ctx.handle, bufs[0][1:].data_ptr(), d_grad.data_ptr(), bufs[1][1:].data_ptr(), bufs[2][1:].data_ptr(), n, lr, momentum, None))
        torch.cuda.synchronize()
        assert np.array_equal(d_grad.cpu().numpy(), grad), "the gradient changed"
        for b, w, name in zip(bufs, update_reference(Y, grad, update, gains, lr, momentum), ("Y", "update", "gains")):
            h = b.cpu().numpy()
            assert (h[0] == NAN_BITS).all() and (h[n + 1] == NAN_BITS).all(), "a guard row was written"
            assert np.array_equal(h[1:n + 1].view(np.uint32), w.view(np.uint32)), (name, lr)


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refused_calls(torch_mod, ctx):
    from birdnet_stm32 import _hip

    torch = torch_mod
    n, k = 32, 8
    score = torch.full((n, k), 0.5, dtype=torch.float32, device="cuda")
    p = torch.full((n, k), 9.0, dtype=torch.float32, device="cuda")
    beta = torch.full((n,), 9.0, dtype=torch.float64, device="cuda")
    y = torch.full((n, 2), 0.25, dtype=torch.float32, device="cuda")
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    col = torch.zeros(4, dtype=torch.int32, device="cuda")
    val = torch.zeros(4, dtype=torch.float32, device="cuda")
    grad = torch.full((n, 2), 9.0, dtype=torch.float32, device="cuda")
    z = torch.full((1,), 9.0, dtype=torch.float64, device="cuda")
    kl = torch.full((n,), 9.0, dtype=torch.float64, device="cuda")
    upd = torch.full((n, 2), 9.0, dtype=torch.float32, device="cuda")
    gains = torch.full((n, 2), 9.0, dtype=torch.float32, device="cuda")
    ok = dict(score=score.data_ptr(), n=n, k=k, perplexity=2.0, p=p.data_ptr(), beta=beta.data_ptr(), y=y.data_ptr(), rowptr=rowptr.data_ptr(), col=col.data_ptr(),
              val=val.data_ptr(), E=1.0, grad=grad.data_ptr(), z=z.data_ptr(), kl=kl.data_ptr(), upd=upd.data_ptr(), gains=gains.data_ptr(), lr=100.0, momentum=0.5)

    def perplexity(**kw):
        a = dict(ok, **kw)
        return ctx.lib.bn_tsne_perplexity(ctx.handle, a["score"], a["n"], a["k"], a["perplexity"], a["p"], a["beta"], None)

    def gradient(**kw):
        a = dict(ok, **kw)
        return ctx.lib.bn_tsne_gradient(ctx.handle, a["y"], a["n"], a["rowptr"], a["col"], a["val"], a["E"], a["grad"], a["z"], a["kl"], None)

    def update(**kw):
        a = dict(ok, **kw)
        return ctx.lib.bn_tsne_update(ctx.handle, a["y"], a["grad"], a["upd"], a["gains"], a["n"], a["lr"], a["momentum"], None)

    for kw in (dict(n=0), dict(n=-1), dict(n=1 << 31), dict(k=0), dict(k=_hip.TSNE_MAX_K + 1), dict(perplexity=0.99), dict(perplexity=float("nan")),
               dict(perplexity=_hip.TSNE_MAX_K / 3 + 0.01), dict(score=None), dict(p=None), dict(beta=None), dict(score=score.data_ptr() + 2), dict(beta=beta.data_ptr() + 4)):
        assert perplexity(**kw) == BN_ERR_ARG and ctx.lib.bn_last_error(), kw
    for kw in (dict(n=1), dict(n=0), dict(n=-1), dict(n=_hip.TSNE_MAX_N + 1), dict(E=float("inf")), dict(E=float("nan")), dict(y=None), dict(rowptr=None), dict(col=None),
               dict(val=None), dict(grad=None), dict(z=None), dict(y=y.data_ptr() + 4), dict(grad=grad.data_ptr() + 4), dict(kl=kl.data_ptr() + 4), dict(col=col.data_ptr() + 2)):
        assert gradient(**kw) == BN_ERR_ARG and ctx.lib.bn_last_error(), kw
    for kw in (dict(n=0), dict(n=-1), dict(n=1 << 30), dict(lr=float("nan")), dict(momentum=float("inf")), dict(y=None), dict(grad=None), dict(upd=None), dict(gains=None),
               dict(upd=upd.data_ptr() + 2)):
        assert update(**kw) == BN_ERR_ARG and ctx.lib.bn_last_error(), kw
    torch.cuda.synchronize()
    for t, v in ((p, 9.0), (beta, 9.0), (grad, 9.0), (z, 9.0), (kl, 9.0), (upd, 9.0), (gains, 9.0), (y, 0.25), (score, 0.5)):
        assert bool((t == v).all()), "a refused call wrote to its outputs"
    assert gradient(kl=None) == 0 and perplexity() == 0   # the divergence's rows may be NULL
    torch.cuda.synchronize()
    assert bool((grad == 0.0).all()) and bool((kl == 9.0).all()) and float(z.item()) == n * (n - 1)   # one point 32 times: w = 1, no force
    assert bool((p == 0.125).all()) and bool(torch.isfinite(beta).all())


# ------------------------------------------------------------------------------------------------------------------- end to end
def _index(rows, zero_point=0, scale=1.0):
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    n = rows.shape[0]
    return EmbeddingIndex(rows, np.zeros(n, np.int64), 3.0 * np.arange(n), ["a.wav"], "int8" if rows.dtype == np.int8 else "float32", scale, zero_point)


@pytest.mark.parametrize("dtype", ["float32", "int8"])
def test_three_clusters_end_to_end(torch_mod, ctx, dtype):
    """500 iterations on the input the reference separates completely: at least 98 % of the points have their nearest map neighbour in
    their own cluster (the 2 % allow for the float32 trajectory; a condition, not a measurement), the divergence falls after the
    exaggeration ends, two runs give equal bits, and a zero row comes back NaN without moving any other point."""
    from birdnet_stm32.evaluation.project import project_index

    rows, zp = cases.three_clusters(), 0
    if dtype == "int8":   # the bytes of the same rows
        zp = -3
        rows = np.clip(np.rint(rows * 30.0) + zp, -128, 127).astype(np.int8)
    cluster = cases.cluster_of_rows()
    a = project_index(_index(rows, zp), n_iter=cases.ITERATIONS, kl_every=250, ctx=ctx)
    share = cases.same_cluster_share(a.xy, cluster)
    print(dtype, "share", share, "kl", a.kl_history)
    assert a.xy.shape == (300, 2) and a.xy.dtype == np.float32 and np.isfinite(a.xy).all() and a.n_iter == 500 and a.beta.shape == (300,)
    assert share >= 0.98
    assert [it for it, _ in a.kl_history] == [250, 500] and a.kl == a.kl_history[1][1] and a.kl_history[1][1] < a.kl_history[0][1]
    assert np.abs(a.xy.astype(np.float64).mean(axis=0)).max() <= 1e-5 * np.abs(a.xy).max()
    b = project_index(_index(rows, zp), n_iter=cases.ITERATIONS, kl_every=250, ctx=ctx)
    assert np.array_equal(a.xy.view(np.uint32), b.xy.view(np.uint32)) and a.kl_history == b.kl_history and np.array_equal(a.beta, b.beta)
    with_zero = np.insert(rows, 5, zp if dtype == "int8" else 0, axis=0)
    c = project_index(_index(with_zero, zp), n_iter=cases.ITERATIONS, ctx=ctx)
    assert c.xy.shape == (301, 2) and np.isnan(c.xy[5]).all() and np.isnan(c.beta[5])
    assert np.array_equal(np.delete(c.xy, 5, axis=0).view(np.uint32), a.xy.view(np.uint32)) and c.kl == a.kl


def test_project_index_refusals(torch_mod, ctx):
    from birdnet_stm32.evaluation.project import project_index

    x = np.zeros((5, 4), np.float32)
    x[0, 0] = 1
    with pytest.raises(ValueError, match="at least 2"):
        project_index(_index(x), perplexity=1, ctx=ctx)
    with pytest.raises(ValueError, match="below the number"):
        project_index(_index(cases.three_clusters()[:20]), perplexity=20, ctx=ctx)


def test_command_line(torch_mod, tmp_path):
    from birdnet_stm32.cli import project as project_cli

    rows = cases.three_clusters()[::5].copy()   # 60 rows, 20 of each cluster
    rows[7] = 0
    db = str(tmp_path / "db.npz")
    paths = np.asarray([f"clip{j}.wav" for j in range(6)])
    with open(db, "wb") as f:
        np.savez(f, embeddings=rows, file_index=np.arange(60) // 10, start_s=3.0 * (np.arange(60) % 10), paths=paths)
    out, npz = str(tmp_path / "map.csv"), str(tmp_path / "map.npz")
    res = project_cli.main(["--database", db, "--output", out, "--perplexity", "10", "--n_iter", "300", "--exaggeration_iter", "100", "--chunk_duration", "3",
                            "--npz_out", npz])
    with open(out, newline="") as f:
        lines = list(csv.reader(f))
    assert tuple(lines[0]) == project_cli.CSV_COLUMNS == ("path", "start_s", "end_s", "x", "y") and len(lines) == 61
    assert [r[0] for r in lines[1:]] == [f"clip{j // 10}.wav" for j in range(60)] and all(float(r[2]) == float(r[1]) + 3.0 for r in lines[1:])
    assert lines[8][3:] == ["", ""]
    xy = np.array([[float(r[3]), float(r[4])] for j, r in enumerate(lines[1:]) if j != 7])
    assert np.isfinite(xy).all() and np.allclose(xy, np.delete(res.xy, 7, axis=0), rtol=1e-6)
    with np.load(npz, allow_pickle=False) as z:
        assert np.array_equal(z["xy"], res.xy, equal_nan=True) and z["xy"].dtype == np.float32 and np.isnan(z["xy"][7]).all()
        assert z["paths"].tolist() == paths.tolist() and np.array_equal(z["file_index"], np.arange(60) // 10) and float(z["kl"]) == res.kl
    small = str(tmp_path / "small.npz")
    with open(small, "wb") as f:
        np.savez(f, embeddings=rows[:3], file_index=np.zeros(3, np.int64), start_s=np.zeros(3), paths=paths[:1])
    with pytest.raises(SystemExit, match="below the number"):
        project_cli.main(["--database", small, "--output", out])   # the default perplexity of 30 against 3 rows
