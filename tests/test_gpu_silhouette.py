"""GPU tests of the silhouette (csrc/bn_silhouette.hip, evaluation/silhouette.py, the flags of cli/cluster.py and cli/density.py) against
the numpy specification.

Equality tests use inputs on which the specification has one value whatever the summation order: rows and "sums" on the lattice
{0, 1/16, ..., 15/16}, INT8 bytes against lattice sums (every product and partial sum is exact in float32 for D <= 256), and weights that
are powers of two or zero.  Real-valued planted rows are held to written-out bounds (silhouette_cases.py): teacher-forced through the C
ABI — the float64 reference takes the float32 inverse norms, sums and weights the device was given — and end to end through
``silhouette_index``, where the rounding of the device's own sums joins the bound.  ``nearest`` must be equal on every row the float64
reference alone separates by more than the two bounds (at least 99 % of the live rows, computed before the device output is read)."""

import csv

import numpy as np
import pytest

import silhouette_cases as cases

pytestmark = pytest.mark.gpu

U = cases.U
NAN_BITS = 0x7FC0BEEF
FILL_NEAREST = -77


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


def _means(torch, ctx, rows, labels, sums, weight, zp=0, off=False):
    """bn_silhouette_means through the C ABI, the three outputs between guard rows of a fill pattern:
    (own float32, other float32, nearest int64, the device's inverse norms) on the host."""
    from birdnet_stm32 import _hip

    n, D = rows.shape
    K = sums.shape[0]
    labels, sums, weight = np.asarray(labels, np.int32), np.ascontiguousarray(sums, np.float32), np.ascontiguousarray(weight, np.float32)
    d_rows, d_inv = _inv_norms(torch, ctx, rows, zp, off)
    d_lab, d_sums, d_w = torch.from_numpy(labels).cuda(), torch.from_numpy(sums).cuda(), torch.from_numpy(weight).cuda()
    own = torch.full((n + 2,), NAN_BITS, dtype=torch.int32, device="cuda")
    other = torch.full((n + 2,), NAN_BITS, dtype=torch.int32, device="cuda")
    nearest = torch.full((n + 2,), FILL_NEAREST, dtype=torch.int32, device="cuda")
    code = _hip.DTYPE_I8 if rows.dtype == np.int8 else _hip.DTYPE_F32
    _hip.check(ctx.lib.bn_silhouette_means(ctx.handle, d_rows.data_ptr(), code, n, D, zp, d_inv.data_ptr(), d_lab.data_ptr(), d_sums.data_ptr(), d_w.data_ptr(), K,
                                           own[1:].data_ptr(), other[1:].data_ptr(), nearest[1:].data_ptr(), None))
    torch.cuda.synchronize()
    o, t, e = own.cpu().numpy(), other.cpu().numpy(), nearest.cpu().numpy()
    for a, fill in ((o, NAN_BITS), (t, NAN_BITS), (e, FILL_NEAREST)):
        assert a[0] == fill and a[n + 1] == fill, "a guard row was written"
    assert np.array_equal(d_rows.cpu().numpy(), rows) and np.array_equal(d_lab.cpu().numpy(), labels), "an input changed"
    assert np.array_equal(d_sums.cpu().numpy(), sums) and np.array_equal(d_w.cpu().numpy(), weight), "an input changed"
    return o[1:n + 1].view(np.float32), t[1:n + 1].view(np.float32), e[1:n + 1].astype(np.int64), d_inv.cpu().numpy()


def _tile(D, K):
    from birdnet_stm32 import _hip

    return _hip.kmeans_tile_centroids(D, K)


def _tile_crossing_k():
    """One sum more than an LDS tile holds at D = 256, from the header's constants."""
    from birdnet_stm32 import _hip

    tile = _hip.kmeans_tile_centroids(256, _hip.KMEANS_MAX_K)
    assert tile == min(_hip.KMEANS_MAX_TILE, _hip.KMEANS_LDS_BYTES // ((256 + 4) * 4) // 16 * 16)
    return tile + 1


# (N, D, K): one and several row tiles, ragged D, one sum tile and several, K = 1024 at D = 8 (eight tiles).  A fourth entry "off": the rows
# start one element behind a 16-byte boundary while D is a multiple of 16, so every chunk of every row takes the loader's slow path
SHAPES = [(2, 256, 2), (15, 96, 2), (17, 255, 15), (1000, 8, 16), (4099, 256, 17), (1000, 96, 100), (17, 8, 100), (1000, 256, "tile"), (1000, 8, 1024),
          (17, 256, 2, "off")]


def _shape(s):
    N, D, K = s[:3]
    return N, D, (_tile_crossing_k() if K == "tile" else K), len(s) > 3


def _shape_id(s):
    return "N{}-D{}-K{}".format(*s) + "-off" * (len(s) > 3)


def _lattice(N, D, K, seed, int8_zp=None):
    """Rows (lattice values, or int8 bytes over the full range), lattice sums, labels, and two sets of weights (powers of two and zeros).

    Sums: some are copies of others, with their weight (ties).  Labels: every cluster id, with -1, K and a cluster of weight 0 among them
    from N = 15 on.  Rows: two zero rows from N = 15 on.  Weights "mixed": about a quarter of the clusters are empty.  Weights "lonely":
    in the first LDS tile only the cluster of row 0 is non-empty (with a single tile: the only non-empty cluster at all, so its rows have
    no other cluster, and every other live row has just that one)."""
    rng = np.random.default_rng(seed)
    S = (rng.integers(0, 16, (K, D)) / 16.0).astype(np.float32)
    S[S.sum(axis=1) == 0, 0] = 0.5
    w = (2.0 ** -rng.integers(0, 7, K)).astype(np.float32)
    if K >= 3:
        w[rng.choice(K, max(1, K // 4), replace=False)] = 0
    dup_to, dup_from = rng.integers(0, K, max(1, K // 4)), rng.integers(0, K, max(1, K // 4))
    S[dup_to], w[dup_to] = S[dup_from], w[dup_from]   # duplicated sums with the same weight tie
    if not w.any():
        w[0] = 1.0
    if int8_zp is None:
        X = (rng.integers(0, 16, (N, D)) / 16.0).astype(np.float32)
        take = min(N, K, 8)
        X[:take] = S[rng.integers(0, K, take)]
        zero = 0.0
    else:
        X = rng.integers(-128, 128, (N, D)).astype(np.int8)
        zero = int8_zp
    lab = rng.integers(0, K, N)
    if N >= 15:
        X[[N // 2, N - 2]] = zero
        lab[[1, N // 3]] = -1
        lab[[2, N - 1]] = K
        if (w == 0).any():
            lab[3] = np.flatnonzero(w == 0)[0]
    tile = _tile(D, K)
    lonely = w.copy()
    lonely[:tile] = 0
    lonely[lab[0]] = 0.25   # (lab[0] is below K: the rows above leave row 0 alone)
    if lab[0] >= tile:
        lab[0] = 0
        lonely[0] = 0.25
    if K > tile and not lonely[tile:].any():
        lonely[K - 1] = 0.5
    return X, S, lab.astype(np.int64), {"mixed": w, "lonely": lonely}


def _check_exact(torch, ctx, shape, seed, zp=None):
    from birdnet_stm32.evaluation.silhouette import means_reference

    N, D, K, off = _shape(shape)
    X, S, lab, weights = _lattice(N, D, K, seed, zp)
    for name, w in weights.items():
        what = (shape, zp, name)
        own, other, nearest, inv = _means(torch, ctx, X, lab, S, w, zp or 0, off)
        want_own, want_other, want_nearest = means_reference(X, lab, S, w, zp or 0)
        live = (inv != 0) & (lab >= 0) & (lab < K)
        assert np.array_equal(nearest, want_nearest), f"{what}: nearest differs on {int((nearest != want_nearest).sum())} of {N} rows"
        assert np.array_equal(own.view(np.uint32), want_own.view(np.uint32)), f"{what}: own differs"
        assert np.array_equal(other.view(np.uint32), want_other.view(np.uint32)), f"{what}: other differs"
        assert (nearest[~live] == -1).all() and not own[~live].view(np.uint32).any() and not other[~live].view(np.uint32).any()
        assert (w[nearest[nearest >= 0]] != 0).all() and (nearest[live] != lab[live]).all()
        if N >= 15:
            assert (~live).sum() == 6, f"{what}: two zero rows, two labels -1, two labels K"
        if name == "mixed" and N >= 1000 and K >= 15:
            dup = {i for i in range(K) if w[i] != 0 and any(w[j] == w[i] and np.array_equal(S[i], S[j]) for j in range(i))}
            first = {i: min(j for j in range(K) if w[j] == w[i] and np.array_equal(S[i], S[j])) for i in dup}
            lose = np.isin(nearest, sorted(dup)) & (lab != np.array([first.get(int(c), -9) for c in nearest]))
            assert dup and not lose.any(), "a duplicated sum ties with its first copy and loses, unless that copy is the row's own cluster"
        if name == "lonely":
            tile = _tile(D, K)
            mine = live & (lab == lab[0])
            assert mine[0] and (w[:tile] != 0).sum() == 1
            if K <= tile:
                assert (nearest[mine] == -1).all() and not other[mine].view(np.uint32).any(), "no other non-empty cluster: other = 0, nearest = -1"
                assert (nearest[live & ~mine] == lab[0]).all()
            else:
                assert (nearest[mine] >= tile).all(), "the only candidates sit in later tiles"


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_means_of_lattice_rows_equal_the_reference_bit_for_bit(torch_mod, ctx, shape):
    N, D, K, _ = _shape(shape)
    _check_exact(torch_mod, ctx, shape, 11 + N + D + K)


@pytest.mark.parametrize("zp", [-128, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_means_of_int8_rows_equal_the_reference_bit_for_bit(torch_mod, ctx, shape, zp):
    N, D, K, _ = _shape(shape)
    _check_exact(torch_mod, ctx, shape, 2000 + N + D + K + zp, zp)


# ------------------------------------------------------------------------------------------------------------- mean-cosine bound
@pytest.mark.parametrize("int8", [False, True], ids=["f32", "i8"])
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_means_of_planted_rows_within_the_bound(torch_mod, ctx, shape, int8):
    """|own - own64| and |other - other64| <= (D + 3) 2^-24 sum_d |x_id| |S_cd| inv_i w_c, per element in float64 (silhouette_cases.py)."""
    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation.cluster import update_reference
    from birdnet_stm32.evaluation.silhouette import means_reference, weights_from_counts

    N, D, K, off = _shape(shape)
    rows, lab = cases.planted(N, D, K, seed=7, noise=0.5)
    zp = 0
    if int8:
        rows, zp = cases.quantised(rows, 5), 5
    S, counts = update_reference(rows, lab, K, zp)   # the float32 sums the device is given
    w = weights_from_counts(counts)
    d_rows, d_inv = _inv_norms(torch_mod, ctx, rows, zp)
    inv = d_inv.cpu().numpy()
    bound = cases.mean_cosine_bound(rows, zp, inv, S, w)
    _, cand = cases.candidate_means(rows, zp, inv, S, w, lab)
    sep = cases.separated_rows(cand, bound, lab)
    own64, other64, near64 = means_reference(rows, lab, S, w, zp, np.float64, inv)
    print(f"{shape}: the float64 reference separates {sep.mean():.4f} of the rows")
    assert sep.mean() >= 0.99
    own, other, nearest, inv_again = _means(torch_mod, ctx, rows, lab, S, w, zp, off)
    assert np.array_equal(inv_again, inv)
    r = np.arange(N)
    e_own = np.abs(own - own64) / bound[r, lab]
    has = near64 >= 0
    cand_bound = np.where(np.isfinite(cand), bound, 0).max(axis=1)
    e_other = np.abs(other - other64)[has] / cand_bound[has]
    print(f"{shape}: own at {e_own.max():.3f} of its bound, other at {e_other.max() if has.any() else 0:.3f}")
    assert (np.abs(own - own64) <= bound[r, lab]).all()
    assert (np.abs(other - other64) <= cand_bound).all()
    assert (np.abs(other - other64)[sep & has] <= bound[r, near64][sep & has]).all()
    assert np.array_equal(nearest[sep], near64[sep])
    assert (nearest >= 0).all() and (nearest != lab).all()


# ------------------------------------------------------------------------------------------------------------------- end to end
def _index(rows, zero_point=0, **kw):
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    n = rows.shape[0]
    return EmbeddingIndex(rows, np.zeros(n, np.int64), np.arange(n, dtype=np.float64), ["a.wav"], zero_point=zero_point, **kw)


def _end_to_end_bounds(rows, zp, lab, K, blocks):
    """Float64 quantities of the end-to-end bound: E[i, c] = (D + 256 + ceil(n_c / 256) + 8 + (blocks - 1)) u sum_d |x^_id| sum_{j in c}
    |x^_jd| / n_c — the device's sums add segments of at most 256 members one after the other and fold them in order, one more fold per
    further block, on top of the mean cosine's own (D + 3) u and the roundings of the inverse norms and the weight."""
    x = cases.as_float64(rows, zp)
    xn = np.abs(x / np.linalg.norm(x, axis=1, keepdims=True))
    A = np.zeros((K, rows.shape[1]))
    np.add.at(A, lab, xn)
    n = np.bincount(lab, minlength=K).astype(np.float64)
    factor = rows.shape[1] + 256 + np.ceil(n / cases.SEGMENT_ROWS) + 8 + (blocks - 1)
    return (xn @ A.T) * (factor * U / np.maximum(n, 1))[None, :]


@pytest.mark.parametrize("streamed", [False, True], ids=["resident", "streamed"])
@pytest.mark.parametrize("int8", [False, True], ids=["f32", "i8"])
@pytest.mark.parametrize("N, D, K", [(1000, 96, 100), (4099, 255, 17)])
def test_silhouette_index_within_the_end_to_end_bound(torch_mod, ctx, N, D, K, int8, streamed):
    from birdnet_stm32.evaluation.silhouette import silhouette_index, silhouette_reference

    rows, lab = cases.planted(N, D, K, seed=7, noise=0.5)
    zp = 0
    if int8:
        rows, zp = cases.quantised(rows, 5), 5
    index = _index(rows, zp, budget_bytes=-(-N // 3) * D * rows.itemsize) if streamed else _index(rows, zp)
    blocks = len(index.block_ranges())
    assert blocks >= 3 if streamed else blocks == 1
    want = silhouette_reference(rows, lab, K, zp, dtype=np.float64)
    E = _end_to_end_bounds(rows, zp, lab, K, blocks)
    assert E.max() <= 3.1e-5
    r = np.arange(N)
    n_a = want.counts[lab].astype(np.float64)
    a = (1.0 - want.own) * n_a / np.maximum(n_a - 1, 1)
    b = 1.0 - want.other
    top = np.maximum(a, b)
    keep = top >= 0.05
    assert keep.mean() >= 0.99
    d_own = E[r, lab]
    E_other = E.copy()
    E_other[r, lab] = 0
    d_other = E_other.max(axis=1)
    d_s = (d_own * n_a / np.maximum(n_a - 1, 1) + d_other) * 2 / top

    got = silhouette_index(index, lab, K, ctx=ctx)
    assert (index._resident is None) == streamed, "a resident block is left behind, a streamed index leaves none"
    assert np.array_equal(got.counts, want.counts) and got.n_live == N
    print(f"own {np.abs(got.own - want.own).max():.3g} (bound up to {d_own.max():.3g}), other {np.abs(got.other - want.other).max():.3g}, "
          f"silhouette {np.abs(got.silhouette - want.silhouette)[keep].max():.3g} (bound up to {d_s[keep].max():.3g})")
    assert (np.abs(got.own - want.own) <= d_own).all()
    assert (np.abs(got.other - want.other) <= d_other).all()
    assert (np.abs(got.silhouette - want.silhouette)[keep] <= d_s[keep]).all()
    single = n_a == 1
    assert (got.silhouette[single] == 0).all()
    assert abs(got.mean - want.mean) <= d_s[keep].max() and np.abs(got.cluster_mean - want.cluster_mean).max() <= d_s[keep].max() + (~keep).mean()
    again = silhouette_index(index, lab, K, ctx=ctx)
    assert np.array_equal(again.silhouette, got.silhouette) and np.array_equal(again.nearest, got.nearest)


def test_silhouette_index_leaves_noise_and_zero_rows_out(torch_mod, ctx):
    from birdnet_stm32.evaluation.silhouette import silhouette_index, silhouette_reference

    rows, lab = cases.planted(300, 8, 3, seed=7, noise=0.5)
    rows[[5, 17]] = 0
    lab[[7, 100]] = -1
    lab[200] = 3
    got = silhouette_index(_index(rows), lab, 3, ctx=ctx)
    want = silhouette_reference(rows, lab, 3, dtype=np.float64)
    dead = [5, 7, 17, 100, 200]
    assert np.isnan(got.silhouette[dead]).all() and (got.nearest[dead] == -1).all() and got.n_live == 295
    assert np.array_equal(got.counts, want.counts) and np.array_equal(np.isnan(got.silhouette), np.isnan(want.silhouette))
    live = ~np.isnan(want.silhouette)
    assert np.abs(got.silhouette - want.silhouette)[live].max() <= 1e-4 and np.array_equal(got.nearest, want.nearest)
    with pytest.raises(ValueError, match="2 non-empty"):
        silhouette_index(_index(rows), np.where(lab == 0, 0, -1), 3, ctx=ctx)
    with pytest.raises(ValueError, match="labels"):
        silhouette_index(_index(rows), lab[:-1], 3, ctx=ctx)


# ------------------------------------------------------------------------------------------------- same bits, guards, refusals
def test_library_names_the_silhouette_kernel(ctx):
    from birdnet_stm32 import _hip

    assert "bn_silhouette_means" in _hip.EXPORTS
    assert "silhouette_means_kernel" in ctx.lib.bn_kernel_names().decode().split("\n")


def test_two_calls_give_the_same_bits(torch_mod, ctx):
    from birdnet_stm32.evaluation.cluster import update_reference
    from birdnet_stm32.evaluation.silhouette import weights_from_counts

    K = _tile_crossing_k()
    rows, lab = cases.planted(1000, 256, K, seed=7, noise=0.5)
    S, counts = update_reference(rows, lab, K)
    w = weights_from_counts(counts)
    first = _means(torch_mod, ctx, rows, lab, S, w)
    second = _means(torch_mod, ctx, rows, lab, S, w)
    for a, b in zip(first[:3], second[:3]):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def test_refused_calls(torch_mod, ctx):
    from birdnet_stm32 import _hip

    torch = torch_mod
    rows = torch.zeros((32, 16), dtype=torch.float32, device="cuda")
    inv = torch.ones(32, dtype=torch.float32, device="cuda")
    label = torch.zeros(32, dtype=torch.int32, device="cuda")
    sums = torch.ones((4, 16), dtype=torch.float32, device="cuda")
    weight = torch.ones(4, dtype=torch.float32, device="cuda")
    own = torch.full((32,), NAN_BITS, dtype=torch.int32, device="cuda")
    other = torch.full((32,), NAN_BITS, dtype=torch.int32, device="cuda")
    nearest = torch.full((32,), FILL_NEAREST, dtype=torch.int32, device="cuda")
    ok = dict(rows=rows.data_ptr(), dtype=_hip.DTYPE_F32, n=32, D=16, zp=0, inv=inv.data_ptr(), label=label.data_ptr(), sums=sums.data_ptr(), weight=weight.data_ptr(),
              K=4, own=own.data_ptr(), other=other.data_ptr(), nearest=nearest.data_ptr())

    def call(**kw):
        a = dict(ok, **kw)
        return ctx.lib.bn_silhouette_means(ctx.handle, a["rows"], a["dtype"], a["n"], a["D"], a["zp"], a["inv"], a["label"], a["sums"], a["weight"], a["K"], a["own"],
                                           a["other"], a["nearest"], None)

    for kw in [dict(K=0), dict(K=_hip.KMEANS_MAX_K + 1), dict(D=0), dict(D=_hip.KMEANS_MAX_D + 1), dict(n=-1), dict(own=None), dict(other=None), dict(nearest=None),
               dict(rows=None), dict(inv=None), dict(label=None), dict(sums=None), dict(weight=None), dict(dtype=7), dict(rows=rows.data_ptr() + 2),
               dict(dtype=_hip.DTYPE_I8, zp=128)]:
        assert call(**kw) == -1, f"{kw} should be refused with BN_ERR_ARG"
    torch.cuda.synchronize()
    assert bool((own == NAN_BITS).all()) and bool((other == NAN_BITS).all()) and bool((nearest == FILL_NEAREST).all()), "a refused call wrote to its outputs"
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((own == NAN_BITS).all()) and bool((nearest == FILL_NEAREST).all()), "no rows, nothing written"
    assert call() == 0
    torch.cuda.synchronize()
    # every mean is 0 (the rows hold zeros; the inverse norms handed in are ones, so they count as rows): cluster 1 is the lowest other index
    assert bool((nearest == 1).all()) and not bool(own.any()) and not bool(other.any())


# --------------------------------------------------------------------------------------------------------------------- commands
def _archive(path, int8=False):
    rows, lab = cases.planted(240, 32, 3, seed=0, noise=0.5)
    rows = np.concatenate([rows, np.zeros((2, 32), np.float32)])
    keys = dict(file_index=np.arange(242) // 61, start_s=(np.arange(242) % 61) * 3.0, paths=np.asarray([f"rec_{i}.wav" for i in range(4)]))
    if int8:
        keys.update(embeddings=cases.quantised(rows, 5), scale=np.float32(0.01), zero_point=np.int64(5))
        keys["embeddings"][240:] = 5
    else:
        keys.update(embeddings=rows)
    with open(path, "wb") as f:
        np.savez(f, **keys)
    return lab


def _read(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_cluster_sweep_chooses_the_planted_three_and_writes_its_files(torch_mod, tmp_path, capsys):
    import birdnet_stm32.cli.cluster as cli
    from birdnet_stm32.evaluation.search import EmbeddingIndex
    from birdnet_stm32.evaluation.silhouette import silhouette_index

    db, out = str(tmp_path / "db.npz"), str(tmp_path / "c.csv")
    planted = _archive(db)
    res = cli.main(["--database", db, "--k", "2", "--k_sweep", "3", "4", "5", "6", "--n_init", "2", "--output", out, "--chunk_duration", "3",
                    "--centroids_out", str(tmp_path / "cent.npz"), "--exemplars", "2"])
    said = capsys.readouterr().out
    assert res.centroids.shape[0] == 3 and "Chose k = 3" in said and "mean silhouette" in said
    sweep = _read(str(tmp_path / "c_sweep.csv"))
    assert len(sweep) == 6 and tuple(sweep[0]) == cli.SWEEP_COLUMNS and [int(r[0]) for r in sweep[1:]] == [2, 3, 4, 5, 6]
    sil = [float(r[1]) for r in sweep[1:]]
    assert max(sil) == sil[1] > 0.7 and all(s < 0.65 for i, s in enumerate(sil) if i != 1)
    assert all(int(r[5]) <= int(r[6]) for r in sweep[1:])
    rows = _read(out)
    assert tuple(rows[0]) == cli.CSV_COLUMNS + cli.SILHOUETTE_COLUMNS and len(rows) == 243
    labels = np.array([int(r[3]) for r in rows[1:]])
    assert (labels[240:] == -1).all() and [r[5:] for r in rows[241:]] == [["", "-1"], ["", "-1"]]
    same = np.array([len(set(labels[:240][planted == c])) for c in range(3)])
    assert (same == 1).all() and len(set(labels[:240])) == 3, "the planted clusters are found"
    index = EmbeddingIndex.from_npz(db)
    want = silhouette_index(index, labels, 3)
    index.close()
    assert [r[5] for r in rows[1:241]] == [f"{s:.7g}" for s in want.silhouette[:240]]
    assert [int(r[6]) for r in rows[1:]] == list(want.nearest)
    summary = _read(str(tmp_path / "c_summary.csv"))
    assert summary[0] == ["cluster", "count", "mean_score", "silhouette", "exemplar_1", "exemplar_2"] and len(summary) == 4
    assert [r[3] for r in summary[1:]] == [f"{m:.7g}" for m in want.cluster_mean]
    assert np.load(str(tmp_path / "cent.npz"))["embeddings"].shape == (3, 32)
    with pytest.raises(SystemExit, match="k_sweep"):
        cli.main(["--database", db, "--k", "1", "--k_sweep", "2", "--output", out])


def test_cluster_without_the_flags_writes_the_same_bytes_and_the_flag_only_appends(torch_mod, tmp_path):
    import birdnet_stm32.cli.cluster as cli
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    db, out, flagged = str(tmp_path / "db.npz"), str(tmp_path / "c.csv"), str(tmp_path / "s.csv")
    _archive(db)
    res = cli.main(["--database", db, "--k", "3", "--output", out, "--chunk_duration", "3", "--exemplars", "2"])
    index = EmbeddingIndex.from_npz(db)
    cli.write_clusters_csv(str(tmp_path / "w.csv"), index, res, 3.0)
    cli.write_summary_csv(str(tmp_path / "w_summary.csv"), index, res)
    index.close()
    plain, plain_summary = open(out, "rb").read(), open(str(tmp_path / "c_summary.csv"), "rb").read()
    assert plain == open(str(tmp_path / "w.csv"), "rb").read() and plain_summary == open(str(tmp_path / "w_summary.csv"), "rb").read()
    assert plain.splitlines()[0] == b"path,start_s,end_s,cluster,score" and plain_summary.splitlines()[0] == b"cluster,count,mean_score,exemplar_1,exemplar_2"
    assert not (tmp_path / "c_sweep.csv").exists()
    cli.main(["--database", db, "--k", "3", "--output", flagged, "--chunk_duration", "3", "--exemplars", "2", "--silhouette"])
    assert [r[:5] for r in _read(flagged)] == _read(out), "the flag appends columns and changes nothing else"
    assert [r[:3] + r[4:] for r in _read(str(tmp_path / "s_summary.csv"))] == _read(str(tmp_path / "c_summary.csv"))
    assert not (tmp_path / "s_sweep.csv").exists()


def test_density_with_the_flag_and_an_int8_archive(torch_mod, tmp_path):
    import birdnet_stm32.cli.cluster as cli
    import birdnet_stm32.cli.density as dcli

    db, db8 = str(tmp_path / "db.npz"), str(tmp_path / "db8.npz")
    _archive(db)
    _archive(db8, int8=True)
    out = str(tmp_path / "d.csv")
    res = dcli.main(["--database", db, "--output", out, "--silhouette"])
    rows = _read(out)
    assert tuple(rows[0]) == cli.CSV_COLUMNS + cli.SILHOUETTE_COLUMNS and res.n_clusters >= 2
    noise = res.labels < 0
    assert noise[240:].all()
    assert all((r[5] == "") == bool(n) and (r[6] == "-1") == bool(n) for r, n in zip(rows[1:], noise))
    summary = _read(str(tmp_path / "d_summary.csv"))
    assert summary[0][:4] == ["cluster", "count", "stability", "silhouette"] and all(float(r[3]) > 0.5 for r in summary[1:])
    plain = str(tmp_path / "p.csv")
    dcli.main(["--database", db, "--output", plain])
    assert [r[:5] for r in rows] == _read(plain)
    with pytest.raises(SystemExit, match="at least 2 clusters"):
        dcli.main(["--database", db, "--output", out, "--silhouette", "--min_cluster_size", "100", "--min_samples", "15"])
    out8 = str(tmp_path / "c8.csv")
    res8 = cli.main(["--database", db8, "--k", "2", "--k_sweep", "3", "4", "--n_init", "2", "--output", out8, "--exemplars", "0"])
    rows8 = _read(out8)
    assert res8.centroids.shape[0] == 3 and tuple(rows8[0]) == cli.CSV_COLUMNS + cli.SILHOUETTE_COLUMNS
    assert [r[5:] for r in rows8[241:]] == [["", "-1"], ["", "-1"]] and all(r[5] != "" for r in rows8[1:241])
