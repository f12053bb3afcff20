"""GPU tests of reduction (csrc/bn_pca.hip, evaluation/reduce.py, cli/reduce.py, project's PCA start) against the numpy specification.

The error bounds are counted from the kernels' code, with u = 2^-24 and v = 2^-53:

  bn_pca_colsum     every value passes through at most n float64 additions (a lane's chain over its rows, the groups of a workgroup, the
                    workgroups): |sum - ref| <= n v sum_i |x_id|.  Integers (int8, lattice rows) are exact: every partial sum is an integer
                    below 2^53.
  bn_pca_gram       c_i = fl32(x_i - mean) is the reference's own operand.  Within a run of BN_PCA_RUN_ROWS rows the products enter a
                    float32 accumulator of the matrix cores: at most RUN_ROWS roundings on a term's way, then exact conversion to float64
                    and float64 additions (below u for any n < 2^29): |G - ref| <= (RUN_ROWS + 1) u sum_i |c_ia c_ib|
                    (``gram_entry_bound``).  Integer operands are exact while a run's sum of |products| stays below 2^24: int8 at any
                    magnitude (256 * 255^2 < 2^24), lattice rows here (256 * 8^2).
  bn_pca_transform  one fused float32 chain of the matrix cores over d ascending, zeros beyond D: at most D roundings on a term's way, one
                    for the float32 result of the reference, one spare: |y - ref| <= (D + 2) u sum_d |W_kd c_id| (``transform_bound``).
"""

import csv

import numpy as np
import pytest

import reduce_cases as cases

pytestmark = pytest.mark.gpu

U, V = 2.0 ** -24, 2.0 ** -53
NAN64_BITS = 0x7FF80000DEADBEEF
NAN_BITS = 0x7FC0BEEF
BN_ERR_ARG = -1
F32, I8 = 0, 1


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


def test_library_names_the_pca_kernels(ctx):
    names = ctx.lib.bn_kernel_names().decode().split("\n")
    assert {"pca_colsum_kernel", "pca_colsum_fold_kernel", "pca_gram_kernel", "pca_gram_fold_kernel", "pca_transform_kernel"} <= set(names)


# --------------------------------------------------------------------------------------------------------------------- helpers
def _dev_rows(torch, rows, offset=0):
    """The rows on the device, ``offset`` bytes behind a 256-byte boundary: ``(owner, address)``."""
    raw = torch.zeros(rows.nbytes + 64, dtype=torch.uint8, device="cuda")
    if rows.nbytes:
        raw[offset:offset + rows.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1)))
    assert raw.data_ptr() % 256 == 0
    return raw, raw.data_ptr() + offset


def _code(rows):
    return I8 if rows.dtype == np.int8 else F32


def _f64_out(torch, elems):
    """``elems`` float64 behind and in front of a guard value."""
    return torch.full((elems + 2,), NAN64_BITS, dtype=torch.int64, device="cuda")


def _f64_read(buf, elems):
    h = buf.cpu().numpy()
    assert h[0] == NAN64_BITS and h[elems + 1] == NAN64_BITS, "a guard value was written"
    return h[1:elems + 1].view(np.float64)


def _colsum(torch, ctx, rows, zp=0, offset=0):
    n, D = rows.shape
    owner, ptr = _dev_rows(torch, rows, offset)
    out = _f64_out(torch, D)
    rc = ctx.lib.bn_pca_colsum(ctx.handle, ptr, _code(rows), n, D, zp, out[1:].data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, ctx.lib.bn_last_error()
    return _f64_read(out, D)


def _gram(torch, ctx, rows, zp=0, mean=None, offset=0, expect=0):
    n, D = rows.shape
    owner, ptr = _dev_rows(torch, rows, offset)
    out = _f64_out(torch, D * D)
    d_mean = None if mean is None else torch.from_numpy(np.ascontiguousarray(mean, np.float32)).cuda()
    rc = ctx.lib.bn_pca_gram(ctx.handle, ptr, _code(rows), n, D, zp, None if d_mean is None else d_mean.data_ptr(), out[1:].data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == expect, ctx.lib.bn_last_error()
    if rc:
        assert (out.cpu().numpy() == NAN64_BITS).all(), "a refused call wrote"
        return None
    return _f64_read(out, D * D).reshape(D, D)


def _transform(torch, ctx, rows, W, zp=0, mean=None, offset=0):
    n, D = rows.shape
    r = W.shape[0]
    owner, ptr = _dev_rows(torch, rows, offset)
    out = torch.full(((n + 2) * r,), NAN_BITS, dtype=torch.int32, device="cuda")
    d_mean = None if mean is None else torch.from_numpy(np.ascontiguousarray(mean, np.float32)).cuda()
    d_W = torch.from_numpy(np.ascontiguousarray(W, np.float32)).cuda()
    rc = ctx.lib.bn_pca_transform(ctx.handle, ptr, _code(rows), n, D, zp, None if d_mean is None else d_mean.data_ptr(), d_W.data_ptr(), r, out[r:].data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, ctx.lib.bn_last_error()
    h = out.cpu().numpy().reshape(n + 2, r)
    assert (h[0] == NAN_BITS).all() and (h[n + 1] == NAN_BITS).all(), "a guard row was written"
    return h[1:n + 1].view(np.float32)


def _centred(rows, mean, zp):
    from birdnet_stm32.evaluation.reduce import centred

    return centred(rows, np.zeros(rows.shape[1], np.float32) if mean is None else mean, zp)


# ------------------------------------------------------------------------------------------------------------------ column sums
COLSUM_SHAPES = [(0, 16), (1, 1), (63, 3), (64, 17), (65, 64), (257, 100), (1000, 256), (4097, 260), (4097, 1), (1000, 16), (64, 260), (257, 3)]


@pytest.mark.parametrize("n,D", COLSUM_SHAPES)
def test_colsum(torch_mod, ctx, n, D):
    """int8 with three zero points and float32 lattice rows: the exact integer sums; real-valued rows: within n v sum|x|."""
    b = cases.int8_rows(n, D, 10 * n + D)
    for zp in (-128, 0, 5):
        want = (b.astype(np.int64) - zp).sum(axis=0)
        assert np.array_equal(_colsum(torch_mod, ctx, b, zp, offset=n % 2), want.astype(np.float64)), zp
    lat = cases.lattice_rows(n, D, n + D, mean=3)
    assert np.array_equal(_colsum(torch_mod, ctx, lat, offset=4 * (D % 2)), lat.astype(np.float64).sum(axis=0))
    x = cases.real_rows(n, D, n + 7 * D)
    got = _colsum(torch_mod, ctx, x)
    x64 = x.astype(np.float64)
    bound = n * V * np.abs(x64).sum(axis=0)
    err = np.abs(got - x64.sum(axis=0))
    print(f"colsum n={n} D={D}: largest share of the bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------------------------- scatter matrix
def _int_gram(b, zp):
    x = b.astype(np.int64) - zp
    return (x.T @ x).astype(np.float64)


@pytest.mark.parametrize("n,D,zp,kind,offset", [
    (300, 17, 127, "extreme", 0),      # every byte at magnitude 255 across a run boundary: 256 * 255^2 per run
    (300, 64, 127, "extreme", 0),      # the same through the wide loads
    (1000, 100, 5, "mixed", 0),
    (257, 260, 0, "mixed", 1),         # unaligned row starts, five macro tiles
    (4097, 256, -128, "mixed", 0),     # wide loads, several row ranges
    (65, 64, 0, "mixed", 0),
    (1, 3, -7, "mixed", 0),
    (0, 16, 0, "mixed", 0),
])
def test_gram_int8_is_the_exact_integer_matrix(torch_mod, ctx, n, D, zp, kind, offset):
    b = np.full((n, D), -128, np.int8) if kind == "extreme" else cases.int8_rows(n, D, n + D)
    got = _gram(torch_mod, ctx, b, zp, offset=offset)
    assert np.array_equal(got, _int_gram(b, zp))
    assert np.array_equal(got.view(np.uint64), got.T.view(np.uint64))


def test_gram_int8_refuses_a_mean(torch_mod, ctx):
    b = cases.int8_rows(64, 16, 1)
    assert _gram(torch_mod, ctx, b, 0, mean=np.zeros(16, np.float32), expect=BN_ERR_ARG) is None


GRAM_SHAPES = [(1, 3, 0), (64, 64, 0), (65, 100, 0), (300, 17, 4), (257, 256, 0), (1000, 40, 0), (4097, 260, 4), (2049, 130, 8)]


@pytest.mark.parametrize("n,D,offset", GRAM_SHAPES)
def test_gram_float32(torch_mod, ctx, n, D, offset):
    """Lattice rows with an integer mean are exact; real-valued rows stay within the entry bound against the float64 product of the same
    centred float32 rows; the matrix is symmetric bit for bit and a second run gives the same bits; so does a NULL mean against a zero mean."""
    from birdnet_stm32.evaluation.reduce import gram_entry_bound

    lat, mean = cases.lattice_rows(n, D, n + D, mean=5), np.full(D, 5, np.float32)
    c = _centred(lat, mean, 0).astype(np.float64)
    assert np.array_equal(_gram(torch_mod, ctx, lat, mean=mean, offset=offset), c.T @ c)
    x = cases.real_rows(n, D, 3 * n + D)
    mean = (x.astype(np.float64).sum(axis=0) / n).astype(np.float32)
    got = _gram(torch_mod, ctx, x, mean=mean, offset=offset)
    c = _centred(x, mean, 0)
    c64 = c.astype(np.float64)
    err, bound = np.abs(got - c64.T @ c64), gram_entry_bound(c)
    print(f"gram n={n} D={D}: largest share of the bound {float((err / np.maximum(bound, 1e-300)).max()):.4f}")
    assert (err <= bound).all()
    assert np.array_equal(got.view(np.uint64), got.T.view(np.uint64))
    assert np.array_equal(got.view(np.uint64), _gram(torch_mod, ctx, x, mean=mean, offset=offset).view(np.uint64))
    raw = _gram(torch_mod, ctx, x, offset=offset)
    assert np.array_equal(raw.view(np.uint64), _gram(torch_mod, ctx, x, mean=np.zeros(D, np.float32), offset=offset).view(np.uint64))
    x64 = x.astype(np.float64)
    assert (np.abs(raw - x64.T @ x64) <= gram_entry_bound(x)).all()


# -------------------------------------------------------------------------------------------------------------------- transform
TRANSFORM_SHAPES = [(3, 1, 63), (3, 2, 1), (64, 1, 65), (64, 16, 257), (64, 17, 63), (64, 64, 1000), (100, 2, 257), (100, 17, 65), (100, 64, 63),
                    (256, 16, 1000), (256, 64, 65), (256, 130, 257)]


@pytest.mark.parametrize("D,r,n", TRANSFORM_SHAPES)
def test_transform(torch_mod, ctx, D, r, n):
    """Integer W, mean and rows are exact; real-valued inputs stay within the bound; NULL mean; int8 rows with a mean; unaligned rows."""
    from birdnet_stm32.evaluation.reduce import transform_bound

    rng = np.random.default_rng(1000 * D + 10 * r + n)
    lat, mean = cases.lattice_rows(n, D, n + D + r, mean=2), np.full(D, 2, np.float32)
    Wi = rng.integers(-4, 5, (r, D)).astype(np.float32)
    assert np.array_equal(_transform(torch_mod, ctx, lat, Wi, mean=mean, offset=4 * (n % 2)), (_centred(lat, mean, 0).astype(np.float64) @ Wi.T.astype(np.float64)).astype(np.float32))
    x = cases.real_rows(n, D, n + 3 * D + r)
    W = (rng.standard_normal((r, D)) / np.sqrt(D)).astype(np.float32)
    worst = 0.0
    for mean, offset in ((x.mean(axis=0).astype(np.float32), 0), (None, 4)):
        got = _transform(torch_mod, ctx, x, W, mean=mean, offset=offset)
        c = _centred(x, mean, 0)
        err, bound = np.abs(got.astype(np.float64) - c.astype(np.float64) @ W.astype(np.float64).T), transform_bound(c, W)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
    b, zp = cases.int8_rows(n, D, n + D), 5
    mean = ((b.astype(np.float64) - zp).mean(axis=0)).astype(np.float32)
    got = _transform(torch_mod, ctx, b, W, zp=zp, mean=mean, offset=n % 2)
    c = _centred(b, mean, zp)
    err, bound = np.abs(got.astype(np.float64) - c.astype(np.float64) @ W.astype(np.float64).T), transform_bound(c, W)
    worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"transform D={D} r={r} n={n}: largest share of the bound {worst:.4f}")
    assert (err <= bound).all()
    assert np.array_equal(_transform(torch_mod, ctx, b, Wi, zp=zp), ((b.astype(np.float64) - zp) @ Wi.T.astype(np.float64)).astype(np.float32))


def test_refusals_write_nothing(torch_mod, ctx):
    torch = torch_mod
    x = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    out = _f64_out(torch, 64)
    lib, h = ctx.lib, ctx.handle
    assert lib.bn_pca_colsum(h, x.data_ptr(), F32, 4, 0, 0, out[1:].data_ptr(), None) == BN_ERR_ARG
    assert lib.bn_pca_colsum(h, x.data_ptr(), F32, 4, 2049, 0, out[1:].data_ptr(), None) == BN_ERR_ARG
    assert lib.bn_pca_colsum(h, x.data_ptr(), 7, 4, 8, 0, out[1:].data_ptr(), None) == BN_ERR_ARG
    assert lib.bn_pca_colsum(h, x.data_ptr(), F32, -1, 8, 0, out[1:].data_ptr(), None) == BN_ERR_ARG
    assert lib.bn_pca_colsum(h, x.data_ptr() + 2, F32, 2, 8, 0, out[1:].data_ptr(), None) == BN_ERR_ARG
    assert lib.bn_pca_gram(h, x.data_ptr(), F32, 4, 8, 0, None, None, None) == BN_ERR_ARG
    assert lib.bn_pca_gram(h, x.data_ptr(), F32, 4, 8, 0, None, out[1:].data_ptr() + 4, None) == BN_ERR_ARG
    w = torch.zeros((8, 8), dtype=torch.float32, device="cuda")
    y = torch.full((4, 9), NAN_BITS, dtype=torch.int32, device="cuda")
    assert lib.bn_pca_transform(h, x.data_ptr(), F32, 4, 8, 0, None, w.data_ptr(), 0, y.data_ptr(), None) == BN_ERR_ARG
    assert lib.bn_pca_transform(h, x.data_ptr(), F32, 4, 8, 0, None, w.data_ptr(), 9, y.data_ptr(), None) == BN_ERR_ARG
    assert lib.bn_pca_transform(h, x.data_ptr(), F32, 4, 8, 0, None, None, 2, y.data_ptr(), None) == BN_ERR_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == NAN64_BITS).all() and (y.cpu().numpy() == NAN_BITS).all()


# ------------------------------------------------------------------------------------------------------------------- whole fits
def _index(rows, zero_point=0, scale=1.0, budget_bytes=2 << 30):
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    n = rows.shape[0]
    return EmbeddingIndex(rows, np.zeros(n, np.int64), 3.0 * np.arange(n), ["a.wav"], "int8" if rows.dtype == np.int8 else "float32", scale, zero_point,
                          budget_bytes=budget_bytes)


def _same_model(a, b):
    for name in ("mean", "components", "weights", "explained_variance"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name
    assert (a.total_variance, a.n_rows, a.whiten, a.dtype, a.scale, a.zero_point) == (b.total_variance, b.n_rows, b.whiten, b.dtype, b.scale, b.zero_point)


@pytest.mark.parametrize("whiten", [False, True])
def test_int8_fit_equals_the_reference_bit_for_bit(torch_mod, ctx, whiten):
    """The device part is exact and the host part is shared: every field of the model is the reference's, from one block and from several."""
    from birdnet_stm32.evaluation.reduce import fit_pca, pca_reference, transform_bound, transform_index, centred

    scale, zp = 0.11, -100
    b = cases.int8_features(700, 48, 5, scale, zp)
    b[[3, 500]] = zp   # zero rows
    want, scores = pca_reference(b, zp, scale, 6, whiten)
    for budget in (2 << 30, 300 * 48):
        idx = _index(b, zp, scale, budget)
        assert len(idx.block_ranges()) == (1 if budget > 1 << 20 else 3)
        got = fit_pca(idx, 6, whiten, ctx=ctx)
        _same_model(got, want)
        y = transform_index(idx, got, ctx=ctx)
        assert y.shape == (700, 6) and y.dtype == np.float32 and not y[[3, 500]].any()
        c = centred(b, got.mean32, zp)
        assert (np.abs(y.astype(np.float64) - scores) <= transform_bound(c, got.weights)).all()


def test_float32_fit_on_the_planted_spectrum(torch_mod, ctx):
    """n = 1000, D = 40, 8 components: every component within its Davis-Kahan angle of the reference's, every explained variance within
    its Weyl bound; both bounds come from the input and are below 0.01, so the test cannot pass vacuously."""
    from birdnet_stm32.evaluation.reduce import fit_pca

    x = cases.planted_rows()
    want, sin_bound, var_bound = cases.fit_bounds(x, 8)
    assert (sin_bound < 0.01).all() and (var_bound < 0.01).all(), (sin_bound, var_bound)
    got = fit_pca(_index(x), 8, ctx=ctx)
    assert got.n_rows == 1000 and got.components.shape == (8, 40) and np.array_equal(got.weights, got.components)
    a, b = got.components.astype(np.float64), want.components.astype(np.float64)
    cosine = (a * b).sum(axis=1)
    sine = np.linalg.norm(a - cosine[:, None] * b, axis=1)   # (the part of a across b: well conditioned near 0, unlike sqrt(1 - cos^2))
    rel = np.abs(got.explained_variance / want.explained_variance - 1)
    print("sine", sine, "of", sin_bound, "variance", rel, "of", var_bound)
    assert (cosine > 0).all(), "a sign differs"
    assert (sine <= sin_bound + 2 * U).all()   # (both sets of components are stored as float32: u of a unit vector's length each)
    assert (rel <= var_bound).all()
    assert abs(got.total_variance / want.total_variance - 1) <= var_bound.max()


def test_zero_rows_and_blocks_give_the_model_of_the_same_rows(torch_mod, ctx):
    """1000 live rows in one block against the same rows with three zero rows among them, split into blocks of 512: the runs of 256 rows
    hold the same rows, so the scatter matrices differ by the float64 reordering of four run sums only, and the zero rows come out as zeros."""
    from birdnet_stm32.evaluation.reduce import centred, device_scatter, reduce_index

    x = cases.planted_rows()
    with_zero = np.insert(x, [600, 600, 1000], 0.0, axis=0)
    one, split = _index(x), _index(with_zero, budget_bytes=512 * 40 * 4)
    assert len(split.block_ranges()) == 2
    live = np.ones(1003, bool)
    live[[600, 601, 1002]] = False
    s1, m1, G1 = device_scatter(one, np.ones(1000, bool), ctx)
    s2, m2, G2 = device_scatter(split, live, ctx)
    assert (np.abs(s1 - s2) <= 2 * 1000 * V * np.abs(x.astype(np.float64)).sum(axis=0)).all() and np.array_equal(m1, m2)
    a = np.abs(centred(x, m1).astype(np.float64))
    # either matrix is a float64 sum of the same four run sums: three additions each, the run sums within (1 + 257 u) of sum |c c|
    assert (np.abs(G1 - G2) <= 6 * V * (1 + 257 * U) * (a.T @ a)).all()
    reduced, model = reduce_index(split, 8, ctx=ctx)
    assert len(reduced) == 1003 and reduced.dim == 8 and reduced.dtype == "float32" and model.n_rows == 1000
    assert not reduced.embeddings[[600, 601, 1002]].any() and reduced.embeddings[live].any(axis=1).all()
    assert np.array_equal(reduced.start_s, split.start_s) and reduced.paths == split.paths
    same, _ = reduce_index(split, model, ctx=ctx)
    assert np.array_equal(same.embeddings.view(np.uint32), reduced.embeddings.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------- command
def test_command_line(torch_mod, ctx, tmp_path):
    from birdnet_stm32.cli import reduce as reduce_cli
    from birdnet_stm32.evaluation.cluster import cluster_index
    from birdnet_stm32.evaluation.reduce import PcaModel
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    rows, cluster = cases.three_clusters()
    rows[7] = 0
    db, out, pca, var, again = (str(tmp_path / name) for name in ("db.npz", "r.npz", "pca.npz", "var.csv", "again.npz"))
    cases.write_archive(db, rows)
    reduce_cli.main(["--database", db, "--output", out, "--components", "4", "--whiten", "--model_out", pca, "--variance_out", var])
    idx = EmbeddingIndex.from_npz(out)
    assert len(idx) == 120 and idx.dim == 4 and idx.dtype == "float32" and idx.paths == [f"clip{j}.wav" for j in range(4)] and not idx.embeddings[7].any()
    live = np.arange(120) != 7
    assert cases.same_cluster_share(idx.embeddings[live], cluster[live], cosine=True) == 1.0
    res = idx.search(idx.embeddings[live][:5], k=3, ctx=ctx)
    assert res.idx.shape == (5, 3) and (cluster[res.idx] == 0).all()
    fit = cluster_index(idx, 3, ctx=ctx)
    assert fit.labels[7] == -1 and len({tuple(sorted(set(fit.labels[live][cluster[live] == c]))) for c in range(3)}) == 3
    model = PcaModel.load(pca)
    assert model.whiten and model.n_components == 4 and model.n_rows == 119
    with open(var, newline="") as f:
        lines = list(csv.reader(f))
    assert tuple(lines[0]) == reduce_cli.VARIANCE_COLUMNS and len(lines) == 5 and float(lines[4][3]) <= 1.0 + 1e-9
    reduce_cli.main(["--model", pca, "--database", db, "--output", again])
    with np.load(out) as a, np.load(again) as b:
        assert a["embeddings"].tobytes() == b["embeddings"].tobytes() and a["embeddings"].shape == b["embeddings"].shape
        assert a["pca_weights"].tobytes() == b["pca_weights"].tobytes()
    idx.close()


# ---------------------------------------------------------------------------------------------------------------- project --init pca
def test_project_with_the_pca_start(torch_mod, ctx):
    """The start is ``initial_map_pca`` of the device scores, bit for bit; a short run on three separated clusters ends with a finite
    divergence and every point next to one of its own cluster."""
    from birdnet_stm32.evaluation.project import device_pca_scores, initial_map_pca, project_index

    rows, cluster = cases.three_clusters(per=40, D=24)
    rows = np.insert(rows, 5, 0.0, axis=0)
    live = np.arange(121) != 5
    idx = _index(rows)
    res = project_index(idx, perplexity=10, n_iter=300, exaggeration_iter=100, init="pca", snapshots=(0,), ctx=ctx)
    y0 = initial_map_pca(device_pca_scores(idx, np.flatnonzero(live), ctx))
    assert y0.dtype == np.float32 and np.array_equal(res.trajectory[0].view(np.uint32), y0.view(np.uint32))
    assert abs(float(y0[:, 0].astype(np.float64).std()) / 1e-4 - 1) < 1e-6
    assert np.isfinite(res.kl) and np.isnan(res.xy[5]).all() and np.isfinite(res.xy[live]).all()
    assert cases.same_cluster_share(res.xy[live], cluster) == 1.0
    again = project_index(idx, perplexity=10, n_iter=300, exaggeration_iter=100, init="pca", seed=7, ctx=ctx)
    assert np.array_equal(again.xy[live].view(np.uint32), res.xy[live].view(np.uint32)), "the PCA start does not depend on the seed"
    with pytest.raises(ValueError, match="init must be"):
        project_index(idx, perplexity=10, init="spectral", ctx=ctx)
