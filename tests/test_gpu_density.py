"""GPU tests of density clustering: ``bn_density_nearest`` against ``nearest_reference`` bit for bit where the specification has one value
(lattice rows, int8 bytes), symmetry and a rounding bound on real-valued rows, whole spanning trees against the float64 optimum, whole
fits against ``hdbscan_reference`` and the ``density`` command end to end with both shipped models."""

import csv
import os
import wave

import numpy as np
import pytest

from conftest import CONFIG_PATH, KERAS_PATH, TFLITE_PATH

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # unit roundoff of float32
GUARD = 8
GUARD_BITS = 0x7FC0BEEF7FC0BEEF   # a NaN pattern in both halves


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


class _Device:
    """Rows and their inverse norms on the device, and ``bn_density_nearest`` through the C ABI: keys [n] uint64 on the host.  The output
    sits between guard entries; the inputs are compared with what went up after every call."""

    def __init__(self, torch, ctx, rows, zp=0):
        from birdnet_stm32 import _hip

        self.torch, self.ctx, self.hip, self.rows, self.zp = torch, ctx, _hip, rows, zp
        self.n, self.D = rows.shape
        self.code = _hip.DTYPE_I8 if rows.dtype == np.int8 else _hip.DTYPE_F32
        self.d_rows = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        self.d_inv = torch.empty(self.n, dtype=torch.float32, device="cuda")
        _hip.check(ctx.lib.bn_search_inv_norms(ctx.handle, self.d_rows.data_ptr(), self.code, self.n, self.D, zp, self.d_inv.data_ptr(), None))
        self.inv = self.d_inv.cpu().numpy()

    def nearest(self, core, comp):
        torch = self.torch
        core, comp = np.ascontiguousarray(core, np.float32), np.ascontiguousarray(comp, np.int32)
        d_core, d_comp = torch.from_numpy(core).cuda(), torch.from_numpy(comp).cuda()
        buf = torch.from_numpy(np.full(self.n + 2 * GUARD, GUARD_BITS, np.uint64).view(np.int64)).cuda()
        out = buf[GUARD:GUARD + self.n]
        self.hip.check(self.ctx.lib.bn_density_nearest(self.ctx.handle, self.d_rows.data_ptr(), self.code, self.n, self.D, self.zp, self.d_inv.data_ptr(),
                                                       d_core.data_ptr(), d_comp.data_ptr(), out.data_ptr(), None))
        torch.cuda.synchronize()
        got = buf.cpu().numpy().view(np.uint64)
        assert (got[:GUARD] == GUARD_BITS).all() and (got[GUARD + self.n:] == GUARD_BITS).all(), "wrote outside the n keys"
        assert np.array_equal(self.d_rows.cpu().numpy(), self.rows) and np.array_equal(self.d_inv.cpu().numpy().view(np.uint32), self.inv.view(np.uint32))
        assert np.array_equal(d_core.cpu().numpy().view(np.uint32), core.view(np.uint32)) and np.array_equal(d_comp.cpu().numpy(), comp)
        return got[GUARD:GUARD + self.n].copy()


# ------------------------------------------------------------------------------------------------------------------- equality
def _tile_and_range_crossings():
    """An N one past a staged tile and one past a workgroup's range of streamed rows, from the header's constants."""
    from birdnet_stm32 import _hip

    tile = _hip.density_tile_rows(1 << 18, 96, False)
    rng = _hip.DENSITY_MIN_WG_STEPS * _hip.DENSITY_STEP_ROWS
    assert tile == _hip.DENSITY_MAX_TILE == 128 and _hip.density_rows_per_workgroup(rng) == rng and _hip.density_rows_per_workgroup(rng + 1) < rng
    return tile + 1, rng + 1


# every N of {2, 15, 17, 1000, 4099} and every D of {8, 96, 255, 256} at least once, then the two crossings
SHAPES = [(2, 8), (15, 96), (17, 255), (1000, 256), (4099, 96), (4099, 255), ("tile", 96), ("range", 8), ("range", 256)]


def _shape(s):
    n, D = s
    tile, rng = _tile_and_range_crossings()
    return ({"tile": tile, "range": rng}.get(n, n), D)


def _lattice_rows(n, D, seed, zp=None):
    """float32 rows on {0, 1/16, ..., 15/16} (dot products exact for D <= 256) or full-range bytes; a tenth of the rows duplicated."""
    rng = np.random.default_rng(seed)
    if zp is None:
        x = (rng.integers(0, 16, (n, D)) / 16.0).astype(np.float32)
        x[x.sum(axis=1) == 0, 0] = 0.5
    else:
        x = rng.integers(-128, 128, (n, D)).astype(np.int8)
        x[(x.astype(np.int64) == zp).all(axis=1), 0] = zp + 1 if zp < 127 else zp - 1
    for _ in range(n // 10):
        a, b = rng.integers(0, n, 2)
        x[a] = x[b]
    return x


def _components(n, seed):
    with_out = np.arange(n) % 5
    with_out[np.random.default_rng(seed).integers(0, n, max(1, n // 8))] = -1
    return {"identity": np.arange(n), "two": (np.arange(n) >= n // 2).astype(np.int64), "mod7": np.arange(n) % 7, "one": np.zeros(n, np.int64), "out": with_out}


def _check_nearest(torch, ctx, x, zp, seed):
    from birdnet_stm32.evaluation.density import core_scores_reference, mutual_reachability, nearest_from_scores, pair_scores, split_keys

    n, zero = x.shape[0], zp or 0
    dev = _Device(torch, ctx, x, zero)
    s = pair_scores(x, zero)
    comps = _components(n, seed)
    cores = {1: np.full(n, np.inf, np.float32)}
    # (for the suite's time the largest shapes take one search on the host, and none where it multiplies int8 rows in int64)
    for ms in (2, 5, 16) if n <= 2100 else (5,) if zp is None else ():
        if ms <= n:
            cores[ms] = core_scores_reference(x, ms, zero)
    # every component vector under one kind of core, every kind of core under one component vector (all of both where that is cheap)
    cases = [(ms, c) for ms in cores for c in comps] if n <= 1000 else [(max(cores), c) for c in comps] + [(ms, "mod7") for ms in cores]
    for ms, c in cases:
        want = nearest_from_scores(mutual_reachability(s, cores[ms]), comps[c])
        got = dev.nearest(cores[ms], comps[c])
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"min_samples {ms}, components {c}: {bad.size} keys differ, first row {bad[0]}: got {split_keys(got[bad[:1]])}, want {split_keys(want[bad[:1]])}"
        if c == "one":
            assert (got == 0).all()
        if c == "out":
            partner = split_keys(got)[1]
            assert (got[comps[c] < 0] == 0).all() and (comps[c][partner[partner >= 0]] >= 0).all()
    if n > 16 and max(cores) > 1:
        m = mutual_reachability(s, cores[max(cores)])
        assert (np.sort(m, axis=1)[:, -3] == np.sort(m, axis=1)[:, -2]).mean() > 0.5, "the input should make many scores tie"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nearest_of_lattice_rows_equals_the_reference_bit_for_bit(torch_mod, ctx, shape):
    n, D = _shape(shape)
    _check_nearest(torch_mod, ctx, _lattice_rows(n, D, 10 + D), None, n)


# every shape and every zero point several times; all three zero points at the shapes that take more than one tile or workgroup
INT8_CASES = [(2, 8, -128), (2, 8, 0), (2, 8, 5), (15, 96, 0), (15, 96, 5), (17, 255, -128), (17, 255, 5), (1000, 256, -128), (1000, 256, 0), (1000, 256, 5),
              (4099, 96, 5), (4099, 255, -128), ("tile", 255, -128), ("tile", 255, 0), ("tile", 255, 5), ("range", 8, -128), ("range", 8, 0), ("range", 8, 5)]


@pytest.mark.parametrize("n, D, zp", INT8_CASES)
def test_nearest_of_int8_rows_equals_the_reference_bit_for_bit(torch_mod, ctx, n, D, zp):
    n, D = _shape((n, D))
    _check_nearest(torch_mod, ctx, _lattice_rows(n, D, 20 + D, zp), zp, n)


# ------------------------------------------------------------------------------------------------------------- real-valued rows
def _clusters(n, D, C, seed):
    """Rectified Gaussian clusters as tests/test_gpu_search.py makes them, and the blob every row was drawn from."""
    cent = np.random.default_rng(1000 + D + C).standard_normal((C, D))
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, C, n)
    return np.maximum(cent[lab] + 1.5 * rng.standard_normal((n, D)), 0).astype(np.float32), lab


def _pair_bound(x):
    """Float64 scores S [n, n] and a bound on the float32 device error of each: ``_score_bound`` (cosine) of tests/test_gpu_search.py for
    the symmetric product.  fl(dot * fl(inv_i * inv_j)) has as many roundings as fl(fl(dot * inv_q) * inv_row), so the bound is the same:
    1.01 ((D + 2) u adot inv_i inv_j + |S| (D + 8) u)."""
    D = x.shape[1]
    X = x.astype(np.float64)
    dot, adot = X @ X.T, np.abs(X) @ np.abs(X).T
    nx = np.sqrt((X * X).sum(axis=1))
    ix = np.divide(1.0, nx, out=np.zeros_like(nx), where=nx > 0)
    S = dot * ix[:, None] * ix[None, :]
    return S, 1.01 * ((D + 2) * U * adot * ix[:, None] * ix[None, :] + np.abs(S) * (D + 8) * U)


def test_pair_scores_are_symmetric_on_real_valued_rows(torch_mod, ctx):
    from birdnet_stm32.evaluation.density import split_keys

    x, _ = _clusters(1537, 64, 6, 7)
    n = x.shape[0]
    m, j = split_keys(_Device(torch_mod, ctx, x).nearest(np.full(n, np.inf, np.float32), np.arange(n)))
    assert (j >= 0).all() and (j != np.arange(n)).all()
    mutual = np.flatnonzero(j[j] == np.arange(n))
    assert mutual.size >= 2, "no mutual pair in the input"
    assert np.array_equal(m[mutual].view(np.uint32), m[j[mutual]].view(np.uint32)), "a pair has two scores"


@pytest.mark.parametrize("n, D, C, seed", [(4099, 256, 8, 5), (1000, 96, 4, 6), (1537, 64, 6, 7)])
def test_real_valued_rows_within_the_bound(torch_mod, ctx, n, D, C, seed):
    from birdnet_stm32.evaluation.density import split_keys

    x, blob = _clusters(n, D, C, seed)
    S, B = _pair_bound(x)
    dev = _Device(torch_mod, ctx, x)
    rows = np.arange(n)
    for name, comp in (("identity", rows), ("mod7", rows % 7), ("blob", blob)):
        # clean rows from the float64 reference alone: the best foreign row beats the runner-up by more than the two bounds
        foreign = comp[None, :] != comp[:, None]
        Sf = np.where(foreign, S, -np.inf)
        order = np.argsort(-Sf, axis=1, kind="stable")[:, :2]
        best, second = order[:, 0], order[:, 1]
        clean = (Sf[rows, best] - Sf[rows, second]) > (B[rows, best] + B[rows, second])
        print(f"{n} x {D}, components {name}: clean share {clean.mean():.4%}")
        assert clean.mean() >= 0.99
        m, j = split_keys(dev.nearest(np.full(n, np.inf, np.float32), comp))
        assert np.array_equal(j[clean], best[clean])
        err = np.abs(m[clean].astype(np.float64) - S[rows, best][clean])
        print(f"    largest error / bound {np.max(err / B[rows, best][clean]):.3f}")
        assert (err <= B[rows, best][clean]).all()


def _index(x, zp=0, scale=1.0):
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    n = x.shape[0]
    return EmbeddingIndex(x, np.zeros(n, np.int64), 3.0 * np.arange(n), ["a.wav"], scale=scale, zero_point=zp)


def test_whole_tree_on_real_valued_rows_is_optimal_within_the_bound(torch_mod, ctx):
    from birdnet_stm32.evaluation.density import density_index, mst_reference

    x, _ = _clusters(1000, 96, 4, 6)
    n, ms = x.shape[0], 5
    res = density_index(_index(x), 15, ms, ctx=ctx)
    edges = res.mst_edges
    assert edges.shape == (n - 1, 2)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in edges.tolist():   # n - 1 edges that never close a cycle: a spanning tree
        ra, rb = find(a), find(b)
        assert ra != rb
        parent[ra] = rb
    S, B = _pair_bound(x)
    off = np.where(np.eye(n, dtype=bool), -np.inf, S)
    core = np.sort(off, axis=1)[:, -(ms - 1)]   # float64 cores: the (min_samples - 1)-th best other row
    M = np.minimum(np.minimum(S, core[:, None]), core[None, :])
    b_max = B[~np.eye(n, dtype=bool)].max()   # (a core is a pair's score: the pair bound covers it)
    assert np.abs(res.core.astype(np.float64) - core).max() <= b_max
    want_edges, _ = mst_reference(M)
    got, want = M[edges[:, 0], edges[:, 1]].sum(), M[want_edges[:, 0], want_edges[:, 1]].sum()
    print(f"tree weight {got:.9f}, float64 optimum {want:.9f}, margin {2 * (n - 1) * b_max:.3e}")
    assert got >= want - 2 * (n - 1) * b_max


# ----------------------------------------------------------------------------------------------------------------- whole fits
def _lattice_blobs(seed, int8_zp=None):
    """About 600 rows: base patterns with small lattice perturbations, scattered rows in between, two zero rows."""
    rng = np.random.default_rng(seed)
    D, k, per, scattered = 32, 6, 90, 58
    if int8_zp is None:
        base = rng.integers(0, 16, (k, D))
        x = np.concatenate([np.clip(base[c] + rng.integers(-1, 2, (per, D)) * (rng.random((per, D)) < 0.3), 0, 15) for c in range(k)] + [rng.integers(0, 16, (scattered, D))])
        x = (x / 16.0).astype(np.float32)
        x[x.sum(axis=1) == 0, 0] = 0.5
        zero = 0
    else:
        base = rng.integers(-100, 100, (k, D))
        x = np.concatenate([np.clip(base[c] + rng.integers(-6, 7, (per, D)), -128, 127) for c in range(k)] + [rng.integers(-128, 128, (scattered, D))]).astype(np.int8)
        zero = int8_zp
    x = x[rng.permutation(x.shape[0])]
    x[[17, 401]] = zero
    return x


def _same_fit(a, b):
    assert np.array_equal(a.labels, b.labels) and np.array_equal(a.score.view(np.uint64), b.score.view(np.uint64)) and a.n_clusters == b.n_clusters
    assert np.array_equal(a.mst_edges, b.mst_edges) and np.array_equal(a.mst_weight.view(np.uint32), b.mst_weight.view(np.uint32))
    assert np.array_equal(a.stability.view(np.uint64), b.stability.view(np.uint64)) and np.array_equal(a.exemplar_idx, b.exemplar_idx)
    assert np.array_equal(a.core.view(np.uint32), b.core.view(np.uint32)) and a.rounds == b.rounds


@pytest.mark.parametrize("zp, sizes", [(None, (10, 5)), (None, (15, None)), (None, (8, 1)), (5, (10, 5)), (-128, (12, 3))])
def test_whole_fit_equals_the_reference(torch_mod, ctx, zp, sizes):
    from birdnet_stm32.evaluation.density import density_index, hdbscan_reference

    x = _lattice_blobs(3, zp)
    want = hdbscan_reference(x, sizes[0], sizes[1], zero_point=zp or 0)
    assert want.n_clusters >= 3 and (want.labels[[17, 401]] == -1).all() and (want.score[[17, 401]] == 0).all() and (want.labels < 0).sum() > 2
    index = _index(x, zp or 0, 0.05)
    got = density_index(index, sizes[0], sizes[1], ctx=ctx)
    _same_fit(got, want)
    _same_fit(density_index(index, sizes[0], sizes[1], ctx=ctx), got)   # the same bits on every run
    assert np.isnan(got.core[[17, 401]]).all() and 1 <= got.rounds <= 10


def test_fit_without_zero_rows_shares_the_resident_block(torch_mod, ctx):
    from birdnet_stm32.evaluation.density import density_index, hdbscan_reference

    x = _lattice_blobs(4)
    x = np.delete(x, [17, 401], axis=0)
    index = _index(x)
    got = density_index(index, 10, 5, ctx=ctx)
    assert index._resident is not None   # the block `search` keeps
    _same_fit(got, hdbscan_reference(x, 10, 5))


def test_refusals_surface_as_value_errors(torch_mod, ctx):
    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation.density import density_index

    x = _lattice_blobs(3)[:40]
    for kw, what in ((dict(min_cluster_size=1), "min_cluster_size"), (dict(min_cluster_size=41), "min_cluster_size"), (dict(min_cluster_size=5, min_samples=0), "min_samples"),
                     (dict(min_cluster_size=5, min_samples=40), "min_samples"), (dict(min_cluster_size=5, exemplars=-1), "exemplars")):
        with pytest.raises(ValueError, match=what):
            density_index(_index(x), ctx=ctx, **kw)   # (row 17 is a zero row: 39 rows take part)
    z = np.zeros((3, 32), np.float32)
    z[1, 0] = 1
    with pytest.raises(ValueError, match="at least 2 non-zero rows"):
        density_index(_index(z), 2, ctx=ctx)
    # the C ABI itself
    dev = _Device(torch_mod, ctx, x)
    d = torch_mod.zeros(64, dtype=torch_mod.int64, device="cuda")
    lib, h = ctx.lib, ctx.handle
    for args in ((h, None, dev.code, 40, 32, 0, dev.d_inv.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr(), None),
                 (h, dev.d_rows.data_ptr(), dev.code, 40, 0, 0, dev.d_inv.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr(), None),
                 (h, dev.d_rows.data_ptr(), dev.code, _hip.DENSITY_MAX_N + 1, 32, 0, dev.d_inv.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr(), None),
                 (h, dev.d_rows.data_ptr(), 7, 40, 32, 0, dev.d_inv.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr(), None),
                 (h, dev.d_rows.data_ptr(), dev.code, 40, 32, 0, dev.d_inv.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr() + 4, None)):
        with pytest.raises(_hip.HipError):
            _hip.check(lib.bn_density_nearest(*args))
    torch_mod.cuda.synchronize()
    assert (d.cpu().numpy() == 0).all()   # a refused call writes nothing


def test_library_names_the_density_kernel(ctx):
    assert "density_nearest_kernel" in ctx.lib.bn_kernel_names().decode().split("\n")


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
def test_embed_then_density_end_to_end(torch_mod, tmp_path, model, dtype):
    from birdnet_stm32.cli import cluster as cluster_cli
    from birdnet_stm32.cli import density as density_cli
    from birdnet_stm32.cli import embed as embed_cli
    from birdnet_stm32.evaluation.density import hdbscan_reference, hierarchy
    from birdnet_stm32.evaluation.search import EmbeddingIndex, inv_norms_reference
    from birdnet_stm32.models.runners import load_model_runner

    paths = []
    for kind, freq in enumerate((700.0, 2000.0, 4800.0)):   # the 24 clips of tests/test_gpu_cluster.py: three kinds of tone, eight of each
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
    out = str(tmp_path / "density.csv")
    res = density_cli.main(["--database", db_npz, "--output", out, "--min_cluster_size", "4", "--exemplars", "2", "--chunk_duration", "3"])
    if dtype == "int8":   # exact dot products: the specification has one value
        want = hdbscan_reference(index.embeddings, 4, zero_point=index.zero_point, exemplars=2)
        assert np.array_equal(res.labels, want.labels) and np.array_equal(res.score, want.score) and np.array_equal(res.mst_edges, want.mst_edges)
        assert np.array_equal(res.exemplar_idx, want.exemplar_idx) and np.array_equal(res.stability, want.stability)
    else:
        # float32 dot products are summed in the device's order, and clips that differ by 0.4 % in pitch are near-duplicates: lambda =
        # (2 - 2 m)^-1/2 is ill-conditioned there, so numpy's tree is no reference for the labels.  What must hold exactly: the device's
        # edges span the rows, and labels and scores are the host hierarchy of that very tree.
        assert (inv_norms_reference(index.embeddings) != 0).all() and res.mst_edges.shape == (23, 2)
        seen = {0}
        for _ in range(23):
            seen |= {int(b) for a, b in res.mst_edges if int(a) in seen} | {int(a) for a, b in res.mst_edges if int(b) in seen}
        assert seen == set(range(24))
        h = hierarchy(res.mst_edges, res.mst_weight, 24, 4)
        assert np.array_equal(res.labels, h.labels) and np.array_equal(res.score, h.score) and np.array_equal(res.stability, h.cluster_stability)
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == density_cli.CSV_COLUMNS == ("path", "start_s", "end_s", "cluster", "score") and len(rows) == 25
    assert [int(r[3]) for r in rows[1:]] == res.labels.tolist() and [r[4] for r in rows[1:]] == [f"{s:.7g}" for s in res.score]
    assert all(float(r[2]) == float(r[1]) + 3.0 for r in rows[1:]) and all(0.0 <= float(r[4]) <= 1.0 for r in rows[1:])
    kout = str(tmp_path / "clusters.csv")
    cluster_cli.main(["--database", db_npz, "--k", "3", "--output", kout, "--exemplars", "0", "--chunk_duration", "3"])
    with open(kout, newline="") as f:
        krows = list(csv.reader(f))
    assert [r[:3] for r in krows] == [r[:3] for r in rows]   # line by line with `cluster`'s file for the same archive
    with open(density_cli.summary_path(out), newline="") as f:
        summary = list(csv.reader(f))
    assert summary[0] == ["cluster", "count", "stability", "exemplar_1", "exemplar_2"] and len(summary) == 1 + res.n_clusters
    assert [int(r[1]) for r in summary[1:]] == [int((res.labels == c).sum()) for c in range(res.n_clusters)]
    with pytest.raises(SystemExit, match="min_cluster_size"):
        density_cli.main(["--database", db_npz, "--output", out, "--min_cluster_size", "25"])
