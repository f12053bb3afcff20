"""GPU tests of query by example (csrc/bn_search.hip, evaluation/search.py, cli/search.py) against the numpy specification
``search_reference``.

Equality tests use inputs on which the specification has one value whatever the summation order: a lattice {0, 1/16, ..., 15/16} (every
product and partial sum is exact in float32 for D <= 256) and INT8 bytes (integer sums).  Real-valued rows are held to a written-out error
bound, with exact index equality required on the queries the float64 reference alone separates.  The shapes cover one MFMA tile and less,
ragged tiles, widths that are no multiple of the 16-byte load, a second query pass, every k the lists hold, and a row count derived from
the kernel's own constants at which several workgroups and the merge kernel take part."""

import csv
import ctypes
import os
import wave

import numpy as np
import pytest

from conftest import CONFIG_PATH, KERAS_PATH, TFLITE_PATH

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # unit roundoff of float32


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


def _multi_wg_rows():
    """Two full workgroups and a ragged third, from the constants the launcher deals rows by."""
    from birdnet_stm32 import _hip

    per_wg = _hip.SEARCH_STEP_ROWS * _hip.SEARCH_MIN_WG_STEPS
    n = 2 * per_wg + per_wg // 2 + 37
    steps = -(-n // _hip.SEARCH_STEP_ROWS)
    wgs = -(-steps // _hip.SEARCH_MIN_WG_STEPS)
    per = -(-steps // wgs)
    assert -(-steps // per) == 3 and n % _hip.SEARCH_STEP_ROWS != 0 and 3 <= _hip.SEARCH_MAX_WGS
    return n


# (N, D, Q, k): every N, D, Q and k of the grid at least once, k > N, and the multi-workgroup N at a small D.  A fifth entry "off": the rows
# start one element behind a 16-byte boundary while D is a multiple of 16, so every chunk of every row takes the loader's slow path (one
# full 16-row tile, one ragged tile, one chunk group)
SHAPES = [(1, 256, 1, 1), (1, 8, 16, 10), (15, 96, 17, 10), (15, 255, 1, 128), (17, 256, 16, 10), (17, 8, 100, 128), (1000, 256, 17, 10),
          (1000, 96, 100, 1), (1000, 255, 16, 128), (4099, 256, 100, 10), (4099, 8, 1, 1), (4099, 255, 17, 128), (4099, 96, 16, 10),
          ("multi", 8, 17, 10), ("multi", 8, 100, 128), (17, 256, 16, 10, "off")]


def _shape(s):
    N, D, Q, k = s[:4]
    return (_multi_wg_rows() if N == "multi" else N), D, Q, k, len(s) > 4


def _shape_id(s):
    return "N{}-D{}-Q{}-k{}".format(*s) + "-off" * (len(s) > 4)


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
    torch.cuda.synchronize()
    return d, out


def _search(torch, ctx, db, q, k, metric, zp=0, db_group=None, q_group=None, off=False):
    """bn_search_topk through the C ABI: (idx int64, score float32) on the host.  ``off``: the database rows off the 16-byte boundary."""
    from birdnet_stm32 import _hip

    d_db, d_inv = _inv_norms(torch, ctx, db, zp, off)
    d_q, d_qinv = _inv_norms(torch, ctx, q, zp)
    Q = q.shape[0]
    idx = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    score = torch.zeros((Q, k), dtype=torch.float32, device="cuda")
    g_db = torch.from_numpy(np.asarray(db_group, np.int32)).cuda() if db_group is not None else None
    g_q = torch.from_numpy(np.asarray(q_group, np.int32)).cuda() if q_group is not None else None
    code = _hip.DTYPE_I8 if db.dtype == np.int8 else _hip.DTYPE_F32
    _hip.check(ctx.lib.bn_search_topk(ctx.handle, d_db.data_ptr(), code, db.shape[0], db.shape[1], zp, d_inv.data_ptr(), d_q.data_ptr(), Q, d_qinv.data_ptr(),
                                      _hip.SEARCH_METRICS[metric], g_db.data_ptr() if g_db is not None else None, g_q.data_ptr() if g_q is not None else None,
                                      k, idx.data_ptr(), score.data_ptr(), None))
    torch.cuda.synchronize()
    return idx.cpu().numpy().astype(np.int64), score.cpu().numpy()


def _lattice(N, D, Q, seed):
    """Rows and queries on {0, 1/16, ..., 15/16} with duplicated rows (ties inside the top k), a zero row and a zero query."""
    rng = np.random.default_rng(seed)
    db = (rng.integers(0, 16, (N, D)) / 16.0).astype(np.float32)
    if N >= 15:
        src = rng.integers(0, N, N // 3)
        db[rng.integers(0, N, N // 3)] = db[src]
        db[N // 2] = 0.0
    q = (rng.integers(0, 16, (Q, D)) / 16.0).astype(np.float32)
    take = min(Q, N, 8)
    q[:take] = db[rng.integers(0, N, take)]   # queries that are rows: their duplicates tie at the top
    if Q > 1:
        q[-1] = 0.0
    return db, q


def _assert_equal(got, want, what):
    gi, gs = got
    wi, ws = want
    assert np.array_equal(gi, wi), f"{what}: indices differ in {int((gi != wi).any(axis=1).sum())} of {gi.shape[0]} queries"
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), f"{what}: scores differ"


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_lattice_rows_equal_the_reference_bit_for_bit(torch_mod, ctx, shape):
    from birdnet_stm32.evaluation.search import search_reference

    N, D, Q, k, off = _shape(shape)
    db, q = _lattice(N, D, Q, 11 + N + D)
    ties = 0
    for metric in ("cosine", "dot"):
        want = search_reference(db, q, k, metric)
        _assert_equal(_search(torch_mod, ctx, db, q, k, metric, off=off), want, f"{shape} {metric}")
        ties += int((want[1][:, 1:] == want[1][:, :-1]).sum())
    if N >= 1000 and k >= 10:
        assert ties > 0, "the duplicated rows should tie inside the top k"


@pytest.mark.parametrize("zp", [-128, 0, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_int8_rows_equal_the_reference_bit_for_bit(torch_mod, ctx, shape, zp):
    from birdnet_stm32.evaluation.search import search_reference

    N, D, Q, k, off = _shape(shape)
    rng = np.random.default_rng(1000 + N + D + zp)   # (zp may be -128: the seed must not be negative)
    db = rng.integers(-128, 128, (N, D)).astype(np.int8)
    q = rng.integers(-128, 128, (Q, D)).astype(np.int8)
    if N >= 15:
        db[rng.integers(0, N, N // 4)] = db[rng.integers(0, N, N // 4)]
        db[N // 2] = zp   # a zero vector
    q[: min(Q, N, 4)] = db[: min(Q, N, 4)]
    for metric in ("cosine", "dot"):
        _assert_equal(_search(torch_mod, ctx, db, q, k, metric, zp=zp, off=off), search_reference(db, q, k, metric, zero_point=zp), f"{shape} zp={zp} {metric}")


def _clusters(n, D, C, seed):
    """Rectified Gaussian clusters (as test_gpu_probe.py makes them): non-negative like pooled ReLU features."""
    cent = np.random.default_rng(1000 + D + C).standard_normal((C, D))
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, C, n)
    return np.maximum(cent[lab] + 1.5 * rng.standard_normal((n, D)), 0).astype(np.float32)


def _score_bound(db, q, metric):
    """Float64 scores S [Q, N] and a bound on the float32 device error of each.

    Dot product: a length-D sum accumulated in float32 in some order (v_mfma_f32_16x16x4_f32 is an fmaf chain), |d dot| <= (D + 2) u
    sum |x_j q_j|.  Norm: the sum of squares has non-negative terms, so the same bound is relative, (D + 2) u n; the correctly rounded
    square root halves it and adds u, the division adds u: |d inv| <= ((D + 2) / 2 + 2) u inv.  Cosine = fl(fl(dot inv_q) inv_row): two
    more roundings, so |d S| <= (D + 2) u sum |x_j q_j| inv_q inv_row + |S| ((D + 2) + 4 + 2) u, and 1 % on top for the products of
    these first-order terms (D u < 2e-5)."""
    D = db.shape[1]
    X, Y = db.astype(np.float64), q.astype(np.float64)
    dot, adot = Y @ X.T, np.abs(Y) @ np.abs(X).T
    if metric == "dot":
        return dot, 1.01 * (D + 2) * U * adot
    nx, ny = np.sqrt((X * X).sum(axis=1)), np.sqrt((Y * Y).sum(axis=1))
    ix = np.divide(1.0, nx, out=np.zeros_like(nx), where=nx > 0)
    iy = np.divide(1.0, ny, out=np.zeros_like(ny), where=ny > 0)
    S = dot * iy[:, None] * ix[None, :]
    return S, 1.01 * ((D + 2) * U * adot * iy[:, None] * ix[None, :] + np.abs(S) * (D + 8) * U)


@pytest.mark.parametrize("N,D,Q,k,clean_cpu", [(4099, 256, 33, 10, 0.88), (1000, 96, 16, 10, 1.0), (70001, 64, 17, 10, 0.94)])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_real_valued_rows_within_the_bound(torch_mod, ctx, N, D, Q, k, clean_cpu, metric):
    """Rules per query: every returned score within the bound of the float64 score of its row; every row that beats the k-th best by
    more than the two bounds is present; no returned row lies below the k-th best by more than the two bounds; the list is sorted under
    the total order on the device's own scores.  A query is clean when the float64 reference alone separates positions 1 .. k + 1 by
    more than the neighbouring bounds: at least 75 % must be (computed before the device output is looked at; the cosine reference gives
    88 %, 100 % and 94 % for the three shapes on the CPU), and on those the indices must equal the reference's."""
    db = _clusters(N, D, 12, 5)
    q = _clusters(Q, D, 12, 6)
    S, B = _score_bound(db, q, metric)
    order = np.stack([np.lexsort((np.arange(N), -S[i])) for i in range(Q)])[:, : k + 1]
    so, bo = np.take_along_axis(S, order, 1), np.take_along_axis(B, order, 1)
    clean = ((so[:, :-1] - so[:, 1:]) > (bo[:, :-1] + bo[:, 1:])).all(axis=1)
    print(f"{(N, D, Q, k)} {metric}: clean share {clean.mean():.3f}")
    assert clean.mean() >= 0.75
    gi, gs = _search(torch_mod, ctx, db, q, k, metric)
    assert (gi >= 0).all() and all(len(set(r)) == k for r in gi.tolist())
    err = np.abs(gs.astype(np.float64) - np.take_along_axis(S, gi, 1))
    assert (err <= np.take_along_axis(B, gi, 1)).all(), f"largest error / bound {float((err / np.take_along_axis(B, gi, 1)).max()):.3f}"
    kth, kb = so[:, k - 1], bo[:, k - 1]
    for i in range(Q):
        must = np.flatnonzero(S[i] - B[i] > kth[i] + kb[i])
        assert np.isin(must, gi[i]).all(), f"query {i}: a row clearly among the best {k} is missing"
        assert (S[i, gi[i]] + B[i, gi[i]] >= kth[i] - kb[i]).all(), f"query {i}: a returned row is clearly not among the best {k}"
        d = np.diff(gs[i])
        assert ((d < 0) | ((d == 0) & (np.diff(gi[i]) > 0))).all(), f"query {i}: the list is not sorted"
    assert np.array_equal(gi[clean], order[clean, :k]), "indices differ on a clean query"


def test_groups_exclude_the_querys_own_file(torch_mod, ctx):
    from birdnet_stm32.evaluation.search import EmbeddingIndex, search_reference

    N, D, Q, k = 1000, 96, 40, 10
    db, _ = _lattice(N, D, 1, 3)
    group = np.random.default_rng(4).integers(0, 25, N)
    qrow = np.arange(0, N, N // Q)[:Q]
    q, qg = db[qrow], group[qrow]
    for metric in ("cosine", "dot"):
        want = search_reference(db, q, k, metric, db_group=group, query_group=qg)
        got = _search(torch_mod, ctx, db, q, k, metric, db_group=group, q_group=qg)
        _assert_equal(got, want, metric)
        assert (group[got[0]] != qg[:, None]).all()
    index = EmbeddingIndex(db, group, np.zeros(N), [f"f{i}.wav" for i in range(25)])
    res = index.search(q, k=k, query_file_index=qg, exclude_same_file=True, ctx=ctx)
    _assert_equal((res.idx, res.score), search_reference(db, q, k, "cosine", db_group=group, query_group=qg), "EmbeddingIndex")
    assert all(p != f"f{g}.wav" for row, g in zip(res.match_path, qg) for p in row)
    free = index.search(q, k=k, ctx=ctx)
    _assert_equal((free.idx, free.score), search_reference(db, q, k, "cosine"), "EmbeddingIndex without the exclusion")
    assert (free.score[:, 0] >= res.score[:, 0]).all() and (free.idx != res.idx).any()


def test_inverse_norms(torch_mod, ctx):
    from birdnet_stm32.evaluation.search import inv_norms_reference

    for D in (256, 96, 255, 8):
        rows, _ = _lattice(1000, D, 1, D)
        assert np.array_equal(_inv_norms(torch_mod, ctx, rows)[1].cpu().numpy().view(np.uint32), inv_norms_reference(rows).view(np.uint32)), D
        for zp in (-128, 0, 5):
            b = np.random.default_rng(1000 + D + zp).integers(-128, 128, (1000, D)).astype(np.int8)
            b[7] = zp
            got = _inv_norms(torch_mod, ctx, b, zp)[1].cpu().numpy()
            assert got[7] == 0.0 and np.array_equal(got.view(np.uint32), inv_norms_reference(b, zp).view(np.uint32)), (D, zp)
        x = _clusters(1001, D, 12, 9)
        x[5] = 0.0
        got = _inv_norms(torch_mod, ctx, x)[1].cpu().numpy().astype(np.float64)
        n = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
        want = np.divide(1.0, n, out=np.zeros_like(n), where=n > 0)
        assert got[5] == 0.0 and (np.abs(got - want) <= (D + 4) * U * want).all(), D


def test_same_call_same_bits_and_blocks_do_not_show(torch_mod, ctx):
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    db = _clusters(4099, 256, 12, 5)
    q = _clusters(33, 256, 12, 6)
    a, b = _search(torch_mod, ctx, db, q, 10, "cosine"), _search(torch_mod, ctx, db, q, 10, "cosine")
    _assert_equal(a, b, "two calls")
    files = np.arange(4099) // 100
    paths = [f"f{i}.wav" for i in range(41)]
    whole = EmbeddingIndex(db, files, np.zeros(4099), paths).search(q, k=10, ctx=ctx)
    _assert_equal((whole.idx, whole.score), a, "EmbeddingIndex in one block")
    small = EmbeddingIndex(db, files, np.zeros(4099), paths, budget_bytes=700 * 1024)
    assert len(small.block_ranges()) > 4
    parts = small.search(q, k=10, ctx=ctx)
    _assert_equal((parts.idx, parts.score), a, "EmbeddingIndex in several blocks")
    qt = torch_mod.from_numpy(q).cuda()
    _assert_equal((lambda r: (r.idx, r.score))(small.search(qt, k=10, ctx=ctx)), a, "queries as a CUDA tensor")
    rng = np.random.default_rng(8)
    b8, q8 = rng.integers(-128, 128, (3000, 256)).astype(np.int8), rng.integers(-128, 128, (5, 256)).astype(np.int8)
    i8 = EmbeddingIndex(b8, np.zeros(3000, np.int64), np.zeros(3000), ["a.wav"], "int8", 0.05, -128, budget_bytes=64 * 1024)
    from birdnet_stm32.evaluation.search import search_reference

    wi, ws = search_reference(b8, q8, 7, "dot", zero_point=-128)
    r = i8.search(q8, k=7, metric="dot", ctx=ctx)
    assert np.array_equal(r.idx, wi) and np.array_equal(r.score, ws * (np.float32(0.05) * np.float32(0.05)))


def test_refused_calls(torch_mod, ctx):
    from birdnet_stm32 import _hip

    torch = torch_mod
    db = torch.zeros((32, 16), dtype=torch.float32, device="cuda")
    inv = torch.ones(32, dtype=torch.float32, device="cuda")
    idx = torch.full((4, 200), -7, dtype=torch.int32, device="cuda")
    score = torch.full((4, 200), 3.0, dtype=torch.float32, device="cuda")
    ok = dict(db=db.data_ptr(), dtype=_hip.DTYPE_F32, n=32, D=16, zp=0, db_inv=inv.data_ptr(), q=db.data_ptr(), Q=4, q_inv=inv.data_ptr(), metric=0,
              g_db=None, g_q=None, k=5, idx=idx.data_ptr(), score=score.data_ptr())

    def call(**kw):
        a = dict(ok, **kw)
        return ctx.lib.bn_search_topk(ctx.handle, a["db"], a["dtype"], a["n"], a["D"], a["zp"], a["db_inv"], a["q"], a["Q"], a["q_inv"], a["metric"], a["g_db"],
                                      a["g_q"], a["k"], a["idx"], a["score"], None)

    bad = [dict(k=0), dict(k=_hip.SEARCH_MAX_K + 1), dict(D=_hip.SEARCH_MAX_D + 1), dict(D=0), dict(db=None), dict(q=None), dict(idx=None), dict(score=None),
           dict(db_inv=None), dict(q_inv=None), dict(metric=2), dict(metric=-1), dict(dtype=2), dict(dtype=-1), dict(n=-1), dict(n=1 << 31),
           dict(g_db=inv.data_ptr())]
    for kw in bad:
        assert call(**kw) == -1, kw   # BN_ERR_ARG
        assert ctx.lib.bn_last_error(), kw
    assert ctx.lib.bn_search_inv_norms(ctx.handle, None, 0, 32, 16, 0, inv.data_ptr(), None) == -1
    assert ctx.lib.bn_search_inv_norms(ctx.handle, db.data_ptr(), 3, 32, 16, 0, inv.data_ptr(), None) == -1
    assert ctx.lib.bn_search_inv_norms(ctx.handle, db.data_ptr(), 0, 32, _hip.SEARCH_MAX_D + 1, 0, inv.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((score == 3.0).all()) and bool((inv == 1.0).all()), "a refused call wrote to its outputs"
    assert call(db_inv=None, q_inv=None, metric=1) == 0   # the inverse norms may be NULL for dot
    torch.cuda.synchronize()
    assert idx.view(-1)[:20].view(4, 5).cpu().numpy().tolist() == [[0, 1, 2, 3, 4]] * 4   # all scores 0: the first rows, by index


# ------------------------------------------------------------------------------------------------------------------- end to end
SR = 22050   # the shipped model's config


def _write_wav(path, x):
    pcm = np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(SR)
        w.writeframes(pcm.tobytes())


def _tone(freq, seconds=3.0):
    t = np.arange(int(SR * seconds)) / SR
    return 0.5 * np.sin(2 * np.pi * freq * t) + 0.02 * np.sin(2 * np.pi * 3.1 * freq * t)


@pytest.mark.parametrize("model,dtype", [(TFLITE_PATH, "int8"), (KERAS_PATH, "float32")], ids=["int8", "float32"])
def test_embed_then_search_end_to_end(torch_mod, tmp_path, model, dtype):
    from birdnet_stm32.cli import embed as embed_cli
    from birdnet_stm32.cli import search as search_cli
    from birdnet_stm32.evaluation.search import EmbeddingIndex, search_reference
    from birdnet_stm32.models.runners import load_model_runner

    freqs = [700.0, 1500.0, 2600.0, 4100.0]
    paths = []
    for i, f in enumerate(freqs):
        paths.append(str(tmp_path / f"tone{i}.wav"))
        _write_wav(paths[-1], _tone(f))
    long_path = str(tmp_path / "long.wav")
    _write_wav(long_path, np.concatenate([_tone(5200.0), _tone(freqs[1]), _tone(900.0)]))   # tone1 is its chunk at 3 s
    ext = os.path.splitext(model)[1]
    ckpt = tmp_path / ("m" + ext)
    ckpt.write_bytes(open(model, "rb").read())
    (tmp_path / "m_model_config.json").write_text(open(CONFIG_PATH).read())
    runner = load_model_runner(str(ckpt), max_batch=64)
    try:
        db_npz, q_npz = str(tmp_path / "db.npz"), str(tmp_path / "q.npz")
        embed_cli.main(["--model_path", str(ckpt), "--input", *paths, long_path, "--output", db_npz, "--dtype", dtype], runner=runner)
        embed_cli.main(["--model_path", str(ckpt), "--input", paths[1], "--output", q_npz, "--dtype", dtype], runner=runner)
        index = EmbeddingIndex.from_npz(db_npz)
        assert len(index) == len(freqs) + 3 and index.dtype == dtype

        def run(out, *extra):
            search_cli.main(["--model_path", str(ckpt), "--database", db_npz, "--output", str(tmp_path / out), "--top_k", "3", *extra], runner=runner)
            with open(tmp_path / out, newline="") as f:
                rows = list(csv.reader(f))
            assert tuple(rows[0]) == search_cli.CSV_COLUMNS
            return rows[1:]

        hits = run("hits.csv", "--query", paths[1])
        assert len(hits) == 3 and [int(r[2]) for r in hits] == [1, 2, 3] and all(r[0] == paths[1] and float(r[1]) == 0.0 for r in hits)
        # the query's own recording first, with cosine 1.  int8: dot = n exactly, so fl(fl(n inv) inv) is within 4 u of 1 (the roundings of
        # the two inverse norms and of the two products); float32: dot and n are sums in different orders, the bound of _score_bound
        # with sum |x q| inv inv = S = 1.  The CSV holds 7 significant digits: 5e-8 more.
        tol = (4 if dtype == "int8" else (index.dim + 2) + (index.dim + 8)) * U * 1.01 + 5e-8
        assert hits[0][4] == paths[1] and float(hits[0][5]) == 0.0 and float(hits[0][6]) == 3.0 and abs(float(hits[0][3]) - 1.0) <= tol
        want_i, want_s = search_reference(index.embeddings, index.embeddings[1:2], 3, "cosine", zero_point=index.zero_point)
        assert want_i[0, 0] == 1
        if dtype == "int8":
            assert [float(r[3]) for r in hits] == [float(f"{s:.7g}") for s in want_s[0]]
        # ... and without it the same call inside the longer recording
        excl = run("excl.csv", "--query", paths[1], "--exclude_same_file")
        assert all(r[4] != paths[1] for r in excl) and excl[0][4] == long_path and float(excl[0][5]) == 3.0 and float(excl[0][6]) == 6.0
        assert [r[4:] for r in excl[:2]] == [r[4:] for r in hits[1:]]
        # rows already embedded give the same hits
        assert run("npz.csv", "--query_npz", q_npz) == hits
        search_cli.main(["--database", db_npz, "--query_npz", q_npz, "--chunk_duration", "3", "--output", str(tmp_path / "nomodel.csv"), "--top_k", "3"])
        assert open(tmp_path / "nomodel.csv").read() == open(tmp_path / "hits.csv").read()
    finally:
        runner.close()
