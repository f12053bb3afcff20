"""CPU tests of projection: the numpy specification (``conditional_p_reference``, ``symmetrize``, ``gradient_reference``,
``update_reference``, ``tsne_reference``) against scikit-learn and on hand-made cases, every refusal, and the ``project`` command's parser
and writers."""

import csv
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import project_cases as cases
from conftest import PKG


def test_module_needs_no_torch_at_import():
    code = "import sys; import birdnet_stm32.evaluation.project, birdnet_stm32.cli.project; assert 'torch' not in sys.modules"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def _dense_case(n=50, seed=0):
    """A dense P (k = n - 1: the sparse matrix is the dense one) and a map of unit scale."""
    from birdnet_stm32.evaluation.project import symmetrize

    rng = np.random.default_rng(seed)
    p_cond = rng.random((n, n - 1))
    p_cond /= p_cond.sum(axis=1, keepdims=True)
    idx = np.array([[j for j in range(n) if j != i] for i in range(n)])
    return symmetrize(idx, p_cond, n), rng.standard_normal((n, 2))


def test_gradient_and_divergence_against_scikit_learn():
    """Both are float64 and differ in the summation order only: 1e-12 relative, element by element."""
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _kl_divergence

    from birdnet_stm32.evaluation.project import gradient_reference

    n = 50
    (rowptr, col, val), Y = _dense_case(n)
    assert rowptr[-1] == n * (n - 1)
    dense = np.zeros((n, n))
    dense[np.repeat(np.arange(n), np.diff(rowptr)), col] = val.astype(np.float64)
    kl, grad = _kl_divergence(Y.ravel(), squareform(dense, checks=False), 1, n, 2)
    got = gradient_reference(Y, rowptr, col, val, exaggeration=1.0)
    print("kl", kl, got.kl, "largest relative gradient difference", np.max(np.abs(got.grad - grad.reshape(n, 2)) / np.abs(grad.reshape(n, 2))))
    assert abs(got.kl - kl) <= 1e-12 * abs(kl)
    assert np.all(np.abs(got.grad - grad.reshape(n, 2)) <= 1e-12 * np.abs(grad.reshape(n, 2)))
    # exaggeration scales the attraction alone; the absolute sums bound their sums
    g12 = gradient_reference(Y, rowptr, col, val, exaggeration=12.0)
    assert np.allclose(g12.grad, 4 * (12 * got.A - got.R / got.Z), rtol=1e-14, atol=0) and g12.kl == got.kl
    assert (np.abs(got.A) <= got.abs_A).all() and (np.abs(got.R) <= got.abs_R).all() and (np.abs(got.kl_rows) <= got.abs_kl * (1 + 1e-15)).all()
    assert got.Z == got.z_rows.sum() and abs(got.p_sum - 1) < 1e-6


def test_conditional_affinities_sum_to_one_at_the_asked_entropy():
    from birdnet_stm32.evaluation.project import conditional_p_reference, neighbours_reference

    rows = cases.three_clusters()
    for perplexity in (5.0, 30.0):
        k = min(rows.shape[0] - 1, int(3 * perplexity))
        idx, score = neighbours_reference(rows, k)
        p, beta = conditional_p_reference(score, perplexity)
        assert p.shape == (300, k) and (beta > 0).all() and np.isfinite(beta).all()
        assert np.abs(p.sum(axis=1) - 1).max() <= 1e-12
        H = -(p * np.log(np.where(p > 0, p, 1))).sum(axis=1)
        assert np.abs(H - math.log(perplexity)).max() <= 1e-5 + 1e-12
    # equidistant neighbours are uniform whatever beta; a single neighbour has probability 1
    p, beta = conditional_p_reference(np.full((2, 6), 0.25, np.float32), 2.0)
    assert np.array_equal(p, np.full((2, 6), 1 / 6)) and (beta == 2.0 ** 99).all()
    p, _ = conditional_p_reference(np.array([[0.5]], np.float32), 1.0)
    assert p.tolist() == [[1.0]]


def test_symmetrize_is_symmetric_sums_to_one_and_holds_the_union():
    from birdnet_stm32.evaluation.project import conditional_p_reference, neighbours_reference, symmetrize

    rows = cases.three_clusters()
    n = rows.shape[0]
    idx, score = neighbours_reference(rows, 15)
    p, _ = conditional_p_reference(score, 5.0)
    rowptr, col, val = symmetrize(idx, p.astype(np.float32), n)
    assert rowptr.dtype == np.int64 and col.dtype == np.int32 and val.dtype == np.float32 and rowptr[0] == 0 and rowptr[-1] == col.size == val.size
    dense = np.zeros((n, n), np.float32)
    pattern = np.zeros((n, n), bool)
    for i in range(n):
        c = col[rowptr[i]:rowptr[i + 1]]
        assert (np.diff(c) > 0).all() and (c != i).all()
        dense[i, c] = val[rowptr[i]:rowptr[i + 1]]
        pattern[i, c] = True
    assert np.array_equal(dense, dense.T)
    assert abs(float(val.astype(np.float64).sum()) - 1.0) <= 1e-6
    knn = np.zeros((n, n), bool)
    knn[np.repeat(np.arange(n), 15), idx.ravel()] = True
    assert np.array_equal(pattern, knn | knn.T) and (knn != knn.T).any()
    pc = np.zeros((n, n))
    pc[np.repeat(np.arange(n), 15), idx.ravel()] = p.astype(np.float32).astype(np.float64).ravel()
    want = ((pc + pc.T) / (2 * n)).astype(np.float32)
    assert np.array_equal(dense, want)
    # a hand-made case: an empty row, a dropped -1, a one-sided and a two-sided pair
    rowptr, col, val = symmetrize(np.array([[1, 2], [0, -1], [1, -1], [-1, -1]]), np.array([[0.5, 0.5], [1, 0], [1, 0], [0, 0]]), 4)
    assert rowptr.tolist() == [0, 2, 4, 6, 6] and col.tolist() == [1, 2, 0, 2, 0, 1]
    assert val.tolist() == [np.float32(1.5 / 8), np.float32(0.5 / 8), np.float32(1.5 / 8), np.float32(1 / 8), np.float32(0.5 / 8), np.float32(1 / 8)]


def _sklearn_step(p, grad, update, gains, lr, momentum):
    """The body of sklearn.manifold._t_sne._gradient_descent (1.7), on float32 arrays."""
    inc = update * grad < 0.0
    dec = np.invert(inc)
    gains[inc] += np.float32(0.2)
    gains[dec] *= np.float32(0.8)
    np.clip(gains, np.float32(0.01), np.inf, out=gains)
    grad = grad * gains
    update = np.float32(momentum) * update - np.float32(lr) * grad
    p = p + update
    return p, update, gains


def test_update_is_scikit_learns_rule():
    from birdnet_stm32.evaluation.project import update_reference

    #                update * grad:   < 0     > 0     == 0 (zero update)  == 0 (zero gradient)  > 0, gains at the floor   < 0
    Y = np.array([[1.0, -2.0], [0.5, 0.25], [3.0, 1e-3]], np.float32)
    grad = np.array([[0.5, 0.5], [0.3, 0.0], [1e-4, -2.0]], np.float32)
    update = np.array([[-1.0, 2.0], [0.0, 0.7], [1e-5, 0.125]], np.float32)
    gains = np.array([[1.0, 1.0], [2.5, 0.3], [0.01, 0.01]], np.float32)
    for lr, momentum in ((200.0, 0.5), (50.0, 0.8)):
        y1, u1, g1 = update_reference(Y, grad, update, gains, lr, momentum)
        y2, u2, g2 = _sklearn_step(Y.copy(), grad.copy(), update.copy(), gains.copy(), lr, momentum)
        for a, b in ((y1, y2), (u1, u2), (g1, g2)):
            assert a.dtype == np.float32 and b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert g1.ravel().tolist() == [np.float32(1.2), np.float32(0.8), np.float32(2.5) * np.float32(0.8), np.float32(0.3) * np.float32(0.8), np.float32(0.01),
                                   np.float32(0.01) + np.float32(0.2)]


def test_refusals():
    from birdnet_stm32.evaluation.project import check_project_args, tsne_reference

    check_project_args(100, 30, 1000, 12, 250, None)
    for kw, what in ((dict(n=1), "at least 2"), (dict(perplexity=0.5), "perplexity"), (dict(perplexity=float("nan")), "perplexity"),
                     (dict(n=20, perplexity=20), "below the number"), (dict(perplexity=43), "perplexity"), (dict(n_iter=-1), "n_iter"),
                     (dict(early_exaggeration=0.5), "early_exaggeration"), (dict(learning_rate=0.0), "learning_rate"), (dict(kl_every=-1), "kl_every")):
        a = dict(n=100, perplexity=30, n_iter=1000, early_exaggeration=12, exaggeration_iter=250, learning_rate=None, kl_every=0)
        a.update(kw)
        with pytest.raises(ValueError, match=what):
            check_project_args(**a)
    x = np.zeros((5, 4), np.float32)
    x[0, 0] = 1
    with pytest.raises(ValueError, match="at least 2"):
        tsne_reference(x, perplexity=1)   # one non-zero row
    with pytest.raises(ValueError, match="not finite"):
        tsne_reference(np.full((5, 4), np.inf, np.float32))


def test_zero_rows_come_back_nan_and_int8_rows_are_taken():
    from birdnet_stm32.evaluation.project import tsne_reference

    rng = np.random.default_rng(3)
    x = rng.standard_normal((12, 8)).astype(np.float32)
    x[4] = 0
    res = tsne_reference(x, perplexity=3, n_iter=20, exaggeration_iter=10)
    assert res.xy.shape == (12, 2) and res.xy.dtype == np.float32 and np.isnan(res.xy[4]).all() and np.isnan(res.beta[4])
    live = np.delete(np.arange(12), 4)
    assert np.isfinite(res.xy[live]).all() and np.abs(res.xy[live].astype(np.float64).mean(axis=0)).max() < 1e-6
    assert res.kl_history == [(20, res.kl)] and res.n_iter == 20
    alone = tsne_reference(x[live], perplexity=3, n_iter=20, exaggeration_iter=10)
    assert np.array_equal(alone.xy, res.xy[live])
    q = rng.integers(-128, 128, (12, 8)).astype(np.int8)
    q[7] = -3
    r8 = tsne_reference(q, perplexity=3, n_iter=5, zero_point=-3)
    assert np.isnan(r8.xy[7]).all() and np.isfinite(np.delete(r8.xy, 7, axis=0)).all()


def test_reference_separates_three_clusters():
    """500 iterations on 3 x 100 well-separated rows: the divergence falls after the exaggeration ends, and every point's nearest
    neighbour in the map is one of its own cluster."""
    res = cases.reference_fit()
    its = [it for it, _ in res.kl_history]
    assert its == [250, 500] and res.kl == res.kl_history[-1][1]
    print("kl", res.kl_history)
    assert res.kl_history[1][1] < res.kl_history[0][1]
    assert cases.same_cluster_share(res.xy, cases.cluster_of_rows()) == 1.0
    assert sorted(res.trajectory) == [100, 250, 500] and all(v.shape == (300, 2) and v.dtype == np.float32 for v in res.trajectory.values())


def test_parser_defaults_refusals_and_dispatch(tmp_path):
    import birdnet_stm32.__main__ as m
    from birdnet_stm32.cli.project import build_parser, main, validate_args

    db = tmp_path / "db.npz"
    db.write_bytes(b"")
    base = ["--database", str(db), "--output", "map.csv"]
    args = build_parser().parse_args(base)
    assert (args.perplexity, args.n_iter, args.early_exaggeration, args.exaggeration_iter, args.learning_rate, args.seed, args.chunk_duration, args.npz_out,
            args.device) == (30.0, 1000, 12.0, 250, None, 42, 0.0, "", 0)
    validate_args(args)
    for extra, what in ((["--perplexity", "0.5"], "--perplexity"), (["--perplexity", "43"], "--perplexity"), (["--n_iter", "-1"], "n_iter"),
                        (["--exaggeration_iter", "-1"], "exaggeration_iter"), (["--early_exaggeration", "0"], "early_exaggeration"),
                        (["--learning_rate", "0"], "learning_rate"), (["--learning_rate", "nan"], "learning_rate"), (["--chunk_duration", "-1"], "chunk_duration")):
        with pytest.raises(SystemExit, match=what):
            main(base + extra)
    with pytest.raises(SystemExit, match="not found"):
        main(["--database", str(tmp_path / "none.npz"), "--output", "m.csv"])
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--database", str(db)])   # --output is required
    assert "project" in m.USAGE and "project" in m.__doc__
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "birdnet_stm32", "project", "--help"], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "--database" in r.stdout and "--perplexity" in r.stdout and "--npz_out" in r.stdout and "--exaggeration_iter" in r.stdout


def test_writers(tmp_path):
    from birdnet_stm32.cli.project import CSV_COLUMNS, write_map_archive, write_map_csv
    from birdnet_stm32.evaluation.project import ProjectionResult
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    emb = np.eye(3, 4, dtype=np.float32)
    index = EmbeddingIndex(emb, [0, 0, 1], [0.0, 3.0, 0.0], ["a.wav", "b.wav"])
    xy = np.array([[1.5, -2.25], [np.nan, np.nan], [0.0, 1e-3]], np.float32)
    res = ProjectionResult(xy, 0.5, [(10, 0.5)], np.array([1.0, np.nan, 2.0]), 10)
    out = str(tmp_path / "map.csv")
    assert write_map_csv(out, index, res, 3.0) == 3
    lines = list(csv.reader(open(out)))
    assert tuple(lines[0]) == CSV_COLUMNS == ("path", "start_s", "end_s", "x", "y")
    assert lines[1:] == [["a.wav", "0.000", "3.000", "1.5", "-2.25"], ["a.wav", "3.000", "6.000", "", ""], ["b.wav", "0.000", "3.000", "0", "0.001"]]
    npz = str(tmp_path / "map_out")
    write_map_archive(npz, index, res)
    with np.load(npz, allow_pickle=False) as z:
        assert np.array_equal(z["xy"], xy, equal_nan=True) and z["paths"].tolist() == ["a.wav", "b.wav"] and z["file_index"].tolist() == [0, 0, 1]
        assert float(z["kl"]) == 0.5 and np.array_equal(z["beta"], res.beta, equal_nan=True)


def test_abi_constants_stay_in_step():
    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation import project

    hdr = open(os.path.join(os.path.dirname(PKG), "include", "birdnet_hip.h")).read()
    val = {k: eval(v) for k, v in re.findall(r"#define (BN_TSNE_\w+) \(?([\d\*< ]+?)\)? *(?:/\*.*)?\n", hdr)}
    assert (val["BN_TSNE_TILE_I"], val["BN_TSNE_TILE_J"], val["BN_TSNE_SPLIT_J"], val["BN_TSNE_ROW_LANES"], val["BN_TSNE_MAX_K"], val["BN_TSNE_MAX_N"]) == \
        (_hip.TSNE_TILE_I, _hip.TSNE_TILE_J, _hip.TSNE_SPLIT_J, _hip.TSNE_ROW_LANES, _hip.TSNE_MAX_K, _hip.TSNE_MAX_N)
    assert val["BN_TSNE_MAX_PERPLEXITY_STEPS"] == project.PERPLEXITY_STEPS == 100 and project.MAX_N == _hip.TSNE_MAX_N and _hip.TSNE_MAX_K == _hip.SEARCH_MAX_K
    assert {"bn_tsne_perplexity", "bn_tsne_gradient", "bn_tsne_update"} <= set(_hip.EXPORTS)
    for name in ("bn_tsne_perplexity", "bn_tsne_gradient", "bn_tsne_update"):
        assert re.search(r"BN_API int " + name + r"\(", hdr)
