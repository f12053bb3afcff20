"""CPU tests of reduction: the numpy specification (evaluation/reduce.py) against scikit-learn and hand-computed cases, the model file, the
PCA start of ``project`` and the command line.

Tolerances against scikit-learn's ``PCA(svd_solver="full")`` (run in float64 on the same values) come from the float32 centring, the only
place where the specification leaves float64: ``c = fl32(x - fl32(mu))`` differs from ``x - mu`` by at most ``E_id = 2^-24 (|mu_d| + |c_id|)``
per element.  Propagated: ``||dG||_F <= 2 ||C||_F ||E||_F + ||E||_F^2``; a component turns by ``sin <= 2 ||dG||_F / gap_k`` (Davis-Kahan), so
it moves by at most ``sqrt(2)`` times that as a vector, plus 2^-24 for its float32 storage; an explained variance moves by
``||dG||_F / lambda_k`` relative (Weyl); a score by ``||c_i|| ||dv_k|| + sum_d |W_kd| E_id + 2^-24 |y_ik|``.  ``SLACK`` covers the float64
arithmetic of both sides (eigh against SVD: some hundred float64 roundings on unit-scale quantities).
"""

import os
import re

import numpy as np
import pytest

import reduce_cases as cases
from birdnet_stm32.evaluation import reduce as R

U = 2.0 ** -24
SLACK = 1e-11


def _sklearn_bounds(x64, mean, r):
    """``(dv [r], dvar_rel [r], dscore [n, r])`` of the module docstring for live rows ``x64`` (real units) and the specification's mean."""
    c = x64 - mean
    E = U * (np.abs(mean)[None, :] + np.abs(c))
    nE, nC = np.linalg.norm(E), np.linalg.norm(c)
    dG = 2 * nC * nE + nE * nE
    lam = np.linalg.eigvalsh(c.T @ c)[::-1]
    gaps = np.array([min(abs(lam[k] - lam[j]) for j in range(lam.size) if j != k) for k in range(r)])
    dv = np.sqrt(2.0) * 2 * dG / gaps + U + SLACK
    return dv, dG / lam[:r] + SLACK, c, E, dv


def _against_sklearn(rows, zero_point, scale, r, whiten):
    from sklearn.decomposition import PCA

    model, scores = R.pca_reference(rows, zero_point, scale, r, whiten)
    rows_, live = R.live_rows(rows, zero_point)
    x64 = (rows_[live].astype(np.float64) - zero_point) * scale
    sk = PCA(n_components=r, svd_solver="full", whiten=whiten).fit(x64)
    dv, dvar, c, E, _ = _sklearn_bounds(x64, model.mean * scale, r)
    assert dv.max() < 0.05, "the input's gaps make the comparison vacuous"
    comp = model.components.astype(np.float64)
    assert (np.sign(comp[np.arange(r), np.abs(comp).argmax(axis=1)]) > 0).all()
    assert ((comp * sk.components_).sum(axis=1) > 0).all(), "a sign differs from scikit-learn's"
    assert (np.abs(comp - sk.components_).max(axis=1) <= dv).all()
    assert (np.abs(model.explained_variance / sk.explained_variance_ - 1) <= dvar).all()
    assert abs(model.total_variance / (sk.explained_variance_.sum() + sk.noise_variance_ * (x64.shape[1] - r)) - 1) <= dvar.max() + 1e-9
    assert np.allclose(model.explained_variance_ratio, sk.explained_variance_ratio_, rtol=2 * dvar.max() + 1e-9, atol=0)
    W = np.abs(sk.components_)
    dscore = np.linalg.norm(c, axis=1)[:, None] * dv[None, :] + E @ W.T
    want = sk.transform(x64)
    if whiten:
        dscore = dscore / np.sqrt(sk.explained_variance_)[None, :] + np.abs(want) * dvar[None, :]
    dscore = dscore + U * np.abs(want) + SLACK
    assert (np.abs(scores[live] - want) <= dscore).all()
    assert not scores[np.setdiff1d(np.arange(rows.shape[0]), live)].any()
    return model, scores


@pytest.mark.parametrize("whiten", [False, True])
def test_reference_matches_scikit_learn_on_the_planted_spectrum(whiten):
    _against_sklearn(cases.planted_rows(), 0, 1.0, 8, whiten)


@pytest.mark.parametrize("whiten", [False, True])
def test_reference_matches_scikit_learn_with_duplicates_and_a_zero_row(whiten):
    x = cases.planted_rows(300, 12, 3)
    x = np.concatenate([x, x[:100], np.zeros((1, 12), np.float32), x[50:60]])
    model, scores = _against_sklearn(x, 0, 1.0, 5, whiten)
    assert model.n_rows == 410 and np.array_equal(scores[50], scores[401]) and not scores[400].any()


@pytest.mark.parametrize("whiten", [False, True])
def test_reference_matches_scikit_learn_on_int8(whiten):
    scale, zp = 0.11, -100
    b = cases.int8_features(500, 16, 3, scale, zp)
    b[17] = zp
    model, _ = _against_sklearn(b, zp, scale, 5, whiten)
    assert model.dtype == "int8" and model.scale == scale and model.zero_point == zp and model.n_rows == 499


# ------------------------------------------------------------------------------------------------------------ hand-computed cases
def test_two_dimensional_case():
    """Four points around (5, 5): G = diag(8, 2), the components are the axes, the scores the centred rows."""
    x = np.array([[7, 5], [3, 5], [5, 6], [5, 4]], np.float32)
    model, scores = R.pca_reference(x, n_components=2)
    assert np.array_equal(model.mean, [5.0, 5.0]) and np.array_equal(model.components, np.eye(2, dtype=np.float32))
    assert np.array_equal(model.explained_variance, [8 / 3, 2 / 3]) and model.total_variance == 8 / 3 + 2 / 3 and model.n_rows == 4
    assert np.array_equal(scores, x - 5) and np.array_equal(model.weights, model.components)
    white, ws = R.pca_reference(x, n_components=2, whiten=True)
    assert np.allclose(ws.astype(np.float64), (x - 5) / np.sqrt([8 / 3, 2 / 3]), rtol=2 * U, atol=0)
    assert np.allclose(ws.astype(np.float64).var(axis=0, ddof=1), 1.0, rtol=4 * U)
    m8, s8 = R.pca_reference((x + 10).astype(np.int8), zero_point=10, scale=0.5, n_components=2)
    assert np.array_equal(m8.mean, [5.0, 5.0]) and np.array_equal(m8.explained_variance, [8 / 3 * 0.25, 2 / 3 * 0.25])
    assert np.array_equal(m8.weights, 0.5 * np.eye(2, dtype=np.float32)) and np.array_equal(s8, 0.5 * (x - 5))


def test_sign_rule_on_a_tie():
    from sklearn.utils.extmath import svd_flip

    V = np.array([[-0.5, 0.5, 0.1], [0.2, -0.9, 0.9], [0.3, 0.1, -0.2], [0.0, 0.0, 0.0]])
    got = R.flip_signs(V)
    assert np.array_equal(got, [[0.5, -0.5, -0.1], [-0.2, 0.9, -0.9], [0.3, 0.1, -0.2], [0.0, 0.0, 0.0]])
    _, want = svd_flip(np.eye(4), V.copy(), u_based_decision=False)
    assert np.array_equal(got, want)
    _, comp = R.spectrum(np.array([[1.0, -1.0], [-1.0, 1.0]]))
    assert comp[0, 0] > 0 > comp[0, 1] and np.allclose(np.abs(comp[0]), np.sqrt(0.5))


def test_variance_picks_the_component_count():
    ratio = np.array([0.4, 0.3, 0.2, 0.1])
    assert [R.resolve_components(v, ratio, 4, 100) for v in (0.39, 0.41, 0.65, 0.75, 0.95)] == [1, 2, 2, 3, 4]
    assert R.resolve_components(0.999, ratio, 4, 3) == 2   # never more than min(D, n - 1)
    x = cases.planted_rows()
    full, _ = R.pca_reference(x, n_components=39)
    cum = np.cumsum(full.explained_variance_ratio)
    model, scores = R.pca_reference(x, n_components=0.95)
    r = model.n_components
    assert cum[r - 1] > 0.95 and (r == 1 or cum[r - 2] <= 0.95) and scores.shape == (1000, r)


def test_whitened_scores_have_unit_variance():
    model, scores = R.pca_reference(cases.planted_rows(), n_components=8, whiten=True)
    var = scores.astype(np.float64).var(axis=0, ddof=1)
    # the scores are W c with W = v / sqrt(lambda / (n - 1)) and lambda = v^T (sum c c^T) v, so their second moment about 0 is n - 1 up to
    # the float32 roundings of W and of the scores (4 u relative on a square), and their mean is (sum c) v, of the order u |mu| sqrt(n)
    assert np.allclose(var, 1.0, rtol=1e-5, atol=0)


def test_whitening_refuses_a_component_without_variance():
    rng = np.random.default_rng(0)
    # integers of rank 2 after centring: the third eigenvalue is the float64 noise of eigh
    x = (rng.integers(-8, 9, (50, 2)) @ np.array([[1, 0, 1, 2, 0], [0, 1, 1, 0, 2]]) + 20).astype(np.float32)
    R.pca_reference(x, n_components=2, whiten=True)
    R.pca_reference(x, n_components=3, whiten=False)
    with pytest.raises(ValueError, match="component 2 "):
        R.pca_reference(x, n_components=3, whiten=True)


def test_component_limits_and_live_rows():
    x = cases.planted_rows(10, 6, 1)
    for bad in (0, 7, -1, 1.0, 0.0, -0.5, 1.5, True):
        with pytest.raises(ValueError, match="n_components"):
            R.pca_reference(x, n_components=bad)
    assert R.pca_reference(x, n_components=6)[0].n_components == 6
    with pytest.raises(ValueError, match="outside 1..3"):
        R.pca_reference(x[:4], n_components=4)
    one = np.zeros((5, 6), np.float32)
    one[2] = 1
    with pytest.raises(ValueError, match="at least 2"):
        R.pca_reference(one, n_components=1)
    with pytest.raises(ValueError, match="at least 2"):
        R.pca_reference(np.full((5, 6), 3, np.int8), zero_point=3, n_components=1)
    with pytest.raises(ValueError, match="all equal"):
        R.pca_reference(np.ones((5, 6), np.float32), n_components=1)
    with pytest.raises(ValueError, match="not finite"):
        R.pca_reference(np.full((5, 6), np.nan, np.float32), n_components=1)


def test_bounds_are_what_the_docstrings_state():
    c = np.array([[1.0, -2.0], [3.0, 4.0]])
    assert np.array_equal(R.gram_entry_bound(c), 257 * U * np.array([[10.0, 14.0], [14.0, 20.0]]))
    assert np.array_equal(R.transform_bound(c, np.array([[1.0, -1.0]])), 4 * U * np.array([[3.0], [7.0]]))
    assert "(BN_PCA_RUN_ROWS + 1) 2^-24" in R.__doc__ and "(D + 2) 2^-24" in R.__doc__ and "BEFORE the products" in R.__doc__


# -------------------------------------------------------------------------------------------------------------------- model file
def _index(rows, zero_point=0, scale=1.0):
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    n = rows.shape[0]
    return EmbeddingIndex(rows, np.zeros(n, np.int64), 3.0 * np.arange(n), ["a.wav"], "int8" if rows.dtype == np.int8 else "float32", scale, zero_point)


def test_model_round_trip_and_refusals(tmp_path):
    b = cases.int8_features(100, 8, 2, 0.11, -100)
    model, _ = R.pca_reference(b, -100, 0.11, 3, True)
    path = str(tmp_path / "pca.npz")
    model.save(path)
    back = R.PcaModel.load(path)
    for name in ("mean", "components", "weights", "explained_variance"):
        a, c = getattr(model, name), getattr(back, name)
        assert a.dtype == c.dtype and a.tobytes() == c.tobytes()
    assert (back.total_variance, back.n_rows, back.whiten, back.dtype, back.scale, back.zero_point) == (model.total_variance, 100, True, "int8", 0.11, -100)
    with np.load(path, allow_pickle=False) as z:
        good = {k: z[k] for k in z.files}
    bad_path = str(tmp_path / "bad.npz")
    for key in R.MODEL_KEYS:
        np.savez(bad_path, **{k: v for k, v in good.items() if k != key})
        with pytest.raises(ValueError, match=f"no {key}"):
            R.PcaModel.load(bad_path)
    for change, match in ((dict(weights=good["weights"][:2]), "weights"), (dict(mean=good["mean"][:5]), "mean"), (dict(dtype=np.asarray("float16")), "dtype"),
                          (dict(explained_variance=good["explained_variance"][::-1].copy()), "descending"), (dict(components=good["components"].astype(np.float64)), "float32"),
                          (dict(n_rows=np.int64(3)), "components from"), (dict(total_variance=np.float64(1e-9)), "total_variance"), (dict(scale=np.float64(0)), "scale"),
                          (dict(mean=np.full(8, np.nan)), "not finite"), (dict(dtype=np.asarray("float32")), "float32 model")):
        np.savez(bad_path, **{**good, **change})
        with pytest.raises(ValueError, match=match):
            R.PcaModel.load(bad_path)
    R.check_model_applies(model, _index(b, -100, 0.11))
    for index, match in ((_index(b[:, :7].copy(), -100, 0.11), "8 x int8"), (_index(b.astype(np.float32)), "8 x int8"), (_index(b, -100, 0.12), "scale"),
                         (_index(b, -99, 0.11), "zero point")):
        with pytest.raises(ValueError, match=match):
            R.check_model_applies(model, index)


# ---------------------------------------------------------------------------------------------------------------- project --init pca
def test_initial_map_pca_is_scikit_learns_formula():
    from birdnet_stm32.evaluation.project import initial_map_pca

    _, scores = R.pca_reference(cases.planted_rows(200, 10, 2), n_components=3)
    got = initial_map_pca(scores)
    want = scores[:, :2] / np.std(scores[:, 0]) * 1e-4   # sklearn/manifold/_t_sne.py, in float32 there
    assert got.dtype == np.float32 and got.shape == (200, 2) and np.allclose(got, want, rtol=4 * U, atol=0)
    exact = (scores[:, :2].astype(np.float64) / scores[:, 0].astype(np.float64).std() * 1e-4).astype(np.float32)
    assert np.array_equal(got, exact)
    with pytest.raises(ValueError, match="at least 3"):
        initial_map_pca(scores[:2])
    with pytest.raises(ValueError, match="2 components"):
        initial_map_pca(scores[:, :1])
    with pytest.raises(ValueError, match="positive variance"):
        initial_map_pca(np.stack([np.arange(5.0), np.zeros(5)], axis=1))


def test_random_start_is_unchanged_and_pca_start_is_seedless():
    """``init="random"`` is the fit as it was before the argument existed, composed here from the module's own steps; ``init="pca"`` starts
    from the scores and ignores the seed."""
    from birdnet_stm32.evaluation import project as P

    rows, _ = cases.three_clusters(per=10, D=8)
    rows = np.insert(rows, 4, 0.0, axis=0)
    kw = dict(perplexity=5, n_iter=30, exaggeration_iter=10, seed=11)
    got = P.tsne_reference(rows, init="random", **kw)
    live = np.ascontiguousarray(np.delete(rows, 4, axis=0))
    idx, score = P.neighbours_reference(live, P.neighbour_count(30, 5))
    p_cond, beta = P.conditional_p_reference(score, 5)
    b = P._NumpyBackend(P.symmetrize(idx, p_cond.astype(np.float32), 30), P.initial_map(30, 11))
    kl, _, _ = P._descend(b, 30, 30, 12, 10, P.default_learning_rate(30, 12), 0)
    want = P._finish(31, np.delete(np.arange(31), 4), b.Y, beta, kl, [], {}, 30)
    assert np.array_equal(got.xy.view(np.uint32), want.xy.view(np.uint32)) and got.kl == want.kl
    assert np.array_equal(P.tsne_reference(rows, **kw).xy.view(np.uint32), got.xy.view(np.uint32))
    a = P.tsne_reference(rows, init="pca", snapshots=(0,), **kw)
    model, scores = R.pca_reference(live, n_components=2)
    assert np.array_equal(a.trajectory[0], P.initial_map_pca(scores))
    assert np.array_equal(P.tsne_reference(rows, init="pca", **{**kw, "seed": 12}).xy.view(np.uint32), a.xy.view(np.uint32))
    assert not np.array_equal(a.xy.view(np.uint32), got.xy.view(np.uint32))
    with pytest.raises(ValueError, match="init must be"):
        P.tsne_reference(rows, init="spectral", **kw)
    two = np.zeros((4, 8), np.float32)
    two[0, 0] = two[1, 1] = 1
    with pytest.raises(ValueError):
        P.tsne_reference(two, perplexity=1, init="pca")
    line = np.outer(np.arange(1.0, 9.0), np.ones(8)).astype(np.float32)   # one component only
    with pytest.raises(ValueError, match="positive variance"):
        P.tsne_reference(line, perplexity=2, n_iter=1, init="pca")


# ------------------------------------------------------------------------------------------------------------------ command line
def test_command_line_parsing_and_refusals(tmp_path):
    from birdnet_stm32.cli import project as project_cli
    from birdnet_stm32.cli import reduce as cli

    db, out, pca = str(tmp_path / "db.npz"), str(tmp_path / "r.npz"), str(tmp_path / "pca.npz")
    rows = cases.planted_rows(20, 8, 1)
    cases.write_archive(db, rows)
    p = cli.build_parser()
    a = p.parse_args(["--database", db, "--output", out])
    assert a.components is None and a.variance is None and not a.whiten and a.model == "" and a.device == 0
    cli.validate_args(a)
    assert cli.requested_components(a, _index(rows), 20) == 8 and cli.requested_components(a, _index(rows), 5) == 4
    a = p.parse_args(["--database", db, db, "--output", out, "--variance", "0.9", "--whiten", "--model_out", pca, "--variance_out", "v.csv"])
    cli.validate_args(a)
    assert cli.requested_components(a, _index(rows), 20) == 0.9 and a.database == [db, db]
    assert cli.requested_components(p.parse_args(["--database", db, "--output", out, "--components", "3"]), _index(rows), 20) == 3
    model, _ = R.pca_reference(rows, n_components=2)
    model.save(pca)
    cli.validate_args(p.parse_args(["--database", db, "--output", out, "--model", pca]))
    for extra, match in ((["--components", "4", "--variance", "0.5"], "mutually exclusive"), (["--components", "0"], "--components"), (["--variance", "1.0"], "--variance"),
                         (["--variance", "0"], "--variance"), (["--model", pca, "--whiten"], "--model applies"), (["--model", pca, "--components", "2"], "--model applies"),
                         (["--model", str(tmp_path / "none.npz")], "model not found")):
        with pytest.raises((ValueError, FileNotFoundError), match=match):
            cli.validate_args(p.parse_args(["--database", db, "--output", out] + extra))
    with pytest.raises(FileNotFoundError, match="archive not found"):
        cli.validate_args(p.parse_args(["--database", str(tmp_path / "none.npz"), "--output", out]))
    # refusals that need the archive come before a file is written, and before the device is touched
    narrow, lonely = str(tmp_path / "narrow.npz"), str(tmp_path / "lonely.npz")
    cases.write_archive(narrow, rows[:, :5].copy())
    one = np.zeros((6, 8), np.float32)
    one[1] = 1
    cases.write_archive(lonely, one)
    for argv, match in ((["--database", narrow, "--output", out, "--model", pca], "fitted on 8 x float32"), (["--database", lonely, "--output", out], "at least 2"),
                        (["--database", db, "--output", out, "--components", "4", "--variance", "0.5"], "mutually exclusive")):
        with pytest.raises(SystemExit, match=match):
            cli.main(argv)
        assert not os.path.exists(out)
    with open(pca, "wb") as f:
        np.savez(f, mean=np.zeros(8))
    with pytest.raises(SystemExit, match="not a model"):
        cli.main(["--database", db, "--output", out, "--model", pca])
    assert not os.path.exists(out)
    pp = project_cli.build_parser()
    assert pp.parse_args(["--database", db, "--output", "m.csv"]).init == "random" and pp.parse_args(["--database", db, "--output", "m.csv", "--init", "pca"]).init == "pca"
    with pytest.raises(SystemExit):
        pp.parse_args(["--database", db, "--output", "m.csv", "--init", "spectral"])


def test_dispatcher_knows_the_command():
    import birdnet_stm32.__main__ as m

    assert "reduce" in m.USAGE and "reduce" in m.__doc__


def test_binding_restates_the_header():
    from birdnet_stm32 import _hip

    with open(os.path.join(os.path.dirname(_hip.LIB_PATH), "..", "..", "include", "birdnet_hip.h")) as f:
        text = f.read()
    for name in ("MAX_D", "RUN_ROWS", "STAGE_ROWS", "MACRO", "GRAM_TARGET_WGS", "GRAM_MAX_RANGES", "COLSUM_COLS", "COLSUM_MIN_ROWS", "COLSUM_MAX_WGS", "MAX_TILE",
                 "STEP_ROWS", "MIN_WG_STEPS", "MAX_WGS"):
        assert int(re.search(rf"#define BN_PCA_{name} (\d+)", text).group(1)) == getattr(_hip, "PCA_" + name), name
    assert re.search(r"#define BN_PCA_LDS_BYTES \(160 \* 1024\)", text) and _hip.PCA_LDS_BYTES == 160 * 1024
    assert int(re.search(r"#define BN_ABI_VERSION (\d+)", text).group(1)) == _hip.ABI_VERSION
    assert R.RUN_ROWS == _hip.PCA_RUN_ROWS and {"bn_pca_colsum", "bn_pca_gram", "bn_pca_transform"} <= set(_hip.EXPORTS)
    assert _hip.pca_gram_rows_per_range(1000, 40) == 256 and _hip.pca_gram_rows_per_range(262144, 256) == 2560 and _hip.pca_gram_rows_per_range(0, 3) == 256
    assert _hip.pca_tile_rows(256, 32) == 32 and _hip.pca_tile_rows(256, 130) == 128 and _hip.pca_tile_rows(2048, 130) == 16 and _hip.pca_tile_rows(3, 1) == 16
