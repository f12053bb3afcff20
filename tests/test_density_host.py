"""CPU tests of density clustering: the numpy specification (``evaluation/density.py``) on hand-computed cases, the Borůvka loop against
Kruskal bit for bit, the whole fit against scikit-learn's HDBSCAN, every refusal, and the ``density`` command's parser and CSV writers."""

import csv
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG


def _blobs(n_per, D, k, noise, seed):
    """Rectified Gaussian blobs plus rectified-Gaussian noise rows, shuffled."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((k, D))
    x = np.concatenate([cent[c] + 0.35 * rng.standard_normal((n_per, D)) for c in range(k)] + [rng.standard_normal((noise, D))])
    x = np.maximum(x, 0).astype(np.float32)
    return x[rng.permutation(x.shape[0])]


def _lattice(N, D, seed, dup=0):
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 16, (N, D)) / 16.0).astype(np.float32)
    x[x.sum(axis=1) == 0, 0] = 0.5
    for _ in range(dup):
        a, b = rng.integers(0, N, 2)
        x[a] = x[b]
    return x


def test_module_needs_no_torch_at_import():
    code = "import sys; import birdnet_stm32.evaluation.density, birdnet_stm32.cli.density; assert 'torch' not in sys.modules"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_keys_are_the_order():
    from birdnet_stm32.evaluation.density import make_keys, split_keys

    m = np.array([-np.inf, -1.5, -0.0, 0.0, 1e-30, 0.5, 1.0, np.inf], np.float32)
    k = make_keys(m, np.full(m.size, 7))
    assert k.dtype == np.uint64 and (np.diff(k[[0, 1, 3, 4, 5, 6, 7]].astype(object)) > 0).all() and k[2] == k[3]   # -0 is +0
    assert make_keys(np.float32(0.5), 3) > make_keys(np.float32(0.5), 4) and make_keys(np.float32(0.25), 0) < make_keys(np.float32(0.5), 1 << 20)
    assert int(make_keys(np.float32(1.0), 5)) == (0xBF800000 << 32) | (0xFFFFFFFF - 5) and (k != 0).all()
    bm, bj = split_keys(np.concatenate([k, np.zeros(1, np.uint64)]))
    assert np.array_equal(bm[:-1].view(np.uint32), (m + np.float32(0)).view(np.uint32)) and (bj[:-1] == 7).all() and bm[-1] == -np.inf and bj[-1] == -1


def test_total_order_on_ties_by_hand():
    from birdnet_stm32.evaluation.density import hdbscan_reference, mutual_reachability, nearest_reference, pair_scores, split_keys

    x = np.array([[1, 0], [0, 1], [1, 1], [1, 1]], np.float32)
    inv = np.float32(1) / np.sqrt(np.float32(2))
    c = np.float32(np.float32(1) * np.float32(np.float32(1) * inv))   # rows 0 and 1 against rows 2 and 3: four equal scores
    dup = np.float32(np.float32(2) * np.float32(inv * inv))
    s = pair_scores(x)
    assert np.array_equal(s, s.T) and s[0, 1] == 0 and s[0, 2] == s[0, 3] == s[1, 2] == s[1, 3] == c and s[2, 3] == dup > c
    res = hdbscan_reference(x, 2, 1)
    assert res.mst_edges.tolist() == [[2, 3], [0, 2], [1, 2]] and res.mst_weight.tolist() == [dup, c, c] and np.isinf(res.core).all()
    # every row its own component: the best partner, the lower row among equal scores
    m, j = split_keys(nearest_reference(x, res.core, np.arange(4)))
    assert j.tolist() == [2, 2, 3, 2] and m.tolist() == [c, c, dup, dup]
    # rows 2 and 3 united, row 1 taking no part: row 0 sees only component 2
    m, j = split_keys(nearest_reference(x, res.core, np.array([0, -1, 2, 2])))
    assert j.tolist() == [2, -1, 0, 0] and m[1] == -np.inf
    assert (nearest_reference(x, res.core, np.zeros(4, np.int64)) == 0).all()   # one component: no edge left
    # min_samples counts the point itself: 2 is the best other row, 3 the second best
    assert hdbscan_reference(x, 2, 2).core.tolist() == [c, c, dup, dup]
    r3 = hdbscan_reference(x, 2, 3)
    assert r3.core.tolist() == [c, c, c, c] and (r3.mst_weight == c).all() and r3.mst_edges.tolist() == [[0, 2], [0, 3], [1, 2]]
    assert np.array_equal(mutual_reachability(s, r3.core)[np.triu_indices(4, 1)], [0, c, c, c, c, c])


def test_duplicates_zero_row_and_the_lambda_cap_by_hand():
    from birdnet_stm32.evaluation.density import MIN_DISTANCE, hdbscan_reference, score_to_lambda

    assert score_to_lambda(np.float32(1.0)) == 1 / MIN_DISTANCE == 4096.0
    below_one = np.nextafter(np.float32(1), np.float32(0))   # the smallest non-zero distance a float32 score gives is above the cap
    assert score_to_lambda(below_one) == 1 / np.sqrt(2.0 * 2.0 ** -24) < 4096.0 and score_to_lambda(np.float32(-1.0)) == 0.5
    x = np.array([[2, 0], [0, 4], [2, 0], [0, 0], [0, 4], [2, 0], [0, 4]], np.float32)   # two triples of duplicates at a right angle, a zero row
    res = hdbscan_reference(x, 2, 1, exemplars=2)
    root2 = 1 / np.sqrt(2.0)
    assert res.labels.tolist() == [0, 1, 0, -1, 1, 0, 1] and res.score.tolist() == [1, 1, 1, 0, 1, 1, 1] and res.n_clusters == 2
    assert res.mst_edges.tolist() == [[0, 2], [0, 5], [1, 4], [1, 6], [0, 1]] and res.mst_weight.tolist() == [1, 1, 1, 1, 0]
    assert np.allclose(res.stability, 3 * (4096 - root2), rtol=1e-15) and res.exemplar_idx.tolist() == [[0, 2], [1, 4]]
    assert np.isnan(res.core[3]) and np.isinf(np.delete(res.core, 3)).all() and res.score.dtype == np.float64 and res.labels.dtype == np.int64
    b = np.array([[7, 5], [5, 7], [7, 5], [5, 5], [5, 7], [7, 5], [5, 7]], np.int8)   # the same rows as bytes around the zero point 5
    rb = hdbscan_reference(b, 2, 1, zero_point=5, exemplars=2)
    assert rb.labels.tolist() == res.labels.tolist() and rb.mst_edges.tolist() == res.mst_edges.tolist() and rb.exemplar_idx.tolist() == [[0, 2], [1, 4]]


def test_hierarchy_by_hand():
    from birdnet_stm32.evaluation.density import exemplars_of, hierarchy, score_to_lambda

    w = np.array([0.98, 0.98, 0.98, 0.92, 0.68, 0.5], np.float32)
    edges = np.array([[0, 1], [0, 2], [3, 4], [3, 5], [2, 3], [0, 6]])
    hi, mid, join, far = score_to_lambda(w[[0, 3, 4, 5]])
    assert abs(hi - 5) < 1e-5 and abs(mid - 2.5) < 1e-5 and abs(join - 1.25) < 1e-6 and abs(far - 1) < 1e-7
    h = hierarchy(edges, w, 7, 2)
    # row 6 falls out of the root at `far`; the root splits at `join` into {0, 1, 2} and {3, 4, 5}; row 5 leaves its cluster at `mid`
    assert h.parent.tolist() == [-1, 0, 0] and h.birth.tolist() == [0, join, join] and h.size.tolist() == [7, 3, 3] and h.selected.tolist() == [False, True, True]
    assert h.point_cluster.tolist() == [1, 1, 1, 2, 2, 2, 0] and h.point_lambda.tolist() == [hi, hi, hi, hi, hi, mid, far]
    assert np.allclose(h.stability, [far + 6 * join, 3 * (hi - join), (mid - join) + 2 * (hi - join)], rtol=1e-15)
    assert h.labels.tolist() == [0, 0, 0, 1, 1, 1, -1] and h.score.tolist() == [1, 1, 1, 1, 1, mid / hi, 0] and h.max_lambda.tolist() == [join, hi, hi]
    assert exemplars_of(h.labels, h.point_lambda, 2, 3).tolist() == [[0, 1, 2], [3, 4, 5]] and exemplars_of(h.labels, h.point_lambda, 2, 0).shape == (2, 0)
    # with min_cluster_size 3 the same tree: rows 3 and 4 no longer outlive row 5 as a cluster, the three fall out together at `mid`
    h = hierarchy(edges, w, 7, 3)
    assert h.point_lambda.tolist() == [hi, hi, hi, mid, mid, mid, far] and h.labels.tolist() == [0, 0, 0, 1, 1, 1, -1] and h.score.tolist() == [1, 1, 1, 1, 1, 1, 0]
    # with min_cluster_size 4 nothing but the root is left: all noise
    h = hierarchy(edges, w, 7, 4)
    assert h.parent.tolist() == [-1] and (h.labels == -1).all() and (h.score == 0).all() and h.cluster_stability.size == 0
    # excess of mass keeps a parent that outweighs its children: a long-lived cluster of 6 that splits into two triples just before its end
    edges = np.array([[0, 1], [0, 2], [3, 4], [3, 5], [0, 3], [6, 7], [6, 8], [0, 6]])
    w = np.array([0.995, 0.995, 0.995, 0.995, 0.99, 0.9, 0.9, 0.0], np.float32)
    h = hierarchy(edges, w, 9, 3)
    assert h.parent.tolist() == [-1, 0, 0, 1, 1] and h.selected.tolist() == [False, True, True, False, False] and h.labels.tolist() == [0] * 6 + [1] * 3
    tight, split = score_to_lambda(w[[0, 4]])
    assert h.score[:6].tolist() == [1] * 6 and h.max_lambda[1] == split and np.allclose(h.stability[1], 6 * (split - h.birth[1])) and h.stability[3] == 3 * (tight - split)


@pytest.mark.parametrize("make, min_samples", [(lambda: _lattice(150, 8, 1), 1), (lambda: _lattice(150, 8, 2, dup=40), 4), (lambda: _lattice(97, 3, 3), 2),
                                               (lambda: _blobs(30, 16, 4, 20, 5), 5), (lambda: np.repeat(_blobs(12, 8, 3, 6, 6), 3, axis=0), 3),
                                               (lambda: _blobs(20, 32, 3, 10, 7), 1)])
def test_boruvka_gives_kruskals_tree_bit_for_bit(make, min_samples):
    from birdnet_stm32.evaluation.density import _NumpyBackend, boruvka, core_scores_reference, mst_reference

    x = make()
    core = core_scores_reference(x, min_samples)
    b = _NumpyBackend(x, 0, core)
    edges, weight, rounds = boruvka(b, x.shape[0])
    want_e, want_w = mst_reference(b.m)
    assert edges.shape == (x.shape[0] - 1, 2) and np.array_equal(edges, want_e) and np.array_equal(weight.view(np.uint32), want_w.view(np.uint32))
    assert 1 <= rounds <= int(np.ceil(np.log2(x.shape[0]))) and (edges[:, 0] < edges[:, 1]).all()
    assert (np.diff(weight.astype(np.float64)) <= 0).all()


def test_boruvka_on_int8_bytes():
    from birdnet_stm32.evaluation.density import _NumpyBackend, boruvka, core_scores_reference, mst_reference, pair_scores

    rng = np.random.default_rng(8)
    b = rng.integers(-128, 128, (120, 24)).astype(np.int8)
    b[40:60] = b[:20]
    for zp in (-128, 0, 5):
        s = pair_scores(b, zp)
        x = b.astype(np.float64) - zp
        want = (x @ x.T) / np.sqrt((x * x).sum(1))[:, None] / np.sqrt((x * x).sum(1))[None, :]
        assert np.array_equal(s, s.T) and np.abs(s - want).max() < 3e-7
        back = _NumpyBackend(b, zp, core_scores_reference(b, 3, zp))
        edges, weight, _ = boruvka(back, 120)
        want_e, want_w = mst_reference(back.m)
        assert np.array_equal(edges, want_e) and np.array_equal(weight.view(np.uint32), want_w.view(np.uint32))


# D, (min_cluster_size, min_samples), seed.  Seeds are chosen so that no exact tie decides a row: with min_samples > 1 many mutual-reachability
# scores are one row's core score, and where a row hangs between two clusters by two equal scores scikit-learn's tree (Prim's order, an
# unstable sort) may take the other edge than the total order here does (seed 3 of the third input does: one row moves).  The rule stays; the input goes.
SKLEARN_CASES = [(16, (10, 10), 1), (32, (5, 5), 2), (64, (15, 5), 18), (256, (8, 1), 4)]


@pytest.mark.parametrize("D, sizes, seed", SKLEARN_CASES)
def test_fit_against_scikit_learn(D, sizes, seed):
    from sklearn.cluster import HDBSCAN
    from sklearn.metrics import adjusted_rand_score

    from birdnet_stm32.evaluation.density import core_scores_reference, hdbscan_reference, mutual_reachability, pair_scores

    mcs, ms = sizes
    x = _blobs(40, D, 5, 30, seed)
    res = hdbscan_reference(x, mcs, ms)
    assert res.n_clusters >= 2 and (res.labels < 0).any()

    def chord(score):
        d = np.sqrt(np.maximum(0.0, 2.0 - 2.0 * score.astype(np.float64)))
        np.fill_diagonal(d, 0.0)
        return d

    # scikit-learn from the pair distances, its own core distances: the meaning of min_samples and the whole pipeline.  Its cores are
    # order statistics of the symmetric scores, the specification's are `search`'s (the same product rounded in another order: both
    # within 2 roundings of 2^-24 of the true score, so at most 2^-22 apart).  lambda^2 = 1 / (2 - 2 m), so a change dm of a score moves
    # lambda by the factor dm / (2 - 2 m) = dm / d^2 at most, and a membership, the ratio of two of them, by twice that.
    dist = chord(pair_scores(x))
    sk = HDBSCAN(min_cluster_size=mcs, min_samples=ms, metric="precomputed").fit(dist.copy())
    assert np.array_equal(sk.labels_ < 0, res.labels < 0) and adjusted_rand_score(sk.labels_, res.labels) == 1.0
    d_min = dist[np.triu_indices_from(dist, 1)].min()
    assert d_min > 0.05 and np.abs(sk.probabilities_ - res.score).max() <= 2 * 2.0 ** -22 / d_min ** 2
    # scikit-learn from the specification's own mutual-reachability distances (min_samples = 1 leaves them as they are): the same numbers
    # go in, so hierarchy, selection and membership must agree to float64 rounding
    m = mutual_reachability(pair_scores(x), core_scores_reference(x, ms))
    sk = HDBSCAN(min_cluster_size=mcs, min_samples=1, metric="precomputed").fit(chord(m))
    assert np.array_equal(sk.labels_ < 0, res.labels < 0) and adjusted_rand_score(sk.labels_, res.labels) == 1.0
    assert np.abs(sk.probabilities_ - res.score).max() <= 1e-9


def test_refusals():
    from birdnet_stm32.evaluation.density import check_density_args, check_density_flags, hdbscan_reference

    x = _lattice(20, 4, 0)
    for kw, what in ((dict(min_cluster_size=1), "min_cluster_size"), (dict(min_cluster_size=21), "min_cluster_size"), (dict(min_cluster_size=5, min_samples=0), "min_samples"),
                     (dict(min_cluster_size=5, min_samples=21), "min_samples"), (dict(min_cluster_size=5, exemplars=-1), "exemplars")):
        with pytest.raises(ValueError, match=what):
            hdbscan_reference(x, **kw)
    z = np.zeros((5, 4), np.float32)
    z[2, 1] = 1
    with pytest.raises(ValueError, match="at least 2 non-zero rows"):
        hdbscan_reference(z, 2)
    with pytest.raises(ValueError, match="not finite"):
        hdbscan_reference(np.full((4, 4), np.nan, np.float32), 2)
    with pytest.raises(ValueError, match=r"\[N, D\]"):
        hdbscan_reference(np.zeros(4, np.float32), 2)
    with pytest.raises(ValueError, match="at most"):
        check_density_args((1 << 20) + 1, 15, None)
    with pytest.raises(ValueError, match="min_samples"):
        check_density_args(1000, 15, 130)   # the point and 128 neighbours
    with pytest.raises(ValueError, match="pass min_samples"):
        check_density_flags(200, None)
    assert check_density_args(1000, 200, 129) == (200, 129) and check_density_args(20, 15, None) == (15, 15) and check_density_args(2, 2, 2) == (2, 2)


class _Result:
    def __init__(self, labels, score, stability, exemplar_idx):
        self.labels, self.score, self.stability = np.asarray(labels), np.asarray(score, np.float64), np.asarray(stability, np.float64)
        self.exemplar_idx, self.n_clusters = np.asarray(exemplar_idx, np.int64), self.stability.size


def test_csv_and_summary_writers(tmp_path):
    from birdnet_stm32.cli import cluster as cluster_cli
    from birdnet_stm32.cli.density import CSV_COLUMNS, SUMMARY_COLUMNS, summary_path, write_clusters_csv, write_summary_csv
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    index = EmbeddingIndex(np.eye(4, dtype=np.float32), [0, 0, 1, 1], [0.0, 3.0, 1.5, 4.5], ["a.wav", "b.wav"])
    res = _Result([1, 0, 1, -1], [0.5, 1.0, 0.25, 0.0], [2.5, 0.125], [[1, -1], [0, 2]])
    out = str(tmp_path / "density.csv")
    assert summary_path(out) == str(tmp_path / "density_summary.csv") and CSV_COLUMNS == cluster_cli.CSV_COLUMNS and write_clusters_csv is cluster_cli.write_clusters_csv
    assert write_clusters_csv(out, index, res, 3.0) == 4
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == ("path", "start_s", "end_s", "cluster", "score")
    assert rows[1:] == [["a.wav", "0.000", "3.000", "1", "0.5"], ["a.wav", "3.000", "6.000", "0", "1"], ["b.wav", "1.500", "4.500", "1", "0.25"],
                        ["b.wav", "4.500", "7.500", "-1", "0"]]
    assert write_summary_csv(summary_path(out), index, res) == 2 and SUMMARY_COLUMNS == ("cluster", "count", "stability")
    with open(summary_path(out), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["cluster", "count", "stability", "exemplar_1", "exemplar_2"]
    assert rows[1:] == [["0", "1", "2.5", "a.wav@3.000", ""], ["1", "2", "0.125", "a.wav@0.000", "b.wav@1.500"]]
    res = _Result([-1, -1, -1, -1], [0, 0, 0, 0], [], np.zeros((0, 2)))   # all noise: a header and nothing else
    assert write_summary_csv(summary_path(out), index, res) == 0
    with open(summary_path(out), newline="") as f:
        assert list(csv.reader(f)) == [["cluster", "count", "stability", "exemplar_1", "exemplar_2"]]


def test_parser_defaults_refusals_and_dispatch(tmp_path):
    import birdnet_stm32.__main__ as m
    from birdnet_stm32.cli.density import build_parser, main, validate_args

    db = tmp_path / "db.npz"
    db.write_bytes(b"")   # no archive: every refusal below comes before it is read
    base = ["--database", str(db), "--output", "density.csv"]
    args = build_parser().parse_args(base)
    assert (args.min_cluster_size, args.min_samples, args.exemplars, args.chunk_duration, args.device) == (15, None, 5, 0.0, 0)
    validate_args(args)
    args = build_parser().parse_args(base + ["--database", "a.npz", "b.npz", "--min_samples", "3"])
    assert args.database == ["a.npz", "b.npz"] and args.min_samples == 3
    for extra, what in ((["--min_cluster_size", "1"], "--min_cluster_size"), (["--min_samples", "0"], "--min_samples"), (["--min_samples", "130"], "--min_samples"),
                        (["--min_cluster_size", "200"], "--min_samples"), (["--exemplars", "-1"], "--exemplars"), (["--chunk_duration", "-1"], "--chunk_duration")):
        with pytest.raises(SystemExit, match=what):
            main(base + extra)
    with pytest.raises(SystemExit, match="not found"):
        main(["--database", str(tmp_path / "none.npz"), "--output", "d.csv"])
    assert "density" in m.USAGE and "density" in m.__doc__
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "birdnet_stm32", "density", "--help"], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "--database" in r.stdout and "--min_cluster_size" in r.stdout and "--min_samples" in r.stdout and "--exemplars" in r.stdout


def test_abi_constants_stay_in_step():
    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation import density

    hdr = open(os.path.join(os.path.dirname(PKG), "include", "birdnet_hip.h")).read()
    val = {k: eval(v) for k, v in re.findall(r"#define (BN_DENSITY_\w+) \(?([\d\*< ]+)\)?\n", hdr)}
    assert (val["BN_DENSITY_MAX_N"], val["BN_DENSITY_MAX_D"]) == (_hip.DENSITY_MAX_N, _hip.DENSITY_MAX_D) == (density.MAX_N, 2048) == (1 << 20, 2048)
    assert (val["BN_DENSITY_LDS_BYTES"], val["BN_DENSITY_MAX_TILE"], val["BN_DENSITY_STEP_ROWS"], val["BN_DENSITY_MIN_WG_STEPS"], val["BN_DENSITY_MAX_ROW_WGS"]) == (
        _hip.DENSITY_LDS_BYTES, _hip.DENSITY_MAX_TILE, _hip.DENSITY_STEP_ROWS, _hip.DENSITY_MIN_WG_STEPS, _hip.DENSITY_MAX_ROW_WGS)
    assert re.search(r"BN_API int bn_density_nearest\(", hdr) and "bn_density_nearest" in _hip.EXPORTS
    assert _hip.density_tile_rows(1 << 18, 256, False) == 128 and _hip.density_tile_rows(1 << 18, 2048, False) == 16 and _hip.density_tile_rows(1 << 18, 2048, True) == 64
    assert [_hip.density_tile_rows(n, 64, False) for n in (2, 16, 17, 32, 33, 65, 4099)] == [16, 16, 32, 32, 64, 128, 128]
    assert _hip.density_rows_per_workgroup(15) == 64 and _hip.density_rows_per_workgroup(2048) == 2048 and _hip.density_rows_per_workgroup(2049) == 1088
    assert _hip.density_rows_per_workgroup(1 << 20) == 4096
    if os.path.isfile(_hip.LIB_PATH):
        assert "density_nearest_kernel" in _hip.load_library().bn_kernel_names().decode().split("\n")
