"""CPU tests of clustering: the numpy specification (``assign_reference``, ``repair_empty_clusters``, the seeded initialisation,
``kmeans_reference``) on hand-checked cases, every refusal, and the ``cluster`` command's parser, CSV writers and centroid archive."""

import csv
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG


def _blocks(N, D, K, seed=0):
    """Row i belongs to block i mod K: values in [1, 1.5] on the D // K dimensions of its block, 0.05 |N(0, 1)| elsewhere."""
    rng = np.random.default_rng(seed)
    x = 0.05 * np.abs(rng.standard_normal((N, D)))
    w = D // K
    for i in range(N):
        c = i % K
        x[i, c * w:(c + 1) * w] = rng.uniform(1.0, 1.5, w)
    return x.astype(np.float32)


def test_module_needs_no_torch_at_import():
    code = "import sys; import birdnet_stm32.evaluation.cluster, birdnet_stm32.cli.cluster; assert 'torch' not in sys.modules"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_assignment_by_hand_ties_duplicates_and_zero_rows():
    from birdnet_stm32.evaluation.cluster import assign_reference
    from birdnet_stm32.evaluation.search import search_reference

    C = np.array([[0, 1], [1, 0], [2, 0], [1, 0], [1, 1]], np.float32)   # centroids 1, 2 and 3 point the same way
    X = np.array([[3, 0], [0, 0], [0, 5], [1, 1], [2, 1]], np.float32)
    label, score = assign_reference(X, C)
    assert label.tolist() == [1, -1, 0, 4, 4] and label.dtype == np.int64 and score.dtype == np.float32   # row 0 ties three ways: the lowest
    assert score[:4].tolist() == [1.0, 0.0, 1.0, float(np.float32(np.float32(2.0) * (np.float32(1) / np.sqrt(np.float32(2)))) * (np.float32(1) / np.sqrt(np.float32(2))))]
    wi, ws = search_reference(C, X, 1, "cosine")   # the same thing with the roles swapped, apart from the zero row
    live = label >= 0
    assert np.array_equal(label[live], wi[live, 0]) and np.array_equal(score[live].view(np.uint32), ws[live, 0].view(np.uint32))
    assert wi[1, 0] == 0 and ws[1, 0] == 0.0   # search gives a zero query the first row at score 0; clustering gives it no cluster
    # on a lattice the specification has one value: random rows against duplicated centroids
    rng = np.random.default_rng(3)
    X = (rng.integers(0, 16, (200, 24)) / 16.0).astype(np.float32)
    C = (rng.integers(0, 16, (9, 24)) / 16.0).astype(np.float32)
    C[5], C[7] = C[2], C[2]
    X[11] = 0
    label, score = assign_reference(X, C)
    wi, ws = search_reference(C, X, 1, "cosine")
    live = np.arange(200) != 11
    assert np.array_equal(label[live], wi[live, 0]) and np.array_equal(score[live], ws[live, 0]) and label[11] == -1 and score[11] == 0
    assert not np.isin(label, (5, 7)).any() and (label == 2).any()
    # int8 rows: float32(byte - zero_point), exact inverse norms
    b = rng.integers(-128, 128, (50, 24)).astype(np.int8)
    b[4] = 5
    l8, s8 = assign_reference(b, C, zero_point=5)
    lf, sf = assign_reference((b.astype(np.float32) - 5), C)
    assert l8[4] == -1 and np.array_equal(l8, lf)
    l64, s64 = assign_reference(b, C, zero_point=5, dtype=np.float64)
    assert s64.dtype == np.float64 and np.abs(s64 - s8).max() < 1e-5


def test_repair_by_hand():
    from birdnet_stm32.evaluation.cluster import repair_empty_clusters
    from birdnet_stm32.evaluation.search import inv_norms_reference

    C = np.eye(5, 4, dtype=np.float32)
    C[4] = [0.5, 0.5, 0.5, 0.5]
    e = np.float32(1 / 1024)

    def split(v):
        up = v * np.array([1 + e, 1 - e, 1 + e, 1 - e], np.float32)
        down = v * np.array([1 - e, 1 + e, 1 - e, 1 + e], np.float32)
        return [(p * inv_norms_reference(p[None])[0]).astype(np.float32) for p in (up, down)]

    # two empties, and a tie for the largest cluster (1 and 4 hold 7 each: the lower index is split first)
    got, counts, n = repair_empty_clusters(C, [0, 7, 0, 3, 7])
    a, b = split(C[1])
    c, d = split(C[4])
    assert n == 2 and counts.tolist() == [3, 4, 3, 3, 4] and counts.dtype == np.int64 and got.dtype == np.float32
    assert np.array_equal(got[0], a) and np.array_equal(got[1], b) and np.array_equal(got[2], c) and np.array_equal(got[4], d) and np.array_equal(got[3], C[3])
    assert np.array_equal(C[0], [1, 0, 0, 0])   # the input is left alone
    # after the first split the largest is re-read: 9 -> (4, 5), then the 5 is split
    _, counts, n = repair_empty_clusters(C, [0, 9, 0, 1, 1])
    assert n == 2 and counts.tolist() == [4, 3, 2, 1, 1]
    # a largest count of 1 leaves the empty cluster alone
    got, counts, n = repair_empty_clusters(C, [1, 0, 1, 1, 1])
    assert n == 0 and counts.tolist() == [1, 0, 1, 1, 1] and np.array_equal(got, C)
    got, counts, n = repair_empty_clusters(C, [2, 2, 2, 2, 2])
    assert n == 0 and np.array_equal(got, C)


def test_seeded_initialisation():
    from birdnet_stm32.evaluation.cluster import seeded_centroids, seeded_rows
    from birdnet_stm32.evaluation.search import inv_norms_reference

    x = _blocks(300, 16, 4)
    x[::7] = 0
    inv = inv_norms_reference(x)
    a = seeded_rows(inv, 40, 42, 0)
    assert a.shape == (40,) and (np.diff(a) > 0).all() and (inv[a] != 0).all()   # sorted, distinct, no zero rows
    assert np.array_equal(a, seeded_rows(inv, 40, 42, 0)) and not np.array_equal(a, seeded_rows(inv, 40, 42, 1)) and not np.array_equal(a, seeded_rows(inv, 40, 43, 0))
    assert np.array_equal(a, np.sort(np.random.default_rng([42, 0]).choice(np.flatnonzero(inv != 0), 40, replace=False)))
    C = seeded_centroids(x, 0, 40, 42, 0)
    assert C.dtype == np.float32 and np.array_equal(C, (x[a] * inv[a, None]).astype(np.float32))
    b = np.random.default_rng(1).integers(-128, 128, (30, 16)).astype(np.int8)
    C8 = seeded_centroids(b, -3, 5, 1, 0)
    assert np.abs(np.linalg.norm(C8.astype(np.float64), axis=1) - 1).max() < 1e-6


@pytest.mark.parametrize("N,D,K", [(1000, 96, 8), (17, 8, 2)])
def test_reference_recovers_separated_blocks_in_two_assignments(N, D, K):
    from birdnet_stm32.evaluation.cluster import kmeans_reference

    x = _blocks(N, D, K)
    for dtype in (np.float32, np.float64):
        r = kmeans_reference(x, K, init_centroids=x[:K], dtype=dtype)
        assert np.array_equal(r.labels, np.arange(N) % K) and r.n_iter == 1 and r.converged
        assert r.counts.tolist() == np.bincount(np.arange(N) % K).tolist() and r.centroids.dtype == np.float32
        assert np.abs(np.linalg.norm(r.centroids.astype(np.float64), axis=1) - 1).max() < 1e-6
        assert r.score.min() > 0.9 and abs(r.mean_score - r.score.astype(np.float64).mean()) < 1e-12
    r0 = kmeans_reference(x, K, init_centroids=x[:K], max_iter=0)   # one assignment, no update: the centroids come back as given
    assert r0.n_iter == 0 and not r0.converged and np.array_equal(r0.centroids, x[:K]) and np.array_equal(r0.labels, np.arange(N) % K)


def test_the_best_restart_is_chosen_by_the_mean_score():
    from birdnet_stm32.evaluation.cluster import kmeans_reference, seeded_centroids

    rng = np.random.default_rng(5)
    x = np.maximum(rng.standard_normal((6, 12))[rng.integers(0, 6, 400)] + 0.8 * rng.standard_normal((400, 12)), 0).astype(np.float32)
    x[3] = 0
    singles = [kmeans_reference(x, 5, max_iter=4, init_centroids=seeded_centroids(x, 0, 5, 9, r)) for r in range(3)]
    means = [s.mean_score for s in singles]
    assert len(set(means)) == 3, "the restarts should differ"
    best = kmeans_reference(x, 5, max_iter=4, n_init=3, seed=9)
    want = int(np.argmax(means))
    assert best.restart == want and np.array_equal(best.centroids, singles[want].centroids) and np.array_equal(best.labels, singles[want].labels)
    assert best.labels[3] == -1 and best.score[3] == 0 and best.counts.sum() == int((np.abs(x).sum(axis=1) > 0).sum()) < 400
    live = best.labels >= 0
    assert best.mean_score == float(best.score[live].astype(np.float64).sum() / live.sum())
    again = kmeans_reference(x, 5, max_iter=4, n_init=3, seed=9)
    assert np.array_equal(again.centroids.view(np.uint32), best.centroids.view(np.uint32))


def test_a_duplicated_initial_row_goes_through_the_repair():
    from birdnet_stm32.evaluation.cluster import kmeans_reference

    x = _blocks(200, 16, 4)
    init = x[[0, 1, 1, 3]]   # centroid 2 duplicates centroid 1: every tie goes to 1 and 2 comes out empty
    r = kmeans_reference(x, 4, init_centroids=init, max_iter=10)
    assert r.converged and (r.counts > 0).all() and r.counts.sum() == 200


def test_every_refusal():
    from birdnet_stm32.evaluation.cluster import MAX_D, MAX_K, cluster_index, kmeans_reference
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    x = _blocks(20, 8, 2)
    x[5] = 0
    for kw, what in ((dict(k=0), ">= 1"), (dict(k=20), "non-zero rows"), (dict(k=MAX_K + 1), "above"), (dict(k=2, max_iter=-1), "max_iter"),
                     (dict(k=2, n_init=0), "n_init"), (dict(k=2, init_centroids=np.ones((3, 8))), "init_centroids"),
                     (dict(k=2, init_centroids=np.full((2, 8), np.inf)), "finite")):
        with pytest.raises(ValueError, match=what):
            kmeans_reference(x, **kw)
    kmeans_reference(x, 19, max_iter=1)   # exactly the non-zero rows
    with pytest.raises(ValueError, match="finite"):
        kmeans_reference(np.full((4, 8), np.nan, np.float32), 2)
    with pytest.raises(ValueError, match="width"):
        kmeans_reference(np.ones((4, MAX_D + 1), np.float32), 2)
    with pytest.raises(ValueError, match=r"\[N, D\]"):
        kmeans_reference(np.ones(4, np.float32), 2)
    # the device entry refuses the same things before it touches a device
    index = EmbeddingIndex(x, np.zeros(20, np.int64), np.zeros(20), ["a.wav"])
    for kw, what in ((dict(k=0), ">= 1"), (dict(k=20), "non-zero rows"), (dict(k=MAX_K + 1), "above"), (dict(k=2, exemplars=-1), "exemplars"),
                     (dict(k=2, exemplars=129), "exemplars"), (dict(k=2, init_centroids=np.ones((2, 7))), "init_centroids")):
        with pytest.raises(ValueError, match=what):
            cluster_index(index, **kw)
    i8 = EmbeddingIndex(np.ones((4, 8), np.int8), np.zeros(4, np.int64), np.zeros(4), ["a.wav"], "int8", 0.1, 0)
    with pytest.raises(ValueError, match="int8"):
        cluster_index(i8, 2, exemplars=1)


def _result(index, labels, score, centroids, ex_idx):
    from birdnet_stm32.evaluation.cluster import ClusterResult

    labels = np.asarray(labels, np.int64)
    K = len(centroids)
    return ClusterResult(labels, np.asarray(score, np.float32), np.asarray(centroids, np.float32), np.bincount(labels[labels >= 0], minlength=K), 0.5, 2, True,
                         np.asarray(ex_idx, np.int64), np.zeros(np.shape(ex_idx), np.float32))


def test_csv_and_summary_writers(tmp_path):
    from birdnet_stm32.cli.cluster import CSV_COLUMNS, summary_path, write_clusters_csv, write_summary_csv
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    index = EmbeddingIndex(np.eye(4, dtype=np.float32), [0, 0, 1, 1], [0.0, 3.0, 1.5, 4.5], ["a.wav", "b.wav"])
    res = _result(index, [1, 0, 1, -1], [0.5, 1.0, 0.25, 0.0], np.eye(3, 4), [[1, -1], [0, 2], [-1, -1]])
    out = str(tmp_path / "clusters.csv")
    assert summary_path(out) == str(tmp_path / "clusters_summary.csv") and summary_path("x") == "x_summary.csv"
    assert write_clusters_csv(out, index, res, 3.0) == 4
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == CSV_COLUMNS == ("path", "start_s", "end_s", "cluster", "score")
    assert rows[1:] == [["a.wav", "0.000", "3.000", "1", "0.5"], ["a.wav", "3.000", "6.000", "0", "1"], ["b.wav", "1.500", "4.500", "1", "0.25"],
                        ["b.wav", "4.500", "7.500", "-1", "0"]]
    assert write_summary_csv(summary_path(out), index, res) == 3
    with open(summary_path(out), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["cluster", "count", "mean_score", "exemplar_1", "exemplar_2"]
    assert rows[1:] == [["0", "1", "1", "a.wav@3.000", ""], ["1", "2", "0.375", "a.wav@0.000", "b.wav@1.500"], ["2", "0", "0", "", ""]]


def test_centroid_archive_round_trip(tmp_path):
    from birdnet_stm32.cli.cluster import write_centroid_archive
    from birdnet_stm32.evaluation.search import EmbeddingIndex, _load_archive

    C = np.random.default_rng(0).standard_normal((12, 8)).astype(np.float32)
    for name in ("c.npz", "centroids"):   # the name is taken as given
        path = str(tmp_path / name)
        write_centroid_archive(path, C)
        assert os.path.isfile(path)
        a = _load_archive(path)
        assert a["dtype"] == "float32" and np.array_equal(a["embeddings"], C) and a["paths"][:2] == ["cluster_000", "cluster_001"] and a["paths"][11] == "cluster_011"
        index = EmbeddingIndex.from_npz(path)
        assert len(index) == 12 and index.file_index.tolist() == list(range(12)) and (index.start_s == 0).all()


def test_parser_defaults_refusals_and_dispatch(tmp_path):
    import birdnet_stm32.__main__ as m
    from birdnet_stm32.cli.cluster import build_parser, main, validate_args

    db = tmp_path / "db.npz"
    db.write_bytes(b"")
    base = ["--database", str(db), "--output", "clusters.csv"]
    args = build_parser().parse_args(base + ["--k", "64"])
    assert (args.k, args.max_iter, args.n_init, args.seed, args.exemplars, args.centroids_out, args.chunk_duration, args.device) == (64, 25, 1, 42, 5, "", 0.0, 0)
    validate_args(args)
    for extra, what in ((["--k", "0"], "--k"), (["--k", "4097"], "--k"), (["--k", "4", "--max_iter", "-1"], "max_iter"), (["--k", "4", "--n_init", "0"], "n_init"),
                        (["--k", "4", "--exemplars", "129"], "exemplars"), (["--k", "4", "--chunk_duration", "-1"], "chunk_duration")):
        with pytest.raises(SystemExit, match=what):
            main(base + extra)
    with pytest.raises(SystemExit, match="not found"):
        main(["--database", str(tmp_path / "none.npz"), "--output", "c.csv", "--k", "4"])
    with pytest.raises(SystemExit):
        build_parser().parse_args(base)   # --k is required
    assert "cluster" in m.USAGE
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "birdnet_stm32", "cluster", "--help"], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "--database" in r.stdout and "--centroids_out" in r.stdout and "--exemplars" in r.stdout and "--n_init" in r.stdout


def test_abi_constants_stay_in_step():
    from birdnet_stm32 import _hip
    from birdnet_stm32.evaluation import cluster

    hdr = open(os.path.join(os.path.dirname(PKG), "include", "birdnet_hip.h")).read()
    val = {k: eval(v) for k, v in re.findall(r"#define (BN_KMEANS_\w+) \(?([\d\* ]+)\)?\n", hdr)}
    assert (val["BN_KMEANS_MAX_K"], val["BN_KMEANS_MAX_D"]) == (_hip.KMEANS_MAX_K, _hip.KMEANS_MAX_D) == (cluster.MAX_K, cluster.MAX_D) == (4096, 2048)
    assert (val["BN_KMEANS_LDS_BYTES"], val["BN_KMEANS_MAX_TILE"], val["BN_KMEANS_STEP_ROWS"], val["BN_KMEANS_MIN_WG_STEPS"], val["BN_KMEANS_MAX_WGS"],
            val["BN_KMEANS_SEGMENT_ROWS"]) == (_hip.KMEANS_LDS_BYTES, _hip.KMEANS_MAX_TILE, _hip.KMEANS_STEP_ROWS, _hip.KMEANS_MIN_WG_STEPS, _hip.KMEANS_MAX_WGS,
                                               _hip.KMEANS_SEGMENT_ROWS)
    assert _hip.kmeans_tile_centroids(256, 4096) == 128 and _hip.kmeans_tile_centroids(256, 16) == 16 and _hip.kmeans_tile_centroids(256, 17) == 32
    assert _hip.kmeans_tile_centroids(2048, 4096) == 16 and _hip.kmeans_tile_centroids(8, 1024) == 128
    assert {"bn_kmeans_assign", "bn_kmeans_accumulate", "bn_kmeans_centroids"} <= set(_hip.EXPORTS)
