"""CPU tests of the silhouette's numpy specification (evaluation/silhouette.py), the sweep on the host and the commands' flags and writers.

The oracle is scikit-learn's ``silhouette_samples(metric="cosine")`` on the float64-normalised rows: the float64 variant of the reference
must agree to 1e-12, which checks the identity ``sum_{j in c} (1 - x^_i . x^_j) = n_c - x^_i . S_c`` and the conventions at once."""

import io
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import silhouette_cases as cases
from conftest import PKG


def _mod():
    import birdnet_stm32.evaluation.silhouette as m

    return m


def test_module_needs_no_torch_at_import():
    code = "import sys; import birdnet_stm32.evaluation.silhouette, birdnet_stm32.cli.cluster, birdnet_stm32.cli.density; assert 'torch' not in sys.modules"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------------------------------ oracle
def _sklearn(rows, lab, zero_point=0):
    from sklearn.metrics import silhouette_samples

    x = cases.as_float64(rows, zero_point)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return silhouette_samples(x, lab, metric="cosine")


def _against_sklearn(rows, lab, zero_point=0):
    want = _sklearn(rows, lab, zero_point)
    got = _mod().silhouette_reference(rows, lab, zero_point=zero_point, dtype=np.float64)
    err = np.abs(got.silhouette - want).max()
    print(f"float64 reference against scikit-learn: {err:.3g}")
    assert err <= 1e-12
    assert got.n_live == len(lab) and abs(got.mean - want.mean()) <= 1e-12
    for c in range(int(lab.max()) + 1):
        assert abs(got.cluster_mean[c] - want[lab == c].mean()) <= 1e-12
    assert np.array_equal(got.counts, np.bincount(lab))
    return got


@pytest.mark.parametrize("N, D, K", cases.ORACLE_SHAPES)
def test_float64_reference_equals_scikit_learn(N, D, K):
    rows, lab = cases.planted(N, D, K)
    _against_sklearn(rows, lab)


def test_float64_reference_equals_scikit_learn_on_int8_rows():
    x, lab = cases.planted(1000, 96, 100)
    rows = cases.quantised(x, 5)
    assert rows.dtype == np.int8 and np.abs(rows.astype(np.int32) - 5).max() == 122
    _against_sklearn(rows, lab, zero_point=5)


@pytest.mark.parametrize("zp", [None, 5])
@pytest.mark.parametrize("N, D, K", cases.ORACLE_SHAPES)
def test_float32_reference_within_the_mean_cosine_bound(N, D, K, zp):
    """Teacher-forced: the float64 means take the float32 inverse norms, sums and weights the float32 means are computed from."""
    from birdnet_stm32.evaluation.cluster import update_reference
    from birdnet_stm32.evaluation.search import inv_norms_reference

    m = _mod()
    rows, lab = cases.planted(N, D, K)
    zero = 0
    if zp is not None:
        rows, zero = cases.quantised(rows, zp), zp
    inv = inv_norms_reference(rows, zero)
    S, counts = update_reference(rows, lab, K, zero)
    w = m.weights_from_counts(counts)
    bound = cases.mean_cosine_bound(rows, zero, inv, S, w)
    m64, cand = cases.candidate_means(rows, zero, inv, S, w, lab)
    sep = cases.separated_rows(cand, bound, lab)
    assert sep.mean() >= 0.99
    own64, other64, near64 = m.means_reference(rows, lab, S, w, zero, np.float64, inv)
    r = np.arange(N)
    assert np.array_equal(own64, m64[r, lab]) or np.abs(own64 - m64[r, lab]).max() < 1e-15
    own, other, near = m.means_reference(rows, lab, S, w, zero, np.float32, inv)
    assert own.dtype == np.float32 and other.dtype == np.float32
    assert (np.abs(own - own64) <= bound[r, lab]).all()
    assert np.array_equal(near[sep], near64[sep])
    assert (np.abs(other - other64)[sep] <= bound[r, near64][sep]).all()
    # and the whole float32 reference against the float64 one: the issue's figure is about 6e-7
    s32, s64 = m.silhouette_reference(rows, lab, zero_point=zero), m.silhouette_reference(rows, lab, zero_point=zero, dtype=np.float64)
    assert np.abs(s32.silhouette - s64.silhouette)[sep].max() < 5e-6


# ------------------------------------------------------------------------------------------------------------------- conventions
def _unit(*dims, D=8):
    """Rows along the axes: normalised exactly, every dot product 0 or 1."""
    x = np.zeros((len(dims), D), np.float32)
    for i, d in enumerate(dims):
        if d is not None:
            x[i, d] = 2.0
    return x


def test_singleton_cluster_gives_zero():
    r = _mod().silhouette_reference(_unit(0, 0, 1), [0, 0, 1])
    assert r.silhouette[2] == 0.0 and r.silhouette[0] == 1.0 and r.silhouette[1] == 1.0
    assert np.array_equal(r.nearest, [1, 1, 0]) and np.array_equal(r.counts, [2, 1])
    assert r.mean == pytest.approx(2.0 / 3.0) and np.array_equal(r.cluster_mean, [1.0, 0.0])


def test_duplicate_rows_in_two_clusters_give_zero():
    for dtype in (np.float32, np.float64):
        r = _mod().silhouette_reference(_unit(0, 0, 0, 0), [0, 0, 1, 1], dtype=dtype)   # a = b = 0
        assert np.array_equal(r.silhouette, np.zeros(4)) and r.mean == 0.0
        assert np.array_equal(r.own, np.ones(4)) and np.array_equal(r.other, np.ones(4))


def test_noise_labels_and_zero_rows_take_no_part():
    m = _mod()
    rows = _unit(0, 0, 1, 1, None, 2, 3, 1)
    lab = np.array([0, 0, 1, 1, 0, -1, 2, 1])   # row 4: a zero row labelled 0; row 5: noise; row 6: a label outside K = 2
    r = m.silhouette_reference(rows, lab, K=2)
    dead = [4, 5, 6]
    assert np.isnan(r.silhouette[dead]).all() and (r.nearest[dead] == -1).all()
    assert (r.own[dead] == 0).all() and (r.other[dead] == 0).all()
    assert r.n_live == 5 and np.array_equal(r.counts, [2, 3])
    keep = np.setdiff1d(np.arange(8), dead)
    alone = m.silhouette_reference(rows[keep], lab[keep], K=2)
    assert np.array_equal(r.silhouette[keep], alone.silhouette) and r.mean == alone.mean
    assert np.array_equal(r.cluster_mean, alone.cluster_mean)
    assert np.array_equal(r.silhouette[keep], np.ones(5))


def test_empty_cluster_ids_are_skipped_and_a_tie_takes_the_lowest_index():
    rows = _unit(0, 0, 1, 1, 1, 1)
    r = _mod().silhouette_reference(rows, [1, 1, 3, 3, 5, 5])   # K = 6; clusters 0, 2 and 4 are empty; clusters 3 and 5 hold the same rows
    assert np.array_equal(r.counts, [0, 2, 0, 2, 0, 2])
    assert np.isnan(r.cluster_mean[[0, 2, 4]]).all() and not np.isnan(r.cluster_mean[[1, 3, 5]]).any()
    assert np.array_equal(r.nearest, [3, 3, 5, 5, 3, 3]), "rows 0 and 1 are as far from 3 as from 5: the lower index; never an empty cluster"
    assert np.array_equal(r.silhouette, [1, 1, 0, 0, 0, 0])


def test_a_row_with_another_cluster_at_equal_distance():
    x = np.zeros((5, 4), np.float32)
    x[0] = [1, 1, 0, 0]
    x[1] = [1, 1, 0, 0]
    x[2] = [1, 0, 0, 0]
    x[3] = [0, 1, 0, 0]
    x[4] = [0, 1, 0, 0]
    r = _mod().silhouette_reference(x, [0, 0, 1, 2, 2], dtype=np.float64)
    assert r.nearest[0] == 1 and r.nearest[1] == 1, "clusters 1 and 2 are equally far from rows 0 and 1"
    s = _sklearn(x, np.array([0, 0, 1, 2, 2]))
    assert np.abs(r.silhouette - s).max() <= 1e-12


def test_refusals():
    m = _mod()
    rows, lab = cases.planted(40, 8, 3)
    ok = m.silhouette_reference(rows, lab)
    assert ok.n_live == 40
    with pytest.raises(ValueError, match="2 non-empty"):
        m.silhouette_reference(rows, np.zeros(40, np.int64), K=3)
    with pytest.raises(ValueError, match="2 non-empty"):
        m.silhouette_reference(rows, np.where(lab == 0, 0, -1), K=3)
    with pytest.raises(ValueError, match="2 non-empty"):
        m.silhouette_from_means(ok.own, ok.other, ok.nearest, lab, [40, 0, 0])
    for K in (0, -1, m.MAX_K + 1):
        with pytest.raises(ValueError, match="K="):
            m.silhouette_reference(rows, lab, K=K)
    with pytest.raises(ValueError, match="K="):
        m.silhouette_reference(rows, np.full(40, -1))   # K = None: max(label) + 1 = 0
    with pytest.raises(ValueError, match="width"):
        m.silhouette_reference(np.ones((4, m.MAX_D + 1), np.float32), [0, 0, 1, 1])
    with pytest.raises(ValueError, match="width"):
        m.silhouette_reference(np.ones((4, 0), np.float32), [0, 0, 1, 1])
    for bad in (lab[:-1], lab[None, :], np.concatenate([lab, lab])):
        with pytest.raises(ValueError, match="labels"):
            m.silhouette_reference(rows, bad)
    for v in (np.nan, np.inf):
        broken = rows.copy()
        broken[3, 2] = v
        with pytest.raises(ValueError, match="finite"):
            m.silhouette_reference(broken, lab)
    assert m.silhouette_reference(rows, lab, K=m.MAX_K).n_live == 40


# ------------------------------------------------------------------------------------------------------------------------- sweep
@pytest.mark.parametrize("gen_seed", [0, 1, 2])
def test_sweep_on_the_host_finds_the_planted_three(gen_seed):
    from birdnet_stm32.evaluation.cluster import kmeans_reference

    m = _mod()
    rows, _ = cases.planted(240, 32, 3, seed=gen_seed, noise=0.5)
    best, sil, table = m.sweep([6, 2, 3, 4, 5, 3], lambda k: kmeans_reference(rows, k, n_init=2, seed=42),
                               lambda r: m.silhouette_reference(rows, r.labels, r.centroids.shape[0]))
    print([(t["k"], round(t["silhouette"], 3)) for t in table])
    assert [t["k"] for t in table] == [2, 3, 4, 5, 6]
    assert best.centroids.shape[0] == 3 and sil.mean == max(t["silhouette"] for t in table) == table[1]["silhouette"]
    assert set(table[0]) == set(m.SWEEP_COLUMNS)
    assert all(t["smallest_cluster"] <= t["largest_cluster"] and t["smallest_cluster"] + t["largest_cluster"] <= 240 for t in table)
    assert sil.mean > 0.7 and all(t["silhouette"] < 0.65 for t in table if t["k"] != 3)


def test_sweep_keeps_the_lowest_k_among_equal_means_and_refuses_bad_candidates():
    m = _mod()
    fake = lambda k: SimpleNamespace(counts=np.array([3, 2]), mean_score=0.5, n_iter=1, converged=True, k=k)   # noqa: E731
    best, sil, table = m.sweep([4, 3, 2], fake, lambda r: SimpleNamespace(mean=0.25 if r.k == 2 else 0.5))
    assert best.k == 3 and sil.mean == 0.5 and len(table) == 3
    for ks in ([1, 2], [0], [2, m.MAX_K + 1], []):
        with pytest.raises(ValueError):
            m.check_sweep_ks(ks)
    assert m.check_sweep_ks([5, 2, 5, m.MAX_K]) == [2, 5, m.MAX_K]


# --------------------------------------------------------------------------------------------------------------------------- CLI
def _args(tmp_path, *extra):
    import birdnet_stm32.cli.cluster as cli

    db = tmp_path / "a.npz"
    db.write_bytes(b"")
    return cli, cli.build_parser().parse_args(["--database", str(db), "--output", str(tmp_path / "o.csv"), *extra])


def test_parser_takes_the_new_flags_and_refuses_bad_values(tmp_path, capsys):
    cli, a = _args(tmp_path, "--k", "2", "--k_sweep", "3", "4", "2", "6")
    assert a.k == 2 and a.k_sweep == [3, 4, 2, 6] and a.silhouette is False
    cli.validate_args(a)
    assert cli.sweep_candidates(a) == [2, 3, 4, 6]
    _, a = _args(tmp_path, "--k", "7")
    assert a.k_sweep is None and a.silhouette is False
    cli.validate_args(a)
    _, a = _args(tmp_path, "--k", "1")
    cli.validate_args(a)   # k = 1 stays a valid fit
    assert _args(tmp_path, "--k", "3", "--silhouette")[1].silhouette is True
    for extra in (["--k", "1", "--k_sweep", "2", "3"], ["--k", "3", "--k_sweep", "1"], ["--k", "3", "--k_sweep", "0"], ["--k", "3", "--k_sweep", "4097"],
                  ["--k", "3", "--k_sweep", "-2"]):
        with pytest.raises(ValueError, match="k_sweep"):
            cli.validate_args(_args(tmp_path, *extra)[1])
    for extra in (["--k_sweep", "2", "3"], ["--k", "3", "--k_sweep"], ["--k", "3", "--k_sweep", "2.5"], ["--k", "3", "--k_sweep", "x"]):
        with pytest.raises(SystemExit):
            _args(tmp_path, *extra)
    assert "--k" in capsys.readouterr().err
    import birdnet_stm32.cli.density as dcli

    d = dcli.build_parser().parse_args(["--database", "a.npz", "--output", "o.csv"])
    assert d.silhouette is False
    assert dcli.build_parser().parse_args(["--database", "a.npz", "--output", "o.csv", "--silhouette"]).silhouette is True


class _FakeIndex:
    paths, file_index, start_s = ["a.wav", "b,c.wav"], np.array([0, 0, 1, 1]), np.array([0.0, 3.0, 0.0, 1.5])

    def __len__(self):
        return 4


def _fake():
    index = _FakeIndex()
    result = SimpleNamespace(labels=np.array([0, 1, 1, -1]), score=np.array([0.5, 0.25, 1.0, 0.0], np.float32),
                             centroids=np.zeros((3, 2), np.float32), exemplar_idx=np.array([[0, -1], [2, 1], [-1, -1]]),
                             n_clusters=2, stability=np.array([1.5, 0.125]))
    sil = SimpleNamespace(silhouette=np.array([0.75, -0.5, 0.0, np.nan]), nearest=np.array([1, 0, 0, -1]), cluster_mean=np.array([0.75, -0.25, np.nan]),
                          mean=1.0 / 12.0)
    return index, result, sil


TODAY_ROWS = ("path,start_s,end_s,cluster,score\r\n" "a.wav,0.000,3.000,0,0.5\r\n" "a.wav,3.000,6.000,1,0.25\r\n" '"b,c.wav",0.000,3.000,1,1\r\n'
              '"b,c.wav",1.500,4.500,-1,0\r\n')
TODAY_SUMMARY = ("cluster,count,mean_score,exemplar_1,exemplar_2\r\n" "0,1,0.5,a.wav@0.000,\r\n" '1,2,0.625,"b,c.wav@0.000",a.wav@3.000\r\n' "2,0,0,,\r\n")
TODAY_DENSITY_SUMMARY = "cluster,count,stability,exemplar_1,exemplar_2\r\n" "0,1,1.5,a.wav@0.000,\r\n" '1,2,0.125,"b,c.wav@0.000",a.wav@3.000\r\n'


def test_writers_without_the_flag_write_the_bytes_they_wrote_before(tmp_path):
    import birdnet_stm32.cli.cluster as cli
    import birdnet_stm32.cli.density as dcli

    assert cli.CSV_COLUMNS == ("path", "start_s", "end_s", "cluster", "score") and cli.SUMMARY_COLUMNS == ("cluster", "count", "mean_score")
    assert dcli.CSV_COLUMNS == cli.CSV_COLUMNS and dcli.SUMMARY_COLUMNS == ("cluster", "count", "stability")
    index, result, sil = _fake()
    p = str(tmp_path / "o.csv")
    assert cli.write_clusters_csv(p, index, result, 3.0) == 4
    assert open(p, newline="").read() == TODAY_ROWS
    assert cli.write_summary_csv(p, index, result) == 3
    assert open(p, newline="").read() == TODAY_SUMMARY
    assert dcli.write_summary_csv(p, index, result) == 2
    assert open(p, newline="").read() == TODAY_DENSITY_SUMMARY
    assert cli.summary_path("x/o.csv") == "x/o_summary.csv" and cli.sweep_path("x/o.csv") == "x/o_sweep.csv" and cli.sweep_path("o") == "o_sweep.csv"


def test_writers_with_a_silhouette_append_their_columns(tmp_path):
    import csv

    import birdnet_stm32.cli.cluster as cli
    import birdnet_stm32.cli.density as dcli

    index, result, sil = _fake()
    p = str(tmp_path / "o.csv")
    cli.write_clusters_csv(p, index, result, 3.0, sil)
    got = list(csv.reader(open(p, newline="")))
    base = list(csv.reader(io.StringIO(TODAY_ROWS, newline="")))
    assert got[0] == base[0] + ["silhouette", "nearest_cluster"] == list(cli.CSV_COLUMNS + cli.SILHOUETTE_COLUMNS)
    assert [g[:5] for g in got] == base
    assert [g[5:] for g in got[1:]] == [["0.75", "1"], ["-0.5", "0"], ["0", "0"], ["", "-1"]]
    cli.write_summary_csv(p, index, result, sil)
    got = list(csv.reader(open(p, newline="")))
    base = list(csv.reader(io.StringIO(TODAY_SUMMARY, newline="")))
    assert got[0] == ["cluster", "count", "mean_score", "silhouette", "exemplar_1", "exemplar_2"]
    assert [g[:3] + g[4:] for g in got] == base and [g[3] for g in got[1:]] == ["0.75", "-0.25", ""]
    dcli.write_summary_csv(p, index, result, sil)
    got = list(csv.reader(open(p, newline="")))
    assert got[0] == ["cluster", "count", "stability", "silhouette", "exemplar_1", "exemplar_2"] and [g[3] for g in got[1:]] == ["0.75", "-0.25"]
    table = [dict(k=2, silhouette=0.5, mean_score=0.25, n_iter=3, converged=True, smallest_cluster=1, largest_cluster=3),
             dict(k=3, silhouette=0.125, mean_score=0.75, n_iter=25, converged=False, smallest_cluster=0, largest_cluster=4)]
    assert cli.write_sweep_csv(p, table) == 2
    assert open(p, newline="").read() == ("k,silhouette,mean_score,n_iter,converged,smallest_cluster,largest_cluster\r\n" "2,0.5,0.25,3,1,1,3\r\n"
                                          "3,0.125,0.75,25,0,0,4\r\n")
