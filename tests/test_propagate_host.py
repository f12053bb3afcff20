"""Host tests of propagate (evaluation/propagate.py, cli/propagate.py): the float64 recurrence against scikit-learn's LabelSpreading, the
float32 specification against the float64 one, the graph, every refusal, the parsers, the hold-out split, components without seeds and
zero rows.  No device."""

import csv
import os
import re
import warnings

import numpy as np
import pytest

import propagate_cases as cases
from birdnet_stm32.evaluation import propagate as P


@pytest.fixture(scope="module")
def reference():
    """The planted run at tol = 1e-3 and at tol = 0 (200 updates), each once, with its float64 companion."""
    X, _, seed = cases.planted()
    out = {}
    for tol, max_iter in ((1e-3, 30), (0.0, 200)):
        out[tol] = P.propagate_reference(X, seed, cases.C, neighbours=cases.K, tau=cases.TAU, alpha=cases.ALPHA, max_iter=max_iter, tol=tol, float64=True)
    return out


def _dense_w(res, n):
    rowptr, col, w = P.symmetrize_max(res.neighbour_idx, P.edge_weights(res.neighbour_score, cases.TAU), n)
    W = np.zeros((n, n))
    W[np.repeat(np.arange(n), np.diff(rowptr)), col] = w
    return W


@pytest.mark.parametrize("tol,max_iter,n_iter", [(1e-3, 30, 5), (0.0, 200, 200)])
def test_float64_recurrence_is_scikit_learns_label_spreading(reference, tol, max_iter, n_iter):
    from sklearn.semi_supervised import LabelSpreading

    X, _, seed = cases.planted()
    res = reference[tol]
    W = _dense_w(res, cases.N)
    assert np.array_equal(W, W.T) and not W.diagonal().any()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (max_iter reached without convergence at tol = 0)
        ls = LabelSpreading(kernel=lambda A, B: W, alpha=cases.ALPHA, max_iter=max_iter, tol=tol).fit(X, seed)
    assert list(ls.classes_) == list(range(cases.C))
    ours = P.normalized_rows(res.extra["F64"])
    worst = float(np.abs(ours - ls.label_distributions_).max())
    print(f"tol {tol}: |ours - sklearn| max {worst:.3g}, n_iter {res.extra['n_iter64']} vs {ls.n_iter_}")
    assert worst <= 1e-12
    assert np.array_equal(res.extra["labels64"], ls.transduction_)
    assert res.extra["n_iter64"] == ls.n_iter_ == n_iter


def test_float32_specification_against_float64(reference):
    res = reference[1e-3]
    F32, F64 = P.normalized_rows(res.F), P.normalized_rows(res.extra["F64"])
    worst = float(np.abs(F32 - F64).max())
    print(f"normalised rows: float32 against float64 max {worst:.3g}")
    assert worst <= 1e-5
    assert np.array_equal(res.labels, res.extra["labels64"]) and res.n_iter == res.extra["n_iter64"] == 5
    assert len(res.delta_history) == 6 and res.delta_history[0] == cases.SEEDS and res.delta_history[-1] < 1e-3 <= res.delta_history[-2]
    _, true, _ = cases.planted()
    assert (res.labels == true).mean() > 0.5, "the planted classes come back far above chance (1 / 5)"
    assert np.all((res.scores > 0) & (res.scores <= 1))


def test_symmetrize_max_takes_the_union_and_the_larger_weight():
    idx = np.asarray([[1, 2], [0, 3], [2, -1], [0, 9]])   # row 2 names itself and nothing; 9 is out of range
    w = np.asarray([[0.5, 0.25], [0.75, 0.125], [9.0, 9.0], [0.0625, 9.0]])
    rowptr, col, val = P.symmetrize_max(idx, w, 4)
    dense = np.zeros((4, 4))
    dense[np.repeat(np.arange(4), np.diff(rowptr)), col] = val
    want = np.zeros((4, 4))
    for i, j, v in ((0, 1, 0.75), (0, 2, 0.25), (1, 3, 0.125), (0, 3, 0.0625)):
        want[i, j] = want[j, i] = v
    assert np.array_equal(dense, want)
    assert col.dtype == np.int32 and rowptr.dtype == np.int64 and all(np.all(np.diff(col[a:b]) > 0) for a, b in zip(rowptr[:-1], rowptr[1:]))
    empty = P.symmetrize_max(np.full((3, 2), -1), np.ones((3, 2)), 3)
    assert empty[0].tolist() == [0, 0, 0, 0] and empty[1].size == 0 and empty[2].size == 0
    with pytest.raises(ValueError):
        P.symmetrize_max(idx, w[:, :1], 4)


def test_project_symmetrize_is_unchanged():
    from birdnet_stm32.evaluation.project import symmetrize

    rowptr, col, val = symmetrize(np.asarray([[1], [0], [0]]), np.asarray([[0.5], [0.25], [1.0]]), 3)
    assert rowptr.tolist() == [0, 2, 3, 4] and col.tolist() == [1, 2, 0, 0]
    assert np.array_equal(val, np.asarray([0.75, 1.0, 0.75, 1.0], np.float64).astype(np.float32) / np.float32(6))


def test_normalisation_adds_a_row_in_ascending_column_order():
    rng = np.random.default_rng(3)
    idx = np.stack([rng.choice(np.delete(np.arange(40), i), 6, replace=False) for i in range(40)])
    score = rng.uniform(0.2, 1.0, idx.shape).astype(np.float32)
    rowptr, col, val32, val64 = P.build_graph(idx, score, 40, 0.1)
    _, _, w = P.symmetrize_max(idx, P.edge_weights(score, 0.1), 40)
    d = np.zeros(40)
    for i in range(40):
        for t in range(rowptr[i], rowptr[i + 1]):
            d[i] += w[t]
    row = np.repeat(np.arange(40), np.diff(rowptr))
    assert np.array_equal(val64, w / np.sqrt(d[row] * d[col])) and np.array_equal(val32, val64.astype(np.float32)) and val32.dtype == np.float32
    dense = np.zeros((40, 40))
    dense[row, col] = val64
    assert np.array_equal(dense, dense.T)
    assert np.array_equal(P.edge_weights(np.float32([1.0, 0.9]), 0.1), np.exp((np.float32([1.0, 0.9]).astype(np.float64) - 1.0) / 0.1))
    # weights that underflow leave zeros, not NaN
    assert np.array_equal(P.normalize(np.asarray([0, 1, 2]), np.asarray([1, 0]), np.zeros(2)), np.zeros(2))


def test_step_reference_is_the_scalar_loop():
    rowptr, col, val = cases.step_matrix(17, 5)
    F, lab = cases.step_labels(17, 3, 5)
    got = P.step_reference(rowptr, col, val, F, lab, 0.2)
    a, keep = np.float32(0.2), np.float32(1) - np.float32(0.2)
    for i in range(17):
        for c in range(3):
            acc = np.float32(0)
            for t in range(rowptr[i], rowptr[i + 1]):
                if 0 <= col[t] < 17:
                    acc = np.float32(acc + np.float32(val[t] * F[col[t], c]))
            want = np.float32(np.float32(a * acc) + (keep if lab[i] == c else np.float32(0)))
            assert got[i, c].view(np.uint32) == want.view(np.uint32), (i, c)
    assert got.dtype == np.float32 and rowptr[3] == rowptr[4], "row 3 is empty: it keeps only its own label"


def test_decision_ties_and_rows_without_a_label():
    F = np.float32([[0.25, 0.5, 0.5], [0, 0, 0], [1, 0, 0], [0.125, 0.125, 0.125]])
    label, score = P.decide_reference(F)
    assert label.tolist() == [1, -1, 0, 0] and score.tolist() == [np.float32(0.4), 0.0, 1.0, np.float32(1 / 3)]
    assert P.apply_min_score(label, score, 0.35).tolist() == [1, -1, 0, -1] and label.tolist() == [1, -1, 0, 0]
    assert P.apply_min_score([2, -1], np.float32([0.5, np.nan]), 0.0).tolist() == [2, -1]


def test_components_without_seeds_and_zero_rows():
    rng = np.random.default_rng(1)
    a = np.abs(rng.standard_normal((12, 8))).astype(np.float32)
    a[:, 4:] = 0
    b = np.abs(rng.standard_normal((12, 8))).astype(np.float32)
    b[:, :4] = 0   # (orthogonal to a: with k = 8 < 11 no edge joins the two halves, and each half is one component)
    rows = np.concatenate([a, np.zeros((2, 8), np.float32), b])
    seed = np.full(26, -1, np.int32)
    seed[0], seed[5], seed[12] = 0, 2, 1   # (row 12 is a zero row: its label is ignored)
    res = P.propagate_reference(rows, seed, 3, neighbours=8)
    assert res.nonzero.tolist() == list(range(12)) + list(range(14, 26))
    assert np.all(res.labels[12:14] == -1) and np.isnan(res.scores[12:14]).all() and np.isnan(res.F[12:14]).all()
    assert np.all(res.labels[14:] == -1) and np.all(res.scores[14:] == 0) and not res.F[14:].any()
    assert set(res.labels[:12]) <= {0, 2} and res.labels[0] == 0 and res.labels[5] == 2 and np.all(res.scores[:12] > 0)
    assert not np.nan_to_num(res.F[:, 1]).any(), "a class without seeds is allowed and wins nothing"
    q = P.propagate_reference(np.where(rows > 0, 60, 5).astype(np.int8), seed, 3, neighbours=3, zero_point=5)
    assert np.all(q.labels[12:14] == -1) and np.isnan(q.scores[12:14]).all() and q.nonzero.size == 24


def test_every_refusal():
    X, _, seed = cases.planted()
    ok = dict(neighbours=7, tau=0.1, alpha=0.2, max_iter=30, tol=1e-3)

    def run(rows=X, seed_label=seed, classes=cases.C, **kw):
        return P.propagate_reference(rows, seed_label, classes, **{**ok, **kw})

    for kw, text in ((dict(neighbours=0), "neighbours"), (dict(neighbours=240), "below the number"), (dict(neighbours=129), "above the 128"),
                     (dict(tau=0.0), "tau"), (dict(tau=float("inf")), "tau"), (dict(tau=float("nan")), "tau"), (dict(alpha=0.0), "alpha"), (dict(alpha=1.0), "alpha"),
                     (dict(alpha=float("nan")), "alpha"), (dict(max_iter=-1), "max_iter"), (dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"),
                     (dict(holdout=1.0), "holdout"), (dict(holdout=-0.1), "holdout"), (dict(classes=0), "classes"), (dict(classes=4097), "classes"),
                     (dict(classes=4), "outside -1..3"), (dict(seed_label=np.full(240, -1, np.int32)), "no labelled"),
                     (dict(seed_label=seed[:10]), "one per row"), (dict(seed_label=seed.astype(np.float32)), "integers"),
                     (dict(seed_label=np.where(seed < 0, -2, seed)), "outside -1"), (dict(holdout=0.01), "hides 0")):
        with pytest.raises(ValueError, match=text):
            run(**kw)
    with pytest.raises(ValueError, match="at least 2 non-zero rows"):
        run(rows=np.concatenate([X[:1], np.zeros((5, cases.D), np.float32)]), seed_label=np.zeros(6, np.int32), classes=1, neighbours=1)
    zero_seeded = np.full(240, -1, np.int32)
    zero_seeded[0] = 0
    rows = X.copy()
    rows[0] = 0
    with pytest.raises(ValueError, match="no labelled non-zero row"):
        run(rows=rows, seed_label=zero_seeded)
    with pytest.raises(ValueError, match="at most"):
        P.check_propagate_args((1 << 21) + 1, 2, 15, 0.1, 0.2, 30, 1e-3)
    P.check_propagate_args(1 << 21, 4096, 128, 0.1, 0.2, 0, 0.0, 0.5)
    assert run(max_iter=0).n_iter == 0


def test_holdout_split_and_report():
    X, true, seed = cases.planted()
    nonzero = np.arange(cases.N)
    hidden = P.holdout_split(seed, nonzero, 0.25, 0)
    seeds = np.flatnonzero(seed >= 0)
    assert hidden.size == 5 and np.array_equal(hidden, seeds[np.random.default_rng([0]).permutation(20)[:5]])
    assert not np.array_equal(hidden, P.holdout_split(seed, nonzero, 0.25, 1))
    assert P.holdout_split(seed, nonzero[nonzero != hidden[0]], 0.25, 0).size == 5 and hidden[0] not in P.holdout_split(seed, nonzero[nonzero != hidden[0]], 0.25, 0)
    res = P.propagate_reference(X, seed, cases.C, neighbours=cases.K, holdout=0.25, seed=0)
    plain = P.propagate_reference(X, seed, cases.C, neighbours=cases.K)
    assert np.array_equal(res.labels, plain.labels) and np.array_equal(res.F, plain.F) and res.n_iter == plain.n_iter, "what is returned uses every seed"
    shown = seed.copy()
    shown[hidden] = -1
    blind = P.propagate_reference(X, shown, cases.C, neighbours=cases.K)
    rep = res.holdout
    assert np.array_equal(rep.rows, hidden) and np.array_equal(rep.true, true[hidden]) and np.array_equal(rep.predicted, blind.labels[hidden])
    assert rep.accuracy == (blind.labels[hidden] == true[hidden]).mean()
    for c in range(cases.C):
        m = true[hidden] == c
        assert (np.isnan(rep.recall[c]) and not m.any()) or rep.recall[c] == (blind.labels[hidden][m] == c).mean()
    assert plain.holdout is None


# ---------------------------------------------------------------------------------------------------------------- command line
def _index(paths, file_index, start_s):
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    n = len(file_index)
    return EmbeddingIndex(np.ones((n, 4), np.float32), file_index, start_s, paths)


def test_labels_csv_parsers(tmp_path):
    import birdnet_stm32.cli.propagate as cli

    index = _index(["a/x.wav", "a/y.wav", "b/z.wav"], [0, 0, 1, 1, 2], [0.0, 3.0, 0.0, 3.0, 0.0])
    whole, timed = tmp_path / "whole.csv", tmp_path / "timed.csv"
    whole.write_text("path,label\na/x.wav,wren\nb/z.wav,owl\n")
    timed.write_text("path,start_s,label\na/y.wav,3.000,wren\na/x.wav,0,owl\n")
    seed, names = cli.seeds_from_records(index, cli.read_labels_csv(str(whole)))
    assert names == ["owl", "wren"] and seed.tolist() == [1, 1, -1, -1, 0] and seed.dtype == np.int32
    seed, names = cli.seeds_from_records(index, cli.read_labels_csv(str(timed)))
    assert seed.tolist() == [0, -1, -1, 1, -1]
    assert cli.seeds_from_records(index, [(os.path.join(os.getcwd(), "a", "x.wav"), None, "owl")])[0].tolist() == [0, 0, -1, -1, -1], "resolved names match too"
    for text, complaint in (("path,label\nc/none.wav,owl\n", "c/none.wav matches no row"), ("path,start_s,label\na/x.wav,6.0,owl\n", r"a/x.wav at 6.000 s matches no row"),
                            ("path,label\na/x.wav,owl\na/x.wav,wren\n", "is labelled owl and wren"), ("file,label\na/x.wav,owl\n", "header"),
                            ("path,label\n", "no labels"), ("path,label\na/x.wav,\n", "empty"), ("path,start_s,label\na/x.wav,soon,owl\n", "not a number")):
        bad = tmp_path / "bad.csv"
        bad.write_text(text)
        with pytest.raises(ValueError, match=complaint):
            cli.seeds_from_records(index, cli.read_labels_csv(str(bad)))


def test_labelled_archives_take_the_folder_names():
    import birdnet_stm32.cli.propagate as cli

    index = _index(["field/rec.wav", "train/wren/1.wav", "train/owl/2.wav", "train/wren/3.wav"], [0, 0, 0, 1, 2, 2, 3], np.arange(7) * 3.0)
    seed, names = cli.seeds_from_folders(index, 3)
    assert names == ["owl", "wren"] and seed.tolist() == [-1, -1, -1, 1, 0, 0, 1]
    with pytest.raises(ValueError, match="no parent folder"):
        cli.seeds_from_folders(_index(["field/rec.wav", "loose.wav"], [0, 1], [0.0, 0.0]), 1)


def test_writers_and_arguments(tmp_path):
    import birdnet_stm32.cli.propagate as cli

    index = _index(["a/x.wav", "b/z.wav"], [0, 0, 1], [0.0, 3.0, 0.0])
    out = str(tmp_path / "p.csv")
    labels, scores, seed = np.int32([1, -1, 0]), np.float32([0.75, np.nan, 0.5]), np.int32([1, -1, -1])
    assert cli.write_propagate_csv(out, index, labels, scores, seed, ["owl", "wren"]) == 3
    with open(out, newline="") as f:
        assert list(csv.reader(f)) == [list(cli.CSV_COLUMNS), ["0", "a/x.wav", "0.000", "wren", "0.75", "1"], ["1", "a/x.wav", "3.000", "", "", "0"],
                                       ["2", "b/z.wav", "0.000", "owl", "0.5", "0"]]
    report = P.HoldoutReport(np.int64([0]), np.int32([1]), np.int32([1]), 1.0, np.asarray([np.nan, 1.0]))
    assert cli.summary_path(out) == str(tmp_path / "p_summary.csv") and cli.labels_path(out) == str(tmp_path / "p_labels.txt")
    cli.write_summary_csv(cli.summary_path(out), labels, scores, seed, ["owl", "wren"], report)
    with open(cli.summary_path(out), newline="") as f:
        assert list(csv.reader(f)) == [list(cli.SUMMARY_COLUMNS), ["owl", "0", "1", "0.5", ""], ["wren", "1", "1", "0.75", "1"]]
    db = str(tmp_path / "db.npz")
    open(db, "wb").close()
    base = ["--database", db, "--output", out]
    args = cli.build_parser().parse_args(base + ["--labels", db])
    assert (args.neighbours, args.tau, args.alpha, args.max_iter, args.tol, args.min_score, args.holdout, args.holdout_seed) == (15, 0.1, 0.2, 30, 1e-3, 0.0, 0.0, 0)
    cli.validate_args(args)
    for extra, complaint in ((["--neighbours", "0"], "--neighbours"), (["--neighbours", "129"], "--neighbours"), (["--tau", "0"], "--tau"), (["--alpha", "1"], "--alpha"),
                             (["--max_iter", "-1"], "--max_iter"), (["--tol", "-1"], "--tol"), (["--min_score", "2"], "--min_score"), (["--holdout", "1"], "--holdout")):
        with pytest.raises(SystemExit, match=complaint):
            cli.main(base + ["--labels", db] + extra)
    with pytest.raises(SystemExit, match="file not found"):
        cli.main(base + ["--labels", str(tmp_path / "none.csv")])
    for bad in ([], ["--labels", db, "--labelled", db]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(base + bad)


def test_dispatcher_binding_and_header():
    import birdnet_stm32.__main__ as m
    from birdnet_stm32 import _hip

    assert "propagate" in m.USAGE and "propagate" in m.__doc__
    with open(os.path.join(os.path.dirname(_hip.LIB_PATH), "..", "..", "include", "birdnet_hip.h")) as f:
        hdr = f.read()
    for name in ("bn_propagate_step", "bn_propagate_decide"):
        assert re.search(r"BN_API int " + name + r"\(", hdr) and name in _hip.EXPORTS
    for name, value in (("MAX_CLASSES", P.MAX_CLASSES), ("MAX_ROW_LANES", _hip.PROPAGATE_MAX_ROW_LANES)):
        assert int(re.search(rf"#define BN_PROPAGATE_{name} (\d+)", hdr).group(1)) == value == getattr(_hip, "PROPAGATE_" + name)
    assert re.search(r"#define BN_PROPAGATE_MAX_N \(1 << 21\)", hdr) and _hip.PROPAGATE_MAX_N == 1 << 21
    from birdnet_stm32.evaluation.project import MAX_N

    assert MAX_N == _hip.PROPAGATE_MAX_N
    if os.path.isfile(_hip.LIB_PATH):
        names = _hip.load_library().bn_kernel_names().decode().split("\n")
        assert {"propagate_step_kernel", "propagate_delta_kernel", "propagate_decide_kernel"} <= set(names)
    assert P.device_bytes_needed(1000, 256, 4, 15, 50) > 2 * 1000 * 50 * 4
