"""Host tests of select (evaluation/select.py, cli/select.py): the specification against Euclidean farthest-first traversal in float64,
its properties (distinct picks, ties, the falling key sequence, exhaustion), every refusal, the ``min_key`` cut, the uncertainty weights
against hand-written values, the parser and both CSV layouts through a stubbed ``select_index``.  No device."""

import csv
import math
import os
import re

import numpy as np
import pytest

import select_cases as cases
from birdnet_stm32.evaluation import select as S


def _separated(N=120, D=6, seed=3):
    """Points on a coarse integer grid, normalised in float64: chord distances of different pairs differ by far more than float32 sees."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-6, 7, (N, D)).astype(np.float32)
    X[(X == 0).all(axis=1), 0] = 1
    return X


def _euclidean_farthest_first(X, start, budget):
    """The textbook traversal on the normalised rows in float64: farthest from the chosen set, the lowest index among equals."""
    Z = X.astype(np.float64)
    Z /= np.sqrt((Z * Z).sum(axis=1))[:, None]
    d = np.linalg.norm(Z - Z[start], axis=1)
    d[start] = -np.inf
    out = []
    for _ in range(budget):
        c = int(np.argmax(d))
        out.append(c)
        d = np.minimum(d, np.linalg.norm(Z - Z[c], axis=1))
        d[c] = -np.inf
        d[start] = -np.inf
        d[out] = -np.inf
    return out


def test_reference_is_euclidean_farthest_first_on_separated_data():
    X = _separated()
    budget = 25
    want = _euclidean_farthest_first(X, 7, budget)
    # the data must decide every step by more than float32 rounding: the gap between the best and the second-best squared distance
    Z = X.astype(np.float64) / np.sqrt((X.astype(np.float64) ** 2).sum(axis=1))[:, None]
    chosen = [7]
    for c in want:
        d2 = np.min(((Z[:, None, :] - Z[chosen][None, :, :]) ** 2).sum(axis=2), axis=1)
        d2[chosen] = -1
        top = np.sort(d2)[::-1]
        assert d2[c] == top[0] and (top[0] - top[1] > 1e-4 or top[0] == top[1] and c == int(np.argmax(d2))), "change the data: a step is too close to call"
        chosen.append(c)
    got = S.select_reference(X, budget, first=7, min_key=-np.inf)
    assert got.picked.tolist() == want and got.first == 7 and got.seeds.tolist() == [7]
    # key = 1 - cos = chord^2 / 2
    d2 = np.min(((Z[got.picked][:, None, :] - Z[[7]][None, :, :]) ** 2).sum(axis=2), axis=1)
    assert abs(float(got.key[0]) - d2[0] / 2) < 1e-6


def test_picks_are_distinct_never_a_seed_never_a_zero_row_and_ties_go_to_the_lowest_index():
    X = cases.lattice_rows(90, 12, 5)
    X[40] = X[10]
    X[70] = X[10]   # three copies: whichever is picked, it is row 10
    seeds = [3, 45, 88, 3]   # 45 and 88 are zero rows, 3 comes twice
    assert not X[45].any() and not X[88].any()
    res = S.select_reference(X, 87, seeds=seeds, min_key=-np.inf)   # every live row that is no seed
    assert res.seeds.tolist() == [3] and res.first == -1
    picked = res.picked.tolist()
    assert len(set(picked)) == 87 and 3 not in picked and 45 not in picked and 88 not in picked
    order = {r: i for i, r in enumerate(picked)}
    assert order[10] < order[40] < order[70], "copies are taken lowest index first"
    assert float(res.key[order[40]]) <= 2 ** -20 and float(res.key[order[70]]) <= 2 ** -20, "a copy of a taken row is at distance 0"
    assert res.nearest[45] == -1 and np.isnan(res.similarity[45]) and res.nearest[3] == 3 and res.similarity[3] == 1


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["float32", "int8"])
def test_key_sequence_never_increases(kind, weighted):
    X = cases.normal_clusters(400, 24, 6, 0.4, 9)
    zp = 0
    if kind == "int8":
        zp = -7
        X = np.clip(np.rint(X * 30) + zp, -128, 127).astype(np.int8)
    w = cases.weights(400, 4) if weighted else None
    res = S.select_reference(X, 120, weights=w, min_key=-np.inf, zero_point=zp)
    assert res.picked.size == 120 and res.key[0] == np.inf and res.picked[0] == res.first
    assert np.all(res.key[1:] <= res.key[:-1])
    if weighted:
        assert (w[res.picked[1:]] == 0).sum() == 0 or float(res.key[-1]) <= 0, "rows of weight 0 come last"


def test_a_budget_of_all_remaining_rows_takes_each_exactly_once():
    X = cases.lattice_rows(64, 9, 12)
    live = np.flatnonzero(np.abs(X).sum(axis=1) > 0)
    res = S.select_reference(X, live.size - 2, seeds=[int(live[0]), int(live[5])], weights=cases.weights(64, 1), min_key=-np.inf)
    assert sorted(res.picked.tolist() + res.seeds.tolist()) == live.tolist()
    assert np.all(res.similarity[live] == 1) and np.array_equal(res.nearest[live], live)
    whole = S.select_reference(X, live.size, min_key=-np.inf)
    assert sorted(whole.picked.tolist()) == live.tolist() and whole.seeds.size == 0


def test_run_reference_skips_bad_forced_entries_and_stops_at_minus_one():
    X = cases.lattice_rows(17, 4, 2)
    inv = S.inv_norms_reference(X)
    m, nearest = np.full(17, -np.inf, np.float32), np.full(17, -1, np.int32)
    picked, key = S.run_reference(X, inv, m, nearest, [99, 8, -1, 2], 4, 4 + 16)   # row 8 is a zero row
    assert picked[:4].tolist() == [99, 8, -1, 2] and np.isnan(key[:4]).all()
    assert sorted(picked[4:18].tolist()) == [i for i in range(17) if inv[i] != 0 and i != 2]
    assert picked[18:].tolist() == [-1, -1] and np.all(key[18:] == -np.inf)
    before = m.copy(), nearest.copy()
    again, key2 = S.run_reference(X, inv, m, nearest, [], 0, 2)
    assert again.tolist() == [-1, -1] and np.array_equal(m, before[0]) and np.array_equal(nearest, before[1])


def test_refusals():
    X = cases.lattice_rows(40, 8, 1)
    for kw, complaint in ((dict(budget=0), "budget 0 must be >= 1"), (dict(budget=39), "budget 39 above the 38"), (dict(budget=37, seeds=[1, 2]), "above the 36"),
                          (dict(budget=38, first=4), "above the 37"), (dict(budget=5, weights=np.ones(39)), "one per row"),
                          (dict(budget=5, weights=np.full(40, np.nan)), "not finite"), (dict(budget=5, weights=np.full(40, 1e300)), "not finite"),
                          (dict(budget=5, weights=-np.ones(40)), "negative"), (dict(budget=5, weights=np.ones((40, 1))), "one per row"),
                          (dict(budget=5, seeds=[40]), r"outside 0\.\.39"), (dict(budget=5, seeds=[-1]), r"outside 0\.\.39"),
                          (dict(budget=5, seeds=[0.5]), "row numbers"), (dict(budget=5, first=40), r"first 40 outside 0\.\.39"),
                          (dict(budget=5, first=-1), "first -1 outside"), (dict(budget=5, first=20), "first 20 is a zero row")):
        with pytest.raises(ValueError, match=complaint):
            S.select_reference(X, **kw)
    one = np.zeros((5, 3), np.float32)
    one[2, 0] = 1
    with pytest.raises(ValueError, match="at least 2 non-zero rows"):
        S.select_reference(one, 1)
    with pytest.raises(ValueError, match="above 2048"):
        S.select_reference(np.ones((3, 2049), np.float32), 1)
    with pytest.raises(ValueError, match="at most 2097152"):
        S._prepare(S.MAX_N + 5, 4, np.arange(S.MAX_N + 1), 3, None, None, None)
    with pytest.raises(ValueError, match="not finite"):
        S.select_reference(np.full((4, 2), np.inf, np.float32), 1)
    assert S.select_reference(X, 38, min_key=-np.inf).picked.size == 38, "a budget of every live row is allowed"


def test_min_key_cuts_before_the_first_pick_below_it():
    X = cases.normal_clusters(200, 16, 5, 0.3, 4)
    full = S.select_reference(X, 50, first=0, min_key=-np.inf)
    r = float(full.key[20])
    cut = S.select_reference(X, 50, first=0, min_key=r)
    keep = int(np.flatnonzero(full.key < np.float32(r))[0])
    assert keep >= 21 and cut.picked.tolist() == full.picked[:keep].tolist() and np.array_equal(cut.key, full.key[:keep])
    shorter = S.select_reference(X, keep, first=0, min_key=-np.inf)
    assert np.array_equal(cut.nearest, shorter.nearest) and np.array_equal(cut.similarity, shorter.similarity), "the state is that of the picks that remain"
    none = S.select_reference(X, 50, first=0, min_key=3.0)
    assert none.picked.size == 0 and none.key.size == 0 and (none.nearest == 0).all()
    dup = np.vstack([X[:30], X[:30]])
    res = S.select_reference(dup, 59, first=0, min_key=1e-6)   # a copy of a taken row is within rounding of distance 0: nothing new
    assert res.picked.size <= 30 and len(set((res.picked % 30).tolist()) | {0}) == res.picked.size + 1


def test_uncertainty_modes_against_hand_written_values():
    F = np.array([[0.5, 0.25, 0.25], [2.0, 0.0, 0.0], [0.0, 0.0, 0.0], [np.nan, np.nan, np.nan], [1.0, 1.0, 0.0], [0.2, 0.2, 0.2]], np.float32)
    ln3 = math.log(3)
    want = {
        "least_confidence": [0.5, 0.0, 1.0, 0.0, 0.5, 2 / 3],
        "margin": [0.75, 0.0, 1.0, 0.0, 1.0, 1.0],
        "entropy": [(0.5 * math.log(2) + 0.5 * math.log(4)) / ln3, 0.0, 1.0, 0.0, math.log(2) / ln3, 1.0],
    }
    for mode, values in want.items():
        got = S.uncertainty_reference(F, mode)
        assert got.dtype == np.float32 and np.allclose(got, np.asarray(values, np.float32), rtol=0, atol=2 ** -23), (mode, got)
    one = np.array([[0.7], [0.0], [np.nan]], np.float32)
    assert S.uncertainty_reference(one, "least_confidence").tolist() == [0.0, 1.0, 0.0]
    assert S.uncertainty_reference(one, "margin").tolist() == [0.0, 1.0, 0.0], "p2 = 0 when C = 1"
    assert S.uncertainty_reference(one, "entropy").tolist() == [0.0, 1.0, 0.0], "0 when C = 1"
    with pytest.raises(ValueError, match="uncertainty must be one of"):
        S.uncertainty_reference(F, "variance")
    with pytest.raises(ValueError, match=r"\[N, C\]"):
        S.uncertainty_reference(np.zeros(4), "margin")
    w = S.uncertainty_reference(F, "margin")
    assert np.isfinite(w).all() and (w >= 0).all(), "the weights pass select's own check"


# ------------------------------------------------------------------------------------------------------------------------- CLI
def _read(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_cli_validation(tmp_path):
    import birdnet_stm32.cli.select as cli

    db, out = str(tmp_path / "db.npz"), str(tmp_path / "s.csv")
    open(db, "wb").close()
    base = ["--database", db, "--output", out]
    args = cli.build_parser().parse_args(base + ["--budget", "5"])
    assert (args.labels, args.labelled, args.scores, args.uncertainty, args.first, args.min_key, args.coverage_out, args.device) == ("", None, "", None, None, 0.0, "", 0)
    cli.validate_args(args)
    for extra, complaint in ((["--budget", "0"], "--budget"), (["--budget", "5", "--first", "-2"], "--first"), (["--budget", "5", "--min_key", "nan"], "--min_key"),
                             (["--budget", "5", "--uncertainty", "entropy"], "--uncertainty needs --scores"),
                             (["--budget", "5", "--scores", str(tmp_path / "none.npz")], "file not found"),
                             (["--budget", "5", "--labels", str(tmp_path / "none.csv")], "file not found")):
        with pytest.raises(SystemExit, match=complaint):
            cli.main(base + extra)
    for bad in ([], ["--budget", "5", "--labels", db, "--labelled", db], ["--budget", "5", "--scores", db, "--uncertainty", "variance"]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(base + bad)
    assert cli.UNCERTAINTY_MODES == S.UNCERTAINTY_MODES


def test_cli_writes_both_layouts_through_a_stubbed_select_index(tmp_path, monkeypatch, capsys):
    import birdnet_stm32.cli.select as cli

    X = cases.lattice_rows(60, 8, 41)
    db, out, cov, scores, labels_csv = (str(tmp_path / name) for name in ("db.npz", "select.csv", "cov.csv", "f.npz", "labels.csv"))
    file_index, start_s, paths = cases.synthetic_archive(db, X, files=3)
    F = np.random.default_rng(1).random((60, 2)).astype(np.float32)
    F[30] = np.nan   # (a zero row)
    F[11] = 0
    with open(scores, "wb") as f:
        np.savez(f, F=F, labels=np.asarray(["owl", "wren"]), file_index=file_index, start_s=start_s, paths=np.asarray(paths))
    with open(labels_csv, "w") as f:
        f.write("path,start_s,label\nrec/file_0.wav,6.0,owl\nrec/file_1.wav,30.0,wren\n")   # rows 2 and 30 (a zero row)
    seen = {}

    def stub(index, budget, seeds=None, weights=None, first=None, min_key=0.0, device=0, ctx=None):
        seen.update(budget=budget, seeds=None if seeds is None else np.asarray(seeds).tolist(), weights=weights, first=first, min_key=min_key, device=device)
        return S.select_reference(index.embeddings, budget, seeds=seeds, weights=weights, first=first, min_key=min_key, zero_point=index.zero_point)

    monkeypatch.setattr(S, "select_index", stub)
    res = cli.main(["--database", db, "--budget", "8", "--output", out, "--labels", labels_csv, "--scores", scores, "--coverage_out", cov, "--min_key=-inf"])
    assert "Chose 8 of 60 rows x 8 (float32) after 1 chosen already, weighted by margin" in capsys.readouterr().out
    w = S.uncertainty_reference(F, "margin")
    assert seen["budget"] == 8 and seen["seeds"] == [2, 30] and np.array_equal(seen["weights"], w) and seen["first"] is None and seen["min_key"] == -np.inf
    assert res.seeds.tolist() == [2] and w[30] == 0 and w[11] == 1
    taken = np.zeros(60, int)
    taken[res.picked], taken[res.seeds] = 1, 2
    rows = _read(out)
    assert rows[0] == list(cli.CSV_COLUMNS) == ["rank", "row", "path", "start_s", "key", "weight", "guess", "covers"] and len(rows) == 9
    for rank, (line, row, key) in enumerate(zip(rows[1:], res.picked.tolist(), res.key.tolist())):
        covers = int(((res.nearest == row) & (taken == 0)).sum())
        guess = "" if row == 30 else ["owl", "wren"][int(np.argmax(F[row]))]
        assert line == [str(rank), str(row), paths[file_index[row]], f"{start_s[row]:.3f}", f"{key:.7g}", f"{float(w[row]):.7g}", guess, str(covers)]
    assert sum(int(r[7]) for r in rows[1:]) + int(((res.nearest == 2) & (taken == 0)).sum()) == int((taken == 0).sum()) - 2, "every open live row is covered once"
    lines = _read(cov)
    assert lines[0] == list(cli.COVERAGE_COLUMNS) == ["row", "path", "start_s", "nearest_row", "similarity", "taken"] and len(lines) == 61
    for i, line in enumerate(lines[1:]):
        sim = res.similarity[i]
        assert line == [str(i), paths[file_index[i]], f"{start_s[i]:.3f}", "" if res.nearest[i] < 0 else str(int(res.nearest[i])),
                        "" if np.isnan(sim) else f"{float(sim):.7g}", str(taken[i])]
    assert lines[31][3:] == ["", "", "0"] and lines[3][3:] == ["2", "1", "2"]
    # without scores: weight 1, no guess; --first goes through
    cli.main(["--database", db, "--budget", "3", "--output", out, "--first", "5"])
    assert seen["first"] == 5 and seen["weights"] is None and seen["seeds"] is None and seen["min_key"] == 0.0
    plain = _read(out)
    assert all(r[5] == "1" and r[6] == "" for r in plain[1:]) and len(plain) == 4
    # scores that do not line up are refused
    with open(scores, "wb") as f:
        np.savez(f, F=F, labels=np.asarray(["owl", "wren"]), file_index=file_index, start_s=start_s + 1.0, paths=np.asarray(paths))
    with pytest.raises(SystemExit, match="file_index / start_s differ"):
        cli.main(["--database", db, "--budget", "3", "--output", out, "--scores", scores])
    with open(scores, "wb") as f:
        np.savez(f, F=F[:50], labels=np.asarray(["owl", "wren"]), file_index=file_index[:50], start_s=start_s[:50], paths=np.asarray(paths))
    with pytest.raises(SystemExit, match="the database has 60 rows"):
        cli.main(["--database", db, "--budget", "3", "--output", out, "--scores", scores])
    with pytest.raises(SystemExit, match="budget 100 above"):
        cli.main(["--database", db, "--budget", "100", "--output", out])


def test_dispatcher_binding_and_header():
    import birdnet_stm32.__main__ as m
    from birdnet_stm32 import _hip

    assert "select" in m.USAGE and "``select``" in m.__doc__
    with open(os.path.join(os.path.dirname(_hip.LIB_PATH), "..", "..", "include", "birdnet_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"BN_API int bn_select_run\(", hdr) and "bn_select_run" in _hip.EXPORTS
    for name in ("STEP_ROWS", "MIN_WG_STEPS", "MAX_WGS"):
        assert int(re.search(rf"#define BN_SELECT_{name} (\d+)", hdr).group(1)) == getattr(_hip, "SELECT_" + name)
    assert _hip.SELECT_STEP_ROWS == 64 and S.MAX_N == 1 << 21 and S.MAX_D == 2048
    if os.path.isfile(_hip.LIB_PATH):
        assert "select_pass_kernel" in _hip.load_library().bn_kernel_names().decode().split("\n")
    assert S.device_bytes_needed(1000, 256, 4) > 1000 * 256 * 4
