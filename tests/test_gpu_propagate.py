"""GPU tests of propagate (csrc/bn_propagate.hip, evaluation/propagate.py, cli/propagate.py) against the numpy specification.

The update has one value whatever the machine: every (i, c) adds its row's entries in stored order, each operation rounded to float32, so
``bn_propagate_step`` is held to ``step_reference`` bit for bit, on matrices with empty rows, one-entry rows, a hub and columns out of
range, between guard rows of a fill pattern.  The change ``delta`` and the decision's score are sums in the implementation's own order and
are held to written-out rounding bounds; the decision's label is exact.  ``propagate_index`` is compared teacher-forced (the reference
takes the device's neighbours: bit for bit) and independently (labels, wherever the float64 reference separates the top two classes)."""

import csv
import functools

import numpy as np
import pytest

import propagate_cases as cases
from birdnet_stm32.evaluation import propagate as P

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0BEEF
FILL_LABEL = -77
U = 2.0 ** -24


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


def _guarded(torch, n, C, off):
    """A label matrix of n rows between two guard rows of the fill pattern: (the whole buffer as int32, the view of the n rows).  With
    ``off`` everything starts one element behind a 16-byte boundary."""
    flat = torch.full(((n + 2) * C + 1,), NAN_BITS, dtype=torch.int32, device="cuda")
    body = flat[1:] if off else flat[:-1]
    rows = body[C:(n + 1) * C].view(n, C)
    assert rows.data_ptr() % 16 == (4 * C + (4 if off else 0)) % 16
    return body, rows


def _guards_intact(body, n, C):
    b = body.cpu().numpy()
    return np.all(b[:C] == NAN_BITS) and np.all(b[(n + 1) * C:] == NAN_BITS)


@functools.lru_cache(maxsize=None)
def _matrix(n):
    return cases.step_matrix(n, 7 + n)


def _device_steps(torch, ctx, csr, F, lab, alpha, steps, off=False, want_delta=True):
    """``steps`` updates through the C ABI, the two label matrices ping-ponging: the matrices after every update and the deltas."""
    from birdnet_stm32 import _hip

    n, C = F.shape
    rowptr, col, val = csr
    d_rowptr, d_lab = torch.from_numpy(rowptr).cuda(), torch.from_numpy(lab).cuda()
    d_col = torch.from_numpy(col if col.size else np.zeros(1, np.int32)).cuda()
    d_val = torch.from_numpy(val if val.size else np.zeros(1, np.float32)).cuda()
    bodies, views = zip(*(_guarded(torch, n, C, off) for _ in range(2)))
    views[0].copy_(torch.from_numpy(F.view(np.int32)).cuda())
    d_delta = torch.full((3,), -5.0, dtype=torch.float64, device="cuda")
    out, deltas = [], []
    for t in range(steps):
        a, b = views[t % 2], views[1 - t % 2]
        _hip.check(ctx.lib.bn_propagate_step(ctx.handle, d_rowptr.data_ptr(), d_col.data_ptr(), d_val.data_ptr(), a.data_ptr(), d_lab.data_ptr(), n, C,
                                             _hip.c_float(alpha), b.data_ptr(), d_delta[1:].data_ptr() if want_delta else None, None))
        torch.cuda.synchronize()
        out.append(b.cpu().numpy().view(np.float32).copy())
        d = d_delta.cpu().numpy()
        assert d[0] == -5.0 and d[2] == -5.0, "delta's neighbours were written"
        deltas.append(float(d[1]))
        assert _guards_intact(bodies[0], n, C) and _guards_intact(bodies[1], n, C), "a guard row was written"
    assert np.array_equal(d_rowptr.cpu().numpy(), rowptr) and np.array_equal(d_lab.cpu().numpy(), lab), "an input changed"
    return out, deltas


def _reference_steps(csr, F, lab, alpha, steps):
    out, deltas = [], []
    for _ in range(steps):
        nxt = P.step_reference(*csr, F, lab, alpha)
        deltas.append(P.delta_reference(nxt, F))
        out.append(nxt)
        F = nxt
    return out, deltas


def _check_steps(torch, ctx, n, C, off=False):
    csr = _matrix(n)
    F, lab = cases.step_labels(n, C, 31 * n + C)
    for alpha in (0.2, 0.99):
        want, want_delta = _reference_steps(csr, F, lab, alpha, 7)
        got, got_delta = _device_steps(torch, ctx, csr, F, lab, alpha, 7, off)
        for t in (0, 6):
            assert np.array_equal(got[t].view(np.uint32), want[t].view(np.uint32)), f"alpha {alpha}: the matrix after {t + 1} updates differs"
        for t in range(7):   # a float64 sum of n C exact terms, in any order
            assert abs(got_delta[t] - want_delta[t]) <= n * C * 2.0 ** -52 * want_delta[t], (alpha, t, got_delta[t], want_delta[t])


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 63, 64, 65, 130])
@pytest.mark.parametrize("n", [1, 2, 17, 255, 257])
def test_step_is_the_specification_bit_for_bit(torch_mod, ctx, n, C):
    _check_steps(torch_mod, ctx, n, C)


@pytest.mark.parametrize("n,C", [(17, 64), (257, 4), (255, 130), (17, 260)], ids=["17-64-off", "257-4-off", "255-130-off", "17-260-aligned"])
def test_step_off_alignment_and_past_a_group_of_wide_lanes(torch_mod, ctx, n, C):
    """F from an element offset that breaks the 16-byte alignment (the one-class-per-lane path at a C the wide path would take), and
    C = 260: 65 units of four classes, one more than the 64 lanes of a row."""
    _check_steps(torch_mod, ctx, n, C, off=C != 260)


def test_delta_is_left_alone_without_a_pointer(torch_mod, ctx):
    csr = _matrix(257)
    F, lab = cases.step_labels(257, 64, 3)
    got, deltas = _device_steps(torch_mod, ctx, csr, F, lab, 0.2, 2, want_delta=False)
    want, _ = _reference_steps(csr, F, lab, 0.2, 2)
    assert deltas == [-5.0, -5.0] and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_step_refusals(torch_mod, ctx):
    from birdnet_stm32 import _hip

    torch = torch_mod
    n, C = 17, 4
    rowptr, col, val = (torch.from_numpy(a).cuda() for a in _matrix(n))
    f, g = torch.zeros((n, C), device="cuda"), torch.full((n, C), 7.0, device="cuda")
    lab = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    delta = torch.zeros(2, dtype=torch.float64, device="cuda")
    ok = dict(rowptr=rowptr.data_ptr(), col=col.data_ptr(), val=val.data_ptr(), f=f.data_ptr(), lab=lab.data_ptr(), n=n, C=C, alpha=0.2, out=g.data_ptr(), delta=delta.data_ptr())

    def call(**kw):
        a = {**ok, **kw}
        return ctx.lib.bn_propagate_step(ctx.handle, a["rowptr"], a["col"], a["val"], a["f"], a["lab"], a["n"], a["C"], _hip.c_float(a["alpha"]), a["out"], a["delta"], None)

    for kw in (dict(rowptr=None), dict(col=None), dict(val=None), dict(f=None), dict(lab=None), dict(out=None), dict(n=0), dict(n=(1 << 21) + 1), dict(C=0),
               dict(C=4097), dict(alpha=0.0), dict(alpha=1.0), dict(alpha=float("nan")), dict(rowptr=ok["rowptr"] + 4), dict(col=ok["col"] + 2), dict(val=ok["val"] + 1),
               dict(f=ok["f"] + 2), dict(out=ok["out"] + 2), dict(lab=ok["lab"] + 1), dict(delta=ok["delta"] + 4), dict(out=ok["f"]), dict(out=ok["f"] + 16),
               dict(f=ok["out"] + 4 * (n * C - 1))):
        assert call(**kw) == -1, kw   # BN_ERR_ARG
    torch.cuda.synchronize()
    assert bool((g == 7.0).all()) and not bool(delta.any()), "a refused call writes nothing"
    assert call() == 0 and call(delta=None) == 0
    for kw in (dict(f=None), dict(label=None), dict(score=None), dict(n=0), dict(C=0), dict(C=4097), dict(f=ok["f"] + 2)):
        a = {**dict(f=ok["f"], n=n, C=C, label=lab.data_ptr(), score=g.data_ptr()), **kw}
        assert ctx.lib.bn_propagate_decide(ctx.handle, a["f"], a["n"], a["C"], a["label"], a["score"], None) == -1, kw


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 63, 64, 65, 130])
def test_decide_label_exact_and_score_within_the_sum_bound(torch_mod, ctx, C):
    from birdnet_stm32 import _hip

    torch = torch_mod
    for n in (1, 17, 257):
        F, _ = cases.step_labels(n, C, 5 * n + C)
        if n >= 17:
            F[2] = 0.0                                   # no label reaches the row
            F[3] = np.float32(0.375)                     # every class ties: the first wins
            F[4, C - 1] = F[4].max()                     # the last class ties with an earlier one
            F[5] = 0.0
            F[5, C - 1] = np.float32(1e-30)              # the only class is the last
        want_label, _ = P.decide_reference(F)
        d_f = torch.from_numpy(F).cuda()
        label = torch.full((n + 2,), FILL_LABEL, dtype=torch.int32, device="cuda")
        score = torch.full((n + 2,), NAN_BITS, dtype=torch.int32, device="cuda")
        _hip.check(ctx.lib.bn_propagate_decide(ctx.handle, d_f.data_ptr(), n, C, label[1:].data_ptr(), score[1:].data_ptr(), None))
        torch.cuda.synchronize()
        lab, sc = label.cpu().numpy(), score.cpu().numpy()
        assert lab[0] == lab[n + 1] == FILL_LABEL and sc[0] == sc[n + 1] == NAN_BITS, "a guard row was written"
        assert np.array_equal(d_f.cpu().numpy(), F), "an input changed"
        lab, sc = lab[1:n + 1], sc[1:n + 1].view(np.float32).astype(np.float64)
        assert np.array_equal(lab, want_label), f"n {n}"
        exact = np.where(want_label < 0, 0.0, F[np.arange(n), np.maximum(want_label, 0)].astype(np.float64) / np.maximum(F.astype(np.float64).sum(axis=1), 1e-300))
        assert np.all(np.abs(sc - exact) <= (C + 2) * U * exact), f"n {n}: {np.abs(sc - exact).max()}"
        assert np.all(sc[want_label < 0] == 0)


# ------------------------------------------------------------------------------------------------------------------- end to end
def _index(rows, **kw):
    from birdnet_stm32.evaluation.search import EmbeddingIndex

    n = rows.shape[0]
    return EmbeddingIndex(rows, np.arange(n) // 60, (np.arange(n) % 60) * 3.0, [f"rec_{i}.wav" for i in range(-(-n // 60))], **kw)


RUN = dict(neighbours=cases.K, tau=cases.TAU, alpha=cases.ALPHA)


def _teacher_forced(rows, seed_label, got, zero_point=0, **kw):
    """The reference over the device's neighbours, with the precondition for n_iter checked before the device's result is compared."""
    want = P.propagate_reference(rows, seed_label, cases.C, **RUN, zero_point=zero_point, graph=(got.neighbour_idx, got.neighbour_score), **kw)
    tol = kw.get("tol", P.DEFAULT_TOL)
    assert all(abs(d - tol) > 1e-6 * tol for d in want.delta_history), "a delta too close to tol for n_iter to be decided"
    return want


def _same_bits(got, want):
    assert got.n_iter == want.n_iter and np.array_equal(got.labels, want.labels)
    assert np.array_equal(got.F.view(np.uint32), want.F.view(np.uint32)), "F differs"
    assert np.array_equal(np.isnan(got.scores), np.isnan(want.scores))
    live = ~np.isnan(want.scores)
    assert np.all(np.abs(got.scores[live].astype(np.float64) - want.scores[live]) <= (cases.C + 3) * U * want.scores[live])
    assert len(got.delta_history) == len(want.delta_history)
    n_c = got.nonzero.size * cases.C
    assert all(abs(a - b) <= n_c * 2.0 ** -52 * b for a, b in zip(got.delta_history, want.delta_history))


@pytest.fixture(scope="module")
def planted_run(torch_mod, ctx):
    X, _, seed = cases.planted()
    index = _index(np.array(X))
    got = P.propagate_index(index, seed, cases.C, **RUN, ctx=ctx, keep_scores=True)
    return got


def test_propagate_index_teacher_forced_is_bit_equal(planted_run):
    X, _, seed = cases.planted()
    want = _teacher_forced(X, seed, planted_run)
    _same_bits(planted_run, want)
    assert planted_run.n_iter == 5 and planted_run.holdout is None and planted_run.neighbour_idx.shape == (cases.N, cases.K)


def test_propagate_index_against_the_independent_reference(planted_run):
    X, _, seed = cases.planted()
    want = P.propagate_reference(X, seed, cases.C, **RUN, float64=True)
    top = np.sort(P.normalized_rows(want.extra["F64"]), axis=1)
    clear = top[:, -1] - top[:, -2] > 1e-3
    print(f"rows the float64 reference separates by more than 1e-3: {int(clear.sum())} of {cases.N}, smallest margin {float((top[:, -1] - top[:, -2]).min()):.3g}")
    assert clear.sum() >= 0.99 * cases.N
    assert np.array_equal(planted_run.labels[clear], want.extra["labels64"][clear])
    assert np.array_equal(planted_run.labels[clear], want.labels[clear])


def test_tol_zero_runs_every_update_and_no_scores_kept(torch_mod, ctx):
    X, _, seed = cases.planted()
    got = P.propagate_index(_index(np.array(X)), seed, cases.C, **RUN, max_iter=9, tol=0.0, ctx=ctx)
    assert got.n_iter == 9 and len(got.delta_history) == 10 and got.F is None
    want = P.propagate_reference(X, seed, cases.C, **RUN, max_iter=9, tol=0.0, graph=(got.neighbour_idx, got.neighbour_score))
    assert np.array_equal(got.labels, want.labels)


def test_int8_archive_with_a_zero_point(torch_mod, ctx):
    X, _, seed = cases.planted()
    q = cases.quantised(X, 5)
    got = P.propagate_index(_index(q, dtype="int8", scale=0.01, zero_point=5), seed, cases.C, **RUN, ctx=ctx, keep_scores=True)
    _same_bits(got, _teacher_forced(q, seed, got, zero_point=5))
    independent = P.propagate_reference(q, seed, cases.C, **RUN, zero_point=5)
    assert np.array_equal(got.neighbour_idx, independent.neighbour_idx), "int8 scores are exact: the neighbours are the reference's own"


def test_archive_with_zero_rows(torch_mod, ctx):
    X, _, seed = cases.planted()
    rows = np.array(X)
    dead = [0, 100, 239]
    rows[dead] = 0.0
    lab = seed.copy()
    lab[100] = 2   # (a labelled zero row is ignored)
    got = P.propagate_index(_index(rows), lab, cases.C, **RUN, ctx=ctx, keep_scores=True)
    assert got.nonzero.size == cases.N - 3 and np.all(got.labels[dead] == -1) and np.isnan(got.scores[dead]).all() and np.isnan(got.F[dead]).all()
    _same_bits(got, _teacher_forced(rows, lab, got))


def test_holdout_report_is_the_references(torch_mod, ctx, planted_run):
    X, _, seed = cases.planted()
    got = P.propagate_index(_index(np.array(X)), seed, cases.C, **RUN, holdout=0.25, seed=3, ctx=ctx, keep_scores=True)
    want = _teacher_forced(X, seed, got, holdout=0.25, seed=3)
    _same_bits(got, want)
    assert np.array_equal(got.labels, planted_run.labels), "what is returned uses every seed"
    g, w = got.holdout, want.holdout
    assert g.rows.size == 5 and np.array_equal(g.rows, w.rows) and np.array_equal(g.true, w.true) and np.array_equal(g.predicted, w.predicted)
    assert g.accuracy == w.accuracy and np.array_equal(g.recall, w.recall, equal_nan=True)


def _read(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_cli_end_to_end_and_both_ways_to_give_labels(torch_mod, tmp_path, capsys):
    import birdnet_stm32.cli.propagate as cli

    X, true, _ = cases.planted()
    db, lab, out_a, out_b, labels_csv = (str(tmp_path / name) for name in ("db.npz", "lab.npz", "a.csv", "b.csv", "labels.csv"))
    with open(db, "wb") as f:
        np.savez(f, embeddings=X[:200], file_index=np.arange(200) // 50, start_s=(np.arange(200) % 50) * 3.0, paths=np.asarray([f"field/rec_{i}.wav" for i in range(4)]))
    lab_paths = [f"train/c{true[200 + i]}/clip_{i}.wav" for i in range(40)]
    with open(lab, "wb") as f:
        np.savez(f, embeddings=X[200:], file_index=np.arange(40), start_s=np.zeros(40), paths=np.asarray(lab_paths))
    res = cli.main(["--database", db, "--labelled", lab, "--output", out_a, "--neighbours", "7", "--holdout", "0.25", "--scores_out", str(tmp_path / "f.npz")])
    said = capsys.readouterr().out
    names = sorted({f"c{c}" for c in true[200:]})
    assert "Spread 40 labels" in said and "hold-out accuracy" in said and res.holdout.rows.size == 10
    assert (tmp_path / "a_labels.txt").read_text().split() == names
    rows = _read(out_a)
    assert tuple(rows[0]) == cli.CSV_COLUMNS and len(rows) == 241
    assert [r[0] for r in rows[1:]] == [str(i) for i in range(240)]
    assert [r[1] for r in rows[1:201]] == [f"field/rec_{i // 50}.wav" for i in range(200)] and [r[1] for r in rows[201:]] == lab_paths
    assert [r[2] for r in rows[1:201]] == [f"{(i % 50) * 3.0:.3f}" for i in range(200)]
    assert [r[5] for r in rows[1:]] == ["0"] * 200 + ["1"] * 40
    assert [r[3] for r in rows[1:]] == [names[c] for c in res.labels] and all(0 < float(r[4]) <= 1 for r in rows[1:])
    assert np.mean([r[3] == f"c{c}" for r, c in zip(rows[1:201], true[:200])]) > 0.5, "the unlabelled rows come back far above chance (1 / 5)"
    summary = _read(str(tmp_path / "a_summary.csv"))
    assert tuple(summary[0]) == cli.SUMMARY_COLUMNS and [r[0] for r in summary[1:]] == names
    assert sum(int(r[1]) for r in summary[1:]) == 40 and sum(int(r[2]) for r in summary[1:]) == 240
    with np.load(str(tmp_path / "f.npz")) as z:
        assert z["F"].shape == (240, len(names)) and [str(s) for s in z["labels"]] == names and np.array_equal(z["F"].argmax(axis=1), res.labels)
    with open(labels_csv, "w") as f:
        f.write("path,label\n" + "".join(f"{p},c{true[200 + i]}\n" for i, p in enumerate(lab_paths)))
    cli.main(["--database", db, lab, "--labels", labels_csv, "--output", out_b, "--neighbours", "7", "--holdout", "0.25"])
    assert open(out_a, "rb").read() == open(out_b, "rb").read()
    assert open(str(tmp_path / "a_summary.csv"), "rb").read() == open(str(tmp_path / "b_summary.csv"), "rb").read()
    strict = str(tmp_path / "s.csv")
    cli.main(["--database", db, lab, "--labels", labels_csv, "--output", strict, "--neighbours", "7", "--min_score", "0.9"])
    for plain, cut in zip(rows[1:], _read(strict)[1:]):
        assert cut[3] == (plain[3] if np.float32(plain[4]) >= 0.9 else "") and cut[4:] == plain[4:], "only the label column changes"
