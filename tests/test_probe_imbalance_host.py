"""Host-side tests of the probe's tools for long-tailed training sets (no GPU): the focal loss and its gradient, row weights and
``rows`` in the numpy restatement, balanced class weights, minority upsampling, what they do to a long-tailed problem, and the refusals."""

import os

import numpy as np
import pytest

from birdnet_stm32.data.dataset import upsample_minority_classes
from birdnet_stm32.training import linear_probe as lp

GAMMAS = (0.0, 0.5, 1.0, 2.0, 5.0)


# -- the gradient ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("gamma", GAMMAS)
def test_focal_gradient_against_central_differences(gamma, smoothing, weighted):
    """probe_loss_gradient against central differences (h = 1e-5) of the float64 probe_loss through head_scores: with X the identity and
    b = 0 the logits are W itself, so every logit is perturbed on its own.  The largest error is at most 1e-5 of the largest |G|."""
    rng = np.random.default_rng(17)
    N, C, h = 9, 6, 1e-5
    Z = 2.5 * rng.standard_normal((N, C))
    Y = (rng.random((N, C)) < 0.3).astype(np.float64)
    Y[2] = 0.0
    if smoothing:
        Y = lp.smooth_targets(Y, smoothing, "sigmoid")
    w = rng.uniform(0.2, 6.0, N) if weighted else None
    kw = dict(loss="focal", focal_gamma=gamma, sample_weight=w)
    X, b = np.eye(N), np.zeros(C)
    G = lp.probe_loss_gradient(lp.head_scores(X, Z, b, "sigmoid"), Y, "sigmoid", **kw)
    num = np.empty_like(Z)
    for i in range(N):
        for c in range(C):
            up, dn = Z.copy(), Z.copy()
            up[i, c] += h
            dn[i, c] -= h
            num[i, c] = (lp.probe_loss(lp.head_scores(X, up, b, "sigmoid"), Y, "sigmoid", **kw)
                         - lp.probe_loss(lp.head_scores(X, dn, b, "sigmoid"), Y, "sigmoid", **kw)) / (2 * h)
    err = np.abs(G - num).max() / np.abs(G).max()
    print(f"gamma={gamma} smoothing={smoothing} weighted={weighted}: max err / max |G| = {err:.2e}")
    assert G.shape == Z.shape and err <= 1e-5


@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
def test_cross_entropy_gradient_with_weights_against_central_differences(activation):
    rng = np.random.default_rng(3)
    N, C, h = 7, 5, 1e-5
    Z = 2.0 * rng.standard_normal((N, C))
    Y = np.eye(C)[rng.integers(0, C, N)]
    w = rng.uniform(0.2, 6.0, N)
    X, b = np.eye(N), np.zeros(C)
    G = lp.probe_loss_gradient(lp.head_scores(X, Z, b, activation), Y, activation, sample_weight=w)
    num = np.empty_like(Z)
    for i in range(N):
        for c in range(C):
            up, dn = Z.copy(), Z.copy()
            up[i, c] += h
            dn[i, c] -= h
            num[i, c] = (lp.probe_loss(lp.head_scores(X, up, b, activation), Y, activation, sample_weight=w)
                         - lp.probe_loss(lp.head_scores(X, dn, b, activation), Y, activation, sample_weight=w)) / (2 * h)
    assert np.abs(G - num).max() <= 1e-5 * np.abs(G).max()
    # the defaults keep probe_loss's value and the plain (p - y) / scale
    P = lp.head_scores(X, Z, b, activation)
    assert lp.probe_loss(P, Y, activation) == lp.probe_loss(P, Y, activation, loss="auto", focal_gamma=3.0, sample_weight=None)
    assert np.array_equal(lp.probe_loss_gradient(P, Y, activation), (P - Y) / (N if activation == "softmax" else N * C))


# -- bit equalities of the float32 restatement --------------------------------------------------------------------------------------------
def _clusters(n, D, C, seed, noise_rows=True):
    cent = np.random.default_rng(77).standard_normal((C, D))
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, C, n)
    X = np.maximum(cent[lab] + 1.5 * rng.standard_normal((n, D)), 0).astype(np.float32)
    Y = np.eye(C, dtype=np.float32)[lab]
    if noise_rows:
        Y[::9] = 0.0
    return X, Y, lab


FIT = dict(epochs=2, batch_size=32, learning_rate=1e-2, dropout=0.5, clipnorm=1.0, seed=6, dtype=np.float32)


@pytest.fixture(scope="module")
def small():
    X, Y, _ = _clusters(203, 24, 5, 1)
    Xv, Yv, _ = _clusters(60, 24, 5, 2)
    return X, Y, Xv, Yv, lp.fit_probe_reference(X, Y, Xv, Yv, **FIT)


def _same_bits(a, b):
    return (np.array_equal(a.history["W"], b.history["W"]) and np.array_equal(a.history["b"], b.history["b"])
            and np.array_equal(a.history["step_loss"], b.history["step_loss"]) and a.history["val_loss"] == b.history["val_loss"])


@pytest.mark.parametrize("label_smoothing", [0.0, 0.1])
def test_focal_gamma_zero_has_the_bits_of_cross_entropy(small, label_smoothing):
    X, Y, Xv, Yv, _ = small
    a = lp.fit_probe_reference(X, Y, Xv, Yv, label_smoothing=label_smoothing, **FIT)
    b = lp.fit_probe_reference(X, Y, Xv, Yv, label_smoothing=label_smoothing, loss="focal", focal_gamma=0.0, **FIT)
    assert _same_bits(a, b)
    c = lp.fit_probe_reference(X, Y, Xv, Yv, label_smoothing=label_smoothing, loss="focal", focal_gamma=2.0, **FIT)
    assert not np.array_equal(a.history["W"], c.history["W"])


def test_unit_weights_and_identity_rows_have_the_bits_of_none(small):
    X, Y, Xv, Yv, plain = small
    assert _same_bits(plain, lp.fit_probe_reference(X, Y, Xv, Yv, sample_weight=np.ones(len(X)), **FIT))
    assert _same_bits(plain, lp.fit_probe_reference(X, Y, Xv, Yv, rows=np.arange(len(X)), **FIT))
    assert _same_bits(plain, lp.fit_probe_reference(X, Y, Xv, Yv, loss="auto", focal_gamma=2.0, sample_weight=None, rows=None, **FIT))


@pytest.mark.parametrize("loss", ["auto", "focal"])
def test_rows_with_repeats_have_the_bits_of_a_fit_on_the_gathered_rows(small, loss):
    X, Y, Xv, Yv, _ = small
    rng = np.random.default_rng(8)
    rows = np.sort(np.concatenate([np.arange(len(X)), rng.integers(0, 40, 117)])).astype(np.int64)   # 320 entries: ten full batches
    rows = rows[:-3]                                                                                  # ... and then a short last one
    w = rng.uniform(0.5, 4.0, len(X)).astype(np.float32)
    a = lp.fit_probe_reference(X, Y, Xv, Yv, loss=loss, sample_weight=w, rows=rows, **FIT)
    b = lp.fit_probe_reference(X[rows], Y[rows], Xv, Yv, loss=loss, sample_weight=w[rows], **FIT)
    assert _same_bits(a, b)
    assert a.history["step_loss"].shape == (2 * 10,) and len(rows) == 317
    assert not np.array_equal(a.history["W"], lp.fit_probe_reference(X, Y, Xv, Yv, loss=loss, sample_weight=w, **FIT).history["W"])


def test_sweep_reference_passes_the_arguments_on(small):
    X, Y, Xv, Yv, _ = small
    rows, w = np.arange(len(X))[::-1].copy(), np.linspace(0.5, 2.0, len(X))
    trials = [lp.ProbeTrial(learning_rate=1e-2), lp.ProbeTrial(learning_rate=3e-3, label_smoothing=0.1)]
    kw = dict(epochs=2, batch_size=32, seed=6, dtype=np.float32, loss="focal", focal_gamma=1.0, sample_weight=w, rows=rows)
    res = lp.fit_probe_sweep_reference(X, Y, Xv, Yv, trials, **kw)
    for t, head in zip(trials, res.heads):
        assert _same_bits(head, lp.fit_probe_reference(X, Y, Xv, Yv, **kw, **t.fit_kwargs()))


def test_validation_loss_is_focal_unweighted_and_unsmoothed(small):
    X, Y, Xv, Yv, _ = small
    head = lp.fit_probe_reference(X, Y, Xv, Yv, loss="focal", focal_gamma=2.0, label_smoothing=0.1, sample_weight=np.full(len(X), 3.0), **FIT)
    P = lp.head_scores(Xv.astype(np.float32), head.history["W"], head.history["b"], "sigmoid")
    assert head.history["val_loss"][-1] == float(lp.probe_loss(P, Yv, "sigmoid", loss="focal", focal_gamma=2.0))
    assert head.history["val_loss"][-1] != float(lp.probe_loss(P, Yv, "sigmoid"))


# -- helper values ------------------------------------------------------------------------------------------------------------------------
def test_balanced_class_weights_on_hand_counted_lists():
    paths = [f"/d/a/{i}.wav" for i in range(6)] + [f"/d/b/{i}.wav" for i in range(3)] + ["/d/c/0.wav"] + [f"/d/noise/{i}.wav" for i in range(5)]
    w = lp.balanced_class_weights(paths, ["a", "b", "c"])
    assert w.dtype == np.float64 and np.allclose(w, [10 / (3 * 6), 10 / (3 * 3), 10 / (3 * 1)], rtol=0, atol=1e-15)
    # a class with no file counts as 1 (the reference's label_counts.get(i, 1)); the noise files are no part of the total
    w = lp.balanced_class_weights(paths, ["a", "b", "c", "d"])
    assert np.allclose(w, [10 / 24, 10 / 12, 10 / 4, 10 / 4], rtol=0, atol=1e-15)
    assert np.allclose(lp.balanced_class_weights(paths[:9] * 2, ["a", "b"]), [18 / (2 * 12), 18 / (2 * 6)], rtol=0, atol=1e-15)


def test_row_weights_one_hot_all_zero_and_multi_hot():
    cw = np.array([0.5, 2.0, 7.0])
    Y = np.array([[1, 0, 0], [0, 0, 1], [0, 0, 0], [0, 1, 1], [1, 1, 0], [0, 1, 0]], np.float32)
    w = lp.row_weights(Y, cw)
    assert w.dtype == np.float32 and w.tolist() == [0.5, 7.0, 1.0, 2.0, 0.5, 2.0]   # all-zero -> 1.0, multi-hot -> the first maximum
    assert lp.row_weights(np.array([[0.2, 0.9, 0.9]]), cw).tolist() == [2.0]


def test_upsample_rows():
    file_index = np.array([0, 0, 1, 2, 2, 2, 3])
    rows = lp.upsample_rows(file_index, np.array([1, 3, 2, 1]))
    assert rows.dtype == np.int32 and rows.tolist() == [0, 1, 2, 2, 2, 3, 3, 4, 4, 5, 5, 6]
    assert lp.upsample_rows(file_index, np.ones(4, int)).tolist() == list(range(7))
    assert lp.upsample_rows(np.zeros(0, int), np.ones(4, int)).shape == (0,)


# -- upsampling ---------------------------------------------------------------------------------------------------------------------------
def _folders(sizes):
    return [f"/data/{c}/{i:03d}.wav" for c, n in sizes.items() for i in range(n)]


def _upsample_restated(paths, classes, ratio):
    """The rule with the same sequence of np.random calls: one choice per short class in class order, one shuffle of all."""
    by = {c: [p for p in paths if os.path.basename(os.path.dirname(p)) == c] for c in classes}
    target = int(max(len(v) for v in by.values()) * ratio)
    out = []
    for c in classes:
        extra = list(np.random.choice(by[c], size=target - len(by[c]), replace=True)) if len(by[c]) < target else []
        out += by[c] + extra
    np.random.shuffle(out)
    return out


def test_upsample_minority_classes_draws_as_the_restatement():
    sizes = {"big": 40, "mid": 21, "small": 5, "tiny": 2, "noise": 7}
    classes = ["big", "mid", "small", "tiny"]
    paths = _folders(sizes)
    np.random.seed(5)
    np.random.shuffle(paths)
    np.random.seed(5)
    got = upsample_minority_classes(paths, classes, 0.5)
    after = np.random.random()
    np.random.seed(5)
    want = _upsample_restated(paths, classes, 0.5)
    assert got == want and after == np.random.random()    # the same list from the same draws, and the generator left where the rule leaves it
    count = {c: sum(os.path.basename(os.path.dirname(p)) == c for p in got) for c in sizes}
    assert count == {"big": 40, "mid": 21, "small": 20, "tiny": 20, "noise": 0}   # mid is over the target: untouched; noise files are dropped
    assert sorted(p for p in got if "/mid/" in p) == sorted(p for p in paths if "/mid/" in p)
    assert set(got) == {p for p in paths if "/noise/" not in p}   # every original file is still there


def test_upsample_ratio_one_brings_every_class_to_the_largest():
    paths = _folders({"a": 13, "b": 4, "c": 1})
    np.random.seed(2)
    got = upsample_minority_classes(paths, ["a", "b", "c"], 1.0)
    assert [sum(f"/{c}/" in p for p in got) for c in "abc"] == [13, 13, 13]
    got = upsample_minority_classes(paths, ["a", "b", "c"], 0.31)   # target int(4.03) = 4: b is at it and untouched, c gets three more
    assert [sum(f"/{c}/" in p for p in got) for c in "abc"] == [13, 4, 4] and sorted(p for p in got if "/b/" in p) == paths[13:17]
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ratio"):
            upsample_minority_classes(paths, ["a", "b", "c"], bad)


def test_the_commands_path_keeps_noise_files_once():
    sizes = {"big": 12, "small": 3, "noise": 4}
    paths = _folders(sizes)
    np.random.seed(11)
    np.random.shuffle(paths)
    np.random.seed(11)
    mult, upsampled = lp.upsample_multiplicity(paths, ["big", "small"], 0.5)
    assert mult.shape == (len(paths),) and mult.dtype == np.int64
    by = lambda c: mult[[i for i, p in enumerate(paths) if f"/{c}/" in p]]   # noqa: E731
    assert by("noise").tolist() == [1] * 4 and by("big").tolist() == [1] * 12 and by("small").sum() == 6 and by("small").min() >= 1
    assert len(upsampled) == 18 and not any("/noise/" in p for p in upsampled)
    # the balanced weights are counted after upsampling (the reference's order)
    assert np.allclose(lp.balanced_class_weights(upsampled, ["big", "small"]), [18 / (2 * 12), 18 / (2 * 6)])
    # two rows per file: the rows of a file repeated together, in ascending order
    file_index = np.repeat(np.arange(len(paths)), 2)
    rows = lp.upsample_rows(file_index, mult)
    assert len(rows) == 2 * mult.sum() and np.all(np.diff(rows) >= 0) and np.array_equal(np.bincount(rows), np.repeat(mult, 2))


# -- what they do to a long-tailed problem --------------------------------------------------------------------------------------------
COUNTS = (600, 30, 20, 12, 8)


def _long_tailed(seed, D=64):
    C = len(COUNTS)
    centres = np.random.default_rng(1000 + D + C).standard_normal((C, D)) * 0.7
    rng = np.random.default_rng(seed)
    lab = rng.permutation(np.repeat(np.arange(C), COUNTS))
    X = np.maximum(centres[lab] + 1.5 * rng.standard_normal((len(lab), D)), 0)
    lab_v = np.repeat(np.arange(C), 150)
    Xv = np.maximum(centres[lab_v] + 1.5 * rng.standard_normal((len(lab_v), D)), 0)
    return X, np.eye(C)[lab], lab, Xv, lab_v


def _minority_recall(head, Xv, lab_v):
    P = lp.head_scores(Xv, head.history["W"], head.history["b"], "sigmoid")
    return float(np.mean([(P[lab_v == c, c] >= 0.5).mean() for c in range(1, len(COUNTS))]))


@pytest.mark.parametrize("seed", [3, 7])
def test_minority_recall_on_a_long_tailed_problem(seed):
    """600/30/20/12/8 training rows, 150 validation rows per class, the float64 restatement: 12 epochs of batch 32, Adam at 1e-2, dropout
    0.2, clip 1.  The mean recall at 0.5 of the four minority classes must beat the plain fit's by 0.15 with balanced weights and with
    upsampling to half the largest class, and by 0.05 with the focal loss at gamma = 2 (DESIGN.md 5d has the measured values)."""
    X, Y, lab, Xv, lab_v = _long_tailed(seed)
    kw = dict(epochs=12, batch_size=32, learning_rate=1e-2, dropout=0.2, clipnorm=1.0, seed=seed, dtype=np.float64)
    plain = _minority_recall(lp.fit_probe_reference(X, Y, **kw), Xv, lab_v)
    cw = len(lab) / (len(COUNTS) * np.asarray(COUNTS, np.float64))   # balanced_class_weights of one file per row
    weighted = _minority_recall(lp.fit_probe_reference(X, Y, sample_weight=lp.row_weights(Y, cw), **kw), Xv, lab_v)
    rng = np.random.default_rng(seed + 100)
    target = int(max(COUNTS) * 0.5)
    extra = [rng.choice(np.flatnonzero(lab == c), target - COUNTS[c]) for c in range(1, len(COUNTS))]
    rows = np.sort(np.concatenate([np.arange(len(lab))] + extra))
    upsampled = _minority_recall(lp.fit_probe_reference(X, Y, rows=rows, **kw), Xv, lab_v)
    focal = _minority_recall(lp.fit_probe_reference(X, Y, loss="focal", focal_gamma=2.0, **kw), Xv, lab_v)
    print(f"seed {seed}: minority recall plain {plain:.3f}, balanced weights {weighted:.3f} ({weighted - plain:+.3f}), "
          f"upsampled {upsampled:.3f} ({upsampled - plain:+.3f}), focal {focal:.3f} ({focal - plain:+.3f})")
    assert len(rows) == 600 + 4 * 300
    assert weighted - plain >= 0.15
    assert upsampled - plain >= 0.15
    assert focal - plain >= 0.05


# -- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_fit_arguments():
    X, Y, _ = _clusters(40, 8, 3, 1)
    fits = [lambda **kw: lp.fit_probe_reference(X, Y, epochs=1, **kw),
            lambda **kw: lp.fit_probe(None, X, Y, epochs=1, **kw),                       # refused before anything is uploaded: no context needed
            lambda **kw: lp.fit_probe_sweep(None, X, Y, None, None, [lp.ProbeTrial()], epochs=1, **kw),
            lambda **kw: lp.fit_probe_sweep_reference(X, Y, None, None, [lp.ProbeTrial()], epochs=1, **kw)]
    for fit in fits:
        with pytest.raises(ValueError, match="softmax"):
            fit(loss="focal", activation="softmax")
        with pytest.raises(ValueError, match="loss must be"):
            fit(loss="hinge")
        for gamma in (-0.1, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="focal_gamma"):
                fit(loss="focal", focal_gamma=gamma)
        for w in (np.ones(39), np.ones((40, 1)), np.full(40, np.nan), -np.ones(40)):
            with pytest.raises(ValueError, match="sample_weight"):
                fit(sample_weight=w)
        for rows in (np.array([0, 40]), np.array([-1, 2]), np.zeros((2, 2), int), np.zeros(0, int), np.array([0.5, 1.0])):
            with pytest.raises(ValueError, match="rows"):
                fit(rows=rows)
    with pytest.raises(ValueError, match="softmax"):
        lp.probe_loss(np.full((2, 3), 0.3), np.eye(3)[:2], "softmax", loss="focal")
    with pytest.raises(ValueError, match="focal_gamma"):
        lp.probe_loss_gradient(np.full((2, 3), 0.3), np.eye(3)[:2], "sigmoid", loss="focal", focal_gamma=-1.0)


def test_refusals_of_the_command_line(tmp_path):
    """Bad values end the command before the model is looked for (the model path does not exist: a FileNotFoundError would say otherwise)."""
    from birdnet_stm32.cli import probe as probe_cli

    base = ["--model_path", str(tmp_path / "none.tflite"), "--data_path_train", str(tmp_path), "--output", str(tmp_path / "h")]
    for extra, word in [(["--loss", "focal", "--activation", "softmax"], "softmax"), (["--loss", "focal", "--focal_gamma", "-1"], "focal_gamma"),
                        (["--focal_gamma", "nan"], "focal_gamma"), (["--upsample_ratio", "1.5"], "upsample_ratio"),
                        (["--upsample_ratio", "-0.25"], "upsample_ratio"), (["--upsample_ratio", "nan"], "upsample_ratio")]:
        with pytest.raises(SystemExit, match=word):
            probe_cli.main(base + extra)
    with pytest.raises(SystemExit):
        probe_cli.build_parser().parse_args(base + ["--class_weights", "inverse"])
    args = probe_cli.build_parser().parse_args(base)
    assert lp.imbalance_from_args(args) == {"loss": "auto", "focal_gamma": 2.0, "class_weights": "none", "upsample_ratio": 0.0}
    args = probe_cli.build_parser().parse_args(base + ["--loss", "focal", "--focal_gamma", "1.5", "--class_weights", "balanced", "--upsample_ratio", "0.5"])
    assert lp.imbalance_from_args(args) == {"loss": "focal", "focal_gamma": 1.5, "class_weights": "balanced", "upsample_ratio": 0.5}
